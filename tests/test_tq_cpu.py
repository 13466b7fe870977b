"""TQ1_0 / TQ2_0 on the CPU side: the numpy restatement of tests/tq_ref.py on hand-packed blocks with closed-form answers, the trit encoding's bijection, the
reference quantisers, what the synthetic writer's tq1_0 / tq2_0 files contain (and that every older ftype still writes the bytes it wrote), the host-only
load planner on such files, and the reference models against their parents on a file without ternary tensors."""
import hashlib

import numpy as np
import pytest

import oracle_py as oq
import tq_ref as tq
from gguf_read import read_gguf
from qwen3_ref import Qwen3Ref
from qwen3moe_ref import Qwen3MoeRef
from test_model_plan_cpu import ROW, Maker, model_file, plan, plan_exe  # noqa: F401  (plan_exe: the session's host test program)

TYPES = [tq.TQ1_0, tq.TQ2_0]
NAME = {tq.TQ1_0: "tq1_0", tq.TQ2_0: "tq2_0"}


def _q8k_of_codes(a):
    """One Q8_K block with d = 1 holding the int8 codes a[256] (hand-built, so a test's integers are the ones it wrote down)."""
    b = np.zeros(1, tq.DT_Q8K)
    b["d"], b["qs"] = 1.0, np.asarray(a, np.int8)
    b["bsums"] = np.asarray(a, np.int64).reshape(16, 16).sum(axis=1)
    return b.view(np.uint8)


# ------------------------------------------------------------------------------------------------ hand-packed blocks
def test_block_sizes_and_type_ids():
    assert (tq.TQ1_0, tq.TQ2_0) == (34, 35)
    assert tq.row_bytes(tq.TQ1_0, 256) == 54 and tq.row_bytes(tq.TQ2_0, 256) == 66 and tq.row_bytes(tq.TQ1_0, 4096) == 16 * 54


def test_all_plus_one_by_hand():
    """Every weight + 1.  TQ2_0: every field 2, every byte 0b10101010.  TQ1_0: five trits of 2 are 242 -> (242 * 256 + 242) / 243 = 255; four trits of 2
    times 3 are 240 -> (240 * 256 + 242) / 243 = 253."""
    b2 = np.zeros(1, tq.DT[tq.TQ2_0]); b2["qs"], b2["d"] = 0xAA, 0.5
    b1 = np.zeros(1, tq.DT[tq.TQ1_0]); b1["qs"], b1["qh"], b1["d"] = 255, 253, 0.5
    a = np.arange(256) % 100 - 50
    for t, b in ((tq.TQ2_0, b2), (tq.TQ1_0, b1)):
        raw = b.view(np.uint8)
        assert (tq.dequantize(t, raw, 256) == np.float32(0.5)).all()
        assert tq.pack(t, np.full((1, 256), 2), [0.5]).tobytes() == raw.tobytes()
        assert tq.vec_dot_int_partials(t, raw, _q8k_of_codes(a), 256).tolist() == [int(a.sum())]
        assert tq.vec_dot(t, raw, _q8k_of_codes(a), 256) == np.float32(a.sum()) * np.float32(0.5)


# one - 1 in an otherwise all-zero-weight block: (element, byte, hand-computed byte value).  An all-ones byte is 1 + 3 + 9 + 27 + 81 = 121 -> (121 * 256 + 242) /
# 243 = 128; four ones times 3: 120 -> 127.  Trit position n has weight 3^(4 - n): clearing it to 0 takes that off before the byte is scaled.
TQ1_MINUS = [
    (32 * 2 + 5, 5, ((121 - 9) * 256 + 242) // 243),            # region 1: element 69 = trit 2 of qs[5]
    (160 + 16 * 4 + 3, 32 + 3, ((121 - 1) * 256 + 242) // 243),  # region 2: element 227 = trit 4 of qs[35]
    (240 + 4 * 1 + 2, 48 + 2, ((120 - 27) * 256 + 242) // 243),  # region 3: element 246 = trit 1 of qh[2]
]


@pytest.mark.parametrize("elem,byte,value", TQ1_MINUS)
def test_tq1_one_minus_one_in_each_region(elem, byte, value):
    b = np.zeros(1, tq.DT[tq.TQ1_0]); b["qs"], b["qh"], b["d"] = 128, 127, 2.0
    if byte < 48:
        b["qs"][0, byte] = value
    else:
        b["qh"][0, byte - 48] = value
    y = tq.dequantize(tq.TQ1_0, b.view(np.uint8), 256)
    want = np.zeros(256, np.float32); want[elem] = -2.0
    assert (y == want).all(), np.flatnonzero(y != want)
    a = np.arange(256) - 128
    assert tq.vec_dot_int_partials(tq.TQ1_0, b.view(np.uint8), _q8k_of_codes(a), 256).tolist() == [-int(a[elem])]


def test_tq2_one_minus_one():
    """Element 128 h + 32 l + m = bits 2 l of qs[32 h + m]: element 128 + 64 + 7 is field 2 of qs[39]; all other fields 1 (0b01010101)."""
    b = np.zeros(1, tq.DT[tq.TQ2_0]); b["qs"], b["d"] = 0x55, 2.0
    b["qs"][0, 39] = 0x55 & ~(3 << 4)
    want = np.zeros(256, np.float32); want[199] = -2.0
    assert (tq.dequantize(tq.TQ2_0, b.view(np.uint8), 256) == want).all()


@pytest.mark.parametrize("t", TYPES)
def test_position_pattern(t):
    """A block whose element i carries code (i + i // 3 + i // 32 + i // 160) % 3 - no period the layouts share - packed by hand from the element map in the
    module docstring, so a slip of index order in any region moves a code: decode gives the pattern back, and the dot against a = i - 128 is the closed form."""
    i = np.arange(256)
    codes = (i + i // 3 + i // 32 + i // 160) % 3
    b = np.zeros(1, tq.DT[t]); b["d"] = 1.0
    if t == tq.TQ2_0:
        for h in range(2):
            for m in range(32):
                b["qs"][0, 32 * h + m] = sum(int(codes[128 * h + 32 * l + m]) << (2 * l) for l in range(4))
    else:
        def enc(tr):                                                       # most significant first; four trits: one more * 3
            q = 0
            for x in tr:
                q = q * 3 + int(x)
            if len(tr) == 4:
                q *= 3
            return (q * 256 + 242) // 243
        for m in range(32):
            b["qs"][0, m] = enc([codes[32 * n + m] for n in range(5)])
        for m in range(16):
            b["qs"][0, 32 + m] = enc([codes[160 + 16 * n + m] for n in range(5)])
        for j in range(4):
            b["qh"][0, j] = enc([codes[240 + 4 * n + j] for n in range(4)])
    raw = b.view(np.uint8)
    d, q = tq.decode(t, raw, 256)
    assert (q[0] == codes).all(), np.flatnonzero(q[0] != codes)
    assert tq.pack(t, codes[None, :], [1.0]).tobytes() == raw.tobytes()
    a = i - 128
    assert tq.vec_dot_int_partials(t, raw, _q8k_of_codes(a), 256).tolist() == [int(((codes - 1) * a).sum())]


def test_trit_encoding_is_a_bijection_and_every_byte_decodes():
    """All 243 five-trit and all 81 four-trit values survive encode -> decode; every one of the 256 byte values decodes to trits in 0..2."""
    for nt, count in ((5, 243), (4, 81)):
        seen = set()
        for v in range(count):
            tr = [(v // 3 ** (nt - 1 - k)) % 3 for k in range(nt)]
            q = v * 3 if nt == 4 else v
            byte = (q * 256 + 242) // 243
            assert 0 <= byte <= 255 and [int(tq.trit(byte, k)) for k in range(nt)] == tr, (v, byte)
            seen.add(byte)
        assert len(seen) == count
    allb = np.arange(256)
    for k in range(5):
        assert tq.trit(allb, k).max() <= 2


@pytest.mark.parametrize("t", TYPES)
def test_quantise_dequantise_exact_on_ternary_inputs(pkg, t):
    """x in {-d, 0, d} (d an f16 value) comes back exactly, through the restatement's quantiser and the writer's (the same bytes); an all-zero block gives d = 0."""
    rng = np.random.default_rng(t)
    d = np.float32(np.float16(0.0371))
    x = (rng.integers(-1, 2, 4 * 256).astype(np.float32) * d).astype(np.float32)
    x[:256][0] = d                                                         # every block holds its maximum
    x[256:512] = 0.0
    raw = tq.quantize(t, x)
    assert (tq.dequantize(t, raw, x.size) == x).all()
    assert tq.blocks(t, raw, x.size)["d"][1] == 0
    gs = pkg.gguf_synth
    assert (gs.quantize_tq1_0 if t == tq.TQ1_0 else gs.quantize_tq2_0)(x).tobytes() == raw.tobytes()
    # rounding: lroundf(x / max) with halves away from zero
    y = np.zeros(256, np.float32); y[0], y[1], y[2], y[3], y[4] = 1.0, 0.5, -0.5, 0.49, -0.49
    assert tq.dequantize(t, tq.quantize(t, y), 256)[:5].tolist() == [1.0, 1.0, -1.0, 0.0, 0.0]


@pytest.mark.parametrize("t", TYPES)
def test_negative_d_gives_negative_zero(t):
    raw = tq.pack(t, np.ones((1, 256), int), [-1.5])
    y = tq.dequantize(t, raw, 256)
    assert (y.view(np.uint32) == 0x80000000).all()


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K", [256, 4096])
def test_dot_against_f64_of_dequantised_rows(pkg, t, K):
    gs = pkg.gguf_synth
    rng = np.random.default_rng(K + t)
    N, T = 8, 3
    W = gs.random_blocks(rng, t, N * K, 0.05)
    x = rng.standard_normal((T, K)).astype(np.float32)
    y = tq.mul_mat(t, W, N, K, x)
    Wf = tq.dequantize(t, W, N * K).reshape(N, K).astype(np.float64)
    rb = tq.row_bytes(t, K)
    for tt in range(T):
        aq = tq.quantize_act(x[tt])
        af = oq.dequantize(oq.Q8_K, aq, K).astype(np.float64)
        ref = Wf @ af
        scale = np.abs(Wf).dot(np.abs(af))
        assert np.all(np.abs(y[tt] - ref) <= 2e-6 * scale + 1e-30)
        for n in range(N):
            isum = tq.vec_dot_int_partials(t, W[n * rb:(n + 1) * rb], aq, K)
            assert np.abs(isum).max() <= 256 * 127
        assert tq.vec_dot(t, W[:rb], aq, K) == y[tt, 0]


# ------------------------------------------------------------------------------------------------ the writer
@pytest.mark.parametrize("t", TYPES)
def test_random_blocks_are_well_formed(pkg, t):
    """Uniform trits (never TQ2_0's code 3, only TQ1_0 bytes that five / four trits encode), finite d, the std asked for, and the writer's own unpacking agrees."""
    gs = pkg.gguf_synth
    n = 256 * 2048
    raw = gs.random_blocks(np.random.default_rng(5), t, n, 0.02)
    assert raw.size == tq.row_bytes(t, n)
    d, q = tq.decode(t, raw, n)
    assert np.isfinite(d).all() and (d > 0).all() and q.max() == 2
    assert (gs.unpack_ternary(t, raw) == q).all()
    assert tq.pack(t, q, d).tobytes() == raw.tobytes()                      # valid bytes: re-encoding the trits gives them back
    assert np.abs(np.bincount(q.reshape(-1), minlength=3) / n - 1 / 3).max() < 0.01
    y = tq.dequantize(t, raw, n)
    assert abs(y.std() / 0.02 - 1.0) < 0.06 and abs(y.mean()) < 0.001
    assert gs._UNIT_STD[t] == pytest.approx(np.sqrt(2 / 3))


@pytest.mark.parametrize("ftype,fid,t", [("tq1_0", 36, tq.TQ1_0), ("tq2_0", 37, tq.TQ2_0)])
@pytest.mark.parametrize("cfg", ["tiny-gqa4", "tiny-8b-2l", "tiny-qwen3", "tiny-qwen3moe", "tiny-w320", "llama-3-8b"])
def test_writer_mix(pkg, cfg, ftype, fid, t):
    """token_embd Q4_K, output Q6_K, every other 2-D weight the ternary type (experts included); rows that are no multiple of 256 fall back: Q4_0 for the
    ternary type, Q4_K's and Q6_K's own fallbacks for the two tables."""
    gs = pkg.gguf_synth
    c = gs.CONFIGS[cfg]
    assert gs.FTYPE_ID[ftype] == fid and gs.TYPE_NAME[t] == ftype and gs.BLOCK_BYTES[t] == tq.BLOCK_BYTES[t] and gs.BLOCK_ELEMS[t] == 256
    assert gs.FALLBACK_32[t] == gs.Q4_0
    seen = set()
    for name, ne, ty, _ in gs.model_tensors(c, ftype):
        if len(ne) == 1 or name.endswith("ffn_gate_inp.weight"):
            continue
        whole = ne[0] % 256 == 0
        if name == "token_embd.weight":
            want = gs.Q4_K if whole else gs.Q5_0
        elif name == "output.weight":
            want = gs.Q6_K if whole else gs.Q8_0
        else:
            want = t if whole else gs.Q4_0
        assert ty == want, (name, ty, want)
        seen.add(ty)
    assert (t in seen) == (cfg != "tiny-w320")                  # (320 / 608 wide: every row of that config falls back)


@pytest.mark.parametrize("ftype,fid,t", [("tq1_0", 36, tq.TQ1_0), ("tq2_0", 37, tq.TQ2_0)])
@pytest.mark.parametrize("cfg", ["tiny-gqa4", "tiny-qwen3moe"])
def test_writer_files_parse(pkg, tmp_path, cfg, ftype, fid, t):
    gs = pkg.gguf_synth
    path = str(tmp_path / "m.gguf")
    gs.write_synthetic_llama(path, cfg, ftype, seed=7)
    kv, tensors = read_gguf(path)
    assert kv["general.file_type"] == fid
    want = {n: (ne, ty) for n, ne, ty, _ in gs.model_tensors(gs.CONFIGS[cfg], ftype)}
    assert set(tensors) == set(want)
    n_t = 0
    for n, (ne, ty, raw) in tensors.items():
        assert (ne, ty) == want[n], n
        if ty == t:
            n_el = int(np.prod(ne))
            d, q = tq.decode(t, raw[: tq.row_bytes(t, n_el)], n_el)
            assert raw.size >= tq.row_bytes(t, n_el) and np.isfinite(d).all() and q.max() <= 2
            n_t += 1
    assert n_t >= 7


# sha256 of files the parent commit's writer produced (config, ftype, seed 7, with the vocabulary): every existing ftype still writes these bytes
OLD_FILES = {
    ("tiny-gqa4", "q4_k_m"): "3c685bf8b491dec2db330bc12f2a2be710e170b7580f661d67d5e74a8229f5ec", ("tiny-gqa4", "q2_k"): "a8e30ceb020bf63c0903fc16938428c4042c501760c3c4e79ef261c3d67628d8", ("tiny-gqa4", "iq4_xs"): "66c2c19ea765d5782dae368565eb14ca0aa2885bee75e665e3996770561002ea", ("tiny-gqa4", "q4_1"): "328258f248ac019b49b055ee4f11607d16028ad0eb95c3cf57b845fb9f6a9e67", ("tiny-gqa4", "q8_0"): "82fbd75f1193484cb65b5e6a2e1c9c8cb1c9e3d735ef29c4620dd0f80b9c0503",
    ("tiny-gqa4", "f16"): "b7c4a66bd43378fce48e518a85e8b80061a13f799c5b3713cf9a75770e9559a5", ("tiny-gqa4", "bf16"): "95bba0856c8dbd5d145166ce08658651ee29c25afcb05cb317f45efc3f2b7719", ("tiny-gqa4", "q4_0"): "47b6a5f45a25171a12fc99a30f60f4cabfa96a954dae912e39173ad620f38b32", ("tiny-gqa4", "q5_0"): "071d3b61d471374fb4dbd0705d954dbef49cd0baa228b4e6e7d64cc8dbdbf483", ("tiny-gqa4", "q5_1"): "0395d2fe3a3bff235324dc3d91c76841c3436df14268f5ed32640d8755f2ee7b",
    ("tiny-gqa4", "iq4_nl"): "5e8b97e443abede23437cffc467a4b89fe55132667c8c8608f6e4458dce4566c", ("tiny-gqa4", "q3_k_m"): "dfe538211168dcb4036e1aad0b4083c471a2341b667d1ab195ce487e4e14e00b", ("tiny-gqa4", "q5_k_m"): "77a81270582541f9088bcebb91cd79a2145bbf2ed3c4d9a538008fae3f876c75", ("tiny-gqa4", "q6_k"): "14c3af453c984d4fe9129895461547a036341df300520d7e24c22bed52670783", ("tiny-gqa4", "mxfp4"): "3561d9c61ac3496e6c1b5b8e5da4eeec93c7367202121b0cdf2eb90c0b7a4990",
    ("tiny-qwen3moe", "mxfp4_moe"): "ca9392cf85f74c9fbf5ee150396a045eeafb79f7b592e163402187897fdc0e68", ("tiny-qwen3moe", "iq4_xs"): "e2e489668424c474e0275ae8e59d0d845fcce3f4ed9510066235ff8c13b259e9", ("tiny-w320", "q4_k_m"): "097c85f9a86df425314991a8226bceebdbf0069abd8795ec26f499373c639881",
}


@pytest.mark.parametrize("key", list(OLD_FILES), ids=lambda k: "-".join(k))
def test_existing_ftypes_write_the_same_bytes(pkg, tmp_path, key):
    cfg, ftype = key
    path = str(tmp_path / "m.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, cfg, ftype, seed=7)
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == OLD_FILES[key]


# ------------------------------------------------------------------------------------------------ the host-only load planner
@pytest.mark.parametrize("ftype,t", [("tq1_0", tq.TQ1_0), ("tq2_0", tq.TQ2_0)])
@pytest.mark.parametrize("cfg", ["tiny-gqa4", "tiny-qwen3", "tiny-qwen3moe", "tiny-w320"])
def test_planner_accepts_ternary_files(pkg, plan_exe, tmp_models, cfg, ftype, t):
    """The planner takes the file; a ternary tensor's device row is the file's bytes padded to 16 (the packed trits, nothing wider) and it is staged for the
    regrouping into planes.  On the parent commit these files stop at `has unsupported type unknown`."""
    gs = pkg.gguf_synth
    c = gs.CONFIGS[cfg]
    p = plan(plan_exe, model_file(gs, tmp_models, cfg, ftype))
    assert "err" not in p, p
    file_tensors = {name: (ne, ty) for name, ne, ty, _ in gs.model_tensors(c, ftype)}
    n_t = stage = 0
    for x in p["tensors"]:
        ne, ty = file_tensors[x["name"]]
        assert x["type"] == ty
        if ty == t:
            K, rows = ne[0], int(np.prod(ne[1:]))
            assert x["row_bytes"] == (tq.row_bytes(t, K) + 15) & ~15 and x["bytes"] == x["row_bytes"] * rows
            assert x["src_bytes"] == x["file_bytes"] == tq.row_bytes(t, K) * rows
            stage = max(stage, x["src_bytes"])
            n_t += 1
    assert (n_t > 0) == (cfg != "tiny-w320") and p["max_stage"] >= stage
    assert p["bytes_per_token"] > 0


@pytest.mark.parametrize("ftype,t", [("tq1_0", tq.TQ1_0), ("tq2_0", tq.TQ2_0)])
def test_planner_refusals_name_the_type(pkg, plan_exe, tmp_models, tmp_path, monkeypatch, ftype, t):
    m = Maker(pkg.gguf_synth, tmp_models, tmp_path, monkeypatch)
    # a row split: in the words of the other types (layer 0's tensors are all refused; the last one asked for is the one reported)
    p = plan(plan_exe, m.copy("tiny-d128", ftype), 0, 2)
    assert p == {"status": -102, "err": ROW + " of " + ftype + " tensors is not supported (tensor blk.0.ffn_down.weight): load the file on one device"}
    # a 1-D tensor of the type
    p = plan(plan_exe, m.retyped("tiny", "blk.0.attn_norm.weight", t))
    assert p == {"status": -102, "err": "tensor blk.0.attn_norm.weight has type " + ftype + ": norm and bias vectors must be f32"}
    # the encoder graph
    p = plan(plan_exe, m.retyped("tiny-nomic", "blk.0.attn_qkv.weight", t, "f16"))
    assert p == {"status": -102, "err": "tensor blk.0.attn_qkv.weight has type " + ftype + ": the encoder graph is not supported with ternary tensors"}
    # rows that are not whole 256-blocks: refused per tensor, as for every 256-element type
    p = plan(plan_exe, m.retyped("tiny-w320", "blk.0.attn_q.weight", t, "q8_0"))
    assert p == {"status": -102, "err": "tensor blk.0.attn_q.weight (" + ftype + "): its row length 320 is not a whole number of 256-element blocks"}


# ------------------------------------------------------------------------------------------------ the reference models
@pytest.mark.parametrize("cfg,ref,sub", [("tiny-gqa4", Qwen3Ref, tq.TqRef), ("tiny-qwen3", Qwen3Ref, tq.TqRef), ("tiny-qwen3moe", Qwen3MoeRef, tq.TqMoeRef)])
def test_reference_models_are_their_parents_without_ternary_tensors(pkg, tmp_path, cfg, ref, sub):
    path = str(tmp_path / "m.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, cfg, "q4_k_m", seed=11)
    a, b = ref(path, 64, oq.Q8_0, oq.Q8_0), sub(path, 64, oq.Q8_0, oq.Q8_0)
    toks = [1, 17, 42, 5]
    la, lb = a.decode(toks, np.arange(4)), b.decode(toks, np.arange(4))
    assert la.tobytes() == lb.tobytes()
    for il in range(a.n_layer):
        assert a.layer_out(il, 4).tobytes() == b.layer_out(il, 4).tobytes()
    la, lb = a.decode([9], [4]), b.decode([9], [4])
    assert la.tobytes() == lb.tobytes()


@pytest.mark.parametrize("ftype", ["tq1_0", "tq2_0"])
def test_reference_model_runs_on_ternary_files(pkg, tmp_path, ftype):
    path = str(tmp_path / "m.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny-qwen3moe", ftype, seed=2)
    r = tq.TqMoeRef(path, 32, oq.Q8_0, oq.Q8_0)
    lg = r.decode([1, 7, 3], np.arange(3))
    assert np.isfinite(lg).all() and np.abs(lg).max() > 0
