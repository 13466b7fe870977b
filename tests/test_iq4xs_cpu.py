"""IQ4_XS on the CPU side: the numpy restatement of tests/iq4xs_ref.py on hand-built blocks, its dot product against an f64 dot of the dequantised rows,
what the synthetic writer's iq4_xs files contain, and the reference models against their parents on a file without IQ4_XS tensors."""
import numpy as np
import pytest

import iq4xs_ref as ix
import oracle_py as oq
from gguf_read import read_gguf
from qwen3_ref import Qwen3Ref
from qwen3moe_ref import Qwen3MoeRef


def _block(d=1.0, ls=None, nib=None):
    """One IQ4_XS block: ls[8] 6-bit scales, nib[256] code-book indices (element order)."""
    b = np.zeros(1, ix.DT)
    b["d"] = np.float16(d)
    ls = np.full(8, 32) if ls is None else np.asarray(ls)
    nib = np.zeros(256, np.int64) if nib is None else np.asarray(nib)
    for ib in range(8):
        b["scales_l"][0, ib // 2] |= (ls[ib] & 0xF) << (4 * (ib % 2))
        b["scales_h"][0] |= ((ls[ib] >> 4) & 3) << (2 * ib)
        for j in range(16):
            b["qs"][0, 16 * ib + j] = nib[32 * ib + j] | (nib[32 * ib + 16 + j] << 4)
    return b.view(np.uint8)


def test_block_size_and_type_id():
    assert ix.IQ4_XS == 23 and ix.row_bytes(256) == 136 and ix.row_bytes(4096) == 16 * 136


def test_scale_32_gives_zeros():
    rng = np.random.default_rng(1)
    raw = _block(3.5, np.full(8, 32), rng.integers(0, 16, 256))
    assert not ix.dequantize(raw, 256).any()


def test_extreme_scales_and_code_book():
    """ls = 0 and 63 (the ends of (ls - 32): -32, 31) against the ends of the code book (-127, 113), in every sub-block position."""
    nib = np.tile(np.r_[np.zeros(16, int), np.full(16, 15)], 8)
    ls = np.array([0, 63, 0, 63, 63, 0, 63, 0])
    y = ix.dequantize(_block(0.5, ls, nib), 256).reshape(8, 32)
    for ib in range(8):
        s = np.float32(0.5) * np.float32(ls[ib] - 32)
        assert (y[ib, :16] == s * np.float32(-127)).all() and (y[ib, 16:] == s * np.float32(113)).all()
    assert y.min() == np.float32(31 * 0.5 * -127) and y.max() == np.float32(-32 * 0.5 * -127)


@pytest.mark.parametrize("ib", range(8))
def test_scales_h_bit_positions(ib):
    """Only sub-block ib carries a high scale bit pair: bits 2 ib, 2 ib + 1 of scales_h; its low nibble is nibble ib of scales_l."""
    for hi in (1, 2, 3):
        ls = np.full(8, 32)
        ls[ib] = (hi << 4) | 5
        b = _block(1.0, ls, np.full(256, 8)).view(ix.DT)                         # level[8] = 1
        assert b["scales_h"][0] == (hi << (2 * ib)) | sum(2 << (2 * k) for k in range(8) if k != ib)
        y = ix.dequantize(b.view(np.uint8), 256).reshape(8, 32)
        want = np.full(8, 0.0, np.float32)
        want[ib] = ls[ib] - 32
        assert (y[:, 0] == want).all()


def test_nibble_order():
    """Element j < 16 of a sub-block is the low nibble of its code byte j, element j >= 16 the high nibble of byte j - 16."""
    nib = np.arange(256) % 16
    y = ix.dequantize(_block(1.0, np.full(8, 33), nib), 256)
    assert (y == ix.KVALUES[nib].astype(np.float32)).all()


@pytest.mark.parametrize("K", [256, 4096, 14336])
def test_dot_against_f64_of_dequantised_rows(pkg, K):
    """mul_mat in the generic f32 order against the f64 dot of the dequantised row and the dequantised Q8_K activation: within f32 rounding."""
    gs = pkg.gguf_synth
    rng = np.random.default_rng(K)
    N, T = 8, 3
    W = gs.random_blocks(rng, ix.IQ4_XS, N * K, 0.05)
    x = rng.standard_normal((T, K)).astype(np.float32)
    y = ix.mul_mat(W, N, K, x)
    Wf = ix.dequantize(W, N * K).reshape(N, K).astype(np.float64)
    for t in range(T):
        aq = ix.quantize_act(x[t])
        af = oq.dequantize(oq.Q8_K, aq, K).astype(np.float64)
        ref = Wf @ af
        scale = np.abs(Wf).dot(np.abs(af))
        assert np.all(np.abs(y[t] - ref) <= 2e-6 * scale + 1e-30), (np.abs(y[t] - ref) / scale).max()
        # the integer per super-block is the dot of the scaled levels and the codes
        for n in range(N):
            isum = ix.vec_dot_int_partials(W[n * ix.row_bytes(K):(n + 1) * ix.row_bytes(K)], aq, K)
            d, ls, lev = ix.decode(W[n * ix.row_bytes(K):(n + 1) * ix.row_bytes(K)], K)
            q8 = aq.view(ix.DT_Q8K)["qs"].astype(np.int64)
            want = ((np.repeat(ls, 32, axis=1) * lev).astype(np.int64) * q8).sum(axis=1)
            assert (isum == want).all() and np.abs(isum).max() < 1.3e8


def test_random_blocks_spread(pkg):
    """The writer's IQ4_XS blocks: finite d, and a dequantised std near the one asked for."""
    gs = pkg.gguf_synth
    raw = gs.random_blocks(np.random.default_rng(5), gs.IQ4_XS, 256 * 4096, 0.02)
    assert np.isfinite(raw.view(ix.DT)["d"].astype(np.float32)).all()
    y = ix.dequantize(raw, 256 * 4096)
    assert abs(y.std() / 0.02 - 1.0) < 0.05 and abs(y.mean()) < 0.002


@pytest.mark.parametrize("cfg", ["tiny-gqa4", "tiny-8b-2l", "tiny-qwen3", "tiny-qwen3moe", "llama-3-8b"])
def test_writer_mix(pkg, cfg):
    """iq4_xs: output Q6_K; attn_v Q5_K with a head ratio >= 4; the first eighth of ffn_down Q5_K; rows not a multiple of 256 IQ4_NL; token_embd and
    everything else (experts included) IQ4_XS; general.file_type 30."""
    gs = pkg.gguf_synth
    c = gs.CONFIGS[cfg]
    assert gs.FTYPE_ID["iq4_xs"] == 30 and gs.TYPE_NAME[gs.IQ4_XS] == "iq4_xs"
    for name, ne, t, _ in gs.model_tensors(c, "iq4_xs"):
        if len(ne) == 1 or name.endswith("ffn_gate_inp.weight") or name == "token_types.weight":
            continue
        il = int(name.split(".")[1]) if name.startswith("blk.") else 0
        if name == "output.weight":
            want = gs.Q6_K
        elif ".attn_v." in name and c.n_head // c.n_head_kv >= 4:
            want = gs.Q5_K
        elif ".ffn_down" in name and il < max(1, c.n_layer // 8):
            want = gs.Q5_K
        else:
            want = gs.IQ4_XS if ne[0] % 256 == 0 else gs.IQ4_NL
        assert t == want, (name, t, want)


@pytest.mark.parametrize("cfg", ["tiny-gqa4", "tiny-qwen3", "tiny-qwen3moe"])
def test_writer_files_parse(pkg, tmp_path, cfg):
    gs = pkg.gguf_synth
    path = str(tmp_path / "m.gguf")
    gs.write_synthetic_llama(path, cfg, "iq4_xs", seed=7)
    kv, t = read_gguf(path)
    assert kv["general.file_type"] == 30
    want = {n: (ne, ty) for n, ne, ty, _ in gs.model_tensors(gs.CONFIGS[cfg], "iq4_xs")}
    assert set(t) == set(want)
    for n, (ne, ty, raw) in t.items():
        assert (ne, ty) == want[n], n
        if ty == gs.IQ4_XS:
            nbytes = ix.row_bytes(ne[0]) * int(np.prod(ne)) // ne[0]
            assert raw.size >= nbytes and np.isfinite(ix.dequantize(raw[:nbytes], int(np.prod(ne)))).all()
    assert t["token_embd.weight"][1] == gs.IQ4_XS


def test_tiny_qwen3_head_is_iq4xs(pkg):
    gs = pkg.gguf_synth
    c = gs.CONFIGS["tiny-qwen3"]
    names = {n: t for n, _, t, _ in gs.model_tensors(c, "iq4_xs")}
    assert c.tied_output and "output.weight" not in names and names["token_embd.weight"] == gs.IQ4_XS


@pytest.mark.parametrize("cfg,ref,sub", [("tiny-gqa4", Qwen3Ref, ix.Iq4xsRef), ("tiny-qwen3", Qwen3Ref, ix.Iq4xsRef),
                                         ("tiny-qwen3moe", Qwen3MoeRef, ix.Iq4xsMoeRef)])
def test_reference_models_are_their_parents_without_iq4xs(pkg, tmp_path, cfg, ref, sub):
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


def test_reference_model_runs_on_iq4xs_file(pkg, tmp_path):
    """The reference decodes an iq4_xs file: finite logits, and its embedding rows are the dequantised IQ4_XS table."""
    gs = pkg.gguf_synth
    path = str(tmp_path / "m.gguf")
    gs.write_synthetic_llama(path, "tiny-qwen3", "iq4_xs", seed=2)
    r = ix.Iq4xsRef(path, 32, oq.Q8_0, oq.Q8_0)
    ne, ty, raw = r._embd_iq4
    E = ne[0]
    assert (r.t["token_embd.weight"][2].view("<f4")[7 * E:8 * E] == ix.dequantize(raw[7 * ix.row_bytes(E):8 * ix.row_bytes(E)], E)).all()
    lg = r.decode([1, 7, 3], np.arange(3))
    assert lg.shape == (1, ne[1]) and np.isfinite(lg).all()


def test_qkv_attn_plan_takes_the_llama_iq4xs_mix(pkg):
    """Host logic: at Llama-3-8B geometry the IQ4_XS mix (attn_q, attn_k, attn_output IQ4_XS, attn_v Q5_K) runs Q | K | V inside the attention launch, in no
    more LDS and DMA slots than Q4_K_M's layer; a Q4_K_M layer with an IQ4_XS attn_output takes it too."""
    import ctypes as C
    lib = pkg.load_library()

    def plan(tq, tk, tv, to):
        slots = C.c_int32(0)
        return int(lib.mi355_debug_qkv_attn_plan(tq, tk, tv, to, 4096, 32, 8, 128, 8, 576, C.byref(slots))), int(slots.value)

    lds, slots = plan(ix.IQ4_XS, ix.IQ4_XS, oq.Q5_K, ix.IQ4_XS)
    lds_q4, slots_q4 = plan(oq.Q4_K, oq.Q4_K, oq.Q5_K, oq.Q4_K)
    assert 0 < lds <= lds_q4 and 0 < slots <= slots_q4, (lds, slots, lds_q4, slots_q4)
    assert plan(oq.Q4_K, oq.Q4_K, oq.Q5_K, ix.IQ4_XS)[0] > 0
