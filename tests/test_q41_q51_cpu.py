"""Q4_1 / Q5_1 on the CPU side: the numpy restatement of tests/q41_q51_ref.py on hand-built blocks, the writer's reference quantisers, the restatement's
mul_mat against the oracle's F32 mul_mat of the dequantised operands and against ggml's Q8_1 form, and what the synthetic writer's q4_1 / q5_1 files hold."""
import numpy as np
import pytest

import oracle_py as oq
import q41_q51_ref as mr
from gguf_read import read_gguf

Q4_1, Q5_1 = mr.Q4_1, mr.Q5_1
TOP = {Q4_1: 15, Q5_1: 31}
SHAPES = [(32, 33), (96, 33), (2080, 33), (4096, 128)]          # (K, N): the shapes of tests/test_gpu_q41_q51.py


def _block(t, d, m, q):
    """One block from its codes q[32] (element order), built byte by byte from the layout in the issue: d | m | [qh] | qs."""
    q = np.asarray(q, np.int64)
    raw = np.zeros(mr.BLOCK_BYTES[t], np.uint8)
    raw[0:2] = np.array([d], "<f2").view(np.uint8)
    raw[2:4] = np.array([m], "<f2").view(np.uint8)
    o = 4
    if t == Q5_1:
        qh = 0
        for j in range(32):
            qh |= int((q[j] >> 4) & 1) << j
        raw[4:8] = np.array([qh], "<u4").view(np.uint8)
        o = 8
    for j in range(16):
        raw[o + j] = (q[j] & 15) | ((q[j + 16] & 15) << 4)
    return raw


def weights(pkg, rng, t, n, std=0.05, mean=0.02):
    """Random blocks with a weight mean away from zero: every block's minimum shifted up by `mean`."""
    raw = pkg.gguf_synth.random_blocks(rng, t, n, std)
    b = raw.view(mr.DT[t])
    b["m"] = (b["m"].astype(np.float32) + np.float32(mean)).astype("<f2")
    return raw


@pytest.mark.parametrize("t", [Q4_1, Q5_1])
def test_block_layout_and_decode(pkg, t):
    gs = pkg.gguf_synth
    assert gs.BLOCK_BYTES[t] == mr.BLOCK_BYTES[t] == (20 if t == Q4_1 else 24) and gs.BLOCK_ELEMS[t] == 32
    assert gs.BLOCK_DTYPE[t].itemsize == mr.BLOCK_BYTES[t] and gs.TYPE_NAME[t] == ("q4_1" if t == Q4_1 else "q5_1")
    q = (np.arange(32) * 7 + 3) % (TOP[t] + 1)
    raw = _block(t, 0.5, -1.25, q)
    d, m, qq = mr.decode(t, raw, 32)
    assert d[0] == 0.5 and m[0] == -1.25 and (qq[0] == q).all()
    y = mr.dequantize(t, raw, 32)
    assert (y == (q * np.float32(0.5) - np.float32(1.25)).astype(np.float32)).all()
    # the ends of the code range, no offset: 0 -> m, top -> top * d + m
    y = mr.dequantize(t, _block(t, 2.0, 3.0, np.r_[np.zeros(16, int), np.full(16, TOP[t])]), 32)
    assert (y[:16] == 3.0).all() and (y[16:] == 2.0 * TOP[t] + 3.0).all()


def test_q5_1_fifth_bit_positions():
    """Bit j of qh is the fifth bit of element j, for the low-nibble elements (j < 16) and the high-nibble ones alike."""
    for j in range(32):
        q = np.zeros(32, int)
        q[j] = 16
        raw = _block(Q5_1, 1.0, 0.0, q)
        assert raw[4:8].view("<u4")[0] == 1 << j and not raw[8:].any()
        y = mr.dequantize(Q5_1, raw, 32)
        assert y[j] == 16.0 and y.sum() == 16.0


@pytest.mark.parametrize("t", [Q4_1, Q5_1])
def test_reference_quantiser_round_trip(pkg, t):
    """quantize_min32 -> decode: the block's minimum and maximum come back within the f16 rounding of d and m, every value within half a step; the bytes
    are the hand-built block's."""
    gs = pkg.gguf_synth
    rng = np.random.default_rng(t)
    x = (rng.standard_normal(64 * 32) * 0.3 + 0.7).astype(np.float32)
    raw = gs.quantize_min32(t, x)
    assert raw.size == mr.row_bytes(t, x.size)
    d, m, q = mr.decode(t, raw, x.size)
    assert q.min() == 0 and q.max() == TOP[t]
    xb = x.reshape(-1, 32)
    mn, mx = xb.min(axis=1), xb.max(axis=1)
    assert (m == mn.astype(np.float16).astype(np.float32)).all()
    assert (d == ((mx - mn) / np.float32(TOP[t])).astype(np.float16).astype(np.float32)).all()
    y = mr.dequantize(t, raw, x.size).reshape(-1, 32)
    step = ((mx - mn) / TOP[t])[:, None]
    # half a step of the unrounded grid, plus the f16 roundings of d (times up to `top` codes) and of m
    tol = 0.5 * step + 2.0 ** -11 * (TOP[t] * step + np.abs(mn)[:, None]) + 1e-7
    assert (np.abs(y - xb) <= tol).all(), float((np.abs(y - xb) / tol).max())
    # a block on an exact grid quantises to its own codes: x = q * d + m with d, m exact in f16
    qq = (np.arange(32) * 5 + 1) % (TOP[t] + 1)
    qq[0], qq[1] = 0, TOP[t]
    xg = (qq * np.float32(0.25) - np.float32(2.0)).astype(np.float32)
    assert gs.quantize_min32(t, xg).tobytes() == _block(t, 0.25, -2.0, qq).tobytes()
    # a constant block: d = 0, every code 0, m the value
    raw0 = gs.quantize_min32(t, np.full(32, 1.5, np.float32))
    d0, m0, q0 = mr.decode(t, raw0, 32)
    assert d0[0] == 0 and m0[0] == 1.5 and not q0.any()


def test_activation_quantiser_is_the_oracles():
    """The restatement's Q8_0 codes and stored scales are the oracle's quantize_row_q8_0; the unrounded scale rounds to the stored one."""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(4096) * rng.uniform(0.01, 30.0, 4096)).astype(np.float32)
    x[64:96] = 0.0
    q, d16, d32 = mr.quantize_act(x)
    want = np.asarray(oq.quantize(oq.Q8_0, x)).view(np.uint8)[: 128 * 34].view(mr.DT_Q80)
    assert (q == want["qs"]).all() and (d16 == want["d"].astype(np.float32)).all()
    assert (d32.astype(np.float16).astype(np.float32) == d16).all()


@pytest.mark.parametrize("t", [Q4_1, Q5_1])
@pytest.mark.parametrize("K,N", SHAPES)
def test_mul_mat_against_the_oracles_f32_mul_mat(pkg, t, K, N):
    """The restatement against the oracle's F32 mul_mat of the dequantised weights and the dequantised Q8_0 activations, within the f32 summation error:
    both sum K products (the restatement as K / 32 block terms of three roundings each, the oracle element by element), so each is within about
    (K + 3 K / 32) * 2^-24 of the exact sum of |w a|; 2 K * 2^-24 covers the two together.  The integer partials are the dots of the codes."""
    rng = np.random.default_rng(K + N + t)
    T = 3
    W = weights(pkg, rng, t, N * K)
    x = rng.standard_normal((T, K)).astype(np.float32)
    y = mr.mul_mat(t, W, N, K, x)
    Wf = mr.dequantize(t, W, N * K).reshape(N, K)
    af = np.stack([oq.dequantize(oq.Q8_0, oq.quantize(oq.Q8_0, r), K) for r in x])
    ref = oq.mul_mat(oq.F32, Wf.view(np.uint8).reshape(-1), N, K, af, 2)
    scale = np.abs(af.astype(np.float64)) @ np.abs(Wf.astype(np.float64)).T
    assert (np.abs(y.astype(np.float64) - ref) <= 2 * K * 2.0 ** -24 * scale + 1e-30).all(), float((np.abs(y - ref) / scale).max())
    rb = mr.row_bytes(t, K)
    codes = mr.quantize_act(x[1])[0]
    _, _, q = mr.decode(t, W, N * K)
    for r in (0, N - 1):
        isum, asum = mr.vec_dot_int_partials(t, W[r * rb:(r + 1) * rb], codes, K)
        assert (isum == (q.reshape(N, -1, 32)[r].astype(np.int64) * codes).sum(axis=1)).all() and (asum == codes.astype(np.int64).sum(axis=1)).all()
        assert np.abs(isum).max() <= 32 * 127 * TOP[t] and np.abs(asum).max() <= 32 * 127


@pytest.mark.parametrize("t", [Q4_1, Q5_1])
@pytest.mark.parametrize("K,N", SHAPES)
def test_project_order_against_ggmls_q8_1_form(pkg, t, K, N):
    """|mul_mat - mul_mat_ggml| <= 2^-10 sum_b |m_b s_b| per output: the minimum's factor differs by two f16 roundings of 2^-11 each (of d8, and of s)."""
    rng = np.random.default_rng(2 * K + N + t)
    T = 5
    W = weights(pkg, rng, t, N * K)
    x = (rng.standard_normal((T, K)) * rng.uniform(0.1, 3.0, (T, 1))).astype(np.float32)
    a, b = mr.mul_mat(t, W, N, K, x), mr.mul_mat_ggml(t, W, N, K, x)
    bound = 2.0 ** -10 * mr.term_bound(t, W, N, K, x)
    assert (np.abs(a.astype(np.float64) - b) <= bound).all(), float((np.abs(a - b) / bound).max())
    assert (a != b).any() and bound.min() > 0                      # the minimum term is there, and the two forms are not the same number


@pytest.mark.parametrize("t", [Q4_1, Q5_1])
def test_random_blocks_spread(pkg, t):
    """The writer's blocks: finite d and m, a dequantised std near the one asked for, centred on zero."""
    gs = pkg.gguf_synth
    raw = gs.random_blocks(np.random.default_rng(5), t, 32 * 8192, 0.02)
    b = raw.view(mr.DT[t])
    assert np.isfinite(b["d"].astype(np.float32)).all() and np.isfinite(b["m"].astype(np.float32)).all()
    y = mr.dequantize(t, raw, 32 * 8192)
    assert abs(y.std() / 0.02 - 1.0) < 0.05 and abs(y.mean()) < 0.002


@pytest.mark.parametrize("ftype,t,fid", [("q4_1", Q4_1, 3), ("q5_1", Q5_1, 9)])
@pytest.mark.parametrize("cfg", ["tiny-gqa4", "tiny-d128", "tiny-qwen3moe", "llama-3-8b"])
def test_writer_mix(pkg, cfg, ftype, t, fid):
    """q4_1 / q5_1: output Q6_K, every other 2-D weight (token_embd and the experts included) the type; general.file_type 3 / 9."""
    gs = pkg.gguf_synth
    c = gs.CONFIGS[cfg]
    assert gs.FTYPE_ID[ftype] == fid
    seen = 0
    for name, ne, ty, _ in gs.model_tensors(c, ftype):
        if len(ne) == 1 or name.endswith("ffn_gate_inp.weight"):
            assert ty == gs.F32
            continue
        assert ty == (gs.Q6_K if name == "output.weight" else t), (name, ty)
        seen += ty == t
    assert seen >= 7 * c.n_layer + 1
    for kind in ("attn_q", "attn_v", "ffn_down", "token_embd"):
        assert gs.tensor_type(c, ftype, kind, 0) == t
    assert gs.tensor_type(c, "q5_0", "attn_q", 0) == gs.Q5_0 and gs.tensor_type(c, "q4_k_m", "attn_q", 0) == gs.Q4_K      # the other ftypes are what they were


@pytest.mark.parametrize("ftype,t,fid", [("q4_1", Q4_1, 3), ("q5_1", Q5_1, 9)])
@pytest.mark.parametrize("cfg", ["tiny-gqa4", "tiny-qwen3moe"])
def test_writer_files_parse(pkg, tmp_path, cfg, ftype, t, fid):
    gs = pkg.gguf_synth
    path = str(tmp_path / "m.gguf")
    gs.write_synthetic_llama(path, cfg, ftype, seed=7)
    kv, tens = read_gguf(path)
    assert kv["general.file_type"] == fid
    want = {n: (ne, ty) for n, ne, ty, _ in gs.model_tensors(gs.CONFIGS[cfg], ftype)}
    assert set(tens) == set(want)
    for n, (ne, ty, raw) in tens.items():
        assert (ne, ty) == want[n], n
        if ty == t:
            cnt = int(np.prod(ne))
            nbytes = mr.row_bytes(t, ne[0]) * cnt // ne[0]
            assert raw.size >= nbytes and np.isfinite(mr.dequantize(t, raw[:nbytes], cnt)).all()
    assert tens["token_embd.weight"][1] == t


def test_reference_model_runs_on_a_q5_1_file(pkg, tmp_path):
    """The reference decodes a q5_1 file: finite logits, and its embedding rows are the dequantised Q5_1 table."""
    gs = pkg.gguf_synth
    path = str(tmp_path / "m.gguf")
    gs.write_synthetic_llama(path, "tiny-gqa4", "q5_1", seed=2)
    r = mr.MinRef(path, 32, oq.Q8_0, oq.Q8_0)
    ne, ty, raw = r._embd_min
    E, rb = ne[0], mr.row_bytes(Q5_1, ne[0])
    assert ty == Q5_1 and (r.t["token_embd.weight"][2].view("<f4")[7 * E:8 * E] == mr.dequantize(Q5_1, raw[7 * rb:8 * rb], E)).all()
    lg = r.decode([1, 7, 3], np.arange(3))
    assert lg.shape == (1, ne[1]) and np.isfinite(lg).all()
