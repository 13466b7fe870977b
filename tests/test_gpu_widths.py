"""Row lengths that are whole 32-element blocks but no multiple of 256 (Qwen2.5-0.5B: n_embd 896; SmolLM2-135M: 576; gpt-oss: 2880) on the GPU: the
activation quantisers' partial last 256-group, the generic mat-vec (one token, tiled, fused prologue) and the Q8_0 prompt kernel at such K, and whole files
end to end.  The bars are those of tests/test_gpu_ops.py and tests/test_gpu_model.py for multiples of 256, restated here unchanged.  Q4_1 / Q5_1 and MXFP4
are checked against tests/q41_q51_ref.py and tests/mxfp4_ref.py, the project's references for the types the CPU oracle does not have."""
import dataclasses
import struct

import numpy as np
import pytest

import mxfp4_ref as xr
import oracle_py as oq
import q41_q51_ref as mr
from oracle_py import F16, IQ4_NL, Q4_0, Q5_0, Q8_0, Q8_K

pytestmark = pytest.mark.gpu

Q4_1, Q5_1, MXFP4 = mr.Q4_1, mr.Q5_1, xr.MXFP4
KV = {"f16": 1, "q8_0": 8, "q4_0": 2}
FLIP_TOL = 3e-2          # tests/test_gpu_model.py (where the tolerance is derived)
EPS = 1e-5


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


# ------------------------------------------------------------------------------------------------ quantisers
WIDTHS = [32, 96, 288, 896, 2880]       # all end inside a 256-group: tails of 1, 3, 1, 4 and 2 blocks of 32


def planted(n, rows, seed):
    """[rows][n] with the cases of test_activation_quant_bit_exact in the first block of the row's partial last group, one case per row in turn: an all-zero
    block; the rounding ties +-0.5 / 1.5 / 2.5 beside a -127 extreme (block scale 1); equal magnitudes (the first wins)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, n)) * rng.uniform(0.01, 30, (rows, 1))).astype(np.float32)
    g0 = (n // 256) * 256
    case = []
    for r in range(rows):
        c = (r + seed) % 3
        case.append(c)
        x[r, g0:g0 + 32] = np.clip(x[r, g0:g0 + 32], -4.0, 4.0)
        if c == 0:
            x[r, g0:g0 + 32] = 0.0
        elif c == 1:
            x[r, g0:g0 + 6] = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5]
            x[r, g0 + 7] = -127.0
        else:
            x[r, g0 + 10] = 5.0; x[r, g0 + 20] = -5.0
    return x, case


def seeds_for(rows):
    return (0, 1, 2) if rows == 1 else (0,)     # one row: each planted case in its own call


@pytest.mark.parametrize("rows", [1, 5, 40])     # 40: the wide prompt-batch form of the kernels
@pytest.mark.parametrize("n", WIDTHS)
def test_quantize_act_partial_last_group_bit_exact(be, n, rows):
    """Codes and f16 scales of every block, the 1 .. 7 blocks behind the last whole 256-group included, are quantize_row_q8_0's; the hook checks that the row
    behind the last one was not written (it fails with "wrote past the last row").  Q8_K keeps whole 256-blocks."""
    for seed in seeds_for(rows):
        x, _ = planted(n, rows, seed)
        got = be.quantize_act(Q8_0, x)
        assert got.shape == (rows, 34 * (n // 32))
        for r in range(rows):
            assert (got[r] == oq.quantize(Q8_0, x[r])).all(), (seed, r)


def test_q8_k_keeps_whole_256_blocks(be, pkg):
    with pytest.raises(pkg.MI355Error, match="bad args"):
        be.quantize_act(Q8_K, np.ones((2, 288), np.float32))
    with pytest.raises(pkg.MI355Error, match="bad args"):
        be.quantize_act(Q8_0, np.ones((2, 48), np.float32))


@pytest.mark.parametrize("rows", [1, 5, 40])
@pytest.mark.parametrize("n", WIDTHS)
def test_rms_norm_quant_partial_last_group(be, n, rows):
    """RMSNorm * weight -> Q8_0 in one launch: the f32 rows within 2e-5 max|ref| of the oracle's rms_norm * w (the sum of squares over exactly n elements: a
    dropped or doubled tail would move the scale by far more), the blocks bit-equal to quantize_row_q8_0 of those f32 rows."""
    for seed in seeds_for(rows):
        x, case = planted(n, rows, seed)
        rng = np.random.default_rng(100 + n + rows)
        w = rng.uniform(0.5, 1.5, n).astype(np.float32)
        g0 = (n // 256) * 256
        w[g0 + 20] = w[g0 + 10]                           # the equal magnitudes stay equal after the weight
        blocks, y = be.rms_norm_quant(x, w, EPS)
        for r in range(rows):
            ref = oq.rms_norm(x[r], EPS) * w
            assert np.abs(y[r] - ref).max() <= 2e-5 * np.abs(ref).max(), (seed, r)
            assert (blocks[r] == oq.quantize(Q8_0, y[r])).all(), (seed, r)
            if case[r] == 0:
                assert not y[r, g0:g0 + 32].any() and not blocks[r, 34 * (g0 // 32):34 * (g0 // 32 + 1)].any()
        # the launch that writes no blocks gives the same f32 rows
        assert np.array_equal(bits(be.rms_norm_mul(x, w, EPS)), bits(y))


@pytest.mark.parametrize("rows", [1, 5, 40])
@pytest.mark.parametrize("n", WIDTHS)
def test_swiglu_quant_partial_last_group(be, n, rows):
    """silu(gate) * up -> Q8_0 in one launch.  The hook returns blocks only; the f32 rows are those of the SwiGLU launch it shares its arithmetic with
    (mi355_op_swiglu), held to 2e-5 max|ref| of the oracle's silu * up, and the blocks are bit-equal to quantize_row_q8_0 of them.  Planted: gate = 32, where
    silu is exact in f32, and up = value / 32, so that the planted values reach the quantiser exactly."""
    for seed in seeds_for(rows):
        v, _ = planted(n, rows, seed)
        rng = np.random.default_rng(200 + n + rows)
        g = (rng.standard_normal((rows, n)) * 3).astype(np.float32)
        u = rng.standard_normal((rows, n)).astype(np.float32)
        g0 = (n // 256) * 256
        g[:, g0:g0 + 32] = 32.0
        u[:, g0:g0 + 32] = v[:, g0:g0 + 32] / np.float32(32.0)
        blocks = be.swiglu_quant(g, u)
        y = be.swiglu(g.reshape(-1), u.reshape(-1)).reshape(rows, n)
        assert np.array_equal(y[:, g0:g0 + 32], v[:, g0:g0 + 32])
        for r in range(rows):
            ref = oq.silu(g[r]) * u[r]
            assert np.abs(y[r] - ref).max() <= 2e-5 * np.abs(ref).max(), (seed, r)
            assert (blocks[r] == oq.quantize(Q8_0, y[r])).all(), (seed, r)


# ------------------------------------------------------------------------------------------------ mat-mul
SHAPES = [(32, 3, 1), (96, 33, 1), (896, 37, 1), (2880, 33, 1),        # one token: the generic mat-vec
          (896, 33, 3), (2880, 20, 16),                                # 2 + 1 tokens; the tiled form
          (896, 130, 33), (2880, 129, 70), (96, 128, 40)]              # the Q8_0 prompt kernel, on the weights or their Q8_0-layout copy
TYPES = [Q8_0, Q4_0, Q5_0, IQ4_NL, Q4_1, Q5_1, MXFP4, F16]


def ref_mul_mat(t, W, N, K, x):
    if t in (Q4_1, Q5_1):
        return mr.mul_mat(t, W, N, K, x)
    if t == MXFP4:
        return xr.mul_mat(W, N, K, x)
    return oq.mul_mat(t, W, N, K, x)


@pytest.mark.parametrize("K,N,T", SHAPES)
@pytest.mark.parametrize("t", TYPES)
def test_mul_mat_k_not_a_multiple_of_256(be, pkg, t, K, N, T):
    """Integer sums per (token, row, 32-block) bit-exact against the format's vec_dot, the f32 result within 2e-5 max|ref| + 1e-6; from 32 tokens on the
    prompt kernel's MT = 1 / 2 / 4 forms give one result bit for bit."""
    rng = np.random.default_rng(K + 3 * N + 7 * T + 1000 * t)
    W = pkg.gguf_synth.random_blocks(rng, t, N * K, 0.05)
    x = (rng.standard_normal((T, K)) * rng.uniform(0.2, 2.0, (T, 1))).astype(np.float32)
    ref = ref_mul_mat(t, W, N, K, x)
    if t == F16:
        y = be.mul_mat(t, W, N, K, x)
    else:
        y, isum, msum = be.mul_mat(t, W, N, K, x, want_ints=True)
        if t in (Q4_1, Q5_1, MXFP4):
            codes = np.stack([mr.quantize_act(r)[0] for r in x]).astype(np.int64)                 # [T][nb][32]
            q = (mr.decode(t, W, N * K)[2] if t != MXFP4 else xr.decode(W, N * K)[1]).reshape(N, K // 32, 32).astype(np.int64)
            assert np.array_equal(isum, np.einsum("nbk,tbk->tnb", q, codes))
            if t == MXFP4:
                assert not msum.any()
            else:
                assert np.array_equal(msum, np.broadcast_to(codes.sum(axis=2)[:, None, :], msum.shape))
        else:
            rb = oq.row_bytes(t, K)
            for tt in range(T):
                act = oq.quantize(Q8_0, x[tt])
                for r in range(0, N, max(1, N // 7)):
                    wi, wm = oq.vec_dot_int_partials(t, W[r * rb:(r + 1) * rb], act, K)
                    assert (isum[tt, r] == wi).all() and (msum[tt, r] == 0).all(), (tt, r)
    assert np.abs(y - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-6
    if T >= 32 and t != F16:
        try:
            forms = []
            for mt in (1, 2, 4):
                be.set_option("mmq_q80_tiles", mt)
                forms.append(be.mul_mat(t, W, N, K, x))
        finally:
            be.set_option("mmq_q80_tiles", 0)
        assert np.array_equal(bits(forms[0]), bits(forms[1])) and np.array_equal(bits(forms[0]), bits(forms[2]))
        assert np.abs(forms[0] - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-6


@pytest.mark.parametrize("T", [1, 5, 40])
@pytest.mark.parametrize("K", [896, 320])
@pytest.mark.parametrize("t", [Q5_0, Q8_0])
def test_ffn_gate_up_k_not_a_multiple_of_256(be, pkg, t, K, T):
    """ffn_gate | ffn_up with SwiGLU as a layer of such a file runs them (the mat-vec with SwiGLU in its epilogue; from 32 tokens on the Q8_0 prompt kernel and
    the SwiGLU pass), to test_ffn_gate_up_swiglu_launch's bar."""
    N = 70
    rng = np.random.default_rng(K + T + t)
    Wg, Wu = pkg.gguf_synth.random_blocks(rng, t, N * K, 0.05), pkg.gguf_synth.random_blocks(rng, t, N * K, 0.05)
    x = (rng.standard_normal((T, K)) * rng.uniform(0.1, 2.0, (T, 1))).astype(np.float32)
    y = be.ffn_gate_up(t, Wg, Wu, N, K, x)
    g, u = oq.mul_mat(t, Wg, N, K, x), oq.mul_mat(t, Wu, N, K, x)
    with np.errstate(over="ignore"):
        ref = (g / (1.0 + np.exp(-g.astype(np.float64)))).astype(np.float32) * u
    assert np.abs(y - ref).max() <= 4e-5 * np.abs(ref).max() + 1e-6


@pytest.mark.parametrize("K", [96, 896, 2880])
@pytest.mark.parametrize("t", [Q8_0, Q5_0, IQ4_NL, Q4_1, MXFP4])
def test_fused_prologue_is_bitwise_the_two_launches(be, pkg, t, K):
    """One token's mat-vec with its activation made in the launch's prologue - RMSNorm * weight + Q8_0 (fuse mode 1), Q8_0 only (mode 2) - against the
    quantiser's launch followed by the mat-vec's: the same bits."""
    N = 37
    rng = np.random.default_rng(K + t)
    W = pkg.gguf_synth.random_blocks(rng, t, N * K, 0.05)
    x = (rng.standard_normal(K) * 1.7).astype(np.float32)
    w = rng.uniform(0.5, 1.5, K).astype(np.float32)
    sep2 = be.mul_mat(t, W, N, K, x[None, :])[0]
    assert np.array_equal(bits(be.mul_mat_fused(t, W, N, K, x)), bits(sep2))
    blocks, y = be.rms_norm_quant(x[None, :], w, EPS)
    assert (blocks[0] == oq.quantize(Q8_0, y[0])).all()           # (so quantising y again, as mul_mat does, gives the fused launch's codes)
    sep1 = be.mul_mat(t, W, N, K, y)[0]
    assert np.array_equal(bits(be.mul_mat_fused(t, W, N, K, x, norm_w=w, eps=EPS)), bits(sep1))
    ref = ref_mul_mat(t, W, N, K, y)[0]
    assert np.abs(sep1 - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-6


# ------------------------------------------------------------------------------------------------ whole files
def make(pkg, tmp_models, cfg, ftype, seed=11):
    path = str(tmp_models / f"{cfg}-{ftype}-{seed}.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, cfg, ftype, seed=seed)
    return path


def has_min_types(pkg, cfg, ftype):
    gs = pkg.gguf_synth
    return any(t in (gs.Q4_1, gs.Q5_1) for _, _, t, _ in gs.model_tensors(gs.CONFIGS[cfg], ftype))


class Ref:
    """The CPU reference of a file: the oracle, or - for a file with Q4_1 / Q5_1 tensors, which the oracle does not have - tests/q41_q51_ref.py over it."""

    def __init__(self, pkg, path, cfg, ftype, n_ctx, kv):
        self.om = None
        if has_min_types(pkg, cfg, ftype):
            self.c = mr.MinRef(path, n_ctx, KV[kv], KV[kv])
        else:
            self.om = oq.OracleModel(path)
            self.c = oq.OracleContext(self.om, n_ctx, KV[kv], KV[kv], True, oq.threads())

    def decode(self, toks, pos):
        return np.asarray(self.c.decode(toks, pos)[0])

    def layer_out(self, il, n):
        return np.asarray(self.c.layer_out(il, n)).reshape(n, -1)

    def close(self):
        if self.om is not None:
            self.c.close(); self.om.close()


TIED_W896 = ("tiny-w896-2l",)           # CPU top-2 gap >= 0.74 of the logit scale at every step (prompt seeds 0..5): no near tie to flip


@pytest.mark.parametrize("cfg,ftype,kv", [("tiny-w896-2l", "q4_k_m", "q8_0"), ("tiny-w896-2l:40", "q8_0", "f16"), ("tiny-w896-2l-untied:40", "q4_k_m", "q8_0"),
                                          ("tiny-w576-2l", "q4_k_m", "q8_0"), ("tiny-w576-2l:40", "q5_k_m", "f16"),
                                          ("tiny-w320", "q8_0", "q8_0"), ("tiny-w320:40", "q5_0", "q8_0"), ("tiny-w320", "q4_1", "f16"),
                                          ("tiny-w320:70", "iq4_nl", "q4_0"), ("tiny-w320", "f16", "f16")])
def test_prefill_layers_logits_and_greedy_ids(be, pkg, tmp_models, cfg, ftype, kv):
    """The body of tests/test_gpu_model.py's test of the same name on files whose widths are no multiples of 256: per-layer taps and logits within FLIP_TOL, 24
    teacher-forced steps through the captured graph, the first layer's typical token within FLIP_TOL / 10 (Q8_0 activations), a device / CPU arg-max mismatch
    only at a near tie of the CPU logits and at most once per run - never on the tied 896-wide file, whose logits have no near tie."""
    cfg, _, np_s = cfg.partition(":")
    path = make(pkg, tmp_models, cfg, ftype)
    oq.set_fa_v_acc_f32(1 if kv == "f16" else 0)
    try:
        m = pkg.Model(path)
        c = pkg.Context(m, n_ctx=128, type_k=KV[kv], type_v=KV[kv], use_graphs=True, n_ubatch=512)
        oc = Ref(pkg, path, cfg, ftype, 128, kv)
        rng = np.random.default_rng(5)
        n_prompt = int(np_s) if np_s else 21
        prompt = rng.integers(0, m.n_vocab, n_prompt)
        c.enable_taps(True)
        c.decode(prompt, np.arange(n_prompt))
        ref = oc.decode(prompt, np.arange(n_prompt))
        errs = []
        for il in range(m.n_layer):
            errs.append(rel_err(c.layer_out(il, n_prompt).reshape(n_prompt, -1), oc.layer_out(il, n_prompt)))
        a0 = c.layer_out(0, n_prompt).reshape(n_prompt, -1)
        b0 = oc.layer_out(0, n_prompt)
        tok_err0 = np.abs(a0 - b0).max(axis=1) / max(1.0, float(np.abs(b0).max()))
        got = c.logits()
        errs.append(rel_err(got, ref))
        print(f"{cfg}:{np_s} {ftype} {kv}: layer / logit errors {errs}, first-layer median {float(np.median(tok_err0)):.3g}")
        assert max(errs) <= FLIP_TOL, errs
        c.enable_taps(False)
        tok = int(ref.argmax())
        step_err = [errs[-1]]
        mism = 0
        gaps = []
        for step in range(24):
            c.decode([tok], [n_prompt + step])
            r = oc.decode([tok], [n_prompt + step])
            g = c.logits()
            step_err.append(rel_err(g, r))
            tok = int(r.argmax())
            if c.argmax() != tok:
                top2 = np.sort(r)[-2:]
                assert top2[1] - top2[0] <= 2 * FLIP_TOL * max(1.0, np.abs(r).max()), (step, top2)
                mism += 1
                gaps.append((step, float((top2[1] - top2[0]) / max(1.0, np.abs(r).max()))))
            assert int(g.argmax()) == c.argmax()
        print(f"  step errors max {max(step_err):.3g}, arg-max mismatches {mism} {gaps}")
        assert max(step_err) <= FLIP_TOL, step_err
        if kv != "f16" and ftype != "f16":
            assert float(np.median(tok_err0)) <= FLIP_TOL / 10, (errs, step_err, tok_err0)
        assert mism <= 1, (mism, gaps)
        if cfg in TIED_W896:
            assert mism == 0, gaps
        c.close(); m.close(); oc.close()
    finally:
        oq.set_fa_v_acc_f32(0)


def test_graph_and_eager_agree_bitwise(be, pkg, tmp_models):
    path = make(pkg, tmp_models, "tiny-w320", "q4_k_m")
    m = pkg.Model(path)
    outs = []
    for graphs in (True, False):
        c = pkg.Context(m, n_ctx=64, type_k=8, type_v=8, use_graphs=graphs)
        c.decode([1, 2, 3, 4, 5], np.arange(5))
        seq = []
        t = c.argmax()
        for s in range(8):
            c.decode([t], [5 + s])
            seq.append(c.logits().copy())
            t = c.argmax()
        outs.append(np.stack(seq))
        c.close()
    assert np.isfinite(outs[0]).all()
    assert (outs[0].view(np.uint32) == outs[1].view(np.uint32)).all()
    m.close()


# ------------------------------------------------------------------------------------------------ refusals
def _forge_tensor_type(path, name, new_type):
    """Overwrite the ggml type id in a 2-D tensor's record: name string, n_dims u32, two u64 extents, then the type."""
    blob = bytearray(open(path, "rb").read())
    k = name.encode()
    at = blob.find(struct.pack("<Q", len(k)) + k + struct.pack("<I", 2))
    assert at >= 0, name
    off = at + 8 + len(k) + 4 + 16
    blob[off:off + 4] = struct.pack("<I", new_type)
    open(path, "wb").write(bytes(blob))


def test_a_k_quant_tensor_with_a_896_long_row_is_refused_by_name(be, pkg, tmp_path):
    path = str(tmp_path / "m.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny-w896-2l", "q8_0", seed=3)
    m = pkg.Model(path); m.close()                                 # the untouched file loads
    _forge_tensor_type(path, "blk.1.attn_q.weight", pkg.gguf_synth.Q4_K)
    with pytest.raises(pkg.MI355Error) as ei:
        pkg.Model(path)
    msg = str(ei.value)
    assert "blk.1.attn_q.weight" in msg and "q4_K" in msg and "896" in msg, msg


def test_moe_and_bf16_files_at_such_a_width_are_refused_by_name(be, pkg, tmp_path):
    gs = pkg.gguf_synth
    moe = dataclasses.replace(gs.CONFIGS["tiny-moe"], name="tiny-moe-w320", n_embd=320, n_head=5, n_head_kv=1)
    path = str(tmp_path / "moe.gguf")
    gs.write_synthetic_llama(path, moe, "q8_0", seed=3)
    with pytest.raises(pkg.MI355Error, match="mixture-of-experts"):
        pkg.Model(path)
    path = str(tmp_path / "bf16.gguf")
    gs.write_synthetic_llama(path, "tiny-w320", "bf16", seed=3)
    with pytest.raises(pkg.MI355Error, match="bf16"):
        pkg.Model(path)
