"""TQ1_0 / TQ2_0 (ggml types 34 / 35) on the GPU: the mat-vec forms (generic, register ring, weight stream), the plane expansion of prompt batches, get_rows,
the launch plan, and whole files end to end - against the numpy restatement of tests/tq_ref.py (the CPU oracle has neither type)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_py as oq
import tq_ref as tq

pytestmark = pytest.mark.gpu

TYPES = [pytest.param(tq.TQ1_0, id="tq1_0"), pytest.param(tq.TQ2_0, id="tq2_0")]
FTYPE = {tq.TQ1_0: "tq1_0", tq.TQ2_0: "tq2_0"}
KV = {"f16": 1, "q8_0": 8}
FLIP_TOL = 3e-2          # the end-to-end tolerances of tests/test_gpu_model.py
TIGHT_TOL = 2e-5
GREEDY = dict(temperature=0.0, repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def make(pkg, tmp_models, cfg, ftype, seed, with_vocab=False):
    path = str(tmp_models / f"{cfg}-{ftype}-{seed}{'-v' if with_vocab else ''}.gguf")
    if not os.path.exists(path):
        pkg.gguf_synth.write_synthetic_llama(path, cfg, ftype, seed=seed, with_vocab=with_vocab)
    return path


def weights(pkg, rng, t, n, dscale=0.02):
    return pkg.gguf_synth.random_blocks(rng, t, n, dscale)


def _check_mul_mat(be, t, W, N, K, x, planes):
    T = x.shape[0]
    be.set_option("mmq_planes", planes)
    try:
        y, isum, msum = be.mul_mat(t, W, N, K, x, want_ints=True)
    finally:
        be.set_option("mmq_planes", 1)
    ref = tq.mul_mat(t, W, N, K, x)
    rb = tq.row_bytes(t, K)
    for tt in range(0, T, max(1, T // 5)):
        act = tq.quantize_act(x[tt])
        for r in range(0, N, max(1, N // 7)):
            assert (isum[tt, r] == tq.vec_dot_int_partials(t, W[r * rb:(r + 1) * rb], act, K)).all(), (tt, r)
            assert not msum[tt, r].any()
    assert np.abs(y - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-6


# ------------------------------------------------------------------------------------------------ op level
@pytest.mark.parametrize("planes", [1, 0])
@pytest.mark.parametrize("K", [256, 4096, 14336])
@pytest.mark.parametrize("T", [1, 2, 5, 31, 32, 200])
@pytest.mark.parametrize("t", TYPES)
def test_mul_mat_int_partials_exact_and_value(be, pkg, t, K, T, planes):
    """Integer per (token, row, super-block) exact against the restatement (sum (q - 1) a) and msum zero; the f32 result within 2e-5 of the output scale of the
    generic order.  T = 1: weight stream (K 4096, 14336) or register ring (K 256); 2 .. 31: the generic mat-vec; 32, 200: the plane kernels (planes 1) or the
    mat-vec (0)."""
    rng = np.random.default_rng(K + 7 * T + planes + t)
    N = 40 if K >= 14336 else 96
    _check_mul_mat(be, t, weights(pkg, rng, t, N * K), N, K, rng.standard_normal((T, K)).astype(np.float32), planes)


@pytest.mark.parametrize("T", [1, 5, 40])
@pytest.mark.parametrize("t", TYPES)
def test_mul_mat_arbitrary_bytes(be, pkg, t, T):
    """K = 256 with arbitrary code bytes - TQ2_0's code 3 (weight + 2 d), TQ1_0 bytes above 242 and bytes no trits encode: the formula still rules, on the
    ring (T 1), the generic mat-vec (5) and the plane expansion (40).  Every byte value occurs."""
    rng = np.random.default_rng(90 + t + T)
    N, K = 96, 256
    blk = np.zeros(N, tq.DT[t])
    qs = rng.integers(0, 256, blk["qs"].shape, dtype=np.uint8)
    qs.reshape(-1)[:256] = np.arange(256)
    blk["qs"] = qs
    if t == tq.TQ1_0:
        qh = rng.integers(0, 256, blk["qh"].shape, dtype=np.uint8)
        qh.reshape(-1)[:256] = np.arange(255, -1, -1)
        blk["qh"] = qh
    blk["d"] = rng.uniform(0.01, 0.03, N).astype(np.float16)
    W = blk.view(np.uint8).reshape(-1)
    d, q = tq.decode(t, W, N * K)
    assert q.max() == (3 if t == tq.TQ2_0 else 2) and len(np.unique(blk["qs"])) == 256
    _check_mul_mat(be, t, W, N, K, rng.standard_normal((T, K)).astype(np.float32), 1)


@pytest.mark.parametrize("K,N", [(4096, 1024), (4096, 14336), (14336, 4096), (2048, 768)])
@pytest.mark.parametrize("t", TYPES)
def test_single_token_ring_stream_and_generic_agree(be, pkg, t, K, N):
    """One token at the shapes of a Llama-3-8B layer: the weight stream (where it has a form) and the register ring give the same bits - one lane role, one
    arithmetic - and both are the restatement within the f32 bound."""
    rng = np.random.default_rng(K + N + t)
    W = weights(pkg, rng, t, N * K)
    x = rng.standard_normal((1, K)).astype(np.float32)
    ys = {}
    for stream in (1, 0):
        be.set_option("mmvq_stream", stream)
        try:
            ys[stream] = be.mul_mat(t, W, N, K, x)
        finally:
            be.set_option("mmvq_stream", 1)
    ref = tq.mul_mat(t, W, N, K, x)
    assert np.array_equal(ys[1].view(np.uint32), ys[0].view(np.uint32)), float(np.abs(ys[1] - ys[0]).max())
    assert np.abs(ys[1] - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-6


@pytest.mark.parametrize("K,N,T", [(1024, 64, 40), (256, 32, 257)])
@pytest.mark.parametrize("t", TYPES)
def test_ffn_gate_up_swiglu_launch(be, pkg, t, K, N, T):
    rng = np.random.default_rng(3 * K + N + T + t)
    Wg, Wu = weights(pkg, rng, t, N * K), weights(pkg, rng, t, N * K)
    x = (rng.standard_normal((T, K)) * rng.uniform(0.1, 2.0, (T, 1))).astype(np.float32)
    be.set_option("mmq_tiles", 4)
    try:
        y = be.ffn_gate_up(t, Wg, Wu, N, K, x)
    finally:
        be.set_option("mmq_tiles", 0)
    g, u = tq.mul_mat(t, Wg, N, K, x), tq.mul_mat(t, Wu, N, K, x)
    with np.errstate(over="ignore"):
        ref = (g / (1.0 + np.exp(-g.astype(np.float64)))).astype(np.float32) * u
    # (two products of the 2e-5 bound and the sigmoid's slope: the bound tests/test_gpu_iq4xs.py derives for this launch)
    assert np.abs(y - ref).max() <= 4e-5 * np.abs(ref).max() + 1e-6


@pytest.mark.parametrize("K", [256, 512])
@pytest.mark.parametrize("t", TYPES)
def test_get_rows_bit_exact(be, pkg, t, K):
    """Rows holding every byte value, under positive and negative d: bit for bit the restatement's product, - 0.0 included."""
    rng = np.random.default_rng(23 + t + K)
    R = 12
    blk = np.zeros(R * K // 256, tq.DT[t])
    qs = rng.integers(0, 256, blk["qs"].shape, dtype=np.uint8)
    qs.reshape(-1)[:256] = np.arange(256)
    blk["qs"] = qs
    if t == tq.TQ1_0:
        qh = rng.integers(0, 256, blk["qh"].shape, dtype=np.uint8)
        qh.reshape(-1)[-48:] = np.arange(208, 256)                          # (with qs: every byte value in a qh position too is more than 48 slots hold)
        blk["qh"] = qh
    blk["d"] = (rng.uniform(0.5, 1.5, blk.shape[0]) * np.where(np.arange(blk.shape[0]) % 2, -1.0, 1.0)).astype(np.float16)
    table = blk.view(np.uint8).reshape(-1)
    ids = np.array([0, R - 1, 7, 7, 3], np.int32)                              # (row 0 holds the byte ramp; odd blocks have d < 0)
    got = be.get_rows(t, table, K, R, ids)
    rb = tq.row_bytes(t, K)
    neg_zero = 0
    for i, r in enumerate(ids):
        want = tq.dequantize(t, table[r * rb:(r + 1) * rb], K)
        assert got[i].view(np.uint32).tolist() == want.view(np.uint32).tolist(), r
        neg_zero += int((want.view(np.uint32) == 0x80000000).sum())
    assert neg_zero > 0


@pytest.mark.parametrize("t", TYPES)
def test_qkv_attn_plan_is_not_fused_for_ternary_tensors(pkg, t):
    """Llama-3-8B geometry with a ternary Q | K | V (and attn_output): the one-launch attention block answers "separate launches"; Q4_K_M's layer takes it."""
    lib = pkg.load_library()

    def plan(tq_, tk, tv, to):
        slots = C.c_int32(0)
        return int(lib.mi355_debug_qkv_attn_plan(tq_, tk, tv, to, 4096, 32, 8, 128, 8, 576, C.byref(slots)))

    assert plan(12, 12, 13, 12) > 0
    assert plan(t, t, t, t) == 0 and plan(t, t, t, 12) == 0


# ------------------------------------------------------------------------------------------------ model level
def _check_run(pkg, c, m, ref, n_prompt, kv, tight, steps=8, forced=False):
    rng = np.random.default_rng(5)
    prompt = rng.integers(0, m.n_vocab, n_prompt)

    def run(toks, pos):
        r = ref.decode(toks, pos)
        if forced:
            c.force_moe_ids(ref.routes[-1])
        assert c.decode(toks, pos) == 0
        return r[0]

    c.enable_taps(True)
    r = run(prompt, np.arange(n_prompt))
    errs = [rel_err(c.layer_out(il, n_prompt).reshape(n_prompt, -1), ref.layer_out(il, n_prompt)) for il in range(m.n_layer)]
    a0, b0 = c.layer_out(0, n_prompt).reshape(n_prompt, -1), ref.layer_out(0, n_prompt)
    tok_err0 = np.abs(a0 - b0).max(axis=1) / max(1.0, float(np.abs(b0).max()))
    errs.append(rel_err(c.logits(), r))
    print("layer / logit errors", errs, "median first-layer token error", float(np.median(tok_err0)))
    assert max(errs) <= FLIP_TOL, errs
    c.enable_taps(False)
    tok, mism, step_err = int(r.argmax()), 0, []
    for step in range(steps):
        r = run([tok], [n_prompt + step])
        step_err.append(rel_err(c.logits(), r))
        tok = int(r.argmax())
        if c.argmax() != tok:
            top2 = np.sort(r)[-2:]
            assert top2[1] - top2[0] <= 2 * FLIP_TOL * max(1.0, np.abs(r).max()), (step, top2)
            mism += 1
    print("step errors", step_err, "flips", mism)
    assert max(step_err) <= FLIP_TOL, step_err
    assert mism <= 1, (mism, step_err)
    if tight and kv != "f16":
        assert float(np.median(tok_err0)) <= TIGHT_TOL, (errs, tok_err0)


# (config, cache, prompt tokens) -> the file seed.  Chosen on the CPU: the first seed from 11 on at which the restatement's own top-two logit gap is above
# 2 * FLIP_TOL * max(1, max |logit|) at every compared single-token step, so that the one-flip allowance of _check_run stays a cap that the case does not
# need; where no seed up to 40 managed that, the seed with the widest smallest gap (its multiple of the bar is noted).  One seed serves both types: the writer
# draws the same trits and scales for a tq1_0 and a tq2_0 file of one seed, so the two files hold the same weights and the restatement the same logits.
SEEDS = {
    ("tiny-gqa4", "q8_0", 21): 29,      # smallest gap 1.54 x the bar
    ("tiny-gqa4", "f16", 40): 28,       # 0.56 x: no seed up to 40 clears every step
    ("tiny-gqa4", "q8_0", 130): 28,     # 0.82 x: likewise
    ("tiny-d128", "q8_0", 40): 40,      # 0.95 x: likewise
    ("tiny-8b-2l", "q8_0", 21): 17,     # 1.46 x (seeds 11 .. 18 tried, four steps)
    ("tiny-qwen3", "f16", 21): 11,      # 9.5 x
}
MOE_SEEDS = {("q8_0", 40): 25, ("f16", 130): 29}      # 1.81 x and 1.03 x (six steps)
BATCHED_SEED = 11                        # (no greedy comparison in that test)


@pytest.mark.parametrize("cfg,kv,n_prompt", list(SEEDS))
@pytest.mark.parametrize("t", TYPES)
def test_ternary_layers_logits_and_greedy_ids(be, pkg, tmp_models, t, cfg, kv, n_prompt):
    """A prompt (21 tokens: the generic mat-vec; 40, 130: the plane kernels), then single-token steps (ring / stream) teacher-forced with the reference's
    tokens: per layer, logits and greedy ids."""
    path = make(pkg, tmp_models, cfg, FTYPE[t], SEEDS[(cfg, kv, n_prompt)])
    oq.set_fa_v_acc_f32(1 if kv == "f16" else 0)
    try:
        m = pkg.Model(path)
        c = pkg.Context(m, n_ctx=512, n_batch=512, n_ubatch=512, type_k=KV[kv], type_v=KV[kv])
        ref = tq.TqRef(path, 512, KV[kv], KV[kv])
        # tight (median of the first layer's tokens within f32 round-off) where the contractions are short; not at Llama-3-8B's widths, for the reason
        # tests/test_gpu_iq4xs.py gives: the device's f32 order over a row differs from the generic one, and at 4096 / 14336 columns that 1e-7 flips a
        # Q8_K code of the next activation in most tokens
        _check_run(pkg, c, m, ref, n_prompt, kv, tight=cfg != "tiny-8b-2l", steps=4 if cfg == "tiny-8b-2l" else 8)
        c.close(); m.close()
    finally:
        oq.set_fa_v_acc_f32(0)


@pytest.mark.parametrize("kv,n_prompt", list(MOE_SEEDS))
@pytest.mark.parametrize("t", TYPES)
def test_ternary_qwen3moe_forced_routing(be, pkg, tmp_models, t, kv, n_prompt):
    """tiny-qwen3moe with ternary experts and the reference's expert selections handed over: 40 / 130 tokens go through the grouped-expert plane kernels, the
    single-token steps through the expert mat-vec."""
    path = make(pkg, tmp_models, "tiny-qwen3moe", FTYPE[t], MOE_SEEDS[(kv, n_prompt)])
    oq.set_fa_v_acc_f32(1 if kv == "f16" else 0)
    try:
        m = pkg.Model(path)
        c = pkg.Context(m, n_ctx=256, type_k=KV[kv], type_v=KV[kv])
        ref = tq.TqMoeRef(path, 256, KV[kv], KV[kv])
        _check_run(pkg, c, m, ref, n_prompt, kv, tight=False, steps=6, forced=True)
        c.close(); m.close()
    finally:
        oq.set_fa_v_acc_f32(0)


@pytest.mark.parametrize("t", TYPES)
def test_ternary_batched_steps(be, pkg, tmp_models, t):
    """Three sequences at different positions advance together (3-token steps: the generic mat-vec), against the reference sequence by sequence."""
    path = make(pkg, tmp_models, "tiny-gqa4", FTYPE[t], BATCHED_SEED)
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=512, n_seq_max=4, type_k=8, type_v=8)
    refs = [tq.TqRef(path, 512, 8, 8) for _ in range(3)]
    rng = np.random.default_rng(17)
    lens = [40, 9, 33]
    nxt = []
    for sq, n in enumerate(lens):
        p = rng.integers(0, m.n_vocab, n)
        r = refs[sq].decode(p, np.arange(n))[0]
        assert c.decode(p, np.arange(n), [sq] * n) == 0
        nxt.append(int(r.argmax()))
    for step in range(4):
        toks, pos = nxt, [lens[s] + step for s in range(3)]
        assert c.decode(toks, pos, [0, 1, 2], [1, 1, 1]) == 0
        got = [c.logits(i) for i in range(3)]
        for s in range(3):
            r = refs[s].decode([toks[s]], [pos[s]])[0]
            assert rel_err(got[s], r) <= FLIP_TOL, (step, s)
            nxt[s] = int(r.argmax())
    c.close(); m.close()


# ------------------------------------------------------------------------------------------------ engine level
def _greedy_ref(path, pkg, prompt: str, n_predict: int):
    m = pkg.Model(path)
    toks = m.tokenize(prompt, add_special=True, parse_special=True)
    eos = m.lib.mi355_token_eos(m.h)
    ref = tq.TqRef(path, 256, 8, 8)
    r = ref.decode(toks, np.arange(len(toks)))[0]
    out, pos = b"", len(toks)
    for _ in range(n_predict + 1):                      # (as tests/test_gpu_qwen3.py's _greedy: the engine's count of max_tokens)
        t = int(r.argmax())
        if t == eos:
            break
        out += m.token_to_piece(t)
        r = ref.decode([t], [pos])[0]
        pos += 1
    m.close()
    return out.decode("utf-8", errors="replace")


@pytest.mark.parametrize("t", TYPES)
def test_ternary_engine_chat_and_row_split_refused(pkg, tmp_models, t):
    """/v1/chat/completions on a ternary file returns the reference's greedy tokens; a row split of the file is refused with an error naming the type."""
    name_t = FTYPE[t]
    path = make(pkg, tmp_models, "tiny-gqa4", name_t, 3, with_vocab=True)
    e = pkg.Engine()
    try:
        st, body = e.load_model(llama_model_path=path, ctx_len=256, n_parallel=1, ngl=100, user_prompt="u:", ai_prompt="a:", system_prompt="s:")
        assert st["status_code"] == 200 and not st["has_error"], (st, body)
        msgs = [{"role": "system", "content": "be brief"}, {"role": "user", "content": "hello world"}]
        name = os.path.splitext(os.path.basename(path))[0]                      # (the engine names a model after its file)
        st, body = e.chat_completion(model=name, messages=msgs, max_tokens=8, **GREEDY)[-1]
        assert st["status_code"] == 200 and not st["has_error"], (st, body)
        content = body["choices"][0]["message"]["content"]
        want = _greedy_ref(path, pkg, "s:be briefu:hello worlda:", 8)
        if "u:" not in want:
            assert content in (want.lstrip(" "), want), (content, want)
        e.unload_model(model=name)
        st, body = e.load_model(llama_model_path=path, ctx_len=128, split_mode="row", split_ranks=2)
        assert st["status_code"] != 200 and name_t in str(body), (st, body)
    finally:
        e.close()
    with pytest.raises(pkg.binding.MI355Error, match=name_t):
        pkg.Model(path, tp_rank=0, tp_size=2)
