"""MXFP4 (ggml type 39) on the GPU: the mat-vec forms (generic, tiled, register ring, weight stream), the E8 form of the Q8_0 matrix-core prompt kernel and its
grouped-expert launch, get_rows, and whole files end to end - against the numpy restatement of tests/mxfp4_ref.py (the CPU oracle does not have the type)."""
import os

import numpy as np
import pytest

import mxfp4_ref as xr
import oracle_py as oq

pytestmark = pytest.mark.gpu

MXFP4 = xr.MXFP4
KV = {"f16": 1, "q8_0": 8}
FLIP_TOL = 3e-2          # the end-to-end tolerances of tests/test_gpu_model.py and tests/test_gpu_q41_q51.py
TIGHT_TOL = 2e-5
GREEDY = dict(temperature=0.0, repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def make(pkg, tmp_models, cfg, ftype, seed=11, with_vocab=True):
    path = str(tmp_models / f"{cfg}-{ftype}-{seed}.gguf")
    if not os.path.exists(path):
        pkg.gguf_synth.write_synthetic_llama(path, cfg, ftype, seed=seed, with_vocab=with_vocab)
    return path


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ op level
@pytest.mark.parametrize("planes", [1, 0])
@pytest.mark.parametrize("T", [1, 2, 5, 31, 32, 33, 64, 129])
@pytest.mark.parametrize("K", [32, 96, 2080, 4096])
def test_mul_mat_int_partials_exact_and_value(be, pkg, K, T, planes):
    """isum (sum level * a) per (token, row, block) exact against the restatement (msum is 0: the format has no minimum); the f32 result within TIGHT_TOL of
    the output scale of the block-order restatement.  K 32: one block; 96: an odd block count against the two-lanes-per-block role; 2080: one Q80_KC chunk of
    the prompt kernel plus one block, a tail that is no multiple of its unroll of 4.  T 1: the generic mat-vec (K 4096: quantised in the prologue of the weight
    stream or the register ring); 2 .. 31: the generic and the tiled mat-vec; from 32 on: the matrix cores through the Q8_0-layout copy (planes 1; bit for bit
    the restatement, each output's chain in block order) or the mat-vec again (planes 0)."""
    for N in (33, 128):
        rng = np.random.default_rng(K + 7 * T + planes + N)
        W = pkg.gguf_synth.random_blocks(rng, MXFP4, N * K, 0.05)
        x = (rng.standard_normal((T, K)) * rng.uniform(0.2, 2.0, (T, 1))).astype(np.float32)
        be.set_option("mmq_planes", planes)
        try:
            y, isum, msum = be.mul_mat(MXFP4, W, N, K, x, want_ints=True)
        finally:
            be.set_option("mmq_planes", 1)
        ref = xr.mul_mat(W, N, K, x)
        lv = xr.decode(W, N * K)[1].reshape(N, K // 32, 32).astype(np.int64)
        codes = np.stack([xr.quantize_act(r)[0] for r in x]).astype(np.int64)            # [T][nb][32]
        assert np.array_equal(isum, np.einsum("nbk,tbk->tnb", lv, codes)), N
        assert not msum.any()
        rb = xr.row_bytes(K)
        assert (isum[T - 1, N - 1] == xr.vec_dot_int_partials(W[(N - 1) * rb:N * rb], codes[T - 1], K)).all()
        scale = np.abs(ref).max()
        e_ref = np.abs(y - ref).max()
        print(f"K={K} T={T} planes={planes} N={N}: |y-ref|/scale={e_ref / scale:.3g}")
        assert e_ref <= TIGHT_TOL * scale + 1e-6
        if planes and T >= 32:
            assert np.array_equal(bits(y), bits(ref)), (N, float(np.abs(y - ref).max()))


def _forms_are_one_result(be, W, N, K, x, resid):
    ref = xr.mul_mat(W, N, K, x)
    assert np.isfinite(ref).all()
    try:
        for mt in (1, 2, 4):
            be.set_option("mmq_q80_tiles", mt)
            y = be.mul_mat(MXFP4, W, N, K, x)
            ya = be.mul_mat_add(MXFP4, W, N, K, x, resid)
            assert np.array_equal(bits(y), bits(ref)), (mt, float(np.abs(y - ref).max()))
            assert np.array_equal(bits(ya), bits((resid + ref).astype(np.float32))), mt
    finally:
        be.set_option("mmq_q80_tiles", 0)


@pytest.mark.parametrize("K,N,T", [(2080, 200, 129), (4096, 128, 256), (96, 33, 64)])
def test_prompt_kernel_forms_are_bitwise_one_result(be, pkg, K, N, T):
    """The MT = 1 / 2 / 4 forms of the prompt kernel (token tiles per wave) give the restatement's bits, with and without a residual in the epilogue
    (y = resid + sum: one more f32 add per output)."""
    rng = np.random.default_rng(K + N + T)
    W = pkg.gguf_synth.random_blocks(rng, MXFP4, N * K, 0.05)
    x = (rng.standard_normal((T, K)) * rng.uniform(0.2, 2.0, (T, 1))).astype(np.float32)
    _forms_are_one_result(be, W, N, K, x, rng.standard_normal((T, N)).astype(np.float32))


def test_prompt_kernel_scale_range(be, pkg):
    """Block scales e spread over 90 .. 160 (d from 2^-38 to 2^32: far outside what an f16 scale plane holds, 104 <= e <= 143), the activations scaled down so
    that nothing overflows (|sum| < 4096 * 12 * 127 * 2^32 * 2^-8 / 127): the copy's scale plane must be exact for every e."""
    K, N, T = 4096, 128, 129
    rng = np.random.default_rng(39)
    W = pkg.gguf_synth.random_blocks(rng, MXFP4, N * K, 0.05)
    b = W.view(pkg.gguf_synth.DT_MXFP4)
    b["e"] = rng.integers(90, 161, size=b.size).astype(np.uint8)
    b["e"][:71] = np.arange(90, 161)                                  # every value at least once
    x = (rng.standard_normal((T, K)) * 2.0 ** -8).astype(np.float32)
    resid = (rng.standard_normal((T, N)) * 2.0 ** 20).astype(np.float32)
    _forms_are_one_result(be, W, N, K, x, resid)
    be.set_option("mmq_planes", 0)                                    # and the mat-vec on the format's own rows
    try:
        y = be.mul_mat(MXFP4, W, N, K, x[:5])
    finally:
        be.set_option("mmq_planes", 1)
    ref = xr.mul_mat(W, N, K, x[:5])
    assert np.abs(y - ref).max() <= TIGHT_TOL * np.abs(ref).max()


@pytest.mark.parametrize("K,N", [(4096, 1024), (2048, 768), (1024, 33)])
def test_single_token_ring_and_stream(be, pkg, K, N):
    """One token, quantised in the mat-vec's prologue as a decode step's ffn_down and head are: the weight stream (stream 1: row pairs, where it has a form
    for the shape) and the register ring (0) against the restatement - and against each other bit for bit, as for every other type."""
    rng = np.random.default_rng(K + N)
    W = pkg.gguf_synth.random_blocks(rng, MXFP4, N * K, 0.05)
    x = rng.standard_normal((1, K)).astype(np.float32)
    ys = {}
    for stream in (1, 0):
        be.set_option("mmvq_stream", stream)
        try:
            ys[stream] = be.mul_mat(MXFP4, W, N, K, x)
        finally:
            be.set_option("mmvq_stream", 1)
    ref = xr.mul_mat(W, N, K, x)
    scale = np.abs(ref).max()
    for stream, y in ys.items():
        assert np.abs(y - ref).max() <= TIGHT_TOL * scale + 1e-6, stream
    assert np.array_equal(bits(ys[1]), bits(ys[0]))


@pytest.mark.parametrize("planes", [1, 0])
@pytest.mark.parametrize("K,N,T", [(1024, 64, 40), (256, 32, 257)])
def test_ffn_gate_up_swiglu(be, pkg, K, N, T, planes):
    """ffn_gate | ffn_up with SwiGLU as a layer runs them: the two prompt-kernel launches and the SwiGLU pass (planes 1), or the mat-vec with SwiGLU in its
    epilogue (0; chunks of 16, 8, .. tokens).  Twice the single product's tolerance: the error of g passes through silu's slope (at most 1.1) times u."""
    rng = np.random.default_rng(3 * K + N + T)
    Wg, Wu = (pkg.gguf_synth.random_blocks(rng, MXFP4, N * K, 0.05) for _ in range(2))
    x = (rng.standard_normal((T, K)) * rng.uniform(0.1, 2.0, (T, 1))).astype(np.float32)
    be.set_option("mmq_planes", planes)
    try:
        y = be.ffn_gate_up(MXFP4, Wg, Wu, N, K, x)
    finally:
        be.set_option("mmq_planes", 1)
    g, u = xr.mul_mat(Wg, N, K, x), xr.mul_mat(Wu, N, K, x)
    with np.errstate(over="ignore"):
        ref = (g / (1.0 + np.exp(-g.astype(np.float64)))).astype(np.float32) * u
    assert np.abs(y - ref).max() <= 2 * TIGHT_TOL * np.abs(ref).max() + 1e-6


def test_get_rows_bit_exact(be, pkg):
    """Rows whose blocks carry e = 2 (the smallest normal scale), 103 | 104 and 143 | 144 (either side of what an f16 would hold), 254 (level * 2^126: the larger
    levels overflow to the infinity of their sign, as the one f32 product does) and the writer's own band."""
    rng = np.random.default_rng(23)
    K, R = 1024, 40
    table = pkg.gguf_synth.random_blocks(rng, MXFP4, R * K, 1.0)
    b = table.view(pkg.gguf_synth.DT_MXFP4).reshape(R, K // 32)
    special = {3: 2, 5: 103, 6: 104, 8: 143, 9: 144, 11: 254}
    for r, e in special.items():
        b[r]["e"] = e
    b[12]["e"] = np.resize(np.array([2, 103, 104, 143, 144, 254], np.uint8), K // 32)
    ids = np.array([0, 39, 7, 7, 21, 12] + list(special), np.int32)
    got = be.get_rows(MXFP4, table, K, R, ids)
    rb = xr.row_bytes(K)
    for i, r in enumerate(ids):
        want = xr.dequantize(table[r * rb:(r + 1) * rb], K)
        assert not np.isnan(want).any()
        assert got[i].view(np.uint32).tolist() == want.view(np.uint32).tolist(), r


# ------------------------------------------------------------------------------------------------ model level
def _check_run(pkg, c, m, ref, n_prompt, kv, tight, steps=8, forced=False):
    """The method and bounds of tests/test_gpu_q41_q51.py: a prompt, then teacher-forced single-token steps; per layer, logits and greedy ids."""
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
    print(f"n_prompt={n_prompt} kv={kv}: layer / logit errors {errs}, first layer median {float(np.median(tok_err0)):.3g}")
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
    assert max(step_err) <= FLIP_TOL, step_err
    assert mism <= 1, (mism, step_err)
    if tight and kv != "f16":
        assert float(np.median(tok_err0)) <= TIGHT_TOL, (errs, tok_err0)


@pytest.mark.parametrize("cfg,kv,n_prompt", [("tiny-gqa4", "q8_0", 21), ("tiny-gqa4", "f16", 40), ("tiny-d128", "q8_0", 40), ("tiny-d128", "f16", 21)])
def test_layers_logits_and_greedy_ids(be, pkg, tmp_models, cfg, kv, n_prompt):
    """An mxfp4 file (every 2-D weight MXFP4, token_embd included; an F16 head): a prompt (21 tokens: the generic and tiled mat-vec; 40: the matrix cores
    through the Q8_0-layout copies), then single-token steps (ring / stream) teacher-forced with the reference's tokens: per layer, logits and greedy ids;
    the first layer within f32 round-off for most tokens."""
    path = make(pkg, tmp_models, cfg, "mxfp4", with_vocab=False)
    oq.set_fa_v_acc_f32(1 if kv == "f16" else 0)
    try:
        m = pkg.Model(path)
        c = pkg.Context(m, n_ctx=1024, n_batch=512, n_ubatch=512, type_k=KV[kv], type_v=KV[kv])
        ref = xr.Mxfp4Ref(path, 1024, KV[kv], KV[kv])
        _check_run(pkg, c, m, ref, n_prompt, kv, tight=True)
        c.close(); m.close()
    finally:
        oq.set_fa_v_acc_f32(0)


@pytest.mark.parametrize("kv,n_prompt", [("q8_0", 40), ("f16", 21)])
def test_qwen3moe_forced_routing(be, pkg, tmp_models, kv, n_prompt):
    """tiny-qwen3moe as an MXFP4_MOE file (MXFP4 experts, everything else Q8_0), the reference's expert selections handed over: a prompt of 40 tokens (the
    grouped-expert launch) or 21 (a launch per expert), then 6 single-token steps (the selected-experts weight stream)."""
    path = make(pkg, tmp_models, "tiny-qwen3moe", "mxfp4_moe", with_vocab=False)
    oq.set_fa_v_acc_f32(1 if kv == "f16" else 0)
    try:
        m = pkg.Model(path)
        c = pkg.Context(m, n_ctx=256, type_k=KV[kv], type_v=KV[kv])
        ref = xr.Mxfp4MoeRef(path, 256, KV[kv], KV[kv])
        _check_run(pkg, c, m, ref, n_prompt, kv, tight=False, steps=6, forced=True)
        c.close(); m.close()
    finally:
        oq.set_fa_v_acc_f32(0)


def test_grouped_launch_against_per_expert_launches(be, pkg, tmp_models):
    """64 tokens with the expert ids forced so that layer 1's batches are of 192 rows (expert 5, three ranks of every token: more than a 128-token tile), 33
    (expert 9), 32 (expert 7), 1 (expert 11), a spread of small ones, and none at all for most experts: every layer's output with the "moe_q80_grouped"
    switch on (one launch for all experts) is bit for bit the output with it off (a launch per expert, the same kernel body)."""
    path = make(pkg, tmp_models, "tiny-qwen3moe", "mxfp4_moe", with_vocab=False)
    m = pkg.Model(path)
    T, KU, NE = 64, 8, 128
    rng = np.random.default_rng(64)
    ids = np.stack([np.stack([rng.permutation(NE)[:KU] for _ in range(T)]) for _ in range(m.n_layer)]).astype(np.int32)
    L1 = ids[1]
    L1[:, 0:3] = 5
    L1[:32, 3], L1[32:, 3] = 7, 9
    L1[:, 4] = 20 + np.arange(T) % 50
    L1[0, 4], L1[1, 4] = 9, 11
    L1[:, 5:] = 70 + (np.arange(T)[:, None] * 3 + np.arange(3)[None, :]) % 58
    counts = np.bincount(L1.reshape(-1), minlength=NE)
    assert counts[5] == 192 and counts[9] == 33 and counts[7] == 32 and counts[11] == 1 and (counts == 0).sum() >= 4 and counts.sum() == T * KU
    toks = rng.integers(0, m.n_vocab, T)
    taps = {}
    try:
        for on in (1, 0):
            be.set_option("moe_q80_grouped", on)
            c = pkg.Context(m, n_ctx=256, type_k=8, type_v=8)
            c.enable_taps(True)
            c.force_moe_ids(ids)
            assert c.decode(toks, np.arange(T)) == 0
            taps[on] = [c.layer_out(il, T).copy() for il in range(m.n_layer)] + [c.logits().copy()]
            c.close()
    finally:
        be.set_option("moe_q80_grouped", 1)
    m.close()
    for il, (a, b) in enumerate(zip(taps[1], taps[0])):
        assert np.isfinite(a).all() and np.abs(a).max() > 0
        assert np.array_equal(bits(a), bits(b)), (il, float(np.abs(a - b).max()))


def test_batched_steps(be, pkg, tmp_models):
    """Five sequences at different positions; steps of 2, 3, 4 and 5 tokens advance the first 2 .. 5 of them together, against the reference sequence by
    sequence (as tests/test_gpu_q41_q51.py's test_batched_steps)."""
    path = make(pkg, tmp_models, "tiny-gqa4", "mxfp4", with_vocab=False)
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=512, n_seq_max=8, type_k=8, type_v=8)
    refs = [xr.Mxfp4Ref(path, 512, 8, 8) for _ in range(5)]
    rng = np.random.default_rng(17)
    lens = [40, 9, 33, 5, 12]
    nxt = []
    for sq, n in enumerate(lens):
        p = rng.integers(0, m.n_vocab, n)
        r = refs[sq].decode(p, np.arange(n))[0]
        assert c.decode(p, np.arange(n), [sq] * n) == 0
        nxt.append(int(r.argmax()))
    pos = list(lens)
    for n in (2, 3, 4, 5):
        assert c.decode(nxt[:n], pos[:n], list(range(n)), [1] * n) == 0
        got = [c.logits(i) for i in range(n)]
        for s in range(n):
            r = refs[s].decode([nxt[s]], [pos[s]])[0]
            assert rel_err(got[s], r) <= FLIP_TOL, (n, s)
            nxt[s] = int(r.argmax())
            pos[s] += 1
    c.close(); m.close()


# ------------------------------------------------------------------------------------------------ engine level
def _greedy_ref(path, pkg, prompt: str, n_predict: int):
    m = pkg.Model(path)
    toks = m.tokenize(prompt, add_special=True, parse_special=True)
    eos = m.lib.mi355_token_eos(m.h)
    ref = xr.Mxfp4Ref(path, 256, KV["f16"], KV["f16"])          # the engine's cache type where the request names none: f16
    r = ref.decode(toks, np.arange(len(toks)))[0]
    out, pos = b"", len(toks)
    for _ in range(n_predict + 1):                      # (as tests/test_gpu_q41_q51.py's _greedy_ref: the engine's count of max_tokens)
        t = int(r.argmax())
        if t == eos:
            break
        out += m.token_to_piece(t)
        r = ref.decode([t], [pos])[0]
        pos += 1
    m.close()
    return out.decode("utf-8", errors="replace")


def test_engine_chat_and_row_split_refused(pkg, tmp_models):
    """/v1/chat/completions on an mxfp4 file returns the reference's greedy tokens; a row split of the file is refused with an error naming mxfp4."""
    path = make(pkg, tmp_models, "tiny-gqa4", "mxfp4", seed=3)
    e = pkg.Engine()
    try:
        st, body = e.load_model(llama_model_path=path, ctx_len=256, n_parallel=1, ngl=100, user_prompt="u:", ai_prompt="a:", system_prompt="s:")
        assert st["status_code"] == 200 and not st["has_error"], (st, body)
        msgs = [{"role": "system", "content": "be brief"}, {"role": "user", "content": "hello world"}]
        name = os.path.splitext(os.path.basename(path))[0]                      # (the engine names a model after its file)
        st, body = e.chat_completion(model=name, messages=msgs, max_tokens=8, **GREEDY)[-1]
        assert st["status_code"] == 200 and not st["has_error"], (st, body)
        content = body["choices"][0]["message"]["content"]
        oq.set_fa_v_acc_f32(1)                                                  # (as the f16-cache cases above)
        try:
            want = _greedy_ref(path, pkg, "s:be briefu:hello worlda:", 8)
        finally:
            oq.set_fa_v_acc_f32(0)
        want = want.split("u:")[0]                                              # (the stop string never leaves the engine: the text before it)
        assert content in (want.lstrip(" "), want), (content, want)
        e.unload_model(model=name)
        st, body = e.load_model(llama_model_path=path, ctx_len=128, split_mode="row", split_ranks=2)
        assert st["status_code"] != 200 and "mxfp4" in str(body), (st, body)
    finally:
        e.close()
    with pytest.raises(pkg.binding.MI355Error, match="mxfp4"):
        pkg.Model(path, tp_rank=0, tp_size=2)
