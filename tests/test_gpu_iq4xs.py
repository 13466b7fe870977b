"""IQ4_XS (ggml type 23) on the GPU: the mat-vec forms (generic, register ring, weight stream), the plane expansion of prompt batches, get_rows, the
one-launch attention block, and whole files end to end - against the numpy restatement of tests/iq4xs_ref.py (the CPU oracle has no IQ4_XS)."""
import ctypes as C
import os

import numpy as np
import pytest

import iq4xs_ref as ix
import oracle_py as oq

pytestmark = pytest.mark.gpu

IQ4_XS = ix.IQ4_XS
KV = {"f16": 1, "q8_0": 8, "q4_0": 2}
FLIP_TOL = 3e-2          # the end-to-end tolerances of tests/test_gpu_model.py
TIGHT_TOL = 2e-5
GREEDY = dict(temperature=0.0, repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def make(pkg, tmp_models, cfg, ftype="iq4_xs", seed=11, with_vocab=True):
    path = str(tmp_models / f"{cfg}-{ftype}-{seed}.gguf")
    if not os.path.exists(path):
        pkg.gguf_synth.write_synthetic_llama(path, cfg, ftype, seed=seed, with_vocab=with_vocab)
    return path


def weights(pkg, rng, n, dscale=0.02):
    return pkg.gguf_synth.random_blocks(rng, IQ4_XS, n, dscale)


# ------------------------------------------------------------------------------------------------ op level
@pytest.mark.parametrize("planes", [1, 0])
@pytest.mark.parametrize("K", [256, 4096, 14336])
@pytest.mark.parametrize("T", [1, 2, 5, 31, 32, 200])
def test_mul_mat_int_partials_exact_and_value(be, pkg, K, T, planes):
    """Integer partial per (token, row, super-block) exact against the restatement; the f32 result within 2e-5 of the output scale of the generic order.
    T = 1: weight stream (K 4096, 14336) or register ring (K 256); 2 .. 31: the generic mat-vec; 32, 200: the plane kernels (planes 1) or the mat-vec (0)."""
    rng = np.random.default_rng(K + 7 * T + planes)
    N = 40 if K >= 14336 else 96
    W = weights(pkg, rng, N * K)
    x = rng.standard_normal((T, K)).astype(np.float32)
    be.set_option("mmq_planes", planes)
    try:
        y, isum, msum = be.mul_mat(IQ4_XS, W, N, K, x, want_ints=True)
    finally:
        be.set_option("mmq_planes", 1)
    ref = ix.mul_mat(W, N, K, x)
    rb = ix.row_bytes(K)
    for tt in range(0, T, max(1, T // 5)):
        act = ix.quantize_act(x[tt])
        for r in range(0, N, max(1, N // 7)):
            assert (isum[tt, r] == ix.vec_dot_int_partials(W[r * rb:(r + 1) * rb], act, K)).all(), (tt, r)
            assert not msum[tt, r].any()
    assert np.abs(y - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-6


@pytest.mark.parametrize("stream", [1, 0])
@pytest.mark.parametrize("K,N", [(4096, 1024), (4096, 14336), (14336, 4096), (2048, 768)])
def test_single_token_ring_and_stream(be, pkg, K, N, stream):
    """One token at the shapes of a Llama-3-8B layer: the weight stream (stream 1, where it has a form) and the register ring (0) against the restatement."""
    rng = np.random.default_rng(K + N + stream)
    W = weights(pkg, rng, N * K)
    x = rng.standard_normal((1, K)).astype(np.float32)
    be.set_option("mmvq_stream", stream)
    try:
        y = be.mul_mat(IQ4_XS, W, N, K, x)
    finally:
        be.set_option("mmvq_stream", 1)
    ref = ix.mul_mat(W, N, K, x)
    assert np.abs(y - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-6


@pytest.mark.parametrize("K,N,T", [(1024, 64, 40), (4096, 96, 300), (256, 32, 257)])
def test_ffn_gate_up_swiglu_launch(be, pkg, K, N, T):
    rng = np.random.default_rng(3 * K + N + T)
    Wg, Wu = weights(pkg, rng, N * K), weights(pkg, rng, N * K)
    x = (rng.standard_normal((T, K)) * rng.uniform(0.1, 2.0, (T, 1))).astype(np.float32)
    be.set_option("mmq_tiles", 4)
    try:
        y = be.ffn_gate_up(IQ4_XS, Wg, Wu, N, K, x)
    finally:
        be.set_option("mmq_tiles", 0)
    g, u = ix.mul_mat(Wg, N, K, x), ix.mul_mat(Wu, N, K, x)
    with np.errstate(over="ignore"):
        ref = (g / (1.0 + np.exp(-g.astype(np.float64)))).astype(np.float32) * u
    assert np.abs(y - ref).max() <= 4e-5 * np.abs(ref).max() + 1e-6


def test_get_rows_bit_exact(be, pkg):
    rng = np.random.default_rng(23)
    K, R = 1024, 40
    table = weights(pkg, rng, R * K, 1.0)
    ids = np.array([0, 39, 7, 7, 21], np.int32)
    got = be.get_rows(IQ4_XS, table, K, R, ids)
    rb = ix.row_bytes(K)
    for i, r in enumerate(ids):
        want = ix.dequantize(table[r * rb:(r + 1) * rb], K)
        assert got[i].view(np.uint32).tolist() == want.view(np.uint32).tolist(), r


# ------------------------------------------------------------------------------------------------ the one-launch attention block
def test_qkv_attn_plan_takes_the_llama_iq4xs_mix(pkg):
    """Llama-3-8B geometry, attn_q / attn_k / attn_output IQ4_XS and attn_v Q5_K: Q | K | V run inside the attention launch, in no more LDS than Q4_K_M's."""
    lib = pkg.load_library()

    def plan(tq, tk, tv, to):
        slots = C.c_int32(0)
        return int(lib.mi355_debug_qkv_attn_plan(tq, tk, tv, to, 4096, 32, 8, 128, 8, 576, C.byref(slots))), int(slots.value)

    lds, slots = plan(IQ4_XS, IQ4_XS, 13, IQ4_XS)
    lds_q4, slots_q4 = plan(12, 12, 13, 12)
    assert 0 < lds <= lds_q4 and 0 < slots <= slots_q4, (lds, slots, lds_q4, slots_q4)


@pytest.mark.parametrize("cfg,kv", [("tiny-8b-2l", "q8_0"), ("tiny-8b-2l", "f16")])
def test_qkv_inside_the_attention_launch_is_bitwise_the_separate_launch(be, pkg, tmp_models, cfg, kv):
    """An IQ4_XS layer's single-token steps with Q | K | V inside the attention + attn_output launch equal the separate launches bit for bit, and the fused
    form really ran."""
    path = make(pkg, tmp_models, cfg, with_vocab=False)
    rows = {}
    for fused in (1, 0):
        be.set_option("qkv_attn_fused", fused)
        try:
            m = pkg.Model(path)
            c = pkg.Context(m, n_ctx=1024, type_k=KV[kv], type_v=KV[kv])
            out = []
            for seed, n_p in enumerate((3, 127, 600)):
                rng = np.random.default_rng(300 + seed)
                c.kv_clear()
                c.decode(rng.integers(0, m.n_vocab, n_p), np.arange(n_p))
                for s, t in enumerate(rng.integers(0, m.n_vocab, 6)):
                    assert c.decode([int(t)], [n_p + s]) == 0
                    out.append(c.logits().copy())
            rows[fused] = np.stack(out)
            assert (c.qkv_attn_launches() > 0) == bool(fused), c.qkv_attn_launches()
            c.close(); m.close()
        finally:
            be.set_option("qkv_attn_fused", -1)
    assert np.isfinite(rows[1]).all()
    assert np.array_equal(rows[1], rows[0]), float(np.abs(rows[1] - rows[0]).max())


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


@pytest.mark.parametrize("cfg,kv,n_prompt", [("tiny-gqa4", "q8_0", 21), ("tiny-gqa4", "f16", 40), ("tiny-d128", "q8_0", 40), ("tiny-d128", "f16", 21),
                                             ("tiny-8b-2l", "q8_0", 21), ("tiny-8b-2l", "f16", 40), ("tiny-qwen3", "q8_0", 21), ("tiny-qwen3", "f16", 40),
                                             ("tiny-gqa4", "q8_0", 130), ("tiny-d128", "q8_0", 512)])
def test_iq4xs_layers_logits_and_greedy_ids(be, pkg, tmp_models, cfg, kv, n_prompt):
    """A prompt (21 tokens: the generic mat-vec; 40, 130, 512: the plane kernels), then single-token steps (ring / stream / the one-launch attention block)
    teacher-forced with the reference's tokens: per layer, logits and greedy ids."""
    path = make(pkg, tmp_models, cfg, with_vocab=False)
    oq.set_fa_v_acc_f32(1 if kv == "f16" else 0)
    try:
        m = pkg.Model(path)
        c = pkg.Context(m, n_ctx=1024, n_batch=512, n_ubatch=512, type_k=KV[kv], type_v=KV[kv])
        ref = ix.Iq4xsRef(path, 1024, KV[kv], KV[kv])
        # tight (median of the first layer's tokens within f32 round-off) where the contractions are short: the device sums each lane's sub-block terms in
        # another f32 order than the generic one of the reference, and at Llama-3-8B's widths (gate / up 4096 -> 14336, down 14336 -> 4096) that 1e-7 is
        # enough to flip a Q8_K code of the next activation in most tokens (measured: median 4e-3 at 21 tokens, every token within FLIP_TOL)
        _check_run(pkg, c, m, ref, n_prompt, kv, tight=cfg != "tiny-8b-2l")
        c.close(); m.close()
    finally:
        oq.set_fa_v_acc_f32(0)


@pytest.mark.parametrize("kv,n_prompt", [("q8_0", 40), ("f16", 21), ("q8_0", 130)])
def test_iq4xs_qwen3moe_forced_routing(be, pkg, tmp_models, kv, n_prompt):
    """tiny-qwen3moe in IQ4_XS with the reference's expert selections handed over: 40 / 130 tokens go through the grouped-expert plane kernels."""
    path = make(pkg, tmp_models, "tiny-qwen3moe", with_vocab=False)
    oq.set_fa_v_acc_f32(1 if kv == "f16" else 0)
    try:
        m = pkg.Model(path)
        c = pkg.Context(m, n_ctx=256, type_k=KV[kv], type_v=KV[kv])
        ref = ix.Iq4xsMoeRef(path, 256, KV[kv], KV[kv])
        _check_run(pkg, c, m, ref, n_prompt, kv, tight=False, steps=6, forced=True)
        c.close(); m.close()
    finally:
        oq.set_fa_v_acc_f32(0)


def test_iq4xs_batched_steps(be, pkg, tmp_models):
    """Three sequences at different positions advance together (3-token steps: the generic mat-vec), against the reference sequence by sequence."""
    path = make(pkg, tmp_models, "tiny-gqa4", with_vocab=False)
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=512, n_seq_max=4, type_k=8, type_v=8)
    refs = [ix.Iq4xsRef(path, 512, 8, 8) for _ in range(3)]
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
    ref = ix.Iq4xsRef(path, 256, 8, 8)
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


def test_iq4xs_engine_chat_and_row_split_refused(pkg, tmp_models):
    """/v1/chat/completions on an IQ4_XS file returns the reference's greedy tokens; a row split of the file is refused with an error naming iq4_xs."""
    path = make(pkg, tmp_models, "tiny-gqa4", seed=3)
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
        assert st["status_code"] != 200 and "iq4_xs" in str(body), (st, body)
    finally:
        e.close()
    with pytest.raises(pkg.binding.MI355Error, match="iq4_xs"):
        pkg.Model(path, tp_rank=0, tp_size=2)
