"""BF16 (ggml type 30) on the GPU: the activation rounding, get_rows, the bf16 weight stream and the matrix-core contraction, their launch forms against each
other bit for bit, and whole files end to end - against the numpy restatement of tests/bf16_ref.py (the CPU oracle has no BF16)."""
import os

import numpy as np
import pytest

import bf16_ref as bf
import oracle_py as oq

pytestmark = pytest.mark.gpu

BF16 = bf.BF16
KV = {"f16": 1, "q8_0": 8, "q4_0": 2}
FLIP_TOL = 3e-2          # the end-to-end tolerance of tests/test_gpu_model.py
# The model test's own bar, tighter than FLIP_TOL: twice the worst relative error measured over its ten cases (taps, logits, 24 steps each) in the MI355X
# run of this file recorded in profiles/bf16_gpu_tests.txt (the lines "bf16 <config> kv <cache> prompt <n>: worst relative error"), 5.45e-3 (tiny-qwen3, q8_0 cache, 21-token prompt; the others 2.6e-3 .. 5.3e-3).  There are no integer activation codes to flip, but a
# last-bit f32 difference can still flip the bf16 rounding of a later activation (2^-8 of that value), which is what these figures are.  The mixed-file and the
# batched-step tests (other shapes of run: 8 steps, two sequences) stay on FLIP_TOL.
BF16_MODEL_TOL = 1.1e-2
MM_TOL = 2e-5            # mat-vec / contraction f32 output, of the output scale
GREEDY = dict(temperature=0.0, repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)
SPECIAL = np.array([0x3F808000, 0x3F818000, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7F800001, 0x7FC00000, 0xFFFFFFFF, 0x00000000, 0x80000000, 0x00400000,
                    0x80012345, 0x00008000, 0x00018000, 0x3F808001, 0x3F807FFF], np.uint32)


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def make(pkg, tmp_models, cfg, ftype="bf16", seed=11, with_vocab=True):
    path = str(tmp_models / f"{cfg}-{ftype}-{seed}.gguf")
    if not os.path.exists(path):
        pkg.gguf_synth.write_synthetic_llama(path, cfg, ftype, seed=seed, with_vocab=with_vocab)
    return path


def weights(rng, N, K, std=0.02):
    """N x K bf16 bits, values in the normal range."""
    return bf.round_bf16((rng.standard_normal((N, K)) * std).astype(np.float32))


def acts(rng, T, K):
    return (rng.standard_normal((T, K)) * rng.uniform(0.1, 3.0, (T, 1))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ rounding and get_rows
def test_activation_rounding_bit_exact(be):
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(1 << 16) * np.exp(rng.uniform(-40, 40, 1 << 16))).astype(np.float32)
    x[:SPECIAL.size] = SPECIAL.view(np.float32)
    x[64:64 + 4096] = rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32).view(np.float32)     # any bit pattern: NaNs, subnormals, ties
    x[8192:8192 + 2048] = (rng.integers(0, 1 << 16, 2048, dtype=np.uint32) << 16 | 0x8000).view(np.float32)  # exact ties
    got = be.f32_to_bf16(x)
    want = bf.round_bf16(x)
    assert (got == want).all(), [(hex(int(a)), hex(int(g)), hex(int(w))) for a, g, w in zip(x.view(np.uint32)[got != want][:5], got[got != want][:5], want[got != want][:5])]
    assert got[:4].tolist() == [0x3F80, 0x3F82, 0x7F80, 0x7F80]


def test_get_rows_bit_exact(be):
    K = 256
    table = np.arange(65536, dtype=np.uint32).astype(np.uint16).reshape(-1, K)       # every bf16 pattern
    ids = np.array([0, 255, 127, 128, 1, 254, 127], np.int32)                        # rows 127 / 128 / 254 / 255: infinities and NaNs of both signs; 0 / 128: subnormals
    got = be.get_rows(BF16, table, K, table.shape[0], ids)
    assert (got.view(np.uint32) == bf.get_rows(table, K, ids).view(np.uint32)).all()
    assert (got.view(np.uint32) == (table[ids].astype(np.uint32) << 16)).all()


# ------------------------------------------------------------------------------------------------ the contraction
# (K, N, bias) of a layer's projections: Llama-3-8B, Qwen2-7B (3584 / 18944, biases on Q | K | V), Qwen3-4B (attention width 4096 over n_embd 2560)
SHAPES = [(4096, 4096, False), (4096, 1024, False), (4096, 14336, False), (14336, 4096, False),
          (3584, 3584, True), (3584, 512, True), (3584, 18944, False), (18944, 3584, False),
          (2560, 4096, False), (4096, 2560, False), (2560, 9728, False), (9728, 2560, False)]
TS = [1, 2, 3, 5, 8, 16, 17, 33, 512]


@pytest.mark.parametrize("K,N,bias", SHAPES)
def test_mul_mat_all_token_counts(be, K, N, bias):
    """The model path's choice (weight stream below 8 tokens, matrix cores from 8 on), both paths forced at 8 / 16 / 17 tokens, against the restatement: <= 2e-5 of
    the output scale.  N is cut to 1056 rows (33 tiles of 32, not a multiple of 64 or 128: edge tiles in every kernel); the full widths run below."""
    rng = np.random.default_rng(K + N)
    Nc = min(N, 1056)
    W = weights(rng, Nc, K)
    b = (rng.standard_normal(Nc) * 0.25).astype(np.float32) if bias else None
    worst = 0.0
    for T in TS:
        x = acts(rng, T, K)
        ref = bf.mul_mat(W, Nc, K, x) + (b if bias else np.float32(0))
        scale = float(np.abs(ref).max())
        runs = [("model", be.mul_mat_bf16([W], K, x, bias=[b] if bias else None)[0])]
        if not bias:
            runs.append(("op_mul_mat", be.mul_mat(BF16, W, Nc, K, x)))
        if T in (8, 16, 17):
            runs.append(("stream", be.mul_mat_bf16([W], K, x, bias=[b] if bias else None, path=1)[0]))
        if T in (3, 5, 17):
            runs.append(("mfma", be.mul_mat_bf16([W], K, x, bias=[b] if bias else None, path=2)[0]))
        for what, y in runs:
            err = float(np.abs(y - ref).max()) / scale
            worst = max(worst, err)
            assert err <= MM_TOL, (what, T, err)
    print(f"bf16 mul_mat K={K} N={Nc}: worst error {worst:.3e} of the output scale")


@pytest.mark.parametrize("K,N,T", [(K, N, T) for K, N in [(4096, 14336), (14336, 4096), (3584, 18944), (18944, 3584), (2560, 9728)] for T in (1, 512)] + [(4096, 128256, 1)])
def test_mul_mat_full_width(be, K, N, T):
    """The full tensors at one token and at 512, and Llama-3's head (128256 rows) at one token: every 97th row and the last against the restatement."""
    rng = np.random.default_rng(K + N + T)
    W = weights(rng, N, K) if N < 100000 else np.tile(weights(rng, N // 32, K), (32, 1))
    x = acts(rng, T, K)
    y = be.mul_mat(BF16, W, N, K, x)
    rows = np.unique(np.r_[np.arange(0, N, 97), N - 1])
    ref = bf.mul_mat(W[rows], rows.size, K, x)
    assert np.abs(y[:, rows] - ref).max() <= MM_TOL * np.abs(ref).max()
    assert np.isfinite(y).all()


@pytest.mark.parametrize("forms", ["128", "64", "lds"])
def test_matrix_core_forms_agree_bitwise(be, forms, monkeypatch):
    """The three matrix-core kernels run the same chain of steps over k: bit-identical results (and equal to the default choice)."""
    rng = np.random.default_rng(9)
    K, N, T = 3584, 1056, 130
    W, x = weights(rng, N, K), acts(rng, T, K)
    b = (rng.standard_normal(N) * 0.25).astype(np.float32)
    r = acts(rng, T, N)
    base = be.mul_mat_bf16([W], K, x, bias=[b], resid=r, epi=1, path=2)[0]
    monkeypatch.setenv("MI355_MMBF16_FORM", forms)
    got = be.mul_mat_bf16([W], K, x, bias=[b], resid=r, epi=1, path=2)[0]
    assert np.array_equal(got.view(np.uint32), base.view(np.uint32))
    ref = r + (bf.mul_mat(W, N, K, x) + b)
    assert np.abs(got - ref).max() <= MM_TOL * np.abs(ref).max()


@pytest.mark.parametrize("K,Nq,Nkv,bias", [(4096, 4096, 1024, False), (3584, 3584, 512, True), (2560, 4096, 1024, False), (256, 40, 8, True)])
@pytest.mark.parametrize("T", [1, 2, 4, 5, 16])
def test_fused_qkv_launch_is_bitwise_the_separate_launches(be, K, Nq, Nkv, bias, T):
    rng = np.random.default_rng(K + Nq + T)
    Ws = [weights(rng, Nq, K), weights(rng, Nkv, K), weights(rng, Nkv, K)]
    bs = [(rng.standard_normal(w.shape[0]) * 0.25).astype(np.float32) for w in Ws] if bias else None
    x = acts(rng, T, K)
    fused = be.mul_mat_bf16(Ws, K, x, bias=bs, path=1)
    for i, w in enumerate(Ws):
        alone = be.mul_mat_bf16([w], K, x, bias=[bs[i]] if bias else None, path=1)[0]
        assert np.array_equal(fused[i].view(np.uint32), alone.view(np.uint32)), i
        ref = bf.mul_mat(w, w.shape[0], K, x) + (bs[i] if bias else np.float32(0))
        assert np.abs(alone - ref).max() <= MM_TOL * np.abs(ref).max()


@pytest.mark.parametrize("K,N", [(4096, 14336), (3584, 1184), (256, 50)])
@pytest.mark.parametrize("T", [1, 3, 16])
def test_swiglu_and_residual_epilogues_are_bitwise_the_separate_launches(be, K, N, T):
    rng = np.random.default_rng(K + N + T)
    N = min(N, 2080)
    Wg, Wu = weights(rng, N, K), weights(rng, N, K)
    x = acts(rng, T, K)
    fused = be.mul_mat_bf16([Wg, Wu], K, x, epi=2, path=1)[0]
    g = be.mul_mat_bf16([Wg], K, x, path=1)[0]
    u = be.mul_mat_bf16([Wu], K, x, path=1)[0]
    assert np.array_equal(fused.view(np.uint32), be.swiglu(g, u).view(np.uint32))
    r = acts(rng, T, N)
    added = be.mul_mat_bf16([Wg], K, x, resid=r, epi=1, path=1)[0]
    assert np.array_equal(added.view(np.uint32), (r + g).view(np.uint32))


@pytest.mark.parametrize("K,N", [(4096, 1056), (18944, 96), (3584, 200), (11008, 64), (264, 37)])
def test_one_token_is_bitwise_its_row_of_a_wider_launch(be, K, N):
    """The summation order of an output does not depend on the launch width: token t of a 16-, 8-, 4- and 2-token launch equals a launch of that token alone."""
    rng = np.random.default_rng(K + N)
    W, x = weights(rng, N, K), acts(rng, 16, K)
    single = be.mul_mat_bf16([W], K, x, path=1, tokens_per_launch=1)[0]
    for width in (16, 8, 4, 2):
        wide = be.mul_mat_bf16([W], K, x, path=1, tokens_per_launch=width)[0]
        assert np.array_equal(wide.view(np.uint32), single.view(np.uint32)), width
    chunks = be.mul_mat_bf16([W], K, x[:13], path=1)[0]                              # 8 + 4 + 1
    assert np.array_equal(chunks.view(np.uint32), single[:13].view(np.uint32))
    ref = bf.mul_mat(W, N, K, x)
    assert np.abs(single - ref).max() <= MM_TOL * np.abs(ref).max()


@pytest.mark.parametrize("path,T", [(1, 1), (1, 5), (2, 40)])
def test_graph_replay_is_bitwise_eager(be, path, T):
    rng = np.random.default_rng(40 + T)
    K, N = 4096, 1056
    Ws = [weights(rng, N, K), weights(rng, 256, K)]
    x = acts(rng, T, K)
    eager = be.mul_mat_bf16(Ws, K, x, path=path)
    graph = be.mul_mat_bf16(Ws, K, x, path=path, graph=True)
    for a, b in zip(eager, graph):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ model level
def _check_run(c, m, ref, n_prompt, steps=24):
    """The checks of tests/test_gpu_model.py::test_prefill_layers_logits_and_greedy_ids with its bars; returns the worst relative error seen."""
    rng = np.random.default_rng(5)
    prompt = rng.integers(0, m.n_vocab, n_prompt)
    c.enable_taps(True)
    assert c.decode(prompt, np.arange(n_prompt)) == 0
    r = ref.decode(prompt, np.arange(n_prompt))[0]
    errs = [rel_err(c.layer_out(il, n_prompt).reshape(n_prompt, -1), ref.layer_out(il, n_prompt)) for il in range(m.n_layer)]
    errs.append(rel_err(c.logits(), r))
    assert max(errs) <= FLIP_TOL, errs
    c.enable_taps(False)
    tok, mism, step_err = int(r.argmax()), 0, []
    for step in range(steps):
        assert c.decode([tok], [n_prompt + step]) == 0
        r = ref.decode([tok], [n_prompt + step])[0]
        g = c.logits()
        step_err.append(rel_err(g, r))
        tok = int(r.argmax())
        if c.argmax() != tok:
            top2 = np.sort(r)[-2:]
            assert top2[1] - top2[0] <= 2 * FLIP_TOL * max(1.0, np.abs(r).max()), (step, top2)
            mism += 1
        assert int(g.argmax()) == c.argmax()
    assert max(step_err) <= FLIP_TOL, step_err
    assert mism <= 1, (mism, step_err)
    return max(errs + step_err)


@pytest.mark.parametrize("cfg,kv,n_prompt", [("tiny", "q8_0", 21), ("tiny", "f16", 40), ("tiny", "q8_0", 5), ("tiny-qwen2", "q8_0", 21), ("tiny-qwen2", "f16", 40),
                                             ("tiny-qwen3", "q8_0", 21), ("tiny-qwen3", "f16", 40), ("tiny-8b-2l", "q8_0", 21), ("tiny-8b-2l", "q8_0", 70),
                                             ("tiny-qwen2-7b-2l", "q8_0", 40)])
def test_bf16_layers_logits_and_greedy_ids(be, pkg, tmp_models, cfg, kv, n_prompt):
    """A prompt (5 tokens: the weight stream in chunks of 4 + 1; 21, 40, 70: the matrix cores), then 24 single-token steps through the captured graph (the weight
    stream), teacher-forced with the reference's tokens: per-layer taps, logits and greedy ids."""
    path = make(pkg, tmp_models, cfg, with_vocab=False)
    oq.set_fa_v_acc_f32(1 if kv == "f16" else 0)
    try:
        m = pkg.Model(path)
        c = pkg.Context(m, n_ctx=128, type_k=KV[kv], type_v=KV[kv])
        ref = bf.Bf16Ref(path, 128, KV[kv], KV[kv])
        worst = _check_run(c, m, ref, n_prompt)
        assert worst <= BF16_MODEL_TOL, worst
        print(f"bf16 {cfg} kv {kv} prompt {n_prompt}: worst relative error {worst:.3e}")
        c.close(); m.close()
    finally:
        oq.set_fa_v_acc_f32(0)


def _retyped(pkg, monkeypatch, change):
    """The synthetic writer with the types of some tensors changed: change(name, ne, type) -> type."""
    gs = pkg.gguf_synth
    orig = gs.model_tensors
    monkeypatch.setattr(gs, "model_tensors", lambda cfg, ftype: [(n, ne, change(n, ne, t), f) for n, ne, t, f in orig(cfg, ftype)])
    return gs


def test_mixed_file_bf16_embeddings_and_head(be, pkg, tmp_path, monkeypatch):
    """A q4_k_m file whose token_embd and output are BF16 (quantised mixes that keep those two in bf16 are published): quantised layers, a bf16 get_rows and a bf16 head."""
    gs = _retyped(pkg, monkeypatch, lambda n, ne, t: BF16 if n in ("token_embd.weight", "output.weight") else t)
    path = str(tmp_path / "mixed.gguf")
    gs.write_synthetic_llama(path, "tiny", "q4_k_m", seed=5, with_vocab=False)
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=128, type_k=8, type_v=8)
    ref = bf.Bf16Ref(path, 128, 8, 8)
    assert ref._embd_bf16 is not None and ref.t["output.weight"][1] == BF16
    _check_run(c, m, ref, 21, steps=8)
    c.close(); m.close()


def test_bf16_batched_steps(be, pkg, tmp_models):
    """Two sequences at different positions advance together (2-token steps: one launch of the weight stream per projection), against the reference sequence
    by sequence."""
    path = make(pkg, tmp_models, "tiny-qwen2", with_vocab=False)
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=256, n_seq_max=4, type_k=8, type_v=8)
    refs = [bf.Bf16Ref(path, 256, 8, 8) for _ in range(2)]
    rng = np.random.default_rng(17)
    lens = [40, 9]
    nxt = []
    for sq, n in enumerate(lens):
        p = rng.integers(0, m.n_vocab, n)
        r = refs[sq].decode(p, np.arange(n))[0]
        assert c.decode(p, np.arange(n), [sq] * n) == 0
        nxt.append(int(r.argmax()))
    for step in range(4):
        toks, pos = nxt, [lens[s] + step for s in range(2)]
        assert c.decode(toks, pos, [0, 1], [1, 1]) == 0
        got = [c.logits(i) for i in range(2)]
        for s in range(2):
            r = refs[s].decode([toks[s]], [pos[s]])[0]
            assert rel_err(got[s], r) <= FLIP_TOL, (step, s)
            nxt[s] = int(r.argmax())
    c.close(); m.close()


# ------------------------------------------------------------------------------------------------ engine level and refusals
def _greedy_ref(path, pkg, prompt: str, n_predict: int):
    m = pkg.Model(path)
    toks = m.tokenize(prompt, add_special=True, parse_special=True)
    eos = m.lib.mi355_token_eos(m.h)
    ref = bf.Bf16Ref(path, 256, 8, 8)
    r = ref.decode(toks, np.arange(len(toks)))[0]
    out, gaps, pos = [], [], len(toks)
    for _ in range(n_predict + 1):                      # (as tests/test_gpu_qwen3.py's _greedy: the engine's count of max_tokens)
        t = int(r.argmax())
        if t == eos:
            break
        top2 = np.sort(r)[-2:]
        out.append(m.token_to_piece(t))
        gaps.append(float((top2[1] - top2[0]) / max(1.0, np.abs(r).max())))
        r = ref.decode([t], [pos])[0]
        pos += 1
    m.close()
    return out, gaps


def test_bf16_engine_chat_and_row_split_refused(pkg, tmp_models):
    """/v1/chat/completions on a bf16 file returns the reference's greedy tokens; a row split of the file (tp_size 2) is refused with an error naming bf16."""
    path = make(pkg, tmp_models, "tiny", seed=3)
    e = pkg.Engine()
    try:
        st, body = e.load_model(llama_model_path=path, ctx_len=256, n_parallel=1, ngl=100, user_prompt="u:", ai_prompt="a:", system_prompt="s:")
        assert st["status_code"] == 200 and not st["has_error"], (st, body)
        msgs = [{"role": "system", "content": "be brief"}, {"role": "user", "content": "hello world"}]
        name = os.path.splitext(os.path.basename(path))[0]                      # (the engine names a model after its file)
        st, body = e.chat_completion(model=name, messages=msgs, max_tokens=8, **GREEDY)[-1]
        assert st["status_code"] == 200 and not st["has_error"], (st, body)
        content = body["choices"][0]["message"]["content"]
        pieces, gaps = _greedy_ref(path, pkg, "s:be briefu:hello worlda:", 8)
        want = b"".join(pieces).decode("utf-8", errors="replace")
        assert "u:" not in want, want                  # (the engine stops at the user marker: this seed's text must not hold it, or nothing below would be checked)
        if content not in (want.lstrip(" "), want):
            # free-running greedy text: it may leave the reference's only where the reference's two best logits are a near tie (the bar of the model test:
            # a gap within 2 FLIP_TOL of the logits' scale), and must agree with it up to there - at least the first token
            agree = 0
            for i in range(1, len(pieces) + 1):
                pre = b"".join(pieces[:i]).decode("utf-8", errors="replace")
                if content.startswith(pre.lstrip(" ")) or content.startswith(pre):
                    agree = i
            assert 1 <= agree < len(pieces) and gaps[agree] <= 2 * FLIP_TOL, (content, want, agree, gaps)
        e.unload_model(model=name)
    finally:
        e.close()
    with pytest.raises(pkg.binding.MI355Error, match="bf16"):
        pkg.Model(path, tp_rank=0, tp_size=2)


def test_bf16_norm_and_experts_refused(be, pkg, tmp_path):
    """A BF16 norm vector and BF16 expert tensors are refused at load, each with an error that names the tensor and bf16."""
    import struct
    path = str(tmp_path / "norm.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny", "q4_k_m", seed=5, with_vocab=False)
    # the file's own entry for the vector, its type word changed from f32 to bf16: name | n_dims (1) | ne[0] | type | offset
    raw = bytearray(open(path, "rb").read())
    name = b"blk.0.attn_norm.weight"
    at = raw.index(struct.pack("<Q", len(name)) + name) + 8 + len(name)
    assert struct.unpack_from("<I", raw, at)[0] == 1 and struct.unpack_from("<I", raw, at + 12)[0] == 0
    struct.pack_into("<I", raw, at + 12, BF16)
    open(path, "wb").write(raw)
    with pytest.raises(pkg.binding.MI355Error, match=r"blk\.0\.attn_norm\.weight.*bf16"):
        pkg.Model(path)
    path = str(tmp_path / "moe.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny-qwen3moe", "bf16", seed=5, with_vocab=False)
    with pytest.raises(pkg.binding.MI355Error, match=r"_exps\.weight.*bf16"):
        pkg.Model(path)
