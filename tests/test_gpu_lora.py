"""LoRA adapters on the GPU: the adapter kernels (csrc/lora.hip) op by op against float64 on the same rounded operands, whole models with adapters set
against the composed reference of tests/lora_ref.py (prompt, single steps, batched steps, embeddings, greedy_steps), the neutrality of a context that has
no adapter set, and /loadmodel's "lora" key through the engine."""
import numpy as np
import pytest

import lora_cases as lc
import oracle_py as oq
from lora_cases import FLIP_TOL, KV, TIGHT_TOL, rel_err

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit round-off of f32


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


# ------------------------------------------------------------------------------------------------ op level
def seg_operands(rng, K, N, r, dtype):
    A = (rng.standard_normal((r, K)) / np.sqrt(K)).astype(dtype)
    B = (rng.standard_normal((N, r)) * 0.5).astype(dtype)
    return A, B


def exact_and_bound(A, B, x, scale, f16):
    """float64 delta scale * B (A x) on the operands as the kernel rounds them, and the bound per element.  With u = 2^-24:
      first product, n = K terms:    e1[j] = (K - 1) u sum_k |A[j][k] x[k]|, carried to the output through |B|;
      second product, n = r terms:   (r - 1) u sum_j |B[n][j] t[j]|;
      F16 pairs: t is rounded to f16 once - 2^-11 |t[j]| (2^-25 at least: the f16 subnormal step), carried through |B|;
      all times |scale|.
    The standard bound takes the n - 1 additions of a serial sum.  The kernel's sums are short chains and a tree (K / 256 pieces of 4 or 8 per lane, six
    levels), so of the (K - 1) u it uses at most (K / 64 + 8) u; what is left (for K >= 256 more than 240 u sum |A x| |B| >= 240 u |B t|) covers the
    roundings the two sums do not count: each product's own (f32 pairs: one u each), scale * sum, and out + delta where a test adds onto a previous delta."""
    xr = x.astype(np.float16).astype(np.float64) if f16 else x.astype(np.float64)
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    K, r = A.shape[1], A.shape[0]
    t = xr @ A64.T                                                  # [T][r]
    e1 = (K - 1) * U * (np.abs(xr) @ np.abs(A64).T)
    y = t @ B64.T                                                   # [T][N]
    bound = e1 @ np.abs(B64).T + (r - 1) * U * (np.abs(t) @ np.abs(B64).T)
    if f16:
        bound += np.maximum(2.0 ** -11 * (np.abs(t) + e1), 2.0 ** -25) @ np.abs(B64).T
    return scale * y, abs(scale) * bound


SHAPES = [(256, 512, 1, 1), (576, 192, 12, 3), (4096, 1024, 64, 1), (1024, 4096, 8, 37),
          (320, 100, 3, 2), (320, 100, 3, 8), (512, 260, 512, 9)]       # ... the 2- and 8-token forms of the one launch, the largest rank on the two launches


@pytest.mark.parametrize("n_seg", [1, 2, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("K,N,r,T", SHAPES)
def test_lora_delta_op(be, K, N, r, T, dtype, n_seg):
    rng = np.random.default_rng(K + 7 * N + 13 * r + T + n_seg)
    f16 = dtype == np.float16
    x = rng.standard_normal((T, K)).astype(np.float32)
    Ns = [N, N // 2 + 5, 77][:n_seg]
    rs = [r, r, max(1, r // 2)][:n_seg]
    scales = [1.5, -0.25, 2.0][:n_seg]
    pad, guard = 7, np.float32(-12345.5)
    segs, outs0 = [], []
    for s in range(n_seg):
        A, B = seg_operands(rng, K, Ns[s], rs[s], dtype)
        out0 = np.zeros((T, Ns[s] + pad), np.float32)
        out0[:, Ns[s]:] = guard
        segs.append((A, B, scales[s], out0))
        outs0.append(out0)
    got = be.lora_delta(segs, x)
    again = be.lora_delta(segs, x)
    for s in range(n_seg):
        A, B, sc, _ = segs[s]
        want, bound = exact_and_bound(A, B, x, sc, f16)
        assert (got[s][:, Ns[s]:] == guard).all(), "wrote beyond N"
        err = np.abs(got[s][:, :Ns[s]].astype(np.float64) - want)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"seg {s}: max err {err.max():.3e}, max err / bound {worst:.3f}")
        assert (err <= bound).all(), (s, worst)
        assert np.abs(want).max() > 5 * bound.max()                       # (a dropped or swapped operand would land far outside the bound)
        assert got[s].tobytes() == again[s].tobytes()                     # the same call twice: the same bits
    # the delta is ADDED: onto rows that hold something, the result is the f32 sum of what was there and the delta computed above, bit for bit
    held = [(rng.standard_normal(o.shape) * 3).astype(np.float32) for o in outs0]
    got2 = be.lora_delta([(sg[0], sg[1], sg[2], h) for sg, h in zip(segs, held)], x)
    for s in range(n_seg):
        want2 = held[s].copy()
        want2[:, :Ns[s]] = held[s][:, :Ns[s]] + got[s][:, :Ns[s]]
        assert got2[s].tobytes() == want2.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("T", [1, 20])
def test_two_stacked_adapters(be, dtype, T):
    """Two adapters on one tensor, applied one after the other onto the same rows: the sum of both deltas within the sum of both bounds."""
    rng = np.random.default_rng(91 + T)
    K, N = 1024, 333
    x = rng.standard_normal((T, K)).astype(np.float32)
    A1, B1 = seg_operands(rng, K, N, 16, dtype)
    A2, B2 = seg_operands(rng, K, N, 5, np.float32)
    out = be.lora_delta([(A1, B1, 1.0, np.zeros((T, N), np.float32))], x)[0]
    out = be.lora_delta([(A2, B2, -0.5, out)], x)[0]
    w1, b1 = exact_and_bound(A1, B1, x, 1.0, dtype == np.float16)
    w2, b2 = exact_and_bound(A2, B2, x, -0.5, False)
    assert (np.abs(out.astype(np.float64) - (w1 + w2)) <= b1 + b2).all()


def test_lora_delta_refusals(pkg, be):
    x = np.zeros((1, 256), np.float32)
    ok = (np.zeros((4, 256), np.float32), np.zeros((8, 4), np.float32), 1.0, np.zeros((1, 8), np.float32))
    be.lora_delta([ok], x)
    for bad, xx in (((np.zeros((0, 256), np.float32), np.zeros((8, 0), np.float32), 1.0, np.zeros((1, 8), np.float32)), x),          # r = 0
                    ((np.zeros((513, 256), np.float32), np.zeros((8, 513), np.float32), 1.0, np.zeros((1, 8), np.float32)), x),      # r = 513
                    ((np.zeros((4, 272), np.float32), np.zeros((8, 4), np.float32), 1.0, np.zeros((1, 8), np.float32)), np.zeros((1, 272), np.float32))):   # K % 32
        with pytest.raises(pkg.MI355Error, match=r"\(-103\)"):
            be.lora_delta([bad], xx)


# ------------------------------------------------------------------------------------------------ model level
def open_case(pkg, tmp_models, case, n_ctx, **ctx_kw):
    gs = pkg.gguf_synth
    base = lc.base_file(gs, tmp_models, case)
    paths = [lc.adapter_file(gs, tmp_models, case.cfg, ad) for ad in case.adapters]
    m = pkg.Model(base)
    ads = [pkg.LoraAdapter(m, p) for p in paths]
    c = pkg.Context(m, n_ctx=n_ctx, type_k=KV[case.kv], type_v=KV[case.kv], **ctx_kw)
    for a, spec in zip(ads, case.adapters):
        c.set_adapter_lora(a, spec.scale)
    return base, paths, m, ads, c


@pytest.mark.parametrize("case", lc.CASES, ids=lc.CASE_IDS)
def test_model_with_adapters(pkg, tmp_models, case):
    """A 21-token prompt (the two-launch form of the kernels), teacher-forced single steps (the one-launch form inside the captured step), then a batched
    step over three sequences: per-layer taps and logits against LoraRef, at the tolerances and by the rules of tests/test_gpu_qwen3.py."""
    oq.set_fa_v_acc_f32(1 if case.kv == "f16" else 0)
    try:
        base, paths, m, ads, c = open_case(pkg, tmp_models, case, 64)
        assert [a.n_pairs for a in ads] == [len(pkg.gguf_synth.lora_pairs(pkg.gguf_synth.CONFIGS[case.cfg], s.rank, s.targets)) for s in case.adapters]
        ref = lc.reference(case, base, paths, 64)
        n = 21
        prompt = np.random.default_rng(5).integers(0, m.n_vocab, n)
        c.enable_taps(True)
        assert c.decode(prompt, np.arange(n)) == 0
        r = ref.decode(prompt, np.arange(n))[0]
        errs = [rel_err(c.layer_out(il, n).reshape(n, -1), ref.layer_out(il, n)) for il in range(m.n_layer)]
        a0, b0 = c.layer_out(0, n).reshape(n, -1), ref.layer_out(0, n)
        tok_err0 = np.abs(a0 - b0).max(axis=1) / max(1.0, float(np.abs(b0).max()))
        errs.append(rel_err(c.logits(), r))
        print("prompt errors:", errs, "median first-layer token error:", float(np.median(tok_err0)))
        assert max(errs) <= FLIP_TOL, errs
        c.enable_taps(False)
        tok, mism, step_err = int(r.argmax()), 0, []
        for step in range(6):
            assert c.decode([tok], [n + step]) == 0
            r = ref.decode([tok], [n + step])[0]
            step_err.append(rel_err(c.logits(), r))
            tok = int(r.argmax())
            if c.argmax() != tok:                # only at a near tie of the reference's logits
                top2 = np.sort(r)[-2:]
                assert top2[1] - top2[0] <= 2 * FLIP_TOL * max(1.0, np.abs(r).max()), (step, top2)
                mism += 1
        print("step errors:", step_err)
        assert max(step_err) <= FLIP_TOL, step_err
        assert mism <= 1, (mism, step_err)
        if lc.tight_applies(case):
            assert float(np.median(tok_err0)) <= TIGHT_TOL, (errs, tok_err0)
            assert int((tok_err0 <= TIGHT_TOL).sum()) * 3 >= 2 * n, (errs, tok_err0)
        c.close()

        # three sequences advance together (a batched step: the 4-token form of the one launch), after prompts of 12, 5 and 9 tokens
        c = pkg.Context(m, n_ctx=128, n_seq_max=4, type_k=KV[case.kv], type_v=KV[case.kv])
        for a, spec in zip(ads, case.adapters):
            c.set_adapter_lora(a, spec.scale)
        ref = lc.reference(case, base, paths, 128)
        rng = np.random.default_rng(17)
        lens = [12, 5, 9]
        for sq, ln in enumerate(lens):
            p = rng.integers(0, m.n_vocab, ln)
            fl = np.zeros(ln, np.int8); fl[-1] = 1
            assert c.decode(p, np.arange(ln), [sq] * ln, fl) == 0
            rr = ref.decode(p, np.arange(ln), [sq] * ln, fl)
            assert rel_err(c.logits(ln - 1), rr[0]) <= FLIP_TOL
        toks = [3, 5, 7]
        for step in range(3):
            pos = [ln + step for ln in lens]
            assert c.decode(toks, pos, [0, 1, 2], [1, 1, 1]) == 0
            rr = ref.decode(toks, pos, [0, 1, 2], [1, 1, 1])
            for j in range(3):
                assert rel_err(c.logits(j), rr[j]) <= FLIP_TOL, (step, j)
            toks = [int(v.argmax()) for v in rr]
        c.close()
        for a in ads:
            a.close()
        m.close()
    finally:
        oq.set_fa_v_acc_f32(0)


def test_embeddings_mode_and_greedy_steps(pkg, tmp_models):
    """Embeddings mode returns the final-norm rows of the adapted layers; greedy_steps gives the tokens and the last logits row, bit for bit, of the same
    steps decoded one call at a time on a second context."""
    case = lc.CASES[lc.CASE_IDS.index("d128-all")]
    base, paths, m, ads, c = open_case(pkg, tmp_models, case, 64)
    ref = lc.reference(case, base, paths, 64)
    n = 10
    prompt = np.random.default_rng(9).integers(0, m.n_vocab, n)
    c.set_embeddings(True)
    assert c.decode(prompt, np.arange(n)) == 0
    ref.decode(prompt, np.arange(n))
    want = (oq.rms_norm(ref.layer_out(m.n_layer - 1, n)[-1], ref.eps) * ref._f32("output_norm.weight")).astype(np.float32)
    assert rel_err(c.embeddings(-1), want) <= FLIP_TOL
    c.set_embeddings(False)
    c.kv_clear()
    c2 = pkg.Context(m, n_ctx=64, type_k=KV[case.kv], type_v=KV[case.kv])
    for a, spec in zip(ads, case.adapters):
        c2.set_adapter_lora(a, spec.scale)
    for cc in (c, c2):
        assert cc.decode(prompt, np.arange(n)) == 0
    first = int(c.logits().argmax())
    assert first == int(c2.logits().argmax())
    toks = c.greedy_steps(first, n, 5)
    tok, toks2 = first, []
    for i in range(5):
        assert c2.decode([tok], [n + i]) == 0
        tok = c2.argmax()
        toks2.append(tok)
    assert list(toks) == toks2
    assert c.logits().tobytes() == c2.logits().tobytes()
    c.close(); c2.close()
    for a in ads:
        a.close()
    m.close()


# ------------------------------------------------------------------------------------------------ neutrality
def test_a_context_without_adapters_is_unchanged(pkg, tmp_models):
    """tiny-d128 with a q8_0 cache takes the one-launch attention block.  The logits of a prompt and of single steps before any adapter, after set and clear,
    and from a fresh context are the same bits, and the counter of one-launch attention blocks advances equally; while an attention adapter is set it stands
    still (an adapter on the feed-forward alone leaves it running); scale 0 gives the base model's logits."""
    case = lc.CASES[lc.CASE_IDS.index("d128-two")]
    gs = pkg.gguf_synth
    base = lc.base_file(gs, tmp_models, case)
    attn_ad = lc.adapter_file(gs, tmp_models, case.cfg, case.adapters[0])
    ffn_case = lc.CASES[lc.CASE_IDS.index("d128-ffn")]
    ffn_ad = lc.adapter_file(gs, tmp_models, ffn_case.cfg, ffn_case.adapters[0])
    m = pkg.Model(base)
    vram0 = m.lib.mi355_model_other_buffer(m.h)
    a_attn, a_ffn = pkg.LoraAdapter(m, attn_ad), pkg.LoraAdapter(m, ffn_ad)
    assert m.lib.mi355_model_other_buffer(m.h) > vram0                  # the model counts its adapters' device bytes
    n = 9
    prompt = np.random.default_rng(3).integers(0, m.n_vocab, n)

    def run(c):
        """prompt + 3 single steps from an empty cache: (every logits row, how far the one-launch counter moved)"""
        c.kv_clear()
        k0 = c.qkv_attn_launches()
        rows = []
        assert c.decode(prompt, np.arange(n)) == 0
        rows.append(c.logits())
        for i in range(3):
            assert c.decode([5 + i], [n + i]) == 0
            rows.append(c.logits())
        return np.stack(rows), c.qkv_attn_launches() - k0

    c = pkg.Context(m, n_ctx=64, type_k=8, type_v=8)
    before, k_before = run(c)
    assert k_before > 0                                                  # (the base does take the one-launch block here)
    c.set_adapter_lora(a_attn, 1.0)
    adapted, k_adapted = run(c)
    assert k_adapted == 0
    assert rel_err(adapted[-1], before[-1]) >= FLIP_TOL                  # (and the adapter is applied)
    assert not c.rm_adapter_lora(a_ffn) and c.rm_adapter_lora(a_attn)    # rm of one that is not set: false
    c.set_adapter_lora(a_ffn, 1.0)
    ffn_only, k_ffn = run(c)
    assert k_ffn > 0 and rel_err(ffn_only[-1], before[-1]) >= FLIP_TOL
    c.set_adapter_lora(a_attn, 0.0)
    c.rm_adapter_lora(a_ffn)
    zero, _ = run(c)
    ref = lc.reference(case, base, [], 64, False)
    ref.decode(prompt, np.arange(n))
    for i in range(3):
        r = ref.decode([5 + i], [n + i])[0]
    assert rel_err(zero[-1], r) <= FLIP_TOL and rel_err(before[-1], r) <= FLIP_TOL
    c.clear_adapter_lora()
    after, k_after = run(c)
    fresh_ctx = pkg.Context(m, n_ctx=64, type_k=8, type_v=8)
    fresh, k_fresh = run(fresh_ctx)
    assert before.tobytes() == after.tobytes() == fresh.tobytes()
    # (the counter counts launches made, and a captured step is launched once, when it is captured: the first run of a context and the run after the
    # clear - which dropped the captured steps - count the same launches)
    assert k_before == k_after == k_fresh
    c.close(); fresh_ctx.close()
    a_attn.close(); a_ffn.close()
    assert m.lib.mi355_model_other_buffer(m.h) == vram0
    m.close()


def test_adapter_of_another_model_is_refused(pkg, tmp_models):
    gs = pkg.gguf_synth
    case = lc.CASES[lc.CASE_IDS.index("d128-all")]
    base = lc.base_file(gs, tmp_models, case)
    other = lc.CASES[lc.CASE_IDS.index("qwen3-all")]
    m = pkg.Model(base)
    with pytest.raises(pkg.MI355Error, match="adapter architecture 'qwen3' does not match the model's 'llama'"):
        pkg.LoraAdapter(m, lc.adapter_file(gs, tmp_models, other.cfg, other.adapters[0]))
    with pytest.raises(pkg.MI355Error):
        pkg.LoraAdapter(m, str(tmp_models / "no-such-adapter.gguf"))
    m.close()


# ------------------------------------------------------------------------------------------------ engine
GREEDY = dict(temperature=0.0, repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)


def test_engine_loadmodel_lora(pkg, tmp_path_factory, tmp_models):
    """/loadmodel with "lora": the chat completion is the greedy continuation of LoraRef (compared up to the reference's first near tie) and differs from the
    base model's; the listing's vram counts the adapter; a bad path, an adapter of another architecture and a row split fail in the load-error shape."""
    gs = pkg.gguf_synth
    d = tmp_path_factory.mktemp("englora")
    path = str(d / "tiny-d128.gguf")
    gs.write_synthetic_llama(path, "tiny-d128", "q4_k_m", with_vocab=True)
    spec = lc.Ad(8, 16.0, lc.ALL7 + ("output",), std=0.1)
    ad = lc.adapter_file(gs, tmp_models, "tiny-d128", spec)
    wrong = lc.adapter_file(gs, tmp_models, "tiny-qwen3", spec)
    msgs = [{"role": "user", "content": "hello world"}]
    n_predict = 8
    common = dict(llama_model_path=path, ctx_len=256, n_parallel=1, cache_type="q8_0", user_prompt="u:", ai_prompt="a:", system_prompt="s:")

    def chat(**load):
        e = pkg.Engine()
        try:
            st, body = e.load_model(**common, **load)
            assert st["status_code"] == 200 and not st["has_error"], (st, body)
            vram = e.get_models()[1]["data"][0]["vram"]
            st, body = e.chat_completion(model="tiny-d128", messages=msgs, max_tokens=n_predict, **GREEDY)[-1]
            assert st["status_code"] == 200 and not st["has_error"], (st, body)
            return body["choices"][0]["message"]["content"], vram
        finally:
            e.close()

    base_text, base_vram = chat()
    lora_text, lora_vram = chat(lora=[{"path": ad, "scale": 0.75}])
    plain_text, _ = chat(lora=[ad])                                        # a path alone: scale 1
    assert lora_text != base_text and plain_text != base_text
    assert lora_vram >= base_vram + sum(raw.size for _, _, raw in lc_read(ad).values())

    # LoraRef's greedy tokens for the same prompt, as text
    from lora_ref import Adapter, LoraRef
    m = pkg.Model(path)
    toks = m.tokenize("u:hello worlda:", add_special=True, parse_special=True)
    eos = m.lib.mi355_token_eos(m.h)
    ref = LoraRef(path, 64, 8, 8)
    ref.set_adapters([(Adapter(ad), 0.75)])
    r = ref.decode(toks, np.arange(len(toks)))[0]
    want, pos = b"", len(toks)
    for _ in range(n_predict + 1):                                         # (the reference's budget rule: n_predict + 1 sampled tokens)
        top2 = np.sort(r)[-2:]
        if top2[1] - top2[0] <= 2 * FLIP_TOL * max(1.0, float(np.abs(r).max())):
            break                                                          # a near tie: either token is a correct greedy choice, the texts may part here
        t = int(r.argmax())
        if t == eos:
            break
        want += m.token_to_piece(t)
        r = ref.decode([t], [pos])[0]
        pos += 1
    m.close()
    want = want.decode("utf-8", errors="replace")
    assert len(want) > 0
    assert lora_text.startswith(want) or lora_text.startswith(want.lstrip(" ")), (lora_text, want)

    # failures: the reference's load-error shape, and no model left behind
    e = pkg.Engine()
    try:
        for load, needle in ((dict(lora=[str(d / "missing.gguf")]), "missing.gguf"), (dict(lora=[wrong]), "does not match the model's 'llama'"),
                             (dict(lora=[ad], split_mode="row", split_ranks=2), "lora"), (dict(lora="x.gguf"), "lora")):
            st, body = e.load_model(**common, **load)
            assert st == {"is_done": False, "has_error": True, "is_stream": False, "status_code": 500}, (load, st)
            assert body["message"] == "Failed to load model" and needle in body["error"], body
            assert e.get_models()[1]["data"] == []
        st, body = e.load_model(**common, lora=[ad], split_mode="row", split_ranks=2)
        assert "split_mode" in body["error"] and "row" in body["error"]
    finally:
        e.close()


def lc_read(path):
    from gguf_read import read_gguf
    return read_gguf(path)[1]
