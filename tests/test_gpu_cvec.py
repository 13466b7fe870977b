"""Control vectors on the GPU: the row-broadcast add op by op, its exactness inside the model (taps), whole models with a vector applied
against the composed reference of tests/cvec_ref.py, the neutrality of apply then clear, the refusals, the power method's kernels against float64, /loadmodel's
"control_vectors" key through the engine, and tools/cvector_generator.py on a tiny model."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cvec_cases as cc
import cvec_ref as cr
import lora_cases as lc
import oracle_py as oq
from lora_cases import FLIP_TOL, KV, TIGHT_TOL, rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def open_case(pkg, tmp_models, case, n_ctx, **kw):
    base = lc.base_file(pkg.gguf_synth, tmp_models, case)
    m = pkg.Model(base)
    c = pkg.Context(m, n_ctx=n_ctx, type_k=KV[case.kv], type_v=KV[case.kv], **kw)
    return base, m, c


def prompt_of(m):
    return np.random.default_rng(cc.PROMPT_SEED).integers(0, m.n_vocab, cc.N_PROMPT)


def taps_of(c, m, prompt):
    """the layers' output rows and the logits of the prompt from an empty cache, taps on"""
    c.kv_clear()
    c.enable_taps(True)
    assert c.decode(prompt, np.arange(prompt.size)) == 0
    taps = [c.layer_out(il, prompt.size).reshape(prompt.size, -1).copy() for il in range(m.n_layer)]
    c.enable_taps(False)
    return taps, c.logits().copy()


# ------------------------------------------------------------------------------------------------ op level
@pytest.mark.parametrize("T", [1, 3, 67])
@pytest.mark.parametrize("E", [32, 576, 4096])
def test_add_row_vec_op(be, E, T):
    rng = np.random.default_rng(E + T)
    x = (rng.standard_normal((T, E)) * 3).astype(np.float32)
    v = rng.standard_normal(E).astype(np.float32)
    x[0, 0], v[0] = np.float32(1e8), np.float32(1.0)                    # (an addition that rounds)
    y = be.add_row_vec(x, v)
    assert y[:T].tobytes() == (x + v[None, :]).astype(np.float32).tobytes()
    assert y[T].tobytes() == b"\xa5" * (4 * E), "wrote behind the rows"
    assert be.add_row_vec(x, v).tobytes() == y.tobytes()


def test_add_row_vec_refuses_a_width_off_32(pkg, be):
    with pytest.raises(pkg.MI355Error, match=r"\(-103\)"):
        be.add_row_vec(np.zeros((2, 48), np.float32), np.zeros(48, np.float32))


# ------------------------------------------------------------------------------------------------ exactness in the model
@pytest.mark.parametrize("case", cc.MODEL_CASES, ids=cc.MODEL_IDS)
def test_the_add_is_exact_in_the_model(pkg, tmp_models, case):
    base, m, c = open_case(pkg, tmp_models, case, 64)
    prompt = prompt_of(m)
    L, E = m.n_layer, m.n_embd
    vec = cc.case_vector(case, L, E)
    taps0, logits0 = taps_of(c, m, prompt)
    for l in sorted({1, L - 1}):
        # a buffer that holds layers 1 .. l alone, with every other row zero: layer l only
        only = np.zeros((l, E), np.float32)
        only[l - 1] = vec[l - 1]
        c.apply_cvec(only, 1, L)
        taps_a, logits_a = taps_of(c, m, prompt)
        # ... and the range [l, l] narrowed from the buffer that holds all layers
        c.apply_cvec(vec, l, l)
        taps_b, logits_b = taps_of(c, m, prompt)
        for taps in (taps_a, taps_b):
            for il in range(l):
                assert taps[il].tobytes() == taps0[il].tobytes(), (l, il)
            assert taps[l].tobytes() == (taps0[l] + vec[l - 1][None, :]).astype(np.float32).tobytes(), l
        assert logits_a.tobytes() == logits_b.tobytes() and logits_a.tobytes() != logits0.tobytes()
        for il in range(l + 1, L):                                       # (adding zeros: the same bits as a layer without a vector)
            assert taps_a[il].tobytes() == taps_b[il].tobytes()
    # layers beyond the buffer's length, and layers outside the range, are untouched
    c.apply_cvec(vec[:0].reshape(0, E), 1, L, n_embd=E)
    t, lg = taps_of(c, m, prompt)
    assert lg.tobytes() == logits0.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(t, taps0))
    c.apply_cvec(vec, L, L + 3)                                          # layer L does not exist, L - 1 is outside
    t, lg = taps_of(c, m, prompt)
    assert lg.tobytes() == logits0.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(t, taps0))
    c.apply_cvec(vec, 0, 0)                                              # layer 0 never has a vector
    t, lg = taps_of(c, m, prompt)
    assert lg.tobytes() == logits0.tobytes()
    c.close(); m.close()


def test_the_context_counts_the_buffer(pkg, tmp_models):
    case = cc.MODEL_CASES[0]
    base, m, c = open_case(pkg, tmp_models, case, 64)
    b0 = int(c.lib.mi355_context_device_bytes(c.h))
    c.apply_cvec(cc.case_vector(case, m.n_layer, m.n_embd), 1, m.n_layer)
    assert int(c.lib.mi355_context_device_bytes(c.h)) >= b0 + m.n_layer * m.n_embd * 4
    c.close(); m.close()


# ------------------------------------------------------------------------------------------------ against the composed reference
@pytest.mark.parametrize("rng_name", ["all", "middle"])
@pytest.mark.parametrize("case", cc.MODEL_CASES, ids=cc.MODEL_IDS)
def test_model_with_a_vector(pkg, tmp_models, case, rng_name):
    """A 9-token prompt, 4 teacher-forced single steps (captured steps: the add is inside the graph), then one batched step of 3 sequences: per-layer rows and
    logits against CvecRef at the bars of tests/test_gpu_lora.py."""
    oq.set_fa_v_acc_f32(1 if case.kv == "f16" else 0)
    try:
        base, m, c = open_case(pkg, tmp_models, case, 64)
        L, E = m.n_layer, m.n_embd
        vec = cc.case_vector(case, L, E)
        _, a, b = [r for r in cc.ranges(L) if r[0] == rng_name][0]
        c.apply_cvec(vec, a, b)
        ref = cc.reference(case, base, 64)
        ref.apply_cvec(vec, a, b)
        n = cc.N_PROMPT
        prompt = prompt_of(m)
        c.enable_taps(True)
        assert c.decode(prompt, np.arange(n)) == 0
        r = ref.decode(prompt, np.arange(n))[0]
        errs = [rel_err(c.layer_out(il, n).reshape(n, -1), ref.layer_out(il, n)) for il in range(L)]
        a1, b1 = c.layer_out(a, n).reshape(n, -1), ref.layer_out(a, n)                      # the first steered layer
        tok_err = np.abs(a1 - b1).max(axis=1) / max(1.0, float(np.abs(b1).max()))
        errs.append(rel_err(c.logits(), r))
        print("prompt errors:", errs, "median token error on the first steered layer:", float(np.median(tok_err)))
        assert max(errs) <= FLIP_TOL, errs
        assert c.argmax() == int(r.argmax()) or np.sort(r)[-1] - np.sort(r)[-2] <= 2 * FLIP_TOL * max(1.0, np.abs(r).max())
        if lc.tight_applies(case):
            assert float(np.median(tok_err)) <= TIGHT_TOL, (errs, tok_err)
        c.enable_taps(False)
        tok, mism, step_err = int(r.argmax()), 0, []
        for step in range(4):
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
        c.close()

        c = pkg.Context(m, n_ctx=128, n_seq_max=4, type_k=KV[case.kv], type_v=KV[case.kv])
        c.apply_cvec(vec, a, b)
        ref = cc.reference(case, base, 128)
        ref.apply_cvec(vec, a, b)
        rng = np.random.default_rng(17)
        lens = [7, 3, 5]
        for sq, ln in enumerate(lens):
            p = rng.integers(0, m.n_vocab, ln)
            fl = np.zeros(ln, np.int8); fl[-1] = 1
            assert c.decode(p, np.arange(ln), [sq] * ln, fl) == 0
            rr = ref.decode(p, np.arange(ln), [sq] * ln, fl)
            assert rel_err(c.logits(ln - 1), rr[0]) <= FLIP_TOL
        toks = [3, 5, 7]
        assert c.decode(toks, lens, [0, 1, 2], [1, 1, 1]) == 0
        rr = ref.decode(toks, lens, [0, 1, 2], [1, 1, 1])
        for j in range(3):
            assert rel_err(c.logits(j), rr[j]) <= FLIP_TOL, j
        c.close(); m.close()
    finally:
        oq.set_fa_v_acc_f32(0)


# ------------------------------------------------------------------------------------------------ neutrality
@pytest.mark.parametrize("case", cc.MODEL_CASES[:2] + cc.MODEL_CASES[3:], ids=cc.MODEL_IDS[:2] + cc.MODEL_IDS[3:])
def test_apply_then_clear_is_neutral(pkg, tmp_models, case):
    base, m, c = open_case(pkg, tmp_models, case, 64)
    L, E = m.n_layer, m.n_embd
    prompt = prompt_of(m)
    n = prompt.size

    def run():
        """prompt + 3 single steps from an empty cache: (every logits row, how far the one-launch counters moved)"""
        c.kv_clear()
        k0 = c.mega_steps() + c.engine_steps()
        rows = []
        assert c.decode(prompt, np.arange(n)) == 0
        rows.append(c.logits())
        for i in range(3):
            assert c.decode([5 + i], [n + i]) == 0
            rows.append(c.logits())
        return np.stack(rows), c.mega_steps() + c.engine_steps() - k0

    before, k_before = run()
    c.apply_cvec(cc.case_vector(case, L, E), 1, L)
    applied, k_applied = run()
    assert k_applied == 0                                               # neither one-launch path while a vector is applied
    assert rel_err(applied[-1], before[-1]) >= FLIP_TOL                 # (and the vector is applied)
    c.clear_cvec()
    after, k_after = run()
    assert after.tobytes() == before.tobytes()
    assert k_after == k_before                                          # they advance again where they advanced before
    c.clear_cvec()                                                      # clearing twice is no error
    # an applied all-zero vector: the taps of the plain run with taps, bit for bit
    taps0, lg0 = taps_of(c, m, prompt)
    c.apply_cvec(np.zeros((L - 1, E), np.float32), 1, L)
    taps1, lg1 = taps_of(c, m, prompt)
    assert lg1.tobytes() == lg0.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(taps1, taps0))
    c.close(); m.close()


EXPERIMENTS_LIB = os.path.join(ROOT, "cortex.llamacpp_amd", "lib", "libmi355_llama_experiments.so")


@pytest.mark.parametrize("option,cfg", [("decode_mega", "tiny-8b-2l"), ("decode_engine", "tiny-8b-3l")])
def test_one_launch_paths_stand_still_and_resume(be, pkg, tmp_models, option, cfg, request):
    """The single-launch step and the layer engine live in the experiments library (tests/test_gpu_model.py): where this process holds the product library the
    test runs in a child pytest on that one and passes or fails with it.  Their step counters advance before apply, stand still while a vector is applied
    (the steps then run the per-launch route, with the add), and advance again after clear - with the logits of before, bit for bit."""
    try:
        be.set_option(option, 1)
    except Exception as e:
        assert "MI355_BUILD_EXPERIMENTS" in str(e), e
        assert os.environ.get("MI355_LLAMA_LIB") != EXPERIMENTS_LIB and os.path.exists(EXPERIMENTS_LIB), e
        r = subprocess.run([sys.executable, "-m", "pytest", request.node.nodeid, "-q", "-p", "no:cacheprovider"], cwd=ROOT, capture_output=True, text=True,
                           timeout=600, env=dict(os.environ, MI355_LLAMA_LIB=EXPERIMENTS_LIB))
        assert r.returncode == 0 and "1 passed" in r.stdout, (r.stdout + r.stderr)[-6000:]
        return
    be.set_option("attn_out_fused", 0)      # (as the tests of these two paths in tests/test_gpu_model.py run them)
    try:
        path = str(tmp_models / f"{cfg}-q4_k_m-cvec.gguf")
        if not os.path.exists(path):
            pkg.gguf_synth.write_synthetic_llama(path, cfg, "q4_k_m", seed=11)
        m = pkg.Model(path)
        c = pkg.Context(m, n_ctx=128, type_k=8, type_v=8)
        counter = c.mega_steps if option == "decode_mega" else c.engine_steps
        prompt = np.random.default_rng(9).integers(0, m.n_vocab, 12)

        def run():
            c.kv_clear()
            k0 = counter()
            assert c.decode(prompt, np.arange(12)) == 0
            rows = [c.logits().copy()]
            for s in range(5):
                assert c.decode([int(rows[-1].argmax())], [12 + s]) == 0
                rows.append(c.logits().copy())
            return np.stack(rows), counter() - k0

        before, k_before = run()
        assert k_before == 5                                            # (the path under test really ran)
        c.apply_cvec(np.random.default_rng(2).standard_normal((m.n_layer - 1, m.n_embd)).astype(np.float32), 1, m.n_layer)
        applied, k_applied = run()
        assert k_applied == 0 and not np.array_equal(applied, before)
        c.clear_cvec()
        after, k_after = run()
        assert k_after == 5 and after.tobytes() == before.tobytes()
        c.close(); m.close()
    finally:
        be.set_option(option, 0 if option == "decode_mega" else -1)
        be.set_option("attn_out_fused", -1)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_context_unchanged(pkg, tmp_models):
    case = cc.MODEL_CASES[0]
    base, m, c = open_case(pkg, tmp_models, case, 64)
    L, E = m.n_layer, m.n_embd
    prompt = prompt_of(m)
    vec = cc.case_vector(case, L, E)
    c.apply_cvec(vec, 1, L)

    def logits():
        c.kv_clear()
        assert c.decode(prompt, np.arange(prompt.size)) == 0
        return c.logits().tobytes()

    want = logits()
    nan = vec.copy(); nan[0, 3] = np.nan
    inf = vec.copy(); inf[-1, 0] = np.inf
    err = lambda: (c.lib.mi355_last_error() or b"").decode()
    for data, size, ne, a, b, text in ((vec, vec.size, E + 32, 1, L, "is not the model's"), (vec, vec.size - 5, E, 1, L, "is not a multiple of n_embd"),
                                       (nan, nan.size, E, 1, L, "non-finite"), (inf, inf.size, E, 1, L, "non-finite"), (vec, vec.size, E, 2, 1, "il_start 2 > il_end 1")):
        rc = c.lib.mi355_apply_adapter_cvec(c.h, data.ctypes.data, size, ne, a, b)
        assert rc == -103 and text in err(), (rc, err())
        assert logits() == want, text
    assert c.lib.mi355_apply_adapter_cvec(None, vec.ctypes.data, vec.size, E, 1, L) == -103 and "null context" in err()
    c.close(); m.close()
    enc = str(tmp_models / "tiny-nomic-f16-cvec.gguf")
    pkg.gguf_synth.write_synthetic_llama(enc, "tiny-nomic", "f16")
    me = pkg.Model(enc)
    ce = pkg.Context(me, n_ctx=64)
    toks = np.arange(3, 9)
    assert ce.decode(toks, np.arange(6)) == 0
    e0 = ce.embeddings(-1).tobytes()
    v = np.ones((me.n_layer - 1, me.n_embd), np.float32)
    assert ce.lib.mi355_apply_adapter_cvec(ce.h, v.ctypes.data, v.size, me.n_embd, 1, me.n_layer) == -103
    assert "encoder" in (ce.lib.mi355_last_error() or b"").decode()
    assert ce.decode(toks, np.arange(6)) == 0 and ce.embeddings(-1).tobytes() == e0
    ce.close(); me.close()


# ------------------------------------------------------------------------------------------------ the power method
@pytest.mark.parametrize("R,E", cc.PCA_CASES, ids=cc.PCA_IDS)
def test_pca_direction(be, R, E):
    D, u, b0 = cc.pca_rows(R, E)
    u64, _ = cr.top_eigvec64(D)
    d, iters, dist = be.cvec_direction(D, b0, "pca", cc.PCA_ITERS, 16, 0.0)
    err = cr.one_minus_abs_cos(d, u64)
    print(f"1 - |cos| = {err:.3e} (M_PCA {cc.M_PCA:.3e}), last distance {dist:.3e}")
    assert iters == cc.PCA_ITERS                                         # tol = 0: never early
    assert err <= cc.M_PCA
    assert abs(float(np.linalg.norm(d.astype(np.float64))) - 1.0) < 1e-6
    assert float((D.astype(np.float64) @ d.astype(np.float64)).sum()) >= 0          # the sign rule
    if R == 1:
        assert cr.one_minus_abs_cos(d, D[0]) <= cc.M_PCA
    d2, _, _ = be.cvec_direction(D, b0, "pca", cc.PCA_ITERS, 16, 0.0)
    assert d2.tobytes() == d.tobytes()                                   # the same call twice: the same bytes
    dn, _, _ = be.cvec_direction(-D, b0, "pca", cc.PCA_ITERS, 64, 0.0)   # the rows negated: the same iterates, the other sign
    assert dn.tobytes() == (-d).tobytes()
    dm, it_m, _ = be.cvec_direction(D, None, "mean")
    assert cr.one_minus_abs_cos(dm, cr.mean_dir64(D)) <= cc.M_PCA and float(dm.astype(np.float64) @ cr.mean_dir64(D)) > 0


def test_pca_stops_at_tol(be):
    D, u, b0 = cc.pca_rows(67, 576)
    d, iters, dist = be.cvec_direction(D, b0, "pca", 1000, 4, 1e-5)
    assert iters % 4 == 0 and iters < 100 and dist < 1e-5
    assert cr.one_minus_abs_cos(d, cr.top_eigvec64(D)[0]) <= 1e-9


def test_pca_refusals(pkg, be):
    D, u, b0 = cc.pca_rows(3, 64)
    bad_nan = D.copy(); bad_nan[1, 5] = np.nan
    cases = [(D[:0], b0, "pca", "n_rows"), (np.zeros((3, 48), np.float32), np.ones(48, np.float32), "pca", "multiple of 32"), (bad_nan, b0, "pca", "non-finite"),
             (D, np.zeros(64, np.float32), "pca", "init is the zero vector"), (np.zeros((3, 64), np.float32), b0, "pca", "every row is zero"),
             (np.zeros((3, 64), np.float32), None, "mean", "every row is zero"), (D, b0, 7, "method")]
    for rows, init, method, text in cases:
        out = np.full(rows.shape[1], 7.0, np.float32)
        with pytest.raises(pkg.MI355Error, match=text) as ei:
            be.cvec_direction(rows, init, method, 8, 4, 0.0, dir_out=out)
        assert "(-103)" in str(ei.value) and (out == 7.0).all(), text
    # a start vector orthogonal to every row: the iteration reaches the zero vector
    one = np.zeros((1, 64), np.float32); one[0, 0] = 1.0
    init = np.zeros(64, np.float32); init[1] = 1.0
    out = np.full(64, 7.0, np.float32)
    with pytest.raises(pkg.MI355Error, match="zero vector"):
        be.cvec_direction(one, init, "pca", 8, 4, 0.0, dir_out=out)
    assert (out == 7.0).all()


# ------------------------------------------------------------------------------------------------ engine
GREEDY = dict(temperature=0.0, repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)


def test_engine_loadmodel_control_vectors(pkg, tmp_path_factory, tmp_models):
    import importlib.util
    spec = importlib.util.spec_from_file_location("cvector_generator", os.path.join(ROOT, "tools", "cvector_generator.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    gs = pkg.gguf_synth
    d = tmp_path_factory.mktemp("engcvec")
    path = str(d / "tiny-d128.gguf")
    gs.write_synthetic_llama(path, "tiny-d128", "q4_k_m", with_vocab=True)
    m = pkg.Model(path)
    L, E = m.n_layer, m.n_embd
    toks = m.tokenize("u:hello worlda:", add_special=True, parse_special=True)
    eos = m.lib.mi355_token_eos(m.h)
    n_predict = 8
    # the vector and its scale, on the CPU: the first of a few seeded directions and a doubling series of scales at which CvecRef's first token moves and is
    # no near tie (a tiny random model's top two logits are often closer than the bar the device is compared at)
    ref = cr.CvecRef(path, 64, 8, 8)
    r0 = ref.decode(toks, np.arange(len(toks)))[0]
    clear = lambda r: np.sort(r)[-1] - np.sort(r)[-2] > 2 * FLIP_TOL * max(1.0, float(np.abs(r).max()))
    scale = None
    for seed in range(6):
        unit = np.random.default_rng(0xE7 + seed).standard_normal((L - 1, E)).astype(np.float32)
        for s in (2.0, 4.0, 8.0, 16.0):
            ref = cr.CvecRef(path, 64, 8, 8)
            ref.apply_cvec(np.float32(s) * unit, 1, L)
            r1 = ref.decode(toks, np.arange(len(toks)))[0]
            if int(r1.argmax()) != int(r0.argmax()) and clear(r1):
                scale = s
                break
        if scale is not None:
            break
    assert scale is not None
    vfile = str(d / "cv.gguf")
    tool.write_cvec(vfile, {il: unit[il - 1] for il in range(1, L)}, "llama")

    # by hand: the same file through the loader, apply_cvec, greedy steps
    data, ne = pkg.Backend().load_control_vectors([(vfile, scale)])
    c = pkg.Context(m, n_ctx=256, type_k=8, type_v=8)
    c.apply_cvec(data, 1, L, n_embd=ne)
    assert c.decode(toks, np.arange(len(toks))) == 0
    tok, hand = c.argmax(), b""
    assert tok == int(r1.argmax()) != int(r0.argmax())
    for i in range(n_predict):
        if tok == eos:
            break
        hand += m.token_to_piece(tok)
        assert c.decode([tok], [len(toks) + i]) == 0
        tok = c.argmax()
    hand = hand.decode("utf-8", errors="replace")
    c.close(); m.close()

    msgs = [{"role": "user", "content": "hello world"}]
    common = dict(llama_model_path=path, ctx_len=256, n_parallel=1, cache_type="q8_0", user_prompt="u:", ai_prompt="a:", system_prompt="s:")

    def chat(**load):
        e = pkg.Engine()
        try:
            st, body = e.load_model(**common, **load)
            assert st["status_code"] == 200 and not st["has_error"], (st, body)
            st, body = e.chat_completion(model="tiny-d128", messages=msgs, max_tokens=n_predict, **GREEDY)[-1]
            assert st["status_code"] == 200 and not st["has_error"], (st, body)
            return body["choices"][0]["message"]["content"]
        finally:
            e.close()

    plain = chat()
    steered = chat(control_vectors=[{"path": vfile, "scale": scale}])
    assert steered != plain
    assert len(hand) > 0 and (steered.startswith(hand) or steered.startswith(hand.lstrip(" ")) or hand.startswith(steered) or hand.lstrip(" ").startswith(steered)), (steered, hand)
    ranged = chat(control_vectors=[vfile], control_vector_layer_range=[L, L])         # a path alone: scale 1; a range without a present layer: the plain text
    assert ranged == plain
    e = pkg.Engine()
    try:
        for load, needle in ((dict(control_vectors=[vfile], split_mode="row", split_ranks=2), "control_vectors"), (dict(control_vectors="x.gguf"), "control_vectors"),
                             (dict(control_vectors=[str(d / "missing.gguf")]), "missing.gguf"), (dict(control_vectors=[vfile], embedding=True), "embedding"),
                             (dict(control_vectors=[vfile], control_vector_layer_range=[1]), "control_vector_layer_range")):
            st, body = e.load_model(**common, **load)
            assert st == {"is_done": False, "has_error": True, "is_stream": False, "status_code": 500}, (load, st)
            assert body["message"] == "Failed to load model" and needle in body["error"], body
            assert e.get_models()[1]["data"] == []
        st, body = e.load_model(**common, control_vectors=[vfile], split_mode="row", split_ranks=2)
        assert "split_mode" in body["error"] and "row" in body["error"]
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ the tool
def test_the_tool_on_a_tiny_model(pkg, tmp_path):
    gs = pkg.gguf_synth
    path = str(tmp_path / "tiny.gguf")
    gs.write_synthetic_llama(path, "tiny-gqa4", "q4_k_m", with_vocab=True)
    pos, neg, out = str(tmp_path / "pos.txt"), str(tmp_path / "neg.txt"), str(tmp_path / "cv.gguf")
    open(pos, "w").write("hello world good\nthe sun is bright today\nyes\n")
    open(neg, "w").write("hello world bad\nthe night is dark\nno no no\n")
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tools", "cvector_generator.py"), "-m", path, "--positive-file", pos, "--negative-file", neg,
           "-o", out, "--pca-iter", "200", "--pca-batch", "20", "--seed", "3", "--ctx", "64", "--cache-type", "q8_0"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    be = pkg.Backend()
    data, ne = be.load_control_vectors([(out, 1.0)])
    m = pkg.Model(path)
    L, E = m.n_layer, m.n_embd
    assert ne == E and data.size == (L - 1) * E
    dirs = data.reshape(L - 1, E)
    assert np.allclose(np.linalg.norm(dirs.astype(np.float64), axis=1), 1.0, atol=1e-5)
    c = pkg.Context(m, n_ctx=64, type_k=8, type_v=8)
    prompt = np.asarray(m.tokenize("the sun is bright today", add_special=True, parse_special=True))

    def projection(scale):
        """the mean projection of the last layer's rows onto its direction"""
        if scale is None:
            c.clear_cvec()
        else:
            c.apply_cvec(np.float32(scale) * dirs, 1, L)
        taps, _ = taps_of(c, m, prompt)
        return float((taps[L - 1].astype(np.float64) @ dirs[L - 2].astype(np.float64)).mean())

    p0, up, down = projection(None), projection(4.0), projection(-4.0)
    print("projections:", down, p0, up)
    assert down < p0 < up
    c.close(); m.close()
