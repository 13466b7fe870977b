"""Perplexity and KL divergence without a GPU: the references of logprob_cases.py on hand-made rows, the f32 twin of the kernels' part and fold order against the
op bars on every input the GPU op tests use (a bar the twin cannot meet must not be asked of the kernel), the procedure on the CPU reference model, the pair's
divergence, and the new C-ABI entries' answer on a machine with no device."""
import ctypes as C

import numpy as np
import pytest

import logprob_cases as lc
import oracle_py as oq
import spec_cases as sc

PAIR = ("tiny-d128", 10)


def test_logprob_rule_on_hand_made_rows():
    """A check of the REFERENCE, not of the kernel: it passes without the feature."""
    inf, nan = np.inf, np.nan
    x = np.array([[1.0, 3.0, 3.0, 2.0], [nan, 2.0, nan, 2.0], [nan, nan, nan, nan], [-inf, -inf, -inf, -inf], [0.0, inf, 1.0, nan], [5.0, 5.0, 5.0, 5.0],
                  [-inf, 0.0, -inf, nan]], np.float32)
    top = [sc.argmax_rule(r) for r in x]
    lp, rank = lc.token_logprob_ref(x, top)
    _, p = sc.argmax_prob_ref(x)
    live = [0, 1, 5, 6]
    assert np.allclose(lp[live], np.log(p[live]), rtol=0, atol=1e-12)                 # the logprob of the arg-max is log(argmax_prob)
    assert rank[live].tolist() == [0, 0, 0, 0]
    assert np.isnan(lp[[2, 3, 4]]).all() and rank[[2, 3, 4]].tolist() == [-1, -1, -1]   # all NaN, all -inf, a +inf entry
    # rank == 0 exactly where argmax_rule names the target; ties resolve to the lower index
    for r in live:
        for t in range(4):
            l1, k1 = lc.token_logprob_ref(x[r], [t])
            if np.isnan(x[r, t]):
                assert np.isnan(l1[0]) and k1[0] == -1                                  # a NaN target: dead
            else:
                assert (k1[0] == 0) == (t == top[r]), (r, t, k1)
    assert lc.token_logprob_ref(x[0], [2])[1][0] == 1 and lc.token_logprob_ref(x[0], [0])[1][0] == 3
    l6, k6 = lc.token_logprob_ref(x[6], [0])                                            # -inf under a finite maximum: -inf and the count
    assert l6[0] == -inf and k6[0] == 1
    assert lc.token_logprob_ref(x[6], [2])[1][0] == 2                                   # an equal -inf at a lower index beats it too


def test_kl_rule_on_hand_made_rows():
    """A check of the REFERENCE, not of the kernel: it passes without the feature."""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((6, 300)) * 3).astype(np.float32)
    y = (rng.standard_normal((6, 300)) * 3).astype(np.float32)
    kl, top, _, _ = lc.kl_ref(x, x)
    assert (kl == 0.0).all() and (top == 1).all()
    kl, top, _, _ = lc.kl_ref(x, x + np.float32(2.0))
    assert np.abs(kl).max() < 1e-6 and (top == 1).all()
    kl, top, _, _ = lc.kl_ref(x, y)
    assert (kl > 0).all()
    a = np.array([0.0, np.log(3.0)], np.float32); b = np.array([0.0, 0.0], np.float32)     # P = (1/4, 3/4), Q = (1/2, 1/2)
    assert lc.kl_ref(a, b)[0][0] == pytest.approx(0.25 * np.log(0.5) + 0.75 * np.log(1.5), abs=1e-7)
    y[1, 5] = np.nan; x[2, 7] = np.inf
    kl, top, _, _ = lc.kl_ref(x, y)
    assert np.isnan(kl[[1, 2]]).all() and top[[1, 2]].tolist() == [-1, -1] and np.isfinite(kl[[0, 3, 4, 5]]).all()


@pytest.mark.parametrize("n", lc.OP_NS)
def test_f32_twin_meets_the_op_bars(n):
    """The kernels' arithmetic - f32 throughout, 64 part pairs folded in part order - restated in numpy meets the bars the GPU op tests ask for, on their inputs."""
    worst_lp = worst_kl = 0.0
    for rows in lc.OP_ROWS:
        base, idx, tg = lc.logprob_op_case(n, rows)
        ref, ref_rank = lc.token_logprob_ref(base[idx], tg)
        got, got_rank = lc.token_logprob_twin(base[idx], tg)
        assert got_rank.tolist() == ref_rank.tolist()
        ok = lc.logprob_ok(got, ref)
        assert ok.all(), (n, rows, np.flatnonzero(~ok), got[~ok], ref[~ok])
        fin = np.isfinite(ref)
        if fin.any():
            worst_lp = max(worst_lp, float((np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))).max()))
        P, Q, rp, rq = lc.kl_op_case(n, rows)
        kref, tref, lp_, lq_ = lc.kl_ref(P[rp], Q[rq])
        kgot, tgot = lc.kl_twin(P[rp], Q[rq])
        assert tgot.tolist() == tref.tolist()
        dead = np.isnan(kref)
        assert np.isnan(kgot[dead]).all()
        if (~dead).any():
            rel = np.abs(kgot[~dead] - kref[~dead]) / lc.kl_bar(kref[~dead], lp_[~dead], lq_[~dead])
            assert (rel <= 1.0).all(), (n, rows, rel, kgot[~dead], kref[~dead])
            worst_kl = max(worst_kl, float(rel.max()) * lc.TIGHT_TOL)
        same = np.flatnonzero((np.arange(rows) % lc.KL_KINDS == 0))
        assert (kgot[same] == 0.0).all() and (tgot[same] == 1).all()
    print(f"n={n}: twin max logprob err / max(1, |ref|) {worst_lp:.3g}; max KL err / max(1, |lse|, |ref|) {worst_kl:.3g}")


@pytest.fixture(scope="module")
def pair(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("logprob")
    tgt, dft = sc.write_pair(pkg.gguf_synth, oq, d, *PAIR)
    T, D = sc.OracleSide(oq, tgt, 64, oq.Q8_0), sc.OracleSide(oq, dft, 64, oq.Q8_0)
    yield T, D
    T.close(); D.close()


def oracle_fns(side):
    def rows(tk, pos, flags):
        return side.c.decode(tk, pos, None, flags)
    return rows, lambda: side.c.kv_seq_rm(0, 0, -1)


def test_perplexity_procedure_on_the_reference_model(pair):
    T, _ = pair
    V = T.m.n_vocab
    tokens = np.random.default_rng(11).integers(0, V, 3 * 32 + 9).astype(np.int32)      # 3 chunks of 32 and a tail of 9 that is dropped
    bos = 1
    fn, clear = oracle_fns(T)
    st = lc.perplexity_ref(fn, tokens, 32, bos=bos, n_ubatch=8, clear_fn=clear)
    assert st["n_chunks"] == 3 and st["count"] == 3 * 15 and st["dead"] == 0 and st["logprobs"].size == 45
    # the direct computation: one all-rows decode per chunk, the first token overwritten by bos
    direct, scale = [], 1.0
    for c in range(3):
        clear()
        tk = tokens[c * 32:(c + 1) * 32].copy()
        tk[0] = bos
        rows = T.c.decode(tk, np.arange(32), None, np.ones(32, np.int8))
        lp, _ = lc.token_logprob_ref(rows[16:31], tk[17:32])
        direct.append(lp)
        scale = max(scale, float(np.abs(rows[16:31]).max()))
    direct = np.concatenate(direct)
    # (pieces of 8 against one batch of 32: the rows move by batch-size rounding only, and a log-softmax by at most twice the max-norm change of its row)
    assert np.abs(st["logprobs"] - direct).max() <= 2 * lc.FLIP_TOL * scale
    assert st["nll"] == pytest.approx(-st["logprobs"].sum(), rel=1e-12) and st["nll2"] == pytest.approx((st["logprobs"] ** 2).sum(), rel=1e-12)
    whole = lc.perplexity_ref(fn, tokens, 32, bos=bos, clear_fn=clear)                    # one piece per chunk: exactly the direct computation
    assert np.array_equal(whole["logprobs"], direct)
    # bos matters: without the overwrite the first chunk's rows differ
    nobos = lc.perplexity_ref(fn, tokens, 32, bos=-1, clear_fn=clear)
    assert tokens[0] != bos and not np.array_equal(nobos["logprobs"][:15], whole["logprobs"][:15])
    # the tail is dropped: the same tokens without it give the same result
    cut = lc.perplexity_ref(fn, tokens[:96], 32, bos=bos, clear_fn=clear)
    assert np.array_equal(cut["logprobs"], whole["logprobs"])
    stopped = lc.perplexity_ref(fn, tokens, 32, bos=bos, clear_fn=clear, stop_after=1)
    assert stopped["n_chunks"] == 1 and stopped["count"] == 15 and stopped["stopped"] == 1


# (cfg, seed) -> (min, mean) of the per-row KL(target || draft) over KL_TOKENS, measured on the CPU reference model
KL_TOKEN_SEED = 7
KL_PAIRS = {("tiny-d128", 10): (0.13, 2.96), ("tiny-gqa4", 3): (0.19, 3.31), ("tiny-moe", 32): (0.12, 4.24)}


@pytest.mark.parametrize("cfg_seed", list(KL_PAIRS), ids=lambda c: f"{c[0]}-{c[1]}")
def test_draft_against_target_kl_is_well_clear_of_zero(pkg, tmp_path_factory, cfg_seed):
    """What entitles the GPU test to ask for a mean KL above 0.05 on these pairs: 64 tokens (default_rng(7)), every row, target as P and draft as Q."""
    d = tmp_path_factory.mktemp("logprob-kl")
    tgt, dft = sc.write_pair(pkg.gguf_synth, oq, d, *cfg_seed)
    T, D = sc.OracleSide(oq, tgt, 64, oq.Q8_0), sc.OracleSide(oq, dft, 64, oq.Q8_0)
    tokens = np.random.default_rng(KL_TOKEN_SEED).integers(0, T.m.n_vocab, 64).astype(np.int32)
    rt = T.c.decode(tokens, np.arange(64), None, np.ones(64, np.int8))
    rd = D.c.decode(tokens, np.arange(64), None, np.ones(64, np.int8))
    T.close(); D.close()
    kl, top, _, _ = lc.kl_ref(rt, rd)
    print(f"{cfg_seed}: KL(target || draft) min {kl.min():.3g} mean {kl.mean():.3g} same top {top.mean():.2f}")
    assert kl.min() > 0.05
    want_min, want_mean = KL_PAIRS[cfg_seed]
    assert kl.min() == pytest.approx(want_min, abs=0.006) and kl.mean() == pytest.approx(want_mean, abs=0.006)


def test_new_entries_answer_without_a_device(pkg):
    """On a machine without a GPU every new entry answers MI355_ERR_NO_DEVICE (-100); with one, the argument checks answer.  Fails without the feature."""
    lib = pkg.load_library()
    for name in ("mi355_get_token_logprobs", "mi355_logits_kl", "mi355_perplexity", "mi355_op_token_logprob_rows", "mi355_op_logits_kl_rows"):
        assert hasattr(lib, name) and name in pkg.binding.SYMBOLS, name
    has_gpu = lib.mi355_device_count() > 0
    x = np.zeros((2, 8), np.float32); lp = np.zeros(2, np.float32); rk = np.zeros(2, np.int32)
    rows = np.array([0, 1], np.int32); tg = np.array([3, 4], np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    r1 = lib.mi355_op_token_logprob_rows(vp(x), 8, 2, vp(rows), vp(tg), 2, vp(lp), vp(rk))
    r2 = lib.mi355_op_logits_kl_rows(vp(x), 2, vp(x), 2, 8, vp(rows), vp(rows), 2, vp(lp), vp(rk))
    r3 = lib.mi355_get_token_logprobs(None, 2, vp(rows), vp(tg), vp(lp), vp(rk))
    r4 = lib.mi355_logits_kl(None, None, 2, vp(rows), vp(rows), vp(lp), vp(rk))
    st = pkg.binding.PplStats()
    r5 = lib.mi355_perplexity(None, None, vp(tg), 2, 2, -1, 0, None, None, None, None, C.byref(st))
    if has_gpu:
        assert (r1, r2) == (0, 0) and r3 == r4 == r5 == -103
        assert lp.tolist() == [0.0, 0.0] and rk.tolist() == [1, 1]
    else:
        assert r1 == r2 == r3 == r4 == r5 == -100
    assert C.sizeof(pkg.binding.PplStats) == 5 * 8 + 2 * 4 + 6 * 8
