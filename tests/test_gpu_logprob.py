"""Context.token_logprobs / logits_kl / perplexity (csrc/logprob.hip behind mi355_get_token_logprobs, mi355_logits_kl, mi355_perplexity) on tiny synthetic
files: against float64 reductions of the same context's logits(i) rows at the per-op bar, against the procedure restated in Python (logprob_cases.perplexity_ref)
driven through decode / logits, against the CPU reference model at the full-forward bar, and tools/perplexity.py in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import logprob_cases as lc
import oracle_py as oq
import spec_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q8 = 8
N_CTX, N_UBATCH, N_CHUNK = 64, 8, 32
PAIRS = [("tiny-d128", 10), ("tiny-moe", 32)]
STAT_INTS = ("n_chunks", "count", "top1", "dead", "same_top", "has_base", "stopped")
STAT_SUMS = ("nll", "nll2", "nll_base", "nll2_base", "kl", "kl2")


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


@pytest.fixture(scope="module")
def pairs(pkg, tmp_models):
    """(cfg, seed) -> (target path, draft path, target Model, draft Model), loaded once"""
    cache = {}

    def get(key):
        if key not in cache:
            tgt, dft = sc.write_pair(pkg.gguf_synth, oq, tmp_models, *key)
            cache[key] = (tgt, dft, pkg.Model(tgt), pkg.Model(dft))
        return cache[key]
    yield get
    for _, _, mt, md in cache.values():
        mt.close(); md.close()


def ctx_of(pkg, model, **kw):
    return pkg.Context(model, n_ctx=N_CTX, n_ubatch=N_UBATCH, type_k=Q8, type_v=Q8, **kw)


def gpu_fns(c):
    V = c.model.n_vocab

    def rows(tk, pos, flags):
        assert c.decode(tk, pos, logits=flags) == 0
        at = np.flatnonzero(flags)
        return np.stack([c.logits(int(i)) for i in at]) if at.size else np.zeros((0, V), np.float32)
    return rows, lambda: c.kv_seq_rm(0, 0, -1)


def tokens_of(n_vocab, n, seed=11):
    return np.random.default_rng(seed).integers(0, n_vocab, n).astype(np.int32)


def check_stats(got, ref, with_base, lse=1.0):
    """The counters equal; a sum of `count` terms each within its op bar of the reference: |d sum x| <= TIGHT_TOL (L count + |sum|) with L = 1 for a
    log-probability and max(1, |lse|) for a divergence, and, from d(x^2) ~ 2 |x| dx and |x| <= 1 + x^2, |d sum x^2| <= 2 TIGHT_TOL (L (count + sum x^2) + sum x^2)."""
    for k in STAT_INTS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    n = ref["count"]
    for k in STAT_SUMS if with_base else STAT_SUMS[:2]:
        L = max(1.0, lse) if k.startswith("kl") else 1.0
        bar = 2 * lc.TIGHT_TOL * (L * (n + abs(ref[k])) + abs(ref[k])) if k.endswith("2") else lc.TIGHT_TOL * (L * n + abs(ref[k]))
        assert abs(got[k] - ref[k]) <= bar * (1 + 1e-3), (k, got[k], ref[k], bar)


@pytest.mark.parametrize("to_host", [False, True])
def test_token_logprobs_over_three_micro_batches(be, pkg, pairs, to_host):
    """20 rows with n_ubatch 8 span three micro-batches; the device log-probabilities equal the float64 log-softmax of the same context's logits(i) at the op
    bar with logits_to_host 0 and 1, also after a single-token step, and logits() returns the same rows before and after."""
    _, _, mt, _ = pairs(PAIRS[0])
    c = ctx_of(pkg, mt, logits_to_host=to_host)
    tk = tokens_of(mt.n_vocab, 21, seed=5)
    assert c.decode(tk[:20], np.arange(20), logits=[1] * 20) == 0
    before = np.stack([c.logits(i) for i in range(20)])                                # (with logits_to_host 0 the rows are copied when first asked for)
    order = np.random.default_rng(1).permutation(20)[:17]                              # any rows, any order, a row twice
    order = np.concatenate([order, order[:2]]).astype(np.int32)
    tg = np.concatenate([tk[order[:10] + 1], [0, mt.n_vocab - 1], np.arange(7)]).astype(np.int32)
    lp, rank = c.token_logprobs(order, tg)
    rows = np.stack([c.logits(i) for i in range(20)])
    assert rows.tobytes() == before.tobytes()
    ref, ref_rank = lc.token_logprob_ref(rows[order], tg)
    err = float((np.abs(lp - ref) / np.maximum(1.0, np.abs(ref))).max())
    print(f"to_host={to_host}: max |logprob - ref| / max(1, |ref|) {err:.3g} over {tg.size} rows")
    assert rank.tolist() == ref_rank.tolist() and lc.logprob_ok(lp, ref).all(), (lp, ref)
    am = np.array([sc.argmax_rule(r) for r in rows], np.int32)                            # the arg-max of every row has rank 0
    assert c.token_logprobs(np.arange(20), am)[1].tolist() == [0] * 20
    lp2, rank2 = c.token_logprobs(order, tg)
    assert lp2.tobytes() == lp.tobytes() and rank2.tobytes() == rank.tobytes()
    assert np.stack([c.logits(i) for i in range(20)]).tobytes() == rows.tobytes()
    # a single-token step: row -1
    assert c.decode([tk[20]], [20]) == 0
    lp1, rank1 = c.token_logprobs([-1], [7])
    ref1, ref_rank1 = lc.token_logprob_ref(c.logits(), [7])
    assert rank1.tolist() == ref_rank1.tolist() and lc.logprob_ok(lp1, ref1).all()
    c.close()


def test_refusals_say_which(be, pkg, pairs, tmp_models):
    _, _, mt, md = pairs(PAIRS[0])
    Err = pkg.binding.MI355Error
    a, b = ctx_of(pkg, mt, logits_to_host=False), ctx_of(pkg, md, logits_to_host=False)
    tk = tokens_of(mt.n_vocab, 6)
    for c in (a, b):
        assert c.decode(tk, np.arange(6), logits=[1, 1, 0, 1, 1, 1]) == 0
    with pytest.raises(Err, match="not flagged"):
        a.token_logprobs([1, 2], [3, 4])
    with pytest.raises(Err, match="not flagged"):
        a.token_logprobs([6], [3])
    with pytest.raises(Err, match=r"target .* outside"):
        a.token_logprobs([0, 1], [3, mt.n_vocab])
    with pytest.raises(Err, match=r"target .* outside"):
        a.token_logprobs([0], [-1])
    with pytest.raises(Err, match="not flagged"):
        a.logits_kl(b, [0, 2], [0, 1])
    with pytest.raises(Err, match="not flagged"):
        a.logits_kl(b, [0, 1], [2, 1])
    with pytest.raises(Err, match="same context"):
        a.logits_kl(a, [0], [0])
    kl, top = a.logits_kl(b, [0, 1], [0, 1])                                              # (the well-formed call goes through)
    assert np.isfinite(kl).all() and set(top.tolist()) <= {0, 1}
    # another vocabulary: tiny-gqa4 has 768 tokens, tiny-d128 512
    other_path = os.path.join(str(tmp_models), "logprob-tiny-gqa4-q8_0.gguf")
    pkg.gguf_synth.write_synthetic_llama(other_path, "tiny-gqa4", "q8_0", seed=3)
    other = pkg.Model(other_path)
    assert other.n_vocab == 768 and mt.n_vocab == 512
    m = ctx_of(pkg, other, logits_to_host=False)
    assert m.decode(tk, np.arange(6), logits=[1] * 6) == 0
    with pytest.raises(Err, match="n_vocab differs"):
        a.logits_kl(m, [0], [0])
    with pytest.raises(Err, match="n_vocab differs"):
        m.logits_kl(a, [0], [0])
    with pytest.raises(Err, match="n_vocab differs"):
        a.perplexity(tokens_of(mt.n_vocab, 64), 32, base=m)
    with pytest.raises(Err, match="n_vocab differs"):
        m.perplexity(tokens_of(mt.n_vocab, 64), 32, base=a)
    assert a.kv_used() == 6 and m.kv_used() == 6                                          # (a refused run touches neither cache)
    m.close(); other.close()
    with pytest.raises(Err, match="n_chunk"):
        a.perplexity(tokens_of(mt.n_vocab, 200), N_CTX + 1)
    with pytest.raises(Err, match="n_chunk"):
        a.perplexity(tokens_of(mt.n_vocab, 200), 1)
    with pytest.raises(Err, match="same context"):
        a.perplexity(tokens_of(mt.n_vocab, 64), 32, base=a)
    a.set_embeddings(True); b.set_embeddings(True)
    assert a.decode(tk[:2], [6, 7], logits=[1, 1]) == 0 and b.decode(tk[:2], [6, 7], logits=[1, 1]) == 0
    with pytest.raises(Err, match="embeddings"):
        a.token_logprobs([0], [3])
    with pytest.raises(Err, match="embeddings"):
        b.logits_kl(a, [0], [0])
    a.close(); b.close()


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_perplexity_equals_the_procedure_in_python_and_the_reference_model(be, pkg, pairs, pair):
    tgt, _, mt, _ = pairs(pair)
    tokens = tokens_of(mt.n_vocab, 3 * N_CHUNK + 9)
    c = ctx_of(pkg, mt, logits_to_host=False)
    seen = []
    got = c.perplexity(tokens, N_CHUNK, bos=1, callback=lambda st: seen.append((st["n_chunks"], st["count"])) and False)
    assert got["count"] == 45 and got["n_chunks"] == 3 and got["dead"] == 0 and got["stopped"] == 0 and seen == [(1, 15), (2, 30), (3, 45)]
    assert c.kv_used() == 0
    # (a) the same context driven from Python: decode, logits(i), float64
    h = ctx_of(pkg, mt)
    fn, clear = gpu_fns(h)
    ref = lc.perplexity_ref(fn, tokens, N_CHUNK, bos=1, n_ubatch=N_UBATCH, clear_fn=clear)
    err = float((np.abs(got["logprobs"] - ref["logprobs"]) / np.maximum(1.0, np.abs(ref["logprobs"]))).max())
    print(f"{pair}: PPL {got['ppl']:.4f}; max |logprob - ref| / max(1, |ref|) {err:.3g}; top-1 {got['top1']} of {got['count']}")
    assert lc.logprob_ok(got["logprobs"], ref["logprobs"]).all()
    check_stats(got, ref, False)
    assert got["ppl"] == pytest.approx(np.exp(ref["nll"] / 45), rel=2 * lc.TIGHT_TOL * (1 + ref["nll"] / 45))          # (d ppl / ppl = d mean nll)
    # (b) the CPU reference model: a log-softmax moves by at most twice the max-norm change of its row
    side = sc.OracleSide(oq, tgt, N_CTX, oq.Q8_0)
    scale = [1.0]

    def cpu_rows(tk, pos, flags):
        r = side.c.decode(tk, pos, None, flags)
        if r.size:
            scale[0] = max(scale[0], float(np.abs(r).max()))
        return r
    cpu = lc.perplexity_ref(cpu_rows, tokens, N_CHUNK, bos=1, n_ubatch=N_UBATCH, clear_fn=lambda: side.c.kv_seq_rm(0, 0, -1))
    side.close()
    bound = 2 * lc.FLIP_TOL * scale[0]
    d = np.abs(got["logprobs"] - cpu["logprobs"])
    print(f"{pair}: against the CPU reference model max |d logprob| {d.max():.3g}, mean nll {got['nll'] / 45:.5f} vs {cpu['nll'] / 45:.5f}, bound {bound:.3g}")
    assert d.max() <= bound and abs(got["nll"] - cpu["nll"]) / 45 <= bound
    # the callback stops the run after chunk 1; the sequence is gone afterwards all the same
    part = c.perplexity(tokens, N_CHUNK, bos=1, callback=lambda st: True)
    assert part["n_chunks"] == 1 and part["count"] == 15 and part["stopped"] == 1 and c.kv_used() == 0
    assert part["logprobs"].tobytes() == got["logprobs"][:15].tobytes()
    c.close(); h.close()


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_perplexity_with_a_base_model(be, pkg, pairs, pair):
    """The coarser-rounded twin as the model under test, the file it was made from as the base."""
    _, _, mt, md = pairs(pair)
    tokens = tokens_of(mt.n_vocab, 2 * N_CHUNK, seed=7)
    q, p = ctx_of(pkg, md, logits_to_host=False), ctx_of(pkg, mt, logits_to_host=False)
    got = q.perplexity(tokens, N_CHUNK, bos=1, base=p)
    assert got["count"] == 30 and got["has_base"] == 1 and q.kv_used() == 0 and p.kv_used() == 0
    hq, hp = ctx_of(pkg, md), ctx_of(pkg, mt)
    fq, cq = gpu_fns(hq)
    fp, cp = gpu_fns(hp)
    kl_rows = []

    def base_rows(tk, pos, flags):
        r = fp(tk, pos, flags)
        kl_rows.append(r)
        return r
    q_rows = []

    def self_rows(tk, pos, flags):
        r = fq(tk, pos, flags)
        q_rows.append(r)
        return r
    ref = lc.perplexity_ref(self_rows, tokens, N_CHUNK, bos=1, n_ubatch=N_UBATCH, base_rows_fn=base_rows, clear_fn=lambda: (cq(), cp()))
    P, Q = np.concatenate(kl_rows), np.concatenate(q_rows)
    kref, tref, lse_p, lse_q = lc.kl_ref(P, Q)
    assert np.array_equal(kref, ref["kls"])
    rel = np.abs(got["kls"] - kref) / lc.kl_bar(kref, lse_p, lse_q)
    print(f"{pair}: mean KL {got['mean_kl']:.4f} (ref {kref.mean():.4f}); max |KL - ref| / max(1, |lse|, |ref|) {rel.max() * lc.TIGHT_TOL:.3g}; "
          f"same top {got['same_top']} of 30; PPL {got['ppl']:.3f} base {got['ppl_base']:.3f}")
    assert (rel <= 1.0).all()
    assert lc.logprob_ok(got["logprobs"], ref["logprobs"]).all()
    check_stats(got, ref, True, lse=float(max(np.abs(lse_p).max(), np.abs(lse_q).max())))
    assert got["mean_kl"] > 0.05 and got["same_top"] == int(tref.sum())
    # a second context of the target file as the base of the first: nothing but rounding between them
    p2 = ctx_of(pkg, mt, logits_to_host=False)
    same = p.perplexity(tokens, N_CHUNK, bos=1, base=p2)
    lse = max(1.0, float(np.abs(lse_p).max()))
    print(f"{pair}: target against itself: mean |KL| {np.abs(same['kls']).mean():.3g}, same top {same['same_top']} of 30")
    assert np.abs(same["kls"]).mean() <= lc.TIGHT_TOL * lse and same["same_top"] == 30
    assert same["nll"] == pytest.approx(same["nll_base"], rel=lc.TIGHT_TOL)
    for c in (q, p, p2, hq, hp):
        c.close()


def test_the_tool_in_a_child_process(be, pkg, pairs, tmp_path):
    tgt, dft, mt, md = pairs(PAIRS[0])
    tokens = tokens_of(mt.n_vocab, 3 * N_CHUNK, seed=9)
    tok_path, out_path = str(tmp_path / "tokens.npy"), str(tmp_path / "ppl.json")
    np.save(tok_path, tokens)
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tools", "perplexity.py"), "-m", dft, "--base", tgt, "--tokens", tok_path, "--ctx", str(N_CHUNK),
           "--ubatch", str(N_UBATCH), "--cache-type", "q8_0", "--chunks", "2", "--json", out_path]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[1]" in r.stdout and "[2]" in r.stdout and "[3]" not in r.stdout and "PPL = " in r.stdout and "mean KLD = " in r.stdout and "s per chunk" in r.stdout
    out = json.load(open(out_path))
    q, p = (pkg.Context(m, n_ctx=N_CHUNK, n_batch=N_UBATCH, n_ubatch=N_UBATCH, type_k=Q8, type_v=Q8, logits_to_host=False) for m in (md, mt))      # the tool's contexts
    bos = out["bos"]
    want = q.perplexity(tokens[:2 * N_CHUNK], N_CHUNK, bos=bos, base=p)
    for k in STAT_INTS + STAT_SUMS:
        assert out[k] == want[k], (k, out[k], want[k])
    assert out["count"] == 30 and out["ppl"] == pytest.approx(want["ppl"], rel=1e-12) and out["mean_kl"] == pytest.approx(want["mean_kl"], rel=1e-12)
    q.close(); p.close()
