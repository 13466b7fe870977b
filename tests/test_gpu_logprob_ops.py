"""The two kernels of csrc/logprob.hip through their test entries, against the float64 references of logprob_cases.py: ranks, arg-max agreement, dead rows and
-inf exact; log-probabilities within TIGHT_TOL * max(1, |ref|); divergences within TIGHT_TOL * max(1, |lse_p|, |lse_q|, |ref|); the same bits run to run.
test_logprob_cpu.py shows that f32 arithmetic in the kernels' part and fold order meets both bars on these inputs."""
import numpy as np
import pytest

import logprob_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


@pytest.mark.parametrize("rows", lc.OP_ROWS)
@pytest.mark.parametrize("n", lc.OP_NS)
def test_token_logprob_rows(be, n, rows):
    base, idx, tg = lc.logprob_op_case(n, rows)
    ref, ref_rank = lc.token_logprob_ref(base[idx], tg)
    got, got_rank = be.token_logprob_rows(base, tg, rows=idx)
    assert got_rank.tolist() == ref_rank.tolist()
    fin = np.isfinite(ref)
    err = float((np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))).max()) if fin.any() else 0.0
    print(f"n={n} rows={rows} launch rows {tg.size}: max |logprob - ref| / max(1, |ref|) {err:.3g}; dead {int(np.isnan(ref).sum())} -inf {int(np.isinf(ref).sum())}")
    ok = lc.logprob_ok(got, ref)
    assert ok.all(), (np.flatnonzero(~ok), got[~ok], ref[~ok])
    again, again_rank = be.token_logprob_rows(base, tg, rows=idx)
    assert again.tobytes() == got.tobytes() and again_rank.tobytes() == got_rank.tobytes()          # the same bits run to run
    if rows == 17:
        assert np.isnan(ref).any() and (ref_rank == 0).any() and (n == 1 or (np.isinf(ref).any() and (ref_rank > 0).any()))
    # rows == nullptr: launch row r is base row r
    plain, plain_rank = be.token_logprob_rows(base[idx[:3]], tg[:3])
    assert lc.logprob_ok(plain, ref[:3]).all() and plain_rank.tolist() == got_rank[:3].tolist()       # (another row start: the walk's head differs, so not the same bits)


@pytest.mark.parametrize("rows", lc.OP_ROWS)
@pytest.mark.parametrize("n", lc.OP_NS)
def test_logits_kl_rows(be, n, rows):
    P, Q, rp, rq = lc.kl_op_case(n, rows)
    ref, ref_top, lse_p, lse_q = lc.kl_ref(P[rp], Q[rq])
    got, got_top = be.logits_kl_rows(P, Q, rp, rq)
    assert got_top.tolist() == ref_top.tolist()
    dead = np.isnan(ref)
    assert np.isnan(got[dead]).all()
    live = ~dead
    rel = np.abs(got[live] - ref[live]) / lc.kl_bar(ref[live], lse_p[live], lse_q[live]) if live.any() else np.zeros(0)
    print(f"n={n} rows={rows}: max |KL - ref| / max(1, |lse_p|, |lse_q|, |ref|) {(rel.max() if rel.size else 0.0) * lc.TIGHT_TOL:.3g}; largest KL {np.nanmax(np.r_[ref, 0.0]):.3g}")
    assert (rel <= 1.0).all(), (rel, got[live], ref[live])
    same = np.arange(rows) % lc.KL_KINDS == 0
    assert (got[same] == 0.0).all() and (got_top[same] == 1).all()                                  # identical rows: exactly 0
    again, again_top = be.logits_kl_rows(P, Q, rp, rq)
    assert again.tobytes() == got.tobytes() and again_top.tobytes() == got_top.tobytes()
    if rows == 17 and n >= 256:
        k = np.arange(rows) % lc.KL_KINDS
        assert (ref[k == 3] > 40).all() and (ref_top[k == 3] == 0).all() and (ref_top[k == 4] == 1).all() and (ref_top[k == 5] == 0).all()
        assert (ref_top[(k == 6) | (k == 7)] == -1).all() and (np.abs(ref[k == 1]) < 1e-5).all()
