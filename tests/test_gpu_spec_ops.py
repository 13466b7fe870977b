"""The two kernels of a speculative round (csrc/spec.hip) through their test entries, against the numpy restatement of their rules (spec_cases.py):
indices and acceptance counts exact, the probability within the per-op float bar against float64."""
import numpy as np
import pytest

import spec_cases as sc

pytestmark = pytest.mark.gpu

TIGHT_TOL = 2e-5          # the project's per-op float bar (test_gpu_model.py)
N_KINDS = 11


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def special_rows(n: int, rows: int, seed: int) -> np.ndarray:
    """Row r is of kind r % 11: plain; ties at the first and last index; a tie across the boundary of the first two parts; NaNs, one of them where the maximum
    was; -inf entries; all NaN; all -inf; a +inf entry; one dominant logit (p ~ 1); flat (p = 1 / n); plain at another scale."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, n)) * 3.0).astype(np.float32)
    chunk = (n + 63) // 64
    for r in range(rows):
        kind, row = r % N_KINDS, x[r]
        top = np.float32(row.max() + 1.0)
        if kind == 1:
            row[0] = row[n - 1] = top
        elif kind == 2 and n > chunk:
            row[chunk - 1] = row[chunk] = top
        elif kind == 3:
            row[int(row.argmax())] = np.nan
            row[rng.integers(0, n, max(1, n // 7))] = np.nan
        elif kind == 4:
            row[rng.integers(0, n, max(1, n // 5))] = -np.inf
        elif kind == 5:
            row[:] = np.nan
        elif kind == 6:
            row[:] = -np.inf
        elif kind == 7:
            row[int(rng.integers(0, n))] = np.inf
        elif kind == 8:
            row[int(rng.integers(0, n))] = np.float32(60.0)
        elif kind == 9:
            row[:] = np.float32(1.5)
        elif kind == 10:
            row *= np.float32(0.05)
    return x


@pytest.mark.parametrize("rows", [1, 3, 17])
@pytest.mark.parametrize("n", [1, 31, 256, 257, 1000, 32000, 151936])
def test_argmax_prob_rows(be, n, rows):
    x = special_rows(n, rows, 1000 * rows + n % 997)
    want_i, want_p = sc.argmax_prob_ref(x)
    got_i, got_p = be.argmax_prob_rows(x)
    assert got_i.tolist() == want_i.tolist()
    dead = want_p == 0.0
    assert (got_p[dead] == 0.0).all(), (got_p[dead], np.flatnonzero(dead))
    rel = np.abs(got_p[~dead].astype(np.float64) - want_p[~dead]) / want_p[~dead]
    print(f"n={n} rows={rows} max rel err of p {rel.max() if rel.size else 0.0:.3g}")
    assert (rel <= TIGHT_TOL).all(), (rel, np.flatnonzero(~dead))
    again_i, again_p = be.argmax_prob_rows(x)
    assert again_i.tobytes() == got_i.tobytes() and again_p.tobytes() == got_p.tobytes()       # the same bits run to run
    if rows == 17 and n > 1:
        assert got_p[8] > 0.999 and got_p[9] == pytest.approx(1.0 / n, rel=TIGHT_TOL)           # the dominant and the flat row


@pytest.mark.parametrize("G", [1, 5, 64])
def test_spec_verify(be, G):
    n = 1000
    rng = np.random.default_rng(40 + G)
    ks = [(0, 1, 7, 16)[g % 4] for g in range(G)] if G > 1 else [16]
    gs = np.concatenate([[0], np.cumsum([k + 1 for k in ks])]).astype(np.int32)
    R = int(gs[-1])
    base = (rng.standard_normal((R + 9, n)) * 2.0).astype(np.float32)
    base[3, :] = np.nan                                                  # a row of NaNs answers 0
    base[5, 17] = base[5, 900] = 40.0                                    # a tie: the lower index
    rows = rng.permutation(R + 9)[:R].astype(np.int32)                   # a shuffled subset of the base rows
    ids = np.array([sc.argmax_rule(base[r]) for r in rows], np.int32)
    draft = np.empty(R, np.int32)
    want_acc = []
    for g, k in enumerate(ks):
        lo = int(gs[g])
        a = (0, k // 2, k)[(g + 1) % 3] if G > 1 else 9                  # accepted: none, a middle length, all
        a = min(a, k)
        draft[lo:lo + k] = ids[lo:lo + k]
        if a < k:
            draft[lo + a] = (ids[lo + a] + 1) % n                        # the first mismatch; what follows it matches again and must not be counted
        draft[lo + k] = ids[lo + k]                                      # the ignored entry of the group's last row equals the arg-max: not counted either
        want_acc.append(a)
    ref_ids, ref_acc = sc.spec_verify_ref(base, rows, gs, draft)
    assert ref_acc.tolist() == want_acc and ref_ids.tolist() == ids.tolist()
    got_ids, got_acc = be.spec_verify(base, rows, gs, draft)
    assert got_ids.tolist() == ids.tolist()
    assert got_acc.tolist() == want_acc
    if G > 1:
        pairs = list(zip(want_acc, ks))
        assert any(a == k >= 1 for a, k in pairs) and any(0 < a < k for a, k in pairs) and any(a == 0 and k >= 1 for a, k in pairs), pairs
    again_ids, again_acc = be.spec_verify(base, rows, gs, draft)
    assert again_ids.tobytes() == got_ids.tobytes() and again_acc.tobytes() == got_acc.tobytes()
