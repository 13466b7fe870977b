"""The collector launch of csrc/imatrix.hip through mi355_op_imatrix_accum: exact on integer inputs, within the rounding bound of imatrix_cases.py on normal
ones, the same bits run to run, the SwiGLU producer bit-equal to mi355_op_swiglu followed by the plain form, per-expert launches with empty experts and a
row-source table, and the refusals."""
import numpy as np
import pytest

import imatrix_cases as ic

pytestmark = pytest.mark.gpu

ERR_ARG = -103            # MI355_ERR_ARG


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def start(rng, n_mat, K, integer):
    """a non-zero running total, its guard row and counts"""
    s = rng.integers(0, 1000, (n_mat + 1, K)).astype(np.float32) if integer else (rng.random((n_mat + 1, K)) * 50).astype(np.float32)
    return s, rng.integers(1, 100, n_mat).astype(np.int32)


@pytest.mark.parametrize("pad", [0, 32])
@pytest.mark.parametrize("R", ic.OP_RS)
@pytest.mark.parametrize("K", ic.OP_KS)
def test_exact_on_integers(be, K, R, pad):
    """Two calls into a non-zero running total equal the integer reference bit for bit; ld = K and ld = K + 32 (the pad columns are never read into a sum)."""
    rng = np.random.default_rng(K * 7 + R + pad)
    s0, c0 = start(rng, 1, K, True)
    x1, x2 = ic.int_rows(rng, R, K + pad), ic.int_rows(rng, R, K + pad)
    s1, c1 = be.imatrix_accum(x1, s0, c0, K=K)
    s2, c2 = be.imatrix_accum(x2, s1, c1, K=K)
    want = s0[0].astype(np.float64) + ic.sq_sum(x1, K) + ic.sq_sum(x2, K)
    assert want.max() < 2 ** 24
    assert np.array_equal(s2[0].astype(np.float64), want)
    assert np.array_equal(s2[1], s0[1]) and c2.tolist() == [int(c0[0]) + 2 * R]


@pytest.mark.parametrize("pad", [0, 32])
@pytest.mark.parametrize("R", ic.OP_RS)
@pytest.mark.parametrize("K", ic.OP_KS)
def test_float_bound_and_same_bits(be, K, R, pad):
    rng = np.random.default_rng(K * 11 + R + pad)
    x1, x2 = ic.normal_rows(rng, R, K + pad), ic.normal_rows(rng, R, K + pad)
    z = np.zeros((2, K), np.float32)
    s1, c1 = be.imatrix_accum(x1, z, np.zeros(1, np.int32), K=K)
    ref1 = ic.sq_sum(x1, K)
    err1 = np.abs(s1[0] - ref1) / ref1
    assert (np.abs(s1[0] - ref1) <= ic.float_bound(ref1, R)).all(), float(err1.max())
    s2, c2 = be.imatrix_accum(x2, s1, c1, K=K)
    ref2 = s1[0].astype(np.float64) + ic.sq_sum(x2, K)            # (the previous total as the device holds it)
    err2 = np.abs(s2[0] - ref2) / ref2
    print(f"K={K} R={R} ld={K + pad}: max |dev - ref| / ref {float(err1.max()):.3g} (bound {(R + 4) * ic.U:.3g}), second call {float(err2.max()):.3g}")
    assert (np.abs(s2[0] - ref2) <= ic.float_bound(ref2, 2 * R)).all(), float(err2.max())
    again, _ = be.imatrix_accum(x1, z, np.zeros(1, np.int32), K=K)
    assert again.tobytes() == s1.tobytes() and c2.tolist() == [2 * R]


@pytest.mark.parametrize("R", ic.PRODUCER_RS)
@pytest.mark.parametrize("K", ic.PRODUCER_KS)
def test_swiglu_producer_is_the_swiglu_launch(be, K, R):
    rng = np.random.default_rng(K + R)
    g, u = (ic.normal_rows(rng, R, K) * 3).astype(np.float32), ic.normal_rows(rng, R, K)
    g[0, :8] = [0.0, -0.0, 40.0, -40.0, 90.0, -90.0, 1e-30, -1e-30]
    z = np.zeros((2, K), np.float32)
    fused, cf = be.imatrix_accum(g, z, np.zeros(1, np.int32), x2=u)
    y = be.swiglu(g.reshape(-1), u.reshape(-1)).reshape(R, K)
    plain, cp = be.imatrix_accum(y, z, np.zeros(1, np.int32))
    assert fused.tobytes() == plain.tobytes() and cf.tolist() == cp.tolist() == [R]
    assert (fused[0] > 0).any()


EXPERT_CASES = [
    ("8 experts, one empty, one single row", 8, [5, 0, 1, 9, 3, 7, 2, 13]),
    ("8 experts, all rows in expert 7", 8, [0, 0, 0, 0, 0, 0, 0, 37]),
    ("256 experts, 4 rows", 256, None),
    ("160 experts, 320 rows", 160, None),
]


@pytest.mark.parametrize("what,n_mat,counts", EXPERT_CASES, ids=[c[0] for c in EXPERT_CASES])
def test_experts_and_row_source(be, what, n_mat, counts):
    """Integer inputs, so exact: every expert's row of sums and count equals the reference of its run of launch rows read through row_src (repeated and
    out-of-order source rows); experts without rows and the guard row come back as they went in; the counts are the histogram."""
    rng = np.random.default_rng(n_mat + 1)
    K = 96
    if counts is None:
        R = 4 if n_mat == 256 else 320
        ids = np.sort(rng.integers(0, n_mat, R)) if n_mat == 160 else np.array([3, 3, 200, 255])
        counts = np.bincount(ids, minlength=n_mat)
    counts = np.asarray(counts, np.int32)
    R = int(counts.sum())
    n_src = max(3, R // 3)
    x = ic.int_rows(rng, n_src, K)
    row_src = rng.integers(0, n_src, R).astype(np.int32)           # repeats, no order
    s0, c0 = start(rng, n_mat, K, True)
    s1, c1 = be.imatrix_accum(x, s0, c0, row_src=row_src, counts_per_mat=counts)
    want = s0[:n_mat].astype(np.float64) + ic.expert_ref(x, K, counts, row_src)
    assert np.array_equal(s1[:n_mat].astype(np.float64), want)
    assert np.array_equal(s1[n_mat], s0[n_mat])
    assert np.array_equal(c1, c0 + counts)
    empty = counts == 0
    assert empty.any() and s1[:n_mat][empty].tobytes() == s0[:n_mat][empty].tobytes()
    # without a table: launch row r is source row r
    x_all = ic.int_rows(rng, R, K)
    s2, c2 = be.imatrix_accum(x_all, s0, c0, counts_per_mat=counts)
    assert np.array_equal(s2[:n_mat].astype(np.float64), s0[:n_mat].astype(np.float64) + ic.expert_ref(x_all, K, counts))


def test_refusals_leave_the_outputs_alone(be, pkg):
    lib = be.lib
    x = np.ones((8, 128), np.float32)

    def call(ld, K, R, n_mat, counts, n_src=8):
        s = np.full((max(n_mat, 0) + 1, max(K, 1)), 7.0, np.float32)
        c = np.full(max(n_mat, 1), 3, np.int32)
        cm = None if counts is None else np.asarray(counts, np.int32)
        rc = lib.mi355_op_imatrix_accum(x.ctypes.data, None, ld, K, R, None, n_src, None if cm is None else cm.ctypes.data, n_mat, s.ctypes.data, c.ctypes.data)
        assert (s == 7.0).all() and (c == 3).all()
        return rc

    assert call(128, 48, 8, 1, None) == ERR_ARG                      # K no multiple of 32
    assert call(128, 0, 8, 1, None) == ERR_ARG
    assert call(128, 128, 8, 0, None) == ERR_ARG                     # n_mat outside 1 .. 256
    assert call(128, 128, 8, 257, [0] * 256 + [8]) == ERR_ARG
    assert call(128, 128, 8, 2, [3, 4]) == ERR_ARG                   # counts that do not add up to R
    assert call(128, 128, 8, 2, [9, -1]) == ERR_ARG
    assert call(128, 128, 8, 2, None) == ERR_ARG                     # several matrices, no counts
    assert call(96, 128, 8, 1, None) == ERR_ARG                      # ld < K
    assert call(128, 128, 0, 1, None) == ERR_ARG
    assert call(128, 128, 9, 1, None) == ERR_ARG                     # more launch rows than source rows
    assert b"imatrix_accum" in (lib.mi355_last_error() or b"")
    s, c = be.imatrix_accum(x, np.zeros((2, 128), np.float32), np.zeros(1, np.int32))
    assert (s[0] == 8.0).all() and c.tolist() == [8]
