"""csrc/quantize.hip through mi355_quantize_chunk over the cases of quantize_cases.py, with and without the importance matrix, from F32, F16 and BF16 rows:
Q8_0 / Q5_0 / Q5_1 equal the numpy twin's bytes (Q8_0 also the oracle's); the K types' weighted error per row stays within (1 + M_TYPE) of the f32 twin's;
every block dequantises finite; a second call and another split of the rows over calls give the same bytes; the importance matrix lowers the error on its
heavy columns; every refusal is MI355_ERR_ARG.  The entry checks a guard row behind the output on the device after every launch and fails the call
(MI355_ERR_HIP) if it was written, so every call that returns here also says the guard was intact."""
import functools

import numpy as np
import pytest

import quantize_cases as qc
import quantize_ref as qr

pytestmark = pytest.mark.gpu

ERR_ARG = -103            # MI355_ERR_ARG
ALL_TYPES = qc.TYPES_32 + qr.K_TYPES
SRC = {"f32": qr.F32, "f16": qr.F16, "bf16": qr.BF16}


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def rows_of(K, what):
    return qc.special(K) if what == "special" else qc.normal(K, what)


@functools.lru_cache(maxsize=None)
def source(K, what, st):
    """(the rows in the source format, the f32 values they hold)"""
    s = qc.as_source(rows_of(K, what), st)
    return s, qr.to_f32(s, st).reshape(s.shape)


@functools.lru_cache(maxsize=None)
def twin(t, K, what, st, imx):
    return qr.quantize_rows(t, source(K, what, st)[1], qc.heavy_imatrix(K) if imx else None)


def device(be, t, K, what, st, imx):
    return be.quantize_rows(t, source(K, what, st)[0], qc.heavy_imatrix(K) if imx else None, src_type=st)


def identical_share(t, a, b):
    nb = a.size // qr.BLOCK_BYTES[t]
    return float((a.reshape(nb, -1) == b.reshape(nb, -1)).all(axis=1).mean())


@pytest.mark.parametrize("imx", [False, True], ids=["plain", "imatrix"])
@pytest.mark.parametrize("st", list(SRC), ids=list(SRC))
@pytest.mark.parametrize("t", qc.TYPES_32, ids=lambda t: qc.NAME[t])
def test_32_element_types_equal_the_twin(be, t, st, imx):
    import oracle_py as op
    for K in qc.K32_SHAPES:
        for what in qc.ROWS + ("special",):
            got = device(be, t, K, what, SRC[st], imx)
            assert np.array_equal(got, twin(t, K, what, SRC[st], imx)), (K, what)
            assert np.isfinite(qc.dequantize(t, got, K)).all()
            if t == qr.Q8_0:
                assert np.array_equal(got, np.stack([op.quantize(op.Q8_0, r) for r in source(K, what, SRC[st])[1]])), (K, what)
            assert np.array_equal(device(be, t, K, what, SRC[st], imx), got)


@pytest.mark.parametrize("imx", [False, True], ids=["plain", "imatrix"])
@pytest.mark.parametrize("st", list(SRC), ids=list(SRC))
@pytest.mark.parametrize("t", qr.K_TYPES, ids=lambda t: qc.NAME[t])
def test_k_types_within_the_margin_of_the_twin(be, t, st, imx):
    worst, shares = 0.0, []
    for K in qc.K_SHAPES:
        w = qc.heavy_imatrix(K) if imx else None
        for what in qc.ROWS + ("special",):
            x = source(K, what, SRC[st])[1]
            got, ref = device(be, t, K, what, SRC[st], imx), twin(t, K, what, SRC[st], imx)
            assert got.shape == ref.shape
            assert np.isfinite(qc.dequantize(t, got, K)).all(), (K, what)
            e_dev, e_ref = qc.weighted_error(t, x, got, w), qc.weighted_error(t, x, ref, w)
            shares.append(identical_share(t, got, ref))
            nz = e_ref > 0
            if nz.any():
                worst = max(worst, float((e_dev[nz] / e_ref[nz]).max()))
            print(f"{qc.NAME[t]} {st} K={K} rows={what}: identical blocks {shares[-1]:.4f}, largest error ratio {float((e_dev[nz] / e_ref[nz]).max()) if nz.any() else 1.0:.6f}")
            assert (e_dev <= (1.0 + qc.M_TYPE[t]) * e_ref).all(), (K, what, e_dev, e_ref)
            assert np.array_equal(device(be, t, K, what, SRC[st], imx), got), "a second call gave other bytes"
            if what == "special":                    # the zero row dequantises to zeros
                assert (qc.dequantize(t, got[:1], K) == 0).all()
    print(f"{qc.NAME[t]} {st} {'imatrix' if imx else 'plain'}: byte-identical blocks {np.mean(shares):.4f}; largest device / twin error ratio {worst:.6f} "
          f"(allowed {1 + qc.M_TYPE[t]:.4f})")


@pytest.mark.parametrize("t", ALL_TYPES, ids=lambda t: qc.NAME[t])
def test_split_of_the_rows_over_calls(be, t):
    """67 rows in one call, and as 64 + 3"""
    for K in qc.shapes(t):
        x = qc.normal(K, 67)
        for w in (None, qc.heavy_imatrix(K)):
            whole = be.quantize_rows(t, x, w)
            parts = np.concatenate([be.quantize_rows(t, x[:64], w), be.quantize_rows(t, x[64:], w)])
            assert np.array_equal(whole, parts), K


@pytest.mark.parametrize("t", qr.K_TYPES, ids=lambda t: qc.NAME[t])
def test_heavy_columns_gain_from_the_imatrix(be, t):
    heavy = heavy_im = 0.0
    for K in qc.K_SHAPES:
        for R in qc.ROWS:
            x = qc.normal(K, R)
            y = qc.dequantize(t, be.quantize_rows(t, x), K)
            yi = qc.dequantize(t, be.quantize_rows(t, x, qc.heavy_imatrix(K)), K)
            heavy += float(((y - x)[:, ::4].astype(np.float64) ** 2).sum())
            heavy_im += float(((yi - x)[:, ::4].astype(np.float64) ** 2).sum())
    print(f"{qc.NAME[t]}: squared error on the heavy columns {heavy:.4e} -> {heavy_im:.4e}")
    assert heavy_im < heavy


def test_the_common_row_gives_the_same_bytes_from_every_source(be):
    for t in ALL_TYPES:
        for K in qc.shapes(t):
            common = qc.special(K)[5:6]
            got = [be.quantize_rows(t, qc.as_source(common, st), src_type=st) for st in SRC.values()]
            assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2]), (t, K)


def test_refusals(be, pkg):
    lib = be.lib
    x = qc.normal(256, 3).copy()
    out = np.zeros(3 * 210, np.uint8)

    def call(dst_type, src_type, src, n, rows, im=None):
        rc = lib.mi355_quantize_chunk(dst_type, src_type, src.ctypes.data, n, rows, None if im is None else im.ctypes.data, out.ctypes.data)
        return rc, (lib.mi355_last_error() or b"").decode()

    for dst in (0, 2, 20, 23, 39, 99):                                       # F32, Q4_0, IQ4_NL, IQ4_XS, MXFP4, nothing
        rc, msg = call(dst, 0, x, 256, 3)
        assert rc == ERR_ARG and "destination type" in msg, (dst, rc, msg)
        assert lib.mi355_quantize_supported(dst) == 0
    for src in (8, 12, 2, -1):
        rc, msg = call(qr.Q4_K, src, x, 256, 3)
        assert rc == ERR_ARG and "source type" in msg, (src, rc, msg)
    for t, n in ((qr.Q4_K, 128), (qr.Q4_K, 288), (qr.Q8_0, 48), (qr.Q6_K, 0)):
        rc, msg = call(t, 0, x, n, 1)
        assert rc == ERR_ARG and "n_per_row" in msg, (t, n, rc, msg)
    for rows in (0, -2):
        rc, msg = call(qr.Q4_K, 0, x, 256, rows)
        assert rc == ERR_ARG and "n_rows" in msg
    for bad in (-1.0, np.nan, np.inf):
        im = np.ones(256, np.float32)
        im[17] = bad
        rc, msg = call(qr.Q4_K, 0, x, 256, 3, im)
        assert rc == ERR_ARG and "imatrix[17]" in msg, (bad, rc, msg)
    for st in SRC.values():
        for bad in (np.nan, np.inf, -np.inf):
            xb = x.copy()
            xb[2, 100] = bad
            for t in (qr.Q8_0, qr.Q4_K, qr.Q3_K):
                out[:] = 0x5A
                rc, msg = call(t, st, qc.as_source(xb, st), 256, 3)
                assert rc == ERR_ARG and "row 2" in msg and "non-finite" in msg, (st, bad, t, rc, msg)
                assert (out == 0x5A).all()
    with pytest.raises(pkg.MI355Error, match="row 2"):
        xb = x.copy()
        xb[2, 0] = np.nan
        be.quantize_rows(qr.Q5_K, xb)
