"""csrc/quant_error.hip through mi355_dequantize_rows and mi355_quant_error_rows against quant_error_ref.py: every weight type decodes to the reference's f32 bit
for bit (and to its nearest-even f16) from the file's own blocks; the four per-row error figures match float64 within the margin the reference's own two
summation orders set, the maximum exactly; rows cut into two calls give the same bits; every refusal is MI355_ERR_ARG and names its cause.  The entries check a
guard row behind each output after the launch, so every call that returns here also says the guard was intact."""
import functools

import numpy as np
import pytest

import quant_error_ref as qe
import quantize_cases as qc
import quantize_ref as qr

gs = qe.gs
gpu = pytest.mark.gpu
ERR_ARG, ERR_NO_DEVICE = -103, -100
SHAPES_256, SHAPES_32 = (256, 768), (32, 288, 2080)    # one wave; 288: a wave straddles a row end and the last one is ragged; 2080: more than one workgroup


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


@functools.lru_cache(maxsize=None)
def blocks(t, n, rows):
    """rows x n elements of type t from the writer's seeded block generator, uint8 [rows][row bytes]; with five rows the last one holds the extremes: every
    byte value in its payload, a first block of zeros (scale 0) and a last block with the largest finite scale"""
    rng = np.random.default_rng(100 * t + n + rows)
    raw = gs.random_blocks(rng, t, rows * n, 0.02).reshape(rows, -1).copy()
    if rows == 5 and t in (gs.F32, gs.F16, gs.BF16):        # bit patterns: zeros of both signs, the largest finite values, subnormals, the least normal
        sign, big, norm = {gs.F32: (31, 0x7F7FFFFF, 0x00800000), gs.F16: (15, 0x7BFF, 0x0400), gs.BF16: (15, 0x7F7F, 0x0080)}[t]
        raw[4].view(np.uint32 if t == gs.F32 else np.uint16)[:8] = [0, 1 << sign, big, big | 1 << sign, 1, 1 | 1 << sign, norm - 1, norm]
    elif rows == 5:
        blk, ends = raw[4].view(gs.BLOCK_DTYPE[t]), {"d": (0.0, 65504.0), "dmin": (0.0, 65504.0), "m": (0.0, -65504.0), "e": (0, 252)}       # (2^124: with the level 12 the largest finite product)
        for name in blk.dtype.names:
            if name in ends:
                blk[name][0], blk[name][-1] = ends[name]
            else:
                blk[name] = ((np.arange(blk[name].size) * 37 + 11) & 255).reshape(blk[name].shape).astype(blk[name].dtype)
    return raw


@gpu
@pytest.mark.parametrize("t", qe.TYPES, ids=lambda t: qe.NAME[t])
def test_decode_equals_the_reference_bit_for_bit(be, t):
    for n in SHAPES_256 if gs.BLOCK_ELEMS[t] == 256 else SHAPES_32:
        for rows in (1, 5):
            raw = blocks(t, n, rows)
            want = qe.decode(t, raw, n)
            assert np.isfinite(want).all()
            got = be.dequantize_rows(raw, t, n)
            assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, rows)
            with np.errstate(over="ignore"):
                want16 = want.astype(np.float16)
            assert np.array_equal(be.dequantize_rows(raw, t, n, dst="f16").view(np.uint16), want16.view(np.uint16)), (n, rows)


def quantise(t, x):
    """x [rows][n] f32 as blocks of t by the tree's own quantisers"""
    if t in qr.BLOCK_BYTES:
        return qr.quantize_rows(t, x)
    return {gs.TQ1_0: gs.quantize_tq1_0, gs.Q4_1: lambda v: gs.quantize_min32(gs.Q4_1, v), gs.MXFP4: gs.quantize_mxfp4}[t](x).reshape(x.shape[0], -1)


@functools.lru_cache(maxsize=None)
def error_case(rt, ct, n):
    """(reference rows in their format, their f32, candidate blocks, their f32): five seeded normal rows; a block-type reference is their quantisation"""
    x = qc.normal(n, 5)
    ref = quantise(rt, x) if rt in gs.BLOCK_DTYPE else qc.as_source(x, rt)
    cand = quantise(ct, x)
    return ref, qe.decode(rt, ref, n), cand, qe.decode(ct, cand, n)


ERROR_CASES = [(gs.F32, gs.Q8_0, 288), (gs.F16, gs.Q6_K, 768), (gs.BF16, gs.TQ1_0, 768), (gs.F32, gs.MXFP4, 288), (gs.F16, gs.Q3_K, 256),
               (gs.Q8_0, gs.Q4_1, 288), (gs.Q6_K, gs.Q4_K, 768)]                     # the last two: two block sets


@gpu
@pytest.mark.parametrize("weights", [False, True], ids=["plain", "col_weights"])
@pytest.mark.parametrize("rt,ct,n", ERROR_CASES, ids=lambda v: qe.NAME.get(v, str(v)))
def test_error_against_float64(be, rt, ct, n, weights):
    ref, w, cand, y = error_case(rt, ct, n)
    c = qc.heavy_imatrix(n) if weights else None
    want = qe.errors(w, y, c)
    spread, margin = qe.margin(w, y, c)
    got = be.quant_error_rows(ref, rt, cand, ct, n, c)
    rel = np.abs(got[:, :3] - want[:, :3]) / want[:, :3]
    print(f"{qe.NAME[rt]} / {qe.NAME[ct]} n={n}: spread {spread:.3e} margin {margin:.3e} device {rel.max():.3e}")
    assert got.shape == (5, 4) and (want[:, :3] > 0).all()
    assert rel.max() <= margin, (rel.max(), margin)
    assert np.array_equal(got[:, 3], want[:, 3])
    if not weights:
        assert np.array_equal(got[:, 2], got[:, 0])


@gpu
@pytest.mark.parametrize("rt,ct,n", [ERROR_CASES[0], ERROR_CASES[1], ERROR_CASES[5]], ids=lambda v: qe.NAME.get(v, str(v)))
def test_rows_cut_into_two_calls_give_the_same_bits(be, rt, ct, n):
    ref, _, cand, _ = error_case(rt, ct, n)
    c = qc.heavy_imatrix(n)
    whole = be.quant_error_rows(ref, rt, cand, ct, n, c)
    parts = np.concatenate([be.quant_error_rows(ref[:3], rt, cand[:3], ct, n, c), be.quant_error_rows(ref[3:], rt, cand[3:], ct, n, c)])
    assert np.array_equal(whole.view(np.uint64), parts.view(np.uint64))


@gpu
def test_refusals_name_their_cause(be, pkg):
    x = qc.normal(256, 5)
    q = qr.quantize_rows(qr.Q4_K, x)
    for args, word in (((x, gs.F32, q, gs.Q8_K, 256), "q8_K"), ((x, gs.Q8_K, q, gs.Q4_K, 256), "q8_K"), ((x, gs.F32, q, 99, 256), "99"),
                       ((x[:1, :100], gs.F32, q[:1], gs.Q4_K, 100), "n_per_row 100")):
        with pytest.raises(pkg.MI355Error, match=rf"\({ERR_ARG}\).*{word}"):
            be.quant_error_rows(*args)
    for t, n, word in ((gs.Q8_K, 256, "q8_K"), (99, 256, "99"), (gs.Q4_K, 100, "n_per_row 100")):
        with pytest.raises(pkg.MI355Error, match=rf"\({ERR_ARG}\).*{word}"):
            be.dequantize_rows(q[:1], t, n)
    lib = pkg.load_library()
    out = np.zeros((5, 4))
    assert lib.mi355_quant_error_rows(gs.F32, x.ctypes.data, gs.Q4_K, q.ctypes.data, 256, 0, None, out.ctypes.data) == ERR_ARG
    assert lib.mi355_quant_error_rows(gs.F32, None, gs.Q4_K, q.ctypes.data, 256, 5, None, out.ctypes.data) == ERR_ARG
    bad = x.copy()
    bad[3, 17] = np.nan
    out[:] = 7.0
    assert lib.mi355_quant_error_rows(gs.F32, bad.ctypes.data, gs.Q4_K, q.ctypes.data, 256, 5, None, out.ctypes.data) == ERR_ARG
    assert b"row 3" in lib.mi355_last_error() and (out == 7.0).all()


def test_no_device_is_answered_before_the_arguments(pkg):
    lib = pkg.load_library()
    want = ERR_NO_DEVICE if lib.mi355_device_count() <= 0 else ERR_ARG
    assert lib.mi355_quant_error_rows(99, None, 99, None, 0, 0, None, None) == want
    assert lib.mi355_dequantize_rows(99, None, 0, 0, 0, None) == want
    assert [lib.mi355_quant_error_supported(t) for t in (gs.Q6_K, gs.MXFP4, gs.Q8_K, 99)] == [1, 1, 0, 0]
