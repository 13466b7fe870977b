"""Inputs of the quantiser tests (test_quantize_cpu.py, test_gpu_quantize_ops.py): the shapes, the normal and the special rows, the 1/4-heavy importance
matrix and the margins of the K-type error comparison."""
from __future__ import annotations

import functools

import numpy as np

import quantize_ref as qr

K_SHAPES = (256, 768, 2304)          # one super-block, odd counts of them
K32_SHAPES = (32, 96, 576)           # the 32-element types: one block, odd counts
ROWS = (1, 3, 67)
TYPES_32 = (qr.Q8_0, qr.Q5_0, qr.Q5_1)
NAME = {qr.Q8_0: "q8_0", qr.Q5_0: "q5_0", qr.Q5_1: "q5_1", qr.Q2_K: "q2_K", qr.Q3_K: "q3_K", qr.Q4_K: "q4_K", qr.Q5_K: "q5_K", qr.Q6_K: "q6_K"}

# m_type: the device's weighted error per row may exceed the f32 twin's by this share.  Twice the largest per-row relative difference in weighted error between
# the f32 twin and the f64 twin over every case below, with and without the importance matrix (test_quantize_cpu.py::test_rounding_spread prints the spreads
# and checks these constants against them); a type whose twins agree on every row would get one part in 10^4.
# Measured spreads: q2_K 6.506e-2, q3_K 1.057e-3, q4_K 3.538e-2, q5_K 8.969e-2, q6_K 4.142e-2 (a single-row case where one sub-block's search lands on another
# candidate moves a row's error by that much).
M_TYPE = {qr.Q2_K: 0.1302, qr.Q3_K: 2.12e-3, qr.Q4_K: 0.0708, qr.Q5_K: 0.1794, qr.Q6_K: 0.0829}


def shapes(t: int):
    return K32_SHAPES if t in TYPES_32 else K_SHAPES


@functools.lru_cache(maxsize=None)
def normal(K: int, rows: int) -> np.ndarray:
    return (np.random.default_rng(1000 * K + rows).standard_normal((rows, K)) * 0.02).astype(np.float32)


SPECIAL_NAMES = ("zero", "constant", "outlier", "positive_subblock", "tiny", "common")


@functools.lru_cache(maxsize=None)
def special(K: int) -> np.ndarray:
    """one row each: all zero | constant | one element 100 x the rest | a sub-block that is all positive (the min <= 0 clamp) | values of 1e-30 (d underflows
    in f16) | values that F32, F16 and BF16 all hold exactly"""
    rng = np.random.default_rng(77 + K)
    base = (rng.standard_normal((6, K)) * 0.02).astype(np.float32)
    base[0] = 0.0
    base[1] = 0.0173
    base[2, K // 3] = 100.0 * np.abs(base[2]).max()
    base[3, :32] = np.abs(base[3, :32]) + 0.01
    base[4] = np.where(rng.integers(0, 2, K) == 1, 1e-30, -1e-30).astype(np.float32)
    c = (base[5].view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)            # 8 significant bits ...
    base[5] = np.where(np.abs(c) < 2.0 ** -14, 0.0, c)                                  # ... inside f16's normal range
    return base


def heavy_imatrix(K: int) -> np.ndarray:
    """1/4-heavy: 1000 on every fourth column, 1 elsewhere"""
    w = np.ones(K, np.float32)
    w[::4] = 1000.0
    return w


def as_source(x: np.ndarray, src_type: int) -> np.ndarray:
    """the rows in a source format: f32, f16, or bf16 bits as uint16 (nearest even)"""
    if src_type == qr.F16:
        return x.astype(np.float16)
    if src_type == qr.BF16:
        u = np.ascontiguousarray(x, np.float32).view(np.uint32)
        return ((u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)).astype(np.uint16)
    return np.ascontiguousarray(x, np.float32)


def dequantize(t: int, raw: np.ndarray, K: int) -> np.ndarray:
    """uint8 [rows][row bytes] -> f32 [rows][K] through the oracle (Q5_1: the numpy decoder of q41_q51_ref)"""
    import oracle_py as op
    raw = np.ascontiguousarray(raw, np.uint8).reshape(-1, K // qr.BLOCK_ELEMS[t] * qr.BLOCK_BYTES[t])
    if t == qr.Q5_1:
        import q41_q51_ref as q51
        return np.stack([q51.dequantize(t, r, K) for r in raw]).astype(np.float32)
    return np.stack([op.dequantize(t, r, K) for r in raw])


def weighted_error(t: int, x: np.ndarray, raw: np.ndarray, imatrix=None) -> np.ndarray:
    """per row, in float64: sum over the columns of w (x - dequantised)^2, w the importance matrix or 1"""
    y = dequantize(t, raw, x.shape[1]).astype(np.float64)
    w = np.ones(x.shape[1]) if imatrix is None else np.asarray(imatrix, np.float64)
    return (w * (x.astype(np.float64) - y) ** 2).sum(axis=1)
