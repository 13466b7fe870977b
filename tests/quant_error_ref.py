"""Reference of csrc/quant_error.hip (test_gpu_quant_error.py, test_quantize_stats_tool.py): the f32 value of every element of rows in a GGUF file's layout,
by the decoders the tree already states (the oracle's dequantize_row_* for the types it has, the numpy restatements for the others), and the four per-row
error figures in float64.  Nothing here re-derives a decode."""
from __future__ import annotations

import numpy as np

import __graft_entry__ as ge
import bf16_ref
import iq4xs_ref
import mxfp4_ref
import oracle_py as op
import q41_q51_ref
import tq_ref

gs = ge.load_pkg().gguf_synth

TYPES = (gs.F32, gs.F16, gs.BF16, gs.Q4_0, gs.Q4_1, gs.Q5_0, gs.Q5_1, gs.Q8_0, gs.Q2_K, gs.Q3_K, gs.Q4_K, gs.Q5_K, gs.Q6_K, gs.IQ4_NL, gs.IQ4_XS, gs.TQ1_0,
         gs.TQ2_0, gs.MXFP4)
NAME = {t: gs.TYPE_NAME[t] for t in TYPES}


def decode(t: int, blocks: np.ndarray, n_per_row: int) -> np.ndarray:
    """rows of type t as the file holds them (any dtype, any shape) -> f32 [n_rows][n_per_row]"""
    raw = np.ascontiguousarray(blocks).reshape(-1).view(np.uint8)
    n = raw.size // gs.BLOCK_BYTES[t] * gs.BLOCK_ELEMS[t]
    if t == gs.BF16:
        y = bf16_ref.widen(bf16_ref.bits_of(raw, n))
    elif t == gs.IQ4_XS:
        y = iq4xs_ref.dequantize(raw, n)
    elif t == gs.MXFP4:
        y = mxfp4_ref.dequantize(raw, n)
    elif t in (gs.Q4_1, gs.Q5_1):
        y = q41_q51_ref.dequantize(t, raw, n)
    elif t in (gs.TQ1_0, gs.TQ2_0):
        y = tq_ref.dequantize(t, raw, n)
    else:
        y = op.dequantize(t, raw, n)
    return np.asarray(y, np.float32).reshape(-1, n_per_row)


def terms(ref: np.ndarray, deq: np.ndarray, c=None):
    """the float64 terms of the three sums, [n_rows][n_per_row] each, and |e|"""
    w, e = ref.astype(np.float64), ref.astype(np.float64) - deq.astype(np.float64)
    e2 = e * e
    return e2, w * w, e2 if c is None else np.asarray(c, np.float32).astype(np.float64)[None, :] * e2, np.abs(e)


def errors(ref: np.ndarray, deq: np.ndarray, c=None) -> np.ndarray:
    """per row {sum e^2, sum w^2, sum c e^2, max |e|}, float64 [n_rows][4] (numpy's pairwise sums)"""
    e2, w2, ce2, ae = terms(ref, deq, c)
    return np.stack([e2.sum(axis=1), w2.sum(axis=1), ce2.sum(axis=1), ae.max(axis=1)], axis=1)


def margin(ref: np.ndarray, deq: np.ndarray, c=None):
    """(spread, margin): the largest relative difference, over the rows and the three sums, between numpy's pairwise sum and a plain left-to-right float64
    sum of the same terms; the device, which differs from either by its summation order alone, is allowed ten times the larger of that and 1e-15."""
    spread = 0.0
    for t in terms(ref, deq, c)[:3]:
        pair, seq = t.sum(axis=1), np.cumsum(t, axis=1)[:, -1]
        nz = pair != 0
        if nz.any():
            spread = max(spread, float((np.abs(pair - seq)[nz] / pair[nz]).max()))
    return spread, 10.0 * max(spread, 1e-15)
