"""Plain numpy references of the kernels that produce indices (csrc/misc.hip: row arg-max, top-k of a logits row, the grouping of a prompt batch's expert
selections, the copies into and the weighted sum out of the grouped rows).  Every one is exact: tests/test_gpu_select.py compares for equality, and
tests/test_select_cpu.py shows that the shared inputs (tests/select_cases.py) tell these references from deliberately wrong restatements."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def argmax_rows(x: np.ndarray) -> np.ndarray:
    """Per row the lowest index of the largest value; NaN entries never win; a row with no comparable entry gives 0."""
    x = np.asarray(x, F32)
    out = np.zeros(x.shape[0], np.int32)
    for r, v in enumerate(x):
        ok = ~np.isnan(v)
        if ok.any():
            out[r] = np.flatnonzero(ok & (v == v[ok].max()))[0]
    return out


def topk_adjust(row: np.ndarray, adj) -> np.ndarray:
    """The logits of one row after its adjustments adj = (tok [m], bias [m], cnt [m], repeat, freq, present) or None, in f32 and step by step as
    Sampler::sample_chain treats a token: l = l + bias; if cnt > 0: l = l * repeat if l <= 0 else l / repeat, then l = l - (f32(cnt) * freq + present)."""
    l = np.array(row, F32, copy=True)
    if adj is None:
        return l
    toks, bias, cnt, repeat, freq, present = adj
    repeat, freq, present = F32(repeat), F32(freq), F32(present)
    with np.errstate(all="ignore"):
        for t, b, c in zip(toks, bias, cnt):
            v = F32(l[t] + F32(b))
            if c > 0:
                v = F32(v * repeat) if v <= 0 else F32(v / repeat)
                v = F32(v - F32(F32(F32(c) * freq) + present))
            l[t] = v
    return l


def topk_rows(base: np.ndarray, rows, k: int, adjs=None):
    """(tokens [n_rows][k] int32, logits [n_rows][k] f32): row r = base[rows[r]] after adjs[r], ordered by the host sampler's `better` - a stable sort by
    (-l, tok) with l compared as floats, so -0.0 and +0.0 tie and the lower token id goes first.  A zero candidate is handed back as +0.0.  No NaN inputs."""
    base = np.asarray(base, F32)
    toks = np.zeros((len(rows), k), np.int32)
    logits = np.zeros((len(rows), k), F32)
    for r, br in enumerate(rows):
        l = topk_adjust(base[br], None if adjs is None else adjs[r])
        assert not np.isnan(l).any()
        order = np.lexsort((np.arange(l.size), -l))[:k]
        toks[r], logits[r] = order, l[order] + F32(0.0)
    return toks, logits


def topk_keys(toks: np.ndarray, logits: np.ndarray) -> np.ndarray:
    """The 64-bit keys the device hands back for (token, logit) pairs: the order-preserving image of the logit's bits above, 0xffffffff - token below."""
    u = np.ascontiguousarray(logits, F32).view(np.uint32)
    u = np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    return (u << np.uint64(32)) | (np.uint64(0xffffffff) - np.asarray(toks).astype(np.uint64))


def moe_group(ids: np.ndarray, n_expert: int):
    """A counting sort of the selections ids [T][k] by expert, stable in (token, rank) order: (meta = counts | exclusive offsets | total, slot_of [T * k] =
    grouped row of pair t * k + j, tok_of [T * k] = token of a grouped row)."""
    T, k = ids.shape
    flat = np.asarray(ids, np.int64).reshape(-1)
    counts = np.bincount(flat, minlength=n_expert)
    offs = np.concatenate(([0], np.cumsum(counts)))
    order = np.argsort(flat, kind="stable")
    slot_of = np.empty(T * k, np.int32)
    slot_of[order] = np.arange(T * k)
    return np.concatenate((counts, offs)).astype(np.int32), slot_of, (order // k).astype(np.int32)


def moe_combine(x: np.ndarray, eo: np.ndarray, w: np.ndarray) -> np.ndarray:
    """x [T][E] + sum over the ranks of eo [k][T][E] * w [T][k], in f32 and in the kernels' order: o = eo_0 * w_0; o = o + eo_j * w_j ...; x = x + o."""
    x, eo, w = np.asarray(x, F32), np.asarray(eo, F32), np.asarray(w, F32)
    o = eo[0] * w[:, 0:1]
    for j in range(1, eo.shape[0]):
        o = o + eo[j] * w[:, j:j + 1]
    return x + o


def moe_scatter_combine(x: np.ndarray, y: np.ndarray, w: np.ndarray, slot_of: np.ndarray) -> np.ndarray:
    """The same sum over grouped rows y [T * k][E]: rank j of token t is row slot_of[t * k + j]."""
    T, k = np.asarray(w).shape
    return moe_combine(x, np.asarray(y, F32)[np.asarray(slot_of).reshape(T, k).T], w)


def gather_rows(src: np.ndarray, rows) -> np.ndarray:
    return np.asarray(src)[np.asarray(rows)]
