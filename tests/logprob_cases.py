"""Perplexity and KL divergence (csrc/logprob.hip, Context.perplexity): the float64 references, the procedure restated over a callback that returns logits
rows, an f32 numpy twin of the kernels' part and fold order, and the row generators.  Shared by test_logprob_cpu.py (the references on hand-made rows, the
twin against the op bars, the procedure on the CPU reference model) and the GPU tests.

The bars.  A log-probability is compared at TIGHT_TOL * max(1, |ref|), the per-op bar argmax_prob_rows meets for p, in log space.  A divergence is a
difference of two f32 log-sum-exps, so its bar is TIGHT_TOL * max(1, |lse_p|, |lse_q|, |ref|)."""
from __future__ import annotations

import numpy as np

from spec_cases import argmax_rule

TIGHT_TOL = 2e-5          # the project's per-op float bar (test_gpu_model.py)
FLIP_TOL = 3e-2           # test_gpu_model.py's bar for a full forward pass
PARTS = 64
N_KINDS = 11
OP_NS = [1, 31, 256, 257, 1000, 32000, 151936]
OP_ROWS = [1, 3, 17]


# ---------------------------------------------------------------- float64 references
def lse_ref(row: np.ndarray) -> float:
    """log sum exp over the non-NaN entries in float64; NaN where the maximum is not finite."""
    v = np.asarray(row, np.float32)
    v = v[~np.isnan(v)].astype(np.float64)
    if not v.size or not np.isfinite(v.max()):
        return float("nan")
    m = v.max()
    return float(m + np.log(np.exp(v - m).sum()))


def token_logprob_ref(x: np.ndarray, targets):
    """(logprob float64 [rows], rank int64 [rows]): logprob = x_t - lse over the non-NaN entries; rank = the non-NaN entries that beat the target (greater, or
    equal at a lower index).  A row whose maximum is not finite, or whose target is NaN, is dead: NaN and -1.  x_t = -inf under a finite maximum: -inf."""
    x = np.asarray(x, np.float32)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    lp = np.full(x.shape[0], np.nan, np.float64)
    rank = np.full(x.shape[0], -1, np.int64)
    for r, row in enumerate(x):
        t = int(targets[r])
        lse = lse_ref(row)
        xt = row[t]
        if np.isnan(lse) or np.isnan(xt):
            continue
        lp[r] = float(xt) - lse if np.isfinite(xt) else -np.inf
        with np.errstate(invalid="ignore"):
            rank[r] = int((row > xt).sum() + (row[:t] == xt).sum())
    return lp, rank


def kl_ref(x: np.ndarray, y: np.ndarray):
    """(KL(P || Q) float64 [rows], same_top int64 [rows], lse_p, lse_q) for P = softmax(x), Q = softmax(y); a pair with a non-finite entry: NaN and -1."""
    x = np.asarray(x, np.float32); y = np.asarray(y, np.float32)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    y = y.reshape(1, -1) if y.ndim == 1 else y
    kl = np.full(x.shape[0], np.nan, np.float64)
    top = np.full(x.shape[0], -1, np.int64)
    lp_, lq_ = np.full(x.shape[0], np.nan), np.full(x.shape[0], np.nan)
    for r in range(x.shape[0]):
        if not (np.isfinite(x[r]).all() and np.isfinite(y[r]).all()):
            continue
        a, b = x[r].astype(np.float64), y[r].astype(np.float64)
        la, lb = lse_ref(x[r]), lse_ref(y[r])
        p = np.exp(a - la)
        kl[r] = float((p * ((a - la) - (b - lb))).sum())
        top[r] = int(argmax_rule(x[r]) == argmax_rule(y[r]))
        lp_[r], lq_[r] = la, lb
    return kl, top, lp_, lq_


def logprob_ok(got, ref) -> np.ndarray:
    """per row: dead rows NaN, -inf exact, otherwise within the op bar"""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(ref), np.isnan(got), np.where(np.isinf(ref), got == ref, np.abs(got - ref) <= TIGHT_TOL * np.maximum(1.0, np.abs(ref))))


def kl_bar(ref, lse_p, lse_q) -> np.ndarray:
    return TIGHT_TOL * np.maximum.reduce([np.ones_like(ref), np.abs(lse_p), np.abs(lse_q), np.abs(ref)])


# ---------------------------------------------------------------- the procedure
def perplexity_ref(decode_rows_fn, tokens, n_chunk: int, bos: int = -1, n_ubatch: int = 1 << 30, base_rows_fn=None, clear_fn=None, stop_after=None):
    """Context.perplexity restated.  decode_rows_fn(piece tokens, positions, flags) returns the logits rows of the flagged positions [n_flagged][n_vocab] (it is
    also called for pieces without a flagged position); clear_fn() empties the sequence before a chunk.  Returns the stats dict with "logprobs" (and "kls")."""
    tokens = np.asarray(tokens, np.int32)
    n_chunks = tokens.size // n_chunk
    first = n_chunk // 2
    st = dict(n_chunks=0, count=0, top1=0, dead=0, same_top=0, has_base=int(base_rows_fn is not None), stopped=0, nll=0.0, nll2=0.0, nll_base=0.0, nll2_base=0.0,
              kl=0.0, kl2=0.0)
    lps, kls = [], []
    for c in range(n_chunks):
        if clear_fn is not None:
            clear_fn()
        tk = tokens[c * n_chunk:(c + 1) * n_chunk].copy()
        if bos >= 0:
            tk[0] = bos
        for i0 in range(0, n_chunk, n_ubatch):
            pos = np.arange(i0, min(i0 + n_ubatch, n_chunk))
            flags = ((pos >= first) & (pos <= n_chunk - 2)).astype(np.int8)
            rows = decode_rows_fn(tk[pos], pos, flags)
            rows_b = base_rows_fn(tk[pos], pos, flags) if base_rows_fn is not None else None
            if not flags.any():
                continue
            tg = tk[pos[flags != 0] + 1]
            lp, rank = token_logprob_ref(rows, tg)
            if rows_b is not None:
                lpb, _ = token_logprob_ref(rows_b, tg)
                kl, top, _, _ = kl_ref(rows_b, rows)
            for r in range(tg.size):
                dead = np.isnan(lp[r]) or (rows_b is not None and (np.isnan(lpb[r]) or np.isnan(kl[r])))
                lps.append(np.nan if dead else lp[r])
                kls.append(np.nan if dead or rows_b is None else kl[r])
                if dead:
                    st["dead"] += 1
                    continue
                st["count"] += 1; st["nll"] -= lp[r]; st["nll2"] += lp[r] * lp[r]; st["top1"] += int(rank[r] == 0)
                if rows_b is not None:
                    st["nll_base"] -= lpb[r]; st["nll2_base"] += lpb[r] * lpb[r]; st["kl"] += kl[r]; st["kl2"] += kl[r] * kl[r]; st["same_top"] += int(top[r] == 1)
        st["n_chunks"] = c + 1
        if stop_after is not None and c + 1 >= stop_after:
            st["stopped"] = 1
            break
    st["logprobs"] = np.asarray(lps, np.float64)
    if base_rows_fn is not None:
        st["kls"] = np.asarray(kls, np.float64)
    return st


# ---------------------------------------------------------------- the kernels' order in f32
def _parts(row: np.ndarray):
    """the row cut as spec_part_range cuts it: [64][chunk], padded with NaN (a NaN takes no part in anything below)"""
    n = row.size
    chunk = (n + PARTS - 1) // PARTS
    pad = np.full(PARTS * chunk, np.nan, np.float32)
    pad[:n] = row
    return pad.reshape(PARTS, chunk)


def _part_pairs(row: np.ndarray):
    """(m [64], s [64]) in f32: a part's maximum over its non-NaN entries (-inf for none) and s = sum exp(x - m) (0 where m is not finite).  Inside a part the
    kernel adds thread sums in a tree; numpy's pairwise f32 sum stands in for it - the part order and the fold below are the kernel's."""
    p = _parts(row)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.where(np.isnan(p), -np.inf, p).max(axis=1).astype(np.float32)
        fin = np.isfinite(m)
        e = np.exp((p - np.where(fin, m, 0)[:, None]).astype(np.float32)).astype(np.float32)
        s = np.where(np.isnan(p), np.float32(0), e).sum(axis=1, dtype=np.float32)
    return m, np.where(fin, s, np.float32(0)).astype(np.float32)


def _fold(m, s, M):
    """sum_k s_k exp(m_k - M) in part order, f32"""
    acc = np.float32(0.0)
    for k in range(PARTS):
        term = np.float32(s[k] * np.exp(np.float32(m[k] - M), dtype=np.float32)) if m[k] > -np.inf else np.float32(0.0)
        acc = np.float32(acc + term)
    return acc


def token_logprob_twin(x: np.ndarray, targets):
    x = np.asarray(x, np.float32)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    lp = np.full(x.shape[0], np.nan, np.float32)
    rank = np.full(x.shape[0], -1, np.int32)
    for r, row in enumerate(x):
        t = int(targets[r])
        m, s = _part_pairs(row)
        M, xt = m.max(), row[t]
        if not np.isfinite(M) or np.isnan(xt):
            continue
        S = _fold(m, s, M)
        with np.errstate(invalid="ignore", divide="ignore"):
            lp[r] = np.float32(np.float32(xt - M) - np.log(S, dtype=np.float32))
            rank[r] = int((row > xt).sum() + (row[:t] == xt).sum())
    return lp, rank


def kl_twin(x: np.ndarray, y: np.ndarray):
    x = np.asarray(x, np.float32); y = np.asarray(y, np.float32)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    y = y.reshape(1, -1) if y.ndim == 1 else y
    kl = np.full(x.shape[0], np.nan, np.float32)
    top = np.full(x.shape[0], -1, np.int32)
    for r in range(x.shape[0]):
        if not (np.isfinite(x[r]).all() and np.isfinite(y[r]).all()):
            continue
        mp, sp = _part_pairs(x[r])
        mq, sq = _part_pairs(y[r])
        px, py = _parts(x[r]), _parts(y[r])
        with np.errstate(invalid="ignore"):
            e = np.exp((px - np.where(np.isfinite(mp), mp, 0)[:, None]).astype(np.float32)).astype(np.float32)
            a = np.where(np.isnan(px), np.float32(0), (e * (px - py).astype(np.float32)).astype(np.float32)).sum(axis=1, dtype=np.float32)
        Mp, Mq = mp.max(), mq.max()
        Sp, Sq, A = _fold(mp, sp, Mp), _fold(mq, sq, Mq), _fold(mp, a, Mp)
        lse_p = np.float32(Mp + np.log(Sp, dtype=np.float32)); lse_q = np.float32(Mq + np.log(Sq, dtype=np.float32))
        kl[r] = np.float32(np.float32(A / Sp) - np.float32(lse_p - lse_q))
        top[r] = int(argmax_rule(x[r]) == argmax_rule(y[r]))
    return kl, top


# ---------------------------------------------------------------- rows
def special_rows(n: int, rows: int, seed: int) -> np.ndarray:
    """test_gpu_spec_ops.py's generator restated.  Row r is of kind r % 11: plain; ties at the first and last index; a tie across the boundary of the first two
    parts; NaNs, one of them where the maximum was; -inf entries; all NaN; all -inf; a +inf entry; one dominant logit; flat; plain at another scale."""
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


def logprob_op_case(n: int, rows: int):
    """(base [rows + 5][n], row index [R], targets [R]) of the op test: every special row, through a shuffled index into a larger base, once per kind of target
    - index 0, n - 1, both sides of the first part boundary, the arg-max, a tied entry, a NaN entry, a -inf entry (where the row has one; index 0 otherwise)."""
    seed = 1000 * rows + n % 997
    rng = np.random.default_rng(seed + 7)
    x = special_rows(n, rows, seed)
    order = rng.permutation(rows + 5)
    base = (rng.standard_normal((rows + 5, n)) * 3.0).astype(np.float32)
    base[order[:rows]] = x
    chunk = (n + 63) // 64
    idx, tg = [], []
    for r in range(rows):
        row = x[r]
        with np.errstate(invalid="ignore"):
            mx = row[~np.isnan(row)].max() if (~np.isnan(row)).any() else np.nan
            tied = np.flatnonzero(row == mx)
        nan_at, ninf_at = np.flatnonzero(np.isnan(row)), np.flatnonzero(row == -np.inf)
        for t in (0, n - 1, min(chunk - 1, n - 1), min(chunk, n - 1), argmax_rule(row), int(tied[-1]) if tied.size else 0, int(nan_at[0]) if nan_at.size else 0,
                  int(ninf_at[-1]) if ninf_at.size else 0):
            idx.append(int(order[r])); tg.append(int(t))
    return base, np.asarray(idx, np.int32), np.asarray(tg, np.int32)


KL_KINDS = 9


def kl_op_case(n: int, rows: int):
    """(p base [rows + 3][n], q base [rows + 2][n], rows_p [rows], rows_q [rows]).  Pair r is of kind r % 9: identical rows; y = x + 3.5; y = x + small noise;
    dominant logits at different indices (KL ~ 50); dominant logits at the same index; a tie in both whose lower index differs; a NaN in y; an inf in x;
    unrelated rows."""
    seed = 7000 * rows + n % 991
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, n)) * 3.0).astype(np.float32)
    y = (rng.standard_normal((rows, n)) * 3.0).astype(np.float32)
    for r in range(rows):
        kind = r % KL_KINDS
        i, j = int(rng.integers(0, n)), int(rng.integers(0, n))
        if n > 1 and j == i:
            j = (i + 1) % n
        if kind == 0:
            y[r] = x[r]
        elif kind == 1:
            y[r] = x[r] + np.float32(3.5)
        elif kind == 2:
            y[r] = x[r] + (rng.standard_normal(n) * 0.05).astype(np.float32)
        elif kind == 3:
            x[r, i] = np.float32(60.0); y[r] = x[r]; y[r, i] = np.float32(0.0); y[r, j] = np.float32(60.0)
        elif kind == 4:
            x[r, i] = np.float32(60.0); y[r, i] = np.float32(55.0)
        elif kind == 5:
            lo, hi = min(i, j), max(i, j)
            x[r, lo] = x[r, hi] = np.float32(20.0)                     # x: the tie resolves to lo
            y[r] = x[r]; y[r, lo] = np.float32(-1.0)                   # y: hi alone (n == 1: lo == hi, the rows then share the top)
            y[r, hi] = np.float32(20.0)
        elif kind == 6:
            y[r, i] = np.nan
        elif kind == 7:
            x[r, i] = np.inf if r % 2 else -np.inf
    op, oq_ = rng.permutation(rows + 3), rng.permutation(rows + 2)
    P = (rng.standard_normal((rows + 3, n)) * 3.0).astype(np.float32)
    Q = (rng.standard_normal((rows + 2, n)) * 3.0).astype(np.float32)
    P[op[:rows]] = x
    Q[oq_[:rows]] = y
    return P, Q, op[:rows].astype(np.int32), oq_[:rows].astype(np.int32)
