"""Inputs of the arg-max, top-k, grouping, gather and combine tests (tests/test_gpu_select.py), shared with the CPU check that they discriminate
(tests/test_select_cpu.py).  A model's logits and router never produce these: equal maxima in different workgroups' parts, every winner inside one
512-logit list, a winner in the last partial list, -inf, signed zeros, every selection on expert 255."""
from __future__ import annotations

import dataclasses
import functools
import zlib

import numpy as np

F32 = np.float32
ARGMAX_PARTS = 64
TOPK_LIST = 512
TOPK_MAX_ADJ = 192


def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


# ------------------------------------------------------------------------------------------------ arg-max
ARGMAX_NS = (1, 5, 63, 64, 65, 257, 16384, 16385, 32001, 151936)


@functools.lru_cache(maxsize=None)
def argmax_rows_case(n: int):
    """(names, x [rows][n]): every crafted row of one width.  The background is below 1, a planted maximum is 7."""
    rng = _rng(f"argmax-{n}")
    chunk = -(-n // ARGMAX_PARTS)
    names, rows = [], []

    def bg():
        return (rng.random(n, dtype=F32) * 2 - 1).astype(F32)

    def planted(name, *pos):
        if all(0 <= p < n for p in pos) and len(set(pos)) == len(pos):
            v = bg()
            v[list(pos)] = 7.0
            names.append(name); rows.append(v)

    planted("first", 0)
    planted("last", n - 1)
    planted("chunk-end", chunk - 1)
    planted("chunk-start", chunk)
    planted("two-parts", n // 3, n - 1 - n // 5)                    # (different parts for every n >= 5)
    planted("two-parts-adjacent", chunk - 1, chunk)
    lo = (ARGMAX_PARTS // 2) * chunk if n >= ARGMAX_PARTS * 4 else 0
    planted("two-lanes", lo + 2, lo + 3)                            # neighbours in one wave of one part (or, for a narrow row, in two parts)
    planted("two-waves", lo + 5, lo + 5 + 64)
    planted("two-passes", lo + 1, lo + 1 + 256)                     # one thread's first and second element (chunk > 256 only)
    names.append("constant"); rows.append(np.full(n, 0.25, F32))
    names.append("all-neg-inf"); rows.append(np.full(n, -np.inf, F32))
    v = bg(); v[n // 2] = np.inf; v[n - 1] = np.inf
    names.append("pos-inf"); rows.append(v)
    v = bg(); v[::3] = np.nan; v[0] = np.nan; v[n - 1] = np.nan
    if n > 2:
        v[n - 2] = 7.0
    if n > 40:
        v[37] = 7.0
    names.append("nan-beside-max"); rows.append(v)
    names.append("all-nan"); rows.append(np.full(n, np.nan, F32))
    v = np.full(n, -0.0, F32); v[n - 1] = 0.0
    names.append("signed-zeros"); rows.append(v)                    # -0.0 == +0.0: index 0
    return tuple(names), np.stack(rows)


ARGMAX_SEQUENCES = ((2, 1, 3, 4, 1), (4, 4))
ARGMAX_SEQ_NS = (257, 16385)
ARGMAX_CAP_ROWS = 4


@functools.lru_cache(maxsize=None)
def argmax_sequence_case(launches: tuple, n: int):
    """x [sum(launches)][n] with one planted maximum per row, all rows at different places (so a stale part of an earlier launch names another winner)."""
    rng = _rng(f"argmax-seq-{launches}-{n}")
    rows = sum(launches)
    x = (rng.random((rows, n), dtype=F32) * 2 - 1).astype(F32)
    win = rng.permutation(n)[:rows]
    win[0], win[-1] = n - 1, 0
    x[np.arange(rows), win] = 7.0
    return x


# ------------------------------------------------------------------------------------------------ top-k
TOPK_SHAPES = ((1, 1), (300, 16), (512, 128), (128, 128),                    # one list
               (513, 17), (4096, 128), (32768, 16),                          # one merge level
               (4609, 128), (32773, 16), (20000, 33),                        # two
               (33000, 128), (151936, 40), (151936, 128))                    # three


def topk_levels(n: int, k: int) -> int:
    kk = 16
    while kk < k:
        kk <<= 1
    lists, per, levels = -(-n // TOPK_LIST), 1024 // kk, 0
    while lists > 1:                                               # (a single list still passes through one merge launch: that is level 0 here)
        lists = -(-lists // per)
        levels += 1
    return levels


@dataclasses.dataclass(frozen=True)
class TopkCase:
    name: str
    base: np.ndarray               # [B][n]
    rows: tuple                    # base row of each launch row
    k: int
    adjs: tuple                    # per launch row: None or (tok, bias, cnt, repeat, freq, present)


def _winner_rows(n: int, k: int, rng):
    """The placement rows of one shape: (names, base [8][n]).  Background in [-4, -1], winners distinct values in [1, 3] unless said."""
    lists = -(-n // TOPK_LIST)
    m = min(k, n)

    def bg():
        return (-1 - 3 * rng.random(n, dtype=F32)).astype(F32)

    def plant(pos):
        v = bg()
        pos = np.asarray(pos, np.int64)
        v[pos] = rng.permutation(np.linspace(1, 3, pos.size).astype(F32))
        return v

    def in_list(li):
        a, b = li * TOPK_LIST, min(n, (li + 1) * TOPK_LIST)
        a = max(0, b - max(m, b - a))                               # a short last list: the rest comes from the list before it
        return a + rng.permutation(b - a)[:m]

    names, rows = [], []
    names.append("first-list"); rows.append(plant(in_list(0)))
    names.append("middle-list"); rows.append(plant(in_list(lists // 2)))
    names.append("last-list"); rows.append(plant(in_list(lists - 1)))
    own = np.unique(np.linspace(0, lists - 1, m).astype(np.int64))  # one winner per list, the lists spread over the row
    pos = [li * TOPK_LIST + int(rng.integers(0, min(n, (li + 1) * TOPK_LIST) - li * TOPK_LIST)) for li in own]
    names.append("one-per-list"); rows.append(plant(pos))
    edge = [p for p in (0, 511, 512, n - 1) if 0 <= p < n]
    edge = list(dict.fromkeys(edge))[:m]
    rest = np.setdiff1d(rng.permutation(n)[:m + 4], edge)[:m - len(edge)]
    names.append("list-edges"); rows.append(plant(edge + rest.tolist()))
    names.append("seven-values"); rows.append((rng.integers(0, 7, n).astype(F32) - 3).astype(F32))
    v = np.full(n, -np.inf, F32)
    fin = rng.permutation(n)[:m // 2]
    v[fin] = rng.standard_normal(fin.size).astype(F32)
    names.append("neg-inf"); rows.append(v)
    # signed zeros around the cut: m // 2 positive winners, then more zeros of both signs than places are left, the first zero a -0.0
    v = bg()
    order = rng.permutation(n)
    pos_n = m // 2
    v[order[:pos_n]] = np.linspace(1, 3, pos_n).astype(F32) if pos_n else 0
    zeros = np.sort(order[pos_n:pos_n + 2 * (m - pos_n) + 2])
    v[zeros] = np.where(np.arange(zeros.size) % 2 == 0, F32(-0.0), F32(0.0))
    names.append("signed-zeros"); rows.append(v)
    return names, np.stack(rows)


def _adjustments(base: np.ndarray, k: int, rng):
    """One adjustment list per placement row (see the names in _winner_rows), each a different one."""
    B, n = base.shape
    best = [np.lexsort((np.arange(n), -base[r])) for r in range(B)]                  # the unadjusted order of every row
    last_list = np.arange((-(-n // TOPK_LIST) - 1) * TOPK_LIST, n)

    def pick(want, size):
        """`want` first (distinct, in range), then random tokens up to `size` entries: no token twice."""
        want = list(dict.fromkeys(int(t) for t in want if 0 <= t < n))
        fill = [int(t) for t in rng.permutation(n)[:size + len(want)] if int(t) not in set(want)]
        return np.asarray((want + fill)[:min(size, n)], np.int32)

    adjs = [None] * B                                                                # row 0 (first-list): no adjustment
    # row 1: ONE entry, a bias that lifts the last token of the row into the top k (bias with cnt = 0)
    adjs[1] = (np.asarray([n - 1], np.int32), np.asarray([10.0], F32), np.asarray([0], np.int32), 1.0, 0.0, 0.0)
    # row 2: 192 entries, every kind: -inf removes the best token; cnt > 0 on a positive, a negative and (where the row has one) a zero logit; bias with
    # cnt = 0 and cnt > 0 with bias 0; a winner penalised out of the top k; tokens of the last partial list and n - 1
    r = 2
    toks = pick([best[r][0], best[r][1 % n], best[r][min(2, n - 1)], best[r][min(3, n - 1)], n - 1, *last_list[:6], best[r][n - 1]], TOPK_MAX_ADJ)
    bias = np.where(rng.random(toks.size) < 0.5, 0.0, rng.standard_normal(toks.size)).astype(F32)
    cnt = rng.integers(0, 4, toks.size).astype(np.int32)
    bias[0] = -np.inf; cnt[0] = 0
    if toks.size > 3:
        bias[1], cnt[1] = 0.5, 2                                                     # bias and penalty on a winner that stays: the order of the two shows
        bias[2], cnt[2] = 0.25, 0                                                    # cnt = 0: `present` must not apply
        bias[3], cnt[3] = 0.0, 100                                                   # 100 * freq: falls out of the top k
    adjs[2] = (toks, bias, cnt, 1.3, 0.1, 0.2)
    # row 3: 192 entries, repeat 1.0
    toks = pick([*best[3][:4], n - 1, *last_list[-3:]], TOPK_MAX_ADJ)
    adjs[3] = (toks, rng.standard_normal(toks.size).astype(F32), rng.integers(0, 3, toks.size).astype(np.int32), 1.0, 0.1, 0.0)
    # row 4: freq 0, present 0.2, cnt > 0 with bias 0 on the winners
    toks = pick([*best[4][:6], n - 1], 40)
    adjs[4] = (toks, np.zeros(toks.size, F32), rng.integers(1, 5, toks.size).astype(np.int32), 1.3, 0.0, 0.2)
    # row 5 (seven values: -3 .. 3, zeros among them): penalties on zero, positive and negative logits; biases that make new ties and new zeros
    zero = np.flatnonzero(base[5] == 0)
    toks = pick([*zero[:8], *best[5][:8], *best[5][-4:], n - 1], TOPK_MAX_ADJ)
    bias = rng.integers(-2, 3, toks.size).astype(F32)
    cnt = rng.integers(0, 3, toks.size).astype(np.int32)
    bias[:4] = 0.0; cnt[:4] = 1
    adjs[5] = (toks, bias, cnt, 1.3, 0.1, 0.2)
    # row 6 (-inf everywhere but k / 2 entries): biases and penalties on -inf entries (they stay -inf) and on the finite ones
    toks = pick([*best[6][:3], n - 1, 0], 12)
    bias = rng.standard_normal(toks.size).astype(F32)
    cnt = rng.integers(0, 2, toks.size).astype(np.int32)
    adjs[6] = (toks, bias, cnt, 1.3, 0.1, 0.2)
    # row 7 (signed zeros): bias 0 on a -0.0 (-0.0 + 0 = +0.0) and penalties that keep a zero a zero - and repeat = 0, the one finite setting at which
    # `l <= 0` and `l < 0` part on a zero logit (0 * 0 = 0, 0 / 0 = NaN); a positive logit becomes +inf, a negative one -0.0
    zero = np.flatnonzero(base[7] == 0)
    toks = pick([*zero[:6], *best[7][:2], n - 1], 16)
    cnt = np.ones(toks.size, np.int32)
    cnt[1::3] = 0
    adjs[7] = (toks, np.zeros(toks.size, F32), cnt, 0.0, 0.0, 0.0)
    return adjs


@functools.lru_cache(maxsize=None)
def topk_cases(n: int, k: int):
    """The launches of one shape: all eight placement rows without adjustments, the same rows each with its own adjustment list, one row alone, and three
    rows through an indirection with a repeated base row."""
    rng = _rng(f"topk-{n}-{k}")
    names, base = _winner_rows(n, k, rng)
    adjs = _adjustments(base, k, rng)
    tag = f"n{n}-k{k}"
    B = base.shape[0]
    return (TopkCase(f"{tag}-plain8", base, tuple(range(B)), k, (None,) * B),
            TopkCase(f"{tag}-adj8", base, tuple(range(B)), k, tuple(adjs)),
            TopkCase(f"{tag}-adj1", base, (2,), k, (adjs[2],)),
            TopkCase(f"{tag}-rows3", base, (2, 0, 2), k, (adjs[2], adjs[1], adjs[5])))


TOPK_ROW_NAMES = ("first-list", "middle-list", "last-list", "one-per-list", "list-edges", "seven-values", "neg-inf", "signed-zeros")


# ------------------------------------------------------------------------------------------------ grouping
GROUP_SHAPES = ((1, 1, 1), (5, 2, 8), (7, 8, 60), (33, 8, 128), (40, 8, 256), (512, 8, 128), (64, 1, 3), (63, 1, 4), (65, 3, 5))
GROUP_LIMIT = (7680, 8, 256)                  # 60 * 1024 selections: the kernel's limit
GROUP_PATTERNS = ("uniform", "all-last", "all-first", "upper-only", "few-used", "descending")


@functools.lru_cache(maxsize=None)
def group_ids(T: int, k: int, n_expert: int, pattern: str) -> np.ndarray:
    """ids [T][k] int32.  uniform: k distinct experts per token where there are k; upper-only: experts >= 64 (the upper half of fewer than 128);
    few-used: 200 of 256 experts (the same share of fewer) never chosen; descending: a token's ranks in falling expert order."""
    rng = _rng(f"group-{T}-{k}-{n_expert}-{pattern}")

    def distinct(lo, pool):
        pool = np.asarray(pool)
        if pool.size >= k:
            return np.stack([lo + rng.permutation(pool)[:k] for _ in range(T)])
        return lo + rng.choice(pool, (T, k))

    if pattern == "uniform":
        ids = distinct(0, np.arange(n_expert))
    elif pattern == "all-last":
        ids = np.full((T, k), n_expert - 1)
    elif pattern == "all-first":
        ids = np.zeros((T, k))
    elif pattern == "upper-only":
        lo = 64 if n_expert > 64 else n_expert // 2
        ids = distinct(lo, np.arange(n_expert - lo))
    elif pattern == "few-used":
        used = np.sort(rng.permutation(n_expert)[:max(1, n_expert * 56 // 256)])
        ids = distinct(0, used)
    elif pattern == "descending":
        ids = -np.sort(-distinct(0, np.arange(n_expert)), axis=1)
    else:
        raise ValueError(pattern)
    return np.ascontiguousarray(ids, np.int32)


def group_cases():
    for shape in GROUP_SHAPES:
        for p in GROUP_PATTERNS:
            yield (*shape, p)
    for p in ("uniform", "all-last"):
        yield (*GROUP_LIMIT, p)


# ------------------------------------------------------------------------------------------------ gather and combine
GATHER_ACT_KS = (256, 768, 4096, 5632)
GATHER_ACT_TS = ((3, 4), (40, 2))             # (T, k): n_rows = T * k, every token k times
GATHER_ACT_FORMS = ("q8k", "q80", "both")
GUARD = 0xA5


@functools.lru_cache(maxsize=None)
def gather_act_case(K: int, T: int, k: int):
    """(planes (qs, d, bsums, qs0, d0) as uint8 [T][row bytes] of seeded random bytes, tok_of [T * k]: the rows of a random grouping)."""
    rng = _rng(f"gather-act-{K}-{T}-{k}")
    planes = tuple(rng.integers(0, 256, (T, nb), dtype=np.uint8) for nb in (K, K // 256 * 4, K // 16 * 2, K, K // 32 * 2))
    tok_of = np.argsort(rng.integers(0, 8, T * k), kind="stable") // k
    return planes, tok_of.astype(np.int32)


COMBINE_SHAPES = ((1, 256, 1), (5, 768, 2), (40, 2048, 8), (33, 100, 4))


@functools.lru_cache(maxsize=None)
def combine_case(T: int, E: int, k: int):
    """(x [T][E], eo [k][T][E], w [T][k], ids [T][k] over 16 experts for the grouped form)."""
    rng = _rng(f"combine-{T}-{E}-{k}")
    x = rng.standard_normal((T, E)).astype(F32)
    eo = rng.standard_normal((k, T, E)).astype(F32)
    w = rng.random((T, k)).astype(F32)
    w = (w / w.sum(axis=1, keepdims=True)).astype(F32)
    ids = np.stack([rng.permutation(16)[:k] for _ in range(T)]).astype(np.int32)
    return x, eo, w, ids


GATHER_ROWS_NS = (1, 255, 4096, 5000)


@functools.lru_cache(maxsize=None)
def gather_rows_case(n: int):
    """(src [9][n], row lists: descending, duplicates, one row)."""
    rng = _rng(f"gather-rows-{n}")
    src = rng.standard_normal((9, n)).astype(F32)
    return src, ((8, 7, 6, 5, 4, 3, 2, 1, 0), (3, 3, 0, 8, 3, 0, 8, 8), (5,), tuple(int(v) for v in rng.integers(0, 9, 40)))


# ------------------------------------------------------------------------------------------------ router ties
ROUTE_TIE_SHAPES = ((8, 2), (64, 4), (128, 8), (256, 8), (160, 4))


@functools.lru_cache(maxsize=None)
def route_tie_case(n_expert: int, k: int):
    """(logits [rows][n_expert], tied: per row the experts with bit-equal logits, or None).  Each tie row has k - m // 2 experts above a group of m equal
    ones, so that the cut falls inside the group; the underflow rows have logits 200 below the maximum, whose probability is exactly 0."""
    rng = _rng(f"route-tie-{n_expert}-{k}")
    groups = [(3, 5), (1, 6, 7)]
    if n_expert > 64:
        groups += [(9, 9 + 64), (63, 64), (2, 40, 2 + 64, 40 + 64)]
    if n_expert > 192:
        groups += [(17, 17 + 64, 17 + 128, 17 + 192), (200, 255), (0, 255)]
    rows, tied = [], []
    for g in groups:
        lg = np.minimum(rng.standard_normal(n_expert) * 2, 4.0).astype(F32)
        above = [e for e in rng.permutation(n_expert) if e not in g][:max(0, k - max(1, len(g) // 2))]
        lg[above] = (8 + np.arange(len(above))).astype(F32)
        lg[list(g)] = F32(6.5)
        rows.append(lg); tied.append(g)
    for n_max in (1, max(1, k - 1)):                               # fewer experts with p > 0 than k: the rest of the picks are the lowest indices
        lg = np.full(n_expert, -200.0, F32)
        lg[rng.permutation(n_expert)[:n_max]] = 0.0
        rows.append(lg); tied.append(None)
    lg = np.full(n_expert, -200.0, F32); lg[n_expert - 1] = 0.0
    rows.append(lg); tied.append(None)
    return np.stack(rows), tuple(tied)
