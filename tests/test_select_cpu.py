"""The inputs of tests/test_gpu_select.py discriminate (no GPU): for every builder of tests/select_cases.py the reference of tests/select_ref.py and a list
of deliberately wrong restatements run on the shared cases, and every wrong one must differ from the reference on at least one case - a crafted input
that a wrong kernel would also pass is worth nothing.  The restatements follow the kernels' structure (64 parts per row; 512-logit lists, KK kept per list,
1024 / KK lists per merge block; 64 selections per ballot) so that a fault can be put where a kernel could have it; without a fault they must equal the
references on every case, which also ties the references' order to the 64-bit keys the device compares."""
import functools

import numpy as np
import pytest

import select_cases as sc
import select_ref as ref

F32 = np.float32
BIG = 0x7fffffff


# ------------------------------------------------------------------------------------------------ arg-max
def argmax_model(x, bug=None):
    out = np.zeros(x.shape[0], np.int32)
    hi_wins = bug == "ties-high"
    for r, v in enumerate(x):
        n = v.size
        chunk = -(-n // sc.ARGMAX_PARTS)
        best, idx = -np.inf, BIG
        for p in range(sc.ARGMAX_PARTS):
            lo, hi = p * chunk, min(n, (p + 1) * chunk)
            if lo >= hi or (bug == "skip-last-part" and hi == n):
                continue
            seg = v[lo:hi]
            nan = np.isnan(seg)
            if bug == "nan-wins" and nan.any():
                pb, pi = np.inf, lo + int(np.flatnonzero(nan)[0])
            elif nan.all():
                continue
            else:
                pb = seg[~nan].max()
                hit = np.flatnonzero(~nan & (seg == pb))
                pi = lo + int(hit[-1] if hi_wins else hit[0])
            if pb > best or (pb == best and ((pi > idx or idx == BIG) if hi_wins else pi < idx)):
                best, idx = pb, pi
        out[r] = 0 if idx == BIG else idx
    return out


ARGMAX_BUGS = ("ties-high", "skip-last-part", "nan-wins")


def test_argmax_model_is_the_reference():
    for n in sc.ARGMAX_NS:
        names, x = sc.argmax_rows_case(n)
        assert argmax_model(x).tolist() == ref.argmax_rows(x).tolist(), n
        want = dict(zip(names, ref.argmax_rows(x).tolist()))
        assert want["constant"] == 0 and want["all-neg-inf"] == 0 and want["all-nan"] == 0 and want["signed-zeros"] == 0
        assert want["last"] == n - 1 and want["pos-inf"] == n // 2
    for seq in sc.ARGMAX_SEQUENCES:
        for n in sc.ARGMAX_SEQ_NS:
            w = ref.argmax_rows(sc.argmax_sequence_case(seq, n))
            assert len(set(w.tolist())) == w.size                     # consecutive launches never share a winner


@pytest.mark.parametrize("bug", ARGMAX_BUGS)
def test_argmax_cases_catch(bug):
    caught = [n for n in sc.ARGMAX_NS if argmax_model(sc.argmax_rows_case(n)[1], bug).tolist() != ref.argmax_rows(sc.argmax_rows_case(n)[1]).tolist()]
    assert caught, bug
    if bug != "skip-last-part":
        assert len(caught) >= len(sc.ARGMAX_NS) - 1, (bug, caught)      # (n = 1 has no second entry to tie with)


# ------------------------------------------------------------------------------------------------ top-k
def adjust_model(row, adj, bug, first_list_only):
    l = np.array(row, F32, copy=True)
    if adj is None:
        return l
    toks, bias, cnt, repeat, freq, present = adj
    repeat, freq, present = F32(repeat), F32(freq), F32(present)
    with np.errstate(all="ignore"):
        for t, b, c in zip(toks, bias, cnt):
            if first_list_only and t >= sc.TOPK_LIST:
                continue
            v = l[t]
            if bug != "penalty-before-bias":
                v = F32(v + F32(b))
            if c > 0:
                neg = v < 0 if bug == "lt-zero" else v <= 0
                v = F32(v * repeat) if neg else F32(v / repeat)
                v = F32(v - F32(F32(F32(c) * freq) + present))
            elif bug == "present-without-count":
                v = F32(v - present)
            if bug == "penalty-before-bias":
                v = F32(v + F32(b))
            l[t] = v
    return l


def keys_of(l, ties_high):
    u = np.ascontiguousarray(l, F32).view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    u = np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    tok = np.arange(l.size, dtype=np.uint64)
    return (u << np.uint64(32)) | (tok if ties_high else np.uint64(0xffffffff) - tok)


def topk_model(case, bug=None):
    """The launches of launch_topk_rows on 64-bit keys: (tokens, logits)."""
    B, n = case.base.shape
    k = case.k
    kk = 16
    while kk < k:
        kk <<= 1
    per = 1024 // kk
    out = np.zeros((len(case.rows), k), np.uint64)
    for r, br in enumerate(case.rows):
        adj = case.adjs[0 if bug == "adj-of-row-0" else r]
        l = adjust_model(case.base[r if bug == "base-row-r" else br], adj, bug, bug == "adjust-first-list-only")
        keys = keys_of(l, bug == "ties-high")
        L = -(-n // sc.TOPK_LIST)
        pad = np.zeros(L * sc.TOPK_LIST, np.uint64)
        pad[:n] = keys
        lists = np.sort(pad.reshape(L, sc.TOPK_LIST), axis=1)[:, ::-1][:, :kk].copy()
        if bug == "skip-last-list" and n % sc.TOPK_LIST:
            lists[-1] = 0
        if bug == "keep-half":
            lists[:, kk // 2:] = 0
        while True:
            blocks = -(-lists.shape[0] // per)
            nxt = np.zeros((blocks, kk), np.uint64)
            for b in range(blocks):
                mine = lists[b * per:(b + 1) * per]
                if bug == "merge-drops-last-list":
                    mine = mine[:-1]
                s = np.zeros(1024, np.uint64)
                s[:mine.size] = mine.reshape(-1)
                nxt[b] = np.sort(s)[::-1][:kk]
            lists = nxt
            if blocks == 1:
                break
        out[r] = lists[0, :k]
    u = (out >> np.uint64(32)).astype(np.uint32)
    u = np.where(u >> np.uint32(31), u ^ np.uint32(0x80000000), ~u).astype(np.uint32)
    low = (out & np.uint64(0xffffffff)).astype(np.uint32)
    toks = (low if bug == "ties-high" else np.uint32(0xffffffff) - low).astype(np.uint32).view(np.int32)
    return toks, u.view(F32)


TOPK_BUGS = ("ties-high", "skip-last-list", "keep-half", "merge-drops-last-list", "adjust-first-list-only", "penalty-before-bias", "present-without-count",
             "lt-zero", "base-row-r", "adj-of-row-0")


@functools.lru_cache(maxsize=None)
def topk_ref(n, k, i):
    c = sc.topk_cases(n, k)[i]
    return ref.topk_rows(c.base, c.rows, c.k, c.adjs)


def same(a, b):
    return a[0].tolist() == b[0].tolist() and a[1].view(np.uint32).tolist() == b[1].view(np.uint32).tolist()


def test_topk_shapes_have_the_levels_they_are_listed_under():
    assert [sc.topk_levels(n, k) for n, k in sc.TOPK_SHAPES] == [0] * 4 + [1] * 3 + [2] * 3 + [3] * 3


@pytest.mark.parametrize("n,k", sc.TOPK_SHAPES)
def test_topk_model_is_the_reference(n, k):
    for i, c in enumerate(sc.topk_cases(n, k)):
        want = topk_ref(n, k, i)
        assert same(topk_model(c), want), c.name
        assert (ref.topk_keys(*want) == ref.topk_keys(*topk_model(c))).all()
        for adj in c.adjs:
            assert adj is None or (len(set(adj[0].tolist())) == adj[0].size and adj[0].size <= sc.TOPK_MAX_ADJ)      # no token twice (plan_front)
        for r in range(len(c.rows)):                                                     # ranks fall, ties in token order
            l, t = want[1][r], want[0][r]
            assert all(l[j] > l[j + 1] or (l[j] == l[j + 1] and t[j] < t[j + 1]) for j in range(k - 1))


def test_topk_cases_hold_what_they_are_named_for():
    """-inf candidates are returned, a penalised winner leaves the top k, a biased token enters it, signed zeros sit on both sides of the cut."""
    for n, k in sc.TOPK_SHAPES[1:]:
        plain, adj8 = sc.topk_cases(n, k)[0], sc.topk_cases(n, k)[1]
        tp, lp = topk_ref(n, k, 0)
        ta, la = topk_ref(n, k, 1)
        i = sc.TOPK_ROW_NAMES.index
        assert np.isneginf(lp[i("neg-inf")]).sum() >= k - k // 2
        z = plain.base[i("signed-zeros")]
        zeros = np.flatnonzero(z == 0)
        assert np.signbit(z[zeros]).any() and not np.signbit(z[zeros]).all()
        assert n == k or zeros.size > (lp[i("signed-zeros")] == 0).sum() > 0               # (n == k: the whole row comes back)
        assert n - 1 in ta[1] and (n - 1 in tp[1]) == (plain.base[1, n - 1] > 0)         # the bias of row 1 lifts token n - 1 in
        assert n == k or tp[2][0] not in ta[2]                                               # -inf bias: the best token of row 2 is gone
        if n > 4 * k:
            assert tp[2][3] not in ta[2]                                                 # penalised out
            assert adj8.adjs[2][0][1] in ta[2] and adj8.adjs[2][0][2] in ta[2]


@pytest.mark.parametrize("bug", TOPK_BUGS)
def test_topk_cases_catch(bug):
    caught = []
    for n, k in sc.TOPK_SHAPES:
        if n > 40000 and caught:
            continue                                                                     # (the widest rows only where nothing narrower caught it)
        for i, c in enumerate(sc.topk_cases(n, k)):
            if not same(topk_model(c, bug), topk_ref(n, k, i)):
                caught.append(c.name)
    assert caught, bug
    levels = {sc.topk_levels(int(name.split("-")[0][1:]), int(name.split("-")[1][1:])) for name in caught}
    if bug in ("merge-drops-last-list", "adjust-first-list-only"):                       # (faults that need a second list)
        assert levels >= {1, 2}, (bug, caught)
    elif bug != "skip-last-list":
        assert levels >= {0, 1, 2}, (bug, caught)


# ------------------------------------------------------------------------------------------------ grouping
def group_model(ids, n_expert, bug=None):
    T, k = ids.shape
    flat = ids.reshape(-1).astype(np.int64)
    n_sel = flat.size
    if bug == "mod-128":
        flat = flat % 128
    if bug == "mod-64":
        flat = flat % 64
    seen = n_sel - n_sel % 64 if bug == "ballot-tail-ignored" else n_sel
    counts = np.bincount(flat[:seen], minlength=n_expert)[:n_expert]
    offs = np.concatenate(([0], np.cumsum(counts)))
    slot_of = np.full(n_sel, -1, np.int32)
    tok_of = np.full(n_sel, -1, np.int32)
    for e in range(n_expert):
        hit = np.flatnonzero(flat[:seen] == e)
        if bug == "reversed-within-expert":
            hit = hit[::-1]
        rows = offs[e] + np.arange(hit.size)
        slot_of[hit] = rows
        tok_of[rows] = hit % k if bug == "tok-is-rank" else hit // k
    return np.concatenate((counts, offs)).astype(np.int32), slot_of, tok_of


GROUP_BUGS = ("mod-128", "mod-64", "ballot-tail-ignored", "reversed-within-expert", "tok-is-rank")


def group_same(a, b):
    return all(x.tolist() == y.tolist() for x, y in zip(a, b))


def test_group_model_is_the_reference():
    for T, k, ne, p in sc.group_cases():
        ids = sc.group_ids(T, k, ne, p)
        assert ids.shape == (T, k) and ids.min() >= 0 and ids.max() < ne
        meta, slot_of, tok_of = ref.moe_group(ids, ne)
        assert group_same(group_model(ids, ne), (meta, slot_of, tok_of)), (T, k, ne, p)
        assert sorted(slot_of.tolist()) == list(range(T * k)) and (tok_of[slot_of] == np.arange(T * k) // k).all()
        assert meta.size == 2 * ne + 1 and meta[2 * ne] == T * k
    ids = sc.group_ids(40, 8, 256, "all-last")
    assert (ids == 255).all()
    assert (sc.group_ids(40, 8, 256, "upper-only") >= 64).all()
    assert (ref.moe_group(sc.group_ids(40, 8, 256, "few-used"), 256)[0][:256] == 0).sum() >= 200
    d = sc.group_ids(40, 8, 256, "descending")
    assert (np.diff(d, axis=1) < 0).all()


@pytest.mark.parametrize("bug", GROUP_BUGS)
def test_group_cases_catch(bug):
    caught = [c for c in sc.group_cases() if c[0] < 1000 and not group_same(group_model(sc.group_ids(*c), c[2], bug), ref.moe_group(sc.group_ids(*c), c[2]))]
    assert caught, bug


# ------------------------------------------------------------------------------------------------ combine
def combine_model(x, eo, w, bug):
    if bug == "ranks-reversed":
        return ref.moe_combine(x, eo[::-1], w[:, ::-1])
    o = x + eo[0] * w[:, 0:1]                                      # "residual-first"
    for j in range(1, eo.shape[0]):
        o = o + eo[j] * w[:, j:j + 1]
    return o


@pytest.mark.parametrize("bug", ("ranks-reversed", "residual-first"))
def test_combine_cases_catch(bug):
    caught = []
    for shape in sc.COMBINE_SHAPES:
        x, eo, w, ids = sc.combine_case(*shape)
        want = ref.moe_combine(x, eo, w)
        if combine_model(x, eo, w, bug).view(np.uint32).tolist() != want.view(np.uint32).tolist():
            caught.append(shape)
        # the grouped form of the same data is the same sum
        T, E, k = shape
        _, slot_of, _ = ref.moe_group(ids, 16)
        y = np.zeros((T * k, E), F32)
        y[slot_of.reshape(T, k)] = eo.transpose(1, 0, 2)
        assert ref.moe_scatter_combine(x, y, w, slot_of).view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert caught, bug
    # one rank has nothing to reorder, and two products commute in their one sum
    assert caught == [s for s in sc.COMBINE_SHAPES if s[2] >= (3 if bug == "ranks-reversed" else 2)]


def test_gather_cases_repeat_tokens():
    for K in sc.GATHER_ACT_KS:
        for T, k in sc.GATHER_ACT_TS:
            planes, tok_of = sc.gather_act_case(K, T, k)
            assert sorted(tok_of.tolist()) == sorted(list(range(T)) * k) and (np.diff(tok_of) < 0).any()
            assert [p.shape[1] for p in planes] == [K, K // 64, K // 8, K, K // 16]
