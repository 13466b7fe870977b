"""Op-level tests of the kernels that produce indices (csrc/misc.hip), each against its plain numpy reference in tests/select_ref.py on the crafted inputs
of tests/select_cases.py: row arg-max, top-k of a logits row, the grouping of a prompt batch's expert selections, the copies into and the weighted sums out
of the grouped rows, the output-row gather, and the router on tied logits.  The kernels are exact by construction (the build contracts no multiply-add, the
keys compare as integers), so every assertion is an equality: uint32 views for floats, ids as they are.  tests/test_select_cpu.py shows that these inputs
tell the references from wrong restatements of the kernels.

Top-k takes no NaN inputs: the host sampler's `better` is not an order on them."""
import numpy as np
import pytest

import select_cases as sc
import select_ref as ref
from test_gpu_qwen3moe import kernel_selection

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ arg-max
@pytest.mark.parametrize("n", sc.ARGMAX_NS)
def test_argmax_rows(be, n):
    """Every crafted row of one width in one launch: the maximum at the ends of the row and of a part, twice in two parts / two lanes / two waves / one
    thread's two passes (the lowest index wins), constant and all -inf rows (0), +inf, NaNs beside a finite maximum (never win), an all-NaN row (0)."""
    names, x = sc.argmax_rows_case(n)
    want = ref.argmax_rows(x)
    got = be.argmax_rows(x)
    assert dict(zip(names, got.tolist())) == dict(zip(names, want.tolist()))
    assert got[names.index("all-nan")] == 0


@pytest.mark.parametrize("n", sc.ARGMAX_SEQ_NS)
@pytest.mark.parametrize("launches", sc.ARGMAX_SEQUENCES)
def test_argmax_launch_sequence(be, launches, n):
    """Launches of 2, 1, 3, 4, 1 rows (and 4, 4) back to back on ONE scratch of four rows, zeroed once: every launch finds its ticket words re-armed and at
    the same place whatever its row count, and no row takes a part of an earlier launch for its own (all rows have different winners)."""
    x = sc.argmax_sequence_case(launches, n)
    got = be.argmax_rows(x, launches=launches, cap_rows=sc.ARGMAX_CAP_ROWS)
    assert got.tolist() == ref.argmax_rows(x).tolist()


def test_argmax_refuses(be, pkg):
    x = np.zeros((5, 8), np.float32)
    for launches in ((5,), (4, 0, 1), (2, -1, 4)):
        with pytest.raises(pkg.binding.MI355Error, match="cap_rows"):
            be.argmax_rows(x, launches=launches, cap_rows=4)


# ------------------------------------------------------------------------------------------------ top-k
@pytest.mark.parametrize("n,k", sc.TOPK_SHAPES)
def test_topk_rows(be, n, k):
    """One shape per number of merge levels and list geometry (tests/select_cases.py TOPK_SHAPES).  Rows: all k winners inside the first, a middle and the
    last partial 512-list; one winner per list; winners at 511 | 512 and n - 1; seven distinct values (ties across lists and merge blocks go to the lower
    token id); -inf in more than n - k entries (-inf candidates come back, above the padding key); signed zeros around the cut (they tie on the token id, and
    come back as +0.0).  Launches: the eight rows plain (adj_n = 0); each with its own adjustment list (adj_n 1, 12 .. 192: biases that lift a token in, -inf
    that removes the best one, penalties on positive, negative and zero logits with repeat 1.0 / 1.3 / 0, freq 0 / 0.1, present 0 / 0.2, bias with cnt = 0,
    cnt > 0 with bias 0, tokens of the last partial list and n - 1); one row alone; rows [2, 0, 2] of the base with three different lists.  Tokens, logit
    bits (those of adjusted tokens among them) and the raw keys equal the reference's.  No NaN inputs: `better` is not an order on them."""
    for c in sc.topk_cases(n, k):
        want_t, want_l = ref.topk_rows(c.base, c.rows, c.k, c.adjs)
        toks, logits, keys = be.topk_rows(c.base, c.rows, c.k, c.adjs)
        for r in range(len(c.rows)):
            what = (c.name, r, sc.TOPK_ROW_NAMES[c.rows[r]])
            assert toks[r].tolist() == want_t[r].tolist(), what
            assert bits(logits[r]).tolist() == bits(want_l[r]).tolist(), what
        assert (keys == ref.topk_keys(want_t, want_l)).all(), c.name
        assert (keys > 0).all()                                         # no padding key among k <= n candidates, -inf ones included
        for r, adj in enumerate(c.adjs):                                # the adjusted tokens that were returned carry the reference's adjusted logit
            if adj is not None:
                l = ref.topk_adjust(c.base[c.rows[r]], adj)
                hit = np.isin(toks[r], adj[0])
                assert bits(logits[r][hit]).tolist() == bits(l[toks[r][hit]] + np.float32(0)).tolist(), (c.name, r)


def test_topk_refuses(be, pkg):
    base = np.zeros((3, 100), np.float32)
    err = pkg.binding.MI355Error
    for k in (0, 129, 101):
        with pytest.raises(err, match="k outside"):
            be.topk_rows(base, (0,), k)
    for an in (-1, 193):
        with pytest.raises(err, match="adj_n"):
            be.topk_rows(base, (0, 1), 4, adj_n=(0, an))
    for rows in ((3,), (0, -1)):
        with pytest.raises(err, match="rows"):
            be.topk_rows(base, rows, 4)


# ------------------------------------------------------------------------------------------------ grouping
@pytest.mark.parametrize("T,k,n_expert,pattern", list(sc.group_cases()))
def test_moe_group(be, T, k, n_expert, pattern):
    """meta (counts, exclusive offsets, the total at [2 n_expert]), slot_of and tok_of equal the stable counting sort; slot_of is a permutation of [0, T k)
    and tok_of[slot_of[i]] == i // k.  Patterns: uniform, every pair on the last expert (255: an id that a signed or narrower staging would wrap), on expert
    0, experts >= 64 only, 200 of 256 experts unused, a token's ranks in falling expert order; T k not a multiple of the ballot's 64, and the 60 K limit."""
    ids = sc.group_ids(T, k, n_expert, pattern)
    meta_r, slot_r, tok_r = ref.moe_group(ids, n_expert)
    meta, slot_of, tok_of = be.moe_group(ids, n_expert)
    assert meta.tolist() == meta_r.tolist()
    assert np.sort(slot_of).tolist() == list(range(T * k))
    assert (tok_of[slot_of] == np.arange(T * k) // k).all()
    assert slot_of.tolist() == slot_r.tolist() and tok_of.tolist() == tok_r.tolist()


def test_moe_group_refuses(be, pkg):
    err = pkg.binding.MI355Error
    with pytest.raises(err, match="T \\* k"):
        be.moe_group(np.zeros((60 * 1024 + 1, 1), np.int32), 8)
    for ne in (257, 0):
        with pytest.raises(err, match="n_expert"):
            be.moe_group(np.zeros((4, 2), np.int32), ne)
    with pytest.raises(err, match="ids"):
        be.moe_group(np.full((4, 2), 8, np.int32), 8)


# ------------------------------------------------------------------------------------------------ gather and combine
@pytest.mark.parametrize("form", sc.GATHER_ACT_FORMS)
@pytest.mark.parametrize("T,k", sc.GATHER_ACT_TS)
@pytest.mark.parametrize("K", sc.GATHER_ACT_KS)
def test_moe_gather_act(be, K, T, k, form):
    """Every plane of the wanted form(s) byte-equal to the gathered rows, the guard row behind each unchanged, the planes of the other form not touched."""
    planes, tok_of = sc.gather_act_case(K, T, k)
    given = [p if (form != "q80" and i < 3) or (form != "q8k" and i >= 3) else None for i, p in enumerate(planes)]
    out = be.moe_gather_act(given, tok_of, K, guard=sc.GUARD)
    for i, (p, o) in enumerate(zip(given, out)):
        assert (p is None) == (o is None)
        if p is not None:
            assert o.shape == (T * k + 1, p.shape[1])
            assert (o[:-1] == ref.gather_rows(p, tok_of)).all(), i
            assert (o[-1] == sc.GUARD).all(), i


def test_moe_gather_act_refuses(be, pkg):
    planes = [np.zeros((2, nb), np.uint8) for nb in (300, 4, 36, 300, 18)]
    with pytest.raises(pkg.binding.MI355Error, match="multiple of 256"):
        be.moe_gather_act(planes, (0, 1), 300)


@pytest.mark.parametrize("T,E,k", sc.COMBINE_SHAPES)
def test_moe_combine(be, T, E, k):
    """Both combines bit-equal to the f32 reference in the kernels' order (ranks in order, then the residual), and the grouped form on slot_of from the
    grouping op equal to the plain form on the same data."""
    x, eo, w, ids = sc.combine_case(T, E, k)
    want = ref.moe_combine(x, eo, w)
    plain = be.moe_combine(x, eo, w)
    assert bits(plain).tolist() == bits(want).tolist()
    _, slot_of, _ = be.moe_group(ids, 16)
    y = np.zeros((T * k, E), np.float32)
    y[slot_of.reshape(T, k)] = eo.transpose(1, 0, 2)                    # rank j of token t at its grouped row
    grouped = be.moe_combine(x, y, w, slot_of=slot_of)
    assert bits(grouped).tolist() == bits(ref.moe_scatter_combine(x, y, w, slot_of)).tolist()
    assert bits(grouped).tolist() == bits(plain).tolist()


@pytest.mark.parametrize("n", sc.GATHER_ROWS_NS)
def test_gather_rows_f32(be, pkg, n):
    src, lists = sc.gather_rows_case(n)
    for rows in lists:
        assert bits(be.gather_rows_f32(src, rows)).tolist() == bits(ref.gather_rows(src, rows)).tolist(), rows
    with pytest.raises(pkg.binding.MI355Error, match="rows"):
        be.gather_rows_f32(src, (0, 9))


# ------------------------------------------------------------------------------------------------ router ties
@pytest.mark.parametrize("n_expert,k", sc.ROUTE_TIE_SHAPES)
def test_moe_route_ties(be, n_expert, k):
    """mi355_op_moe_route on logits a router never produces: two to four experts with bit-equal logits straddling the k cut, in different lanes and 64
    apart (one lane's registers e and e + 64), and rows whose other logits lie 200 below the maximum, so that p is exactly 0 for more experts than
    n_expert - k.  The ids are the lowest indices among equals; ids equal the numpy restatement of the kernel's arithmetic and the weights lie within the
    difference between the device's expf and libm's (the cap of tests/test_gpu_qwen3moe.py) - and are bit-equal where every p is 0 or 1."""
    lg, tied = sc.route_tie_case(n_expert, k)
    ids, w = be.moe_route(lg, k)
    for t in range(lg.shape[0]):
        ids_r, w_r = kernel_selection(lg[t], k)
        assert ids[t].tolist() == ids_r.tolist(), (t, tied[t])
        assert len(set(ids[t].tolist())) == k
        if tied[t] is not None:
            g = sorted(tied[t])
            inside = [e for e in ids[t].tolist() if e in g]
            assert 0 < len(inside) < len(g) and inside == g[:len(inside)], (t, g, ids[t])
            assert np.abs(w[t] - w_r).max() <= 4e-7 * max(1.0, float(w_r.max())), t
        else:
            top = np.flatnonzero(lg[t] == 0).tolist()
            zero_p = [e for e in range(n_expert) if e not in top]
            assert ids[t].tolist() == (top + zero_p)[:k], t
            assert bits(w[t]).tolist() == bits(w_r).tolist(), t
            assert (w[t][len(top):] == 0).all()
