"""The grouped-expert launch cases without a GPU (tests/moe_grouped_cases.py): the table reaches the edges it is there for, the reference is the per-pair
product scattered by the model's grouping, and a launch that read a neighbouring expert's weights or rows could not meet the tolerance - so that
tests/test_gpu_moe_grouped.py cannot pass vacuously.

edges_reached() is what the table's cases reach, computed from their counts.  Per form, the cases' union (a name: the first case that reaches the edge):

    form 0 (tile 256)   empty first / interior expert, one-row batch, 255 / 256 / 257 rows, idle half (129) and none (128): f0_q4k_edges8_n128_k256_ld3;
                        three tiles of one expert: f0_q4k_last_only_n128_k768_ld0; slots at the bound less one: f0_q4k_ones16_n128_k256_ld3;
                        nine row tiles: f0_q4k_edges8_n1152_k256_ld0; 128 / 160 / 256 experts: the qwen128 / qwen160 / max256 cases
    form 1 (tile 256)   the same edges on f1_q4k_edges8_n128_k256_ld3, f1_q4k_last_only_n128_k256_ld3, f1_q4k_ones16_n128_k512_ld0; ten 64-row tiles:
                        f1_q5k_edges8_n640_k256_ld3
    form 2 / 3          tile 32: 31 / 32 / 33 rows (edges9); tile 64: 63 / 64 (edges_mt) / 65 (edges9); tile 128: 127 (edges_mt) / 128 / 129 (edges9);
                        at least three tiles at every tile size (edges8: 257 rows; edges_mt: 385); slots at the bound less one: ones16 at tile 32
                        (the launcher's own choice for it)

Measured minimum of the neighbour-expert difference over every case (test_neighbouring_experts_differ prints it): 0.68 of the batch's scale with the
neighbouring expert's weights, 0.76 with the neighbouring rows - two orders of magnitude above 100 x the tolerance (2e-3, 4e-3 with SwiGLU)."""
import numpy as np
import pytest

import moe_grouped_cases as mc
import select_ref
from moe_grouped_cases import CASES, P2_TOK

FORMS = (0, 1, 2, 3)


def edges_reached(c: dict, tile: int) -> set:
    """What a case's counts reach at a token tile of `tile` rows."""
    n = mc.counts_of(c)
    nz = np.flatnonzero(n)
    out = set()
    if n[0] == 0:
        out.add("empty_first")
    if any(n[e] == 0 for e in range(nz[0] + 1, nz[-1])):
        out.add("empty_interior")
    for v, nm in ((1, "one_row"), (tile - 1, "tile_minus_1"), (tile, "tile"), (tile + 1, "tile_plus_1")):
        if (n == v).any():
            out.add(nm)
    if ((n + tile - 1) // tile >= 3).any():
        out.add("three_tiles")
    if ((n + tile - 1) // tile >= 2).any():
        out.add("second_tile")
    if mc.slot_bound(n, tile) - mc.tiles_used(n, tile) <= 1:
        out.add("slots_at_bound")
    if n[-1] > 0:
        out.add("last_batch_ends_array")
    return out


def test_table_is_well_formed():
    for c in CASES:
        n = mc.counts_of(c)
        ids = mc.DISTS[c["dist"]][1]
        assert n.size == c["n_expert"] <= mc.MOE_MAX_EXPERT and (n >= 0).all() and int(n.sum()) == ids.size >= 1, c["name"]
        assert c["N"] % 128 == 0 and c["ld_out"] >= c["N"], c["name"]
        assert c["K"] % (32 if c["form"] >= 2 else 256) == 0 and (c["type"] == mc.MXFP4) == (c["form"] >= 2), c["name"]
        inp = mc.inputs(c) if c["n_expert"] <= 16 and c["N"] * c["K"] <= 128 * 768 else None
        if inp is not None:                                      # counts sum to R, the offsets are their running sum, x is xp in grouped order
            assert int(inp["counts"].sum()) == inp["R"] == inp["x"].shape[0] and (inp["counts"] == n).all(), c["name"]
            assert (inp["offs"] == np.concatenate(([0], np.cumsum(n)[:-1]))).all(), c["name"]
            assert (inp["x"][inp["slot_of"]] == inp["xp"]).all(), c["name"]
    assert mc.DISTS["max256"][0] == mc.MOE_MAX_EXPERT


def test_tiles_stay_within_the_slots_the_launchers_give():
    """Every case, every tile size it runs at: tiles used <= ceil(R / tile) + n_expert; per form one case within one of that bound."""
    tight = {f: [] for f in FORMS}
    for c in CASES:
        n = mc.counts_of(c)
        for tile in mc.tiles_of(c):
            used, bound = mc.tiles_used(n, tile), mc.slot_bound(n, tile)
            assert used <= bound, (c["name"], tile)
            if bound - used <= 1:
                tight[c["form"]].append((c["name"], tile))
    for f in FORMS:
        assert tight[f], f
    # the copy form reaches it at the tile its launcher picks for that distribution
    for f in (2, 3):
        assert any(tile == mc.q80_tile(mc.counts_of(mc.BY_NAME[nm]), 0) for nm, tile in tight[f]), f


def test_every_form_reaches_every_edge():
    want = {"empty_first", "empty_interior", "one_row", "tile_minus_1", "tile", "tile_plus_1", "three_tiles", "slots_at_bound", "last_batch_ends_array"}
    for f in FORMS:
        tiles = (P2_TOK,) if f < 2 else (32, 64, 128)
        for tile in tiles:
            got = set()
            for c in CASES:
                if c["form"] == f and tile in mc.tiles_of(c):
                    got |= edges_reached(c, tile)
            missing = want - got - ({"slots_at_bound"} if tile in (64, 128) else set())     # (one-row batches fill the slots of the smallest tile only)
            assert not missing, (f, tile, missing)


def test_plane_forms_reach_the_shape_edges():
    """Both plane bodies on every distribution; every N / K on a distribution with a multi-tile expert; more than eight row tiles; both ld_out forms."""
    for f in (0, 1):
        cs = [c for c in CASES if c["form"] == f]
        for d in ("edges8", "last_only", "ones16", "qwen128", "qwen160", "max256"):
            ts = {c["type"] for c in cs if c["dist"] == d}
            assert ts & set(mc.MINS_TYPES) and ts - set(mc.MINS_TYPES), (f, d)
            for t in (mc.Q4_K, mc.Q5_K, mc.Q6_K):
                assert t in ts, (f, d, t)
        for t in (mc.IQ4_XS, mc.TQ1_0, mc.TQ2_0):
            assert {c["dist"] for c in cs if c["type"] == t} >= {"edges8", "qwen128"}, (f, t)
        multi = [c for c in cs if "second_tile" in edges_reached(c, P2_TOK)]
        Ns, Ks = ((128, 1152), (256, 768, 1536)) if f == 0 else ((128, 640), (256, 512))
        for mins in (True, False):
            m2 = [c for c in multi if (c["type"] in mc.MINS_TYPES) == mins]
            assert {c["N"] for c in m2} >= set(Ns) and {c["K"] for c in m2} >= set(Ks), (f, mins)
        full = [t for t in mc.MINS_TYPES if {(c["N"], c["K"]) for c in multi if c["type"] == t} >= {(N, K) for N in Ns for K in Ks}]
        assert full, f                                           # one of the two types with the block-sum term takes every N x K
        assert any((c["N"] + (127 if f == 0 else 63)) // (128 if f == 0 else 64) > 8 for c in multi), f
        assert {c["ld_out"] - c["N"] for c in cs} == {0, 3}, f


def test_copy_forms_reach_the_shape_edges():
    for f in (2, 3):
        cs = [c for c in CASES if c["form"] == f]
        assert {c["dist"] for c in cs} >= set(mc.DISTS), f
        multi = [c for c in cs if "second_tile" in edges_reached(c, 32)]
        assert {c["ld_out"] - c["N"] for c in cs} == {0, 3}, f
        assert {c["K"] for c in multi} >= {96} and {c["N"] for c in multi} >= {128}, f
    multi = [c for c in CASES if c["form"] >= 2 and "second_tile" in edges_reached(c, 32)]
    assert {c["N"] for c in multi} == {128, 384} and {c["K"] for c in multi} == {96, 2080, 4096}
    assert set(mc.TILES_Q80) == {0, 1, 2, 4}


SCATTER = [c["name"] for c in CASES if c["N"] * c["K"] <= 128 * 768 and c["dist"] in ("edges8", "edges9", "ones16", "qwen128", "qwen160")]


@pytest.mark.parametrize("name", SCATTER)
def test_reference_is_the_ungrouped_product_scattered_by_the_grouping(name):
    """The reference of the grouped rows equals the reference of the rows in pair order - pair p = t * k + j through the expert ids[t][j] selects, a few pairs
    per call and in another batching than reference() uses - moved to row slot_of[p] of select_ref.moe_group: bit for bit, every reference being row by row."""
    c = mc.BY_NAME[name]
    inp, ref = mc.prepared(name)
    meta, slot_of, tok_of = select_ref.moe_group(inp["ids"], c["n_expert"])
    assert (meta[:c["n_expert"]] == inp["counts"]).all() and (slot_of == inp["slot_of"]).all()
    k = inp["ids"].shape[1]
    flat = inp["ids"].reshape(-1)
    rng = np.random.default_rng(c["seed"])
    pairs = rng.permutation(flat.size)[:48]
    for e in np.unique(flat[pairs]):
        ps = pairs[flat[pairs] == e]
        got = mc.expert_rows(c, inp, int(e), inp["xp"][ps])
        for o, r in zip(got, ref):
            assert np.array_equal(o.view(np.uint32), r[slot_of[ps]].view(np.uint32)), (name, int(e))
    # (and the rows of the grouped array belong to the tokens the grouping names)
    assert (tok_of == np.argsort(flat, kind="stable") // k).all()


def test_neighbouring_experts_differ(capsys):
    """A launch that read the planes of the expert next door, or that expert's rows, is off by a good part of the batch's scale: on up to four rows of every
    non-empty expert of every case, the relative difference is at least 100 x the tolerance (the MXFP4 forms, compared for equality, against the plane bound)."""
    lo_w, lo_x = np.inf, np.inf
    for c in CASES:
        inp, ref = mc.prepared(c["name"])
        nz = [int(e) for e in np.flatnonzero(inp["counts"])]
        step = max(1, len(nz) // 6)                              # (six experts of the many-expert cases)
        for i in range(0, len(nz), step):
            e, e2 = nz[i], nz[(i + 1) % len(nz)]
            if e2 == e:
                continue
            o, o2 = int(inp["offs"][e]), int(inp["offs"][e2])
            n = min(4, int(inp["counts"][e]), int(inp["counts"][e2]))
            own = [r[o:o + n] for r in ref]
            wrong_w = mc.expert_rows(c, inp, e2, inp["x"][o:o + n])
            wrong_x = mc.expert_rows(c, inp, e, inp["x"][o2:o2 + n])
            for a, bw, bx in zip(own, wrong_w, wrong_x):
                scale = float(np.abs(a).max())
                dw, dx = float(np.abs(a - bw).max()) / scale, float(np.abs(a - bx).max()) / scale
                assert min(dw, dx) >= 100 * mc.tol_rel(c), (c["name"], e, dw, dx)
                lo_w, lo_x = min(lo_w, dw), min(lo_x, dx)
    with capsys.disabled():
        print(f"\nneighbour-expert difference, minimum over {len(CASES)} cases: weights {lo_w:.3g}, rows {lo_x:.3g} of the batch's scale")
    assert min(lo_w, lo_x) >= 100 * 4e-5


def test_bound_is_the_reassociation_bound():
    r = np.array([[3.0, -8.0]], np.float32)
    assert mc.bound(mc.BY_NAME["f0_q4k_edges8_n128_k256_ld3"], r) == pytest.approx(2e-5 * 8.0 + 1e-6)
    assert mc.bound(mc.BY_NAME["f1_q4k_edges8_n128_k256_ld3"], r) == pytest.approx(4e-5 * 8.0 + 1e-6)
    assert mc.bound(mc.BY_NAME["f2_mxfp4_edges9_n128_k96_ld3"], r) == 0.0
