"""The prompt mat-mul cases without a GPU (tests/prompt_mul_mat_cases.py): the table is well-formed and restates the launchers' row rules, the reference is the
oracle's mat-mul, every case whose activation is computed sits away from the quantiser's rounding boundaries, and the producers' edge rows reach the ends of the
block sums' range."""
import numpy as np
import pytest

import iq4xs_ref
import np_twin as tw
import oracle_py as oq
import prompt_mul_mat_cases as pc
from prompt_mul_mat_cases import ADD, CASES, IQ4_XS, STORE, SWIGLU
from oracle_py import Q4_K, Q6_K, Q8_K


def planes_refuses(c) -> bool:
    """launch_mmq_planes_multi's row rules (mmq.hip mmq_planes_form) restated: a residual with several segments; a non-last segment that does not end on a
    32-row tile; the two plane formats in one launch unless every non-last segment ends on a 128-row tile and the 128 x 256 kernel takes the launch (here:
    forced by mmq_tiles 4 - without it a 40-token batch never does)."""
    n = len(c["types"])
    if n > 1 and c["epi"] == ADD:
        return True
    if any(N % 32 for N in c["Ns"][:-1]):
        return True
    mixed = len({t in pc.HAS_MINS for t in c["types"]}) > 1
    if mixed and (any(N % 128 for N in c["Ns"][:-1]) or not (c["tiles"] == 4 or (c["tiles"] == 0 and c["T"] > 128))):
        return True
    return False


def test_table_is_well_formed():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        n = len(c["types"])
        nm = c["name"]
        assert 1 <= n <= 3 and len(c["Ns"]) == n and 3 <= c["T"] <= 600 and c["K"] % 256 == 0, nm
        assert c["epi"] in (STORE, ADD, SWIGLU) and c["prologue"] in (0, 1, 2, 3) and c["form"] in (0, 1, 2, 3) and c["tiles"] in (0, 1, 2, 4), nm
        for t in c["types"]:
            assert t in pc.KQ or (t in pc.PLANES_ONLY and n == 1 and c["form"] in (pc.FORM_MODEL, pc.FORM_PLANES)), nm
        if c["refused"]:
            assert c["path"] is None, nm
            continue
        if c["epi"] == ADD:
            assert n == 1, nm
        if c["epi"] == SWIGLU:
            assert n == 2 and c["Ns"][0] == c["Ns"][1] and c["types"][0] == c["types"][1], nm
        p = c["path"]
        # every case has 3 pad columns; a K split with its reduction has n_rows % 4 == 0 and 4 (mmq_splitk_reduce_kernel moves four rows at a time)
        if p["n_split"] > 1:
            assert sum(c["Ns"]) % 4 == 0 and c["ld_pad"] == 4 and p["kernel"] == pc.KERNEL_LDS and c["split"] == p["n_split"] <= c["K"] // 256, nm
        else:
            assert c["ld_pad"] == 3, nm
        assert p["prep"] == (1 if c["prologue"] == 0 else 0) and p["swiglu"] == (1 if c["epi"] == SWIGLU else 0), nm
        # the path against the form and the options
        if c["form"] == pc.FORM_KSPLIT:
            assert p["kernel"] == pc.KERNEL_KSPLIT and c["T"] <= 256 and all(t in pc.KQ for t in c["types"]), nm
        if c["form"] == pc.FORM_FLY:
            assert p["kernel"] == pc.KERNEL_FLY and n == 1 and c["T"] >= 32 and c["tiles"] in (1, 2), nm
        if c["form"] == pc.FORM_PLANES:
            assert c["T"] >= 32 and not planes_refuses(c), nm
            want = {1: pc.KERNEL_PLANES_256X32, 2: pc.KERNEL_PLANES_128X128, 4: pc.KERNEL_LDS}[c["tiles"]]      # (no case leaves the tile form to the CU count)
            assert p["kernel"] == want, nm
            if c["tiles"] == 4 and c["epi"] != SWIGLU:
                assert c["split"] >= 1, nm                         # ... nor the split
        if p["kernel"] == pc.KERNEL_KSPLIT:
            assert p["token_tiles"] == (1 if c["T"] <= 32 else 2) and p["n_split"] == 1 and not p["mixed"], nm
        else:
            assert p["token_tiles"] == 0, nm
        if p["mixed"]:
            assert p["kernel"] == pc.KERNEL_LDS and len({t in pc.HAS_MINS for t in c["types"]}) == 2, nm
        elif c["form"] == pc.FORM_PLANES and c["epi"] != SWIGLU:
            assert len({t in pc.HAS_MINS for t in c["types"]}) == 1, nm
        if c["prologue"] in (1, 2):
            assert c["T"] * c["K"] <= 40 * 1024, nm               # few enough values for a seed to keep them all off a rounding boundary


def test_refusals_restate_the_launchers_rules():
    by = pc.BY_NAME
    for nm in ("refuse_two_segments_with_residual", "refuse_planes_segment_not_32_rows", "refuse_mixed_segment_not_128_rows", "refuse_mixed_without_lds_kernel_t40"):
        assert by[nm]["form"] == pc.FORM_PLANES and planes_refuses(by[nm]), nm
    c = by["refuse_swiglu_pair_unequal_types"]
    assert c["epi"] == SWIGLU and c["types"][0] != c["types"][1]
    c = by["refuse_model_gate_up_t40_swiglu_behind"]
    assert c["form"] == pc.FORM_MODEL and c["epi"] == SWIGLU and 32 < c["T"] <= 128
    assert len(pc.REFUSED_CASES) == 6 and len(pc.RUN_CASES) + 6 == len(CASES)


def test_the_table_covers_what_it_names():
    """Every launcher with a residual, both tile forms of the two kernels that have them, the split with its reduction, every producer before every family."""
    add = {(c["path"]["kernel"], c["path"]["n_split"] > 1) for c in pc.RUN_CASES if c["epi"] == ADD and c["form"] != pc.FORM_MODEL}
    assert add == {(1, False), (2, False), (3, False), (4, False), (4, True), (5, False)}
    assert {c["tiles"] for c in pc.RUN_CASES if c["form"] == pc.FORM_FLY and c["epi"] == ADD} == {1, 2}
    assert {c["types"][0] for c in pc.RUN_CASES if c["epi"] == ADD and c["form"] == pc.FORM_PLANES} == set(pc.KQ + pc.PLANES_ONLY)
    for pro in (1, 2, 3):
        assert {c["path"]["kernel"] for c in pc.RUN_CASES if c["prologue"] == pro} == {1, 2, 4, 5}, pro
    multi = [c for c in pc.RUN_CASES if len(c["types"]) > 1 and c["epi"] == STORE and c["form"] != pc.FORM_MODEL]
    assert {c["path"]["kernel"] for c in multi} == {1, 2, 3, 4} and any(c["path"]["mixed"] and c["path"]["n_split"] == 2 for c in multi)


@pytest.mark.parametrize("c", [c for c in pc.RUN_CASES if c["prologue"] in (1, 2)], ids=lambda c: c["name"])
def test_computed_activation_codes_are_stable(c):
    """The device's sum of squares, or its expf, may differ from the oracle's in the last place; the codes must not depend on it."""
    assert pc.codes_stable(c, pc.inputs(c)), f"{c['name']}: seed {c['seed']} puts a value on a rounding boundary - pick another in prompt_mul_mat_cases.SEEDS"


SIX = ["add_ksplit_q4k_k512_n37_t5", "add_planes1_iq4xs_k512_n300_t40", "mixed_lds_q6k_q5k_t140", "swiglu_ksplit_q6k_n37_t32", "pro_norm_planes1_q4k_k1024_n70_t40",
       "pro_swiglu_fly_q5k_k1024_n70_t40"]


@pytest.mark.parametrize("name", SIX)
def test_reference_is_vec_dot_per_row(name):
    """reference() against its own definition written out: the activation, quantised to Q8_K, one vec_dot per row, then the epilogue - on a few rows and tokens."""
    c = pc.BY_NAME[name]
    inp = pc.inputs(c)
    ref = pc.reference(c, inp)
    y = pc.activation(c, inp)
    K = c["K"]

    def dot(s, r, aq):
        t, N = c["types"][s], c["Ns"][s]
        W = inp["W"][s]
        rb = len(W) // N
        w_row = W[r * rb:(r + 1) * rb]
        return np.float32(iq4xs_ref.vec_dot(w_row, aq, K) if t == IQ4_XS else oq.vec_dot(t, w_row, aq, K))

    for j in (0, c["T"] // 2, c["T"] - 1):
        aq = oq.quantize(Q8_K, y[j])
        for s in range(1 if c["epi"] == SWIGLU else len(c["types"])):
            N = c["Ns"][s]
            for r in (0, 1, N // 2, N - 1):
                if c["epi"] == SWIGLU:
                    g, u = dot(0, r, aq), dot(1, r, aq)
                    want = np.float32(oq.silu(np.array([g], np.float32))[0] * u)
                elif c["epi"] == ADD:
                    want = np.float32(inp["resid"][j, r] + dot(0, r, aq))
                else:
                    want = dot(s, r, aq)
                assert ref[s][j, r] == want, (name, s, j, r)


@pytest.mark.parametrize("name", ["add_ksplit_q6k_k256_n5_t9", "add_planes1_q2k_k512_n300_t40", "add_planes1_iq4xs_k512_n300_t40", "multi_planes1_q4k_q5k_q4k_t40",
                                  "pro_norm_ksplit_q4k_k1024_n37_t9"])
def test_reference_is_a_mat_mul(name):
    """... and close to the product of the dequantised weights with the unquantised activation: the 8-bit activation's error, a few parts in a thousand."""
    c = pc.BY_NAME[name]
    inp = pc.inputs(c)
    ref = pc.reference(c, inp)
    y = pc.activation(c, inp).astype(np.float64)
    for s, (t, N) in enumerate(zip(c["types"], c["Ns"])):
        W = inp["W"][s]
        deq = (iq4xs_ref.dequantize(W, N * c["K"]) if t == IQ4_XS else oq.dequantize(t, W, N * c["K"])).astype(np.float64).reshape(N, c["K"])
        want = y @ deq.T
        if c["epi"] == ADD:
            want = want + inp["resid"][:, :N]
        assert np.abs(ref[s] - want).max() <= 2e-2 * np.abs(want).max(), (name, s)


def test_inputs_differ_in_scale_from_token_to_token():
    c = pc.BY_NAME["add_lds_q4k_k512_n130_t257"]
    x = pc.inputs(c)["x"]
    d = np.stack([oq.quantize(Q8_K, r).view(tw.DT[Q8_K])["d"] for r in x[:8]])
    assert len(np.unique(d[:, 0])) == 8


def test_bounds_are_the_projects():
    r = np.array([[3.0, -8.0]], np.float32)
    assert pc.bound(pc.BY_NAME["add_ksplit_q4k_k512_n37_t5"], r) == pytest.approx(2e-5 * 8.0 + 1e-6)
    assert pc.bound(pc.BY_NAME["swiglu_ksplit_q4k_n37_t5"], r) == pytest.approx(4e-5 * 8.0 + 1e-6)
    assert pc.SPLIT_BOUND == 2e-6


@pytest.mark.parametrize("producer", [0, 1, 2])
def test_producer_edge_rows_reach_the_ends_of_the_block_sums(producer):
    """The oracle's blocks of the edge rows: block sums 2032 (bh 31, bl 48), -2032 (bh -32, bl 16) and 0, the ends of what bsum = 64 * bh + bl must hold."""
    for T, n in ((7, 256), (40, 1024)):
        x, x2, nw, n_edge = pc.producer_inputs(producer, T, n)
        assert x.shape == (T, n) and n_edge == 4
        rows = pc.producer_reference(producer, x, x2, nw)
        for e in range(n_edge):
            b = oq.quantize(Q8_K, rows[T - n_edge + e]).view(tw.DT[Q8_K])
            bsum, bh, bl = pc.EDGE_SUMS[e]
            assert (b["bsums"][:, 1:] == bsum).all(), (producer, e, b["bsums"][0])
            assert bsum == 64 * bh + bl and bh == bsum >> 6 and 0 <= bl <= 63
    x, _, _, n_edge = pc.producer_inputs(0, 1, 256)
    assert x.shape == (1, 256) and n_edge == 0
