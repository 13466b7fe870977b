"""The mat-vec step cases without a GPU (tests/matvec_step_cases.py): the table is well-formed, the reference is the oracle's mat-vec, and every case whose
activation is normalised inside the launch sits away from the quantiser's rounding boundaries, so that the reference alone meets the re-association bound."""
import numpy as np
import pytest

import matvec_step_cases as mc
import oracle_py as oq
import tq_ref
from matvec_step_cases import ADD, CASES, STORE, SWIGLU


def test_table_is_well_formed():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        n = len(c["types"])
        assert 1 <= n <= 3 and len(c["Ns"]) == n and 1 <= c["T"] <= 17, c["name"]
        assert c["epi"] in (STORE, ADD, SWIGLU) and c["fuse"] in (0, 1, 2), c["name"]
        if c["epi"] == ADD:
            assert n == 1, c["name"]
        if c["epi"] == SWIGLU:
            assert n == 2 and c["Ns"][0] == c["Ns"][1] and c["types"][0] == c["types"][1], c["name"]
        if c["fuse"]:
            assert c["T"] == 1, c["name"]
        if c["host"]:
            assert n == 1 and c["T"] == 1 and c["epi"] == STORE, c["name"]
        if c["sel"]:
            assert 2 <= len(c["sel"]) <= 8 and c["T"] == 1 and all(0 <= e < c["n_expert"] for e in c["sel"]), c["name"]
        for t in c["types"]:
            assert c["K"] % (32 if t in mc.Q80_TYPES else 256) == 0, c["name"]
        # one launch per chunk of 16 / 8 / 4 / 2 / 1 tokens, and the pass count of a stream launch is the case's
        assert [p["T"] for p in c["path"]] == mc.tokens_split(c["T"]), c["name"]
        for p in c["path"]:
            if p["kernel"] == "stream":
                assert p["kb"] == mc.kb_of(c["K"]) and p["kb"] in (1, 2, 3, 4, 6, 7, 10), c["name"]
    for var, sub in mc.SWITCH_CASES.items():
        for nm in sub:
            assert nm in mc.BY_NAME, (var, nm)


def test_token_chunks():
    assert mc.tokens_split(3) == [2, 1] and mc.tokens_split(5) == [4, 1] and mc.tokens_split(9) == [8, 1] and mc.tokens_split(17) == [16, 1]
    assert mc.tokens_split(2) == [2] and mc.tokens_split(15) == [8, 4, 2, 1]


@pytest.mark.parametrize("c", [c for c in CASES if c["fuse"] == 1], ids=lambda c: c["name"])
def test_normalised_activation_codes_are_stable(c):
    """The device's sum of squares may differ from the oracle's in the last place (test_rms_norm_mul); the codes must not depend on it."""
    assert mc.codes_stable(c, mc.inputs(c)), f"{c['name']}: seed {c['seed']} puts a value on a rounding boundary - pick another in matvec_step_cases.SEEDS"


@pytest.mark.parametrize("name", ["qkv_k2048_q5k_q80_q80", "gate_up_k2048_q40", "ffn_down_k2048_n300_q4k", "moe_down_k4096_q4k_sel8", "tq_gate_up_k4096", "tok3_qkv_mixed"])
def test_reference_is_vec_dot_per_row(name):
    """reference() against its own definition written out: normalise, quantise to the vec_dot type, one vec_dot per row, then the epilogue - on a few rows."""
    c = mc.BY_NAME[name]
    inp = mc.inputs(c)
    ref = mc.reference(c, inp)
    y = mc.normed(c, inp)
    K = c["K"]
    rows = (0, 1, c["Ns"][0] // 2, c["Ns"][0] - 1)

    def dot(s, r, act_row, e=0):
        t, N = c["types"][s], c["Ns"][s]
        W = inp["W"][s]
        rb = len(W) // (c["n_expert"] * N)
        w_row = W[(e * N + r) * rb:(e * N + r + 1) * rb]
        aq = oq.quantize(mc.act_type(t), act_row)
        return np.float32(tq_ref.vec_dot(t, w_row, aq, K) if t in tq_ref.TYPES else oq.vec_dot(t, w_row, aq, K))

    R = len(c["sel"]) if c["sel"] else c["T"]
    for j in range(R):
        e = c["sel"][j] if c["sel"] else 0
        a = y[j if (not c["sel"] or c["fuse"] == 2) else 0]
        for r in rows:
            if c["epi"] == SWIGLU:
                g, u = dot(0, r, a, e), dot(1, r, a, e)
                want = np.float32(oq.silu(np.array([g], np.float32))[0] * u)
            elif c["epi"] == ADD:
                want = np.float32(inp["resid"][j, r] + dot(0, r, a, e))
            else:
                want = dot(0, r, a, e)
            assert ref[0][j, r] == want, (name, j, r)


@pytest.mark.parametrize("name", ["qkv_k1024_q4k_q4k_q6k", "ffn_down_k4096_n37_q6k", "base_k2080_q40_fuse1", "tq_qkv_k4096"])
def test_reference_is_a_mat_vec(name):
    """... and close to the product of the dequantised weights with the unquantised activation: the 8-bit activation's error, a few parts in a thousand."""
    c = mc.BY_NAME[name]
    inp = mc.inputs(c)
    ref = mc.reference(c, inp)
    y = mc.normed(c, inp).astype(np.float64)
    for s, (t, N) in enumerate(zip(c["types"], c["Ns"])):
        W = inp["W"][s]
        deq = (tq_ref.dequantize(t, W, N * c["K"]) if t in tq_ref.TYPES else oq.dequantize(t, W, N * c["K"])).astype(np.float64).reshape(N, c["K"])
        want = y @ deq.T
        if c["epi"] == ADD:
            want = want + inp["resid"][:, :N]
        assert np.abs(ref[s] - want).max() <= 2e-2 * np.abs(want).max(), (name, s)


def test_bound_is_the_reassociation_bound():
    r = np.array([[3.0, -8.0]], np.float32)
    assert mc.bound(r) == pytest.approx(2e-5 * 8.0 + 1e-6)

