"""Speculative decoding without a GPU: the numpy restatement of the two kernels' rules on hand-made rows, the round on the CPU oracle for every case of
spec_cases.py - with the three conditions that entitle the GPU tests to demand identical tokens - and the new C-ABI entries' answer on a machine with no device."""
import ctypes as C

import numpy as np
import pytest

import oracle_py as oq
import spec_cases as sc

ALL_CASES = sc.CASES + [sc.MOE_CASE]


def test_argmax_prob_rule_on_hand_made_rows():
    """A check of the REFERENCE (spec_cases.argmax_prob_ref), not of the kernel: it passes without the feature.  The kernel meets it in test_gpu_spec_ops.py."""
    inf, nan = np.inf, np.nan
    x = np.array([[1.0, 3.0, 3.0, 2.0], [nan, 2.0, nan, 2.0], [nan, nan, nan, nan], [-inf, -inf, -inf, -inf], [0.0, inf, 1.0, nan], [5.0, 5.0, 5.0, 5.0],
                  [-inf, 0.0, -inf, nan]], np.float32)
    idx, p = sc.argmax_prob_ref(x)
    assert idx.tolist() == [1, 1, 0, 0, 1, 0, 1]
    assert p[0] == pytest.approx(1.0 / (np.exp(-2.0) + 2.0 + np.exp(-1.0)))
    assert p[1] == pytest.approx(0.5) and p[5] == pytest.approx(0.25) and p[6] == pytest.approx(1.0)
    assert p[2] == 0.0 and p[3] == 0.0 and p[4] == 0.0


def test_spec_verify_rule_on_hand_made_rows():
    """A check of the REFERENCE (spec_cases.spec_verify_ref), not of the kernel: it passes without the feature.  The kernel meets it in test_gpu_spec_ops.py."""
    V = 8
    want = [3, 1, 4, 1, 5, 2, 6]                                        # the arg-max of rows 0 .. 6
    logits = np.zeros((7, V), np.float32)
    for r, t in enumerate(want):
        logits[r, t] = 1.0
    # group 0: rows 0 .. 2, drafts 3, 1 both right (its last entry equals the arg-max and must not count); group 1: row 3 alone (k = 0);
    # group 2: rows 4 .. 6, draft 0 wrong, draft 1 right again (must not count)
    ids, acc = sc.spec_verify_ref(logits, np.arange(7), [0, 3, 4, 7], [3, 1, 4, 1, 9, 2, 6])
    assert ids.tolist() == want and acc.tolist() == [2, 0, 0]


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_case_conditions_hold_on_the_oracle(pkg, tmp_path_factory, case):
    """(1) a round with every draft accepted, a partial one and one with none; (2) every top-2 gap of the target's logits along the emitted path beyond
    2 * FLIP_TOL of the row's scale; (3) no draft probability within P_MARGIN of p_min.  And the round emits the target's own greedy tokens."""
    d = tmp_path_factory.mktemp("spec")
    _, _, _, n_max, p_min = case
    T, D, prompt, first = sc.open_case(oq, pkg.gguf_synth, d, case, oq.Q8_0)
    toks, stats, tr = sc.speculative_round_loop(T, D, first, sc.N_PROMPT, sc.N_TOKENS, n_max, 0, p_min)
    acc = tr["accept"]
    assert any(k >= 1 and a == k for k, a in acc) and any(0 < a < k for k, a in acc) and any(k >= 1 and a == 0 for k, a in acc), acc
    assert min(tr["gap"]) > 2 * sc.FLIP_TOL, tr["gap"]
    assert all(abs(pr - p_min) > sc.P_MARGIN for pr in tr["p"]), (p_min, tr["p"])
    assert sc.trace_ok(tr, p_min)
    assert stats[0] == len(acc) and stats[1] == sum(k for k, _ in acc) and stats[0] + stats[2] == sc.N_TOKENS and stats[2] <= sum(a for _, a in acc) and stats[3] == sum(k == 0 for k, _ in acc)
    assert stats[1] > stats[2] > 0
    # the same tokens as plain greedy steps of the target on a fresh context
    T.rm(0)
    row = T.decode(prompt, np.arange(sc.N_PROMPT), False)[-1]
    plain = []
    for i in range(sc.N_TOKENS):
        t = sc.argmax_rule(row)
        if i == 0:
            assert t == first
        row = T.decode([t], [sc.N_PROMPT + i], False)[-1]
        plain.append(sc.argmax_rule(row))
    assert toks.tolist() == plain
    T.close(); D.close()


def test_new_entries_answer_without_a_device(pkg):
    """On a machine without a GPU every new entry answers MI355_ERR_NO_DEVICE (-100) or fails cleanly; with one, the argument checks answer."""
    lib = pkg.load_library()
    has_gpu = lib.mi355_device_count() > 0
    x = np.zeros((2, 8), np.float32); idx = np.zeros(2, np.int32); p = np.zeros(2, np.float32)
    rows = np.array([0, 1], np.int32); gs = np.array([0, 2], np.int32); draft = np.zeros(2, np.int32); acc = np.zeros(1, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    r1 = lib.mi355_op_argmax_prob_rows(vp(x), 8, 2, vp(idx), vp(p))
    r2 = lib.mi355_op_spec_verify(vp(x), 8, 2, vp(rows), 2, vp(gs), 1, vp(draft), vp(idx), vp(acc))
    pf = C.c_float(0.0)
    r3 = lib.mi355_get_argmax_prob_ith(None, 0, C.byref(pf))
    r4 = lib.mi355_spec_verify(None, 1, vp(gs), vp(draft), vp(idx), vp(acc))
    r5 = lib.mi355_speculative_steps(None, None, 0, 0, 0, 1, 4, 0, 0.5, None, None)
    if has_gpu:
        assert (r1, r2) == (0, 0) and r3 == r4 == r5 == -103
    else:
        assert r1 == r2 == r3 == r4 == r5 == -100
