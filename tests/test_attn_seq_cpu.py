"""CPU checks behind tests/test_gpu_attn_seq.py: every case of tests/attn_seq_cases.py holds what it is there for (a sub-tile of two sequences, an open chunk,
a chunk hidden from part of a tile by sequence alone, an invisible chunk; for a batched step empty (token, chunk) pairs, uneven chunk lists, a new cell at a
chunk's edge), tells the right visibility rule from three wrong ones by 100 x the GPU tolerance on a row the GPU test checks, and the oracle itself sits at
float64's distance.  Each test prints its counts (pytest -s)."""
import numpy as np
import pytest

import attn_seq_cases as ac
import oracle_py as oq
from oracle_py import F16, Q4_0, Q8_0

NEED = 100 * ac.TOL


def moved(ref: dict, wrong: dict) -> float:
    """Largest distance of a wrong reference from the right one over the rows, in units of max(1, |ref|.max())."""
    worst = 0.0
    for t, r in ref.items():
        w = wrong[t]
        worst = max(worst, float(np.abs(r - w).max()) / max(1.0, float(np.abs(r).max())))
    return worst


def test_every_query_sees_a_cell_and_the_tail_is_empty():
    n = 0
    for c in ac.prefill_cases() + ac.split_cases():
        cell_pos, cell_seq, q_pos, q_seq, *_ = ac.fa_inputs(c)
        assert c.n_kv % 32 != 0 and (cell_pos[c.n_kv:] == -1).all(), c.id
        assert q_seq.min() >= 0 and q_seq.max() <= 63
        for t in range(c.T):
            assert ac.visible(cell_pos, cell_seq, c.n_kv, q_pos, q_seq, t).size >= 1, (c.id, t)
            n += 1
    for c in ac.step_cases():
        inp = ac.step_inputs(c)
        assert c.n_kv % 32 != 0 and (inp[0][c.n_kv:] == -1).all(), c.id
        for t in range(c.T):
            assert ac.visible(inp[0], inp[1], c.n_kv, inp[2], inp[3], t).size >= 1, (c.id, t)
            n += 1
    print(f"{n} queries, each sees at least one cell")


def test_case_lists_cover_the_issue():
    pf, sp, st = ac.prefill_cases(), ac.split_cases(), ac.step_cases()
    for cases in (pf, sp, st):
        assert len({c.id for c in cases}) == len(cases)
    assert {(c.D, c.R, c.tk) for c in pf} == ({(64, R, t) for R in (1, 2, 4, 8) for t in (Q8_0, F16)} | {(128, R, t) for R in (3, 5, 6, 7) for t in (Q8_0, F16)} |
                                             {(128, R, Q4_0) for R in (1, 2, 8)} | {(128, R, Q8_0) for R in (1, 2, 4, 8)})
    assert all(c.G == 2 and c.T == ac.prefill_T(c.R) and c.T >= 32 for c in pf) and {c.n_cells for c in pf} == {70, 600}
    for R in (1, 4):
        assert {c.layout for c in pf if c.R == R and c.n_cells == 600} == set(ac.LAYOUTS)
    assert all({"interleaved", "shared"} <= {c.layout for c in pf if (c.D, c.R, c.tk, c.n_cells) == k} for k in {(c.D, c.R, c.tk, c.n_cells) for c in pf})
    s = [c for c in sp if c.kind == "split"]
    assert {(c.R, c.D, c.tk, c.tv) for c in s} >= {(R, D, tk, tv) for R in (2, 3, 5, 6, 7) for D in (64, 128)
                                                     for (tk, tv) in ((F16, F16), (Q8_0, Q8_0), (Q4_0, Q4_0), (Q8_0, F16), (F16, Q8_0))}
    assert {c.T for c in s} == {1, 5, 31} and {c.n_cells for c in s} == {33, 300, 2100} and {c.layout for c in s} >= {"interleaved", "shared", "shuffled"}
    for T in (1, 5, 31):
        assert {c.n_cells for c in s if c.T == T} >= {33, 300} and {c.layout for c in s if c.T == T} >= {"interleaved", "shared", "shuffled"}, T
    assert sum(c.kind == "parity" for c in sp) == 1
    assert {(c.D, c.R) for c in st} == {(128, R) for R in (1, 2, 4, 8, 3, 7)} | {(64, 1), (64, 4)}
    assert {c.T for c in st} == {2, 5, 64} and {c.n_cells for c in st} == {384, 4480} and {c.layout for c in st} == {"regions", "ragged", "interleaved"}
    assert {(c.tk, c.tv) for c in st} == {(F16, F16), (Q8_0, Q8_0), (Q8_0, F16), (F16, Q8_0), (Q4_0, Q4_0)} and {c.rope for c in st} == {"norm", "neox", "rot64"}
    for T in (2, 5, 64):
        assert {c.rope for c in st if c.T == T} >= {"norm", "neox"} and len({(c.tk, c.tv) for c in st if c.T == T}) >= 4, T
    print(f"{len(pf)} prompt-kernel cases, {len(s)} split-kernel cases, 1 parity case, {len(st)} batched-step cases")


def test_prefill_cases_hold_the_tile_structures():
    """All four in every case - except "interleaved": in a period-3 pattern every 32-cell chunk holds cells of all three sequences at the same positions, so
    no chunk can be open for a tile (its cells are not all in the tile's sequences) and none is hidden from a query by sequence as a whole.  What that
    layout holds instead is the same distinction INSIDE every chunk (a query's own cells next to others' at or below its position); it must show that, the
    two-sequence sub-tile and the invisible chunk."""
    tot = {"mixed_sub_tiles": 0, "open": 0, "partial_by_seq": 0, "invisible": 0, "mixed_chunks": 0}
    cases = ac.prefill_cases()
    for c in cases:
        st = ac.prefill_structure(c, ac.fa_inputs(c))
        assert st["mixed_sub_tiles"] >= 1 and st["invisible"] >= 1, (c.id, st)
        if c.layout == "interleaved":
            assert st["open"] == 0 and st["mixed_chunks"] >= 3, (c.id, st)
        else:
            assert st["open"] >= 1 and st["partial_by_seq"] >= 1, (c.id, st)
        for k in tot:
            tot[k] += st[k]
    print(f"{len(cases)} prompt-kernel cases: {tot}")


def test_step_cases_hold_the_list_structures():
    cases = ac.step_cases()
    tot = {"empty_pairs": 0, "edge_cells": 0, "lone_tokens": 0}
    for c in cases:
        st = ac.step_structure(c, ac.step_inputs(c))
        L = st["list_lengths"]
        assert st["empty_pairs"] >= 1 and len(set(L)) >= 2 and any(x % 4 for x in L) and st["edge_cells"] >= 1, (c.id, st)
        assert st["lone_tokens"] >= 1 or c.T == 2, (c.id, st)
        for k in tot:
            tot[k] += st[k]
    assert any(c.n_cells == 4480 and (c.n_kv + 63) // 64 > 64 for c in cases)
    print(f"{len(cases)} batched-step cases: {tot}")


@pytest.mark.parametrize("kind", ["prefill", "split"])
def test_wrong_visibility_rules_are_told_apart_fa(kind):
    """Each wrong rule moves a checked row by >= 100 x the tolerance.  A single query is its own sub-tile: the two sub-tile rules need T > 1."""
    cases = ac.prefill_cases() if kind == "prefill" else ac.split_cases()
    low = {m: (np.inf, "") for m in ac.MUTANTS}
    for c in cases:
        inp = ac.fa_inputs(c)
        rows = ac.checked_rows(c.T, inp[3])
        ref = ac.fa_reference(c, inp, rows)
        for m in ac.MUTANTS:
            if c.T == 1 and m != "noseq":
                continue
            d = moved(ref, ac.fa_reference(c, inp, rows, m))
            assert d >= NEED, (c.id, m, d)
            low[m] = min(low[m], (d, c.id))
    print(f"{kind}: {len(cases)} cases, smallest move per wrong rule: " + ", ".join(f"{m} {low[m][0]:.3g} ({low[m][1]})" for m in ac.MUTANTS))


def test_wrong_visibility_rules_are_told_apart_step():
    cases = ac.step_cases()
    low = {m: (np.inf, "") for m in ac.MUTANTS}
    for c in cases:
        inp = ac.step_inputs(c)
        qr, _, k_rows, v_rows = ac.step_new_rows(c, inp)
        kc, vc = inp[8].copy(), inp[9].copy()
        kc[inp[4]], vc[inp[4]] = k_rows, v_rows
        rows = ac.checked_rows(c.T, inp[3])
        ref = ac.step_reference(c, inp, qr, kc, vc, rows)
        for m in ac.MUTANTS:
            d = moved(ref, ac.step_reference(c, inp, qr, kc, vc, rows, m))
            assert d >= NEED, (c.id, m, d)
            low[m] = min(low[m], (d, c.id))
    print(f"step: {len(cases)} cases, smallest move per wrong rule: " + ", ".join(f"{m} {low[m][0]:.3g} ({low[m][1]})" for m in ac.MUTANTS))


@pytest.mark.parametrize("t,tol", [(F16, 3e-3), (Q8_0, 3e-5), (Q4_0, 3e-5)], ids=lambda v: ac.TNAME.get(v, "") if isinstance(v, int) else "")
def test_oracle_vs_float64_on_the_smallest_case(t, tol):
    """The reference of the smallest multi-sequence case of each cache type against float64 attention, at test_oracle_kat.py::test_flash_attn_vs_float64's bounds."""
    c = min((c for c in ac.prefill_cases() + ac.split_cases() if c.tk == t and c.tv == t and c.T > 1 and c.kind != "parity"), key=lambda c: (c.n_cells * c.T * c.H * c.D, c.id))
    inp = ac.fa_inputs(c)
    cell_pos, cell_seq, q_pos, q_seq, q, kc, vc = inp
    rows = ac.checked_rows(c.T, q_seq)
    ref = ac.fa_reference(c, inp, rows)
    worst = 0.0
    for r in rows:
        cells = ac.visible(cell_pos, cell_seq, c.n_kv, q_pos, q_seq, r)
        want = ac.float64_attention(q[r], c.H, c.G, c.D, t, kc, t, vc, cells, c.scale)
        worst = max(worst, float(np.abs(ref[r] - want).max()))
    print(f"{c.id}: oracle within {worst:.3g} of float64 over {len(rows)} rows")
    assert worst < tol, (c.id, worst)
