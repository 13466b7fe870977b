"""CPU checks behind tests/test_gpu_kv_store.py: its cases keep the properties the issue of that file asks for, and the oracle reference itself stays inside
the caps the GPU tests apply when its rotated rows move by as much as a device rope may differ - so a GPU failure there is the kernel's, not the cap's."""
import numpy as np
import pytest

import kv_store_cases as kc
import oracle_py as oq
from kv_store_cases import N_CELLS
from oracle_py import F16, Q4_0, Q8_0


def test_cases_cover_what_they_claim():
    cases = kc.rotated_cases()
    assert len({c.id for c in cases}) == len(cases)
    assert {(c.H, c.G, c.D) for c in cases if not c.fast} == set(kc.GENERIC_SHAPES)
    assert {(c.tk, c.tv) for c in cases if c.fast} == set(kc.FAST_PAIRS) and {(c.tk, c.tv) for c in cases if not c.fast} == set(kc.GENERIC_PAIRS)
    assert any(c.fast and c.G * c.D == 2048 for c in cases) and any(c.fast and c.n_rot < c.D and c.ff for c in cases)
    rng = np.random.default_rng(0)
    for T in kc.TS[1:]:
        cells = kc.scattered_cells(rng, T)
        assert len(set(cells.tolist())) == T and 0 in cells and N_CELLS - 1 in cells and cells.min() >= 0 and cells.max() < N_CELLS
        assert not (np.diff(cells) > 0).all()                       # scattered, not ascending
    d = kc.shift_deltas(rng)
    assert 0.5 < (d == 0).mean() < 0.8 and set(d[d != 0].tolist()) <= {-10, -32, 5, -4000}
    x = kc.crafted_rows(rng, 6, 3, 64, 0).reshape(6, 3, 2, 32)
    assert (x[:, 1] != 0).all()                                     # the middle head is left random
    assert any((x[t, g, b] == 0).all() for t in range(6) for g in (0, 2) for b in range(2))


@pytest.mark.parametrize("t", [F16, Q8_0, Q4_0], ids=lambda t: kc.TNAME[t])
def test_reference_stays_inside_the_rotated_row_caps(t):
    """The identical share of 99 % is a cap, not a measurement: the oracle's rotated K rows of every committed case, quantised as they are and moved up or down
    per element (seeded sign), must keep kc.REF_SHARE of their elements identical (the move overstates a device's difference several times, see below) and stay within the per-element bound.
    A case that did not with its first seed takes a later one (kc.SEED_BUMP).
    Moved by 4e-6 (test_rope's bound on a rotated unit-scale value): q8_0 and q4_0.  An f16 element below 0.004 has a spacing under 4e-6, and a fortieth of
    unit-normal values flips under that move whatever the seed (measured here: 0.977 identical), so for f16 the move is what a device rope may differ by: cos
    and sin within 4 ulp (the OpenCL-class bound of the device's single-precision library) through y = x0 c - x1 s, that is (|x0| + |x1|) * 4 * 2^-24."""
    shares = []
    for c in kc.rotated_cases():
        if c.tk != t:
            continue
        _, k, _, pos, _, _, _ = kc.rotated_inputs(c)
        rot = kc.rope_rows(c, k, c.G, pos)
        rng = np.random.default_rng(c.seed("perturb"))
        sign = rng.choice(np.array([-1.0, 1.0], np.float32), rot.shape)
        if t == F16:
            pair = np.abs(k).reshape(c.T, c.G, c.D)
            half = c.n_rot // 2
            mate = pair.copy()
            if c.neox:
                mate[..., :half], mate[..., half:c.n_rot] = pair[..., half:c.n_rot], pair[..., :half]
            else:
                mate[..., 0:c.n_rot:2], mate[..., 1:c.n_rot:2] = pair[..., 1:c.n_rot:2], pair[..., 0:c.n_rot:2]
            move = ((pair + mate) * (4 * 2.0 ** -24)).reshape(rot.shape).astype(np.float32)
        else:
            move = np.float32(kc.Q_TOL)
        worst, same, inside = kc.code_distance(t, rot, kc.quant_rows(t, rot), kc.quant_rows(t, rot + sign * move))
        assert inside or t == F16, (c.id, worst)   # (f16: a rotated value near 0 has a step below any move; the share is what is checked)
        shares.append((same, c.id))
    low = min(shares)
    print(f"{kc.TNAME[t]}: lowest identical share under the move {low[0]:.5f} ({low[1]}), over {len(shares)} cases")
    assert low[0] >= kc.REF_SHARE, low


@pytest.mark.parametrize("t", [F16, Q8_0, Q4_0], ids=lambda t: kc.TNAME[t])
def test_there_and_back_bound_holds_for_the_oracle(t):
    """The two-step bound of test_k_shift_there_and_back on the oracle's own chain, quantize(rope(dequantize(row), -8)) and back by +8, on that test's rows."""
    G, D = 2, 128
    n = G * D
    rng = np.random.default_rng(t)
    cache = kc.quant_rows(t, rng.standard_normal((N_CELLS, n)).astype(np.float32))
    a = kc.dequant_rows(t, cache, n)
    there = kc.quant_rows(t, np.stack([oq.rope(r, G, D, -8, kc.BASE).reshape(-1) for r in a]))
    b = kc.dequant_rows(t, kc.quant_rows(t, np.stack([oq.rope(r, G, D, 8, kc.BASE).reshape(-1) for r in kc.dequant_rows(t, there, n)])), n)
    step = np.hypot(a[:, 0::2], a[:, 1::2]).repeat(2, axis=1) * 2.0 ** -10 if t == F16 else kc.code_step(t, a)
    worst = float((np.abs(a - b) / np.maximum(step, 1e-30)).max())
    print(f"{kc.TNAME[t]}: worst {worst:.3g} steps")
    assert (np.abs(a - b) <= 2 * step + 1e-7).all(), worst
