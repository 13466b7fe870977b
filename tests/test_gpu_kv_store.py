"""The kernels that write the K / V cache and the K-shift that re-rotates it, op by op through mi355_op_kv_store / mi355_op_k_shift against the CPU oracle
chained in the op's own order (oq.rope per token, then oq.quantize of the row; qwen3: the per-head RMSNorm first).  The whole cache crosses the boundary, in
and out: it is pre-filled with seeded bytes, the tokens go to scattered cells that include the first and the last one of an odd number of cells (97), and every
cell that was not written must come back byte for byte.

Forms of mi355_op_kv_store: 0 rope_kv_store_kernel computing its angles, 1 the same on the cos / sin table, 2 rope_q_kv_store_fast_kernel, 3
kv_store_fast_kernel.  Quantiser results are compared bit-exactly wherever no device cosf / sinf precedes them; rotated rows within the caps of
tests/test_gpu_ops.py::test_attn_step_decode_block (see kv_store_cases.py; tests/test_kv_store_cpu.py checks on the CPU that the reference itself stays inside
them when its rotated rows move by the device's rope error).  Each case prints its worst figures (pytest -s shows them)."""
import numpy as np
import pytest

import kv_store_cases as kc
import oracle_py as oq
from kv_store_cases import N_CELLS, BASE, Case
from oracle_py import F16, Q4_0, Q8_0

pytestmark = pytest.mark.gpu

ERR_ARG = "(-103)"


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def store(be, form, c: Case, q, k, v, kc0, vc0, pos, cells, **kw):
    return be.kv_store(form, None if form == 3 and q is None else q, k, v, c.H, c.G, c.D, c.tk, kc0, c.tv, vc0, pos, cells, BASE, n_rot=c.n_rot, neox=c.neox,
                       freq_scale=c.fs, freq_factors=c.freq_factors(), **kw)


def assert_other_cells_untouched(before, after, cells, what):
    rest = np.setdiff1d(np.arange(N_CELLS), cells)
    assert (after[rest] == before[rest]).all(), f"{what}: a cell outside tok_cell changed"


def assert_forms_agree(c: Case, outs):
    """2c: form 1 = form 0 (the same rope_angle) in q and both caches; forms 2 and 3 = form 1 (form 3: the caches only)."""
    q1, k1, v1 = outs[1]
    for form, (qf, kf, vf) in outs.items():
        assert (kf == k1).all(), f"K cache of form {form} differs from form 1"
        assert (vf == v1).all(), f"V cache of form {form} differs from form 1"
        if form != 3:
            assert (qf.view(np.uint32) == q1.view(np.uint32)).all(), f"q of form {form} differs from form 1"


@pytest.mark.parametrize("c", kc.quantiser_cases(), ids=lambda c: c.id)
def test_kv_store_quantisers_bit_exact(be, c):
    """2a.  V has no arithmetic before its quantisation, and K at position 0 is rotated by cos = 1, sin = 0 - exact, up to the sign of a zero, which the oracle's
    rope at position 0 produces by the same two multiplies and one add: V rows at any position and K rows at position 0 equal the oracle's bytes, for every
    form and cache type pair.  Crafted blocks in the first and the last kv head: all zero (d = 0), q8_0 rounding ties under d = 1, q4_0 +m / -m in both orders
    (the first one sets d, +8 clamps to 15), f16 ties, overflow to inf, underflow to 0 and -0.0; block scales 0.01 .. 30 elsewhere.  No tolerance."""
    rng = np.random.default_rng(c.seed("quant"))
    q = rng.standard_normal((c.T, c.H * c.D)).astype(np.float32)
    k = kc.crafted_rows(rng, c.T, c.G, c.D, 0)
    v = kc.crafted_rows(rng, c.T, c.G, c.D, 3)
    pos = np.array([0 if t % 2 == 0 else kc.ROT_POS[t % len(kc.ROT_POS)] for t in range(c.T)], np.int32)
    cells = kc.scattered_cells(rng, c.T, first=0)
    kc0, vc0 = kc.byte_pattern(rng, c.tk, c.G * c.D), kc.byte_pattern(rng, c.tv, c.G * c.D)
    k_ref = kc.quant_rows(c.tk, kc.rope_rows(c, k, c.G, pos))
    v_ref = kc.quant_rows(c.tv, v)
    at0 = pos == 0
    assert (kc.rope_rows(c, k[at0], c.G, pos[at0]) == k[at0]).all()          # (the rotation at position 0 changes no value)
    outs = {}
    for form in c.forms:
        outs[form] = qf, kf, vf = store(be, form, c, None if form == 3 else q, k, v, kc0, vc0, pos, cells)
        assert_other_cells_untouched(kc0, kf, cells, f"K, form {form}")
        assert_other_cells_untouched(vc0, vf, cells, f"V, form {form}")
        bad_v = np.nonzero((vf[cells] != v_ref).any(axis=1))[0]
        assert bad_v.size == 0, f"form {form}: V rows of tokens {bad_v.tolist()} differ from oq.quantize"
        bad_k = np.nonzero((kf[cells[at0]] != k_ref[at0]).any(axis=1))[0]
        assert bad_k.size == 0, f"form {form}: K rows at position 0 (tokens {np.nonzero(at0)[0][bad_k].tolist()}) differ from oq.quantize"
        if form != 3:
            assert (qf[at0].view(np.uint32) == q[at0].view(np.uint32)).all(), f"form {form}: q at position 0 changed"
    assert_forms_agree(c, outs)


@pytest.mark.parametrize("c", kc.rotated_cases(), ids=lambda c: c.id)
def test_kv_store_rotated_rows_match_oracle(be, c):
    """2b + 2c.  Positions 1, 17, 4095, 100000 (17 twice per five tokens), unit-scale inputs: q within test_rope's 4e-6 of oq.rope; the K codes within one step
    of oq.quantize(oq.rope(k)) per element (q8_0 amax / 127, q4_0 |max| / 8, f16 |x| 2^-10; x 1.01 + 1e-7) with at least 99 % of the dequantised elements
    identical, both over the whole case - the caps of test_attn_step_decode_block; V bit-exact; all forms byte for byte the same.
    Observed on the MI355X over the 324 cases: q off by at most 4.8e-7 (12 % of the cap); identical elements at least 0.99922 (f16), 0.99999 (q8_0), all
    (q4_0); largest difference 1.0 step (q8_0), none (q4_0).  An f16 element that rotates to nearly 0 differs by up to 12.9 of its own tiny steps: it is inside
    the bound through the absolute 1e-7 alone, which covers the device's cos / sin error only for inputs of unit scale."""
    q, k, v, pos, cells, kc0, vc0 = kc.rotated_inputs(c)
    q_ref = kc.rope_rows(c, q, c.H, pos)
    k_rot = kc.rope_rows(c, k, c.G, pos)
    k_ref = kc.quant_rows(c.tk, k_rot)
    v_ref = kc.quant_rows(c.tv, v)
    outs = {form: store(be, form, c, None if form == 3 else q, k, v, kc0, vc0, pos, cells) for form in c.forms}
    q1, k1, v1 = outs[1]
    for form, (_, kf, vf) in outs.items():
        assert_other_cells_untouched(kc0, kf, cells, f"K, form {form}")
        assert_other_cells_untouched(vc0, vf, cells, f"V, form {form}")
    assert (v1[cells] == v_ref).all()
    q_err = float(np.abs(q1 - q_ref).max())
    worst, same, inside = kc.code_distance(c.tk, k_rot, k_ref, k1[cells])
    print(f"kv_store {c.id}: q err {q_err:.3g} (cap {kc.Q_TOL:g}); K worst {worst:.3g} steps, identical {same:.5f} (cap {kc.SAME_SHARE})")
    assert q_err <= kc.Q_TOL, q_err
    assert inside, worst
    assert same >= kc.SAME_SHARE, same
    assert_forms_agree(c, outs)


@pytest.mark.parametrize("tk,tv", kc.GENERIC_PAIRS, ids=lambda t: kc.TNAME[t])
@pytest.mark.parametrize("H,G,D,T", [(8, 2, 128, 5), (32, 8, 128, 70), (6, 3, 64, 70), (4, 4, 64, 1)])
def test_kv_store_qwen3_head_norm(be, H, G, D, T, tk, tv):
    """qwen3 heads through the generic kernel (forms 0 and 1): every query head and kv head RMS-normalised over its own D values and multiplied by q_norm /
    k_norm before the NEOX rotation, several tokens per launch, D = 64 and 128.  Caps for the normalised and rotated rows as
    tests/test_gpu_qwen3.py::test_attn_decode_qk_norm: K within 1.01 steps + 1e-6, 99 % identical.  That test judges q through its attention output, which is
    not part of this op; here q is held to 1e-6 of the largest normalised value: the norm's scale factor within 4.5e-7 (seven f32 roundings of the butterfly
    sum of squares at half weight, a division and a square root, against the oracle's double sum), cos and sin within 4 ulp on |x0| + |x1| <= 2 max, 4.8e-7 -
    test_rope's 4e-6 is the same 0.9e-6 of its largest input.
    Observed on the MI355X: q off by at most 1.9e-6 (26 % of its cap); K at most 0.95 steps off, at least 0.99996 of the elements identical."""
    c = Case(H, G, D, T, tk, tv, D, neox=True)
    eps = 1e-6
    rng = np.random.default_rng(c.seed("qwen3"))
    q = (rng.standard_normal((T, H, D)) * rng.uniform(0.3, 6.0, (T, H, 1))).astype(np.float32).reshape(T, -1)    # a scale of its own per head
    k = (rng.standard_normal((T, G, D)) * rng.uniform(0.3, 6.0, (T, G, 1))).astype(np.float32).reshape(T, -1)
    v = (rng.standard_normal((T, G * D)) * 1.7).astype(np.float32)
    qn, kn = rng.uniform(0.25, 2.0, D).astype(np.float32), rng.uniform(0.25, 2.0, D).astype(np.float32)
    pos = np.array([kc.ROT_POS[t % len(kc.ROT_POS)] for t in range(T)], np.int32)
    cells = kc.scattered_cells(rng, T, first=N_CELLS - 1)
    kc0, vc0 = kc.byte_pattern(rng, tk, G * D), kc.byte_pattern(rng, tv, G * D)
    qq = np.stack([kc.head_norm(r, H, D, qn, eps) for r in q])
    kk = np.stack([kc.head_norm(r, G, D, kn, eps) for r in k])
    q_ref, k_rot = kc.rope_rows(c, qq, H, pos), kc.rope_rows(c, kk, G, pos)
    k_ref, v_ref = kc.quant_rows(tk, k_rot), kc.quant_rows(tv, v)
    outs = {form: store(be, form, c, q, k, v, kc0, vc0, pos, cells, q_norm=qn, k_norm=kn, eps=eps) for form in (0, 1)}
    q1, k1, v1 = outs[1]
    for form, (_, kf, vf) in outs.items():
        assert_other_cells_untouched(kc0, kf, cells, f"K, form {form}")
        assert_other_cells_untouched(vc0, vf, cells, f"V, form {form}")
    assert (v1[cells] == v_ref).all()
    n = G * D
    a, b = kc.dequant_rows(tk, k_ref, n), kc.dequant_rows(tk, k1[cells], n)
    step = kc.code_step(tk, k_rot)
    diff = np.abs(a - b)
    q_err = float(np.abs(q1 - q_ref).max())
    q_cap = 1e-6 * float(np.abs(q_ref).max())
    print(f"kv_store qwen3 {c.id}: q err {q_err:.3g} (cap {q_cap:.3g}); K worst {float((diff / np.maximum(step, 1e-30)).max()):.3g} steps, "
          f"identical {float((a == b).mean()):.5f}")
    assert (diff <= 1.01 * step + 1e-6).all(), float(diff.max())
    assert (a == b).mean() >= 0.99
    assert q_err <= q_cap, (q_err, q_cap)
    assert_forms_agree(c, outs)
    # the weights are not ignored: without them the K rows differ
    plain = store(be, 1, c, q, k, v, kc0, vc0, pos, cells)
    assert (plain[1][cells] != k1[cells]).any()


@pytest.mark.parametrize("form", [2, 3])
def test_kv_store_fast_forms_refuse_what_they_cannot_run(be, pkg, form):
    """2d.  The vectorised stores have no kernel for a q4_0 cache, NEOX pairing, a q / k norm or a kv width that is no multiple of 1024 (form 2: nor for such a
    q width): MI355_ERR_ARG with a message, and nothing is launched; the generic kernel takes the same arguments."""
    rng = np.random.default_rng(form)
    T = 3
    pos, cells = np.array([1, 17, 17], np.int32), np.array([0, N_CELLS - 1, 40], np.int32)
    w = np.ones(128, np.float32)
    refused = [(Case(8, 8, 128, T, Q4_0, Q4_0, 128), {}), (Case(8, 8, 128, T, Q8_0, Q4_0, 128), {}), (Case(8, 8, 128, T, F16, F16, 128, neox=True), {}),
               (Case(8, 8, 128, T, Q8_0, Q8_0, 128), {"q_norm": w, "k_norm": w, "eps": 1e-6}), (Case(8, 8, 128, T, Q8_0, Q8_0, 128), {"k_norm": w, "eps": 1e-6}),
               (Case(8, 6, 128, T, Q8_0, Q8_0, 128), {}), (Case(8, 3, 64, T, F16, F16, 64), {})]
    if form == 2:
        refused.append((Case(6, 8, 128, T, Q8_0, Q8_0, 128), {}))             # H * D = 768
    for c, kw in refused:
        q = rng.standard_normal((T, c.H * c.D)).astype(np.float32)
        k = rng.standard_normal((T, c.G * c.D)).astype(np.float32)
        kc0, vc0 = kc.byte_pattern(rng, c.tk, c.G * c.D), kc.byte_pattern(rng, c.tv, c.G * c.D)
        with pytest.raises(pkg.MI355Error) as ei:
            store(be, form, c, q, k, k, kc0, vc0, pos, cells, **kw)
        assert ERR_ARG in str(ei.value) and "no form for these arguments" in str(ei.value), (c.id, kw.keys(), str(ei.value))
        store(be, 1, c, q, k, k, kc0, vc0, pos, cells, **kw)                   # the generic kernel runs them
    if form == 3:                                                             # ... and a q width form 2 refuses is none of form 3's business
        c = Case(6, 8, 128, T, Q8_0, Q8_0, 128)
        k = rng.standard_normal((T, c.G * c.D)).astype(np.float32)
        store(be, 3, c, None, k, k, kc.byte_pattern(rng, Q8_0, 1024), kc.byte_pattern(rng, Q8_0, 1024), pos, cells)


# ------------------------------------------------------------------------------------------------ K-shift
def shift_cache(rng, t, G, D):
    """A cache of unit-scale rows: the caps of 2b are those of unit-scale inputs (an f16 element that rotates to nearly 0 differs by the device's cos / sin
    error times its partner, which 1e-7 covers only while the partner is of order 1)."""
    return kc.quant_rows(t, rng.standard_normal((N_CELLS, G * D)).astype(np.float32))


def check_shift(be, t, G, D, n_rot, neox, ff=None, fs=1.0, yarn=None, salt="shift"):
    c = Case(G, G, D, N_CELLS, t, F16, n_rot, neox=neox, ff=ff is not None, fs=fs)
    rng = np.random.default_rng(c.seed(salt))
    cache = shift_cache(rng, t, G, D)
    delta = kc.shift_deltas(rng)
    # the rows that stay hold the seeded byte pattern, not quantiser output: a valid row is a fixed point of dequantise - rotate by 0 - quantise in all three
    # formats, and would come back byte-identical even from a kernel that rewrote it
    cache[delta == 0] = kc.byte_pattern(rng, t, G * D)[delta == 0]
    moved = np.nonzero(delta)[0].astype(np.int32)
    ykw = {} if yarn is None else dict(ext_factor=yarn[0], attn_factor=yarn[1], corr_lo=yarn[2], corr_hi=yarn[3])
    got = be.k_shift(t, G, D, cache, delta, BASE, n_rot=n_rot, neox=neox, freq_scale=fs, freq_factors=ff, **ykw)
    assert (got[delta == 0] == cache[delta == 0]).all(), "a row with delta 0 changed"
    n = G * D
    deq = kc.dequant_rows(t, cache[moved], n)
    if yarn is None:
        rot = np.stack([oq.rope(deq[i], G, D, int(delta[cl]), BASE, neox=neox, n_rot=n_rot, freq_scale=fs, freq_factors=ff).reshape(-1) for i, cl in enumerate(moved)])
    else:
        rot = np.stack([oq.rope_yarn(deq[i], G, D, int(delta[cl]), BASE, fs, *yarn, neox=neox, n_rot=n_rot).reshape(-1) for i, cl in enumerate(moved)])
    worst, same, inside = kc.code_distance(t, rot, kc.quant_rows(t, rot), got[moved])
    print(f"k_shift {c.id}{' yarn' if yarn else ''}: {moved.size} rows moved; worst {worst:.3g} steps, identical {same:.5f} (cap {kc.SAME_SHARE})")
    assert inside, worst
    assert same >= kc.SAME_SHARE, same
    if yarn is None:
        # the same angle recurrence, the same single f32 multiply to dequantise and the same store_row as the generic store computing its angles: byte for byte
        # what mi355_op_kv_store form 0 writes for the dequantised rows at tok_pos = delta, tok_cell = cell (that entry point takes no YaRN parameters)
        vdummy = np.zeros((N_CELLS, 2 * n), np.uint8)
        _, via_store, _ = be.kv_store(0, deq, deq, deq, G, G, D, t, cache, F16, vdummy, delta[moved], moved, BASE, n_rot=n_rot, neox=neox, freq_scale=fs, freq_factors=ff)
        assert (got == via_store).all(), "k_shift differs from rope_kv_store on the dequantised rows"
    return cache, delta, got


@pytest.mark.parametrize("n_rot_div", [1, 2], ids=["rot-all", "rot-half"])
@pytest.mark.parametrize("neox", [False, True], ids=["norm", "neox"])
@pytest.mark.parametrize("G,D", [(2, 128), (3, 64), (8, 128)])
@pytest.mark.parametrize("t", [F16, Q8_0, Q4_0], ids=lambda t: kc.TNAME[t])
def test_k_shift(be, t, G, D, neox, n_rot_div):
    """3.  97 cells, two thirds of them with delta 0 (byte-identical afterwards), the rest moved by -10, -32, +5 or -4000: against
    oq.quantize(oq.rope(oq.dequantize(row), pos = delta)) within the caps of 2b, and byte for byte against the generic store on the dequantised rows."""
    check_shift(be, t, G, D, D // n_rot_div, neox)


@pytest.mark.parametrize("t", [F16, Q8_0, Q4_0], ids=lambda t: kc.TNAME[t])
def test_k_shift_scaled_rope(be, t):
    """freq_factors, a linear freq_scale of 0.25, and YaRN (parameters as tests/test_gpu_ops.py::test_rope_yarn)."""
    check_shift(be, t, 3, 64, 64, False, ff=np.linspace(1.0, 8.0, 32).astype(np.float32))
    check_shift(be, t, 2, 128, 128, True, fs=0.25)
    lo, hi = oq.yarn_corr_dims(128, 256, BASE)
    check_shift(be, t, 2, 128, 128, False, fs=0.25, yarn=(1.0, 0.8, lo, hi))


@pytest.mark.parametrize("t", [F16, Q8_0, Q4_0], ids=lambda t: kc.TNAME[t])
def test_k_shift_there_and_back(be, t):
    """Delta -8, then +8 on the result: back at the start within two steps per element - a sign error in the rotation, which a likewise mistaken reference
    could hide in a single shift, turns by 16 positions instead and misses by the size of the values.  Steps of the ORIGINAL rows: q8_0 amax / 127 and q4_0
    |max| / 8 of the block; f16 2^-10 of the rope pair's length (both roundings are relative to a rotated value, which is as large as the pair, not as the
    element).  Each requantisation is off by half a step of a block whose maximum the rotation may have raised by sqrt 2 (q4_0: a whole step where +8
    clamps to 15), the first one is rotated back; the oracle's own chain on these rows reaches 0.86 (f16), 1.17 (q8_0) and 1.49 (q4_0) steps
    (tests/test_kv_store_cpu.py)."""
    G, D = 2, 128
    n = G * D
    rng = np.random.default_rng(t)
    cache = shift_cache(rng, t, G, D)
    delta = np.full(N_CELLS, -8, np.int32)
    delta[::3] = 0
    cache[delta == 0] = kc.byte_pattern(rng, t, n)[delta == 0]
    there = be.k_shift(t, G, D, cache, delta, BASE)
    back = be.k_shift(t, G, D, there, -delta, BASE)
    assert (back[delta == 0] == cache[delta == 0]).all()
    moved = delta != 0
    assert (there[moved] != cache[moved]).any(axis=1).all()
    a, b = kc.dequant_rows(t, cache[moved], n), kc.dequant_rows(t, back[moved], n)
    if t == F16:
        step = np.hypot(a[:, 0::2], a[:, 1::2]).repeat(2, axis=1) * 2.0 ** -10
    else:
        step = kc.code_step(t, a)
    worst = float((np.abs(a - b) / np.maximum(step, 1e-30)).max())
    print(f"k_shift -8 then +8, {kc.TNAME[t]}: worst {worst:.3g} steps (cap 2)")
    assert (np.abs(a - b) <= 2 * step + 1e-7).all(), worst
