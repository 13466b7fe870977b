"""The LLaVA image encoder's launches one at a time (mi355_op_clip_attn, mi355_op_mul_mat_f16_xh, mi355_op_layer_norm, mi355_op_clip_gelu, ... -
include/mi355_llama.h) against the float64 references of tests/clip_ops_ref.py, within bounds computed per element from the references' own magnitudes, on the
case lists of tests/clip_ops_cases.py (tests/test_clip_ops_cpu.py shows without a GPU that these lists and bounds see a dropped key, a key chunk of 63, a shifted
bias, a residual read at the wrong stride, a one-pass variance and wrong GELU constants).  Kernel variants that state the same order of operations are held
against each other bit for bit; the small kernels are exact.

MI355_TEST_RECORD_FLIPS=<file>: every case's worst error as a share of its bound, and the share of GELU table entries that differ from numpy's f32 recipe (not
asserted on: the device's tanhf and expf are not numpy's)."""
import os

import numpy as np
import pytest

import clip_ops_cases as cs
import clip_ops_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def record(line: str) -> None:
    if os.environ.get("MI355_TEST_RECORD_FLIPS"):
        with open(os.environ["MI355_TEST_RECORD_FLIPS"], "a") as f:
            f.write(line + "\n")


def share(got, ref, bound) -> float:
    """the largest |got - ref| as a share of its bound (0 where the difference is 0)"""
    d = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(d == 0, 0.0, d / bound).max())


def bits(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b) -> bool:
    return np.array_equal(bits(a), bits(b))


def set_switches(monkeypatch, names, values) -> None:
    for n in names:
        monkeypatch.delenv(n, raising=False)
    for n, v in values.items():
        monkeypatch.setenv(n, v)                                  # (the launchers read them at every launch)


# ---------------------------------------------------------------- attention
_attn_runs = {}


def run_attn(be, monkeypatch, D, sw, T, H=cs.ATTN_H, n_img=1):
    """(out, out_h, path) of the shared inputs of (T, H, D, n_img) under a switch; one launch per key, shared between the tests"""
    key = (D, sw, T, H, n_img)
    if key not in _attn_runs:
        set_switches(monkeypatch, cs.SWITCH_VARS, cs.SWITCHES[sw])
        _attn_runs[key] = be.clip_attn(*cs.attn_inputs(T, H, D, n_img), T, H, D, n_img)
    return _attn_runs[key]


@pytest.mark.parametrize("D,sw,T,path", cs.PARITY_CASES, ids=lambda v: str(v))
def test_attention_matches_float64(be, monkeypatch, D, sw, T, path):
    out, out_h, got_path = run_attn(be, monkeypatch, D, sw, T)
    assert got_path == path                                       # the kernel the case names ran, not one it fell through to
    ref, bound = cs.attn_case_ref(T, cs.ATTN_H, D)
    s = share(out, ref, bound)
    record(f"clip_attn D={D} {sw} T={T} path={got_path}: worst error / bound {s:.3g}")
    assert s <= 1.0, s
    assert same_bits(out_h, out.astype(np.float16))


@pytest.mark.parametrize("D,sw,T,path", cs.ATTN_EDGES, ids=lambda v: str(v))
def test_attention_dispatch_edges_by_lds(be, monkeypatch, D, sw, T, path):
    """the largest T a kernel's LDS takes, and one past it: the named kernel runs, and is right there"""
    out, out_h, got_path = run_attn(be, monkeypatch, D, sw, T, H=1)
    assert got_path == path
    ref, bound = cs.attn_case_ref(T, 1, D)
    s = share(out, ref, bound)
    record(f"clip_attn edge D={D} {sw} T={T} path={got_path}: worst error / bound {s:.3g}")
    assert s <= 1.0, s
    assert same_bits(out_h, out.astype(np.float16))


@pytest.mark.parametrize("D,sw,T", cs.ATTN_REFUSALS, ids=lambda v: str(v))
def test_attention_refusals(be, monkeypatch, D, sw, T):
    """a head size without a kernel, a row count past the one-wave kernel's LDS: a non-zero return before anything is launched"""
    set_switches(monkeypatch, cs.SWITCH_VARS, cs.SWITCHES[sw])
    z = np.zeros((T, D), np.float32)
    rc, _, _, path = be.clip_attn_rc(z, z, z, T, 1, D)
    assert rc != 0 and path == cs.REFUSED


@pytest.mark.parametrize("D,sw,path", cs.NEEDLE_CASES, ids=lambda v: str(v))
def test_attention_needle_rows(be, monkeypatch, D, sw, path):
    """A query whose score at one key is 36 above the rest gets that key's V row - for every key and every query row on either side of a tile edge of any of
    the kernels: no edge drops, repeats or misplaces a row, however generous the bound."""
    set_switches(monkeypatch, cs.SWITCH_VARS, cs.SWITCHES[sw])
    q, k, v = cs.needle_inputs(D)
    T, H = cs.NEEDLE_T, cs.ATTN_H
    out, out_h, got_path = be.clip_attn(q, k, v, T, H, D)
    assert got_path == path
    ref, bound = R.attn_ref(q, k, v, T, H, D)
    for h in range(H):
        for qi, kj in cs.needle_pairs(h):
            sl = slice(h * D, (h + 1) * D)
            d = np.abs(out[qi, sl].astype(np.float64) - v[kj, sl])
            assert (d <= bound[qi, sl] + 1e-9).all(), (h, qi, kj, float(d.max()), float(bound[qi, sl].min()))
    assert share(out, ref, bound) <= 1.0
    assert same_bits(out_h, out.astype(np.float16))


@pytest.mark.parametrize("D", [32, 64, 128])
def test_attention_tiled_equals_one_wave_bit_for_bit(be, monkeypatch, D):
    """the LDS-tiled kernel states the sums of the one-wave kernel in the same order: the same bits at every T of the list"""
    tiled = "no-mfma" if D == 64 else "default"
    for T in cs.ATTN_TS:
        a, ah, pa = run_attn(be, monkeypatch, D, tiled, T)
        b, bh, pb = run_attn(be, monkeypatch, D, "one-wave", T)
        assert (pa, pb) == (cs.TILED, cs.WAVE)
        assert same_bits(a, b) and same_bits(ah, bh), (D, T, float(np.abs(a - b).max()))


@pytest.mark.parametrize("D,sw,T,path", cs.BATCH_CASES, ids=lambda v: str(v))
def test_attention_images_do_not_mix(be, monkeypatch, D, sw, T, path):
    """three different images in one launch: each the bits of the same image run alone"""
    q, k, v = cs.attn_inputs(T, cs.ATTN_H, D, 3)
    out, out_h, got_path = run_attn(be, monkeypatch, D, sw, T, n_img=3)
    assert got_path == path
    ref, bound = cs.attn_case_ref(T, cs.ATTN_H, D, 3)
    assert share(out, ref, bound) <= 1.0
    assert same_bits(out_h, out.astype(np.float16))
    set_switches(monkeypatch, cs.SWITCH_VARS, cs.SWITCHES[sw])
    for i in range(3):
        rows = slice(i * T, (i + 1) * T)
        alone, alone_h, p1 = be.clip_attn(q[rows], k[rows], v[rows], T, cs.ATTN_H, D)
        assert p1 == path and same_bits(alone, out[rows]) and same_bits(alone_h, out_h[rows]), (i, float(np.abs(alone - out[rows]).max()))


# ---------------------------------------------------------------- f16 GEMM with its epilogue
def run_gemm(be, monkeypatch, case, kernel, form=0):
    N, T, K, bias, scale, resid, ld_pad, in_place = case
    W, x, b, sc, r, ld = cs.gemm_inputs(case)
    set_switches(monkeypatch, cs.GEMM_VARS, cs.GEMM_KERNELS[kernel])
    return be.mul_mat_f16_xh(W, x, ld_out=ld, bias=b, scale=sc, resid=r, in_place=bool(in_place), form=form, y_init=np.full((T, ld), cs.POISON, np.float32))


@pytest.mark.parametrize("case", cs.GEMM_CASES, ids=lambda c: "N{}-T{}-K{}-b{}s{}r{}-pad{}-inplace{}".format(*c))
def test_f16_gemm_matches_float64(be, monkeypatch, case):
    N, T, K, bias, scale, resid, ld_pad, in_place = case
    ref, bound = R.gemm_ref(*cs.gemm_inputs(case))
    ys = {kern: run_gemm(be, monkeypatch, case, kern) for kern in cs.GEMM_KERNELS}
    y = ys["lds"]
    s = share(y[:, :N], ref, bound)
    record(f"mul_mat_f16_xh {case}: worst error / bound {s:.3g}")
    assert s <= 1.0, s
    # the columns past N come back as they went in: with the scalar store, and under a partial column tile
    assert same_bits(y[:, N:], np.full((T, ld_pad), cs.POISON, np.float32))
    # the three kernels run the same chain of matrix-core steps over k and the same epilogue: the same bits, padding included
    for kern in ("direct-64", "direct-128"):
        assert same_bits(ys[kern], y), (kern, float(np.abs(ys[kern][:, :N] - y[:, :N]).max()))
    if cs.gemm_form1_ok(case):                                    # ... and so does the unfused chain of launches
        for kern in ("direct-64", "direct-128"):
            y1 = run_gemm(be, monkeypatch, case, kern, form=1)
            assert same_bits(y1, y), (kern, float(np.abs(y1 - y).max()))


@pytest.mark.parametrize("N,K", cs.ONE_HOT)
def test_f16_gemm_one_hot_rows_are_exact(be, monkeypatch, N, K):
    """x[t] = e_k: y[t][n] = resid + (W[n][k] + bias[n]) * 2 in small integers - every k at an edge of the kernels' steps over k lands in its own column of
    the product and nowhere else (a k fetched twice, dropped or multiplied against its neighbour shows as a wrong integer)"""
    W, x, b, r, want = cs.one_hot_inputs(N, K)
    for kern in cs.GEMM_KERNELS:
        set_switches(monkeypatch, cs.GEMM_VARS, cs.GEMM_KERNELS[kern])
        forms = (0,) if kern == "lds" else (0, 1)
        for form in forms:
            y = be.mul_mat_f16_xh(W, x, bias=b, scale=2.0, resid=r, form=form)
            bad = np.argwhere(bits(y) != bits(want))
            assert bad.size == 0, (kern, form, [(int(cs.one_hot_ks(K)[t]), int(n)) for t, n in bad[:8]])


@pytest.mark.parametrize("K", cs.GEMM_BAD_KS)
def test_f16_gemm_refuses_k_not_a_multiple_of_16(be, monkeypatch, K):
    """both kernels take k in steps of 16: the launchers refuse before any matrix launch (nothing of such a K is ever run)"""
    W, x = np.zeros((32, K), np.float16), np.zeros((8, K), np.float32)
    for kern in cs.GEMM_KERNELS:
        set_switches(monkeypatch, cs.GEMM_VARS, cs.GEMM_KERNELS[kern])
        for form in (0, 1):
            rc, _ = be.mul_mat_f16_xh_rc(W, x, form=form)
            assert rc != 0, (kern, form)


def test_f32_to_f16_rounds_to_nearest_even(be):
    x = cs.f16_round_inputs()
    got = be.f32_to_f16(x)
    want = R.f16(x)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, [(float(x[i]), hex(int(bits(got)[i])), hex(int(bits(want)[i]))) for i in bad[:8]]


# ---------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("n", cs.LN_NS)
@pytest.mark.parametrize("T", cs.LN_TS)
def test_layer_norm_matches_float64(be, n, T):
    x, w, b = cs.ln_inputs(n, T)
    ref, bound = R.layer_norm_ref(x, w, b, cs.LN_EPS)
    y, y_h = be.layer_norm(x, w, b, cs.LN_EPS)
    s = share(y, ref, bound)
    record(f"layer_norm n={n} T={T}: worst error / bound {s:.3g}" + (f" (far row {share(y[cs.LN_ROW_FAR], ref[cs.LN_ROW_FAR], bound[cs.LN_ROW_FAR]):.3g})" if T >= 5 else ""))
    assert s <= 1.0, s
    assert same_bits(y_h, y.astype(np.float16))
    y2, y2_h = be.layer_norm(x, w, b, cs.LN_EPS, in_place=True)
    assert same_bits(y2, y) and same_bits(y2_h, y_h)
    y3, none = be.layer_norm(x, w, b, cs.LN_EPS, want_h=False)   # the launch without an f16 pointer
    assert none is None and same_bits(y3, y)


# ---------------------------------------------------------------- GELU
@pytest.mark.parametrize("quick", [False, True], ids=["tanh", "quick"])
def test_gelu_table_semantics(be, quick):
    x = cs.gelu_inputs()
    ref, bound, exact = R.gelu_ref(x, quick)
    y, y_h = be.clip_gelu(x, quick)
    s = share(y, ref, bound)
    flips = float((bits(y) != bits(R.gelu_f32(x, quick))).mean())
    record(f"clip_gelu {'quick' if quick else 'tanh'} n={x.size}: worst error / bound {s:.3g}; entries that differ from numpy's f32 recipe {flips:.3%}")
    bad = np.flatnonzero(np.abs(y.astype(np.float64) - ref) > bound)
    assert bad.size == 0, [(float(x[i]), float(y[i]), float(ref[i]), float(bound[i])) for i in bad[:8]]
    assert same_bits(y_h, y.astype(np.float16))
    # the tanh form's cut: exactly 0 at or below -10, exactly x - not rounded to f16 - at or above 10; everything else is a table entry, an f16 value
    assert exact.any() != quick and np.array_equal(y[exact].astype(np.float64), ref[exact])
    assert same_bits(y[~exact], y[~exact].astype(np.float16).astype(np.float32))
    y2, none = be.clip_gelu(x, quick, want_h=False)
    assert none is None and same_bits(y2, y)


# ---------------------------------------------------------------- the small kernels: exact
@pytest.mark.parametrize("S,P", cs.IM2COL_CASES)
def test_im2col_is_exact(be, S, P):
    img = np.random.default_rng([S, P]).standard_normal((3, S, S)).astype(np.float32)
    for ld in cs.im2col_lds(P):
        got = be.clip_im2col(img, P, ld, fill=float(cs.POISON))   # the buffer holds a pattern first: the padding columns must come back as zeros
        assert same_bits(got, R.im2col_ref(img, P, ld)), (S, P, ld)


@pytest.mark.parametrize("E,T", cs.EMBED_CASES)
def test_embed_is_exact(be, E, T):
    rng = np.random.default_rng([E, T])
    patch, cls, pos = (rng.standard_normal(s).astype(np.float32) for s in ((T - 1, E), (E,), (T, E)))
    assert same_bits(be.clip_embed(patch, cls, pos), R.embed_ref(patch, cls, pos))


@pytest.mark.parametrize("n,T", cs.BIAS_CASES)
@pytest.mark.parametrize("scale", [None, cs.GEMM_SCALE], ids=["plain", "scaled"])
def test_bias_is_exact(be, n, T, scale):
    rng = np.random.default_rng([n, T])
    x, b = rng.standard_normal((T, n)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    assert same_bits(be.clip_bias(x, b, scale), R.bias_ref(x, b, scale))


@pytest.mark.parametrize("nq,nkv,T", cs.QKV_CASES)
def test_add_qkv_bias_is_exact(be, nq, nkv, T):
    """nq != nkv; each segment skipped in turn (a null bias, with and without its rows); the second case wraps the grid-stride loop"""
    rng = np.random.default_rng([nq, nkv, T])
    xs = [rng.standard_normal((T, n)).astype(np.float32) for n in (nq, nkv, nkv)]
    bs = [rng.standard_normal(n).astype(np.float32) for n in (nq, nkv, nkv)]
    want = [x + b[None, :] for x, b in zip(xs, bs)]
    got = be.add_qkv_bias(*xs, *bs, nq, nkv, T)
    assert all(same_bits(g, w) for g, w in zip(got, want))
    for skip in range(3):
        b2 = [None if s == skip else b for s, b in enumerate(bs)]
        got = be.add_qkv_bias(*xs, *b2, nq, nkv, T)                # the rows are there, the bias is not: they come back as they went
        assert all(same_bits(g, xs[s] if s == skip else want[s]) for s, g in enumerate(got)), skip
        x2 = [None if s == skip else x for s, x in enumerate(xs)]
        got = be.add_qkv_bias(*x2, *b2, nq, nkv, T)                # neither rows nor bias
        assert got[skip] is None and all(same_bits(g, want[s]) for s, g in enumerate(got) if s != skip), skip
