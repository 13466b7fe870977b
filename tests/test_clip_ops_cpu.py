"""The references, bounds and case lists of the image encoder's op-level tests, checked without a GPU (tests/clip_ops_ref.py, tests/clip_ops_cases.py):

  - chained in the order host/clip.cc issues its launches, the references reproduce the C restatement's encoder (oracle/oq_clip.c) within the tolerance
    tests/test_golden_clip.py holds it to: the references describe the encoder, not something of their own;
  - an f32 evaluation of every op by numpy (its own summation order) stays inside the op's bound on every case: the bounds are not too tight for f32;
  - every mutant - a reference with one fault of the kind a kernel could have - leaves the bound on the case list: the lists and bounds can see such a fault;
  - the dispatch edges and refusals of the case list agree with the LDS arithmetic stated beside them."""
import numpy as np
import pytest

import clip_ops_cases as cs
import clip_ops_ref as R
import oracle_py as oq


def photo(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x * y) % 256)], -1).astype(np.int32)
    img += rng.integers(-40, 41, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("cfg", ["tiny-clip", "tiny-clip-gelu"])
def test_chained_references_reproduce_the_c_restatement(pkg, tmp_path, cfg):
    path = str(tmp_path / (cfg + ".gguf"))
    pkg.gguf_synth.write_synthetic_clip(path, cfg)
    o = oq.OracleClip(path)
    t, kv = R.read_clip_file(path)
    img = o.preprocess(photo(90, 60, 1))
    ref = o.encode(img)
    got = R.encode_chain(t, kv, img)
    o.close()
    err = np.abs(got - ref) / float(np.abs(ref).max())
    assert err.max() <= 2e-3 and np.median(err) <= 2e-4, (float(err.max()), float(np.median(err)))


def worst(got, ref, bound) -> float:
    """the largest |got - ref| as a share of its bound (0 where both are 0)"""
    d = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(d == 0, 0.0, d / bound).max())


def outside(got, ref, bound) -> int:
    return int((np.abs(np.asarray(got, np.float64) - ref) > bound).sum())


# ---------------------------------------------------------------- attention
ATTN_SHAPES = sorted({(T, cs.ATTN_H, D) for D, _, T, _ in cs.PARITY_CASES} | {(T, 1, D) for D, _, T, _ in cs.ATTN_EDGES})


@pytest.mark.parametrize("T,H,D", ATTN_SHAPES)
def test_attention_bound_holds_for_f32(T, H, D):
    ref, bound = cs.attn_case_ref(T, H, D)
    assert worst(R.attn_f32(*cs.attn_inputs(T, H, D), T, H, D), ref, bound) <= 1.0


@pytest.mark.parametrize("D", sorted(cs.D_PATHS))
def test_attention_needles_are_what_they_claim(D):
    """the reference's needle rows are v[j] to 1e-9, and the f32 evaluation has them within the bound"""
    q, k, v = cs.needle_inputs(D)
    T, H = cs.NEEDLE_T, cs.ATTN_H
    ref, bound = R.attn_ref(q, k, v, T, H, D)
    got = R.attn_f32(q, k, v, T, H, D)
    keys, queries = set(), set()
    for h in range(H):
        for qi, kj in cs.needle_pairs(h):
            sl = slice(h * D, (h + 1) * D)
            assert qi != kj and np.abs(ref[qi, sl] - v[kj, sl]).max() <= 1e-9
            assert (np.abs(got[qi, sl] - v[kj, sl].astype(np.float64)) <= bound[qi, sl] + 1e-9).all()
            keys.add(kj); queries.add(qi)
    assert keys == set(cs.NEEDLE_KEYS) and queries >= set(cs.NEEDLE_QUERIES)
    assert worst(got, ref, bound) <= 1.0


def test_attention_mutant_dropped_last_key():
    """every parity shape with more than one key sees the last key missing; so does the needle at key T - 1"""
    for T, H, D in ATTN_SHAPES:
        if T == 1:
            continue
        ref, bound = cs.attn_case_ref(T, H, D)
        mut, _ = R.attn_ref(*cs.attn_inputs(T, H, D), T, H, D, drop_last_key=True)
        assert outside(mut, ref, bound) > 0, (T, H, D)
    for D in sorted(cs.D_PATHS):
        q, k, v = cs.needle_inputs(D)
        ref, bound = R.attn_ref(q, k, v, cs.NEEDLE_T, cs.ATTN_H, D)
        mut, _ = R.attn_ref(q, k, v, cs.NEEDLE_T, cs.ATTN_H, D, drop_last_key=True)
        qi = [a for a, b in cs.needle_pairs(0) if b == cs.NEEDLE_T - 1][0]
        assert (np.abs(mut[qi, :D] - ref[qi, :D]) > 100 * bound[qi, :D]).all(), D


def test_attention_mutant_key_chunk_of_63():
    """63 keys taken of every 64: every shape with T >= 64 sees it (below, there is no key 63 to lose), and the needles at keys 63 and 127"""
    for T, H, D in ATTN_SHAPES:
        ref, bound = cs.attn_case_ref(T, H, D)
        mut, _ = R.attn_ref(*cs.attn_inputs(T, H, D), T, H, D, skip_every=64)
        assert (outside(mut, ref, bound) > 0) == (T >= 64), (T, H, D)
    for D in sorted(cs.D_PATHS):
        q, k, v = cs.needle_inputs(D)
        ref, bound = R.attn_ref(q, k, v, cs.NEEDLE_T, cs.ATTN_H, D)
        mut, _ = R.attn_ref(q, k, v, cs.NEEDLE_T, cs.ATTN_H, D, skip_every=64)
        for kj in (63, 127):
            qi = [a for a, b in cs.needle_pairs(0) if b == kj][0]
            assert (np.abs(mut[qi, :D] - ref[qi, :D]) > 100 * bound[qi, :D]).all(), (D, kj)


# ---------------------------------------------------------------- f16 GEMM
def gemm_ref_of(case, **mutant):
    W, x, b, scale, r, ld = cs.gemm_inputs(case)
    return R.gemm_ref(W, x, b, scale, r, ld, **mutant)


@pytest.mark.parametrize("case", cs.GEMM_CASES)
def test_gemm_bound_holds_for_f32(case):
    W, x, b, scale, r, ld = cs.gemm_inputs(case)
    ref, bound = gemm_ref_of(case)
    assert worst(R.gemm_f32(W, x, b, scale, r, ld), ref, bound) <= 1.0


def test_gemm_case_list_covers_what_it_claims():
    Ns, Ts, Ks = ({c[i] for c in cs.GEMM_CASES} for i in range(3))
    assert Ns == {32, 33, 63, 64, 65, 100, 130, 256} and Ts == {8, 9, 63, 64, 65, 129} and Ks == {16, 48, 64, 80, 592, 1040}
    for i in (3, 4, 5, 6, 7):                                    # bias, scale, residual, padded rows, in place: each on and off
        assert {bool(c[i]) for c in cs.GEMM_CASES} == {False, True}, i
    assert all(c[5] for c in cs.GEMM_CASES if c[7])              # in place only with a residual
    # both stores: the scalar one (ld_out % 4 != 0), the 16-byte one ending in a partial group (N % 4 != 0, ld_out % 4 == 0) and in whole groups
    lds = [(c[0], c[0] + c[6]) for c in cs.GEMM_CASES]
    assert any(ld % 4 for _, ld in lds) and any(N % 4 and ld % 4 == 0 for N, ld in lds) and any(N % 4 == 0 and ld == N and N % 64 for N, ld in lds)
    assert all(K % 16 == 8 for K in cs.GEMM_BAD_KS)
    for N, K in cs.ONE_HOT:
        ks = cs.one_hot_ks(K)
        assert K - 1 in ks and 0 in ks and set(range(16, K, 16)) <= set(ks) and set(range(64, K, 64)) <= set(ks)


def test_gemm_mutant_bias_shifted_by_one_column():
    for case in cs.GEMM_CASES:
        if case[3]:
            ref, bound = gemm_ref_of(case)
            assert outside(gemm_ref_of(case, bias_shift=1)[0], ref, bound) > 0.9 * ref.size, case


def test_gemm_mutant_residual_read_at_stride_n():
    """only the cases with padded rows can see it - and every one of them does, from the second row on"""
    seen = 0
    for case in cs.GEMM_CASES:
        N, T, K, bias, scale, resid, ld_pad, in_place = case
        if resid and ld_pad:
            ref, bound = gemm_ref_of(case)
            mut = gemm_ref_of(case, resid_stride=N)[0]
            assert (np.abs(mut[1:] - ref[1:]) > bound[1:]).mean() > 0.9, case
            seen += 1
    assert seen >= 3


# ---------------------------------------------------------------- LayerNorm
LN_CASES = [(n, T) for n in cs.LN_NS for T in cs.LN_TS]


@pytest.mark.parametrize("n,T", LN_CASES)
def test_layer_norm_bound_holds_for_f32(n, T):
    x, w, b = cs.ln_inputs(n, T)
    ref, bound = R.layer_norm_ref(x, w, b, cs.LN_EPS)
    assert worst(R.layer_norm_f32(x, w, b, cs.LN_EPS), ref, bound) <= 1.0
    if T >= 5:                                                   # variance 0: the bias comes back, exactly
        assert np.array_equal(ref[cs.LN_ROW_CONST], b.astype(np.float64)) and np.array_equal(ref[cs.LN_ROW_ZERO], b.astype(np.float64))


def test_layer_norm_mutant_one_pass_variance():
    """the row with mean 1000 and spread 0.01 is what sees it, at every n"""
    for n, T in LN_CASES:
        if T < 5:
            continue
        x, w, b = cs.ln_inputs(n, T)
        ref, bound = R.layer_norm_ref(x, w, b, cs.LN_EPS)
        mut, _ = R.layer_norm_ref(x, w, b, cs.LN_EPS, one_pass=True)
        r = cs.LN_ROW_FAR
        assert (np.abs(mut[r] - ref[r]) > bound[r]).mean() > 0.5, (n, T)


# ---------------------------------------------------------------- GELU
@pytest.mark.parametrize("quick", [False, True])
def test_gelu_bound_holds_for_the_f32_recipe(quick):
    x = cs.gelu_inputs()
    assert x.size % 256 != 0 and x.size > 4 * 63488 - 8
    ref, bound, exact = R.gelu_ref(x, quick)
    got = R.gelu_f32(x, quick)
    assert worst(got, ref, bound) <= 1.0
    if not quick:
        assert exact.sum() > 1000 and np.array_equal(got[exact].astype(np.float64), ref[exact])
        f = np.float32
        for v, want in ((f(10), f(10)), (np.nextafter(f(10), f(20)), np.nextafter(f(10), f(20))), (f(-10), f(0)), (np.nextafter(f(-10), f(-20)), f(0))):
            assert ref[x == v][0] == want and exact[x == v].all()
        assert not exact[x == np.nextafter(f(10), f(0))].any() and not exact[x == np.nextafter(f(-10), f(0))].any()


def test_gelu_mutant_constants():
    """0.0447 for 0.044715 and 1.7 for 1.702: the table entries f16(r') of the mutant leave the bound on some of the finite f16 inputs"""
    h = cs.all_f16()
    assert h.size == 63488
    ref, bound, _ = R.gelu_ref(h, False)
    mut = R.f16(R.gelu_ref(h, False, gelu_a=0.0447)[0]).astype(np.float64)
    assert outside(mut, ref, bound) >= 50
    ref, bound, _ = R.gelu_ref(h, True)
    mut = R.f16(R.gelu_ref(h, True, quick_c=1.7)[0]).astype(np.float64)
    assert outside(mut, ref, bound) >= 2000


# ---------------------------------------------------------------- the case list's arithmetic
def test_dispatch_edges_and_refusals_agree_with_the_lds_arithmetic():
    for D, sw, T, path in cs.ATTN_EDGES:
        assert cs.expected_path(T, D, sw) == path, (D, sw, T)
    by_kernel = {}
    for D, sw, T, path in cs.ATTN_EDGES:
        by_kernel.setdefault((D, sw), []).append((T, path))
    for (D, sw), (a, b) in by_kernel.items():                    # the largest T of a kernel and one past it: the kernel's LDS fits at one, not at the other
        assert b[0] == a[0] + 1 and a[1] != b[1] and b[1] == cs.WAVE
        assert cs.lds_floats(a[1], a[0], D) <= cs.LDS_FLOATS < cs.lds_floats(a[1], b[0], D)
    assert {(D, sw): a[0] for (D, sw), (a, _) in by_kernel.items()} == {(64, "default"): 896, (64, "no-mfma"): 832, (128, "default"): 640, (32, "default"): 896}
    for D, sw, T in cs.ATTN_REFUSALS:
        assert cs.expected_path(T, D, sw) == cs.REFUSED, (D, sw, T)
    assert cs.expected_path(cs.WAVE_MAX_T, 80, "default") == cs.WAVE and cs.lds_floats(cs.WAVE, cs.WAVE_MAX_T, 80) == cs.WAVE_LDS_FLOATS
    for D, sw, T, path in cs.PARITY_CASES + cs.BATCH_CASES:      # no case falls through to another kernel than it names
        assert cs.expected_path(T, D, sw) == path, (D, sw, T)
    for D, sw, path in cs.NEEDLE_CASES:
        assert cs.expected_path(cs.NEEDLE_T, D, sw) == path
    assert set(cs.ATTN_TS) == {1, 3, 4, 5, 31, 32, 33, 40, 41, 63, 64, 65, 127, 128, 129, 256, 257, 577}
    for n, T in cs.BIAS_CASES:
        assert (n * T) % 256
    nq, nkv, T = cs.QKV_CASES[-1]
    assert nq * T > 2048 * 256 and nq != nkv
