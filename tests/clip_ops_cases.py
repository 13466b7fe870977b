"""Case lists and inputs of the image encoder's op-level tests (tests/test_clip_ops_cpu.py checks the lists themselves, tests/test_gpu_clip_ops.py runs them).

Shapes are the smallest at which a kernel can still go wrong: row counts on either side of every tile and chunk edge (the tiled kernel takes 40 queries and 64
keys at a time, the matrix-core kernel 32 and 128, the one-wave kernel strides the keys by 64), H <= 2, at most 3 images.

Which attention kernel runs is decided by head size, two environment switches and the LDS each kernel asks for (clip_attn_choice, csrc/clip.hip).  A workgroup
may hold 160 KiB = 40960 floats; the one-wave kernel keeps to 64 KiB = 16384 floats.  In floats, with Tp = T rounded up to the key chunk:
    matrix cores (D = 64)  32 * 65 + 128 * 65 + 32 * (Tp + 1)  <= 40960   ->  Tp + 1 <= 955      ->  Tp <= 896 (chunk 128)  ->  T <= 896
    tiled, D = 32          40 * 32 + 64 * 36 + 40 * Tp         <= 40960   ->  Tp <= 934.4        ->  Tp <= 896 (chunk 64)   ->  T <= 896
    tiled, D = 64          40 * 64 + 64 * 68 + 40 * Tp         <= 40960   ->  Tp <= 851.2        ->  Tp <= 832              ->  T <= 832
    tiled, D = 128         40 * 128 + 64 * 132 + 40 * Tp       <= 40960   ->  Tp <= 684.8        ->  Tp <= 640              ->  T <= 640
    one wave per query     4 * T                               <= 16384                                                     ->  T <= 4096
One row past a kernel's last T, the next kernel down takes the call: from the matrix cores at T = 897 the tiled kernel (D = 64: T <= 832) is out as well, so the
one-wave kernel runs; past that one's 4096 rows, and for a head size it is not compiled for, the launcher refuses."""
from __future__ import annotations

import functools

import numpy as np

import clip_ops_ref as R

REFUSED, MFMA, TILED, WAVE = 0, 1, 2, 3
LDS_FLOATS, WAVE_LDS_FLOATS = 160 * 1024 // 4, 64 * 1024 // 4
# the switches a case runs under (every other value of the two variables is removed first)
SWITCHES = {"default": {}, "no-mfma": {"MI355_CLIP_ATTN_MFMA": "0"}, "one-wave": {"MI355_CLIP_ATTN_TILED": "0"}}
SWITCH_VARS = ("MI355_CLIP_ATTN_TILED", "MI355_CLIP_ATTN_MFMA")
# every path a head size can take: (switch, kernel) - for T within that kernel's LDS
D_PATHS = {32: [("default", TILED), ("one-wave", WAVE)],
           64: [("default", MFMA), ("no-mfma", TILED), ("one-wave", WAVE)],
           128: [("default", TILED), ("one-wave", WAVE)],
           80: [("default", WAVE)]}
ATTN_TS = [1, 3, 4, 5, 31, 32, 33, 40, 41, 63, 64, 65, 127, 128, 129, 256, 257, 577]
D80_TS = [5, 65, 130]
ATTN_H = 2
# (D, switch, T, kernel): the largest T each kernel takes and one past it (the arithmetic above), H = 1
ATTN_EDGES = [(64, "default", 896, MFMA), (64, "default", 897, WAVE),
              (64, "no-mfma", 832, TILED), (64, "no-mfma", 833, WAVE),
              (128, "default", 640, TILED), (128, "default", 641, WAVE),
              (32, "default", 896, TILED), (32, "default", 897, WAVE)]
# (D, switch, T): refused - a head size without a kernel; one row past the one-wave kernel's LDS (with D = 80 it is the only kernel, with the switch the only one asked)
ATTN_REFUSALS = [(48, "default", 5), (48, "one-wave", 5), (80, "default", 4097), (64, "one-wave", 4097)]
WAVE_MAX_T = 4096
PARITY_CASES = [(D, sw, T, path) for D in (32, 64, 128) for sw, path in D_PATHS[D] for T in ATTN_TS] + [(80, "default", T, WAVE) for T in D80_TS]
# several images in one launch: rows on both sides of a chunk edge of every kernel
BATCH_CASES = [(D, sw, T, path) for D in (32, 64, 128, 80) for sw, path in D_PATHS[D] for T in (41, 129)]
# needle rows: T = 130 puts keys (and queries) 0, 31, 32, 39, 40, 63, 64, 127, 128 and T - 1 = 129 on both sides of every tile edge of the three kernels
NEEDLE_T = 130
NEEDLE_KEYS = [0, 31, 32, 39, 40, 63, 64, 127, 128, NEEDLE_T - 1]
NEEDLE_QUERIES = [0, 31, 32, 39, 40, NEEDLE_T - 1]
NEEDLE_CASES = [(D, sw, path) for D in (32, 64, 128, 80) for sw, path in D_PATHS[D]]


def lds_floats(path: int, T: int, D: int) -> int:
    """the LDS, in floats, kernel `path` asks for - restated from the kernels' layouts (see the table above)"""
    if path == MFMA:
        return 32 * 65 + 128 * 65 + 32 * ((T + 127) // 128 * 128 + 1)
    if path == TILED:
        return 40 * D + 64 * (D + 4) + 40 * ((T + 63) // 64 * 64)
    return 4 * T


def expected_path(T: int, D: int, switch: str) -> int:
    sw = SWITCHES[switch]
    tiled, mfma = sw.get("MI355_CLIP_ATTN_TILED") != "0", sw.get("MI355_CLIP_ATTN_MFMA") != "0"
    if tiled and mfma and D == 64 and lds_floats(MFMA, T, D) <= LDS_FLOATS:
        return MFMA
    if tiled and D in (32, 64, 128) and lds_floats(TILED, T, D) <= LDS_FLOATS:
        return TILED
    if D in (32, 64, 80, 128) and lds_floats(WAVE, T, D) <= WAVE_LDS_FLOATS:
        return WAVE
    return REFUSED


@functools.lru_cache(maxsize=None)
def attn_inputs(T: int, H: int, D: int, n_img: int = 1, seed: int = 0):
    """q (scaled as the tower scales it), k, v [n_img * T][H * D] - read-only, shared between tests"""
    rng = np.random.default_rng([T, H, D, n_img, seed])
    q = (rng.standard_normal((n_img * T, H * D)) * (2.0 / np.sqrt(D))).astype(np.float32)
    k = rng.standard_normal((n_img * T, H * D)).astype(np.float32)
    v = rng.standard_normal((n_img * T, H * D)).astype(np.float32)
    for a in (q, k, v):
        a.setflags(write=False)
    return q, k, v


@functools.lru_cache(maxsize=None)
def attn_case_ref(T: int, H: int, D: int, n_img: int = 1, seed: int = 0):
    ref, bound = R.attn_ref(*attn_inputs(T, H, D, n_img, seed), T, H, D, n_img)
    ref.setflags(write=False)
    bound.setflags(write=False)
    return ref, bound


def needle_pairs(h: int):
    """(query row, key row) pairs of head h: every boundary key is some query's needle, and every boundary query row holds a needle (the queries sit on the
    key list's rows, which contain NEEDLE_QUERIES; head 0 pairs them in reverse, head 1 three places on, so no query points at its own row)"""
    n = len(NEEDLE_KEYS)
    return [(NEEDLE_KEYS[m], NEEDLE_KEYS[n - 1 - m] if h == 0 else NEEDLE_KEYS[(m + 3) % n]) for m in range(n)]


@functools.lru_cache(maxsize=None)
def needle_inputs(D: int, H: int = ATTN_H):
    """Small random q, k; the needle query and its key share one coordinate of size 6 (a score of 36 where the others stay below about 1), every needle key its
    own coordinate.  v[j] is a ramp that names the row: (j + 1)^2 / 8 + column / 1024, exact in f32 (quadratic in j, so that the mean of the other rows -
    what a query gets whose needle key is dropped - is far from every boundary row)."""
    T = NEEDLE_T
    rng = np.random.default_rng([D, H, 77])
    q = (0.05 * rng.standard_normal((T, H, D))).astype(np.float32)
    k = (0.05 * rng.standard_normal((T, H, D))).astype(np.float32)
    v = ((np.arange(T, dtype=np.float64)[:, None] + 1.0) ** 2 / 8.0 + np.arange(H * D, dtype=np.float64)[None, :] / 1024.0).astype(np.float32)
    for h in range(H):
        for qi, kj in needle_pairs(h):
            slot = NEEDLE_KEYS.index(kj)
            k[kj, h, slot] = 6.0
            q[qi, h, slot] = 6.0
    q, k = q.reshape(T, H * D), k.reshape(T, H * D)
    for a in (q, k, v):
        a.setflags(write=False)
    return q, k, v


# ---------------------------------------------------------------- f16 GEMM: (N, T, K, bias, scale, resid, ld_pad, in_place) - a covering subset of
# N {32, 33, 63, 64, 65, 100, 130, 256} x T {8, 9, 63, 64, 65, 129} x K {16, 48, 64, 80, 592, 1040} with every epilogue part on and off.  The 16-byte store is
# taken when four columns fit and ld_out % 4 == 0: ld_pad 3, and an N that is no multiple of 4, force the scalar store everywhere; (33, ., ., ld 36) and N = 100
# keep the 16-byte store and end in a partial group / a partial column tile.
GEMM_SCALE = 0.11180339753627777                                 # f32(1 / sqrt(80)): no power of two
GEMM_CASES = [
    (32, 8, 16, 0, 0, 0, 0, 0), (33, 9, 48, 1, 0, 0, 0, 0), (63, 63, 64, 1, 1, 1, 0, 0), (64, 64, 80, 1, 0, 1, 0, 0), (65, 65, 592, 1, 1, 0, 0, 0),
    (100, 129, 1040, 1, 0, 1, 0, 1), (130, 8, 64, 0, 1, 1, 3, 0), (256, 129, 48, 1, 1, 1, 0, 1), (64, 9, 16, 1, 0, 1, 3, 0), (100, 64, 80, 1, 1, 1, 3, 1),
    (256, 65, 592, 0, 0, 1, 0, 0), (32, 129, 1040, 1, 0, 0, 3, 0), (130, 63, 16, 1, 1, 0, 0, 0), (100, 8, 592, 0, 0, 0, 0, 0), (65, 64, 1040, 1, 1, 1, 0, 0),
    (63, 65, 48, 0, 0, 1, 3, 0), (33, 129, 80, 1, 1, 1, 3, 0), (64, 8, 1040, 1, 1, 0, 0, 0),
]
GEMM_KERNELS = {"lds": {}, "direct-64": {"MI355_MMF16_LDS": "0"}, "direct-128": {"MI355_MMF16_LDS": "0", "MI355_MMF16_TILE": "128"}}
GEMM_VARS = ("MI355_MMF16_LDS", "MI355_MMF16_TILE")
GEMM_BAD_KS = [24, 40, 72]                                       # K % 16 == 8: refused by the launchers, never run
POISON = np.float32(-7777.25)
ONE_HOT = [(100, 1040), (65, 80)]                                # (N, K) of the one-hot cases


def gemm_form1_ok(case) -> bool:
    """the unfused chain writes [T][N] rows and scales only together with a bias (host/clip.cc)"""
    N, T, K, bias, scale, resid, ld_pad, in_place = case
    return ld_pad == 0 and (bias or not scale)


@functools.lru_cache(maxsize=None)
def gemm_inputs(case):
    N, T, K, bias, scale, resid, ld_pad, in_place = case
    rng = np.random.default_rng([N, T, K, 5])
    W = (rng.standard_normal((N, K)) * 0.5).astype(np.float16)
    x = rng.standard_normal((T, K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32) if bias else None
    ld = N + ld_pad
    r = None
    if resid:
        r = np.full((T, ld), POISON, np.float32)
        r[:, :N] = rng.standard_normal((T, N)).astype(np.float32) * 3.0
    for a in (W, x, b, r):
        if a is not None:
            a.setflags(write=False)
    return W, x, b, (GEMM_SCALE if scale else None), r, ld


def one_hot_ks(K: int):
    """every k a row can single out that sits at an edge of the kernels' steps over k (8 per lane, 16 per matrix-core step, 64 per LDS stage), and K - 1"""
    ks = {0, 1, 7, 8, 9, 15, K - 2, K - 1} | set(range(16, K, 16)) | {m - 1 for m in range(64, K + 1, 64)} | {m + 8 for m in range(0, K - 8, 64)}
    return sorted(k for k in ks if 0 <= k < K)


@functools.lru_cache(maxsize=None)
def one_hot_inputs(N: int, K: int):
    """x[t] = e_k(t); W, bias and the residual small integers, the scale 2: y[t][n] = resid + (W[n][k(t)] + bias[n]) * 2 exactly, in any arithmetic"""
    ks = one_hot_ks(K)
    rng = np.random.default_rng([N, K, 9])
    W = rng.integers(-8, 9, (N, K)).astype(np.float16)
    x = np.zeros((len(ks), K), np.float32)
    x[np.arange(len(ks)), ks] = 1.0
    b = rng.integers(-8, 9, N).astype(np.float32)
    r = rng.integers(-64, 65, (len(ks), N)).astype(np.float32)
    y = (r + (W.astype(np.float32)[:, ks].T + b[None, :]) * np.float32(2.0)).astype(np.float32)
    return W, x, b, r, y


# ---------------------------------------------------------------- LayerNorm
LN_NS, LN_TS, LN_EPS = [16, 100, 128, 256, 257, 1024, 1040], [1, 5, 40], 1e-5
LN_ROW_FAR, LN_ROW_CONST, LN_ROW_ZERO = 1, 2, 3                  # the special rows of a case with T >= 5


@functools.lru_cache(maxsize=None)
def ln_inputs(n: int, T: int):
    rng = np.random.default_rng([n, T, 3])
    x = (rng.standard_normal((T, n)) * 2.0 + 0.5).astype(np.float32)
    if T >= 5:
        x[LN_ROW_FAR] = (1000.0 + 0.01 * rng.standard_normal(n)).astype(np.float32)    # mean 1000, spread 0.01: E[x^2] - mean^2 in f32 is noise
        x[LN_ROW_CONST] = np.float32(3.7)                                               # variance 0: eps decides the result
        x[LN_ROW_ZERO] = 0.0
    w = (1.0 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    b = (0.1 * rng.standard_normal(n)).astype(np.float32)
    for a in (x, w, b):
        a.setflags(write=False)
    return x, w, b


# ---------------------------------------------------------------- GELU
def all_f16() -> np.ndarray:
    """the 63 488 finite f16 values, as f32"""
    h = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    return h[np.isfinite(h)].astype(np.float32)


@functools.lru_cache(maxsize=None)
def gelu_inputs() -> np.ndarray:
    """every finite f16 value; f32 values a quarter, a half (a tie) and three quarters of the way to the next f16 value; +-10 and their f32 neighbours on both
    sides (the tanh form's cut); padded with 0.5 to a length that is no multiple of 256"""
    h = np.sort(all_f16())
    lo, hi = h[:-1].astype(np.float64), h[1:].astype(np.float64)
    between = [(lo + f * (hi - lo)).astype(np.float32) for f in (0.25, 0.5, 0.75)]
    f = np.float32
    cut = np.array([s * v for s in (1.0, -1.0) for v in (np.nextafter(f(10), f(0)), f(10), np.nextafter(f(10), f(20)))], np.float32)
    x = np.concatenate([h] + between + [cut])
    if x.size % 256 == 0:
        x = np.concatenate([x, np.full(3, 0.5, np.float32)])
    x.setflags(write=False)
    return x


# ---------------------------------------------------------------- f32 -> f16
@functools.lru_cache(maxsize=None)
def f16_round_inputs() -> np.ndarray:
    """every finite f16 value; every midpoint between two neighbours (ties: to even, the last one of a binade up into the next, 65520 to infinity) and the f32
    values next to it on both sides; the subnormal range (multiples of 2^-25, so every other one is a tie); +-65504 and beyond; +-0; padded to a multiple of 4"""
    f = np.float32
    h = np.sort(all_f16())
    mid = ((h[:-1].astype(np.float64) + h[1:].astype(np.float64)) / 2).astype(f)          # (exact: one more mantissa bit)
    sub = (np.arange(-80, 81, dtype=np.float64) * 2.0 ** -25).astype(f)
    edge = np.array([65504, 65519.996, 65520, 65536, 1e5, 3e38, 2.0 ** -25, np.nextafter(f(2.0 ** -25), f(1)), 2.0 ** -26, 1e-30, 0.0], np.float64)
    edge = np.concatenate([edge, -edge]).astype(f)                                         # (-0.0 among them)
    x = np.concatenate([h, mid, np.nextafter(mid, f(-np.inf)), np.nextafter(mid, f(np.inf)), sub, edge])
    x = np.concatenate([x, np.zeros(-x.size % 4, f)])
    x.setflags(write=False)
    return x


# ---------------------------------------------------------------- the small kernels
IM2COL_CASES = [(56, 14), (32, 16), (6, 2)]                      # (S, P)
EMBED_CASES = [(16, 5), (100, 17), (1024, 10)]                   # (E, T)
BIAS_CASES = [(100, 13), (16, 17), (1000, 3)]                    # (n, T): n * T is no multiple of 256
QKV_CASES = [(48, 16, 7), (1024, 256, 600)]                      # (nq, nkv, T); the second: 614 400 elements > 2048 x 256, the grid-stride loop wraps


def im2col_lds(P: int):
    """the row lengths of a case: 3 P P itself, and padded to the next multiple of 16 (a further 16 where it is one already)"""
    kp = 3 * P * P
    return [kp, kp + 16 - kp % 16]
