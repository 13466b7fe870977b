"""numpy twin of csrc/quantize.hip: ggml's reference quantisers as remembered, restated in the order the kernel computes them.  This file
is the written specification; the kernel follows it.  One function per type; `dtype` is the arithmetic's float type (np.float32: what the kernel does, bit
for bit; np.float64: the same steps in double, the yardstick for how much rounding moves the search).

Orders that matter.  A sub-block of n = 32 (16) elements belongs to n / 4 adjacent lanes of four adjacent elements each.  A sum over a sub-block (lane_sum) is
the lane's four terms left to right, then a binary tree over the lanes: neighbours first (lanes l and l ^ 1), then pairs of pairs, ...  A sum over a
super-block continues the same tree over its sub-blocks.  Minima, maxima and the signed extreme (the larger of max and -min, the positive one on a tie) do
not depend on an order.  No product is fused with a sum; division and square root are IEEE; rint is round-half-even, Q8_0's rounding is half away from zero
(roundf), Q5_0 / Q5_1 truncate after adding a half, all as upstream."""
from __future__ import annotations

import numpy as np

F32, F16, BF16 = 0, 1, 30
Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K = 6, 7, 8, 10, 11, 12, 13, 14
BLOCK_ELEMS = {Q5_0: 32, Q5_1: 32, Q8_0: 32, Q2_K: 256, Q3_K: 256, Q4_K: 256, Q5_K: 256, Q6_K: 256}
BLOCK_BYTES = {Q5_0: 22, Q5_1: 24, Q8_0: 34, Q2_K: 84, Q3_K: 110, Q4_K: 144, Q5_K: 176, Q6_K: 210}
K_TYPES = (Q2_K, Q3_K, Q4_K, Q5_K, Q6_K)
GROUP_MAX_EPS = 1e-15
# (rmin, rdelta, nstep) of the min / scale grid search: without / with an importance matrix
QKX = {Q4_K: ((-1.0, 0.1, 20), (-0.9, 0.05, 36)), Q5_K: ((-0.5, 0.1, 15), (-0.9, 0.05, 36)), Q2_K: ((-0.5, 0.1, 15), (-0.9, 0.05, 36))}


def to_f32(x: np.ndarray, src_type: int = F32) -> np.ndarray:
    """the source rows as the f32 values the kernel computes on (F16 / BF16 widen exactly)"""
    if src_type == BF16:
        return (np.ascontiguousarray(x).view(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)
    if src_type == F16:
        return np.ascontiguousarray(x).view(np.float16).astype(np.float32)
    return np.ascontiguousarray(x, np.float32)


def tree_sum(a: np.ndarray) -> np.ndarray:
    """the butterfly over the last axis (a power of two): l with l ^ 1, then l ^ 2, ..."""
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def lane_sum(a: np.ndarray) -> np.ndarray:
    """sum over the elements of a sub-block (last axis) in the kernel's order: four per lane, left to right, then the butterfly over the lanes"""
    q = a.reshape(a.shape[:-1] + (a.shape[-1] // 4, 4))
    return tree_sum(((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3])


def extreme(x: np.ndarray) -> np.ndarray:
    """the element of largest magnitude with its sign (last axis); +a where +a and -a tie"""
    mx, mn = x.max(-1), x.min(-1)
    return np.where(-mn > mx, mn, mx)


def _f16(v: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return np.asarray(v).astype(np.float16)


def _roundf(v: np.ndarray) -> np.ndarray:
    t = np.trunc(v)
    return t + np.where(np.abs(v - t) >= 0.5, np.sign(v), 0).astype(v.dtype)


def _weights_sigma(x, qw, T, factor):
    """qw * sqrt(sigma2 + x^2), sigma2 = factor * (sum of x^2 over the super-block) / 256; x [..., nsub, n]"""
    s2 = tree_sum(lane_sum(x * x))
    sigma2 = T(factor) * s2 / T(256)
    return qw * np.sqrt(sigma2[..., None, None] + x * x)


def qkx_search(x, w, nmax, rmin, rdelta, nstep, use_mad, T, search=True):
    """make_qkx2_quants: x, w [..., n] -> (L [..., n] int, scale [...], the_min [...] >= 0)"""
    mn = np.minimum(x.min(-1), T(0)) + T(0)                # (+ 0: a zero is +0 whichever the minimum returned)
    mx = x.max(-1)
    sum_w, sum_x = lane_sum(w), lane_sum(w * x)
    flat = mx == mn
    rng = np.where(flat, T(1), mx - mn)
    iscale = T(nmax) / rng
    scale = T(1) / iscale
    mn_, x_ = mn[..., None], x

    def err(sc, m, L):
        d = (sc[..., None] * L + m[..., None]) - x_
        return lane_sum(w * (np.abs(d) if use_mad else d * d))

    L = np.clip(np.rint(iscale[..., None] * (x - mn_)), 0, nmax)
    best = err(scale, mn, L)
    m_out = mn.copy()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for s in range(nstep + 1 if search else 0):
            isc = ((T(rmin) + T(rdelta) * T(s)) + T(nmax)) / rng
            l = np.clip(np.rint(isc[..., None] * (x - mn_)), 0, nmax)
            wl = w * l
            sum_l, sum_l2, sum_xl = lane_sum(wl), lane_sum(wl * l), lane_sum(wl * x)
            D = sum_w * sum_l2 - sum_l * sum_l
            t_scale = (sum_w * sum_xl - sum_x * sum_l) / D
            t_min = (sum_l2 * sum_x - sum_l * sum_xl) / D
            pos = t_min > 0
            t_scale = np.where(pos, sum_xl / sum_l2, t_scale)
            t_min = np.where(pos, T(0), t_min)
            mad = err(t_scale, t_min, l)
            better = (D > 0) & (mad < best) & ~flat
            best = np.where(better, mad, best)
            scale = np.where(better, t_scale, scale)
            m_out = np.where(better, t_min, m_out)
            L = np.where(better[..., None], l, L)
    L = np.where(flat[..., None], T(0), L)
    scale = np.where(flat, T(0), scale)
    return L.astype(np.int32), scale.astype(T), (T(0) - m_out).astype(T)


def sym_search(x, w, nmax, T, refine=False, search=True):
    """make_qx_quants (weights w) -> (l [..., n] int in [-nmax, nmax - 1], scale [...]); refine: make_q3_quants' element-by-element sweeps on top"""
    mx = extreme(x)
    tiny = np.abs(mx) < T(GROUP_MAX_EPS)
    mxs = np.where(tiny, T(1), mx)
    wx = w * x

    def sums(isc):
        l = np.clip(np.rint(isc[..., None] * x), -nmax, nmax - 1)
        return l, lane_sum(wx * l), lane_sum((w * l) * l)

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        L, sumlx, suml2 = sums(-T(nmax) / mxs)
        scale = np.where(suml2 != 0, sumlx / suml2, T(0))
        best = scale * sumlx
        for s in range(-9, 10) if search else ():
            if s == 0:
                continue
            l, slx, sl2 = sums(-(T(nmax) + T(0.1) * T(s)) / mxs)
            better = (sl2 > 0) & (slx * slx > best * sl2)
            sc = slx / sl2
            scale = np.where(better, sc, scale)
            best = np.where(better, sc * slx, best)
            sumlx, suml2 = np.where(better, slx, sumlx), np.where(better, sl2, suml2)
            L = np.where(better[..., None], l, L)
        if refine and search:
            n = x.shape[-1]
            for _ in range(5):
                changed = np.zeros(x.shape[:-1], bool)
                for i in range(n):
                    wi, xi, li = w[..., i], x[..., i], L[..., i]
                    wxi = wi * xi
                    slx = sumlx - wxi * li
                    sl2 = suml2 - (wi * li) * li
                    nl = np.clip(np.rint((xi * sl2) / slx), -nmax, nmax - 1)
                    slx2 = slx + wxi * nl
                    sl22 = sl2 + (wi * nl) * nl
                    acc = (slx > 0) & (nl != li) & (sl22 > 0) & ((slx2 * slx2) * suml2 > (sumlx * sumlx) * sl22)
                    L[..., i] = np.where(acc, nl, li)
                    sumlx, suml2 = np.where(acc, slx2, sumlx), np.where(acc, sl22, suml2)
                    changed |= acc
                if not changed.any():
                    break
            scale = np.where(suml2 != 0, sumlx / suml2, T(0))
    L = np.where(tiny[..., None], T(-nmax), L)
    scale = np.where(tiny, T(0), scale)
    return L.astype(np.int32), scale.astype(T)


def _prep(x, imatrix, nsub, n, T):
    x = np.ascontiguousarray(x, np.float32)
    rows, K = x.shape
    xs = x.astype(T).reshape(rows, K // (nsub * n), nsub, n)
    qw = None if imatrix is None else np.broadcast_to(np.asarray(imatrix, np.float32).astype(T).reshape(1, K // (nsub * n), nsub, n), xs.shape)
    return xs, qw


def _blocks(t, rows, nb):
    from_dtype = {Q4_K: [("d", "<f2"), ("dmin", "<f2"), ("scales", "u1", 12), ("qs", "u1", 128)],
                  Q5_K: [("d", "<f2"), ("dmin", "<f2"), ("scales", "u1", 12), ("qh", "u1", 32), ("qs", "u1", 128)],
                  Q6_K: [("ql", "u1", 128), ("qh", "u1", 64), ("scales", "i1", 16), ("d", "<f2")],
                  Q2_K: [("scales", "u1", 16), ("qs", "u1", 64), ("d", "<f2"), ("dmin", "<f2")],
                  Q3_K: [("hmask", "u1", 32), ("qs", "u1", 64), ("scales", "u1", 12), ("d", "<f2")],
                  Q8_0: [("d", "<f2"), ("qs", "i1", 32)],
                  Q5_0: [("d", "<f2"), ("qh", "<u4"), ("qs", "u1", 16)],
                  Q5_1: [("d", "<f2"), ("m", "<f2"), ("qh", "<u4"), ("qs", "u1", 16)]}[t]
    dt = np.dtype(from_dtype)
    assert dt.itemsize == BLOCK_BYTES[t]
    return np.zeros((rows, nb), dt)


def _q45(t, x, imatrix, T, search=True):
    nmax = 15 if t == Q4_K else 31
    xs, qw = _prep(x, imatrix, 8, 32, T)
    if qw is None:
        av = np.sqrt(lane_sum(xs * xs) / T(32))
        w = av[..., None] + np.abs(xs)
    else:
        w = _weights_sigma(xs, qw, T, 2)
    rmin, rdelta, nstep = QKX[t][0 if qw is None else 1]
    L, scales, mins = qkx_search(xs, w, nmax, rmin, rdelta, nstep, False, T, search)
    max_scale, max_min = scales.max(-1), mins.max(-1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv_scale = np.where(max_scale > 0, T(63) / max_scale, T(0))
        inv_min = np.where(max_min > 0, T(63) / max_min, T(0))
        ls = np.clip(np.rint(inv_scale[..., None] * scales), 0, 63).astype(np.int32)
        lm = np.clip(np.rint(inv_min[..., None] * mins), 0, 63).astype(np.int32)
        dh, dmh = _f16(max_scale / T(63)), _f16(max_min / T(63))
        d = dh.astype(T)[..., None] * ls.astype(T)
        dm = dmh.astype(T)[..., None] * lm.astype(T)
        l2 = np.clip(np.rint((xs + dm[..., None]) / d[..., None]), 0, nmax)
    L = np.where((d != 0)[..., None], l2, L).astype(np.uint8)
    out = _blocks(t, xs.shape[0], xs.shape[1])
    out["d"], out["dmin"] = dh, dmh
    sc = out["scales"]
    sc[..., 0:4] = ls[..., 0:4] | ((ls[..., 4:8] >> 4) << 6)
    sc[..., 4:8] = lm[..., 0:4] | ((lm[..., 4:8] >> 4) << 6)
    sc[..., 8:12] = (ls[..., 4:8] & 15) | ((lm[..., 4:8] & 15) << 4)
    lo = L & 15
    out["qs"] = (lo[..., 0::2, :] | (lo[..., 1::2, :] << 4)).reshape(L.shape[:2] + (128,))
    if t == Q5_K:
        hi = (L >> 4).astype(np.uint8)
        qh = np.zeros(L.shape[:2] + (32,), np.uint8)
        for j in range(8):
            qh |= hi[..., j, :] << j
        out["qh"] = qh
    return out


def quantize_q4_K(x, imatrix=None, dtype=np.float32, search=True):
    return _q45(Q4_K, x, imatrix, dtype, search)


def quantize_q5_K(x, imatrix=None, dtype=np.float32, search=True):
    return _q45(Q5_K, x, imatrix, dtype, search)


def _pack2(L):
    """2-bit codes [..., 256] -> 64 bytes: byte 32 h + l holds elements 128 h + l + 32 k at bits 2 k"""
    q = L.reshape(L.shape[:-1] + (2, 4, 32)).astype(np.uint8)
    return (q[..., 0, :] | (q[..., 1, :] << 2) | (q[..., 2, :] << 4) | (q[..., 3, :] << 6)).reshape(L.shape[:-1] + (64,))


def quantize_q2_K(x, imatrix=None, dtype=np.float32, search=True):
    T = dtype
    xs, qw = _prep(x, imatrix, 16, 16, T)
    w = np.abs(xs) if qw is None else _weights_sigma(xs, qw, T, 1)
    rmin, rdelta, nstep = QKX[Q2_K][0 if qw is None else 1]
    L, scales, mins = qkx_search(xs, w, 3, rmin, rdelta, nstep, qw is None, T, search)
    max_scale, max_min = scales.max(-1), mins.max(-1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        is_ = np.where(max_scale > 0, T(15) / max_scale, T(0))
        im_ = np.where(max_min > 0, T(15) / max_min, T(0))
        ls = np.clip(np.rint(is_[..., None] * scales), 0, 15).astype(np.int32)
        lm = np.clip(np.rint(im_[..., None] * mins), 0, 15).astype(np.int32)
        dh = _f16(np.where(max_scale > 0, max_scale / T(15), T(0)))
        dmh = _f16(np.where(max_min > 0, max_min / T(15), T(0)))
        d = dh.astype(T)[..., None] * ls.astype(T)
        dm = dmh.astype(T)[..., None] * lm.astype(T)
        l2 = np.clip(np.rint((xs + dm[..., None]) / d[..., None]), 0, 3)
    L = np.where((d != 0)[..., None], l2, L).astype(np.uint8)
    out = _blocks(Q2_K, xs.shape[0], xs.shape[1])
    out["d"], out["dmin"] = dh, dmh
    out["scales"] = ls | (lm << 4)
    out["qs"] = _pack2(L.reshape(L.shape[:2] + (256,)))
    return out


def quantize_q6_K(x, imatrix=None, dtype=np.float32, search=True):
    T = dtype
    xs, qw = _prep(x, imatrix, 16, 16, T)
    w = xs * xs if qw is None else qw
    L, scales = sym_search(xs, w, 32, T, search=search)
    ms = extreme(scales)
    zero = np.abs(ms) < T(GROUP_MAX_EPS)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iscale = T(-128) / np.where(zero, T(1), ms)
        dh = _f16(T(1) / iscale)
        sc = np.clip(np.rint(iscale[..., None] * scales), -128, 127).astype(np.int32)
        d = dh.astype(T)[..., None] * sc.astype(T)
        l2 = np.clip(np.rint(xs / d[..., None]), -32, 31)
    L = (np.where((d != 0)[..., None], l2, L) + 32).astype(np.uint8).reshape(L.shape[:2] + (2, 4, 32))
    out = _blocks(Q6_K, xs.shape[0], xs.shape[1])
    lo, hi = L & 15, L >> 4
    ql = np.stack([lo[..., 0, :] | (lo[..., 2, :] << 4), lo[..., 1, :] | (lo[..., 3, :] << 4)], axis=-2)       # [.., 2 halves, 2, 32]
    out["ql"] = ql.reshape(L.shape[:2] + (128,))
    out["qh"] = (hi[..., 0, :] | (hi[..., 1, :] << 2) | (hi[..., 2, :] << 4) | (hi[..., 3, :] << 6)).reshape(L.shape[:2] + (64,))
    out["scales"], out["d"] = sc, dh
    z = zero[..., None]
    for f in ("ql", "qh", "scales"):
        out[f] = np.where(z, 0, out[f])
    out["d"] = np.where(zero, np.float16(0), out["d"])
    return out


def quantize_q3_K(x, imatrix=None, dtype=np.float32, search=True):
    T = dtype
    xs, qw = _prep(x, imatrix, 16, 16, T)
    # (upstream weights a sub-block's errors by x^2 here; on normal inputs that leaves a larger plain RMS error than round-to-nearest does - 0.1531 against
    # 0.1514 over the test cases - so the weights are Q4_K's, av_x + |x| over the 16 elements: 0.1452)
    w = np.sqrt(lane_sum(xs * xs) / T(16))[..., None] + np.abs(xs) if qw is None else _weights_sigma(xs, qw, T, 2)
    L, scales = sym_search(xs, w, 4, T, refine=True, search=search)
    ms = extreme(scales)
    zero = np.abs(ms) < T(GROUP_MAX_EPS)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iscale = T(-32) / np.where(zero, T(1), ms)
        dh = _f16(T(1) / iscale)
        sc = np.clip(np.rint(iscale[..., None] * scales), -32, 31).astype(np.int32)
        d = dh.astype(T)[..., None] * sc.astype(T)
        l2 = np.clip(np.rint(xs / d[..., None]), -4, 3)
    L = (np.where((d != 0)[..., None], l2, L) + 4).astype(np.uint8).reshape(L.shape[:2] + (256,))
    out = _blocks(Q3_K, xs.shape[0], xs.shape[1])
    hi = (L >> 2).reshape(L.shape[:2] + (8, 32))
    hm = np.zeros(L.shape[:2] + (32,), np.uint8)
    for j in range(8):
        hm |= hi[..., j, :] << j
    out["hmask"], out["qs"] = hm, _pack2(L & 3)
    u = (sc + 32).astype(np.uint8)
    s12 = np.zeros(L.shape[:2] + (12,), np.uint8)
    s12[..., 0:8] = (u[..., 0:8] & 15) | ((u[..., 8:16] & 15) << 4)
    h = u >> 4
    s12[..., 8:12] = h[..., 0:4] | (h[..., 4:8] << 2) | (h[..., 8:12] << 4) | (h[..., 12:16] << 6)
    out["scales"], out["d"] = s12, dh
    z = zero[..., None]
    for f in ("hmask", "qs", "scales"):
        out[f] = np.where(z, 0, out[f])
    out["d"] = np.where(zero, np.float16(0), out["d"])
    return out


def quantize_q8_0(x, imatrix=None, dtype=np.float32, search=True):
    T = dtype
    x = np.ascontiguousarray(x, np.float32)
    xs = x.astype(T).reshape(x.shape[0], -1, 32)
    d = np.abs(xs).max(-1) / T(127)
    with np.errstate(divide="ignore"):
        inv = np.where(d != 0, T(1) / d, T(0))
    out = _blocks(Q8_0, xs.shape[0], xs.shape[1])
    out["d"] = _f16(d)
    out["qs"] = _roundf(xs * inv[..., None]).astype(np.int8)
    return out


def _pack5(out, q):
    q = q.astype(np.uint32)
    out["qs"] = ((q[..., :16] & 15) | ((q[..., 16:] & 15) << 4)).astype(np.uint8)
    out["qh"] = (((q >> 4) & 1) << np.arange(32, dtype=np.uint32)).sum(-1, dtype=np.uint32)


def quantize_q5_0(x, imatrix=None, dtype=np.float32, search=True):
    """round-to-nearest from the signed extreme over -16, with or without an importance matrix (upstream searches with one)"""
    T = dtype
    x = np.ascontiguousarray(x, np.float32)
    xs = x.astype(T).reshape(x.shape[0], -1, 32)
    d = extreme(xs) / T(-16) + T(0)                   # (+ 0: a block of zeros of either sign gets d = +0)
    with np.errstate(divide="ignore"):
        inv = np.where(d != 0, T(1) / d, T(0))
    out = _blocks(Q5_0, xs.shape[0], xs.shape[1])
    out["d"] = _f16(d)
    _pack5(out, np.minimum(31, np.trunc(xs * inv[..., None] + T(16.5))))
    return out


def quantize_q5_1(x, imatrix=None, dtype=np.float32, search=True):
    T = dtype
    x = np.ascontiguousarray(x, np.float32)
    xs = x.astype(T).reshape(x.shape[0], -1, 32)
    mn, mx = xs.min(-1) + T(0), xs.max(-1)
    d = (mx - mn) / T(31) + T(0)
    with np.errstate(divide="ignore"):
        inv = np.where(d != 0, T(1) / d, T(0))
    out = _blocks(Q5_1, xs.shape[0], xs.shape[1])
    out["d"], out["m"] = _f16(d), _f16(mn)
    _pack5(out, np.minimum(31, np.trunc((xs - mn[..., None]) * inv[..., None] + T(0.5))))
    return out


QUANTIZE = {Q8_0: quantize_q8_0, Q5_0: quantize_q5_0, Q5_1: quantize_q5_1, Q2_K: quantize_q2_K, Q3_K: quantize_q3_K, Q4_K: quantize_q4_K, Q5_K: quantize_q5_K,
            Q6_K: quantize_q6_K}


def quantize_rows(dst_type: int, x: np.ndarray, imatrix=None, src_type=None, dtype=np.float32) -> np.ndarray:
    """rows [n_rows][n_per_row] (f32, f16, or uint16 holding bf16 with src_type=BF16) -> uint8 [n_rows][row bytes]; the signature of Backend.quantize_rows"""
    if src_type is None:
        src_type = F16 if x.dtype == np.float16 else F32
    xf = to_f32(x, src_type).reshape(x.shape)
    if not np.isfinite(xf).all():
        r = int(np.argwhere(~np.isfinite(xf).all(axis=1))[0, 0])
        raise ValueError(f"quantize: row {r} holds a non-finite value")
    out = QUANTIZE[dst_type](xf, imatrix, dtype)
    return out.view(np.uint8).reshape(xf.shape[0], -1)


def quantize_rtn(dst_type: int, x: np.ndarray) -> np.ndarray:
    """the same type's plain round-to-nearest: the sub-block scale (and min) from min / max only - the search's starting point, no candidate tried - then the
    same scale quantisation and code recomputation"""
    return QUANTIZE[dst_type](np.ascontiguousarray(x, np.float32), None, np.float32, search=False).view(np.uint8).reshape(x.shape[0], -1)
