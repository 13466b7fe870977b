"""float64 references and per-element bounds of the image encoder's launches (tests/test_clip_ops_cpu.py, tests/test_gpu_clip_ops.py).

Plain numpy on the f32 (or f16-rounded) operand values; no code shared with csrc/.  Every bound is computed per element from the reference's own magnitudes with
u = 2^-24 (the unit round-off of f32), never from what a kernel gives:

  attention  A = max over keys of sum_d |q_d k_d| for the query; an f32 score is off by at most e_s = (D + 2) u A in any summation order; the soft-max weights
             then move by at most 2 e_s relatively (numerator and denominator) and the T-term sums, expf, the division and the P.V sum add (T + 10) u:
             bound = (2 e_s + (T + 10) u) * sum_k p_k |v_kd|.
  f16 GEMM   products of two f16 values are exact in f32; K of them summed in any order, the bias add and the scale: with S = sum_k |w f16(x)|,
             bound = (K + 3) u (S + |bias|) |scale| + u (|y_ref| + |resid|)          (the last term: the residual add's rounding).
  LayerNorm  mean and variance in float64, each cast to f32 (what the kernel's comment states); with s = 1 / sqrt(var + eps):
             bound = 6 u (|x - mu| s |w| + |b|) + 2 u |mu| s |w|                      (the last term: the f32 rounding of the mean and of x - mean).
  GELU       h = f16(x), r = the float64 formula on h, step16(r) the f16 spacing at |r| (2^-24 in the subnormal range):
             tanh form  bound = 0.5 |h| 4u + 8u |r| + step16(r)   (4u: the f32 rounding of 1 + tanhf and a tanhf a few ulp off - below about -4 that
                                                                     cancellation decides the result)
             quick form bound = 8u |r| + step16(r).
  The rest (f32 -> f16, im2col, embed, bias, add_qkv_bias) is exact: one rounding, or none.

The mutants (a reference with one deliberate fault each) are what tests/test_clip_ops_cpu.py holds the case lists against: a case list that cannot tell a
mutant from the reference could not tell such a kernel either."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
GELU_C, GELU_A, QUICK_C = 0.79788456080286535587989211986876, 0.044715, 1.702


def f16(x) -> np.ndarray:
    """round to nearest even, as numpy converts"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16)


def h64(x) -> np.ndarray:
    return f16(x).astype(np.float64)


# ---------------------------------------------------------------- attention
def attn_ref(q, k, v, T: int, H: int, D: int, n_img: int = 1, drop_last_key: bool = False, skip_every: int = 0):
    """-> (out, bound) [n_img * T][H * D] float64.  Mutants: drop_last_key (key T - 1 is not seen); skip_every = c (the keys whose index is c - 1
    modulo c are not seen - skip_every = 64: a chunk loop that takes 63 keys of every chunk of 64)."""
    q, k, v = (np.asarray(a, np.float32).astype(np.float64).reshape(n_img, T, H, D).transpose(0, 2, 1, 3) for a in (q, k, v))
    s = q @ k.transpose(0, 1, 3, 2)                                     # [img][h][tq][tk]
    A = (np.abs(q) @ np.abs(k).transpose(0, 1, 3, 2)).max(-1, keepdims=True)
    seen = np.ones(T, bool)
    if drop_last_key:
        seen[T - 1] = False
    if skip_every:
        seen[skip_every - 1::skip_every] = False
    s = np.where(seen[None, None, None, :], s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    out = p @ v
    e_s = (D + 2) * U * A
    bound = (2.0 * e_s + (T + 10) * U) * (p @ np.abs(v))
    back = lambda a: a.transpose(0, 2, 1, 3).reshape(n_img * T, H * D)
    return back(out), back(bound)


def attn_f32(q, k, v, T: int, H: int, D: int, n_img: int = 1) -> np.ndarray:
    """the same attention evaluated in f32 by numpy (its own summation order): what the bound must hold"""
    f = np.float32
    q, k, v = (np.asarray(a, f).reshape(n_img, T, H, D).transpose(0, 2, 1, 3) for a in (q, k, v))
    s = np.matmul(q, k.transpose(0, 1, 3, 2), dtype=f)
    p = np.exp(s - s.max(-1, keepdims=True), dtype=f)
    p = (p * (f(1) / p.sum(-1, keepdims=True, dtype=f))).astype(f)
    return np.matmul(p, v, dtype=f).transpose(0, 2, 1, 3).reshape(n_img * T, H * D)


# ---------------------------------------------------------------- f16 GEMM with its epilogue
def gemm_ref(W, x, bias=None, scale=None, resid=None, ld_out=None, bias_shift: int = 0, resid_stride=None):
    """y = resid + (W . f16(x) + bias) * scale -> (y, bound) [T][N] float64; W [N][K] f16, x [T][K] f32, resid [T][ld_out] (its first N columns count).
    Mutants: bias_shift (the bias of column n - shift), resid_stride (the residual row t read at t * resid_stride of the flat buffer)."""
    W = np.asarray(W, np.float16).astype(np.float64)
    N, K = W.shape
    xt = h64(x).reshape(-1, K)
    T = xt.shape[0]
    acc = xt @ W.T
    S = np.abs(xt) @ np.abs(W).T
    b = np.zeros(N) if bias is None else np.roll(np.asarray(bias, np.float32).astype(np.float64), bias_shift)
    sc = 1.0 if scale is None else float(np.float32(scale))
    ld = N if ld_out is None else ld_out
    if resid is None:
        r = np.zeros((T, N))
    else:
        flat = np.asarray(resid, np.float32).astype(np.float64).reshape(-1)
        st = ld if resid_stride is None else resid_stride
        r = np.stack([flat[t * st:t * st + N] for t in range(T)])
    y = r + (acc + b) * sc
    bound = (K + 3) * U * (S + np.abs(b)) * abs(sc) + U * (np.abs(y) + np.abs(r))
    return y, bound


def gemm_f32(W, x, bias=None, scale=None, resid=None, ld_out=None) -> np.ndarray:
    f = np.float32
    W = np.asarray(W, np.float16).astype(f)
    N, K = W.shape
    y = np.matmul(f16(x).astype(f).reshape(-1, K), W.T, dtype=f)
    if bias is not None:
        y = y + np.asarray(bias, f)
    if scale is not None:
        y = y * f(scale)
    if resid is not None:
        y = np.asarray(resid, f).reshape(y.shape[0], -1)[:, :N] + y
    return y.astype(f)


# ---------------------------------------------------------------- LayerNorm
def layer_norm_ref(x, w, b, eps: float, one_pass: bool = False):
    """-> (y, bound) float64.  Mutant one_pass: the variance as E[x^2] - mean^2 in f32."""
    f = np.float32
    x32 = np.asarray(x, f)
    x = x32.astype(np.float64)
    w, b = np.asarray(w, f).astype(np.float64), np.asarray(b, f).astype(np.float64)
    mu = x.mean(-1, keepdims=True).astype(f).astype(np.float64)
    xc = x - mu
    var = (xc * xc).mean(-1, keepdims=True).astype(f).astype(np.float64)
    if one_pass:
        mu32 = mu.astype(f)
        var = np.maximum((x32 * x32).mean(-1, keepdims=True, dtype=f) - mu32 * mu32, f(0)).astype(np.float64)
    s = 1.0 / np.sqrt(var + float(f(eps)))
    y = xc * s * w + b
    bound = 6.0 * U * (np.abs(xc) * s * np.abs(w) + np.abs(b)) + 2.0 * U * np.abs(mu) * s * np.abs(w)
    return y, bound


def layer_norm_f32(x, w, b, eps: float) -> np.ndarray:
    f = np.float32
    x, w, b = np.asarray(x, f), np.asarray(w, f), np.asarray(b, f)
    mu = x.mean(-1, keepdims=True, dtype=np.float64).astype(f)      # (the two row sums in double, as the kernel states; everything else in f32)
    xc = x - mu
    var = (xc * xc).mean(-1, keepdims=True, dtype=np.float64).astype(f)
    return ((xc * (f(1) / np.sqrt(var + f(eps), dtype=f))) * w + b).astype(f)


# ---------------------------------------------------------------- GELU through ggml's f16 tables
def step16(r) -> np.ndarray:
    """the spacing of f16 numbers at |r|; 2^-24 below the smallest normal"""
    a = np.abs(np.asarray(r, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


def gelu_ref(x, quick: bool, gelu_a: float = GELU_A, quick_c: float = QUICK_C):
    """-> (r, bound, exact): r the float64 result the f16 table entry approximates; exact marks the inputs the tanh form answers without the table (0 at or
    below -10, x itself at or above 10), where r is the result and the bound is 0.  Mutants: another gelu_a / quick_c."""
    x32 = np.asarray(x, np.float32)
    h = h64(x32)
    with np.errstate(over="ignore"):
        if quick:
            r = h / (1.0 + np.exp(-quick_c * h))
            return r, 8.0 * U * np.abs(r) + step16(r), np.zeros(x32.shape, bool)
        r = 0.5 * h * (1.0 + np.tanh(GELU_C * h * (1.0 + gelu_a * h * h)))
    bound = 0.5 * np.abs(h) * 4.0 * U + 8.0 * U * np.abs(r) + step16(r)
    lo, hi = x32 <= -10.0, x32 >= 10.0
    r = np.where(lo, 0.0, np.where(hi, x32.astype(np.float64), r))
    return r, np.where(lo | hi, 0.0, bound), lo | hi


def gelu_f32(x, quick: bool) -> np.ndarray:
    """ggml's recipe in f32 by numpy: f16(f(f16(x))), the tanh form cut at |x| >= 10"""
    f = np.float32
    x32 = np.asarray(x, f)
    xh = f16(x32).astype(f)
    with np.errstate(over="ignore"):
        if quick:
            return f16(xh * (f(1) / (f(1) + np.exp(f(-QUICK_C) * xh, dtype=f)))).astype(f)
        g = f(0.5) * xh * (f(1) + np.tanh(f(GELU_C) * xh * (f(1) + f(GELU_A) * xh * xh), dtype=f))
    return np.where(x32 <= -10, f(0), np.where(x32 >= 10, x32, f16(g).astype(f))).astype(f)


# ---------------------------------------------------------------- the exact ones
def im2col_ref(img, P: int, ld: int) -> np.ndarray:
    """patches[p][(c P + ky) P + kx] = img[c][py P + ky][px P + kx], p = py G + px; columns from 3 P P on are zero"""
    img = np.asarray(img, np.float32)
    S = img.shape[-1]
    G = S // P
    out = np.zeros((G * G, ld), np.float32)
    for py in range(G):
        for px in range(G):
            out[py * G + px, :3 * P * P] = img[:, py * P:(py + 1) * P, px * P:(px + 1) * P].reshape(-1)
    return out


def embed_ref(patch, cls, pos) -> np.ndarray:
    f = np.float32
    return (np.concatenate([np.asarray(cls, f)[None, :], np.asarray(patch, f)], 0) + np.asarray(pos, f)).astype(f)


def bias_ref(x, b, scale=None) -> np.ndarray:
    f = np.float32
    y = np.asarray(x, f) + np.asarray(b, f)[None, :]
    return (y * f(scale)).astype(f) if scale is not None else y.astype(f)


# ---------------------------------------------------------------- the encoder as host/clip.cc chains its launches, every step one of the references above
def encode_chain(t: dict, kv: dict, img: np.ndarray) -> np.ndarray:
    """t: tensor name -> array (numpy order, slowest dimension first), kv: the file's metadata.  Every launch's result is held in f32, as on the device."""
    f = np.float32
    S, P = kv["clip.vision.image_size"], kv["clip.vision.patch_size"]
    E, H, NL = kv["clip.vision.embedding_length"], kv["clip.vision.attention.head_count"], kv["clip.vision.block_count"]
    eps, use_gelu = kv["clip.vision.attention.layer_norm_epsilon"], bool(kv.get("clip.use_gelu", False))
    D, KP = E // H, 3 * P * P
    ld = (KP + 15) // 16 * 16
    T = (S // P) ** 2 + 1

    def proj(x, w, b, scale=None, resid=None):
        return gemm_ref(t[w], x, None if b is None else t[b], scale, resid)[0].astype(f)

    wpe = np.zeros((E, ld), np.float16)
    wpe[:, :KP] = t["v.patch_embd.weight"].reshape(E, KP)
    t = dict(t, **{"patch_padded": wpe})
    pe = proj(im2col_ref(img, P, ld), "patch_padded", None)
    emb = embed_ref(pe, t["v.class_embd"], t["v.position_embd.weight"])
    emb = layer_norm_ref(emb, t["v.pre_ln.weight"], t["v.pre_ln.bias"], eps)[0].astype(f)
    qs = f(1.0) / np.sqrt(f(D))
    for il in range(NL - 1):
        p = f"v.blk.{il}."
        cur = layer_norm_ref(emb, t[p + "ln1.weight"], t[p + "ln1.bias"], eps)[0].astype(f)
        q = proj(cur, p + "attn_q.weight", p + "attn_q.bias", scale=qs)
        k = proj(cur, p + "attn_k.weight", p + "attn_k.bias")
        v = proj(cur, p + "attn_v.weight", p + "attn_v.bias")
        att = attn_ref(q, k, v, T, H, D)[0].astype(f)
        emb = proj(att, p + "attn_out.weight", p + "attn_out.bias", resid=emb)
        cur = layer_norm_ref(emb, t[p + "ln2.weight"], t[p + "ln2.bias"], eps)[0].astype(f)
        ff = proj(cur, p + "ffn_down.weight", p + "ffn_down.bias")          # (the converter's names: "down" is the first projection)
        ff = gelu_out(ff, not use_gelu)
        emb = proj(ff, p + "ffn_up.weight", p + "ffn_up.bias", resid=emb)
    h1 = gelu_out(proj(emb[1:], "mm.0.weight", "mm.0.bias"), False)
    return proj(h1, "mm.2.weight", "mm.2.bias")


def gelu_out(x, quick: bool) -> np.ndarray:
    """the launch's result from its reference: the table entry f16(r), or r itself where the tanh form leaves the table"""
    r, _, exact = gelu_ref(x, quick)
    return np.where(exact, r, f16(r).astype(np.float64)).astype(np.float32)


def read_clip_file(path: str):
    """-> (tensors by name as f32 / f16 arrays in numpy order, metadata) of a projector file"""
    from gguf_read import read_gguf
    kv, raw = read_gguf(path)
    t = {}
    for name, (ne, ty, b) in raw.items():
        dt = np.float32 if ty == 0 else np.float16
        n = int(np.prod(ne))
        t[name] = np.frombuffer(b[:n * dt().itemsize].tobytes(), dt).reshape(ne[::-1])
    return t, kv
