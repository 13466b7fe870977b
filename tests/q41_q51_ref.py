"""Q4_1 / Q5_1 (ggml types 3 / 7) restated in numpy, and the llama / qwen3 / qwen3moe reference models with such tensors routed through it.

The CPU oracle under oracle/ has neither type, so this module is the reference for both:

    block (32 weights): Q4_1 (20 bytes) d (f16) | m (f16) | qs[16];   Q5_1 (24 bytes) d (f16) | m (f16) | qh[4] | qs[16]
    code q of element j < 16: low nibble of qs[j]; of element j + 16: high nibble of qs[j]; Q5_1: bit j of qh (u32, little endian) is the fifth bit
    q is unsigned (0..15 / 0..31, no offset); weight = q * d + m            (dequantize_row_q4_1 / _q5_1: the product rounded, then the add)
    activations: Q8_0 blocks (d8 f16 | 32 int8 codes a)
    per output and block: isum = sum q a, asum = sum a (both exact integers)

mul_mat - this project's order: a block contributes (d * d8) * (float)isum + m * (d8 * (float)asum), every product and the sum rounded to f32 on its own
(no fused multiply-add), blocks added in order.  d8 is the f16 scale of the Q8_0 block.

mul_mat_ggml - ggml's CPU path (ggml_vec_dot_q4_1_q8_1 / _q5_1_q8_1, generic scalar form): the activation is Q8_1, whose second field is
s = fp16(d_f32 * sum a) with d_f32 the UNROUNDED scale amax / 127, and a block contributes (d * d8) * (float)isum + m * s.  The two second factors differ by
two f16 roundings (of d8 and of s), 2^-11 each: per block |m * d8 * asum - m * s| <= 2^-10 |m * s| to first order (term_bound below).

The reference models: as tests/iq4xs_ref.py - Qwen3Ref / Qwen3MoeRef with the tensors of these two types sent to mul_mat here, every other type to the oracle,
and a token_embd table of either type replaced by its dequantisation (the bits the device's get_rows gives)."""
from __future__ import annotations

import numpy as np

import oracle_py as oq
from qwen3_ref import Qwen3Ref
from qwen3moe_ref import Qwen3MoeRef, route_numpy

Q4_1, Q5_1 = 3, 7
TYPES = (Q4_1, Q5_1)
BLOCK_BYTES = {Q4_1: 20, Q5_1: 24}
DT = {Q4_1: np.dtype([("d", "<f2"), ("m", "<f2"), ("qs", "u1", 16)]),
      Q5_1: np.dtype([("d", "<f2"), ("m", "<f2"), ("qh", "<u4"), ("qs", "u1", 16)])}
DT_Q80 = np.dtype([("d", "<f2"), ("qs", "i1", 32)])
assert DT[Q4_1].itemsize == 20 and DT[Q5_1].itemsize == 24 and DT_Q80.itemsize == 34


def row_bytes(t: int, n: int) -> int:
    assert n % 32 == 0, n
    return n // 32 * BLOCK_BYTES[t]


def blocks(t: int, raw: np.ndarray, n: int) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(raw).view(np.uint8).reshape(-1)[: row_bytes(t, n)]).view(DT[t])


def decode(t: int, raw: np.ndarray, n: int):
    """-> d (f32 [nb]), m (f32 [nb]), q (int32 [nb][32]) of n weights."""
    b = blocks(t, raw, n)
    qs = b["qs"].astype(np.int32)
    q = np.concatenate([qs & 0xF, qs >> 4], axis=1)
    if t == Q5_1:
        q |= ((b["qh"].astype(np.int64)[:, None] >> np.arange(32)) & 1).astype(np.int32) << 4
    return b["d"].astype(np.float32), b["m"].astype(np.float32), q


def dequantize(t: int, raw: np.ndarray, n: int) -> np.ndarray:
    d, m, q = decode(t, raw, n)
    y = (q.astype(np.float32) * d[:, None]).astype(np.float32) + m[:, None]
    return y.astype(np.float32).reshape(-1)


def quantize_act(x: np.ndarray):
    """One row of activations as Q8_0 / Q8_1: -> (codes int8 [nb][32], d8 as stored (f16 -> f32) [nb], the unrounded d_f32 [nb]).
    quantize_row_q8_0_ref / _q8_1_ref: d = amax / 127, id = 1 / d (0 for a zero block), code = roundf(x * id)."""
    x = np.asarray(x, np.float32).reshape(-1, 32)
    amax = np.abs(x).max(axis=1)
    d = (amax / np.float32(127.0)).astype(np.float32)
    with np.errstate(divide="ignore"):
        inv = np.where(d != 0, np.float32(1.0) / d, np.float32(0.0)).astype(np.float32)
    v = (x * inv[:, None]).astype(np.float32)
    q = (np.sign(v) * np.floor(np.abs(v) + np.float32(0.5))).astype(np.int8)          # roundf: halves away from zero
    return q, d.astype(np.float16).astype(np.float32), d


def vec_dot_int_partials(t: int, w_row: np.ndarray, act_codes: np.ndarray, n: int):
    """(isum, asum) per block (int64 [nb] each) of one row against one row of Q8_0 codes ([nb][32])."""
    _, _, q = decode(t, w_row, n)
    a = np.asarray(act_codes).astype(np.int64).reshape(-1, 32)
    return (q.astype(np.int64) * a).sum(axis=1), a.sum(axis=1)


def _mul_mat(t: int, W: np.ndarray, N: int, K: int, x: np.ndarray, ggml: bool):
    nb = K // 32
    d, m, q = decode(t, W, N * K)
    d, m, q = d.reshape(N, nb), m.reshape(N, nb), q.reshape(N, nb, 32).astype(np.float64)
    x = np.asarray(x, np.float32).reshape(-1, K)
    T = x.shape[0]
    acts = [quantize_act(r) for r in x]
    a = np.stack([c for c, _, _ in acts]).astype(np.float64)               # [T][nb][32]
    d8 = np.stack([h for _, h, _ in acts])                                 # [T][nb] f32 (f16 values)
    d32 = np.stack([f for _, _, f in acts])
    asum = a.sum(axis=2).astype(np.float32)                                # exact: |asum| <= 32 * 127
    if ggml:
        s = (d32 * asum).astype(np.float32).astype(np.float16).astype(np.float32)
    else:
        s = (d8 * asum).astype(np.float32)
    out = np.zeros((T, N), np.float32)
    bound = np.zeros((T, N), np.float64)
    for b in range(nb):
        isum = (a[:, b, :] @ q[:, b, :].T).astype(np.float32)              # exact: |isum| <= 32 * 127 * 31
        dd = (d8[:, b][:, None] * d[:, b][None, :]).astype(np.float32)
        ms = (m[:, b][None, :] * s[:, b][:, None]).astype(np.float32)
        term = ((dd * isum).astype(np.float32) + ms).astype(np.float32)
        out = (out + term).astype(np.float32)
        bound += np.abs(ms.astype(np.float64))
    return out, bound


def mul_mat(t: int, W: np.ndarray, N: int, K: int, x: np.ndarray) -> np.ndarray:
    """W: N rows of K of type t (raw bytes); x f32 [T][K] -> f32 [T][N] in this project's order (module docstring)."""
    return _mul_mat(t, W, N, K, x, False)[0]


def mul_mat_ggml(t: int, W: np.ndarray, N: int, K: int, x: np.ndarray) -> np.ndarray:
    """The same with ggml's Q8_1 second factor s = fp16(d_f32 * sum a)."""
    return _mul_mat(t, W, N, K, x, True)[0]


def term_bound(t: int, W: np.ndarray, N: int, K: int, x: np.ndarray) -> np.ndarray:
    """sum over the blocks of |m_b * s_b| per output ([T][N], f64; s as ggml rounds it): times 2^-10 the bound on |mul_mat - mul_mat_ggml|."""
    return _mul_mat(t, W, N, K, x, True)[1]


def _mul(t: int, raw: np.ndarray, N: int, K: int, x: np.ndarray) -> np.ndarray:
    if t in TYPES:
        return mul_mat(t, raw, N, K, x)
    return oq.mul_mat(t, raw, N, K, x, oq.threads())


def _row_bytes(t: int, n: int) -> int:
    return row_bytes(t, n) if t in TYPES else oq.row_bytes(t, n)


class _MinTensors:
    """The routing shared by both models (see the module docstring)."""

    def _min_init(self):
        self._embd_min = None
        ne, ty, raw = self.t["token_embd.weight"]
        if ty in TYPES:
            self._embd_min = (ne, ty, raw)
            self.t = dict(self.t)
            self.t["token_embd.weight"] = (ne, oq.F32, dequantize(ty, raw, ne[0] * ne[1]).view(np.uint8))

    def _mm(self, name, x):
        if name == "token_embd.weight" and self._embd_min is not None:
            ne, ty, raw = self._embd_min
            return mul_mat(ty, raw, ne[1], ne[0], x)
        if name in self.t and self.t[name][1] in TYPES:
            ne, ty, raw = self.t[name]
            return mul_mat(ty, raw, ne[1], ne[0], x)
        return super()._mm(name, x)


class MinRef(_MinTensors, Qwen3Ref):
    """Qwen3Ref (llama, qwen2 and qwen3 files) with Q4_1 / Q5_1 tensors."""

    def __init__(self, path: str, n_ctx: int, type_k: int, type_v: int, qk_norm: bool = True):
        super().__init__(path, n_ctx, type_k, type_v, qk_norm)
        self._min_init()


class MinMoeRef(_MinTensors, Qwen3MoeRef):
    """Qwen3MoeRef (qwen3moe and Mixtral-style llama files) with Q4_1 / Q5_1 tensors, the experts included."""

    def __init__(self, path: str, n_ctx: int, type_k: int, type_v: int, qk_norm: bool = True):
        super().__init__(path, n_ctx, type_k, type_v, qk_norm)
        self._min_init()

    def moe_ffn(self, p: str, h: np.ndarray) -> np.ndarray:
        """Qwen3MoeRef.moe_ffn with each expert's mat-muls through _mul (the two types here, the oracle for every other one)."""
        gi_ne, gi_t, gi_raw = self.t[p + "ffn_gate_inp.weight"]
        g_ne, g_t, g_raw = self.t[p + "ffn_gate_exps.weight"]
        u_ne, u_t, u_raw = self.t[p + "ffn_up_exps.weight"]
        d_ne, d_t, d_raw = self.t[p + "ffn_down_exps.weight"]
        E, F = g_ne[0], g_ne[1]
        gb, ub, db = _row_bytes(g_t, E) * F, _row_bytes(u_t, E) * F, _row_bytes(d_t, F) * E
        out = np.zeros((h.shape[0], E), np.float32)
        sel = np.zeros((h.shape[0], self.k), np.int32)
        for t in range(h.shape[0]):
            logits = oq.mul_mat(gi_t, gi_raw, gi_ne[1], gi_ne[0], h[t:t + 1], oq.threads())[0]
            ids, w = route_numpy(logits, self.k)
            sel[t] = ids
            o = None
            for j, e in enumerate(ids):
                e = int(e)
                g = _mul(g_t, g_raw[e * gb:(e + 1) * gb], F, E, h[t:t + 1])[0]
                u = _mul(u_t, u_raw[e * ub:(e + 1) * ub], F, E, h[t:t + 1])[0]
                a = (oq.silu(g) * u).astype(np.float32)
                y = _mul(d_t, d_raw[e * db:(e + 1) * db], E, F, a[None, :])[0]
                v = (y * w[j]).astype(np.float32)
                o = v if o is None else (o + v).astype(np.float32)
            out[t] = o
        self._layer_routes.append(sel)
        return out
