"""IQ4_XS (ggml type 23) restated in numpy, and the llama / qwen3 / qwen3moe reference models with IQ4_XS tensors routed through it.

The CPU oracle under oracle/ has no IQ4_XS, so this module is the reference for the type:

    block (256 weights, 136 bytes): d (f16) | scales_h (u16) | scales_l[4] | qs[128]
    sub-block ib (0..7, 32 weights): ls = ((scales_l[ib / 2] >> 4 (ib % 2)) & 0xf) | (((scales_h >> 2 ib) & 3) << 4)
    weight j of sub-block ib: level = kvalues_iq4nl[qs[16 ib + j] & 0xf] for j < 16, kvalues_iq4nl[qs[16 ib + j - 16] >> 4] for j >= 16
    dequantize_row_iq4_xs: dl = d * (float)(ls - 32) (f32), y = dl * level (f32)
    ggml_vec_dot_iq4_xs_q8_K (activations: Q8_K blocks from the oracle's own quantiser, oq.quantize(Q8_K, x)):
        the pinned integer per (row, super-block): isum = sum over ib of (ls - 32) * sum_j level_j * q8_j
        the generic scalar f32 order: sumf += (d * d8 * (ls - 32)) * sumi, one term per sub-block, in block order, d * d8 first

The reference models: Qwen3Ref / Qwen3MoeRef (tests/qwen3_ref.py, tests/qwen3moe_ref.py) compute every projection through their _mm (and the experts through
moe_ffn) with the oracle's mul_mat, which does not know type 23; the subclasses here send IQ4_XS tensors to mul_mat below and every other type on to the
oracle unchanged.  The token embedding is the one read that does not go through _mm: Qwen3Ref.decode looks rows of token_embd.weight up with oq.row_bytes /
oq.dequantize.  For an IQ4_XS table the constructor therefore replaces that entry of the tensor dict with its F32 dequantisation (dequantize below: the
same bits the device's get_rows gives) and keeps the IQ4_XS bytes aside, so that a tied head (output = token_embd) still contracts with the IQ4_XS table.
On a file without IQ4_XS tensors both models are their parents, bit for bit (tests/test_iq4xs_cpu.py)."""
from __future__ import annotations

import numpy as np

import oracle_py as oq
from qwen3_ref import Qwen3Ref
from qwen3moe_ref import Qwen3MoeRef, route_numpy

IQ4_XS = 23
QK = 256
BLOCK_BYTES = 136
KVALUES = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.int32)
DT = np.dtype([("d", "<f2"), ("scales_h", "<u2"), ("scales_l", "u1", 4), ("qs", "u1", 128)])
DT_Q8K = np.dtype([("d", "<f4"), ("qs", "i1", 256), ("bsums", "<i2", 16)])
assert DT.itemsize == BLOCK_BYTES and DT_Q8K.itemsize == 292


def row_bytes(n: int) -> int:
    assert n % QK == 0, n
    return n // QK * BLOCK_BYTES


def blocks(raw: np.ndarray, n: int) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(raw).view(np.uint8).reshape(-1)[: row_bytes(n)]).view(DT)


def decode(raw: np.ndarray, n: int):
    """-> d (f32 [nb]), ls - 32 (int32 [nb][8]), levels (int32 [nb][256]) of n weights."""
    b = blocks(raw, n)
    d = b["d"].astype(np.float32)
    ib = np.arange(8)
    lo = (b["scales_l"][:, ib // 2].astype(np.int32) >> (4 * (ib % 2))) & 0xF
    hi = (b["scales_h"].astype(np.int32)[:, None] >> (2 * ib)) & 3
    ls = (lo | (hi << 4)) - 32
    qs = b["qs"].astype(np.int32).reshape(-1, 8, 16)
    nib = np.concatenate([qs & 0xF, qs >> 4], axis=2)               # [nb][8][32]: elements j < 16 low nibbles, j >= 16 high ones
    return d, ls.astype(np.int32), KVALUES[nib].reshape(-1, QK)


def dequantize(raw: np.ndarray, n: int) -> np.ndarray:
    d, ls, lev = decode(raw, n)
    dl = (d[:, None] * ls.astype(np.float32)).astype(np.float32)     # [nb][8]
    y = np.repeat(dl, 32, axis=1) * lev.astype(np.float32)
    return y.astype(np.float32).reshape(-1)


def quantize_act(x: np.ndarray) -> np.ndarray:
    """One row of activations as Q8_K blocks (the oracle's quantize_row_q8_K)."""
    return oq.quantize(oq.Q8_K, np.asarray(x, np.float32).reshape(-1))


def vec_dot_int_partials(w_row: np.ndarray, act_q: np.ndarray, n: int) -> np.ndarray:
    """isum per super-block (int64 [nb]) of one row against one Q8_K row."""
    d, ls, lev = decode(w_row, n)
    q8 = np.asarray(act_q).view(np.uint8)[: n // QK * 292].view(DT_Q8K)["qs"].astype(np.int64)
    sub = (lev.astype(np.int64) * q8).reshape(-1, 8, 32).sum(axis=2)    # [nb][8]
    return (sub * ls).sum(axis=1)


def vec_dot(w_row: np.ndarray, act_q: np.ndarray, n: int) -> np.float32:
    """ggml_vec_dot_iq4_xs_q8_K in the generic scalar order."""
    return mul_mat_q8k(w_row, 1, n, np.asarray(act_q).view(np.uint8).reshape(1, -1))[0, 0]


def mul_mat_q8k(W: np.ndarray, N: int, K: int, aq: np.ndarray) -> np.ndarray:
    """W: N IQ4_XS rows of K; aq: [T] Q8_K rows of K (raw bytes, [T][K / 256 * 292]) -> f32 [T][N], the generic f32 order (exact integers per
    sub-block, then one f32 multiply-add per sub-block in block order)."""
    nb = K // QK
    d, ls, lev = decode(W, N * K)
    d = d.reshape(N, nb)
    ls = ls.reshape(N, nb * 8).astype(np.float32)
    lev = lev.reshape(N, nb * 8, 32).astype(np.float64)
    a = np.ascontiguousarray(aq).view(np.uint8).reshape(aq.shape[0], -1)[:, : nb * 292].reshape(-1).view(DT_Q8K).reshape(aq.shape[0], nb)
    d8 = a["d"].astype(np.float32)                                     # [T][nb]
    q8 = a["qs"].astype(np.float64).reshape(aq.shape[0], nb * 8, 32)
    T = aq.shape[0]
    sumf = np.zeros((T, N), np.float32)
    for s in range(nb * 8):
        sumi = (q8[:, s, :] @ lev[:, s, :].T).astype(np.float32)       # exact: |sumi| <= 32 * 127 * 127
        ibl = s // 8
        d4d8 = (d8[:, ibl][:, None] * d[:, ibl][None, :]).astype(np.float32)
        d1 = (d4d8 * ls[:, s][None, :]).astype(np.float32)
        sumf = (sumf + (d1 * sumi).astype(np.float32)).astype(np.float32)
    return sumf


def mul_mat(W: np.ndarray, N: int, K: int, x: np.ndarray) -> np.ndarray:
    """W: N IQ4_XS rows of K (raw bytes); x f32 [T][K] -> f32 [T][N]: activations quantised to Q8_K by the oracle, as ggml's CPU path does."""
    x = np.asarray(x, np.float32).reshape(-1, K)
    aq = np.stack([quantize_act(r) for r in x])
    return mul_mat_q8k(W, N, K, aq)


def _mul(t: int, raw: np.ndarray, N: int, K: int, x: np.ndarray) -> np.ndarray:
    if t == IQ4_XS:
        return mul_mat(raw, N, K, x)
    return oq.mul_mat(t, raw, N, K, x, oq.threads())


def _row_bytes(t: int, n: int) -> int:
    return row_bytes(n) if t == IQ4_XS else oq.row_bytes(t, n)


class _Iq4xsTensors:
    """The routing shared by both models (see the module docstring)."""

    def _iq4xs_init(self):
        self._embd_iq4 = None
        ne, ty, raw = self.t["token_embd.weight"]
        if ty == IQ4_XS:
            self._embd_iq4 = (ne, ty, raw)
            self.t = dict(self.t)
            self.t["token_embd.weight"] = (ne, oq.F32, dequantize(raw, ne[0] * ne[1]).view(np.uint8))

    def _mm(self, name, x):
        if name == "token_embd.weight" and self._embd_iq4 is not None:
            ne, ty, raw = self._embd_iq4
            return mul_mat(raw, ne[1], ne[0], x)
        if name in self.t and self.t[name][1] == IQ4_XS:
            ne, ty, raw = self.t[name]
            return mul_mat(raw, ne[1], ne[0], x)
        return super()._mm(name, x)


class Iq4xsRef(_Iq4xsTensors, Qwen3Ref):
    """Qwen3Ref (llama, qwen2 and qwen3 files) with IQ4_XS tensors."""

    def __init__(self, path: str, n_ctx: int, type_k: int, type_v: int, qk_norm: bool = True):
        super().__init__(path, n_ctx, type_k, type_v, qk_norm)
        self._iq4xs_init()


class Iq4xsMoeRef(_Iq4xsTensors, Qwen3MoeRef):
    """Qwen3MoeRef (qwen3moe and Mixtral-style llama files) with IQ4_XS tensors, the experts included."""

    def __init__(self, path: str, n_ctx: int, type_k: int, type_v: int, qk_norm: bool = True):
        super().__init__(path, n_ctx, type_k, type_v, qk_norm)
        self._iq4xs_init()

    def moe_ffn(self, p: str, h: np.ndarray) -> np.ndarray:
        """Qwen3MoeRef.moe_ffn with each expert's mat-muls through _mul (IQ4_XS here, the oracle for every other type)."""
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
