"""MXFP4 (ggml type 39) restated in numpy, and the llama / qwen3 / qwen3moe reference models with such tensors routed through it.

The CPU oracle under oracle/ does not have the type, so this module is the reference:

    block (32 weights, 17 bytes): e (u8, E8M0) | qs[16]
    level index of element j < 16: low nibble of qs[j]; of element j + 16: high nibble of qs[j]
    level = KVALUES[index] = {0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12}        (the e2m1 values doubled)
    d = half of 2^(e - 127), as an f32 bit pattern: 0x00200000 << e for e < 2, else (e - 1) << 23; e = 255 gives 2^127 (no NaN case)
    weight = (float)level * d                                                                  (dequantize_row_mxfp4: one product)
    activations: Q8_0 blocks (d8 f16 | 32 int8 codes a)
    per output and block: isum = sum level * a (an exact integer, |isum| <= 32 * 12 * 127)

mul_mat - ggml's order (ggml_vec_dot_mxfp4_q8_0, scalar form) and the device's matrix-core prompt kernel's: sumf += (d8 * d) * (float)isum, every product and
the sum rounded to f32 on its own, blocks in order.  The device's mat-vec kernels (one to 31 tokens) form the same per-block terms and add them across lanes
in a tree: within f32 round-off of this chain (TIGHT_TOL of the output scale in the tests), not bit for bit.

The reference models: as tests/q41_q51_ref.py - Qwen3Ref / Qwen3MoeRef with the MXFP4 tensors sent to mul_mat here, every other type to the oracle, and a
token_embd table of the type replaced by its dequantisation (the bits the device's get_rows gives)."""
from __future__ import annotations

import numpy as np

import oracle_py as oq
from q41_q51_ref import quantize_act
from qwen3_ref import Qwen3Ref
from qwen3moe_ref import Qwen3MoeRef, route_numpy

MXFP4 = 39
FTYPE_MXFP4_MOE = 38
BLOCK_BYTES = 17
DT = np.dtype([("e", "u1"), ("qs", "u1", 16)])
assert DT.itemsize == BLOCK_BYTES
KVALUES = np.array([0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12], np.int32)


def row_bytes(n: int) -> int:
    assert n % 32 == 0, n
    return n // 32 * BLOCK_BYTES


def scale(e) -> np.ndarray:
    """The f32 block scale of E8M0 byte(s) e, from the bit pattern."""
    e = np.asarray(e).astype(np.uint32)
    bits = np.where(e < 2, np.uint32(0x00200000) << e, (np.maximum(e, 1) - np.uint32(1)) << np.uint32(23))
    return np.ascontiguousarray(bits.astype("<u4")).view(np.float32)


def blocks(raw: np.ndarray, n: int) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(raw).view(np.uint8).reshape(-1)[: row_bytes(n)]).view(DT)


def decode(raw: np.ndarray, n: int):
    """-> d (f32 [nb]), level (int32 [nb][32]) of n weights."""
    b = blocks(raw, n)
    qs = b["qs"].astype(np.int32)
    return scale(b["e"]), KVALUES[np.concatenate([qs & 0xF, qs >> 4], axis=1)]


def dequantize(raw: np.ndarray, n: int) -> np.ndarray:
    d, lv = decode(raw, n)
    with np.errstate(over="ignore"):
        return (lv.astype(np.float32) * d[:, None]).astype(np.float32).reshape(-1)


def make_blocks(e: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """Raw blocks from scale bytes e [nb] and level indices idx [nb][32] (0..15)."""
    idx = np.asarray(idx, np.uint8).reshape(-1, 32)
    b = np.zeros(idx.shape[0], DT)
    b["e"] = np.asarray(e, np.uint8).reshape(-1)
    b["qs"] = (idx[:, :16] & 15) | ((idx[:, 16:] & 15) << 4)
    return b.view(np.uint8).reshape(-1)


def vec_dot_int_partials(w_row: np.ndarray, act_codes: np.ndarray, n: int) -> np.ndarray:
    """isum per block (int64 [nb]) of one row against one row of Q8_0 codes ([nb][32])."""
    _, lv = decode(w_row, n)
    return (lv.astype(np.int64) * np.asarray(act_codes).astype(np.int64).reshape(-1, 32)).sum(axis=1)


def mul_mat(W: np.ndarray, N: int, K: int, x: np.ndarray) -> np.ndarray:
    """W: N rows of K MXFP4 weights (raw bytes); x f32 [T][K] -> f32 [T][N], each output's chain in block order (module docstring)."""
    nb = K // 32
    d, lv = decode(W, N * K)
    d, lv = d.reshape(N, nb), lv.reshape(N, nb, 32).astype(np.float64)
    x = np.asarray(x, np.float32).reshape(-1, K)
    acts = [quantize_act(r) for r in x]
    a = np.stack([c for c, _, _ in acts]).astype(np.float64)               # [T][nb][32]
    d8 = np.stack([h for _, h, _ in acts])                                 # [T][nb] f32 (f16 values)
    out = np.zeros((x.shape[0], N), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(nb):
            isum = (a[:, b, :] @ lv[:, b, :].T).astype(np.float32)         # exact
            dd = (d8[:, b][:, None] * d[:, b][None, :]).astype(np.float32)
            out = (out + (dd * isum).astype(np.float32)).astype(np.float32)
    return out


def mul_mat_f64(W: np.ndarray, N: int, K: int, x: np.ndarray) -> np.ndarray:
    """The same contraction of the same quantised activations in float64 (no f32 rounding of products or sums)."""
    nb = K // 32
    d, lv = decode(W, N * K)
    x = np.asarray(x, np.float32).reshape(-1, K)
    acts = [quantize_act(r) for r in x]
    a = np.stack([c for c, _, _ in acts]).astype(np.float64) * np.stack([h for _, h, _ in acts]).astype(np.float64)[:, :, None]
    w = lv.reshape(N, nb, 32).astype(np.float64) * d.reshape(N, nb).astype(np.float64)[:, :, None]
    return np.einsum("tbk,nbk->tn", a, w)


def _mul(t: int, raw: np.ndarray, N: int, K: int, x: np.ndarray) -> np.ndarray:
    if t == MXFP4:
        return mul_mat(raw, N, K, x)
    return oq.mul_mat(t, raw, N, K, x, oq.threads())


def _row_bytes(t: int, n: int) -> int:
    return row_bytes(n) if t == MXFP4 else oq.row_bytes(t, n)


class _Mxfp4Tensors:
    """The routing shared by both models (see the module docstring)."""

    def _mx_init(self):
        self._embd_mx = None
        ne, ty, raw = self.t["token_embd.weight"]
        if ty == MXFP4:
            self._embd_mx = (ne, ty, raw)
            self.t = dict(self.t)
            self.t["token_embd.weight"] = (ne, oq.F32, dequantize(raw, ne[0] * ne[1]).view(np.uint8))

    def _mm(self, name, x):
        if name == "token_embd.weight" and self._embd_mx is not None:
            ne, _, raw = self._embd_mx
            return mul_mat(raw, ne[1], ne[0], x)
        if name in self.t and self.t[name][1] == MXFP4:
            ne, _, raw = self.t[name]
            return mul_mat(raw, ne[1], ne[0], x)
        return super()._mm(name, x)


class Mxfp4Ref(_Mxfp4Tensors, Qwen3Ref):
    """Qwen3Ref (llama, qwen2 and qwen3 files) with MXFP4 tensors."""

    def __init__(self, path: str, n_ctx: int, type_k: int, type_v: int, qk_norm: bool = True):
        super().__init__(path, n_ctx, type_k, type_v, qk_norm)
        self._mx_init()


class Mxfp4MoeRef(_Mxfp4Tensors, Qwen3MoeRef):
    """Qwen3MoeRef (qwen3moe and Mixtral-style llama files) with MXFP4 expert tensors (an MXFP4_MOE file) or MXFP4 everywhere."""

    def __init__(self, path: str, n_ctx: int, type_k: int, type_v: int, qk_norm: bool = True):
        super().__init__(path, n_ctx, type_k, type_v, qk_norm)
        self._mx_init()

    def moe_ffn(self, p: str, h: np.ndarray) -> np.ndarray:
        """Qwen3MoeRef.moe_ffn with each expert's mat-muls through _mul (MXFP4 here, the oracle for every other type)."""
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
