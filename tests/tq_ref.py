"""TQ1_0 / TQ2_0 (ggml types 34 / 35, the ternary formats) restated in numpy, and the llama / qwen3 / qwen3moe reference models with ternary tensors routed
through it.

The CPU oracle under oracle/ has neither type, so this module is the reference for them.  Restated from upstream's generic-scalar code as remembered: its
source is not available where this was written, so the layouts are unpinned in the same sense as every other type restated under tests/.

    both: 256 weights per block, codes q in 0..2, weight = (q - 1) * d, one f16 d per block, activations in Q8_K
    TQ2_0 (66 bytes): qs[64] | d.   element 128 h + 32 l + m = (qs[32 h + m] >> 2 l) & 3      (h 0..1, l 0..3, m 0..31; a code of 3 is weight + 2 d)
    TQ1_0 (54 bytes): qs[48] | qh[4] | d.   trit n of byte b = ((uint8)(b * 3^n) * 3) >> 8 - defined, and in 0..2, for every byte value
        elements 32 n + m        from qs[m]        (n 0..4, m 0..31)
        elements 160 + 16 n + m  from qs[32 + m]   (n 0..4, m 0..15)
        elements 240 + 4 n + j   from qh[j]        (n 0..3, j 0..3)
    dequantize_row_tq*_0: y = (float)(q - 1) * d - a product, so a zero weight under a negative d is - 0.0
    quantize_row_tq*_0_ref: d = max |x|, id = d ? 1 / d : 0, xi = lroundf(x * id) + 1; TQ1_0 accumulates a byte's trits most significant first
        (q = q * 3 + xi), multiplies a qh byte's four by 3 once more and stores (q * 256 + 242) / 243; TQ2_0 stores q |= (xi & 3) << 2 n
    ggml_vec_dot_tq*_0_q8_K (activations: Q8_K blocks from the oracle's own quantiser): per super-block sumi = sum (q - 1) * a over its 256 elements - the
        pinned integer, |sumi| <= 256 * 127 - and sumf += (float)sumi * (d_x * d_y), one term per super-block, in block order

The reference models: as tests/iq4xs_ref.py - TqRef / TqMoeRef send ternary tensors to mul_mat below and every other type on to the oracle unchanged.  The
writer's ternary mixes keep token_embd in Q4_K, so the embedding look-up needs nothing here; a file whose token_embd is ternary all the same is handled as
IQ4_XS's is (the table replaced by its F32 dequantisation, the ternary bytes kept for a tied head).  On a file without ternary tensors both models are their
parents, bit for bit (tests/test_tq_cpu.py)."""
from __future__ import annotations

import numpy as np

import oracle_py as oq
from qwen3_ref import Qwen3Ref
from qwen3moe_ref import Qwen3MoeRef, route_numpy

TQ1_0, TQ2_0 = 34, 35
TYPES = (TQ1_0, TQ2_0)
QK = 256
BLOCK_BYTES = {TQ1_0: 54, TQ2_0: 66}
POW3 = np.array([1, 3, 9, 27, 81], np.uint32)
DT = {TQ1_0: np.dtype([("qs", "u1", 48), ("qh", "u1", 4), ("d", "<f2")]), TQ2_0: np.dtype([("qs", "u1", 64), ("d", "<f2")])}
DT_Q8K = np.dtype([("d", "<f4"), ("qs", "i1", 256), ("bsums", "<i2", 16)])
assert DT[TQ1_0].itemsize == 54 and DT[TQ2_0].itemsize == 66 and DT_Q8K.itemsize == 292


def row_bytes(t: int, n: int) -> int:
    assert n % QK == 0, n
    return n // QK * BLOCK_BYTES[t]


def blocks(t: int, raw: np.ndarray, n: int) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(raw).view(np.uint8).reshape(-1)[: row_bytes(t, n)]).view(DT[t])


def tq1_element_map():
    """(byte, n) per element of a TQ1_0 block, written out region by region: byte indexes qs (0..47) then qh (48..51), n is the trit position."""
    byte, n = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for k in range(5):
        for m in range(32):
            byte[32 * k + m], n[32 * k + m] = m, k
        for m in range(16):
            byte[160 + 16 * k + m], n[160 + 16 * k + m] = 32 + m, k
    for k in range(4):
        for j in range(4):
            byte[240 + 4 * k + j], n[240 + 4 * k + j] = 48 + j, k
    return byte, n


def trit(b, n):
    """Trit n of byte value(s) b by the format's formula: the product wraps to 8 bits before the * 3."""
    b = np.asarray(b).astype(np.uint32)
    return (((b * POW3[n]) & 0xFF) * 3) >> 8


def decode(t: int, raw: np.ndarray, n: int):
    """-> d (f32 [nb]), codes q (int32 [nb][256], 0..2; TQ2_0 also 3) of n weights."""
    b = blocks(t, raw, n)
    d = b["d"].astype(np.float32)
    if t == TQ2_0:
        qs = b["qs"].astype(np.int32).reshape(-1, 2, 32)                       # [nb][h][m]
        q = np.stack([(qs >> (2 * l)) & 3 for l in range(4)], axis=2)          # [nb][h][l][m]
        return d, q.reshape(-1, QK).astype(np.int32)
    byte, pos = tq1_element_map()
    lut = np.stack([trit(np.arange(256), k) for k in range(5)], axis=1).astype(np.uint8)      # [byte value][n]: the formula, tabulated
    by = np.concatenate([b["qs"], b["qh"]], axis=1)                                            # [nb][52]
    return d, lut[by].reshape(-1, 52 * 5)[:, byte * 5 + pos].astype(np.int32)


def dequantize(t: int, raw: np.ndarray, n: int) -> np.ndarray:
    d, q = decode(t, raw, n)
    return ((q - 1).astype(np.float32) * d[:, None]).astype(np.float32).reshape(-1)


def pack(t: int, codes: np.ndarray, d) -> np.ndarray:
    """Blocks (raw bytes) holding codes [nb][256] and scales d [nb], packed as the reference quantisers pack."""
    codes = np.asarray(codes).astype(np.uint32).reshape(-1, QK)
    b = np.zeros(codes.shape[0], DT[t])
    b["d"] = np.asarray(d, np.float32).astype("<f2")
    if t == TQ2_0:
        for h in range(2):
            for m in range(32):
                v = 0
                for l in range(4):
                    v = v | ((codes[:, 128 * h + 32 * l + m] & 3) << (2 * l))
                b["qs"][:, 32 * h + m] = v
        return b.view(np.uint8).reshape(-1)
    assert codes.max(initial=0) <= 2
    byte, pos = tq1_element_map()
    for j in range(52):
        q = np.zeros(codes.shape[0], np.uint32)
        nt = 5 if j < 48 else 4
        for k in range(nt):
            e = int(np.flatnonzero((byte == j) & (pos == k))[0])
            q = q * 3 + codes[:, e]
        if nt == 4:
            q = q * 3
        v = ((q * 256 + 242) // 243).astype(np.uint8)
        if j < 48:
            b["qs"][:, j] = v
        else:
            b["qh"][:, j - 48] = v
    return b.view(np.uint8).reshape(-1)


def quantize(t: int, x: np.ndarray) -> np.ndarray:
    """quantize_row_tq1_0_ref / quantize_row_tq2_0_ref."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, QK)
    d = np.abs(x).max(axis=1).astype(np.float32)
    with np.errstate(divide="ignore"):
        inv = np.where(d != 0, np.float32(1.0) / d, np.float32(0.0)).astype(np.float32)
    v = (x * inv[:, None]).astype(np.float32)
    xi = (np.sign(v) * np.floor(np.abs(v) + np.float32(0.5))).astype(np.int64) + 1      # lroundf: halves away from zero
    return pack(t, xi & 3, d)


def quantize_act(x: np.ndarray) -> np.ndarray:
    """One row of activations as Q8_K blocks (the oracle's quantize_row_q8_K)."""
    return oq.quantize(oq.Q8_K, np.asarray(x, np.float32).reshape(-1))


def vec_dot_int_partials(t: int, w_row: np.ndarray, act_q: np.ndarray, n: int) -> np.ndarray:
    """sumi per super-block (int64 [nb]) of one row against one Q8_K row."""
    d, q = decode(t, w_row, n)
    q8 = np.asarray(act_q).view(np.uint8)[: n // QK * 292].view(DT_Q8K)["qs"].astype(np.int64)
    return ((q.astype(np.int64) - 1) * q8).sum(axis=1)


def vec_dot(t: int, w_row: np.ndarray, act_q: np.ndarray, n: int) -> np.float32:
    """ggml_vec_dot_tq*_0_q8_K in the generic scalar order."""
    return mul_mat_q8k(t, w_row, 1, n, np.asarray(act_q).view(np.uint8).reshape(1, -1))[0, 0]


def levels(t: int, W: np.ndarray, N: int, K: int):
    """A tensor decoded once: d (f32 [N][nb]) and q - 1 (int8 [N][nb][256]) - what mul_mat_q8k contracts with (the models below keep it per tensor)."""
    d, q = decode(t, W, N * K)
    return d.reshape(N, K // QK), (q - 1).astype(np.int8).reshape(N, K // QK, QK)


def mul_mat_q8k(t: int, W: np.ndarray, N: int, K: int, aq: np.ndarray, dec=None) -> np.ndarray:
    """W: N rows of K of type t; aq: [T] Q8_K rows of K (raw bytes) -> f32 [T][N] in the generic order: the exact integer per super-block, then
    sumf += (float)sumi * (d_x * d_y) in block order.  (The integers are summed in f32: every partial sum is an integer below 256 * 127 * 2 < 2^24, exact.)"""
    nb = K // QK
    d, lev = dec if dec is not None else levels(t, W, N, K)
    T = aq.shape[0]
    a = np.ascontiguousarray(aq).view(np.uint8).reshape(T, -1)[:, : nb * 292].reshape(-1).view(DT_Q8K).reshape(T, nb)
    d8 = a["d"].astype(np.float32)
    q8 = a["qs"].astype(np.float32)                                        # [T][nb][256]
    sumf = np.zeros((T, N), np.float32)
    for s in range(nb):
        sumi = q8[:, s, :] @ lev[:, s, :].astype(np.float32).T
        dd = (d[:, s][None, :] * d8[:, s][:, None]).astype(np.float32)
        sumf = (sumf + (sumi * dd).astype(np.float32)).astype(np.float32)
    return sumf


def mul_mat(t: int, W: np.ndarray, N: int, K: int, x: np.ndarray, dec=None) -> np.ndarray:
    """x f32 [T][K] -> f32 [T][N]: activations quantised to Q8_K by the oracle, as ggml's CPU path does."""
    x = np.asarray(x, np.float32).reshape(-1, K)
    aq = np.stack([quantize_act(r) for r in x])
    return mul_mat_q8k(t, W, N, K, aq, dec)


def _mul(t: int, raw: np.ndarray, N: int, K: int, x: np.ndarray, dec=None) -> np.ndarray:
    if t in TYPES:
        return mul_mat(t, raw, N, K, x, dec)
    return oq.mul_mat(t, raw, N, K, x, oq.threads())


def _row_bytes(t: int, n: int) -> int:
    return row_bytes(t, n) if t in TYPES else oq.row_bytes(t, n)


class _TqTensors:
    """The routing shared by both models (see the module docstring)."""

    def _tq_init(self):
        self._embd_tq = None
        self._dec = {}                                     # name (or (name, expert)) -> levels(): a tensor is decoded once, not once per step
        ne, ty, raw = self.t["token_embd.weight"]
        if ty in TYPES:
            self._embd_tq = (ne, ty, raw)
            self.t = dict(self.t)
            self.t["token_embd.weight"] = (ne, oq.F32, dequantize(ty, raw, ne[0] * ne[1]).view(np.uint8))

    def _levels(self, key, ty, raw, N, K):
        if ty not in TYPES:
            return None
        if key not in self._dec:
            self._dec[key] = levels(ty, raw, N, K)
        return self._dec[key]

    def _mm(self, name, x):
        if name == "token_embd.weight" and self._embd_tq is not None:
            ne, ty, raw = self._embd_tq
            return mul_mat(ty, raw, ne[1], ne[0], x, self._levels(name, ty, raw, ne[1], ne[0]))
        if name in self.t and self.t[name][1] in TYPES:
            ne, ty, raw = self.t[name]
            return mul_mat(ty, raw, ne[1], ne[0], x, self._levels(name, ty, raw, ne[1], ne[0]))
        return super()._mm(name, x)


class TqRef(_TqTensors, Qwen3Ref):
    """Qwen3Ref (llama, qwen2 and qwen3 files) with ternary tensors."""

    def __init__(self, path: str, n_ctx: int, type_k: int, type_v: int, qk_norm: bool = True):
        super().__init__(path, n_ctx, type_k, type_v, qk_norm)
        self._tq_init()


class TqMoeRef(_TqTensors, Qwen3MoeRef):
    """Qwen3MoeRef (qwen3moe and Mixtral-style llama files) with ternary tensors, the experts included."""

    def __init__(self, path: str, n_ctx: int, type_k: int, type_v: int, qk_norm: bool = True):
        super().__init__(path, n_ctx, type_k, type_v, qk_norm)
        self._tq_init()

    def moe_ffn(self, p: str, h: np.ndarray) -> np.ndarray:
        """Qwen3MoeRef.moe_ffn with each expert's mat-muls through _mul (the ternary types here, the oracle for every other type)."""
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
                gw, uw, dw = g_raw[e * gb:(e + 1) * gb], u_raw[e * ub:(e + 1) * ub], d_raw[e * db:(e + 1) * db]
                g = _mul(g_t, gw, F, E, h[t:t + 1], self._levels((p, "g", e), g_t, gw, F, E))[0]
                u = _mul(u_t, uw, F, E, h[t:t + 1], self._levels((p, "u", e), u_t, uw, F, E))[0]
                a = (oq.silu(g) * u).astype(np.float32)
                y = _mul(d_t, dw, E, F, a[None, :], self._levels((p, "d", e), d_t, dw, E, F))[0]
                v = (y * w[j]).astype(np.float32)
                o = v if o is None else (o + v).astype(np.float32)
            out[t] = o
        self._layer_routes.append(sel)
        return out
