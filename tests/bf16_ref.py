"""BF16 (ggml type 30) restated in numpy, and the llama / qwen2 / qwen3 reference model with BF16 tensors routed through it.

The CPU oracle under oracle/ has no BF16, and the algorithm's home (llama.cpp) is absent from the reference mount, so this module is the
reference for the type.  Parity with ggml is therefore unpinned in the same sense as §2: what is restated below is ggml's CPU arithmetic as its source
states it, checked against the oracle only where the oracle can speak (tests/test_bf16_cpu.py: the same exact products through its F32 mul_mat).

    a bf16 value is the upper 16 bits of an f32: widening is bits << 16, exact for every pattern (subnormals, infinities, NaNs included)
    f32 -> bf16 (ggml_compute_fp32_to_bf16): nearest, ties to even, on the bits: (u + 0x7fff + ((u >> 16) & 1)) >> 16; a NaN keeps its upper bits and gets
        the quiet bit ((u >> 16) | 64); subnormals are kept, not flushed
    ggml_mul_mat with a BF16 src0: vec_dot_type is BF16 - every activation row is rounded to bf16, every product bf16 x bf16 is exact in f32, and the scalar
        ggml_vec_dot_bf16 sums the products in double in element order and rounds once:  y = float32(sum_k float64(w_k) * float64(bf16(x_k)))
    get_rows on a BF16 table returns the exact widening

The reference model: Qwen3Ref (tests/qwen3_ref.py, which serves llama, qwen2 and qwen3 files) computes every projection through its _mm with the oracle's
mul_mat; the mixin here sends BF16 tensors to mul_mat below and every other type on to the oracle unchanged, the way _Iq4xsTensors does for IQ4_XS.  The token
embedding is looked up with oq.row_bytes / oq.dequantize, so a BF16 table is replaced by its exact F32 widening in the tensor dict and the BF16 bits are
kept aside for a tied head."""
from __future__ import annotations

import numpy as np

import oracle_py as oq
from qwen3_ref import Qwen3Ref

BF16 = 30


def round_bf16(x) -> np.ndarray:
    """f32 values -> bf16 bits (uint16), ggml_compute_fp32_to_bf16."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 64, r).astype(np.uint16)


def widen(bits) -> np.ndarray:
    """bf16 bits -> f32, exact."""
    return (np.ascontiguousarray(bits).view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def bits_of(raw, n: int) -> np.ndarray:
    """the first n bf16 values of a raw tensor (bytes or uint16) as uint16."""
    return np.ascontiguousarray(np.asarray(raw).view(np.uint8).reshape(-1)[: 2 * n]).view("<u2")


def mul_mat(W, N: int, K: int, x) -> np.ndarray:
    """W: N x K bf16 (raw bytes or uint16 bits); x [T][K] f32 -> y [T][N] f32 = float32(sum_k float64(w) * float64(bf16(x)))."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, K)
    xb = widen(round_bf16(x)).astype(np.float64)
    w = bits_of(W, N * K).reshape(N, K)
    y = np.empty((x.shape[0], N), np.float32)
    for n0 in range(0, N, 2048):                                       # (bounds the f64 copy of W)
        y[:, n0:n0 + 2048] = (xb @ widen(w[n0:n0 + 2048]).astype(np.float64).T).astype(np.float32)
    return y


def get_rows(table, K: int, ids) -> np.ndarray:
    b = bits_of(table, np.asarray(table).view(np.uint8).size // 2).reshape(-1, K)
    return widen(b[np.asarray(ids, np.int64)])


class _Bf16Tensors:
    """BF16 tensors through mul_mat above, everything else through the parent's _mm (see the module docstring)."""

    def _bf16_init(self):
        self._embd_bf16 = None
        ne, ty, raw = self.t["token_embd.weight"]
        if ty == BF16:
            self._embd_bf16 = (ne, ty, raw)
            self.t = dict(self.t)
            self.t["token_embd.weight"] = (ne, oq.F32, widen(bits_of(raw, ne[0] * ne[1])).view(np.uint8))

    def _mm(self, name, x):
        if name == "token_embd.weight" and self._embd_bf16 is not None:
            ne, ty, raw = self._embd_bf16
            return mul_mat(raw, ne[1], ne[0], x)
        if name in self.t and self.t[name][1] == BF16:
            ne, ty, raw = self.t[name]
            return mul_mat(raw, ne[1], ne[0], x)
        return super()._mm(name, x)


class Bf16Ref(_Bf16Tensors, Qwen3Ref):
    """Qwen3Ref (llama, qwen2 and qwen3 files) with BF16 tensors."""

    def __init__(self, path: str, n_ctx: int, type_k: int, type_v: int, qk_norm: bool = True):
        super().__init__(path, n_ctx, type_k, type_v, qk_norm)
        self._bf16_init()
