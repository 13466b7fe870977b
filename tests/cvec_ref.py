"""Control vectors on the CPU, for tests/test_cvec_cpu.py and tests/test_gpu_cvec.py.

CvecRef / CvecMoeRef: the forward pass of tests/qwen3_ref.py (and its routed form, tests/qwen3moe_ref.py) with an applied vector.  `decode` restates
Qwen3Ref.decode's loop op for op - every op the oracle's, composed as there - with one line more: after the layer's second residual add, where layer il has a
vector inside the range,

    x = (x + v_il).astype(float32)

for all rows of the batch, before the tap is taken.  Nothing under oracle/ knows about vectors.

The power method's numpy twins (f32, two summation orders) and its float64 yardstick (numpy.linalg.eigh) for the generator's kernels."""
from __future__ import annotations

import numpy as np

import oracle_py as oq
from qwen3_ref import Qwen3Ref
from qwen3moe_ref import Qwen3MoeRef


class CvecRef(Qwen3Ref):
    cvec = None            # f32 [n][E]: the vectors of layers 1 .. n
    il_start, il_end = 1, -1

    def apply_cvec(self, data, il_start: int, il_end: int):
        """llama_apply_adapter_cvec: data [n][E] (or flat) holds layers 1 .. n; None clears."""
        self.cvec = None if data is None else np.ascontiguousarray(data, np.float32).reshape(-1, self.E)
        self.il_start, self.il_end = il_start, il_end

    def _vec(self, il: int):
        if self.cvec is None or il < 1 or il > self.cvec.shape[0] or not (self.il_start <= il <= self.il_end):
            return None
        return self.cvec[il - 1]

    def decode(self, tokens, pos, seq=None, want=None) -> np.ndarray:
        tokens = np.asarray(tokens).reshape(-1)
        pos = np.asarray(pos).reshape(-1)
        seq = np.zeros(tokens.size, np.int64) if seq is None else np.asarray(seq).reshape(-1)
        n, E, H, G, D = tokens.size, self.E, self.H, self.G, self.D
        free = np.nonzero(self.cell_pos < 0)[0]
        assert free.size >= n, "reference cache full"
        cells = free[:n]
        self.cell_pos[cells] = pos
        self.cell_seq[cells] = seq
        ne, ty, raw = self.t["token_embd.weight"]
        rb = oq.row_bytes(ty, E)
        x = np.stack([oq.dequantize(ty, raw[int(tk) * rb:(int(tk) + 1) * rb], E) for tk in tokens]).astype(np.float32)
        scale = np.float32(1.0 / np.sqrt(D))
        self.taps = []
        for il in range(self.n_layer):
            p = f"blk.{il}."
            h = self._norm_rows(x, self._f32(p + "attn_norm.weight"))
            q, k, v = self._mm(p + "attn_q.weight", h), self._mm(p + "attn_k.weight", h), self._mm(p + "attn_v.weight", h)
            for b, y in (("attn_q.bias", q), ("attn_k.bias", k), ("attn_v.bias", v)):
                if p + b in self.t:
                    y += self._f32(p + b)
            for i in range(n):
                qi, ki = q[i], k[i]
                if self.qk_norm:
                    qi = self._head_norm(qi, H, self._f32(p + "attn_q_norm.weight"))
                    ki = self._head_norm(ki, G, self._f32(p + "attn_k_norm.weight"))
                q[i] = oq.rope(qi, H, D, int(pos[i]), self.base, neox=self.neox).reshape(-1)
                kr = oq.rope(ki, G, D, int(pos[i]), self.base, neox=self.neox).reshape(-1)
                self.kc[il, cells[i]] = oq.quantize(self.tk, kr)
                self.vc[il, cells[i]] = oq.quantize(self.tv, v[i])
            att = np.empty((n, H * D), np.float32)
            for i in range(n):
                vis = np.nonzero((self.cell_pos >= 0) & (self.cell_pos <= pos[i]) & (self.cell_seq == seq[i]))[0].astype(np.int32)
                att[i] = oq.flash_attn(q[i], H, G, D, self.tk, self.kc[il], self.tv, self.vc[il], vis, scale).reshape(-1)
            x = x + self._mm(p + "attn_output.weight", att)
            h = self._norm_rows(x, self._f32(p + "ffn_norm.weight"))
            g, u = self._mm(p + "ffn_gate.weight", h), self._mm(p + "ffn_up.weight", h)
            x = x + self._mm(p + "ffn_down.weight", oq.silu(g) * u)
            vec = self._vec(il)
            if vec is not None:
                x = (x + vec).astype(np.float32)
            self.taps.append(x.copy())
        rows = np.nonzero(np.asarray(want).reshape(-1))[0] if want is not None else [n - 1]
        h = self._norm_rows(x[rows], self._f32("output_norm.weight"))
        return self._mm("output.weight" if "output.weight" in self.t else "token_embd.weight", h)


class CvecMoeRef(Qwen3MoeRef, CvecRef):
    """Qwen3MoeRef.decode (the route bookkeeping) runs CvecRef.decode as its super(); the feed-forward calls reach Qwen3MoeRef._mm."""


# ------------------------------------------------------------------------------------------------ the power method
def _sum_serial(a: np.ndarray, axis: int) -> np.ndarray:
    """f32 sum along `axis`, element after element (numpy's accumulate is serial)."""
    return np.take(np.add.accumulate(a, axis=axis, dtype=np.float32), -1, axis=axis)


def _sum_pairwise(a: np.ndarray, axis: int) -> np.ndarray:
    """f32 sum along `axis` as a balanced tree: padded with zeros to a power of two, halves added until one is left."""
    a = np.moveaxis(np.asarray(a, np.float32), axis, -1)
    n = 1 << max(0, int(a.shape[-1] - 1).bit_length())
    if n != a.shape[-1]:
        a = np.concatenate([a, np.zeros(a.shape[:-1] + (n - a.shape[-1],), np.float32)], axis=-1)
    while a.shape[-1] > 1:
        h = a.shape[-1] // 2
        a = (a[..., :h] + a[..., h:]).astype(np.float32)
    return a[..., 0]


SUMS = {"serial": _sum_serial, "pairwise": _sum_pairwise}


def pca_twin(D: np.ndarray, b0: np.ndarray, n_iter: int, order: str = "serial"):
    """n_iter iterations of b <- D^T (D b) / |D^T (D b)| in f32 (products rounded, then summed in `order`), then the sign that makes sum_r D[r] . b >= 0.
    Returns (b, the last |b_new - b_old|)."""
    D = np.ascontiguousarray(D, np.float32)
    b = np.ascontiguousarray(b0, np.float32).copy()
    s = SUMS[order]
    dist = np.float32(0)
    for _ in range(n_iter):
        y = s(D * b[None, :], 1)
        z = s(D * y[:, None], 0)
        nrm = np.sqrt(s(z * z, 0))
        bn = (z / nrm).astype(np.float32)
        dist = np.sqrt(s((bn - b) * (bn - b), 0))
        b = bn
    if s(s(D * b[None, :], 1), 0) < 0:
        b = -b
    return b, float(dist)


def mean_twin(D: np.ndarray, order: str = "serial") -> np.ndarray:
    D = np.ascontiguousarray(D, np.float32)
    s = SUMS[order]
    z = (s(D, 0) * np.float32(1.0 / D.shape[0])).astype(np.float32)
    return (z / np.sqrt(s(z * z, 0))).astype(np.float32)


def top_eigvec64(D: np.ndarray):
    """(the unit top eigenvector of D^T D oriented so that sum_r D[r] . u >= 0, the eigenvalues descending) in float64.  For R < E the eigenvectors come from
    the R x R Gram matrix D D^T (the same non-zero spectrum): u = D^T w / |D^T w|."""
    D64 = np.asarray(D, np.float64)
    R, E = D64.shape
    if R < E:
        lam, W = np.linalg.eigh(D64 @ D64.T)
        u = D64.T @ W[:, -1]
    else:
        lam, W = np.linalg.eigh(D64.T @ D64)
        u = W[:, -1]
    u = u / np.linalg.norm(u)
    if (D64 @ u).sum() < 0:
        u = -u
    return u, lam[::-1]


def mean_dir64(D: np.ndarray) -> np.ndarray:
    z = np.asarray(D, np.float64).mean(axis=0)
    return z / np.linalg.norm(z)


def one_minus_abs_cos(v: np.ndarray, u: np.ndarray) -> float:
    """1 - |cos(v, u)| in float64, as |a -+ b|^2 / 2 of the two unit vectors (no cancellation near 1)."""
    a = np.asarray(v, np.float64); a = a / np.linalg.norm(a)
    b = np.asarray(u, np.float64); b = b / np.linalg.norm(b)
    return float(min(((a - b) ** 2).sum(), ((a + b) ** 2).sum()) / 2.0)
