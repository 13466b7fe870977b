"""Reference importance-matrix collectors: the composed CPU forward passes of tests/qwen3_ref.py and tests/qwen3moe_ref.py with a hook on every projection.
For a projection NAME applied to rows x [n][K] the collector adds sum_t float64(x[t])^2 per column and the row count n under NAME (what llama-imatrix
records for ggml_mul_mat); for the routed feed-forward it keeps one row of sums and one count per expert (ggml_mul_mat_id): ffn_gate_exps / ffn_up_exps see the
normalised row h[t] of every token routed to the expert, ffn_down_exps the product silu(gate) * up of that (token, expert) pair; ffn_gate_inp is dense.

`im` maps a tensor name to [sum2 float64 [n_mat][K], counts int64 [n_mat]] over all decode calls since the object was made."""
from __future__ import annotations

import numpy as np

import oracle_py as oq
from qwen3_ref import Qwen3Ref
from qwen3moe_ref import Qwen3MoeRef, route_numpy


def note(im: dict, name: str, x: np.ndarray, n_mat: int = 1, m: int = 0) -> None:
    x = np.asarray(x, np.float32)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    if name not in im:
        im[name] = [np.zeros((n_mat, x.shape[1]), np.float64), np.zeros(n_mat, np.int64)]
    im[name][0][m] += (x.astype(np.float64) ** 2).sum(axis=0)
    im[name][1][m] += x.shape[0]


class ImatrixRef(Qwen3Ref):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.im: dict = {}

    def _mm(self, name, x):
        note(self.im, name, x)
        return super()._mm(name, x)


class ImatrixMoeRef(Qwen3MoeRef):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.im: dict = {}

    def _mm(self, name, x):
        if not name.endswith(("ffn_gate.weight", "ffn_up.weight", "ffn_down.weight")):      # (Qwen3MoeRef turns those three into the routed feed-forward)
            note(self.im, name, x)
        return super()._mm(name, x)

    def moe_ffn(self, p: str, h: np.ndarray) -> np.ndarray:
        """Qwen3MoeRef.moe_ffn restated with the collection: the same operations in the same order, so the same output and the same selections."""
        gi_ne, gi_t, gi_raw = self.t[p + "ffn_gate_inp.weight"]
        g_ne, g_t, g_raw = self.t[p + "ffn_gate_exps.weight"]
        u_ne, u_t, u_raw = self.t[p + "ffn_up_exps.weight"]
        d_ne, d_t, d_raw = self.t[p + "ffn_down_exps.weight"]
        E, F, NE = g_ne[0], g_ne[1], self.n_expert
        gb, ub, db = oq.row_bytes(g_t, E) * F, oq.row_bytes(u_t, E) * F, oq.row_bytes(d_t, F) * E
        nth = oq.threads()
        out = np.zeros((h.shape[0], E), np.float32)
        sel = np.zeros((h.shape[0], self.k), np.int32)
        note(self.im, p + "ffn_gate_inp.weight", h)
        for t in range(h.shape[0]):
            logits = oq.mul_mat(gi_t, gi_raw, gi_ne[1], gi_ne[0], h[t:t + 1], nth)[0]
            ids, w = route_numpy(logits, self.k)
            sel[t] = ids
            o = None
            for j, e in enumerate(ids):
                e = int(e)
                note(self.im, p + "ffn_gate_exps.weight", h[t], NE, e)
                note(self.im, p + "ffn_up_exps.weight", h[t], NE, e)
                g = oq.mul_mat(g_t, g_raw[e * gb:(e + 1) * gb], F, E, h[t:t + 1], nth)[0]
                u = oq.mul_mat(u_t, u_raw[e * ub:(e + 1) * ub], F, E, h[t:t + 1], nth)[0]
                a = (oq.silu(g) * u).astype(np.float32)
                note(self.im, p + "ffn_down_exps.weight", a, NE, e)
                y = oq.mul_mat(d_t, d_raw[e * db:(e + 1) * db], E, F, a[None, :], nth)[0]
                v = (y * w[j]).astype(np.float32)
                o = v if o is None else (o + v).astype(np.float32)
            out[t] = o
        self._layer_routes.append(sel)
        return out
