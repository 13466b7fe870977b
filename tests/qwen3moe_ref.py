"""The qwen3moe forward pass (llm_build_qwen3moe) composed from the CPU oracle's per-op primitives, for files the oracle's graph cannot load: qwen3's attention
(tests/qwen3_ref.py: per-head q / k RMSNorm before the NEOX rope, head size from attention.key_length) with build_moe_ffn's routed feed-forward in place of
the dense one, and no shared expert.  Per token and layer, after the attention of Qwen3Ref:

    h = rms_norm(x) * ffn_norm
    logits = gate_inp h;  p = soft_max(logits)
    ids = the k largest p, first index on a tie;  w = p[ids] / (sum of p[ids] in rank order, f32)
    x = x + sum over ranks j in order of (W_down[ids[j]] (silu(W_gate[ids[j]] h) * W_up[ids[j]] h)) * w[j]

which is oracle/oq_llama.c ffn_moe op for op.  The selection is restated in numpy (selection_numpy): the oracle's oq_moe_route marks chosen experts in a
64-bit mask and serves at most 64 experts; the restatement serves any number, and equals oq_moe_route where both apply (tests/test_qwen3moe_cpu.py).

The module records its selections: routes[i] is [n_layer][n_tokens][k] for the i-th decode call, ready for Context.force_moe_ids."""
from __future__ import annotations

import numpy as np

import oracle_py as oq
from qwen3_ref import Qwen3Ref


def selection_numpy(probs: np.ndarray, k: int, forced=None):
    """First-max top-k of one token's probabilities and the weights renormalised in f32 in rank order: (ids [k] int32, w [k] f32).  forced: the ids to take
    instead (the weights are still their probabilities, renormalised), as the device's force hook does."""
    probs = np.asarray(probs, np.float32)
    used = np.zeros(probs.size, bool)
    ids = np.zeros(k, np.int32)
    w = np.zeros(k, np.float32)
    for j in range(k):
        best = int(np.argmax(np.where(used, -np.inf, probs)))        # (argmax: the first index of the largest value)
        if forced is not None:
            best = min(max(int(forced[j]), 0), probs.size - 1)
        used[best] = True
        ids[j], w[j] = best, probs[best]
    wsum = np.float32(0.0)
    for j in range(k):
        wsum = np.float32(wsum + w[j])
    return ids, (w / wsum).astype(np.float32)


def route_numpy(logits: np.ndarray, k: int, forced=None):
    """The selection of one token from its router logits: the oracle's soft_max, then selection_numpy."""
    return selection_numpy(oq.soft_max(np.asarray(logits, np.float32), None, 1.0), k, forced)


class Qwen3MoeRef(Qwen3Ref):
    """Qwen3Ref with the routed feed-forward.  Also composes the llama graph of a Mixtral-style file (general.architecture "llama" with experts): there
    the attention is the oracle's own (no q / k norm, rope in adjacent pairs), and tests/test_qwen3moe_cpu.py checks the whole pass against the oracle."""

    def __init__(self, path: str, n_ctx: int, type_k: int, type_v: int, qk_norm: bool = True):
        super().__init__(path, n_ctx, type_k, type_v, qk_norm)
        from gguf_read import read_gguf
        kv, _ = read_gguf(path)
        a = kv["general.architecture"]
        if a == "qwen3moe":                                            # (Qwen3Ref reads these for "qwen3" only)
            self.D = kv[f"{a}.attention.key_length"]
            self.qk_norm = qk_norm
            kvw = self.G * self.D
            self.kc = np.zeros((self.n_layer, n_ctx, oq.row_bytes(type_k, kvw)), np.uint8)
            self.vc = np.zeros((self.n_layer, n_ctx, oq.row_bytes(type_v, kvw)), np.uint8)
        self.n_expert = kv[f"{a}.expert_count"]
        self.k = kv[f"{a}.expert_used_count"]
        self.routes: list[np.ndarray] = []
        self._layer_routes: list[np.ndarray] = []
        self._moe_out = None

    def decode(self, tokens, pos, seq=None, want=None) -> np.ndarray:
        self._layer_routes = []
        out = super().decode(tokens, pos, seq, want)
        self.routes.append(np.stack(self._layer_routes))
        return out

    # Qwen3Ref.decode runs the dense feed-forward as x + _mm(ffn_down, silu(_mm(ffn_gate, h)) * _mm(ffn_up, h)).  Here the ffn_gate call computes the routed
    # feed-forward of h and keeps it, ffn_up hands back zeros, and the ffn_down call returns what ffn_gate kept: x + moe(h), nothing else added.
    def _mm(self, name, x):
        if name.endswith("ffn_gate.weight"):
            self._moe_out = self.moe_ffn(name[: -len("ffn_gate.weight")], x)
            return np.zeros((x.shape[0], 1), np.float32)
        if name.endswith("ffn_up.weight"):
            return np.zeros((x.shape[0], 1), np.float32)
        if name.endswith("ffn_down.weight"):
            out, self._moe_out = self._moe_out, None
            return out
        return super()._mm(name, x)

    def moe_ffn(self, p: str, h: np.ndarray) -> np.ndarray:
        """build_moe_ffn on rows h [T][E] of layer prefix p, token by token as oracle/oq_llama.c ffn_moe; records the layer's selections."""
        gi_ne, gi_t, gi_raw = self.t[p + "ffn_gate_inp.weight"]
        g_ne, g_t, g_raw = self.t[p + "ffn_gate_exps.weight"]
        u_ne, u_t, u_raw = self.t[p + "ffn_up_exps.weight"]
        d_ne, d_t, d_raw = self.t[p + "ffn_down_exps.weight"]
        E, F = g_ne[0], g_ne[1]
        gb, ub, db = oq.row_bytes(g_t, E) * F, oq.row_bytes(u_t, E) * F, oq.row_bytes(d_t, F) * E
        nth = oq.threads()
        out = np.zeros((h.shape[0], E), np.float32)
        sel = np.zeros((h.shape[0], self.k), np.int32)
        for t in range(h.shape[0]):
            logits = oq.mul_mat(gi_t, gi_raw, gi_ne[1], gi_ne[0], h[t:t + 1], nth)[0]
            ids, w = route_numpy(logits, self.k)
            sel[t] = ids
            o = None
            for j, e in enumerate(ids):
                e = int(e)
                g = oq.mul_mat(g_t, g_raw[e * gb:(e + 1) * gb], F, E, h[t:t + 1], nth)[0]
                u = oq.mul_mat(u_t, u_raw[e * ub:(e + 1) * ub], F, E, h[t:t + 1], nth)[0]
                a = (oq.silu(g) * u).astype(np.float32)
                y = oq.mul_mat(d_t, d_raw[e * db:(e + 1) * db], E, F, a[None, :], nth)[0]
                v = (y * w[j]).astype(np.float32)
                o = v if o is None else (o + v).astype(np.float32)
            out[t] = o
        self._layer_routes.append(sel)
        return out
