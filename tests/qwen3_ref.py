"""The qwen3 forward pass (llm_build_qwen3) composed from the CPU oracle's own per-op primitives (tests/oracle_py.py), for files the oracle's graph
cannot load: general.architecture "qwen3" - qwen2's op order without biases, a per-head RMSNorm of Q and K (attn_q_norm / attn_k_norm, [head_dim] f32)
before the NEOX rope, and a head size of its own (attention.key_length), so that the attention width H * D need not be n_embd.

Every op is the oracle's: mul_mat (activations quantised to the weight's vec_dot type, as ggml's CPU path does), rms_norm, rope(neox=True), quantize of the
K / V cache rows, flash_attn, silu; element-wise products and sums are single f32 operations in numpy (bit-identical to ggml's).  Per token and layer:

    h = rms_norm(x) * attn_norm
    q, k, v = W_q h (+ b_q), W_k h (+ b_k), W_v h (+ b_v)          (biases: qwen2 files)
    q_h = rms_norm(q_h) * q_norm, k_h = rms_norm(k_h) * k_norm        (every head over its own head_dim values; qwen3 only)
    q, k = rope_neox(q), rope_neox(k);  K / V rows -> cache;  att = flash_attn(q, cache over the visible cells)
    x = x + W_o att;  h = rms_norm(x) * ffn_norm;  x = x + W_down (silu(W_gate h) * W_up h)
and the head: rms_norm(x) * output_norm, then output.weight (token_embd.weight when the file has none).

With qk_norm=False on a qwen2 file without biases this is the oracle's own graph (tests/test_qwen3_cpu.py checks that it equals OracleContext.decode)."""
from __future__ import annotations

import numpy as np

import oracle_py as oq
from gguf_read import read_gguf


class Qwen3Ref:
    """A context over one file: cells with positions and sequences (the next free cell is taken, as a fresh cache does), per-layer taps of the last
    decode call (layer_out) and the logits of its last token."""

    def __init__(self, path: str, n_ctx: int, type_k: int, type_v: int, qk_norm: bool = True):
        kv, self.t = read_gguf(path)
        a = kv["general.architecture"]
        self.E = kv[f"{a}.embedding_length"]
        self.n_layer = kv[f"{a}.block_count"]
        self.H = kv[f"{a}.attention.head_count"]
        self.G = kv[f"{a}.attention.head_count_kv"]
        self.D = kv.get(f"{a}.attention.key_length", self.E // self.H) if a == "qwen3" else self.E // self.H
        self.eps = kv[f"{a}.attention.layer_norm_rms_epsilon"]
        self.base = kv[f"{a}.rope.freq_base"]
        self.neox = a != "llama"
        self.qk_norm = qk_norm and a == "qwen3"
        self.n_vocab = self.t["token_embd.weight"][0][1]
        self.n_ctx, self.tk, self.tv = n_ctx, type_k, type_v
        kvw = self.G * self.D
        self.kc = np.zeros((self.n_layer, n_ctx, oq.row_bytes(type_k, kvw)), np.uint8)
        self.vc = np.zeros((self.n_layer, n_ctx, oq.row_bytes(type_v, kvw)), np.uint8)
        self.cell_pos = np.full(n_ctx, -1, np.int64)
        self.cell_seq = np.zeros(n_ctx, np.int64)
        self.taps: list[np.ndarray] = []

    def _f32(self, name):
        return self.t[name][2].view("<f4")

    def _mm(self, name, x):
        ne, ty, raw = self.t[name]
        return oq.mul_mat(ty, raw, ne[1], ne[0], x, oq.threads())

    def _norm_rows(self, x, w):
        return np.stack([oq.rms_norm(r, self.eps) * w for r in x]).astype(np.float32)

    def _head_norm(self, rows, n_head, w):
        D = self.D
        out = np.empty_like(rows)
        for h in range(n_head):
            out[h * D:(h + 1) * D] = oq.rms_norm(rows[h * D:(h + 1) * D], self.eps) * w
        return out

    def decode(self, tokens, pos, seq=None, want=None) -> np.ndarray:
        """One batch (every token's K / V row is in the cache before any token attends); returns the logits of the flagged tokens (want; default: the
        last one), [n_out][n_vocab]."""
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
            self.taps.append(x.copy())
        rows = np.nonzero(np.asarray(want).reshape(-1))[0] if want is not None else [n - 1]
        h = self._norm_rows(x[rows], self._f32("output_norm.weight"))
        return self._mm("output.weight" if "output.weight" in self.t else "token_embd.weight", h)

    def layer_out(self, il: int, n_tokens: int) -> np.ndarray:
        assert self.taps[il].shape[0] == n_tokens
        return self.taps[il].copy()
