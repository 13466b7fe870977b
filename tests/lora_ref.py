"""The forward pass with LoRA adapters applied at run time, as llama.cpp's build_lora_mm does inside every mul_mat of the graph: Qwen3Ref (tests/qwen3_ref.py)
and Qwen3MoeRef (tests/qwen3moe_ref.py) with `_mm` adding, for every active adapter that has a pair on the tensor, in the order the adapters were set,

    scale * mul_mat(lora_b, mul_mat(lora_a, x)),     scale = user_scale * alpha / r   (user_scale when alpha == 0)

Both products are the oracle's mul_mat (ggml's CPU arithmetic: an F16 pair rounds its activation - x, then t = A x - to f16 and sums in f32), the scaling and
the additions are single f32 operations.  An adapter file is read with tests/gguf_read.py; nothing under oracle/ knows about adapters."""
from __future__ import annotations

import numpy as np

import oracle_py as oq
from gguf_read import read_gguf
from qwen3_ref import Qwen3Ref
from qwen3moe_ref import Qwen3MoeRef


class Adapter:
    def __init__(self, path: str):
        self.kv, self.t = read_gguf(path)
        self.alpha = np.float32(self.kv["adapter.lora.alpha"])
        self.bases = [n[: -len(".lora_a")] for n in self.t if n.endswith(".lora_a")]

    def scale(self, base: str, user_scale: float) -> np.float32:
        r = self.t[base + ".lora_a"][0][1]
        u = np.float32(user_scale)
        return np.float32(u * self.alpha / np.float32(r)) if self.alpha != 0 else u

    def delta(self, base: str, x: np.ndarray, user_scale: float):
        """scale * B (A x) for rows x [T][K], or None when the adapter has no pair on `base`."""
        if base + ".lora_a" not in self.t:
            return None
        (K, r), ta, A = self.t[base + ".lora_a"]
        (r2, N), tb, B = self.t[base + ".lora_b"]
        assert r == r2 and ta == tb
        t = oq.mul_mat(ta, A, r, K, x, oq.threads())
        return (oq.mul_mat(tb, B, N, r, t, oq.threads()) * self.scale(base, user_scale)).astype(np.float32)


class _LoraMM:
    """Mixin: set_adapters([(Adapter, user_scale), ...]) and the `_mm` that applies them.  A tied head takes an `output.weight` pair."""
    adapters: list = []

    def set_adapters(self, adapters):
        self.adapters = list(adapters)

    def _mm(self, name, x):
        y = super()._mm(name, x)
        base = "output.weight" if name == "token_embd.weight" else name
        for ad, user_scale in self.adapters:
            d = ad.delta(base, x, user_scale)
            if d is not None:
                y = (y + d).astype(np.float32)
        return y


class LoraRef(_LoraMM, Qwen3Ref):
    pass


class LoraMoeRef(_LoraMM, Qwen3MoeRef):
    pass
