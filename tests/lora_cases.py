"""The (base model, adapters) pairs of the end-to-end adapter tests, shared by tests/test_gpu_lora.py (the device against LoraRef) and tests/test_lora_cpu.py
(the delta condition: on every pair the reference alone moves the logits by at least 10 * FLIP_TOL, so a device that ignored the adapter could not pass).

An adapter spec is the keyword set of gguf_synth.write_synthetic_lora plus the user scale it is set with.  `std` (the spread of lora_b) is chosen per case
so that the delta condition holds; it is checked, not assumed."""
from __future__ import annotations

import dataclasses
import os

ALL7 = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")
ATTN = ("attn_q", "attn_k", "attn_v", "attn_output")
KV = {"f16": 1, "q8_0": 8, "q4_0": 2}
FLIP_TOL = 3e-2      # tests/test_gpu_model.py (see the calibration note there)
TIGHT_TOL = 2e-5


@dataclasses.dataclass(frozen=True)
class Ad:
    rank: int
    alpha: float
    targets: tuple
    dtype: str = "f16"
    std: float = 0.1
    seed: int = 0x10A
    scale: float = 1.0

    def file_key(self):
        return f"r{self.rank}-a{self.alpha:g}-{self.dtype}-s{self.seed}-{self.std:g}-" + "+".join(t.replace("attn_", "a").replace("ffn_", "f") for t in self.targets)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    cfg: str
    ftype: str
    kv: str
    adapters: tuple
    moe: bool = False


CASES = [
    # the base takes the one-launch attention block (Q | K | V + attention + attn_output) here: every gate of it is exercised; the head is adapted too
    Case("d128-all", "tiny-d128", "q4_k_m", "q8_0", (Ad(8, 16.0, ALL7 + ("output",)),)),
    Case("tiny-f32", "tiny", "q8_0", "f16", (Ad(4, 8.0, ALL7, dtype="f32"),)),
    Case("qwen2-attn", "tiny-qwen2", "q8_0", "q8_0", (Ad(12, 12.0, ATTN, std=0.2),)),                     # biases, NEOX; a rank that is no multiple of 8
    Case("qwen3-all", "tiny-qwen3", "q4_k_m", "q8_0", (Ad(8, 16.0, ALL7 + ("output",), dtype="f32"),)),   # q / k norm after the delta; a tied head; F32 (tight_applies)
    Case("moe-attn", "tiny-moe", "q4_k_m", "q8_0", (Ad(8, 16.0, ("attn_q", "attn_v", "attn_output"), std=0.3),), moe=True),
    Case("w576-all", "tiny-w576-2l", "q4_k_m", "q8_0", (Ad(5, 10.0, ALL7, std=0.25),)),                          # a width that is no multiple of 256
    Case("d128-two", "tiny-d128", "q4_k_m", "q8_0", (Ad(8, 16.0, ("attn_q", "attn_v"), std=0.3), Ad(3, 0.0, ALL7, dtype="f32", seed=0x20B, scale=-0.5))),
    Case("d128-ffn", "tiny-d128", "q4_k_m", "q8_0", (Ad(16, 16.0, ("ffn_gate", "ffn_down"), std=0.2),)),   # the attention block keeps its one launch
]
CASE_IDS = [c.name for c in CASES]


def tight_applies(case: Case) -> bool:
    """Where the first layer's rows are compared at TIGHT_TOL.  tests/test_gpu_qwen3.py states the rule: before the first rounding flip the device and the
    reference agree to f32 round-off, so the typical token does - except with an f16 cache or Q8_0 weights, where a flip is the rule, not the exception.
    An F16 adapter pair is a third such place.  It rounds x to f16 and then t = A x to f16: the two sides' x differ by 1e-7 .. 1e-6 relative (f32 round-off
    of the norm, of SwiGLU), an f16 step is 5e-4, so some of a row's hundreds of elements round apart on most tokens; each moves t by A[j][k] ulp(x[k]),
    about 4 % of t's own f16 step, and a t[j] that lands on the other side moves the whole output row by scale * B[.][j] * ulp(t[j]) ~ 1e-4 - enough to
    flip a few codes of the next activation quantisation, an error of 1e-3 at that token.  Measured on the MI355X (21-token prompt, first-layer rows,
    tiny-qwen3 q4_k_m, q8_0 cache, all seven tensors adapted): with an F16 pair 17 of 21 tokens are 8e-4 .. 5e-3 apart and the other 4 within 1.5e-5;
    the base model alone has every token within 3e-7.  With an F32 pair nothing is rounded to f16 and the rule holds as it does for the base model
    (measured, same file and prompt: 19 of 21 tokens within 3e-7, two lone tokens at 1.2e-3)."""
    return case.kv != "f16" and case.ftype != "q8_0" and all(ad.dtype == "f32" for ad in case.adapters)


def base_file(gs, tmp_models, case: Case, seed: int = 11) -> str:
    path = str(tmp_models / f"{case.cfg}-{case.ftype}-{seed}.gguf")
    if not os.path.exists(path):
        gs.write_synthetic_llama(path, case.cfg, case.ftype, seed=seed)
    return path


def adapter_file(gs, tmp_models, cfg: str, ad: Ad) -> str:
    path = str(tmp_models / f"lora-{cfg}-{ad.file_key()}.gguf")
    if not os.path.exists(path):
        gs.write_synthetic_lora(path, cfg, rank=ad.rank, alpha=ad.alpha, targets=ad.targets, dtype=ad.dtype, seed=ad.seed, std=ad.std)
    return path


def reference(case: Case, base: str, adapter_paths, n_ctx: int, with_adapters: bool = True):
    """LoraRef / LoraMoeRef over the case's base file with its adapters set (or none)."""
    from lora_ref import Adapter, LoraMoeRef, LoraRef
    ref = (LoraMoeRef if case.moe else LoraRef)(base, n_ctx, KV[case.kv], KV[case.kv])
    if with_adapters:
        ref.set_adapters([(Adapter(p), ad.scale) for p, ad in zip(adapter_paths, case.adapters)])
    return ref


def rel_err(a, b):
    import numpy as np
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))
