"""The cases of the control-vector tests, shared by tests/test_cvec_cpu.py (the reference alone) and tests/test_gpu_cvec.py (the device against it).

Model cases: the tiny synthetic files through lora_cases.base_file.  A case's vector has one row per layer 1 .. n_layer - 1, normal with spread `std`, chosen
so that the delta condition of tests/lora_cases.py holds - on every case the reference alone moves the logits by at least 10 * FLIP_TOL when the vector is
applied (checked in tests/test_cvec_cpu.py, not assumed), so a device that ignored the vector could not pass.

PCA cases: rows a_r u + noise with a planted unit u, a_r >= 1, and noise small enough that lambda_2 / lambda_1 <= 0.1 (asserted from the float64 spectrum).
At that gap 64 iterations shrink the start vector's other components by 10^-64: the iterate is converged far below rounding and what is left is the
arithmetic's own error, which M_PCA bounds."""
from __future__ import annotations

import numpy as np

from lora_cases import Case

MODEL_CASES = [
    Case("llama-gqa4", "tiny-gqa4", "q4_k_m", "q8_0", ()),             # the llama graph, three layers
    Case("qwen3", "tiny-qwen3", "q4_k_m", "q8_0", ()),                 # q / k norm, a tied head, three layers (lora_cases.tight_applies)
    Case("moe", "tiny-moe", "q4_k_m", "q8_0", (), moe=True),           # the routed feed-forward, two layers
    Case("llama-d128-f16", "tiny-d128", "q4_k_m", "f16", ()),          # an f16 cache; the base takes the one-launch attention block
]
MODEL_IDS = [c.name for c in MODEL_CASES]
VEC_STD = {"llama-gqa4": 2.5, "qwen3": 2.5, "moe": 4.0, "llama-d128-f16": 1.5}
PROMPT_SEED, N_PROMPT = 5, 9


def case_vector(case: Case, n_layer: int, n_embd: int) -> np.ndarray:
    """f32 [n_layer - 1][n_embd]: the vectors of layers 1 .. n_layer - 1"""
    rng = np.random.default_rng(0xC7EC + MODEL_IDS.index(case.name))
    return (rng.standard_normal((n_layer - 1, n_embd)) * VEC_STD[case.name]).astype(np.float32)


def ranges(n_layer: int):
    """(name, il_start, il_end): all layers (upstream's default 1 .. n_layer), and a middle range - layer 1 alone"""
    return [("all", 1, n_layer), ("middle", 1, 1)]


def reference(case: Case, base: str, n_ctx: int):
    from cvec_ref import CvecMoeRef, CvecRef
    from lora_cases import KV
    return (CvecMoeRef if case.moe else CvecRef)(base, n_ctx, KV[case.kv], KV[case.kv])


# ------------------------------------------------------------------------------------------------ PCA
PCA_E = (64, 576, 896, 4096)
PCA_R = (1, 3, 67, 300)
PCA_CASES = [(R, E) for E in PCA_E for R in PCA_R]
PCA_IDS = [f"R{R}-E{E}" for R, E in PCA_CASES]
PCA_ITERS = 64
GAP_MAX = 0.1
# twice the largest 1 - |cos| between either f32 twin of tests/cvec_ref.py (serial, pairwise) and the float64 eigenvector over PCA_CASES, as
# tests/test_cvec_cpu.py::test_pca_twin_margin measures it (and checks this constant against what it measures)
M_PCA = 8.5e-14


def pca_rows(R: int, E: int):
    """(D f32 [R][E], the planted unit u f64 [E], the start vector b0 f32 [E])"""
    rng = np.random.default_rng(1000 * E + R)
    u = rng.standard_normal(E)
    u /= np.linalg.norm(u)
    a = 1.0 + np.abs(rng.standard_normal(R))
    sigma = 0.15 * np.sqrt(R) / (np.sqrt(R) + np.sqrt(E)) if R > 1 else 0.0
    D = (a[:, None] * u[None, :] + sigma * rng.standard_normal((R, E))).astype(np.float32)
    b0 = rng.standard_normal(E).astype(np.float32)
    b0 /= np.float32(np.linalg.norm(b0))
    return D, u, b0
