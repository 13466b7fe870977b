"""Case lists, inputs and bounds of the importance-matrix tests (tests/test_imatrix_cpu.py, tests/test_gpu_imatrix_ops.py, tests/test_gpu_imatrix.py).

Bounds, each from the arithmetic and not from what the device gives:
  exact      integer inputs |x| <= 15, at most 4096 rows a matrix: every partial sum is an integer below 15^2 * 4096 < 2^20, exact in f32 in any order.
  float      ref = the float64 sum of the float64 squares of the f32 inputs (plus the previous total).  The terms are non-negative; a square is rounded
             once and n terms take at most n rounded additions in any order (a fused multiply-add rounds less), so per column
             |dev - ref| <= (n + 4) * 2^-24 * ref, n the rows summed into the column so far (the 4 covers the slab sums and the add to the total).
  taps       against sum_t (rmsnorm(tap[t]) * w)^2 in float64 from the device's own layer taps: the norm kernel is held to NORM_REL of the row's
             largest value by test_rms_norm_mul (tests/test_gpu_ops.py); a square doubles a relative deviation: 2 * NORM_REL + (n + 4) * 2^-24 per column.
  reference  rel_err(dev, ref) <= 2 * FLIP_TOL (rel_err, FLIP_TOL of tests/lora_cases.py): the model tests allow a layer's rows FLIP_TOL, the square
             doubles it."""
from __future__ import annotations

import os

import numpy as np

from lora_cases import FLIP_TOL, rel_err  # noqa: F401  (re-exported)

U = 2.0 ** -24
NORM_REL = 2e-7                       # tests/test_gpu_ops.py test_rms_norm_mul
KV = {"f16": 1, "q8_0": 8}
N_PROMPT = 40

OP_KS = [32, 96, 576, 4096, 4128]
OP_RS = [1, 2, 31, 33, 513, 4096]
PRODUCER_KS, PRODUCER_RS = [512, 4864], [1, 40]
DENSE_FILES = [("tiny", "q4_k_m"), ("tiny-w576-2l", "q8_0"), ("tiny-qwen2", "q4_k_m"), ("tiny-qwen3", "q4_k_m")]
MOE_FILES = [("tiny-moe", "q4_k_m"), ("tiny-qwen3moe", "q4_k_m")]
MOE_SHAPES_ONLY = ("tiny-qwen3moe-160e", "q4_k_m")
MOE_TS = [40, 5]


def float_bound(ref: np.ndarray, n) -> np.ndarray:
    return (np.asarray(n, np.float64) + 4.0) * U * np.asarray(ref, np.float64)


def tap_bound(ref: np.ndarray, n) -> np.ndarray:
    return (2.0 * NORM_REL + (np.asarray(n, np.float64) + 4.0) * U) * np.asarray(ref, np.float64)


def int_rows(rng, R: int, ld: int) -> np.ndarray:
    return rng.integers(-15, 16, (R, ld)).astype(np.float32)


def normal_rows(rng, R: int, ld: int) -> np.ndarray:
    return rng.standard_normal((R, ld)).astype(np.float32)


def sq_sum(x: np.ndarray, K: int) -> np.ndarray:
    """float64 column sums of squares of the first K columns"""
    return (np.asarray(x, np.float32)[:, :K].astype(np.float64) ** 2).sum(axis=0)


def expert_ref(x: np.ndarray, K: int, counts, row_src=None):
    """[n_mat][K] float64 sums of squares when launch row r reads x[row_src[r]] and the launch rows are cut into runs of counts[m] rows"""
    counts = np.asarray(counts)
    rows = np.arange(int(counts.sum())) if row_src is None else np.asarray(row_src)
    out = np.zeros((counts.size, K), np.float64)
    r = 0
    for m, c in enumerate(counts):
        out[m] = sq_sum(x[rows[r:r + c]], K) if c else 0.0
        r += int(c)
    return out


def model_file(pkg, tmp_models, cfg: str, ftype: str, seed: int = 29) -> str:
    path = str(tmp_models / f"imx-{cfg}-{ftype}-{seed}.gguf")
    if not os.path.exists(path):
        pkg.gguf_synth.write_synthetic_llama(path, cfg, ftype, seed=seed)
    return path


def prompt_tokens(n_vocab: int, n: int = N_PROMPT, seed: int = 41) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, n_vocab, n).astype(np.int32)


def head_flags(n: int = N_PROMPT) -> np.ndarray:
    """the rows flagged for logits in the model cases: every fourth token and the last (11 of 40)"""
    f = np.zeros(n, np.int8)
    f[3::4] = 1
    f[-1] = 1
    return f


def expected_names(path: str, process_output: bool) -> dict:
    """{tensor name: (ne0, n_mat)} of the 2-D (3-D for experts) weight tensors of the file that a decode multiplies"""
    from gguf_read import read_gguf
    _, t = read_gguf(path)
    stems = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down", "ffn_gate_inp", "ffn_gate_exps", "ffn_up_exps", "ffn_down_exps")
    out = {}
    for name, (ne, _, _) in t.items():
        if name.startswith("blk.") and name.endswith(".weight") and name.split(".")[2] in stems:
            out[name] = (int(ne[0]), int(ne[2]) if len(ne) == 3 else 1)
    if process_output:
        head = "output.weight" if "output.weight" in t else "token_embd.weight"
        out[head] = (int(t[head][0][0]), 1)
    return out
