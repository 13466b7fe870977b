"""The merged-LoRA export in numpy float64 (csrc/lora_merge.hip, tools/export_lora.py): deq(W) + sum_i s_i B_i A_i, rounded once to the out type."""
import numpy as np

import np_twin as tw

F32, F16, BF16, Q8_0, Q4_K, Q5_K, Q6_K = 0, 1, 30, 8, 12, 13, 14
BASE_TYPES = (F32, F16, BF16, Q8_0, Q4_K, Q5_K, Q6_K)
OUT_DTYPE = {F16: np.float16, F32: np.float32}


def dequantize64(t: int, rows: np.ndarray) -> np.ndarray:
    """rows [N][...] as the file holds them (float arrays, uint16 bf16 bits, uint8 blocks) -> float64 [N][K], every value exact"""
    rows = np.ascontiguousarray(rows)
    N = rows.shape[0]
    if t in (F32, F16):
        return rows.view({F32: "<f4", F16: "<f2"}[t]).astype(np.float64).reshape(N, -1)
    if t == BF16:
        return (rows.view("<u2").astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64).reshape(N, -1)
    raw = rows.view(np.uint8).reshape(-1)
    b = raw.view(tw.DT[t])
    q = tw.unpack_ints(t, raw).astype(np.float64)
    d = b["d"].astype(np.float64)
    if t == Q8_0:
        y = q * d[:, None]
    elif t in (Q4_K, Q5_K):
        sc, mn = tw.k_scales(b["scales"])
        y = (d[:, None] * sc)[:, :, None] * q.reshape(-1, 8, 32) - (b["dmin"].astype(np.float64)[:, None] * mn)[:, :, None]
    elif t == Q6_K:
        y = (d[:, None] * b["scales"].astype(np.float64))[:, :, None] * q.reshape(-1, 16, 16)
    else:
        raise ValueError(t)
    return y.reshape(N, -1)


def merge_rows(base_type: int, base_rows: np.ndarray, adapters, out_type: int = F16):
    """adapters = [(A [r][K], B [N][r], scale)] -> (rounded [N][K] of the out type, the float64 value before rounding, the bound sum_i |s_i| |B_i| @ |A_i|)"""
    w = dequantize64(base_type, base_rows)
    ref, bound = w.copy(), np.zeros_like(w)
    for a, b, s in adapters:
        a64, b64, s64 = np.asarray(a, np.float64), np.asarray(b, np.float64), float(np.float32(s))
        ref += s64 * (b64 @ a64)
        bound += abs(s64) * (np.abs(b64) @ np.abs(a64))
    return ref.astype(OUT_DTYPE[out_type]), ref, bound
