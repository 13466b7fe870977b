"""ggml's quantize_row_tq1_0_ref / quantize_row_tq2_0_ref restated in numpy: the specification of csrc/quantize.hip's two ternary branches.  Written from the
arithmetic, not from the decoders; tests/test_ternary_quantize_cpu.py holds it against tests/quant_error_ref.py's decoders.

    per 256-element block: amax = max |x|; d = amax, stored as f16; id = amax != 0 ? 1 / amax : 0 (of the f32, not of the stored f16);
    code = lroundf(x * id) + 1 in 0..2 - a half goes away from zero
    TQ2_0 (66 bytes: qs[64] | d): byte 32 h + l holds elements 128 h + l + 32 k at bits 2 k
    TQ1_0 (54 bytes: qs[48] | qh[4] | d): qs[j] holds elements j + 32 n, qs[32 + j] elements 160 + j + 16 n (n = 0..4), qh[j] elements 240 + j + 4 n
        (n = 0..3) and a fifth trit 0; n = 0 is the most significant base-3 digit of q, and the byte is (q * 256 + 242) / 243 in integers
The importance matrix is accepted and ignored, as upstream does for these types."""
import numpy as np

TQ1_0, TQ2_0 = 34, 35
F32, F16, BF16 = 0, 1, 30
BLOCK_BYTES = {TQ1_0: 54, TQ2_0: 66}


def to_f32(x: np.ndarray, src_type=None) -> np.ndarray:
    x = np.asarray(x)
    if src_type == BF16:
        return (x.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return x.astype(np.float32)


def quantize_rows(t: int, x: np.ndarray, imatrix=None, src_type=None) -> np.ndarray:
    """rows [n_rows][n_per_row] (f32, f16, or uint16 bf16 bits with src_type=30) -> uint8 [n_rows][row bytes] of type t"""
    assert t in BLOCK_BYTES and x.ndim == 2 and x.shape[1] % 256 == 0, (t, x.shape)
    v = to_f32(x, src_type).reshape(-1, 256)
    amax = np.abs(v).max(axis=1)
    with np.errstate(divide="ignore"):
        inv = np.where(amax != 0, np.float32(1) / amax, np.float32(0)).astype(np.float32)
    r = (v * inv[:, None]).astype(np.float32)
    # lroundf: |r| <= 1 has 24 bits, so |r| + 0.5 is exact in f64 (in f32 the largest value below a half would round up to it)
    code = (np.sign(r) * np.floor(np.abs(r).astype(np.float64) + 0.5)).astype(np.int64) + 1
    assert code.min() >= 0 and code.max() <= 2
    out = np.zeros((v.shape[0], BLOCK_BYTES[t]), np.uint8)
    if t == TQ2_0:
        c = code.reshape(-1, 2, 4, 32)                                          # [block][h][k][l]
        out[:, :64] = (c[:, :, 0] | c[:, :, 1] << 2 | c[:, :, 2] << 4 | c[:, :, 3] << 6).reshape(-1, 64)
    else:
        pow3 = np.array([81, 27, 9, 3, 1]).reshape(1, 5, 1)
        q = np.concatenate([(code[:, :160].reshape(-1, 5, 32) * pow3).sum(axis=1), (code[:, 160:240].reshape(-1, 5, 16) * pow3).sum(axis=1),
                            (code[:, 240:].reshape(-1, 4, 4) * pow3[:, :4]).sum(axis=1)], axis=1)
        out[:, :52] = (q * 256 + 242) // 243
    with np.errstate(over="ignore"):
        out[:, -2:] = amax.astype("<f2").view(np.uint8).reshape(-1, 2)
    return out.reshape(x.shape[0], -1)
