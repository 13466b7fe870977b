// ggml_types.h — what the host and the kernels both know about a ggml tensor type: its id, its on-disk block, its device row.
// No HIP header: the load planner (host/model_plan.cc) and its CPU tests compile this with a plain C++ compiler.
#pragma once

#include <stddef.h>
#include <stdint.h>

// callable from kernels under hipcc, plain functions elsewhere
#if defined(__HIP__) || defined(__HIPCC__)
#define MI355_HD __host__ __device__
#else
#define MI355_HD
#endif

namespace mi355 {

// ggml type ids (GGUF on-disk values)
enum : int {
    T_F32 = 0, T_F16 = 1, T_Q4_0 = 2, T_Q4_1 = 3, T_Q5_0 = 6, T_Q5_1 = 7, T_Q8_0 = 8, T_Q2_K = 10, T_Q3_K = 11, T_Q4_K = 12, T_Q5_K = 13, T_Q6_K = 14, T_Q8_K = 15, T_IQ4_NL = 20, T_IQ4_XS = 23, T_BF16 = 30, T_TQ1_0 = 34, T_TQ2_0 = 35, T_MXFP4 = 39,
};

// ---- ggml on-disk block sizes ------------------------------------------------------------
MI355_HD constexpr int ggml_block_elems(int t) {
    return (t == T_F32 || t == T_F16 || t == T_BF16) ? 1 : (t == T_Q4_0 || t == T_Q4_1 || t == T_Q5_0 || t == T_Q5_1 || t == T_Q8_0 || t == T_IQ4_NL || t == T_MXFP4) ? 32 : 256;
}
MI355_HD constexpr int ggml_block_bytes(int t) {
    return t == T_F32 ? 4 : (t == T_F16 || t == T_BF16) ? 2 : t == T_Q4_0 ? 18 : t == T_Q8_0 ? 34 : t == T_Q4_K ? 144 :
           t == T_Q5_K ? 176 : t == T_Q6_K ? 210 : t == T_Q8_K ? 292 : t == T_Q2_K ? 84 : t == T_Q3_K ? 110 : t == T_Q5_0 ? 22 : t == T_Q4_1 ? 20 : t == T_Q5_1 ? 24 : t == T_IQ4_NL ? 18 : t == T_IQ4_XS ? 136 : t == T_MXFP4 ? 17 :
           t == T_TQ1_0 ? 54 : t == T_TQ2_0 ? 66 : 0;
}
MI355_HD inline size_t ggml_row_bytes(int t, int64_t n) {
    return (size_t)(n / ggml_block_elems(t)) * (size_t)ggml_block_bytes(t);
}

// the CPU backend's activation format for a weight type: Q8_0 blocks for the 32-element formats, Q8_K for the K-quants
MI355_HD constexpr bool act_is_q80(int t) { return t == T_Q8_0 || t == T_Q4_0 || t == T_Q4_1 || t == T_Q5_0 || t == T_Q5_1 || t == T_IQ4_NL || t == T_MXFP4; }
// the 32-element nibble formats: a fifth-bit word per block (Q5_0, Q5_1); a per-block f16 minimum m, weight = q d + m with q unsigned (Q4_1, Q5_1)
MI355_HD constexpr bool nib32_has_qh(int t) { return t == T_Q5_0 || t == T_Q5_1; }
MI355_HD constexpr bool nib32_has_min(int t) { return t == T_Q4_1 || t == T_Q5_1; }
// byte offset of the f16 scale plane in a device row of a 32-element nibble format (the minimum plane follows it, K / 32 * 2 bytes on)
MI355_HD constexpr size_t nib32_d_off(int t, size_t K) { return (K >> 1) + (nib32_has_qh(t) ? (K >> 5) * 4 : 0); }
// MXFP4: the block scale is one E8M0 byte e, kept as that byte (a K / 32 byte plane behind the nibbles) and turned into an f32 where it is used:
// half of 2^(e - 127) as a bit pattern, exact for every e (e < 2 gives the two subnormals 2^-128 and 2^-127; e = 255 gives 2^127, no NaN case)
MI355_HD constexpr bool nib32_has_e8(int t) { return t == T_MXFP4; }
MI355_HD constexpr uint32_t e8m0_half_bits(uint32_t e) { return e < 2 ? 0x00200000u << e : (e - 1) << 23; }

// ---- type sets the host code asks about (what a kernel implements is stated by that kernel's own *_applicable) ----
constexpr bool type_is_kq456(int t) { return t == T_Q4_K || t == T_Q5_K || t == T_Q6_K; }
// the ternary types: 256-weight blocks of codes 0..2 (weight = (code - 1) d) with one f16 scale, contracted against Q8_K
MI355_HD constexpr bool type_is_ternary(int t) { return t == T_TQ1_0 || t == T_TQ2_0; }
// reach the matrix cores only through their plane sets (no expand-on-the-fly kernel)
constexpr bool type_is_planes_only(int t) { return t == T_Q2_K || t == T_Q3_K || t == T_IQ4_XS || type_is_ternary(t); }
// the quantised weight types: contracted against a quantised copy of the activation (Q8_0 where act_is_q80, else Q8_K)
constexpr bool type_is_quant(int t) { return type_is_kq456(t) || type_is_planes_only(t) || act_is_q80(t); }
// blocks that are not 16-byte aligned on disk: the upload regroups each row into aligned planes (launch_repack_rows)
constexpr bool type_is_repacked(int t) { return t == T_Q6_K || type_is_planes_only(t) || act_is_q80(t); }
// a 32-element type other than Q8_0 that has an exact Q8_0-layout copy for the Q8_0 prompt kernel (Q4_0, Q5_0, IQ4_NL, Q4_1, Q5_1, MXFP4)
constexpr bool type_has_q80_copy(int t) { return act_is_q80(t) && t != T_Q8_0; }
// the row split's column cuts and exchange steps are untested with these: a file that holds one loads on one device only
constexpr bool type_row_split_unsupported(int t) { return nib32_has_min(t) || t == T_IQ4_XS || t == T_MXFP4 || type_is_ternary(t); }

// ---- device-resident weight row layouts --------------------------------------------------
// Q4_K / Q5_K rows stay in ggml order (144 / 176 B super-blocks are 16-B aligned: header | [qh] | qs).
// Q6_K (210 B) and Q8_0 (34 B) blocks are not 16-B aligned, so at upload each ROW is regrouped into
// aligned planes (same bytes, same total size up to padding):
//   Q6_K row: [ql: nb*128][qh: nb*64][scales: nb*16][d: nb*2] padded to 16
//   Q8_0 row: [qs: K][d: K/32*2] padded to 16
//   Q2_K row (84 B blocks: scales 16 | qs 64 | d | dmin):      [qs: nb*64][scales: nb*16][d, dmin: nb*4] padded to 16
//   Q3_K row (110 B blocks: hmask 32 | qs 64 | scales 12 | d): [hmask: nb*32][qs: nb*64][scales: nb*12][d: nb*2] padded to 16
//   Q4_0 / IQ4_NL row (18 B blocks: d | qs 16):              [qs: K/2][d: K/32*2] padded to 16
//   Q5_0 row (22 B blocks: d | qh 4 | qs 16):                 [qs: K/2][qh: K/32*4][d: K/32*2] padded to 16
//   Q4_1 row (20 B blocks: d | m | qs 16):                    [qs: K/2][d: K/32*2][m: K/32*2] padded to 16
//   Q5_1 row (24 B blocks: d | m | qh 4 | qs 16):             [qs: K/2][qh: K/32*4][d: K/32*2][m: K/32*2] padded to 16
//   MXFP4 row (17 B blocks: e | qs 16):                       [qs: K/2][e: K/32] padded to 16
//   IQ4_XS row (136 B blocks: d | scales_h 2 | scales_l 4 | qs 128): [qs: nb*128][scales_l: nb*4][scales_h: nb*2][d: nb*2] padded to 16
//   TQ2_0 row (66 B blocks: qs 64 | d):                       [qs: nb*64][d: nb*2] padded to 16
//   TQ1_0 row (54 B blocks: qs 48 | qh 4 | d):                [qs: nb*48][qh: nb*4][d: nb*2] padded to 16 (the file's packed trits, nothing wider)
// F16 / F32 rows are unchanged.  BF16 rows too: K is a multiple of 8 wherever the type is accepted, so a row is a whole number of the 16-byte pieces the
// bf16 kernels load (mmv_bf16.hip, mmf_bf16.hip) - no plane set, no second copy.
MI355_HD inline size_t dev_row_bytes(int t, int64_t K) {
    size_t b = ggml_row_bytes(t, K);
    return (b + 15) & ~(size_t)15;
}

}  // namespace mi355
