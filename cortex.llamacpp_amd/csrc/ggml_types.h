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
#define MI355_INLINE __attribute__((always_inline))

namespace mi355 {

// ggml type ids (GGUF on-disk values)
enum : int {
    T_F32 = 0, T_F16 = 1, T_Q4_0 = 2, T_Q4_1 = 3, T_Q5_0 = 6, T_Q5_1 = 7, T_Q8_0 = 8, T_Q2_K = 10, T_Q3_K = 11, T_Q4_K = 12, T_Q5_K = 13, T_Q6_K = 14, T_Q8_K = 15, T_IQ4_NL = 20, T_IQ4_XS = 23, T_BF16 = 30, T_TQ1_0 = 34, T_TQ2_0 = 35, T_MXFP4 = 39,
};

// ---- one row per known type: the on-disk block, and the planes of its device row ---------
// A plane is one field of the on-disk block, gathered over the blocks of a row: {where the field starts in the block, its bytes}.  The planes are listed in
// device order; a type without planes is uploaded as the file holds it.
struct BlockField { int off, bytes; };
struct TypeLayout {
    int id;
    const char *name;
    int block_elems, block_bytes;
    int n_planes;
    BlockField planes[4];
};
constexpr TypeLayout kTypeLayouts[] = {
    {T_F32, "f32", 1, 4, 0, {}},
    {T_F16, "f16", 1, 2, 0, {}},
    {T_BF16, "bf16", 1, 2, 0, {}},
    {T_Q4_K, "q4_K", 256, 144, 0, {}},
    {T_Q5_K, "q5_K", 256, 176, 0, {}},
    {T_Q8_K, "q8_K", 256, 292, 0, {}},                                         // an activation format, never a file type
    {T_Q4_0, "q4_0", 32, 18, 2, {{2, 16}, {0, 2}}},                            // d | qs            -> qs | d
    {T_IQ4_NL, "iq4_nl", 32, 18, 2, {{2, 16}, {0, 2}}},                        // d | qs            -> qs | d
    {T_Q4_1, "q4_1", 32, 20, 3, {{4, 16}, {0, 2}, {2, 2}}},                    // d | m | qs        -> qs | d | m
    {T_Q5_0, "q5_0", 32, 22, 3, {{6, 16}, {2, 4}, {0, 2}}},                    // d | qh | qs       -> qs | qh | d
    {T_Q5_1, "q5_1", 32, 24, 4, {{8, 16}, {4, 4}, {0, 2}, {2, 2}}},            // d | m | qh | qs   -> qs | qh | d | m
    {T_Q8_0, "q8_0", 32, 34, 2, {{2, 32}, {0, 2}}},                            // d | qs            -> qs | d
    {T_MXFP4, "mxfp4", 32, 17, 2, {{1, 16}, {0, 1}}},                          // e | qs            -> qs | e
    {T_Q2_K, "q2_K", 256, 84, 3, {{16, 64}, {0, 16}, {80, 4}}},                // scales | qs | d, dmin       -> qs | scales | (d, dmin)
    {T_Q3_K, "q3_K", 256, 110, 4, {{0, 32}, {32, 64}, {96, 12}, {108, 2}}},    // hmask | qs | scales | d     -> the same order
    {T_Q6_K, "q6_K", 256, 210, 4, {{0, 128}, {128, 64}, {192, 16}, {208, 2}}}, // ql | qh | scales | d        -> the same order
    {T_IQ4_XS, "iq4_xs", 256, 136, 4, {{8, 128}, {4, 4}, {2, 2}, {0, 2}}},     // d | scales_h | scales_l | qs -> qs | scales_l | scales_h | d
    {T_TQ1_0, "tq1_0", 256, 54, 3, {{0, 48}, {48, 4}, {52, 2}}},               // qs | qh | d                 -> the same order (the file's packed trits)
    {T_TQ2_0, "tq2_0", 256, 66, 2, {{0, 64}, {64, 2}}},                        // qs | d                      -> the same order
    {-1, "unknown", 0, 0, 0, {}},                                              // what an id without a row gets
};
constexpr int N_TYPE_LAYOUTS = (int)(sizeof(kTypeLayouts) / sizeof(kTypeLayouts[0])) - 1;
MI355_HD constexpr const TypeLayout &type_layout(int t) {
    int i = 0;
    while (i < N_TYPE_LAYOUTS && kTypeLayouts[i].id != t) i++;
    return kTypeLayouts[i];
}
// plane indices of each repacked type, in device order
namespace q6k { enum : int { P_QL, P_QH, P_SCALES, P_D }; }
namespace q2k { enum : int { P_QS, P_SCALES, P_DM }; }
namespace q3k { enum : int { P_HMASK, P_QS, P_SCALES, P_D }; }
namespace iq4xs { enum : int { P_QS, P_SCALES_L, P_SCALES_H, P_D }; }
namespace tq1 { enum : int { P_QS, P_QH, P_D }; }
namespace tq2 { enum : int { P_QS, P_D }; }
namespace q80 { enum : int { P_QS, P_D }; }

MI355_HD constexpr int ggml_block_elems(int t) { return type_layout(t).block_elems; }
MI355_HD constexpr int ggml_block_bytes(int t) { return type_layout(t).block_bytes; }
MI355_HD constexpr const char *ggml_type_name(int t) { return type_layout(t).name; }
// bytes of the whole blocks in n elements on disk; 0 for an unknown type
MI355_HD constexpr size_t ggml_row_bytes(int t, int64_t n) {
    return ggml_block_elems(t) == 0 ? 0 : (size_t)(n / ggml_block_elems(t)) * (size_t)ggml_block_bytes(t);
}
// byte offset of plane p in a device row of n_blocks blocks (the type's own blocks: K / 256 or K / 32); p = n_planes gives the unpadded row size
MI355_HD constexpr size_t plane_off(int t, int p, size_t n_blocks) {
    int before = 0;
    for (int i = 0; i < p; i++) before += type_layout(t).planes[i].bytes;
    return n_blocks * (size_t)before;
}
// the same with the type and the plane as template arguments, for the kernels: the bytes per block are a constant before the optimiser sees the call, so a
// decoder compiles to what it compiled to with the number written out.  N: size_t, or unsigned where a kernel keeps its LDS offsets in 32 bits
template <int T, int P, typename N> MI355_HD MI355_INLINE constexpr N plane_off(N n_blocks) {
    static_assert((N)-1 > (N)0 && sizeof(N) >= 4, "the block count as size_t or unsigned");
    constexpr N per_block = (N)plane_off(T, P, 1);
    return n_blocks * per_block;
}

// the CPU backend's activation format for a weight type: Q8_0 blocks for the 32-element formats, Q8_K for the K-quants
MI355_HD constexpr bool act_is_q80(int t) { return ggml_block_elems(t) == 32; }
// the 32-element nibble formats: a fifth-bit word per block (Q5_0, Q5_1); a per-block f16 minimum m, weight = q d + m with q unsigned (Q4_1, Q5_1)
MI355_HD constexpr bool nib32_has_qh(int t) { return t == T_Q5_0 || t == T_Q5_1; }
MI355_HD constexpr bool nib32_has_min(int t) { return t == T_Q4_1 || t == T_Q5_1; }
// their planes are qs | [qh] | d | [m]
namespace nib32 { enum : int { P_QS, P_QH }; }
MI355_HD constexpr int nib32_p_d(int t) { return nib32_has_qh(t) ? 2 : 1; }
MI355_HD constexpr int nib32_p_m(int t) { return nib32_p_d(t) + 1; }
// the d plane's offset from the row length K, for the decoders that have K and a run-time type and no block count (asserted against the table below)
MI355_HD constexpr size_t nib32_d_off(int t, size_t K) { return (K >> 1) + (nib32_has_qh(t) ? (K >> 5) * 4 : 0); }
// MXFP4: the block scale is one E8M0 byte e, kept as that byte (plane mxfp4::P_E behind the nibbles) and turned into an f32 where it is used:
// half of 2^(e - 127) as a bit pattern, exact for every e (e < 2 gives the two subnormals 2^-128 and 2^-127; e = 255 gives 2^127, no NaN case)
MI355_HD constexpr bool nib32_has_e8(int t) { return t == T_MXFP4; }
namespace mxfp4 { enum : int { P_QS, P_E }; }
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
constexpr bool type_is_repacked(int t) { return type_layout(t).n_planes > 0; }
// a 32-element type other than Q8_0 that has an exact Q8_0-layout copy for the Q8_0 prompt kernel (Q4_0, Q5_0, IQ4_NL, Q4_1, Q5_1, MXFP4)
constexpr bool type_has_q80_copy(int t) { return act_is_q80(t) && t != T_Q8_0; }
// the row split's column cuts and exchange steps are untested with these: a file that holds one loads on one device only
constexpr bool type_row_split_unsupported(int t) { return nib32_has_min(t) || t == T_IQ4_XS || t == T_MXFP4 || type_is_ternary(t); }

// ---- device-resident weight row layouts --------------------------------------------------
// A block that is not 16-byte aligned on disk (Q6_K 210 B, Q8_0 34 B, ...) cannot be read with aligned 16-byte loads, so at upload each ROW of such a type is
// regrouped into planes (kTypeLayouts above; launch_repack_rows): the same bytes, every plane contiguous over the row's blocks, the row padded to 16.
// Q4_K / Q5_K rows stay in ggml order (144 / 176 B super-blocks are 16-B aligned: header | [qh] | qs); F16 / F32 rows are unchanged.  BF16 rows too: K is a
// multiple of 8 wherever the type is accepted, so a row is a whole number of the 16-byte pieces the bf16 kernels load (mmv_bf16.hip, mmf_bf16.hip) - no plane
// set, no second copy.
MI355_HD constexpr size_t dev_row_bytes(int t, int64_t K) { return (ggml_row_bytes(t, K) + 15) & ~(size_t)15; }

// every repacked type's fields are disjoint and cover its block exactly: the planes, taken in block order, follow each other from 0 to the block's size
constexpr bool planes_tile_block(const TypeLayout &r) {
    int at = 0;
    for (int n = 0; n < r.n_planes; n++) {
        int next = -1;
        for (int i = 0; i < r.n_planes; i++)
            if (r.planes[i].off == at && r.planes[i].bytes > 0) next = i;
        if (next < 0) return false;
        at += r.planes[next].bytes;
    }
    return r.n_planes == 0 || at == r.block_bytes;
}
constexpr bool all_layouts_sound() {
    for (int i = 0; i < N_TYPE_LAYOUTS; i++) {
        const TypeLayout &r = kTypeLayouts[i];
        if (!planes_tile_block(r) || r.block_elems <= 0 || r.block_bytes <= 0) return false;
        if (r.n_planes && plane_off(r.id, r.n_planes, 1) != (size_t)r.block_bytes) return false;
        if (&type_layout(r.id) != &r) return false;                  // no id twice
    }
    return true;
}
static_assert(all_layouts_sound(), "kTypeLayouts: a repacked type's planes must be disjoint fields that cover its block");
static_assert(plane_off(T_IQ4_XS, iq4xs::P_D, 3) == 402 && plane_off(T_Q5_1, nib32_p_m(T_Q5_1), 3) == 66, "plane_off");
constexpr bool nib32_d_off_is_the_tables(int t) { return nib32_d_off(t, 96) == plane_off(t, nib32_p_d(t), 3) && plane_off(t, 1, 3) == 48; }
static_assert(nib32_d_off_is_the_tables(T_Q4_0) && nib32_d_off_is_the_tables(T_IQ4_NL) && nib32_d_off_is_the_tables(T_Q5_0) && nib32_d_off_is_the_tables(T_Q4_1) &&
              nib32_d_off_is_the_tables(T_Q5_1) && plane_off(T_MXFP4, mxfp4::P_E, 3) == 48, "the 32-element decoders' spelled-out offsets (K / 2, nib32_d_off)");

}  // namespace mi355
