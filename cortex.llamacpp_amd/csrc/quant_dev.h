// quant_dev.h — wave-level activation quantisation shared by act.hip (stand-alone kernels) and mmvq.hip
// (fused RMSNorm + quantise prologue).  One wave quantises one 256-element block: lane l holds elements 4l..4l+3.
// Bit-identical to quantize_row_q8_K / quantize_row_q8_0 of the CPU backend.
#pragma once

#include "dev_common.h"

namespace mi355 {

// Q8_K: iscale = -127 / (signed value of the FIRST element with the largest magnitude); codes = min(127, rint(iscale*x));
// d = 1/iscale; bsum16 = sum of the 16-element group this lane belongs to (valid on every lane).
__device__ __forceinline__ void wave_quant_q8k(const float (&vv)[4], int lane, uint32_t &packed, int &bsum16, float &d) {
    // largest magnitude of the block (f32 max over the wave), then the FIRST element holding it: lowest lane whose own
    // first match exists (ballot + find-first-set), its value fetched with one v_readlane
    const float a0 = fabsf(vv[0]), a1 = fabsf(vv[1]), a2 = fabsf(vv[2]), a3 = fabsf(vv[3]);
    const float amax = wave_max(fmaxf(fmaxf(a0, a1), fmaxf(a2, a3)));
    const bool m0 = a0 == amax, m1 = a1 == amax, m2 = a2 == amax, m3 = a3 == amax;
    const float vsrc = m0 ? vv[0] : m1 ? vv[1] : m2 ? vv[2] : vv[3];
    const unsigned long long hit = __ballot(m0 || m1 || m2 || m3);
    const int src_lane = hit ? __builtin_ctzll(hit) : 0;
    const float vmax = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vsrc), src_lane));
    (void)lane;
    int qi[4] = {0, 0, 0, 0};
    d = 0.0f;
    if (amax != 0.0f) {
        const float iscale = -127.0f / vmax;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int t = __float2int_rn(iscale * vv[i]);
            qi[i] = t > 127 ? 127 : t;
        }
        d = 1.0f / iscale;
    }
    packed = (uint32_t)(qi[0] & 0xff) | ((uint32_t)(qi[1] & 0xff) << 8) | ((uint32_t)(qi[2] & 0xff) << 16) | ((uint32_t)(qi[3] & 0xff) << 24);
    int bs = qi[0] + qi[1] + qi[2] + qi[3];
    bs += dpp_i<DPP_QP_1032>(bs);       // 16 codes = 4 lanes = one quad
    bs += dpp_i<DPP_QP_2301>(bs);
    bsum16 = bs;
}

// N blocks of one wave at once (the weight stream's quantising prologue: up to ten 256-blocks per wave).  The same arithmetic block by block; the two IEEE
// divisions per block (-127 / max, 1 / iscale: ~10 instructions each, wave-uniform operands) are done ONCE for all blocks, block i's operand in lane i, and
// the quotients come back through v_readlane - the prologue is instruction-bound (8 waves x 7 blocks x ~80 instructions on an ffn_down launch).
template <int N>
__device__ __forceinline__ void wave_quant_q8k_batch(const float (&vv)[N][4], int lane, uint32_t (&packed)[N], int (&bsum16)[N], float (&d)[N]) {
    static_assert(N >= 1 && N <= 64, "one lane per block");
    bool nz[N];
    float vmax_l = 1.0f;                                       // lane i: block i's first element of the largest magnitude (1 where there is none)
#pragma unroll
    for (int i = 0; i < N; i++) {
        const float a0 = fabsf(vv[i][0]), a1 = fabsf(vv[i][1]), a2 = fabsf(vv[i][2]), a3 = fabsf(vv[i][3]);
        const float amax = wave_max(fmaxf(fmaxf(a0, a1), fmaxf(a2, a3)));
        const bool m0 = a0 == amax, m1 = a1 == amax, m2 = a2 == amax, m3 = a3 == amax;
        const float vsrc = m0 ? vv[i][0] : m1 ? vv[i][1] : m2 ? vv[i][2] : vv[i][3];
        const unsigned long long hit = __ballot(m0 || m1 || m2 || m3);
        const int src_lane = hit ? __builtin_ctzll(hit) : 0;
        const float vmax = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vsrc), src_lane));
        nz[i] = amax != 0.0f;
        if (lane == i && nz[i]) vmax_l = vmax;
    }
    const float iscale_l = -127.0f / vmax_l;
    const float d_l = 1.0f / iscale_l;
#pragma unroll
    for (int i = 0; i < N; i++) {
        int qi[4] = {0, 0, 0, 0};
        d[i] = 0.0f;
        if (nz[i]) {                                           // (wave-uniform)
            const float iscale = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(iscale_l), i));
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int t = __float2int_rn(iscale * vv[i][k]);
                qi[k] = t > 127 ? 127 : t;
            }
            d[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d_l), i));
        }
        packed[i] = (uint32_t)(qi[0] & 0xff) | ((uint32_t)(qi[1] & 0xff) << 8) | ((uint32_t)(qi[2] & 0xff) << 16) | ((uint32_t)(qi[3] & 0xff) << 24);
        int bs = qi[0] + qi[1] + qi[2] + qi[3];
        bs += dpp_i<DPP_QP_1032>(bs);
        bs += dpp_i<DPP_QP_2301>(bs);
        bsum16[i] = bs;
    }
}

// Q8_0: per 32 elements (8 lanes): d = amax/127, codes = roundf(x/d); d returned as f32 (store as f16)
__device__ __forceinline__ void wave_quant_q80(const float (&vv)[4], uint32_t &packed, float &d) {
    float am = fmaxf(fmaxf(fabsf(vv[0]), fabsf(vv[1])), fmaxf(fabsf(vv[2]), fabsf(vv[3])));
    am = fmaxf(am, dpp_f<DPP_QP_1032>(am));   // 32 values = 8 lanes
    am = fmaxf(am, dpp_f<DPP_QP_2301>(am));
    am = fmaxf(am, dpp_f<DPP_HALF_MIRROR>(am));
    d = am / 127.0f;
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    int qi[4];
#pragma unroll
    for (int i = 0; i < 4; i++) qi[i] = (int)roundf(vv[i] * id);
    packed = (uint32_t)(qi[0] & 0xff) | ((uint32_t)(qi[1] & 0xff) << 8) | ((uint32_t)(qi[2] & 0xff) << 16) | ((uint32_t)(qi[3] & 0xff) << 24);
}

// ---------------------------------------------------------------- dequantise one element of a device row
__device__ __forceinline__ void k4_scale_min(int j, const uint8_t *p, int &sc, int &mn) {
    if (j < 4) { sc = p[j] & 63; mn = p[j + 4] & 63; }
    else { sc = (p[j + 4] & 0x0f) | ((p[j - 4] >> 6) << 4); mn = (p[j + 4] >> 4) | ((p[j] >> 6) << 4); }
}

// IQ4_NL's code book (ggml-common.h kvalues_iq4nl): sixteen int8 levels, denser around zero
__device__ __forceinline__ int iq4nl_value(int nib) {
    // packed little-endian: levels 0-3, 4-7, 8-11, 12-15
    const uint32_t w = nib < 8 ? (nib < 4 ? 0xbfad9881u : 0xf6eaddcfu) : (nib < 12 ? 0x26190d01u : 0x71594535u);
    return (int)(int8_t)((w >> (8 * (nib & 3))) & 0xffu);
}

// four IQ4_NL levels (one int8 per byte) from four nibble indices (one per byte): two v_perm_b32 over the packed code book and a select on bit 3
__device__ __forceinline__ uint32_t iq4nl_levels4(uint32_t idx) {
    const uint32_t lo = __builtin_amdgcn_perm(0xf6eaddcfu, 0xbfad9881u, idx & 0x07070707u);
    const uint32_t hi = __builtin_amdgcn_perm(0x71594535u, 0x26190d01u, idx & 0x07070707u);
    const uint32_t m = ((idx >> 3) & 0x01010101u) * 0xffu;
    return (hi & m) | (lo & ~m);
}
// MXFP4's levels (kvalues_mxfp4: the e2m1 values doubled; index bit 3 is the sign): {0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12}
__device__ __forceinline__ int mxfp4_value(int nib) {
    const uint32_t w = nib < 8 ? (nib < 4 ? 0x03020100u : 0x0c080604u) : (nib < 12 ? 0xfdfeff00u : 0xf4f8fafcu);
    return (int)(int8_t)((w >> (8 * (nib & 3))) & 0xffu);
}
// four MXFP4 levels from four nibble indices, as iq4nl_levels4: 7 VALU operations per four weights (and, two v_perm_b32, shift, and, multiply, v_bfi_b32).
// The arithmetic decode of the e2m1 code (m < 4 ? m : (4 + 2 (m & 1)) << ((m >> 1) - 2), then the sign) has no packed-byte form here - there is no per-byte
// variable shift, compare or negate - so on four codes in one register it needs at least a compare mask (3), the two branches (2 + 4), a select (1) and a
// per-byte negate (xor, add with carries masked off: 4): 14 and more.  The lookup is the cheaper one and is used everywhere.
__device__ __forceinline__ uint32_t mxfp4_levels4(uint32_t idx) {
    const uint32_t lo = __builtin_amdgcn_perm(0x0c080604u, 0x03020100u, idx & 0x07070707u);
    const uint32_t hi = __builtin_amdgcn_perm(0xf4f8fafcu, 0xfdfeff00u, idx & 0x07070707u);
    const uint32_t m = ((idx >> 3) & 0x01010101u) * 0xffu;
    return (hi & m) | (lo & ~m);
}
// IQ4_XS: the 6-bit scale of sub-block ib (0..7) from the super-block's scales_l word (nibble ib) and scales_h (bit pair ib), minus 32
__device__ __forceinline__ int iq4xs_scale(uint32_t scales_l, uint32_t scales_h, int ib) {
    return (int)(((scales_l >> (4 * ib)) & 0xfu) | (((scales_h >> (2 * ib)) & 3u) << 4)) - 32;
}

// TQ1_0: a byte b holds five trits, trit n = ((uint8)(b * 3^n) * 3) >> 8 (the product wraps to 8 bits first), defined for all 256 byte values
__device__ __forceinline__ int tq1_trit(uint32_t b, int n) {
    const uint32_t p = n == 0 ? 1u : n == 1 ? 3u : n == 2 ? 9u : n == 3 ? 27u : 81u;
    return (int)((((b * p) & 0xffu) * 3u) >> 8);
}
// the same trit of the four bytes of a word, one code (0..2) per byte, p = 3^n: the bytes are multiplied two at a time in 16-bit lanes (255 * 81 and
// 255 * 3 stay below 2^16, so a lane never carries into its neighbour; 0x00ff00ff and p are 24-bit operands: v_mul_u32_u24).  12 VALU operations per four weights
__device__ __forceinline__ uint32_t tq1_codes4(uint32_t w, uint32_t p) {
    const uint32_t e = __umul24(__umul24(w & 0x00ff00ffu, p) & 0x00ff00ffu, 3u);            // bytes 0, 2: the trit sits in bits 8..9 of its lane
    const uint32_t o = __umul24(__umul24((w >> 8) & 0x00ff00ffu, p) & 0x00ff00ffu, 3u);     // bytes 1, 3
    return ((e >> 8) & 0x00030003u) | (o & 0x03000300u);
}
// byte and trit index of element r (0..255) of a TQ1_0 block: qs[0..31] hold elements 32 n + m, qs[32..47] elements 160 + 16 n + m, qh[0..3] elements 240 + 4 n + j
__device__ __forceinline__ void tq1_elem(int r, int &byte, int &n) {
    if (r < 160) { n = r >> 5; byte = r & 31; }
    else if (r < 240) { n = (r - 160) >> 4; byte = 32 + ((r - 160) & 15); }
    else { n = (r - 240) >> 2; byte = 48 + ((r - 240) & 3); }
}
// The mat-vec lane role of TQ1_0 (mmvq.hip, mmvq_fast_dev.h, the weight stream: one role, so the three agree bit for bit).  Lane v (0..7) of a super-block
// owns elements 32 v .. 32 v + 31, which the packing puts in ONE trit position of 16-byte pieces of the block:
//   v = 0..4 : trit v of qs[0..31]                                          q0 = qs[0..15], q1 = qs[16..31]
//   v = 5, 6 : trits 2 (v - 5) and 2 (v - 5) + 1 of qs[32..47]              q0 = q1 = qs[32..47]
//   v = 7    : trit 4 of qs[32..47], then trits 0..3 of the four qh bytes   q0 = qs[32..47], the qh word four times
// lo / hi: the activation codes 32 v .. + 15 and 32 v + 16 .. + 31.  Returns dot(codes, a) with codes 0..2; the caller subtracts the sum of the 32 a.
__device__ __forceinline__ unsigned tq1_piece0(int v) { return v < 5 ? 0u : 32u; }
__device__ __forceinline__ unsigned tq1_piece1(int v) { return v < 5 ? 16u : 32u; }
template <class V4>
__device__ __forceinline__ int tq1_lane_dot(const V4 &q0, const V4 &q1, uint32_t qh, int v, const V4 &lo, const V4 &hi) {
    const uint32_t p0 = (uint32_t)(0x510901511b090301ull >> (8 * v)) & 0xffu;       // 3^n of the lane's first trit position, per v
    const uint32_t p1 = (uint32_t)(0x011b03511b090301ull >> (8 * v)) & 0xffu;       // ... of its second one (v = 7: 3^0, the first of qh's)
    const bool tail = v == 7;
    int s = 0;
    s = dot4(tq1_codes4(q0.x, p0), lo.x, s); s = dot4(tq1_codes4(q0.y, p0), lo.y, s);
    s = dot4(tq1_codes4(q0.z, p0), lo.z, s); s = dot4(tq1_codes4(q0.w, p0), lo.w, s);
    s = dot4(tq1_codes4(tail ? qh : q1.x, p1), hi.x, s);
    s = dot4(tq1_codes4(tail ? qh : q1.y, tail ? 3u : p1), hi.y, s);
    s = dot4(tq1_codes4(tail ? qh : q1.z, tail ? 9u : p1), hi.z, s);
    s = dot4(tq1_codes4(tail ? qh : q1.w, tail ? 27u : p1), hi.w, s);
    return s;
}

__device__ __forceinline__ float dequant_elem(int type, const uint8_t *row, int K, int e) {
    switch (type) {
        case T_F32: return reinterpret_cast<const float *>(row)[e];
        case T_F16: return h2f(reinterpret_cast<const uint16_t *>(row)[e]);
        case T_BF16: return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t *>(row)[e] << 16);   // the upper half of an f32: exact for every bit pattern
        // the 32-element types: the type is a run-time value and the offsets come from K, not from a block count, so they are spelled out - written as
        // plane_off<>() they compile to other code.  Planes (kTypeLayouts, ggml_types.h): Q8_0 qs [K] | d; the nibble types qs [K / 2] | [qh] | d | [m]; MXFP4 qs | e
        case T_Q8_0: {
            const float d = h2f(*reinterpret_cast<const uint16_t *>(row + K + (e >> 5) * 2));
            return __fmul_rn((float)(int8_t)row[e], d);
        }
        case T_Q4_0: case T_IQ4_NL: case T_Q5_0: {   // element r of block b: nibble r / 16 of qs[16 b + r % 16]; Q5_0: bit r of qh is the fifth bit
            const int b = e >> 5, r = e & 31, nblk = K >> 5;
            const int nib = (row[(size_t)b * 16 + (r & 15)] >> (4 * (r >> 4))) & 0x0f;
            const size_t half = (size_t)K >> 1;
            if (type == T_Q5_0) {
                const uint32_t qh = *reinterpret_cast<const uint32_t *>(row + half + (size_t)b * 4);
                const float d = h2f(*reinterpret_cast<const uint16_t *>(row + half + (size_t)nblk * 4 + (size_t)b * 2));
                return __fmul_rn((float)((nib | (int)(((qh >> r) & 1u) << 4)) - 16), d);
            }
            const float d = h2f(*reinterpret_cast<const uint16_t *>(row + half + (size_t)b * 2));
            if (type == T_Q4_0) return __fmul_rn((float)(nib - 8), d);
            return __fmul_rn(d, (float)iq4nl_value(nib));
        }
        case T_MXFP4: {   // dequantize_row_mxfp4: y = level * d, one product; d from the block's E8M0 byte
            const int b = e >> 5, r = e & 31;
            const int nib = (row[(size_t)b * 16 + (r & 15)] >> (4 * (r >> 4))) & 0x0f;
            return __fmul_rn((float)mxfp4_value(nib), e8f(row[((size_t)K >> 1) + (size_t)b]));
        }
        case T_Q4_1: case T_Q5_1: {   // the same nibble field with unsigned codes and a per-block minimum: y = q d + m, the product rounded before the add
            const int b = e >> 5, r = e & 31;
            int q = (row[(size_t)b * 16 + (r & 15)] >> (4 * (r >> 4))) & 0x0f;
            const size_t half = (size_t)K >> 1, doff = nib32_d_off(type, (size_t)K);
            if (type == T_Q5_1) q |= (int)(((*reinterpret_cast<const uint32_t *>(row + half + (size_t)b * 4) >> r) & 1u) << 4);
            const float d = h2f(*reinterpret_cast<const uint16_t *>(row + doff + (size_t)b * 2));
            const float m = h2f(*reinterpret_cast<const uint16_t *>(row + doff + (size_t)(K >> 5) * 2 + (size_t)b * 2));
            return __fadd_rn(__fmul_rn((float)q, d), m);
        }
        case T_Q4_K: case T_Q5_K: {
            const int bsz = type == T_Q4_K ? 144 : 176;
            const uint8_t *b = row + (size_t)(e >> 8) * bsz;
            const int r = e & 255, j = r >> 5, l = r & 31, c = j >> 1;
            const float d = h2f(*reinterpret_cast<const uint16_t *>(b)), dm = h2f(*reinterpret_cast<const uint16_t *>(b + 2));
            int sc, mn;
            k4_scale_min(j, b + 4, sc, mn);
            const uint8_t *qs = b + (type == T_Q4_K ? 16 : 48);
            int q = (j & 1) ? (qs[32 * c + l] >> 4) : (qs[32 * c + l] & 0x0f);
            if (type == T_Q5_K && ((b[16 + l] >> j) & 1)) q += 16;
            return __fsub_rn(__fmul_rn(__fmul_rn(d, (float)sc), (float)q), __fmul_rn(dm, (float)mn));
        }
        case T_Q2_K: {   // element (n, j, l) of block sb: bits 2 j .. 2 j + 1 of qs[32 n + l]; sub-block is = 8 n + 2 j + l / 16
            const int nb = K >> 8, sb = e >> 8, r = e & 255, n = r >> 7, j = (r >> 5) & 3, l = r & 31, is = 8 * n + 2 * j + (l >> 4);
            const uint8_t q = row[(size_t)sb * 64 + 32 * n + l], sc = row[plane_off<T_Q2_K, q2k::P_SCALES>((size_t)nb) + (size_t)sb * 16 + is];
            const uint16_t *dm = reinterpret_cast<const uint16_t *>(row + plane_off<T_Q2_K, q2k::P_DM>((size_t)nb) + (size_t)sb * 4);
            const float dl = __fmul_rn(h2f(dm[0]), (float)(sc & 0xf)), ml = __fmul_rn(h2f(dm[1]), (float)(sc >> 4));
            return __fsub_rn(__fmul_rn(dl, (float)((q >> (2 * j)) & 3)), ml);
        }
        case T_Q3_K: {
            const int nb = K >> 8, sb = e >> 8, r = e & 255, n = r >> 7, j = (r >> 5) & 3, l = r & 31, is = 8 * n + 2 * j + (l >> 4);
            const uint8_t q = row[plane_off<T_Q3_K, q3k::P_QS>((size_t)nb) + (size_t)sb * 64 + 32 * n + l], hm = row[(size_t)sb * 32 + l];
            const uint8_t *s12 = row + plane_off<T_Q3_K, q3k::P_SCALES>((size_t)nb) + (size_t)sb * 12;
            const int low = is < 8 ? (s12[is] & 0xf) : (s12[is - 8] >> 4), high = (s12[8 + (is & 3)] >> (2 * (is >> 2))) & 3;
            const float d = h2f(*reinterpret_cast<const uint16_t *>(row + plane_off<T_Q3_K, q3k::P_D>((size_t)nb) + (size_t)sb * 2));
            const int code = (int)((q >> (2 * j)) & 3) - (((hm >> (4 * n + j)) & 1) ? 0 : 4);
            return __fmul_rn(__fmul_rn(d, (float)((low | (high << 4)) - 32)), (float)code);
        }
        case T_IQ4_XS: {   // element j of sub-block ib: nibble j / 16 of qs[16 ib + j % 16]; dequantize_row_iq4_xs: dl = d * (ls - 32), y = dl * level
            const int nb = K >> 8, sb = e >> 8, r = e & 255, ib = r >> 5, j = r & 31;
            const int nib = (row[(size_t)sb * 128 + 16 * ib + (j & 15)] >> (4 * (j >> 4))) & 0x0f;
            const uint32_t sl = *reinterpret_cast<const uint32_t *>(row + plane_off<T_IQ4_XS, iq4xs::P_SCALES_L>((size_t)nb) + (size_t)sb * 4);
            const uint32_t sh = *reinterpret_cast<const uint16_t *>(row + plane_off<T_IQ4_XS, iq4xs::P_SCALES_H>((size_t)nb) + (size_t)sb * 2);
            const float d = h2f(*reinterpret_cast<const uint16_t *>(row + plane_off<T_IQ4_XS, iq4xs::P_D>((size_t)nb) + (size_t)sb * 2));
            return __fmul_rn(__fmul_rn(d, (float)iq4xs_scale(sl, sh, ib)), (float)iq4nl_value(nib));
        }
        case T_TQ2_0: {   // element 128 h + 32 l + m: bits 2 l .. 2 l + 1 of qs[32 h + m]; dequantize_row_tq2_0: y = (q - 1) * d (a product: - 0.0 where it gives one)
            const int nb = K >> 8, sb = e >> 8, r = e & 255;
            const int q = (row[(size_t)sb * 64 + 32 * (r >> 7) + (r & 31)] >> (2 * ((r >> 5) & 3))) & 3;
            return __fmul_rn((float)(q - 1), h2f(*reinterpret_cast<const uint16_t *>(row + plane_off<T_TQ2_0, tq2::P_D>((size_t)nb) + (size_t)sb * 2)));
        }
        case T_TQ1_0: {
            const int nb = K >> 8, sb = e >> 8;
            int byte, n;
            tq1_elem(e & 255, byte, n);
            const uint32_t b = byte < 48 ? row[(size_t)sb * 48 + byte] : row[plane_off<T_TQ1_0, tq1::P_QH>((size_t)nb) + (size_t)sb * 4 + (byte - 48)];
            return __fmul_rn((float)(tq1_trit(b, n) - 1), h2f(*reinterpret_cast<const uint16_t *>(row + plane_off<T_TQ1_0, tq1::P_D>((size_t)nb) + (size_t)sb * 2)));
        }
        case T_Q6_K: {
            const int nb = K >> 8, sb = e >> 8, r = e & 255, n = r >> 7, rr = r & 127, k = rr >> 5, l = rr & 31;
            const uint8_t *ql = row + (size_t)sb * 128 + n * 64, *qh = row + plane_off<T_Q6_K, q6k::P_QH>((size_t)nb) + (size_t)sb * 64 + n * 32;
            const int8_t *sc = reinterpret_cast<const int8_t *>(row + plane_off<T_Q6_K, q6k::P_SCALES>((size_t)nb) + (size_t)sb * 16 + n * 8);
            const float d = h2f(*reinterpret_cast<const uint16_t *>(row + plane_off<T_Q6_K, q6k::P_D>((size_t)nb) + (size_t)sb * 2));
            const int lo = (k & 1) ? ql[l + 32] : ql[l];
            const int nib = (k & 2) ? (lo >> 4) : (lo & 0x0f);
            const int q = (nib | (((qh[l] >> (2 * k)) & 3) << 4)) - 32;
            return __fmul_rn(__fmul_rn(d, (float)sc[2 * k + (l >> 4)]), (float)q);
        }
    }
    return 0.0f;
}


}  // namespace mi355
