// quant_error.hip — the weights of a GGUF file back as floats, and the error of one set of weights against another (what upstream's
// llama-quantize-stats measures per tensor).  One decoder, decode4<T>, for every loadable weight type, reading the file's own blocks (ggml layout, no plane
// set: the bytes of the file uploaded as they are), behind three launch forms:
//   decode : blocks of T -> F32 or F16 (nearest even) rows
//   error  : reference rows (F32 / F16 / BF16) against blocks of T -> per row sum e^2, sum w^2, sum c_j e_j^2, max |e|, in f64
//   error, two block sets : the same reduction with the reference rows decoded from blocks of another type
// The value of an element is the f32 that ggml's dequantize_row_* gives: the same products in the same order, none contracted with a sum.
//
// Shape of the work, as quantize.hip has it.  A wave owns 256 adjacent elements: one super-block, eight blocks of a 32-element type, 256 values of F32 / F16 /
// BF16.  Lane l owns elements 4 l .. 4 l + 3; a workgroup is four waves.
//   decode : the rows are one flat run of elements (a row is whole blocks, so the blocks of consecutive rows follow each other), wave c owns elements
//     256 c ..: with rows of 288 a wave straddles a row end, which a decoder does not notice.  The last wave of a call is ragged and guarded.
//   error  : a sum has an order, and the bits must not depend on where a call's first row lies in its tensor - so here the waves are cut at the row ends:
//     wave w of row r owns elements 256 w .. of that row, the last wave of every row is ragged (guarded, its absent lanes add + 0.0), and the slab of partials
//     is [n_rows][waves per row][4].  A lane's row is its wave's.
// Staging.  A block is not 16-byte aligned on disk (Q6_K 210 B, Q8_0 34 B, TQ1_0 54 B, MXFP4 17 B), so a wave's blocks are not either.  The wave copies the
//   16-byte pieces that cover its blocks into LDS with aligned 16-byte loads (at most 19: eight Q8_0 blocks are 272 bytes), keeping the bytes' offset inside
//   the first piece, and its lanes decode from LDS with byte and 16-bit reads.  F32 / F16 / BF16 elements are aligned where they lie and are loaded directly.
// Sums.  A lane forms its four terms in f64 from the f32 values and adds them left to right; the wave's sum is wave_sum(double) of dev_common.h (DPP
//   butterflies inside each row of 16 lanes, then the four row totals (r0 + r1) + (r2 + r3)); a second kernel, one thread per row, adds the row's partials in
//   index order.  No atomics: the bits depend on the types and n_per_row alone.  A non-finite reference value counts as 0 and sets the row's flag (every writer
//   stores the same 1).
#include "dev_common.h"
#include "kernels.h"
#include "quant_dev.h"

namespace mi355 {

namespace {
constexpr int QE_WAVES = 4;              // waves (256-element chunks) of a workgroup
constexpr int QE_CHUNK_MAX = 272;        // bytes of the widest staged chunk: eight Q8_0 blocks
constexpr int QE_STAGE = 304;            // its covering 16-byte pieces: up to 15 bytes before and after it
constexpr int T_ANY = -2;                // a kernel's type argument that is read at run time
static_assert(QE_STAGE % 16 == 0 && QE_STAGE >= QE_CHUNK_MAX + 30 && QE_STAGE / 16 <= 64, "one piece per lane");

template <int T> struct TypeTag { static constexpr int value = T; };
// f(TypeTag<t>) for a decodable type t; false for any other id (Q8_K among them: an activation format)
template <typename F> __host__ __device__ __forceinline__ bool for_type(int t, F &&f) {
    switch (t) {
#define QE_CASE(T) case T: f(TypeTag<T>{}); return true;
        QE_CASE(T_F32) QE_CASE(T_F16) QE_CASE(T_BF16) QE_CASE(T_Q4_0) QE_CASE(T_Q4_1) QE_CASE(T_Q5_0) QE_CASE(T_Q5_1) QE_CASE(T_Q8_0) QE_CASE(T_Q2_K)
        QE_CASE(T_Q3_K) QE_CASE(T_Q4_K) QE_CASE(T_Q5_K) QE_CASE(T_Q6_K) QE_CASE(T_IQ4_NL) QE_CASE(T_IQ4_XS) QE_CASE(T_TQ1_0) QE_CASE(T_TQ2_0) QE_CASE(T_MXFP4)
#undef QE_CASE
    }
    return false;
}

constexpr bool is_float_type(int t) { return t == T_F32 || t == T_F16 || t == T_BF16; }
// where field P of type T starts in its on-disk block (kTypeLayouts)
template <int T, int P> constexpr int FO = type_layout(T).planes[P].off;
// Q4_K and Q5_K have no plane set (their blocks are 16-byte aligned): d | dmin | scales[12] | [qh[32]] | qs[128].  The fields behind the two halves, and qs
// counted back from the block's end
constexpr int K45_DMIN = 2, K45_SCALES = 4, K5_QH = K45_SCALES + 12;
template <int T> constexpr int K45_QS = ggml_block_bytes(T) - 128;
static_assert(K45_QS<T_Q4_K> == K5_QH && K45_QS<T_Q5_K> == K5_QH + 32, "Q4_K / Q5_K fields");

// ---- LDS reads: 16 bits at an even address, 32 bits as two of them, 32 bits at any address
__device__ __forceinline__ uint32_t rd16(const uint8_t *p) { return *reinterpret_cast<const uint16_t *>(p); }
__device__ __forceinline__ uint32_t rd32(const uint8_t *p) { return rd16(p) | rd16(p + 2) << 16; }
__device__ __forceinline__ uint32_t rd32b(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
__device__ __forceinline__ float rdh(const uint8_t *p) { return h2f((uint16_t)rd16(p)); }
__device__ __forceinline__ int byte_of(uint32_t w, int i) { return (int)((w >> (8 * i)) & 0xffu); }

// ---- the wave's blocks into LDS: blocks first .. first + n of type T from `g` (16-byte aligned; readable up to the next multiple of 16 behind its last
// block).  Returns where the first block's first byte lies in `lds`; the caller's barrier makes it readable.  A block of an even size starts at an even address
template <int T> __device__ __forceinline__ const uint8_t *stage_blocks(const uint8_t *g, size_t first, int n, uint8_t *lds, int lane) {
    constexpr int BB = ggml_block_bytes(T);
    static_assert(256 / ggml_block_elems(T) * BB <= QE_CHUNK_MAX, "a chunk's bytes");
    const size_t b0 = first * BB, a0 = b0 & ~(size_t)15;
    const int skew = (int)(b0 - a0), n_piece = n > 0 ? (skew + n * BB + 15) >> 4 : 0;
    if (lane < n_piece) reinterpret_cast<uint4 *>(lds)[lane] = *reinterpret_cast<const uint4 *>(g + a0 + 16 * (size_t)lane);
    return lds + skew;
}

// ---- the lane's four elements (first element e0, a multiple of 4) of F32 / F16 / BF16 rows
template <int T> __device__ __forceinline__ void load4f(const void *src, size_t e0, float y[4]) {
    if constexpr (T == T_F32) {
        const float4 v = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(src) + e0);
        y[0] = v.x; y[1] = v.y; y[2] = v.z; y[3] = v.w;
    } else {
        const uint2 v = *reinterpret_cast<const uint2 *>(reinterpret_cast<const uint16_t *>(src) + e0);
        if constexpr (T == T_F16) {
            y[0] = h2f((uint16_t)(v.x & 0xffffu)); y[1] = h2f((uint16_t)(v.x >> 16)); y[2] = h2f((uint16_t)(v.y & 0xffffu)); y[3] = h2f((uint16_t)(v.y >> 16));
        } else {                                               // bf16 is the upper half of an f32: exact for every bit pattern
            y[0] = __uint_as_float(v.x << 16); y[1] = __uint_as_float(v.x & 0xffff0000u); y[2] = __uint_as_float(v.y << 16); y[3] = __uint_as_float(v.y & 0xffff0000u);
        }
    }
}

// ---- decode4<T>: elements 4 lane .. 4 lane + 3 of the wave's 256, from its staged blocks s (ggml's on-disk layout)
template <int T> __device__ __forceinline__ void decode4(const uint8_t *s, int lane, float y[4]) {
    constexpr int BB = ggml_block_bytes(T);
    if constexpr (T == T_Q8_0) {                               // y = q d
        const uint8_t *b = s + BB * (lane >> 3);
        const float d = rdh(b + FO<T, q80::P_D>);
        const uint32_t q = rd32(b + FO<T, q80::P_QS> + 4 * (lane & 7));
#pragma unroll
        for (int i = 0; i < 4; i++) y[i] = __fmul_rn((float)(int8_t)byte_of(q, i), d);
    } else if constexpr (ggml_block_elems(T) == 32) {
        // the nibble types: element j of a block is the low nibble of qs[j] (j < 16) or the high nibble of qs[j - 16]; bit j of qh is its fifth bit
        const uint8_t *b = s + BB * (lane >> 3);
        const int j0 = 4 * (lane & 7);
        const uint8_t *qp = b + FO<T, nib32::P_QS> + (j0 & 15);
        const uint32_t q = ((BB & 1 ? rd32b(qp) : rd32(qp)) >> (4 * (j0 >> 4))) & 0x0f0f0f0fu;
        int c[4];
#pragma unroll
        for (int i = 0; i < 4; i++) c[i] = byte_of(q, i);
        if constexpr (nib32_has_qh(T)) {
            const uint32_t qh = rd32(b + FO<T, nib32::P_QH>) >> j0;
#pragma unroll
            for (int i = 0; i < 4; i++) c[i] |= (int)((qh >> i) & 1u) << 4;
        }
        if constexpr (T == T_MXFP4) {                          // y = level * d, d = half of 2^(e - 127) from the block's E8M0 byte
            const float d = e8f(b[FO<T, mxfp4::P_E>]);
#pragma unroll
            for (int i = 0; i < 4; i++) y[i] = __fmul_rn((float)mxfp4_value(c[i]), d);
        } else {
            const float d = rdh(b + FO<T, nib32_p_d(T)>);
            if constexpr (nib32_has_min(T)) {                  // Q4_1, Q5_1: y = q d + m, the product rounded before the sum
                const float m = rdh(b + FO<T, nib32_p_m(T)>);
#pragma unroll
                for (int i = 0; i < 4; i++) y[i] = __fadd_rn(__fmul_rn((float)c[i], d), m);
            } else if constexpr (T == T_IQ4_NL) {              // y = d * kvalues_iq4nl[q]
#pragma unroll
                for (int i = 0; i < 4; i++) y[i] = __fmul_rn(d, (float)iq4nl_value(c[i]));
            } else {                                           // Q4_0: y = (q - 8) d; Q5_0: y = (q - 16) d
                static_assert(T == T_Q4_0 || T == T_Q5_0, "a 32-element type without a decoder");
#pragma unroll
                for (int i = 0; i < 4; i++) y[i] = __fmul_rn((float)(c[i] - (T == T_Q4_0 ? 8 : 16)), d);
            }
        }
    } else if constexpr (T == T_Q4_K || T == T_Q5_K) {
        // sub-block j (32 elements) has the 6-bit scale and minimum j of scales[12] (k4_scale_min); its codes are the low (j even) or high nibbles of
        // qs[32 (j / 2) ..], Q5_K's fifth bit is bit j of qh[l]:  y = (d sc) q - (dmin m)
        const int r = 4 * lane, j = r >> 5, l = r & 31;
        int sc, mn;
        k4_scale_min(j, s + K45_SCALES, sc, mn);
        const float d1 = __fmul_rn(rdh(s), (float)sc), m1 = __fmul_rn(rdh(s + K45_DMIN), (float)mn);
        const uint32_t q = (rd32(s + K45_QS<T> + 32 * (j >> 1) + l) >> (4 * (j & 1))) & 0x0f0f0f0fu;
        uint32_t h = 0;
        if constexpr (T == T_Q5_K) h = ((rd32(s + K5_QH + l) >> j) & 0x01010101u) << 4;
#pragma unroll
        for (int i = 0; i < 4; i++) y[i] = __fsub_rn(__fmul_rn(d1, (float)byte_of(q | h, i)), m1);
    } else if constexpr (T == T_Q2_K) {
        // element 128 n + 32 j + l: bits 2 j, 2 j + 1 of qs[32 n + l]; scales[8 n + 2 j + l / 16] holds the 4-bit scale (low) and minimum (high) of its sixteen:
        // y = (d sc) q - (dmin m)
        const int r = 4 * lane, n = r >> 7, j = (r >> 5) & 3, l = r & 31;
        const uint32_t scm = s[FO<T, q2k::P_SCALES> + 8 * n + 2 * j + (l >> 4)];
        const float dl = __fmul_rn(rdh(s + FO<T, q2k::P_DM>), (float)(scm & 15u)), ml = __fmul_rn(rdh(s + FO<T, q2k::P_DM> + 2), (float)(scm >> 4));
        const uint32_t q = (rd32(s + FO<T, q2k::P_QS> + 32 * n + l) >> (2 * j)) & 0x03030303u;
#pragma unroll
        for (int i = 0; i < 4; i++) y[i] = __fsub_rn(__fmul_rn(dl, (float)byte_of(q, i)), ml);
    } else if constexpr (T == T_Q3_K) {
        // the same 2-bit field; bit 4 n + j of hmask[l] CLEAR subtracts 4.  The sixteen 6-bit scales in scales[12]: scale is has its low four bits in the low
        // (is < 8) or high nibble of scales[is % 8] and its upper two in bits 2 (is / 4) of scales[8 + is % 4]:  y = (d (sc - 32)) (q - (hbit ? 0 : 4))
        const int r = 4 * lane, n = r >> 7, j = (r >> 5) & 3, l = r & 31, is = 8 * n + 2 * j + (l >> 4);
        const uint8_t *s12 = s + FO<T, q3k::P_SCALES>;
        const int low = is < 8 ? (s12[is] & 15) : (s12[is - 8] >> 4), high = (s12[8 + (is & 3)] >> (2 * (is >> 2))) & 3;
        const float dl = __fmul_rn(rdh(s + FO<T, q3k::P_D>), (float)((low | (high << 4)) - 32));
        const uint32_t q = (rd32(s + FO<T, q3k::P_QS> + 32 * n + l) >> (2 * j)) & 0x03030303u;
        const uint32_t hm = (rd32(s + FO<T, q3k::P_HMASK> + l) >> (4 * n + j)) & 0x01010101u;
#pragma unroll
        for (int i = 0; i < 4; i++) y[i] = __fmul_rn(dl, (float)(byte_of(q, i) - (byte_of(hm, i) ? 0 : 4)));
    } else if constexpr (T == T_Q6_K) {
        // element 128 n + 32 k + l: the low (k < 2) or high nibble of ql[64 n + 32 (k & 1) + l], upper two bits at 2 k of qh[32 n + l]; the int8 scale of its
        // sixteen is scales[8 n + 2 k + l / 16]:  y = (d sc) (q - 32)
        const int r = 4 * lane, n = r >> 7, k = (r >> 5) & 3, l = r & 31;
        const float dl = __fmul_rn(rdh(s + FO<T, q6k::P_D>), (float)(int8_t)s[FO<T, q6k::P_SCALES> + 8 * n + 2 * k + (l >> 4)]);
        const uint32_t lo = (rd32(s + FO<T, q6k::P_QL> + 64 * n + 32 * (k & 1) + l) >> (4 * (k >> 1))) & 0x0f0f0f0fu;
        const uint32_t hi = ((rd32(s + FO<T, q6k::P_QH> + 32 * n + l) >> (2 * k)) & 0x03030303u) << 4;
#pragma unroll
        for (int i = 0; i < 4; i++) y[i] = __fmul_rn(dl, (float)(byte_of(lo | hi, i) - 32));
    } else if constexpr (T == T_IQ4_XS) {
        // element j of sub-block ib: nibble j / 16 of qs[16 ib + j % 16]; the 6-bit scale ls of ib: nibble ib of scales_l, bit pair ib of scales_h:
        // y = (d (ls - 32)) kvalues_iq4nl[q]
        const int r = 4 * lane, ib = r >> 5, j0 = r & 31;
        const int ls = iq4xs_scale(rd32(s + FO<T, iq4xs::P_SCALES_L>), rd16(s + FO<T, iq4xs::P_SCALES_H>), ib);
        const float dl = __fmul_rn(rdh(s + FO<T, iq4xs::P_D>), (float)ls);
        const uint32_t q = (rd32(s + FO<T, iq4xs::P_QS> + 16 * ib + (j0 & 15)) >> (4 * (j0 >> 4))) & 0x0f0f0f0fu;
#pragma unroll
        for (int i = 0; i < 4; i++) y[i] = __fmul_rn(dl, (float)iq4nl_value(byte_of(q, i)));
    } else if constexpr (T == T_TQ2_0) {                       // element 128 h + 32 l + m: bits 2 l, 2 l + 1 of qs[32 h + m]:  y = (q - 1) d
        const int r = 4 * lane;
        const float d = rdh(s + FO<T, tq2::P_D>);
        const uint32_t q = (rd32(s + FO<T, tq2::P_QS> + 32 * (r >> 7) + (r & 31)) >> (2 * ((r >> 5) & 3))) & 0x03030303u;
#pragma unroll
        for (int i = 0; i < 4; i++) y[i] = __fmul_rn((float)(byte_of(q, i) - 1), d);
    } else {
        // TQ1_0: five base-3 digits per byte (four in a qh byte), digit n of byte b = ((uint8)(b 3^n) 3) >> 8 (tq1_trit); which byte and digit an element has:
        // tq1_elem.  qh follows qs in the block, so the byte index is an offset from qs:  y = (digit - 1) d
        static_assert(T == T_TQ1_0 && FO<T, tq1::P_QH> == FO<T, tq1::P_QS> + 48, "a type without a decoder");
        const float d = rdh(s + FO<T, tq1::P_D>);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            int byte, n;
            tq1_elem(4 * lane + i, byte, n);
            y[i] = __fmul_rn((float)(tq1_trit(s[FO<T, tq1::P_QS> + byte], n) - 1), d);
        }
    }
}

// ---- one operand of a wave: the rows `base` of type T, the wave's first element at e_first (a multiple of its block), n of its 256 elements present.
// stage(): the blocks into LDS (nothing for F32 / F16 / BF16); after the barrier, get(): the lane's four values, 4 lane < n
template <int T> struct Operand {
    static constexpr bool FLOATS = is_float_type(T);
    const uint8_t *s = nullptr;
    __device__ __forceinline__ void stage(const void *base, size_t e_first, int n, uint8_t *lds, int lane) {
        if constexpr (!FLOATS) s = stage_blocks<T>(reinterpret_cast<const uint8_t *>(base), e_first / ggml_block_elems(T), n / ggml_block_elems(T), lds, lane);
    }
    __device__ __forceinline__ void get(const void *base, size_t e_first, int lane, float y[4]) const {
        if constexpr (FLOATS) load4f<T>(base, e_first + 4 * (size_t)lane, y); else decode4<T>(s, lane, y);
    }
};
// the same with the type read at run time (wave-uniform: one scalar branch)
template <> struct Operand<T_ANY> {
    const uint8_t *s = nullptr;
    int t;
    __device__ __forceinline__ void stage(const void *base, size_t e_first, int n, uint8_t *lds, int lane) {
        for_type(t, [&](auto tag) { Operand<decltype(tag)::value> o; o.stage(base, e_first, n, lds, lane); s = o.s; });
    }
    __device__ __forceinline__ void get(const void *base, size_t e_first, int lane, float y[4]) const {
        for_type(t, [&](auto tag) { Operand<decltype(tag)::value> o; o.s = s; o.get(base, e_first, lane, y); });
    }
};

// ---- decode: the flat run of n_total elements -> dst, F32 or (H) F16
template <int T, bool H>
__global__ __launch_bounds__(QE_WAVES * 64) void decode_kernel(const void *__restrict__ src, int64_t n_total, void *__restrict__ dst) {
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[QE_WAVES][QE_STAGE];
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const int64_t chunk = (int64_t)blockIdx.x * QE_WAVES + wv, left = n_total - chunk * 256;
    const int n = left >= 256 ? 256 : left > 0 ? (int)left : 0;
    const size_t e_first = (size_t)chunk * 256;
    Operand<T> op;
    op.stage(src, e_first, n, s_stage[wv], lane);
    if constexpr (!Operand<T>::FLOATS) __syncthreads();
    const bool have = 4 * lane < n;
    float y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (have) op.get(src, e_first, lane, y);
    const size_t e0 = e_first + 4 * (size_t)lane;
    if constexpr (H) {
        // a lane's four halves are 8 bytes: the even lane of a pair stores both lanes' 16 where its neighbour has elements, else its own 8
        const uint32_t a = (uint32_t)f2h(y[0]) | (uint32_t)f2h(y[1]) << 16, b = (uint32_t)f2h(y[2]) | (uint32_t)f2h(y[3]) << 16;
        const uint32_t na = (uint32_t)dpp_i<DPP_QP_1032>((int)a), nb = (uint32_t)dpp_i<DPP_QP_1032>((int)b);
        uint16_t *o = reinterpret_cast<uint16_t *>(dst) + e0;
        if (have && !(lane & 1)) {
            if (4 * (lane + 1) < n) *reinterpret_cast<uint4 *>(o) = uint4{a, b, na, nb};
            else *reinterpret_cast<uint2 *>(o) = uint2{a, b};
        }
    } else if (have) {
        *reinterpret_cast<float4 *>(reinterpret_cast<float *>(dst) + e0) = float4{y[0], y[1], y[2], y[3]};
    }
}

__device__ __forceinline__ double wave_max(double v) {
    v = fmax(v, dpp_d(v, 0)); v = fmax(v, dpp_d(v, 1)); v = fmax(v, dpp_d(v, 2)); v = fmax(v, dpp_d(v, 3));
    return fmax(fmax(readlane_d(v, 0), readlane_d(v, 16)), fmax(readlane_d(v, 32), readlane_d(v, 48)));
}

// ---- error: wave g of the call is wave g % wpr of row g / wpr; its four partial sums go to partial[g][4]
struct ErrorArgs {
    const void *ref, *cand;
    const float *cw;                     // n_per_row column weights, or nullptr: 1
    int rt, ct;                          // the types, for the kernel that reads them at run time
    int64_t n_per_row;
    uint32_t wpr, n_waves;               // waves per row; of the call
    double *partial;
    int32_t *row_flag;
};

template <int RT, int CT> __global__ __launch_bounds__(QE_WAVES * 64) void error_kernel(const ErrorArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[2][QE_WAVES][QE_STAGE];
    const int lane = (int)(threadIdx.x & 63), wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t g = blockIdx.x * QE_WAVES + (uint32_t)wv;
    const bool wave_in = g < a.n_waves;
    const uint32_t row = g / a.wpr, w = g - row * a.wpr;
    const int64_t left = a.n_per_row - (int64_t)w * 256;
    const int n = !wave_in ? 0 : left >= 256 ? 256 : (int)left;
    const size_t e_first = (size_t)row * (size_t)a.n_per_row + (size_t)w * 256;
    Operand<RT> ref;
    Operand<CT> cand;
    if constexpr (RT == T_ANY) { ref.t = a.rt; cand.t = a.ct; }
    ref.stage(a.ref, e_first, n, s_stage[0][wv], lane);
    cand.stage(a.cand, e_first, n, s_stage[1][wv], lane);
    __syncthreads();

    double e2 = 0.0, w2 = 0.0, ce2 = 0.0, mx = 0.0;
    if (4 * lane < n) {
        float x[4], y[4], c[4] = {1.0f, 1.0f, 1.0f, 1.0f};
        ref.get(a.ref, e_first, lane, x);
        cand.get(a.cand, e_first, lane, y);
        if (a.cw) load4f<T_F32>(a.cw, (size_t)w * 256 + 4 * (size_t)lane, c);
        bool bad = false;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (!(fabsf(x[i]) <= 3.4028234664e38f)) { bad = true; x[i] = 0.0f; }
            const double xd = (double)x[i], e = xd - (double)y[i], t = e * e;
            e2 += t; w2 += xd * xd; ce2 += (double)c[i] * t;      // (0.0 + the first term is that term: left to right)
            mx = fmax(mx, fabs(e));
        }
        if (bad) a.row_flag[row] = 1;
    }
    e2 = wave_sum(e2); w2 = wave_sum(w2); ce2 = wave_sum(ce2); mx = wave_max(mx);
    if (wave_in && lane < 4) a.partial[(size_t)g * 4 + lane] = lane == 0 ? e2 : lane == 1 ? w2 : lane == 2 ? ce2 : mx;
}

// a row's partials in index order: thread per row
__global__ __launch_bounds__(256) void error_rows_kernel(const double *__restrict__ partial, uint32_t wpr, int64_t n_rows, double *__restrict__ out) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const double *p = partial + (size_t)row * wpr * 4;
    double e2 = 0.0, w2 = 0.0, ce2 = 0.0, mx = 0.0;
    for (uint32_t w = 0; w < wpr; w++) { e2 += p[4 * w]; w2 += p[4 * w + 1]; ce2 += p[4 * w + 2]; mx = fmax(mx, p[4 * w + 3]); }
    double *o = out + (size_t)row * 4;
    o[0] = e2; o[1] = w2; o[2] = ce2; o[3] = mx;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
// n_per_row is whole blocks of t and whole lanes (four elements: F32 / F16 / BF16 rows of any multiple of 4)
bool row_fits(int t, int64_t n_per_row) { return n_per_row >= 1 && n_per_row % ggml_block_elems(t) == 0 && n_per_row % 4 == 0; }
}  // namespace

bool quant_error_type_supported(int t) { return for_type(t, [](auto) {}); }

size_t quant_error_partial_doubles(int64_t n_per_row, int64_t n_rows) { return (size_t)((n_per_row + 255) / 256) * (size_t)n_rows * 4; }

hipError_t launch_dequantize_rows(int src_type, const void *blocks, int64_t n_per_row, int64_t n_rows, int dst_type, void *dst, hipStream_t st) {
    if (!quant_error_type_supported(src_type) || (dst_type != T_F32 && dst_type != T_F16) || !blocks || !dst || n_rows < 1 || !row_fits(src_type, n_per_row) ||
        n_rows > ((int64_t)1 << 40) / n_per_row || !aligned16(blocks) || !aligned16(dst)) return hipErrorInvalidValue;
    const int64_t n_total = n_per_row * n_rows, chunks = (n_total + 255) / 256;
    if (chunks > (int64_t)0x7fffffff * QE_WAVES) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((chunks + QE_WAVES - 1) / QE_WAVES)), block(QE_WAVES * 64);
    for_type(src_type, [&](auto tag) {
        constexpr int T = decltype(tag)::value;
        if (dst_type == T_F16) hipLaunchKernelGGL((decode_kernel<T, true>), grid, block, 0, st, blocks, n_total, dst);
        else hipLaunchKernelGGL((decode_kernel<T, false>), grid, block, 0, st, blocks, n_total, dst);
    });
    return hipGetLastError();
}

hipError_t launch_quant_error_rows(int ref_type, const void *ref, int q_type, const void *blocks, int64_t n_per_row, int64_t n_rows, const float *col_weights,
                                   double *partial, int32_t *row_flags, double *out, hipStream_t st) {
    if (!quant_error_type_supported(ref_type) || !quant_error_type_supported(q_type) || !ref || !blocks || !partial || !row_flags || !out || n_rows < 1 ||
        !row_fits(ref_type, n_per_row) || !row_fits(q_type, n_per_row) || n_rows > ((int64_t)1 << 40) / n_per_row) return hipErrorInvalidValue;
    if (!aligned16(ref) || !aligned16(blocks) || !aligned16(col_weights) || !aligned16(partial) || !aligned16(out)) return hipErrorInvalidValue;
    const int64_t wpr = (n_per_row + 255) / 256;
    if (wpr * n_rows > (int64_t)0x7fffffff - QE_WAVES) return hipErrorInvalidValue;
    ErrorArgs a{ref, blocks, col_weights, ref_type, q_type, n_per_row, (uint32_t)wpr, (uint32_t)(wpr * n_rows), partial, row_flags};
    const dim3 grid((a.n_waves + QE_WAVES - 1) / QE_WAVES), block(QE_WAVES * 64);
    // rows that are floats on the reference side - a source file against its quantisation - have a kernel per pair of types; two block sets share one that
    // reads both types at run time
    if (is_float_type(ref_type)) {
        for_type(q_type, [&](auto tag) {
            constexpr int CT = decltype(tag)::value;
            if (ref_type == T_F32) hipLaunchKernelGGL((error_kernel<T_F32, CT>), grid, block, 0, st, a);
            else if (ref_type == T_F16) hipLaunchKernelGGL((error_kernel<T_F16, CT>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((error_kernel<T_BF16, CT>), grid, block, 0, st, a);
        });
    } else {
        hipLaunchKernelGGL((error_kernel<T_ANY, T_ANY>), grid, block, 0, st, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(error_rows_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, partial, a.wpr, n_rows, out);
    return hipGetLastError();
}

}  // namespace mi355
