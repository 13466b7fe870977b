// lora_merge.hip — merge LoRA adapters into base weight rows: out[n][k] = round( deq(W)[n][k] + sum_i s_i * sum_j B_i[n][j] * A_i[j][k] ) for up to
// LORA_MERGE_MAX_AD adapters, W being N rows of K elements as the GGUF file holds them (ggml block layout, no plane set), A_i [r_i][K], B_i [N][r_i],
// 1 <= r_i <= 512, each pair F16 or F32, out F16 or F32.  The counterpart of llama-export-lora's ggml graph, as a rank-r update on the matrix cores.
//
// Split.  A workgroup of four waves owns one 128 x 128 tile of out (n x k) and walks the rank of every adapter; a wave owns 64 x 64 of it as 2 x 2 matrix
//   tiles of 32 x 32.  The matrix instruction's row dimension is k and its column dimension is n, so a lane ends up with consecutive k of ONE output row:
//   v_mfma_f32_32x32x16_f16 for an F16 pair (the products of two halves are exact in f32, the sums are f32), v_mfma_f32_32x32x2_f32 for an F32 pair (nothing
//   of an F32 pair is rounded to f16).
// LDS.  A stage is 64 bytes of rank per row (32 halves or 16 floats): the B panel [128 n][64 B] as it lies in memory, the A panel transposed to [128 k][64 B]
//   (a thread loads eight k of two ranks - of one rank for f32 - and writes eight dwords), rows padded to 80 bytes: sixteen consecutive rows' 16-byte reads
//   fall into sixteen different bank quads.  The A panel's rows are stored permuted (panel_row) so that the lanes of a matrix tile read CONSECUTIVE LDS rows
//   and still own eight consecutive k between the wave's two k tiles: register 4 q + e of k tile i, lane half kg, is k = 16 q + 8 kg + 4 i + e.
//   Two buffers: a stage's global loads are issued into registers before the stage in LDS is multiplied and written to the other buffer after it; one
//   barrier per stage.  A rank that is no multiple of the stage, a row past N and a column past K are zeros in LDS: the multiply loop has no branch.
// Arithmetic.  Each adapter's products are summed into a set of f32 accumulators of its own, and acc += s_i * that when its rank is done: one f32 product and
//   one f32 sum per adapter and element.  (Scaling the B panel of an F16 pair while it is staged would round s_i * B to f16, 2^-11 of every term; the
//   bound the kernel is tested against is 2 r 2^-24 of the terms' magnitudes.)  Epilogue: the lane decodes its eight base weights from the file's blocks
//   EXACTLY into f64 (every supported block's value is a sum of two products of small integers and halves), adds the accumulator in f64 and rounds once to
//   the out type - to f16 through an f32 rounded to odd, so that a scale of 0 gives the correctly rounded dequantised base and an F16 base its own bytes.
//   One 16-byte store (f16) or two (f32) per lane and eight elements; K is a multiple of 8, so a piece is whole or absent.
// No atomics, no workgroup waits for another, nothing is written outside out[0 .. N)[0 .. K), the same call gives the same bits.
#include "kernels.h"
#include "quant_dev.h"

namespace mi355 {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int LM_THREADS = 256, LM_TILE = 128, LM_ROW = 80, LM_PANEL = LM_TILE * LM_ROW;   // bytes of a padded panel row; of a panel

struct LoraMergeLaunch {
    LoraMergeAdapter ad[LORA_MERGE_MAX_AD];
    int n_ad;
    const uint8_t *W;
    int base_type, out_type;
    int N, K;
    size_t w_row_bytes;
    void *out;
};

// LDS row of local k (0..127) in the A panel
__device__ __forceinline__ int panel_row(int kl) { return (kl & 64) + 32 * ((kl >> 2) & 1) + 4 * ((kl >> 3) & 7) + (kl & 3); }

// 16 bytes of a row whose start may have any element alignment: elements [j, j + EP) of `row` (r elements), zeros past r
template <bool H> __device__ __forceinline__ uint4 load_b_piece(const uint8_t *row, int j, int r, bool vec) {
    constexpr int EP = H ? 8 : 4;
    uint4 v = {0u, 0u, 0u, 0u};
    if (vec && j + EP <= r) return *reinterpret_cast<const uint4 *>(row + (size_t)j * (H ? 2 : 4));
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < EP; e++)
        if (j + e < r) {
            if (H) w[e >> 1] |= (uint32_t)reinterpret_cast<const uint16_t *>(row)[j + e] << (16 * (e & 1));
            else w[e] = reinterpret_cast<const uint32_t *>(row)[j + e];
        }
    v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    return v;
}

// the registers of one stage on its way from memory to LDS
struct StageRegs { uint4 a[2], b[2]; };

// stage at rank j0: B rows n0 .. n0 + 127, A columns k0 .. k0 + 127
template <bool H> __device__ __forceinline__ void stage_load(const LoraMergeAdapter &ad, int j0, int n0, int k0, int N, int K, StageRegs &s) {
    constexpr int ES = H ? 2 : 4, EP = 16 / ES;
    const int tid = threadIdx.x, r = ad.r;
    const bool vec = ((size_t)r * ES) % 16 == 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int p = tid + h * LM_THREADS, n = n0 + (p >> 2), j = j0 + (p & 3) * EP;
        s.b[h] = uint4{0u, 0u, 0u, 0u};
        if (n < N && j < r) s.b[h] = load_b_piece<H>(reinterpret_cast<const uint8_t *>(ad.B) + (size_t)n * r * ES, j, r, vec);
    }
    // A: eight k of ranks j0 + 2 jp and + 1 (f16: a[0], a[1]) or of rank j0 + jp (f32: a[0] | a[1])
    const int jp = (tid >> 2) & 15, k = k0 + 8 * (4 * (tid >> 6) + (tid & 3));
    s.a[0] = s.a[1] = uint4{0u, 0u, 0u, 0u};
    if (k < K) {
        if (H) {
#pragma unroll
            for (int h = 0; h < 2; h++)
                if (j0 + 2 * jp + h < r) s.a[h] = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(ad.A) + (size_t)(j0 + 2 * jp + h) * K + k);
        } else if (j0 + jp < r) {
            const uint4 *src = reinterpret_cast<const uint4 *>(reinterpret_cast<const float *>(ad.A) + (size_t)(j0 + jp) * K + k);
            s.a[0] = src[0]; s.a[1] = src[1];
        }
    }
}

template <bool H> __device__ __forceinline__ void stage_store(const StageRegs &s, uint8_t *sA, uint8_t *sB) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int p = tid + h * LM_THREADS;
        *reinterpret_cast<uint4 *>(sB + (p >> 2) * LM_ROW + (p & 3) * 16) = s.b[h];
    }
    const int jp = (tid >> 2) & 15, kp = 4 * (tid >> 6) + (tid & 3);
    const uint32_t a0[4] = {s.a[0].x, s.a[0].y, s.a[0].z, s.a[0].w}, a1[4] = {s.a[1].x, s.a[1].y, s.a[1].z, s.a[1].w};
#pragma unroll
    for (int e = 0; e < 8; e++) {
        uint32_t w;
        if (H) {                                               // halves e of the two ranks, the lower rank in the lower half
            const uint32_t lo = (a0[e >> 1] >> (16 * (e & 1))) & 0xffffu, hi = (a1[e >> 1] >> (16 * (e & 1))) & 0xffffu;
            w = lo | (hi << 16);
        } else w = e < 4 ? a0[e] : a1[e - 4];
        *reinterpret_cast<uint32_t *>(sA + panel_row(8 * kp + e) * LM_ROW + 4 * jp) = w;
    }
}

// the stage in LDS against the wave's 2 x 2 tiles
template <bool H> __device__ __forceinline__ void stage_mul(const uint8_t *sA, const uint8_t *sB, f32x16 (&t)[2][2]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 31, kg = lane >> 5;
    const uint8_t *pa = sA + (64 * (wave >> 1) + m) * LM_ROW, *pb = sB + (64 * (wave & 1) + m) * LM_ROW;
    if (H) {
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            f16x8 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; i++) {
                a[i] = *reinterpret_cast<const f16x8 *>(pa + 32 * i * LM_ROW + 32 * ks + 16 * kg);
                b[i] = *reinterpret_cast<const f16x8 *>(pb + 32 * i * LM_ROW + 32 * ks + 16 * kg);
            }
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) t[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], b[j], t[i][j], 0, 0, 0);
        }
    } else {                                                   // step ks of lane half kg is rank 8 kg + ks of the stage, on both sides
        f32x4 a[2][2], b[2][2];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int h = 0; h < 2; h++) {
                a[i][h] = *reinterpret_cast<const f32x4 *>(pa + 32 * i * LM_ROW + 32 * kg + 16 * h);
                b[i][h] = *reinterpret_cast<const f32x4 *>(pb + 32 * i * LM_ROW + 32 * kg + 16 * h);
            }
#pragma unroll
        for (int ks = 0; ks < 8; ks++)
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) t[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][ks >> 2][ks & 3], b[j][ks >> 2][ks & 3], t[i][j], 0, 0, 0);
    }
}

// one adapter: acc += scale * (B A) over the workgroup's tile
template <bool H>
__device__ __forceinline__ void merge_adapter(const LoraMergeAdapter &ad, int n0, int k0, int N, int K, uint8_t *lds, f32x16 (&acc)[2][2]) {
    constexpr int JS = H ? 32 : 16;
    f32x16 t[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int q = 0; q < 16; q++) t[i][j][q] = 0.0f;
    const int n_stage = (ad.r + JS - 1) / JS;
    StageRegs s;
    stage_load<H>(ad, 0, n0, k0, N, K, s);
    stage_store<H>(s, lds, lds + LM_PANEL);
    __syncthreads();
    for (int st = 0; st < n_stage; st++) {
        uint8_t *cur = lds + (st & 1) * 2 * LM_PANEL, *nxt = lds + ((st + 1) & 1) * 2 * LM_PANEL;
        stage_load<H>(ad, (st + 1) * JS, n0, k0, N, K, s);      // past the last stage: every rank is >= r, so zeros and no load
        stage_mul<H>(cur, cur + LM_PANEL, t);
        stage_store<H>(s, nxt, nxt + LM_PANEL);
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int q = 0; q < 16; q++) acc[i][j][q] = acc[i][j][q] + ad.scale * t[i][j][q];
}

// eight bytes at an even address
__device__ __forceinline__ uint64_t load8_u16(const uint8_t *p) {
    const uint16_t *h = reinterpret_cast<const uint16_t *>(p);
    return (uint64_t)h[0] | ((uint64_t)h[1] << 16) | ((uint64_t)h[2] << 32) | ((uint64_t)h[3] << 48);
}

// elements k .. k + 7 (k % 8 == 0) of a row in file layout, exactly
__device__ __forceinline__ void decode8(int type, const uint8_t *row, int k, double (&v)[8]) {
    switch (type) {
        case T_F32: {
            const float *p = reinterpret_cast<const float *>(row) + k;
            const f32x4 x = *reinterpret_cast<const f32x4 *>(p), y = *reinterpret_cast<const f32x4 *>(p + 4);
#pragma unroll
            for (int e = 0; e < 4; e++) { v[e] = (double)x[e]; v[4 + e] = (double)y[e]; }
            return;
        }
        case T_F16: case T_BF16: {
            const uint4 u = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(row) + k);
            const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const uint16_t h = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
                v[e] = (double)(type == T_F16 ? h2f(h) : __uint_as_float((uint32_t)h << 16));
            }
            return;
        }
        case T_Q8_0: {                                          // d | qs[32], 34 bytes
            const uint8_t *b = row + (size_t)(k >> 5) * 34;
            const double d = (double)h2f(*reinterpret_cast<const uint16_t *>(b));
            const uint64_t q = load8_u16(b + 2 + (k & 31));
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = d * (double)(int8_t)(q >> (8 * e));
            return;
        }
        case T_Q4_K: case T_Q5_K: {                             // d | dmin | scales[12] | [qh[32]] | qs[128]: 144 / 176 bytes, 16-byte aligned
            const uint8_t *b = row + (size_t)(k >> 8) * (type == T_Q4_K ? 144 : 176);
            const int rr = k & 255, j = rr >> 5, l = rr & 31;
            int sc, mn;
            k4_scale_min(j, b + 4, sc, mn);
            const double d = (double)h2f(*reinterpret_cast<const uint16_t *>(b)) * (double)sc, m = (double)h2f(*reinterpret_cast<const uint16_t *>(b + 2)) * (double)mn;
            const uint2 qs = *reinterpret_cast<const uint2 *>(b + (type == T_Q4_K ? 16 : 48) + 32 * (j >> 1) + l);
            const uint64_t q = ((uint64_t)qs.y << 32) | qs.x;
            uint64_t h = 0;
            if (type == T_Q5_K) { const uint2 qh = *reinterpret_cast<const uint2 *>(b + 16 + l); h = ((uint64_t)qh.y << 32) | qh.x; }
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int nib = (int)(q >> (8 * e + 4 * (j & 1))) & 15, hb = (int)(h >> (8 * e + j)) & 1;
                v[e] = d * (double)(nib + 16 * hb) - m;
            }
            return;
        }
        case T_Q6_K: {                                          // ql[128] | qh[64] | scales[16] | d: 210 bytes, 2-byte aligned
            const uint8_t *b = row + (size_t)(k >> 8) * 210;
            const int rr = k & 255, n = rr >> 7, c = (rr & 127) >> 5, l = rr & 31;
            const uint64_t ql = load8_u16(b + 64 * n + l + 32 * (c & 1)), qh = load8_u16(b + 128 + 32 * n + l);
            const double d = (double)h2f(*reinterpret_cast<const uint16_t *>(b + 208)) * (double)reinterpret_cast<const int8_t *>(b + 192)[8 * n + 2 * c + (l >> 4)];
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int nib = (int)(ql >> (8 * e + 4 * (c >> 1))) & 15, hi = (int)(qh >> (8 * e + 2 * c)) & 3;
                v[e] = d * (double)((nib | (hi << 4)) - 32);
            }
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = 0.0;
}

// f64 -> f32 rounded to odd: the f32 -> f16 rounding that follows is then the correct rounding of the f64 value
__device__ __forceinline__ float f64_to_f32_odd(double x) {
    const float f = (float)x;
    const double back = (double)f;
    if (back == x || !(fabsf(f) < __builtin_inff())) return f;
    uint32_t u = __float_as_uint(f);
    if (fabs(back) > fabs(x)) u -= 1;                          // back to the truncated value
    return __uint_as_float(u | 1u);
}

__global__ __launch_bounds__(LM_THREADS) void lora_merge_kernel(const LoraMergeLaunch a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2 * 2 * LM_PANEL];
    const int k0 = (int)blockIdx.x * LM_TILE, n0 = (int)blockIdx.y * LM_TILE;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int q = 0; q < 16; q++) acc[i][j][q] = 0.0f;
    for (int i = 0; i < a.n_ad; i++) {
        if (a.ad[i].type == T_F16) merge_adapter<true>(a.ad[i], n0, k0, a.N, a.K, lds, acc);
        else merge_adapter<false>(a.ad[i], n0, k0, a.N, a.K, lds, acc);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 31, kg = lane >> 5;
#pragma unroll
    for (int jn = 0; jn < 2; jn++) {
        const int n = n0 + 64 * (wave & 1) + 32 * jn + m;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = k0 + 64 * (wave >> 1) + 16 * q + 8 * kg;
            if (n >= a.N || k >= a.K) continue;
            double v[8];
            decode8(a.base_type, a.W + (size_t)n * a.w_row_bytes, k, v);
#pragma unroll
            for (int e = 0; e < 8; e++) {                      // (a zero update leaves the base as it is, a -0.0 included)
                const float u = acc[e >> 2][jn][4 * q + (e & 3)];
                v[e] = u == 0.0f ? v[e] : v[e] + (double)u;
            }
            const size_t at = (size_t)n * a.K + k;
            if (a.out_type == T_F16) {
                uint32_t w[4];
#pragma unroll
                for (int e = 0; e < 4; e++) w[e] = (uint32_t)f2h(f64_to_f32_odd(v[2 * e])) | ((uint32_t)f2h(f64_to_f32_odd(v[2 * e + 1])) << 16);
                *reinterpret_cast<uint4 *>(reinterpret_cast<uint16_t *>(a.out) + at) = uint4{w[0], w[1], w[2], w[3]};
            } else {
                f32x4 *dst = reinterpret_cast<f32x4 *>(reinterpret_cast<float *>(a.out) + at);
                dst[0] = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
                dst[1] = f32x4{(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
            }
        }
    }
}

}  // namespace

bool lora_merge_base_supported(int t) { return t == T_F32 || t == T_F16 || t == T_BF16 || t == T_Q8_0 || t == T_Q4_K || t == T_Q5_K || t == T_Q6_K; }

hipError_t launch_lora_merge(int base_type, const void *W, int64_t N, int64_t K, const LoraMergeAdapter *ads, int n_ad, int out_type, void *out, hipStream_t st) {
    if (!lora_merge_base_supported(base_type) || (out_type != T_F16 && out_type != T_F32) || !W || !out || !ads || n_ad < 1 || n_ad > LORA_MERGE_MAX_AD) return hipErrorInvalidValue;
    const int be = ggml_block_elems(base_type);
    if (N < 1 || K < 8 || (K % 8) != 0 || (K % be) != 0 || K > ((int64_t)1 << 30) || N > (int64_t)65535 * LM_TILE || N > ((int64_t)1 << 40) / K) return hipErrorInvalidValue;
    if (((uintptr_t)W | (uintptr_t)out) % 16 != 0) return hipErrorInvalidValue;
    LoraMergeLaunch a{};
    for (int i = 0; i < n_ad; i++) {
        const LoraMergeAdapter &d = ads[i];
        if ((d.type != T_F16 && d.type != T_F32) || d.r < 1 || d.r > LORA_MAX_R || !d.A || !d.B || ((uintptr_t)d.A | (uintptr_t)d.B) % 16 != 0) return hipErrorInvalidValue;
        a.ad[i] = d;
    }
    a.n_ad = n_ad; a.W = reinterpret_cast<const uint8_t *>(W); a.base_type = base_type; a.out_type = out_type; a.N = (int)N; a.K = (int)K;
    a.w_row_bytes = ggml_row_bytes(base_type, K); a.out = out;
    hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)((K + LM_TILE - 1) / LM_TILE), (unsigned)((N + LM_TILE - 1) / LM_TILE)), dim3(LM_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace mi355
