// mmq_q80.hip — prompt batches against Q8_0 weights on the matrix cores (mul_mat_q for Q8_0).
//
//   out[t][r] = sum over 32-blocks b of  (float)isum_b * (d_w[r][b] * d_a[t][b]),   isum_b = sum_{k in b} w[r][k] * a[t][k]
//
// exactly ggml_vec_dot_q8_0_q8_0: integer block sums, one f32 multiply-add per block, blocks added in order — so unlike
// the K-quant kernels (whose super-block sums are re-associated) this one reproduces the CPU result bit for bit.
//
// v_mfma_i32_32x32x32_i8 contracts K = 32 per instruction = one Q8_0 block: A = 32 tokens x 32 codes (lane = token
// lane & 31, k-half lane >> 5, 16 bytes straight from the activation plane), B = 32 weight rows x 32 codes (lane = row,
// k-half; 16 bytes straight from the device row [codes K][scales K/32]).  The result tile holds 16 tokens of one weight
// row per lane, so d_w is a per-lane scalar and the 16 activation scales of the block come from LDS (staged once per
// workgroup as f32, [block][token]: four broadcast ds_read_b128 per block).  Every block costs one MFMA (32 cycles) and
// 16 x (convert, scale product, multiply-add): the fold is the bound (VALU), ~1/8 of the int8 matrix peak — against one
// pass over the weights per 16 tokens with the tiled mat-vec this replaces for T >= 32.
// Workgroup = 4 waves = 128 weight rows x 32 tokens; the four waves share the token tile (L1 hits on the activations).
//
// MINS (the copies of Q4_1 / Q5_1 tensors, device rows [codes K][scales K/32][mins K/32]; codes 0..15 / 0..31): a block adds
//
//   t = (float)isum_b * (d_w * d_a) + m_w[r][b] * s_a[t][b],   s_a = d_a * (float)sum_{k in b} a[t][k],   out += t
//
// every product and sum rounded on its own, each output's chain in block order.  s_a does not depend on the weight row: it is staged in LDS
// beside d_a, once per workgroup and chunk (the staging thread of a (block, token) sums the block's 32 activation codes - exact - and
// multiplies once).  The fold then costs 16 x (one more multiply, one more add) per block: five packed-pair instructions per output pair
// instead of three, so the bound estimate above becomes ~1/13 of the int8 matrix peak for these two types.
//
// E8 (the copies of MXFP4 tensors, device rows [codes K][e K/32]: codes are the format's levels, -12 .. 12; the scale plane is the blocks' E8M0 bytes): d_w is
// formed from the byte with a compare, two shifts and a select (e8f) in place of the f16 conversion - exact for every e, where an f16 plane would hold
// 104 <= e <= 143 only - and the fold is the plain one.
//
// MOE (the grouped-expert form, ggml_mul_mat_id on a prompt batch in ONE launch per projection): a workgroup is (row tile, token-tile slot, segment).  Slot j
// is the j-th tile of 32 MT tokens of the concatenation of the experts' batches; the workgroup finds its expert, the tile within that expert's batch and the
// batch's first grouped row by walking the per-expert counts on the device (as moe_tile_of does for the plane kernels, mmq.hip), and a slot beyond the last
// tile returns before any barrier.  The body then runs on the expert's copy and the batch's rows as "the" token range: the arithmetic is the dense form's.
#include "kernels.h"
#include "quant_dev.h"

namespace mi355 {

namespace {

typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int Q80_UNROLL = 4;

// MT token tiles of 32 per wave: a workgroup covers 128 weight rows x 32 MT tokens, so every weight byte is fetched T / (32 MT) times instead of T / 32
// (with MT = 1 an 8B-shaped prompt is bound by those re-reads out of L2: 8.5k tok/s).  The activation scales are staged per chunk of Q80_KC blocks.
constexpr int Q80_KC = 64;

template <int MT, bool MINS, bool E8>
__device__ __forceinline__ void mmq_q80_body(const uint8_t *__restrict__ W, size_t row_bytes, int n_rows, int K, int T,
                                             const int8_t *__restrict__ aq, const uint16_t *__restrict__ ad, float *__restrict__ out,
                                             int ld_out, const float *__restrict__ resid, int row_tile, int tok_tile) {
    __shared__ __attribute__((aligned(16))) float s_da[(MINS ? 2 : 1) * Q80_KC * 32 * MT];      // [block of the chunk][token of the workgroup's tile]; MINS: s_a behind it
    const float *s_sa = s_da + Q80_KC * 32 * MT;
    constexpr int TT = 32 * MT;
    const int nb = K >> 5;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, kg = lane >> 5;
    const int t0 = tok_tile * TT, r0 = row_tile * 128 + wave * 32;
    const bool rows_ok = r0 < n_rows;                                  // (wave-uniform; such a wave still takes part in the barriers)
    const int row = r0 + n < n_rows ? r0 + n : n_rows - 1;
    const uint8_t *wrow = W + (size_t)row * row_bytes + 16 * kg;
    const uint16_t *wd = reinterpret_cast<const uint16_t *>(W + (size_t)row * row_bytes + K);
    const uint16_t *wm = wd + nb;                                      // (MINS) the row's min plane
    const uint8_t *we = W + (size_t)row * row_bytes + K;               // (E8) the row's E8M0 scale bytes
    auto wscale = [&](int b) -> uint32_t { if constexpr (E8) return we[b]; else return wd[b]; };
    auto wfloat = [](uint32_t s) -> float { if constexpr (E8) return e8f(s); else return h2f((uint16_t)s); };
    const int8_t *arow[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) {
        const int tok = t0 + 32 * m + n < T ? t0 + 32 * m + n : T - 1;
        arow[m] = aq + (size_t)tok * K + 16 * kg;
    }
    float facc[MT][16];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) facc[m][r] = 0.0f;
    i32x16 z;
#pragma unroll
    for (int r = 0; r < 16; r++) z[r] = 0;

    // per output and block: scale = d_w * d_a (exact: two f16 values), product = (float)isum * scale, sum += product - the CPU's three roundings in the CPU's
    // order; written on pairs so that the multiplies and the add become v_pk_mul_f32 / v_pk_add_f32 (two outputs per instruction, same IEEE results)
    // MINS: term = product + m_w * s_a (one more multiply, one more add, each rounded: the build has contraction off), sum += term
    auto fold = [&](const i32x16 &c, float dw, float mw, int bl, int m) {        // bl: block within the chunk
        const f32x2 dw2 = {dw, dw};
        const f32x2 mw2 = {mw, mw};
#pragma unroll
        for (int rq = 0; rq < 4; rq++) {
            const f32x4 da4 = *reinterpret_cast<const f32x4 *>(s_da + bl * TT + 32 * m + 8 * rq + 4 * kg);    // tokens 8 rq + 4 kg + (0..3) of tile m
            f32x4 sa4;
            if constexpr (MINS) sa4 = *reinterpret_cast<const f32x4 *>(s_sa + bl * TT + 32 * m + 8 * rq + 4 * kg);
#pragma unroll
            for (int rp = 0; rp < 2; rp++) {
                const f32x2 da2 = {da4[2 * rp], da4[2 * rp + 1]};
                const f32x2 cf = {(float)c[rq * 4 + 2 * rp], (float)c[rq * 4 + 2 * rp + 1]};
                const f32x2 sc = dw2 * da2;
                f32x2 pr = cf * sc;
                if constexpr (MINS) {
                    const f32x2 sa2 = {sa4[2 * rp], sa4[2 * rp + 1]};
                    const f32x2 ms = mw2 * sa2;
                    pr = pr + ms;
                }
                f32x2 acc = {facc[m][rq * 4 + 2 * rp], facc[m][rq * 4 + 2 * rp + 1]};
                acc = acc + pr;
                facc[m][rq * 4 + 2 * rp] = acc.x; facc[m][rq * 4 + 2 * rp + 1] = acc.y;
            }
        }
    };
    for (int b0 = 0; b0 < nb; b0 += Q80_KC) {
        const int nbc = nb - b0 < Q80_KC ? nb - b0 : Q80_KC;
        __syncthreads();                                               // everyone is done with the previous chunk's scales
        for (int i = tid; i < nbc * TT; i += 256) {
            const int b = i / TT, m = i - b * TT;
            const int t = t0 + m < T ? t0 + m : T - 1;
            const float da = h2f(ad[(size_t)t * nb + b0 + b]);
            s_da[i] = da;
            if constexpr (MINS) {                                      // d_a * (float)(sum of the block's 32 codes): exact integer, one rounding
                const i32x4 *ap = reinterpret_cast<const i32x4 *>(aq + (size_t)t * K + (size_t)(b0 + b) * 32);
                const i32x4 a0 = ap[0], a1 = ap[1];
                int sum = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) { sum = dot4(0x01010101u, (uint32_t)a0[j], sum); sum = dot4(0x01010101u, (uint32_t)a1[j], sum); }
                s_da[Q80_KC * TT + i] = da * (float)sum;
            }
        }
        __syncthreads();
        if (!rows_ok) continue;
        int b = 0;
        for (; b + Q80_UNROLL <= nbc; b += Q80_UNROLL) {               // the loads of a group are issued before its first MFMA
            i32x4 w[Q80_UNROLL];
            uint32_t dh[Q80_UNROLL];
            uint16_t mh[Q80_UNROLL];
#pragma unroll
            for (int u = 0; u < Q80_UNROLL; u++) {
                w[u] = __builtin_nontemporal_load(reinterpret_cast<const i32x4 *>(wrow + (size_t)(b0 + b + u) * 32));
                dh[u] = wscale(b0 + b + u);
                if constexpr (MINS) mh[u] = wm[b0 + b + u];
            }
#pragma unroll
            for (int m = 0; m < MT; m++) {
                i32x4 a[Q80_UNROLL];
#pragma unroll
                for (int u = 0; u < Q80_UNROLL; u++) a[u] = *reinterpret_cast<const i32x4 *>(arow[m] + (size_t)(b0 + b + u) * 32);
#pragma unroll
                for (int u = 0; u < Q80_UNROLL; u++) {
                    const i32x16 c = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[u], w[u], z, 0, 0, 0);
                    fold(c, wfloat(dh[u]), MINS ? h2f(mh[u]) : 0.0f, b + u, m);
                }
            }
        }
        for (; b < nbc; b++) {
            const i32x4 w = *reinterpret_cast<const i32x4 *>(wrow + (size_t)(b0 + b) * 32);
            const float dw = wfloat(wscale(b0 + b)), mw = MINS ? h2f(wm[b0 + b]) : 0.0f;
#pragma unroll
            for (int m = 0; m < MT; m++) {
                const i32x4 a = *reinterpret_cast<const i32x4 *>(arow[m] + (size_t)(b0 + b) * 32);
                const i32x16 c = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, w, z, 0, 0, 0);
                fold(c, dw, mw, b, m);
            }
        }
    }
    if (rows_ok && r0 + n < n_rows) {
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int t = t0 + 32 * m + 8 * (r >> 2) + 4 * kg + (r & 3);
                if (t < T) {
                    const size_t o = (size_t)t * ld_out + row;
                    out[o] = resid ? resid[o] + facc[m][r] : facc[m][r];
                }
            }
    }
}

template <int MT, bool MINS, bool E8>
__global__ __launch_bounds__(256) void mmq_q80_kernel(const uint8_t *__restrict__ W, size_t row_bytes, int n_rows, int K, int T,
                                                      const int8_t *__restrict__ aq, const uint16_t *__restrict__ ad, float *__restrict__ out,
                                                      int ld_out, const float *__restrict__ resid) {
    mmq_q80_body<MT, MINS, E8>(W, row_bytes, n_rows, K, T, aq, ad, out, ld_out, resid, (int)blockIdx.x, (int)blockIdx.y);
}

// the grouped-expert form: meta = moe_group_kernel's [0, NE) tokens per expert, [NE, 2 NE) first grouped row; blockIdx.z picks the segment (ffn_gate | ffn_up
// of one layer share a launch: the same grouped activation rows, two weight tensors, two outputs)
struct MoeQ80 { const int32_t *meta; int n_expert; size_t expert_stride; const uint8_t *W[2]; float *out[2]; };
template <int MT, bool MINS, bool E8>
__global__ __launch_bounds__(256) void mmq_q80_moe_kernel(const MoeQ80 mq, size_t row_bytes, int n_rows, int K, const int8_t *__restrict__ aq,
                                                          const uint16_t *__restrict__ ad, int ld_out) {
    constexpr int TT = 32 * MT;
    int j = (int)blockIdx.y, e = 0, n_e = 0;
    for (; e < mq.n_expert; e++) {                             // (scalar: the counts are a few words of one or two cache lines)
        n_e = mq.meta[e];
        const int tiles = (n_e + TT - 1) / TT;
        if (j < tiles) break;
        j -= tiles;
    }
    if (e >= mq.n_expert) return;                              // a slot beyond the last tile: workgroup-uniform, before any barrier
    const int r0 = mq.meta[mq.n_expert + e];
    const int sg = (int)blockIdx.z;
    mmq_q80_body<MT, MINS, E8>(mq.W[sg] + (size_t)e * mq.expert_stride, row_bytes, n_rows, K, n_e, aq + (size_t)r0 * K, ad + (size_t)r0 * (K >> 5),
                               mq.out[sg] + (size_t)r0 * ld_out, ld_out, nullptr, (int)blockIdx.x, j);
}

}  // namespace

// Q4_0 / Q5_0 / IQ4_NL rows as Q8_0 device rows ([codes K][scales K/32]): code = nibble - 8, (nibble | fifth bit) - 16, level[nibble] - all int8 -
// with the block's own f16 scale.  The copy is EXACT (same integers, same scales), so the kernel above computes the same block sums as the format's
// own vec_dot; it is made once at load for prompt batches (1.06 B per weight beside the file's 0.56 - 0.69).
// Q4_1 / Q5_1: the code is q itself (0..15 / 0..31) and the row gains the blocks' f16 minimums as a third plane ([codes K][scales K/32][mins K/32],
// 1.125 B per weight), for the MINS form of the kernel.
// MXFP4: the code is level[nibble] (kvalues_mxfp4, -12 .. 12) and the scale plane holds the blocks' E8M0 bytes ([codes K][e K/32], 1.03 B per weight), for
// the E8 form of the kernel.
__global__ __launch_bounds__(256) void expand_nib32_q80_kernel(int type, const uint8_t *__restrict__ W, size_t row_bytes, int n_rows, int K, uint8_t *__restrict__ dst,
                                                               size_t dst_row) {
    const int row = blockIdx.y;
    const int nblk = K >> 5;
    // the type is a run-time value here, so the source row's planes are spelled out: qs | [qh] | d | [m], MXFP4 qs | e (kTypeLayouts, ggml_types.h)
    const size_t half = (size_t)K >> 1;                          // plane 1: qh (Q5_0, Q5_1), e (MXFP4), else d
    const uint8_t *r = W + (size_t)row * row_bytes;
    uint8_t *o = dst + (size_t)row * dst_row;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < K; e += gridDim.x * 256) {
        const int b = e >> 5, j = e & 31;
        const int nib = (r[(size_t)b * 16 + (j & 15)] >> (4 * (j >> 4))) & 0x0f;
        int code;
        if (type == T_Q4_0) code = nib - 8;
        else if (type == T_Q5_0 || type == T_Q5_1) {
            const uint32_t qh = *reinterpret_cast<const uint32_t *>(r + half + (size_t)b * 4);
            code = (nib | (int)(((qh >> j) & 1u) << 4)) - (type == T_Q5_0 ? 16 : 0);
        } else if (type == T_Q4_1) code = nib;
        else if (type == T_MXFP4) code = mxfp4_value(nib);
        else code = iq4nl_value(nib);
        o[e] = (uint8_t)(int8_t)code;
        if (j == 0 && nib32_has_e8(type)) o[(size_t)K + (size_t)b] = r[half + (size_t)b];
        else if (j == 0) {
            const uint16_t *dp = reinterpret_cast<const uint16_t *>(r + nib32_d_off(type, (size_t)K));   // plane d; m follows it
            *reinterpret_cast<uint16_t *>(o + (size_t)K + (size_t)b * 2) = dp[b];
            if (nib32_has_min(type)) *reinterpret_cast<uint16_t *>(o + (size_t)K + (size_t)nblk * 2 + (size_t)b * 2) = dp[nblk + b];
        }
    }
}
size_t mmq_q80_copy_row_bytes(int type, int K) {
    const size_t b = (size_t)K + (size_t)(K >> 5) * (nib32_has_min(type) ? 4 : nib32_has_e8(type) ? 1 : 2);
    return (b + 15) & ~(size_t)15;
}
int mmq_q80_copy_form(int type) { return nib32_has_min(type) ? Q80_FORM_MINS : nib32_has_e8(type) ? Q80_FORM_E8 : Q80_FORM_F16; }
size_t mmq_q80_copy_bytes(int type, int64_t n_rows, int K) {
    if (!type_has_q80_copy(type) || (K % 32) != 0 || K > 16384) return 0;
    return (size_t)n_rows * mmq_q80_copy_row_bytes(type, K);
}
hipError_t launch_expand_q80_copy(int type, const uint8_t *W, size_t row_bytes, int n_rows, int K, uint8_t *dst, hipStream_t st) {
    if (!mmq_q80_copy_bytes(type, n_rows, K)) return hipErrorInvalidValue;
    for (int r0 = 0; r0 < n_rows; r0 += 65535) {
        const int nr = n_rows - r0 < 65535 ? n_rows - r0 : 65535;
        hipLaunchKernelGGL(expand_nib32_q80_kernel, dim3((unsigned)((K + 255) / 256 < 8 ? (K + 255) / 256 : 8), nr), dim3(256), 0, st, type, W + (size_t)r0 * row_bytes, row_bytes, nr, K,
                           dst + (size_t)r0 * mmq_q80_copy_row_bytes(type, K), mmq_q80_copy_row_bytes(type, K));
    }
    return hipGetLastError();
}

bool mmq_q80_applicable(int type, int K, int T) { return type == T_Q8_0 && T >= 32 && K >= 32 && (K % 32) == 0 && K <= 16384; }

static int g_q80_mt = 0;      // 0: pick per launch; 1 / 2 / 4: the tests force a form (every form gives the same bits)
void mmq_q80_set_tiles(int mt) { g_q80_mt = (mt == 1 || mt == 2 || mt == 4) ? mt : 0; }

template <bool MINS, bool E8>
static void launch_q80_form(int mt, const uint8_t *W, size_t row_bytes, int n_rows, int K, int T, const ActQuant &q, float *out, int ld_out, const float *resid, hipStream_t st) {
    const dim3 grid((unsigned)((n_rows + 127) / 128), (unsigned)((T + 32 * mt - 1) / (32 * mt)));
    if (mt == 4) hipLaunchKernelGGL((mmq_q80_kernel<4, MINS, E8>), grid, dim3(256), 0, st, W, row_bytes, n_rows, K, T, q.qs0, q.d0, out, ld_out, resid);
    else if (mt == 2) hipLaunchKernelGGL((mmq_q80_kernel<2, MINS, E8>), grid, dim3(256), 0, st, W, row_bytes, n_rows, K, T, q.qs0, q.d0, out, ld_out, resid);
    else hipLaunchKernelGGL((mmq_q80_kernel<1, MINS, E8>), grid, dim3(256), 0, st, W, row_bytes, n_rows, K, T, q.qs0, q.d0, out, ld_out, resid);
}

hipError_t launch_mmq_q80(const uint8_t *W, size_t row_bytes, int n_rows, int K, int T, const ActQuant &q, float *out, int ld_out,
                          const float *resid, hipStream_t st, int form, bool any_T) {
    if (!mmq_q80_applicable(T_Q8_0, K, any_T && T >= 1 ? 32 : T) || !q.qs0 || !q.d0) return hipErrorInvalidValue;
    // four token tiles per wave once that still leaves a workgroup per CU; each output keeps its own block order, so the result does not depend on MT
    const long wg4 = (long)((n_rows + 127) / 128) * ((T + 127) / 128);
    int mt = (T >= 128 && wg4 >= num_cu()) ? 4 : (T >= 64 && wg4 * 2 >= num_cu()) ? 2 : 1;
    if (g_q80_mt) mt = g_q80_mt;
    if (form == Q80_FORM_MINS) launch_q80_form<true, false>(mt, W, row_bytes, n_rows, K, T, q, out, ld_out, resid, st);
    else if (form == Q80_FORM_E8) launch_q80_form<false, true>(mt, W, row_bytes, n_rows, K, T, q, out, ld_out, resid, st);
    else launch_q80_form<false, false>(mt, W, row_bytes, n_rows, K, T, q, out, ld_out, resid, st);
    return hipGetLastError();
}

// every expert's batch of one projection (n_seg = 2: of ffn_gate and ffn_up) in one launch.  rows_max = rows of the grouped arrays (tokens x experts used):
// ceil(rows_max / tile) + n_expert slots cover every split of them into batches, since each expert may end in a partial tile.  Only the E8 form is
// instantiated: the launch is enabled for MXFP4 expert tensors (the other copies keep the per-expert launches they have).
bool mmq_q80_moe_ok(int type, int n_rows, int K) { return nib32_has_e8(type) && mmq_q80_copy_bytes(type, n_rows, K) != 0 && (n_rows % 128) == 0 && K >= 32; }
hipError_t launch_mmq_q80_moe(int type, const uint8_t *const *W, float *const *outs, int n_seg, size_t expert_stride, int n_expert, const int32_t *meta, int n_rows,
                              int K, int rows_max, const ActQuant &q, int ld_out, hipStream_t st) {
    if (!mmq_q80_moe_ok(type, n_rows, K) || n_seg < 1 || n_seg > 2 || n_expert < 1 || rows_max < 1 || !meta || !q.qs0 || !q.d0) return hipErrorInvalidValue;
    // the tile follows the mean batch: at 8 of 128 experts a 512-token prompt batch gives 32 rows an expert, at 2 of 8 it gives 128
    const int mean = rows_max / n_expert;
    int mt = mean > 64 ? 4 : mean > 32 ? 2 : 1;
    if (g_q80_mt) mt = g_q80_mt;
    MoeQ80 mq{};
    mq.meta = meta; mq.n_expert = n_expert; mq.expert_stride = expert_stride;
    for (int i = 0; i < n_seg; i++) { mq.W[i] = W[i]; mq.out[i] = outs[i]; }
    const size_t row_bytes = mmq_q80_copy_row_bytes(type, K);
    const dim3 grid((unsigned)(n_rows / 128), (unsigned)((rows_max + 32 * mt - 1) / (32 * mt) + n_expert), (unsigned)n_seg);
    if (mt == 4) hipLaunchKernelGGL((mmq_q80_moe_kernel<4, false, true>), grid, dim3(256), 0, st, mq, row_bytes, n_rows, K, q.qs0, q.d0, ld_out);
    else if (mt == 2) hipLaunchKernelGGL((mmq_q80_moe_kernel<2, false, true>), grid, dim3(256), 0, st, mq, row_bytes, n_rows, K, q.qs0, q.d0, ld_out);
    else hipLaunchKernelGGL((mmq_q80_moe_kernel<1, false, true>), grid, dim3(256), 0, st, mq, row_bytes, n_rows, K, q.qs0, q.d0, ld_out);
    return hipGetLastError();
}

}  // namespace mi355
