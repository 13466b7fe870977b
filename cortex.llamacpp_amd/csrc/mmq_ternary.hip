// mmq_ternary.hip — prompt batches against TQ1_0 / TQ2_0 weights on the matrix cores, straight from the packed trits: no plane set, no second weight copy.
//
//   out[t][r] = sum over super-blocks sb, in ascending order, of  (float)isum_sb * (d_w[r][sb] * d_a[t][sb]),   isum_sb = sum_{k in sb} p[r][k] * a[t][k]
//
// p = code - 1 (-1, 0, 1; 2 where a TQ2_0 byte holds code 3) is one int8, a is the Q8_K code: a plain int8 x int8 -> int32 product per 256-element super-block
// (|isum| <= 256 * 2 * 127), then ggml_vec_dot_tq*_0_q8_K's one f32 term per super-block, every product and sum rounded on its own.  An output's chain of terms
// does not depend on the tile shape, the token count or the launch form: the same bits from every one of them.  No block sums (p is formed before the
// product), no mmq_prep, no high / low split of either operand.
//
// The contraction order within a super-block.  v_mfma_i32_32x32x32_i8 takes 16 bytes of k per lane and operand: lane = (n = lane & 31, kg = lane >> 5).  Step s
// (0..7) of a super-block contracts, in lane half kg, the sixteen elements
//
//     128 kg + 16 s + (0 .. 15)                      <- THE K-permutation: step s = elements [16 s, 16 s + 16) and [128 + 16 s, 128 + 16 s + 16)
//
// so the activation operand is sixteen consecutive Q8_K codes, and both formats decode whole operands from 16-byte pieces of the row:
//   TQ2_0  element 128 h + 32 l + m sits in bits 2 l .. of qs[32 h + m]: lane half kg loads qs[32 kg .. + 31] as two 16-byte pieces; word j of piece ih under
//          (w >> 2 l) & 0x03030303 is word j of step s = 2 l + ih.  64 bytes per row and super-block, 2 loads per lane.
//   TQ1_0  trit n of qs[0..31] is element 32 n + m, of qs[32..47] element 160 + 16 n + m, of qh[j] element 240 + 4 n + j: trit n of the piece qs[16 q .. + 15]
//          is the 16-element run 2 n + q, trit n of qs[32..47] is run 10 + n, trits 0..3 of the qh word are the four words of run 15.  Lane half 0 (runs 0..7)
//          needs trits 0..3 of the first two pieces, half 1 (runs 8..15) trit 4 of those, all of the third piece and qh: the piece and the power of three
//          are selected per lane half (v_cndmask), the arithmetic is tq1_codes4 (quant_dev.h), defined for all 256 byte values.
//   code - 1 per byte without a borrow between bytes: ((c | 0x80808080) - 0x01010101) ^ 0x80808080.
//
// Tile.  A workgroup is 4 waves = 128 weight rows x 32 MT tokens (MT = 1, 2, 4 by the batch).  A wave owns 32 rows and all the workgroup's tokens: its weight
// bytes go global -> registers -> decode -> MFMA operand (32 operand words per super-block, decoded once and used for MT token tiles), never through LDS.
// The activation is the larger stream (256 B per token and super-block against 52 / 64 B per row) and is the same for the four waves: the workgroup stages
// it through LDS once per super-block - rows padded to 272 B, so that the sixteen lanes of a 16-byte read phase fall into different banks - with the tokens'
// d_a behind it, double-buffered: the next super-block's pieces are in flight (registers) while this one is contracted, one barrier per super-block.
//   LDS      2 x 32 MT x (272 + 4) B = 17.3 / 34.5 / 69 KB (MT = 4: two workgroups per CU of 160 KB)
//   VGPRs    16 MT accumulators + 32 operand words + 16 (the MFMA result) + 4 MT staging words + the next super-block's raw weights, and the activation
//            operands the scheduler keeps in flight: 137 - 154 (MT = 1) and 226 - 240 (MT = 2) under a two-waves-per-SIMD bound, 414 - 428 at MT = 4, which
//            runs one wave per SIMD (bounded to 256 it spilled 160 registers); no scratch in any form.  The SwiGLU form (gate and up rows of one tile in
//            one workgroup: two operand sets, two accumulator sets) runs MT <= 2 for that reason
//   per super-block and wave: 8 MT MFMAs (32 x 32 x 32), 16 MT x (convert, two multiplies, add) for the fold, 32 operand words of decode
//            (5 VALU operations a word for TQ2_0, 17 for TQ1_0) - MT = 4 puts the MFMAs ahead of both VALU parts
#include "kernels.h"
#include "quant_dev.h"

namespace mi355 {

namespace {

typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TERN_ROWS = 128;           // weight rows per workgroup (4 waves x 32)
constexpr int TERN_PITCH = 272;          // LDS bytes per staged token: 256 codes + 16 (bank spread)

struct TernArgs {
    const uint8_t *W[3];                 // device rows of the segments (SwiGLU: gate, up)
    float *out[3];
    int n_rows[3], ld_out[3];
    int tile0[4];                        // first row tile of each segment; tile0[n_seg] = the grid's x extent
    int n_seg;
    size_t row_bytes;
    int K, T;
    const int8_t *aq;                    // Q8_K codes [T][K]
    const float *ad;                     // Q8_K scales [T][K / 256]
    const float *resid;                  // nullable (one segment): out = resid + y
    int32_t *ints;                       // nullable (one segment, tests): isum [T][n_rows][K / 256]
};

__device__ __forceinline__ uint32_t minus1_bytes(uint32_t c) { return ((c | 0x80808080u) - 0x01010101u) ^ 0x80808080u; }

// the raw bytes of one row's super-block a lane decodes from
template <int TYPE> struct TernRaw;
template <> struct TernRaw<T_TQ2_0> {
    i32x4 q0, q1;                        // qs[32 kg .. + 15], qs[32 kg + 16 .. + 31]
    __device__ __forceinline__ void load(const uint8_t *row, int nb, int sb, int kg) {
        const i32x4 *p = reinterpret_cast<const i32x4 *>(row + (size_t)sb * 64 + 32 * kg);
        q0 = p[0]; q1 = p[1];
    }
    __device__ __forceinline__ void decode(i32x4 (&op)[8], int kg) const {
#pragma unroll
        for (int l = 0; l < 4; l++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                op[2 * l][j] = (int)minus1_bytes(((uint32_t)q0[j] >> (2 * l)) & 0x03030303u);
                op[2 * l + 1][j] = (int)minus1_bytes(((uint32_t)q1[j] >> (2 * l)) & 0x03030303u);
            }
    }
};
template <> struct TernRaw<T_TQ1_0> {
    i32x4 a, b, c;                       // qs[0..15], qs[16..31], qs[32..47]
    uint32_t h;                          // the four qh bytes
    __device__ __forceinline__ void load(const uint8_t *row, int nb, int sb, int kg) {
        const i32x4 *p = reinterpret_cast<const i32x4 *>(row + (size_t)sb * 48);
        a = p[0]; b = p[1]; c = p[2];
        h = *reinterpret_cast<const uint32_t *>(row + plane_off<T_TQ1_0, tq1::P_QH>((size_t)nb) + (size_t)sb * 4);
    }
    __device__ __forceinline__ void decode(i32x4 (&op)[8], int kg) const {
        constexpr uint32_t P3[5] = {1u, 3u, 9u, 27u, 81u};
        const bool hi = kg != 0;
#pragma unroll
        for (int s = 0; s < 8; s++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t ab = (uint32_t)((s & 1) ? b[j] : a[j]);                          // half 0, runs 0..7: trit s >> 1 of piece s & 1
                const uint32_t w1 = s < 2 ? ab : s < 7 ? (uint32_t)c[j] : h;                   // half 1, runs 8, 9: trit 4 of the same piece; 10..14: trit s - 2 of
                const uint32_t p1 = s < 2 ? 81u : s < 7 ? P3[(s + 3) % 5] : P3[j];             // the third piece; 15: trit j of the qh word        ((s + 3) % 5 = s - 2)
                op[s][j] = (int)minus1_bytes(tq1_codes4(hi ? w1 : ab, hi ? p1 : P3[s >> 1]));
            }
    }
};

// NW = 1: up to three segments over one activation (Q | K | V), or one with a residual.  NW = 2: W[0] = ffn_gate, W[1] = ffn_up, out[0] = silu(gate) * up.
template <int TYPE, int MT, int NW>
__global__ __launch_bounds__(256, MT == 4 ? 1 : 2) void mmq_ternary_kernel(const TernArgs ka) {
    extern __shared__ __attribute__((aligned(16))) uint8_t tern_lds[];
    constexpr int TT = 32 * MT;
    constexpr int BUF = TT * TERN_PITCH + TT * 4;                 // codes, then the tokens' d_a
    constexpr int NCH = TT * 16 / 256;                            // 16-byte pieces a thread stages per super-block
    const int nb = ka.K >> 8;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, kg = lane >> 5;
    int sg = 0;
    if (NW == 1) while (sg + 1 < ka.n_seg && (int)blockIdx.x >= ka.tile0[sg + 1]) sg++;
    const int n_rows = ka.n_rows[sg], ld_out = ka.ld_out[sg];
    const int t0 = (int)blockIdx.y * TT, r0 = ((int)blockIdx.x - ka.tile0[sg]) * TERN_ROWS + wave * 32;
    const bool rows_ok = r0 < n_rows;                             // (wave-uniform; such a wave still stages and takes part in the barriers)
    const int row = r0 + n < n_rows ? r0 + n : n_rows - 1;
    const uint8_t *wrow[NW];
    const uint16_t *wd[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) {
        wrow[w] = ka.W[NW == 1 ? sg : w] + (size_t)row * ka.row_bytes;
        wd[w] = reinterpret_cast<const uint16_t *>(wrow[w] + (TYPE == T_TQ2_0 ? plane_off<T_TQ2_0, tq2::P_D>((size_t)nb) : plane_off<T_TQ1_0, tq1::P_D>((size_t)nb)));
    }
    // staging role: piece c = tid + 256 i of the tile is bytes 16 (tid & 15) .. of token (tid >> 4) + 16 i (the addresses are formed per fetch: registers are dearer)
    const int stage_tok = tid >> 4, stage_dst = stage_tok * TERN_PITCH + 16 * (tid & 15);
    const int8_t *stage_src = ka.aq + 16 * (tid & 15);
    const float *stage_d = ka.ad + (size_t)(t0 + tid < ka.T ? t0 + tid : ka.T - 1) * nb;      // (threads below TT)

    float facc[NW][MT][16];
#pragma unroll
    for (int w = 0; w < NW; w++)
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int r = 0; r < 16; r++) facc[w][m][r] = 0.0f;

    i32x4 st[NCH];
    float st_d = 0.0f;
    TernRaw<TYPE> raw[NW];
    auto fetch = [&](int sb) {                                    // the super-block's activation pieces and raw weight bytes into registers
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            const int tok = t0 + stage_tok + 16 * i < ka.T ? t0 + stage_tok + 16 * i : ka.T - 1;
            st[i] = *reinterpret_cast<const i32x4 *>(stage_src + (size_t)tok * ka.K + (size_t)sb * 256);
        }
        if (tid < TT) st_d = stage_d[sb];
#pragma unroll
        for (int w = 0; w < NW; w++) raw[w].load(wrow[w], nb, sb, kg);
    };
    auto stash = [&](int buf) {
        uint8_t *b = tern_lds + buf * BUF;
#pragma unroll
        for (int i = 0; i < NCH; i++) *reinterpret_cast<i32x4 *>(b + stage_dst + 16 * i * TERN_PITCH) = st[i];
        if (tid < TT) reinterpret_cast<float *>(b + TT * TERN_PITCH)[tid] = st_d;
    };
    fetch(0);
    stash(0);
    __syncthreads();
    for (int sb = 0; sb < nb; sb++) {
        i32x4 op[NW][8];
        float dw[NW];
#pragma unroll
        for (int w = 0; w < NW; w++) { raw[w].decode(op[w], kg); dw[w] = h2f(wd[w][sb]); }
        fetch(sb + 1 < nb ? sb + 1 : sb);                         // (the last round fetches its own again: in bounds, unused)
        const uint8_t *buf = tern_lds + (sb & 1) * BUF;
        const float *s_da = reinterpret_cast<const float *>(buf + TT * TERN_PITCH);
        if (rows_ok) {
#pragma unroll
            for (int m = 0; m < MT; m++) {
                i32x16 c[NW];
#pragma unroll
                for (int w = 0; w < NW; w++)
#pragma unroll
                    for (int r = 0; r < 16; r++) c[w][r] = 0;
                const uint8_t *arow = buf + (32 * m + n) * TERN_PITCH + 128 * kg;
#pragma unroll
                for (int s = 0; s < 8; s++) {
                    const i32x4 a = *reinterpret_cast<const i32x4 *>(arow + 16 * s);
#pragma unroll
                    for (int w = 0; w < NW; w++) c[w] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, op[w][s], c[w], 0, 0, 0);
                }
                // the fold: result register r of lane (n, kg) is token 8 (r >> 2) + 4 kg + (r & 3) of the tile against row n
#pragma unroll
                for (int rq = 0; rq < 4; rq++) {
                    const f32x4 da4 = *reinterpret_cast<const f32x4 *>(s_da + 32 * m + 8 * rq + 4 * kg);
#pragma unroll
                    for (int w = 0; w < NW; w++)
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const float sc = dw[w] * da4[e];
                            const float pr = (float)c[w][4 * rq + e] * sc;
                            facc[w][m][4 * rq + e] = facc[w][m][4 * rq + e] + pr;
                        }
                }
                if (NW == 1 && ka.ints && r0 + n < n_rows) {
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int t = t0 + 32 * m + 8 * (r >> 2) + 4 * kg + (r & 3);
                        if (t < ka.T) ka.ints[((size_t)t * n_rows + row) * nb + sb] = c[0][r];
                    }
                }
            }
        }
        if (sb + 1 < nb) stash((sb + 1) & 1);                     // (everyone left that buffer at the previous round's barrier)
        __syncthreads();
    }
    if (rows_ok && r0 + n < n_rows) {
        float *out = ka.out[NW == 1 ? sg : 0];
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int t = t0 + 32 * m + 8 * (r >> 2) + 4 * kg + (r & 3);
                if (t < ka.T) {
                    const size_t o = (size_t)t * ld_out + row;
                    if (NW == 2) out[o] = swiglu_f32(facc[0][m][r], facc[NW - 1][m][r]);
                    else out[o] = ka.resid ? ka.resid[o] + facc[0][m][r] : facc[0][m][r];
                }
            }
    }
}

template <int TYPE, int MT, int NW>
hipError_t launch_form(const TernArgs &ka, dim3 grid, hipStream_t st) {
    constexpr int lds = 2 * (32 * MT * TERN_PITCH + 32 * MT * 4);
    if (lds > 64 * 1024) {                                        // (MT = 4: above the default cap on dynamic LDS)
        const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&mmq_ternary_kernel<TYPE, MT, NW>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (attr != hipSuccess) return attr;
    }
    hipLaunchKernelGGL((mmq_ternary_kernel<TYPE, MT, NW>), grid, dim3(256), lds, st, ka);
    return hipGetLastError();
}
template <int TYPE>
hipError_t launch_type(int mt, bool swiglu, const TernArgs &ka, dim3 grid, hipStream_t st) {
    if (swiglu) return mt == 2 ? launch_form<TYPE, 2, 2>(ka, grid, st) : launch_form<TYPE, 1, 2>(ka, grid, st);
    return mt == 4 ? launch_form<TYPE, 4, 1>(ka, grid, st) : mt == 2 ? launch_form<TYPE, 2, 1>(ka, grid, st) : launch_form<TYPE, 1, 1>(ka, grid, st);
}

}  // namespace

bool mmq_ternary_applicable(int type, int K, int T) { return type_is_ternary(type) && T >= 32 && K >= 256 && (K % 256) == 0 && K <= 65536; }

static int g_tern_mt = 0;     // 0: pick per launch; 1 / 2 / 4: the tests force a form (every form gives the same bits)
void mmq_ternary_set_tiles(int mt) { g_tern_mt = (mt == 1 || mt == 2 || mt == 4) ? mt : 0; }

hipError_t launch_mmq_ternary(int type, const MMQTernarySeg *segs, int n_seg, int K, int T, const ActQuant &q, const float *resid, bool swiglu, hipStream_t st,
                              int32_t *isum) {
    if (!mmq_ternary_applicable(type, K, T) || !segs || n_seg < 1 || n_seg > 3 || !q.qs || !q.d) return hipErrorInvalidValue;
    if ((resid || isum) && (n_seg != 1 || swiglu)) return hipErrorInvalidValue;
    if (swiglu && (n_seg != 2 || segs[0].n_rows != segs[1].n_rows)) return hipErrorInvalidValue;
    TernArgs ka{};
    int tiles = 0;
    for (int s = 0; s < n_seg; s++) {
        if (!segs[s].W || segs[s].n_rows < 1 || (!segs[s].out && !(swiglu && s == 1)) || segs[s].ld_out < (swiglu && s == 1 ? 0 : segs[s].n_rows)) return hipErrorInvalidValue;
        ka.W[s] = segs[s].W; ka.out[s] = segs[s].out; ka.n_rows[s] = segs[s].n_rows; ka.ld_out[s] = segs[s].ld_out;
        ka.tile0[s] = tiles;
        if (!(swiglu && s == 1)) tiles += (segs[s].n_rows + TERN_ROWS - 1) / TERN_ROWS;
    }
    for (int s = n_seg; s < 4; s++) ka.tile0[s] = tiles;
    ka.n_seg = swiglu ? 1 : n_seg;
    ka.row_bytes = dev_row_bytes(type, K); ka.K = K; ka.T = T;
    ka.aq = q.qs; ka.ad = q.d; ka.resid = resid; ka.ints = isum;
    // four token tiles per wave once that still leaves a workgroup per CU, two at half of that (the decode of a super-block's weights is shared by the
    // wave's token tiles); each output keeps its own super-block order, so the result does not depend on MT
    const long wg4 = (long)tiles * ((T + 127) / 128);
    int mt = (T >= 128 && wg4 >= num_cu()) ? 4 : (T >= 64 && wg4 * 2 >= num_cu()) ? 2 : 1;
    if (g_tern_mt) mt = g_tern_mt;
    if (swiglu && mt > 2) mt = 2;
    const dim3 grid((unsigned)tiles, (unsigned)((T + 32 * mt - 1) / (32 * mt)));
    return type == T_TQ2_0 ? launch_type<T_TQ2_0>(mt, swiglu, ka, grid, st) : launch_type<T_TQ1_0>(mt, swiglu, ka, grid, st);
}

}  // namespace mi355
