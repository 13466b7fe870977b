// lora.hip — run-time LoRA adapters: out[t][n] += scale * B[n] . (A x[t]) for up to three tensors that share one activation (Q | K | V, gate | up).
//
// Two skinny products: A is [r][K] (r rows of the base tensor's input width), B is [N][r], r <= 512.  Arithmetic as ggml's CPU mul_mat has it:
//   F32 pair: f32 products, f32 sums.
//   F16 pair: x rounded to f16, t = A x summed in f32 and rounded to f16, then B t summed in f32.
// Step 1 (lora_ax): a wave owns LORA_JB rows of A at a time and up to TT tokens; the lanes walk K in 16-byte pieces, the lane sums are folded by the DPP
//   wave_sum (a fixed tree: the same call gives the same bits).
// Step 2 (lora_bt): one thread per output row n walks its r weights in order against t (LDS), then out[t][n] = out[t][n] + scale * sum.
// The single-token form (T <= 8) is ONE launch: every workgroup (256 output rows of one segment) computes its segment's t for itself - A is a few hundred
//   KB at most and comes from L2.  A prompt batch takes two launches with t in a scratch the caller owns.
// No workgroup waits for another, nothing is added with atomics, and nothing is written outside out[t][0 .. N).
#include "kernels.h"

namespace mi355 {
namespace {

constexpr int LORA_THREADS = 256, LORA_WAVES = LORA_THREADS / WAVE, LORA_JB = 4, LORA_ROWS = LORA_THREADS;

struct LoraLaunch {
    LoraSeg seg[3];
    int block0[4];         // workgroups [block0[s], block0[s + 1]) serve segment s
    int n_seg;
    const float *x;
    int ld_x, K, T;
    float *t;              // batch form: [n_seg][T][LORA_MAX_R]
};

__device__ __forceinline__ float round_h(float v) { return h2f(f2h(v)); }

// V consecutive weights of a row as floats: 16 bytes (8 halves or 4 floats)
template <bool H> __device__ __forceinline__ void load_w(const void *row, int k, float (&w)[H ? 8 : 4]) {
    if (H) {
        const uint4 u = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(row) + k);
        const unsigned p[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int i = 0; i < 4; i++) { w[2 * i] = h2f((uint16_t)(p[i] & 0xffffu)); w[2 * i + 1] = h2f((uint16_t)(p[i] >> 16)); }
    } else {
        const float4 f = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(row) + k);
        w[0] = f.x; w[1] = f.y; w[2] = f.z; w[3] = f.w;
    }
}

// rows jb .. jb + LORA_JB of A against tokens t0 .. t0 + TT (those below T): t_out[tt * t_stride + j], rounded to f16 for an F16 pair.  One wave.
// The loop is a latency chain (A comes from L2 or HBM, nothing else runs on the CU), so a trip issues every load it needs before it uses one: KU pieces of K per
// lane, each with its x rows and LORA_JB rows of A, without a branch between them - a row or a token past the end reads the last valid one (its sums are never
// stored), a piece past K reads piece 0 and counts as zeros.  Every lane still adds its products in ascending k.
template <int TT, bool H>
__device__ __forceinline__ void lora_ax(const void *A, int r, int K, const float *x, int ld_x, int t0, int T, int jb, float *t_out, int t_stride) {
    constexpr int V = H ? 8 : 4, KU = TT <= 2 ? 4 : TT == 4 ? 2 : 1;
    const int lane = threadIdx.x & (WAVE - 1);
    const size_t row_bytes = (size_t)K * (H ? 2 : 4);
    const uint8_t *rows[LORA_JB];
    const float *xr[TT];
#pragma unroll
    for (int jj = 0; jj < LORA_JB; jj++) rows[jj] = reinterpret_cast<const uint8_t *>(A) + (size_t)(jb + jj < r ? jb + jj : r - 1) * row_bytes;
#pragma unroll
    for (int tt = 0; tt < TT; tt++) xr[tt] = x + (size_t)(t0 + tt < T ? t0 + tt : T - 1) * ld_x;
    float acc[LORA_JB][TT];
#pragma unroll
    for (int jj = 0; jj < LORA_JB; jj++)
#pragma unroll
        for (int tt = 0; tt < TT; tt++) acc[jj][tt] = 0.0f;
    for (int k0 = lane * V; k0 < K; k0 += WAVE * V * KU) {
        float xv[KU][TT][V], w[KU][LORA_JB][V];
        bool ok[KU];
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int k = k0 + u * WAVE * V;
            ok[u] = k + V <= K;
            const int kc = ok[u] ? k : 0;
#pragma unroll
            for (int tt = 0; tt < TT; tt++)
#pragma unroll
                for (int v = 0; v < V; v += 4) {
                    const float4 f = *reinterpret_cast<const float4 *>(xr[tt] + kc + v);
                    xv[u][tt][v] = f.x; xv[u][tt][v + 1] = f.y; xv[u][tt][v + 2] = f.z; xv[u][tt][v + 3] = f.w;
                }
#pragma unroll
            for (int jj = 0; jj < LORA_JB; jj++) load_w<H>(rows[jj], kc, w[u][jj]);
        }
#pragma unroll
        for (int u = 0; u < KU; u++) {
#pragma unroll
            for (int tt = 0; tt < TT; tt++)
#pragma unroll
                for (int v = 0; v < V; v++) xv[u][tt][v] = ok[u] ? (H ? round_h(xv[u][tt][v]) : xv[u][tt][v]) : 0.0f;
#pragma unroll
            for (int jj = 0; jj < LORA_JB; jj++)
#pragma unroll
                for (int tt = 0; tt < TT; tt++)
#pragma unroll
                    for (int v = 0; v < V; v++) acc[jj][tt] += (ok[u] ? w[u][jj][v] : 0.0f) * xv[u][tt][v];
        }
    }
#pragma unroll
    for (int jj = 0; jj < LORA_JB; jj++)
#pragma unroll
        for (int tt = 0; tt < TT; tt++) {
            const float s = wave_sum(acc[jj][tt]);
            if (lane == 0 && jb + jj < r && t0 + tt < T) t_out[(size_t)tt * t_stride + jb + jj] = H ? round_h(s) : s;
        }
}

// output row n of B against t[tt][0 .. r) (LDS, row stride t_stride), tokens t0 .. t0 + TT: out += scale * sum.  One thread.
template <int TT, bool H>
__device__ __forceinline__ void lora_bt(const LoraSeg &sg, int n, const float *t, int t_stride, int t0, int T) {
    constexpr int V = H ? 8 : 4;
    const int r = sg.r;
    const uint8_t *row = reinterpret_cast<const uint8_t *>(sg.B) + (size_t)n * r * (H ? 2 : 4);
    float acc[TT];
#pragma unroll
    for (int tt = 0; tt < TT; tt++) acc[tt] = 0.0f;
    int j = 0;
    if ((r % V) == 0) {                                          // every row of B starts on 16 bytes
        for (; j < r; j += V) {
            float w[V];
            load_w<H>(row, j, w);
#pragma unroll
            for (int v = 0; v < V; v++)
#pragma unroll
                for (int tt = 0; tt < TT; tt++) acc[tt] += w[v] * t[tt * t_stride + j + v];
        }
    }
    for (; j < r; j++) {
        const float w = H ? h2f(reinterpret_cast<const uint16_t *>(row)[j]) : reinterpret_cast<const float *>(row)[j];
#pragma unroll
        for (int tt = 0; tt < TT; tt++) acc[tt] += w * t[tt * t_stride + j];
    }
#pragma unroll
    for (int tt = 0; tt < TT; tt++)
        if (t0 + tt < T) {
            float *o = sg.out + (size_t)(t0 + tt) * sg.ld_out + n;
            *o = *o + sg.scale * acc[tt];
        }
}

__device__ __forceinline__ int seg_of_block(const LoraLaunch &a, int b) {
    int s = 0;
    while (s + 1 < a.n_seg && b >= a.block0[s + 1]) s++;
    return s;
}

// single-token form: T <= TT <= 8, grid = block0[n_seg]
template <int TT>
__global__ __launch_bounds__(LORA_THREADS) void lora_delta_fused_kernel(const LoraLaunch a) {
    __shared__ float t[TT * LORA_MAX_R];
    const int s = seg_of_block(a, (int)blockIdx.x);
    const LoraSeg &sg = a.seg[s];
    const int wave = threadIdx.x / WAVE;
    for (int jb = wave * LORA_JB; jb < sg.r; jb += LORA_WAVES * LORA_JB) {
        if (sg.type == T_F16) lora_ax<TT, true>(sg.A, sg.r, a.K, a.x, a.ld_x, 0, a.T, jb, t, LORA_MAX_R);
        else lora_ax<TT, false>(sg.A, sg.r, a.K, a.x, a.ld_x, 0, a.T, jb, t, LORA_MAX_R);
    }
    __syncthreads();
    const int n = ((int)blockIdx.x - a.block0[s]) * LORA_ROWS + (int)threadIdx.x;
    if (n >= sg.N) return;
    if (sg.type == T_F16) lora_bt<TT, true>(sg, n, t, LORA_MAX_R, 0, a.T);
    else lora_bt<TT, false>(sg, n, t, LORA_MAX_R, 0, a.T);
}

// batch form, step 1: grid (row groups of LORA_WAVES * LORA_JB, 8-token chunks, segments) -> a.t
__global__ __launch_bounds__(LORA_THREADS) void lora_ax_kernel(const LoraLaunch a) {
    const int s = (int)blockIdx.z;
    const LoraSeg &sg = a.seg[s];
    const int jb = ((int)blockIdx.x * LORA_WAVES + (int)(threadIdx.x / WAVE)) * LORA_JB, t0 = (int)blockIdx.y * 8;
    if (jb >= sg.r) return;
    float *t_out = a.t + ((size_t)s * a.T + t0) * LORA_MAX_R;
    if (sg.type == T_F16) lora_ax<8, true>(sg.A, sg.r, a.K, a.x, a.ld_x, t0, a.T, jb, t_out, LORA_MAX_R);
    else lora_ax<8, false>(sg.A, sg.r, a.K, a.x, a.ld_x, t0, a.T, jb, t_out, LORA_MAX_R);
}

// batch form, step 2: grid (block0[n_seg], 8-token chunks)
__global__ __launch_bounds__(LORA_THREADS) void lora_bt_kernel(const LoraLaunch a) {
    __shared__ float t[8 * LORA_MAX_R];
    const int s = seg_of_block(a, (int)blockIdx.x);
    const LoraSeg &sg = a.seg[s];
    const int t0 = (int)blockIdx.y * 8;
    const float *src = a.t + ((size_t)s * a.T + t0) * LORA_MAX_R;
    for (int i = (int)threadIdx.x; i < 8 * sg.r; i += LORA_THREADS) {
        const int tt = i / sg.r, j = i - tt * sg.r;
        t[tt * LORA_MAX_R + j] = t0 + tt < a.T ? src[(size_t)tt * LORA_MAX_R + j] : 0.0f;
    }
    __syncthreads();
    const int n = ((int)blockIdx.x - a.block0[s]) * LORA_ROWS + (int)threadIdx.x;
    if (n >= sg.N) return;
    if (sg.type == T_F16) lora_bt<8, true>(sg, n, t, LORA_MAX_R, t0, a.T);
    else lora_bt<8, false>(sg, n, t, LORA_MAX_R, t0, a.T);
}

}  // namespace

size_t lora_scratch_floats(int T) { return T > LORA_FUSED_MAX_T ? (size_t)3 * (size_t)T * LORA_MAX_R : 0; }

bool lora_delta_args_ok(const LoraSeg *segs, int n_seg, const float *x, int ld_x, int K, int T) {
    if (!segs || !x || n_seg < 1 || n_seg > 3 || T < 1 || K < 32 || (K % 32) != 0 || ld_x < K || (ld_x % 4) != 0 || ((uintptr_t)x % 16) != 0) return false;
    for (int s = 0; s < n_seg; s++) {
        const LoraSeg &g = segs[s];
        if ((g.type != T_F16 && g.type != T_F32) || g.r < 1 || g.r > LORA_MAX_R || g.N < 1 || g.ld_out < g.N || !g.A || !g.B || !g.out) return false;
        if (((uintptr_t)g.A % 16) != 0 || ((uintptr_t)g.B % 16) != 0) return false;
    }
    return true;
}

hipError_t launch_lora_delta(const LoraSeg *segs, int n_seg, const float *x, int ld_x, int K, int T, float *scratch, hipStream_t st) {
    if (!lora_delta_args_ok(segs, n_seg, x, ld_x, K, T) || (T > LORA_FUSED_MAX_T && !scratch)) return hipErrorInvalidValue;
    LoraLaunch a{};
    a.n_seg = n_seg; a.x = x; a.ld_x = ld_x; a.K = K; a.T = T; a.t = scratch;
    int r_max = 0;
    for (int s = 0; s < n_seg; s++) {
        a.seg[s] = segs[s];
        a.block0[s + 1] = a.block0[s] + (segs[s].N + LORA_ROWS - 1) / LORA_ROWS;
        r_max = segs[s].r > r_max ? segs[s].r : r_max;
    }
    for (int s = n_seg; s < 3; s++) a.block0[s + 1] = a.block0[n_seg];
    const int blocks = a.block0[n_seg];
    if (T <= LORA_FUSED_MAX_T) {
        if (T == 1) hipLaunchKernelGGL(lora_delta_fused_kernel<1>, dim3(blocks), dim3(LORA_THREADS), 0, st, a);
        else if (T == 2) hipLaunchKernelGGL(lora_delta_fused_kernel<2>, dim3(blocks), dim3(LORA_THREADS), 0, st, a);
        else if (T <= 4) hipLaunchKernelGGL(lora_delta_fused_kernel<4>, dim3(blocks), dim3(LORA_THREADS), 0, st, a);
        else hipLaunchKernelGGL(lora_delta_fused_kernel<8>, dim3(blocks), dim3(LORA_THREADS), 0, st, a);
        return hipGetLastError();
    }
    const int chunks = (T + 7) / 8;
    hipLaunchKernelGGL(lora_ax_kernel, dim3((r_max + LORA_WAVES * LORA_JB - 1) / (LORA_WAVES * LORA_JB), chunks, n_seg), dim3(LORA_THREADS), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(lora_bt_kernel, dim3(blocks, chunks), dim3(LORA_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace mi355
