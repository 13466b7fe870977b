// mmf_bf16.hip — batched contraction against BF16 weight tensors (ggml type 30) on the matrix cores: the bf16 sibling of mmf.hip.
//
//   Y[t][n] = resid[t][n] + (sum_k W[n][k] * bf16(X[t][k]) + bias[n]) * scale          (bias, scale and resid each optional)
//
// The activation rows arrive rounded to bf16 already (launch_f32_to_bf16, mmv_bf16.hip: ggml's nearest-even rounding on the bits, once per row).  Both operands are
// K-contiguous rows, the register layout of v_mfma_f32_32x32x16_bf16 (lane = (row m, k-group kg): eight consecutive k).  The products are exact in f32 and summed
// in f32 by the matrix pipe in k order (the CPU sums them in double: equal up to f32 re-association).  Two kernels with the tile shapes of their f16 twins:
//   mmbf16_kernel<WT>   straight from global memory, a wave owns WT x WT tiles of 32 x 32 (a workgroup 128 x 128 or 64 x 64 outputs);
//   mmbf16_lds_kernel   64 x 64 outputs per workgroup, k staged through LDS in whole 128-byte lines, for products with few workgroups.
// Every output is the same chain of matrix-core steps over k in all of them: they agree bit for bit.
#include <cstdlib>

#include "kernels.h"

namespace mi355 {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// register r of a lane holds weight row (r & 3) + 8 (r >> 2) + 4 kg of the 32 x 32 tile, token = lane & 31: four consecutive rows per 16-byte store
__device__ __forceinline__ void store_tile(const f32x16 &acc, int n0, int t, int kg, int N, float *Y, int ldy, const float *resid, const float *bias, float scale, int do_scale) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int n = n0 + 8 * q + 4 * kg;
        float *dst = Y + (size_t)t * ldy + n;
        const float *rs = resid ? resid + (size_t)t * ldy + n : nullptr;
        float r[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            r[e] = acc[4 * q + e];
            if (bias && n + e < N) r[e] = r[e] + bias[n + e];
            if (do_scale) r[e] = r[e] * scale;
        }
        if (n + 3 < N && (ldy & 3) == 0) {
            f32x4 v = {r[0], r[1], r[2], r[3]};
            if (rs) { const f32x4 r4 = *reinterpret_cast<const f32x4 *>(rs); v.x = r4.x + v.x; v.y = r4.y + v.y; v.z = r4.z + v.z; v.w = r4.w + v.w; }
            *reinterpret_cast<f32x4 *>(dst) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) if (n + e < N) dst[e] = rs ? rs[e] + r[e] : r[e];
        }
    }
}

template <int WT>
__global__ __launch_bounds__(256) void mmbf16_kernel(const __bf16 *W, int N, int K, const __bf16 *X, int T, float *Y, int ldy, const float *resid, const float *bias,
                                                     float scale, int do_scale) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 31, kg = lane >> 5;
    const int n0 = blockIdx.x * (64 * WT) + (wave & 1) * (32 * WT), t0 = blockIdx.y * (64 * WT) + (wave >> 1) * (32 * WT);
    if (n0 >= N || t0 >= T) return;                             // (wave-uniform)
    const __bf16 *wr[WT], *xr[WT];
#pragma unroll
    for (int i = 0; i < WT; i++) {
        const int n = n0 + 32 * i + m, t = t0 + 32 * i + m;     // rows past the end read the last row; their results are never stored
        wr[i] = W + (size_t)(n < N ? n : N - 1) * K + 8 * kg;
        xr[i] = X + (size_t)(t < T ? t : T - 1) * K + 8 * kg;
    }
    f32x16 acc[WT][WT];
#pragma unroll
    for (int i = 0; i < WT; i++)
#pragma unroll
        for (int j = 0; j < WT; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.0f;
    for (int k0 = 0; k0 < K; k0 += 16) {
        bf16x8 a[WT], b[WT];
#pragma unroll
        for (int i = 0; i < WT; i++) {
            a[i] = *reinterpret_cast<const bf16x8 *>(wr[i] + k0);
            b[i] = *reinterpret_cast<const bf16x8 *>(xr[i] + k0);
        }
#pragma unroll
        for (int i = 0; i < WT; i++)
#pragma unroll
            for (int j = 0; j < WT; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < WT; i++)
#pragma unroll
        for (int j = 0; j < WT; j++) {
            const int t = t0 + 32 * j + m;
            if (t < T) store_tile(acc[i][j], n0 + 32 * i, t, kg, N, Y, ldy, resid, bias, scale, do_scale);
        }
}

// 64 halves of k per stage (one 128-byte line of every row: eight lanes fetch a row's line together), double-buffered in LDS with PD stages more on their way in
// registers; a wave owns 32 x 32 outputs and reads its two fragments per matrix-core step from rows padded to 144 bytes (conflict-free 16-byte reads).  K >= 64.
__global__ __launch_bounds__(256) void mmbf16_lds_kernel(const __bf16 *__restrict__ W, int N, int K, const __bf16 *__restrict__ X, int T, float *Y, int ldy,
                                                         const float *resid, const float *bias, float scale, int do_scale) {
    constexpr int BK = 64, LDR = 72;                            // elements per stage, padded row length (144 bytes)
    __shared__ __bf16 sA[2][64 * LDR], sB[2][64 * LDR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 31, kg = lane >> 5;
    const int n0 = blockIdx.x * 64, t0 = blockIdx.y * 64;
    const int lr = tid >> 3, lc = tid & 7;                      // loader: rows lr and lr + 32 of both tiles, 16-byte column lc
    const __bf16 *gw[2], *gx[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int n = n0 + lr + 32 * i, t = t0 + lr + 32 * i;   // rows past the end read the last row; their results are never stored
        gw[i] = W + (size_t)(n < N ? n : N - 1) * K + 8 * lc;
        gx[i] = X + (size_t)(t < T ? t : T - 1) * K + 8 * lc;
    }
    constexpr int PD = 4;
    bf16x8 ra[PD][2], rb[PD][2];
    // (no branch and no select around a load.  A piece past K - the last stage of a K that is not a multiple of 64, and the stages requested past the end - is
    // read from the row's last 16 bytes instead and never multiplied; K >= 64 keeps that address inside the row)
    auto fetch = [&](bf16x8 (&a2)[2], bf16x8 (&b2)[2], int k0) {
        const int k = k0 + 8 * lc < K ? k0 : K - 8 - 8 * lc;
#pragma unroll
        for (int i = 0; i < 2; i++) { a2[i] = *reinterpret_cast<const bf16x8 *>(gw[i] + k); b2[i] = *reinterpret_cast<const bf16x8 *>(gx[i] + k); }
    };
    auto put = [&](const bf16x8 (&a2)[2], const bf16x8 (&b2)[2], int buf) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            *reinterpret_cast<bf16x8 *>(&sA[buf][(lr + 32 * i) * LDR + 8 * lc]) = a2[i];
            *reinterpret_cast<bf16x8 *>(&sB[buf][(lr + 32 * i) * LDR + 8 * lc]) = b2[i];
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    const int ar = ((wave & 1) * 32 + m) * LDR + 8 * kg, br = ((wave >> 1) * 32 + m) * LDR + 8 * kg;
    const int nst = (K + BK - 1) / BK;
#pragma unroll
    for (int u = 0; u < PD; u++) fetch(ra[u], rb[u], u * BK);
    put(ra[0], rb[0], 0);
    __syncthreads();
    for (int st = 0; st < nst; st += PD) {
#pragma unroll
        for (int u = 0; u < PD; u++) {
            const int cur = st + u, buf = u & 1;
            if (cur >= nst) break;
            fetch(ra[u], rb[u], (cur + PD) * BK);               // slot u went to LDS a step ago: refill it PD stages ahead
#pragma unroll
            for (int s4 = 0; s4 < 4; s4++) {
                if (cur * BK + 16 * s4 >= K) break;
                const bf16x8 a = *reinterpret_cast<const bf16x8 *>(&sA[buf][ar + 16 * s4]), b = *reinterpret_cast<const bf16x8 *>(&sB[buf][br + 16 * s4]);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
            }
            if (cur + 1 < nst) put(ra[(u + 1) % PD], rb[(u + 1) % PD], buf ^ 1);
            __syncthreads();
        }
    }
    const int t = t0 + (wave >> 1) * 32 + m;
    if (t < T) store_tile(acc, n0 + (wave & 1) * 32, t, kg, N, Y, ldy, resid, bias, scale, do_scale);
}

}  // namespace

// the applicability rule of mmf16_applicable with the type changed
bool mmbf16_applicable(int type, int n_rows, int K, int T, const void *W, const void *xb, const void *y) {
    return type == T_BF16 && T >= 8 && n_rows >= 32 && (K % 16) == 0 && ((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(xb) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
}

// xb: [T][K] bf16 (launch_f32_to_bf16); y = resid + (W xb + bias) * scale, every part optional (resid may be y itself)
hipError_t launch_mmbf16(const uint8_t *W, int n_rows, int K, const void *xb, int T, float *y, int ld_out, const float *resid, const float *bias, float scale, bool do_scale,
                         hipStream_t st) {
    if (n_rows < 1 || T < 1 || K < 16 || (K % 16)) return hipErrorInvalidValue;
    // (the loads are 16 bytes wide; so are the stores and the residual's loads when the leading dimension is a multiple of 4)
    if ((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(xb)) & 15) return hipErrorInvalidValue;
    if ((ld_out & 3) == 0 && ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(resid)) & 15)) return hipErrorInvalidValue;
    const __bf16 *w = reinterpret_cast<const __bf16 *>(W), *x = reinterpret_cast<const __bf16 *>(xb);
    const dim3 big((unsigned)((n_rows + 127) / 128), (unsigned)((T + 127) / 128));
    // MI355_MMBF16_FORM (A/B and tests): "128" / "64" the direct kernel with that tile, "lds" the staged kernel; unset: by the number of workgroups, as the f16 twin
    const char *sw = getenv("MI355_MMBF16_FORM");
    const int form = !sw ? 0 : sw[0] == 'l' ? 3 : atoi(sw) == 128 ? 1 : atoi(sw) == 64 ? 2 : 0;
    if (form == 1 || (form == 0 && big.x * big.y >= 256)) {
        hipLaunchKernelGGL((mmbf16_kernel<2>), big, dim3(256), 0, st, w, n_rows, K, x, T, y, ld_out, resid, bias, scale, (int)do_scale);
        return hipGetLastError();
    }
    const dim3 small((unsigned)((n_rows + 63) / 64), (unsigned)((T + 63) / 64));
    if (form == 2 || K < 64)
        hipLaunchKernelGGL((mmbf16_kernel<1>), small, dim3(256), 0, st, w, n_rows, K, x, T, y, ld_out, resid, bias, scale, (int)do_scale);
    else
        hipLaunchKernelGGL(mmbf16_lds_kernel, small, dim3(256), 0, st, w, n_rows, K, x, T, y, ld_out, resid, bias, scale, (int)do_scale);
    return hipGetLastError();
}

}  // namespace mi355
