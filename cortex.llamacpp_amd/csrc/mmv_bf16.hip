// mmv_bf16.hip — the decode-side contraction against BF16 weight tensors (ggml type 30): a weight stream for 1 <= T <= 16 tokens, and the activation rounding
// both BF16 paths share.
//
//   y[t][n] = sum_k W[n][k] * bf16(x[t][k])          (ggml_mul_mat with a bf16 src0: vec_dot_type is BF16, the activation row is rounded to bf16, nearest-even)
//
// A bf16 value is the upper half of an f32, so widening is a shift and every product bf16 x bf16 is exact in f32.  The CPU sums the products in double and rounds
// once; here they are summed in f32 in ONE fixed order per output, whatever the launch looks like:
//   lane l of the wave that owns the row takes the 16-byte pieces l, l + 64, l + 128 ... of the row in that order, the eight products of a piece in element
//   order, each added with one fmaf (the product is exact, so fmaf rounds exactly what a separate multiply and add would); then wave_sum over the 64 lanes.
// The order does not depend on T, on the number of segments, on the rows a wave holds or on the epilogue: a fused launch and separate launches give the same bits,
// and so does row t of a 16-token launch and a launch of that token alone.
//
// Structure: the weights are read once per launch, straight into registers (no LDS: nothing is shared between waves), 16 bytes per lane per load and R rows x
// UN steps of them in flight per lane; a wave owns R consecutive rows and all T tokens of the launch.  The activation rows arrive as bf16 (launch_f32_to_bf16:
// rounded once per launch, not once per row of W) and are re-read by every wave from L2 - T x K x 2 bytes against R x K x 2 of weights: a quarter of the
// weight bytes at one token (R = 4), but 2x / 4x / 8x of them at 4 / 8 / 16 tokens (R = 2).  The 8- and 16-token forms are therefore bound by L2, not by HBM:
// they exist for narrow tensors and for the order guarantee above; the model path hands batches of 8 tokens and more to the matrix cores (mmf_bf16.hip).  A
// batched step of 5 - 7 tokens runs as chunks (4 + 1, 4 + 2, 4 + 2 + 1) and streams every weight once per chunk, as the quantised mat-vec's chunking does.
// Up to three segments share the activation (Q | K | V), their rows simply follow each other in the wave numbering; EPI_SWIGLU interleaves the rows of gate and
// up so that a wave holds both values of an output.
#include "kernels.h"

namespace mi355 {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ggml_compute_fp32_to_bf16: nearest, ties to even, on the bits; a NaN keeps its upper bits and gets the quiet bit; subnormals are kept
__device__ __forceinline__ unsigned bf16_bits(float f) {
    const unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 64u;
    return (u + (0x7fffu + ((u >> 16) & 1u))) >> 16;
}

__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float *__restrict__ x, unsigned *__restrict__ y, size_t n8) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const f32x4 a = reinterpret_cast<const f32x4 *>(x)[2 * i], b = reinterpret_cast<const f32x4 *>(x)[2 * i + 1];
    u32x4 o;
    o.x = bf16_bits(a.x) | (bf16_bits(a.y) << 16);
    o.y = bf16_bits(a.z) | (bf16_bits(a.w) << 16);
    o.z = bf16_bits(b.x) | (bf16_bits(b.y) << 16);
    o.w = bf16_bits(b.z) | (bf16_bits(b.w) << 16);
    reinterpret_cast<u32x4 *>(y)[i] = o;
}

__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

// one 16-byte piece of R rows against the same piece of NT activation rows
template <int NT, int R>
__device__ __forceinline__ void piece(const u32x4 (&w)[R], const u32x4 (&x)[NT], float (&acc)[R][NT]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
        float xl[NT], xh[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) { xl[t] = bf_lo(x[t][j]); xh[t] = bf_hi(x[t][j]); }
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float wl = bf_lo(w[r][j]), wh = bf_hi(w[r][j]);
#pragma unroll
            for (int t = 0; t < NT; t++) { acc[r][t] = fmaf(wl, xl[t], acc[r][t]); acc[r][t] = fmaf(wh, xh[t], acc[r][t]); }
        }
    }
}

template <int NT, int R, int UN>
__global__ __launch_bounds__(256) void mmv_bf16_kernel(MMVBF16Args a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool swiglu = a.epi == EPI_SWIGLU;
    const int n0 = a.seg[0].n_rows, n1 = a.n_seg > 1 ? a.seg[1].n_rows : 0, n2 = a.n_seg > 2 ? a.seg[2].n_rows : 0;
    const int total = n0 + n1 + n2;                             // (swiglu: n0 == n1, rows interleaved gate, up, gate, up ...)
    const int v0 = (blockIdx.x * 4 + wave) * R;
    if (v0 >= total) return;                                    // (wave-uniform)
    int sg[R], rw[R];
    const uint8_t *wr[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int v = v0 + r < total ? v0 + r : total - 1;      // rows past the end read the last row; their results are never stored
        int s, row;
        if (swiglu) { s = v & 1; row = v >> 1; }
        else if (v < n0) { s = 0; row = v; }
        else if (v < n0 + n1) { s = 1; row = v - n0; }
        else { s = 2; row = v - n0 - n1; }
        sg[r] = s; rw[r] = row;
        wr[r] = a.seg[s].W + (size_t)row * a.seg[s].row_bytes + (size_t)lane * 16;
    }
    float acc[R][NT];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int t = 0; t < NT; t++) acc[r][t] = 0.0f;
    const int K = a.K, npiece = K >> 3, nfull = npiece >> 6, tail = npiece & 63;
    const uint16_t *xp = a.xb + (size_t)lane * 8;
    int i = 0;
    // UN steps at a time: their R * UN weight loads are issued before the first product
    for (; i + UN <= nfull; i += UN) {
        u32x4 w[UN][R], x[UN][NT];
#pragma unroll
        for (int u = 0; u < UN; u++) {
#pragma unroll
            for (int r = 0; r < R; r++) w[u][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(wr[r] + (size_t)(i + u) * 1024));
#pragma unroll
            for (int t = 0; t < NT; t++) x[u][t] = *reinterpret_cast<const u32x4 *>(xp + (size_t)t * K + (size_t)(i + u) * 512);
        }
#pragma unroll
        for (int u = 0; u < UN; u++) piece<NT, R>(w[u], x[u], acc);
    }
    for (; i < nfull; i++) {
        u32x4 w[R], x[NT];
#pragma unroll
        for (int r = 0; r < R; r++) w[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(wr[r] + (size_t)i * 1024));
#pragma unroll
        for (int t = 0; t < NT; t++) x[t] = *reinterpret_cast<const u32x4 *>(xp + (size_t)t * K + (size_t)i * 512);
        piece<NT, R>(w, x, acc);
    }
    if (lane < tail) {                                          // a row whose pieces do not fill the last step (K % 512 != 0)
        u32x4 w[R], x[NT];
#pragma unroll
        for (int r = 0; r < R; r++) w[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(wr[r] + (size_t)nfull * 1024));
#pragma unroll
        for (int t = 0; t < NT; t++) x[t] = *reinterpret_cast<const u32x4 *>(xp + (size_t)t * K + (size_t)nfull * 512);
        piece<NT, R>(w, x, acc);
    }
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int t = 0; t < NT; t++) acc[r][t] = wave_sum(acc[r][t]);

    // epilogue: lane (slot * NT + t) stores token t of the wave's output slot (a row, or with SwiGLU a gate / up pair)
    const int slot = lane / NT, t = lane - slot * NT;
    if (swiglu) {
        float g = 0.0f, u = 0.0f;
        int row = -1;
#pragma unroll
        for (int p = 0; p < R / 2; p++)
#pragma unroll
            for (int tt = 0; tt < NT; tt++)
                if (lane == p * NT + tt) { g = acc[2 * p][tt]; u = acc[2 * p + 1][tt]; row = v0 + 2 * p < total ? rw[2 * p] : -1; }
        if (row >= 0) a.seg[0].out[(size_t)t * a.seg[0].ld_out + row] = (g / (1.0f + expf(-g))) * u;      // (swiglu_kernel's expression, act.hip)
        return;
    }
    float v = 0.0f;
    int row = -1, ld = 0;
    float *out = nullptr;
    const float *bias = nullptr;
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (slot == r && v0 + r < total) { row = rw[r]; out = a.seg[sg[r]].out; bias = a.seg[sg[r]].bias; ld = a.seg[sg[r]].ld_out; }
#pragma unroll
        for (int tt = 0; tt < NT; tt++)
            if (lane == r * NT + tt) v = acc[r][tt];
    }
    if (row < 0) return;
    // y = resid + (acc + bias): the order of the separate bias and add launches (and of the matrix-core kernel's epilogue)
    if (bias) v = v + bias[row];
    const size_t o = (size_t)t * ld + row;
    if (a.epi == EPI_ADD) v = a.resid[o] + v;
    out[o] = v;
}

template <int NT, int R, int UN>
hipError_t launch_t(const MMVBF16Args &a, int total, hipStream_t st) {
    const int waves = (total + R - 1) / R;
    hipLaunchKernelGGL((mmv_bf16_kernel<NT, R, UN>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_f32_to_bf16(const float *x, void *y, size_t n, hipStream_t st) {
    if (n % 8 || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, st, x, reinterpret_cast<unsigned *>(y), n / 8);
    return hipGetLastError();
}

// one launch: a.T in {1, 2, 4, 8, 16}
hipError_t launch_mmv_bf16(const MMVBF16Args &a, hipStream_t st) {
    if (a.n_seg < 1 || a.n_seg > 3 || a.K < 8 || (a.K & 7) || !a.xb || (reinterpret_cast<uintptr_t>(a.xb) & 15)) return hipErrorInvalidValue;
    if (a.epi == EPI_SWIGLU && (a.n_seg != 2 || a.seg[0].n_rows != a.seg[1].n_rows)) return hipErrorInvalidValue;
    if (a.epi == EPI_ADD && (a.n_seg != 1 || !a.resid)) return hipErrorInvalidValue;
    if (a.epi != EPI_STORE && a.epi != EPI_ADD && a.epi != EPI_SWIGLU) return hipErrorInvalidValue;
    int total = 0;
    for (int s = 0; s < a.n_seg; s++) {
        const MMVBF16Seg &g = a.seg[s];
        if (g.n_rows < 1 || !g.W || !g.out || (reinterpret_cast<uintptr_t>(g.W) & 15) || (g.row_bytes & 15) || g.row_bytes < (size_t)a.K * 2 || g.ld_out < g.n_rows) return hipErrorInvalidValue;
        total += g.n_rows;
    }
    switch (a.T) {
        case 1: return launch_t<1, 4, 4>(a, total, st);
        case 2: return launch_t<2, 4, 2>(a, total, st);
        case 4: return launch_t<4, 2, 2>(a, total, st);
        case 8: return launch_t<8, 2, 2>(a, total, st);
        case 16: return launch_t<16, 2, 1>(a, total, st);
        default: return hipErrorInvalidValue;
    }
}

// any T: chunks of 16, 8, 4, 2, 1 tokens (the chunking of the quantised mat-vec); a.xb / out / resid are the first token's
hipError_t launch_mmv_bf16_tokens(const MMVBF16Args &a0, int T, hipStream_t st) {
    for (int t0 = 0; t0 < T;) {
        const int rem = T - t0, nt = rem >= 16 ? 16 : rem >= 8 ? 8 : rem >= 4 ? 4 : rem >= 2 ? 2 : 1;
        MMVBF16Args a = a0;
        a.T = nt;
        a.xb = a0.xb + (size_t)t0 * a0.K;
        if (a0.resid) a.resid = a0.resid + (size_t)t0 * a0.seg[0].ld_out;
        for (int s = 0; s < a0.n_seg; s++) a.seg[s].out = a0.seg[s].out + (size_t)t0 * a0.seg[s].ld_out;
        const hipError_t e = launch_mmv_bf16(a, st);
        if (e != hipSuccess) return e;
        t0 += nt;
    }
    return hipSuccess;
}

}  // namespace mi355
