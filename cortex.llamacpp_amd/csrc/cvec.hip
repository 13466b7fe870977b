// cvec.hip — control vectors (upstream's --control-vector and llama-cvector-generator).
//
// Applying one: x[t][:] = fl32(x[t][:] + v[:]) on a layer's completed output rows - launch_add_row_vec, a launch of its own behind the layer's last launch
// (no other kernel knows about vectors).  A thread owns four adjacent columns of one row: one 16-byte load of x, one of v, four additions, one 16-byte store.
//
// Making one: the first principal direction of rows D [R][E] by the power method on D^T D, never forming the E x E matrix.  An iteration is three launches,
// with no atomic and no kernel that waits for another, every order fixed by (R, E) - the same (D, b) gives the same bits on every call:
//   row pass   y[r] = D[r] . b          a wave per row: a lane walks its 16-byte pieces of the row in column order (fmaf), then the fixed butterfly wave_sum
//   slab pass  slab[s][j] = sum over the rows r of slice s of y[r] * D[r][j]     the scheme of imatrix.hip: slices of S = cvec_slice_rows(R) rows, a workgroup owns
//                                       one slice and 1024 columns, a thread four columns, rows added in row order
//   finish     z[j] = the slabs in slice order; n = |z|; b[j] <- z[j] / n; dist = |b_new - b_old|      one workgroup of 1024 threads: a thread owns columns
//                                       j = tid, tid + 1024, ...; the two norms are per-thread sums in column order, then wave_sum, then the 16 waves in wave order
// The mean method is the slab pass with every weight 1 and the finish with z scaled by 1 / R.
#include <algorithm>

#include "dev_common.h"
#include "kernels.h"

namespace mi355 {

namespace {
constexpr int CV_TILE = 1024;         // columns of a slab-pass workgroup (256 threads x 4)
constexpr int CV_FIN = 1024;          // threads of the finish and orient workgroups

__global__ __launch_bounds__(256) void add_row_vec_kernel(float *__restrict__ x, const float *__restrict__ v, int E4, size_t n4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 b = reinterpret_cast<const float4 *>(v)[i % (size_t)E4];
    float4 a = reinterpret_cast<float4 *>(x)[i];
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    reinterpret_cast<float4 *>(x)[i] = a;
}

__global__ __launch_bounds__(256) void cvec_row_kernel(const float *__restrict__ D, const float *__restrict__ b, int R, int E, float *__restrict__ y) {
    const int row = blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    if (row >= R) return;                        // (the whole wave leaves)
    const float *d = D + (size_t)row * (size_t)E;
    float acc = 0.0f;
    for (int c = lane * 4; c < E; c += 256) {
        const float4 dv = *reinterpret_cast<const float4 *>(d + c), bv = *reinterpret_cast<const float4 *>(b + c);
        acc = fmaf(dv.x, bv.x, acc); acc = fmaf(dv.y, bv.y, acc); acc = fmaf(dv.z, bv.z, acc); acc = fmaf(dv.w, bv.w, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) y[row] = acc;
}

__device__ __forceinline__ void cv_axpy(float4 &acc, float w, const float4 d) {
    acc.x = fmaf(w, d.x, acc.x); acc.y = fmaf(w, d.y, acc.y); acc.z = fmaf(w, d.z, acc.z); acc.w = fmaf(w, d.w, acc.w);
}

// y == nullptr: every weight is 1
__global__ __launch_bounds__(256) void cvec_slab_kernel(const float *__restrict__ D, const float *__restrict__ y, int R, int E, int S, float *__restrict__ slabs) {
    const int c = blockIdx.x * CV_TILE + (int)threadIdx.x * 4, s = blockIdx.y;
    if (c >= E) return;
    const int r0 = s * S, r1 = min(r0 + S, R);
    float4 acc = float4{0.0f, 0.0f, 0.0f, 0.0f};
    int r = r0;
    for (; r + 4 <= r1; r += 4) {                // four rows in flight, added in row order
        float4 d[4];
        float w[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { d[i] = *reinterpret_cast<const float4 *>(D + (size_t)(r + i) * (size_t)E + (size_t)c); w[i] = y ? y[r + i] : 1.0f; }
#pragma unroll
        for (int i = 0; i < 4; i++) cv_axpy(acc, w[i], d[i]);
    }
    for (; r < r1; r++) cv_axpy(acc, y ? y[r] : 1.0f, *reinterpret_cast<const float4 *>(D + (size_t)r * (size_t)E + (size_t)c));
    *reinterpret_cast<float4 *>(slabs + (size_t)s * (size_t)E + (size_t)c) = acc;
}

// the workgroup's total, the same in every thread: wave_sum, then the 16 waves' sums in wave order
__device__ __forceinline__ float cv_block_sum(float v, float *red) {
    v = wave_sum(v);
    __syncthreads();                             // (red may still be read from the call before)
    if (((int)threadIdx.x & 63) == 0) red[(int)threadIdx.x >> 6] = v;
    __syncthreads();
    float t = red[0];
    for (int i = 1; i < CV_FIN / 64; i++) t += red[i];
    return t;
}

// z goes through slab 0 (a thread reads and writes its own columns only).  have_b == 0: b holds nothing yet, dist = 0.
__global__ __launch_bounds__(CV_FIN) void cvec_finish_kernel(float *__restrict__ slabs, int ns, int E, float scale, float *__restrict__ b, int have_b, float *__restrict__ dist) {
    __shared__ float red[CV_FIN / 64];
    const int tid = (int)threadIdx.x;
    float ss = 0.0f;
    for (int j = tid; j < E; j += CV_FIN) {
        float z = slabs[j];
        for (int s = 1; s < ns; s++) z += slabs[(size_t)s * (size_t)E + (size_t)j];
        z *= scale;
        slabs[j] = z;
        ss = fmaf(z, z, ss);
    }
    const float n2 = cv_block_sum(ss, red);
    if (!(n2 > 0.0f) || isinf(n2)) {             // a zero vector (-1), or a square that left f32 (-2): b stays
        if (tid == 0) dist[0] = n2 == 0.0f ? -1.0f : -2.0f;
        return;
    }
    const float n = sqrtf(n2);
    float dd = 0.0f;
    for (int j = tid; j < E; j += CV_FIN) {
        const float bn = slabs[j] / n;
        if (have_b) { const float df = bn - b[j]; dd = fmaf(df, df, dd); }
        b[j] = bn;
    }
    const float d2 = cv_block_sum(dd, red);
    if (tid == 0) dist[0] = sqrtf(d2);
}

__global__ __launch_bounds__(CV_FIN) void cvec_orient_kernel(const float *__restrict__ y, int R, float *__restrict__ b, int E) {
    __shared__ float red[CV_FIN / 64];
    const int tid = (int)threadIdx.x;
    float s = 0.0f;
    for (int r = tid; r < R; r += CV_FIN) s += y[r];
    if (cv_block_sum(s, red) >= 0.0f) return;
    for (int j = tid; j < E; j += CV_FIN) b[j] = -b[j];
}
}  // namespace

hipError_t launch_add_row_vec(float *x, const float *v, int E, int T, hipStream_t st) {
    if (!x || !v || E < 32 || (E & 31) || T < 1 || ((uintptr_t)x & 15) || ((uintptr_t)v & 15)) return hipErrorInvalidValue;
    const size_t n4 = (size_t)T * (size_t)(E / 4), blocks = (n4 + 255) / 256;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(add_row_vec_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, v, E / 4, n4);
    return hipGetLastError();
}

int cvec_slice_rows(int R) { return std::max(8, (R + CVEC_MAX_SLICES - 1) / CVEC_MAX_SLICES); }

size_t cvec_scratch_floats(int R, int E) {
    if (R < 1 || E < 1) return 0;
    const int S = cvec_slice_rows(R);
    return (size_t)((R + S - 1) / S) * (size_t)E;
}

bool cvec_pca_args_ok(const float *D, int R, int E) {
    return D && !((uintptr_t)D & 15) && R >= 1 && R <= CVEC_MAX_ROWS && E >= 32 && !(E & 31) && E <= CVEC_MAX_E;
}

static hipError_t cvec_slabs_finish(const float *D, int R, int E, const float *y, float scale, float *b, int have_b, float *slabs, float *dist, hipStream_t st) {
    const int S = cvec_slice_rows(R), ns = (R + S - 1) / S;
    hipLaunchKernelGGL(cvec_slab_kernel, dim3((unsigned)((E + CV_TILE - 1) / CV_TILE), (unsigned)ns), dim3(256), 0, st, D, y, R, E, S, slabs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cvec_finish_kernel, dim3(1), dim3(CV_FIN), 0, st, slabs, ns, E, scale, b, have_b, dist);
    return hipGetLastError();
}

static bool cvec_bufs_ok(const float *b, const float *slabs, const float *dist) { return b && !((uintptr_t)b & 15) && slabs && !((uintptr_t)slabs & 15) && dist; }

hipError_t launch_cvec_pca_step(const float *D, int R, int E, float *b, float *y, float *slabs, float *dist, hipStream_t st) {
    if (!cvec_pca_args_ok(D, R, E) || !cvec_bufs_ok(b, slabs, dist) || !y) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cvec_row_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, D, b, R, E, y);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return cvec_slabs_finish(D, R, E, y, 1.0f, b, 1, slabs, dist, st);
}

hipError_t launch_cvec_mean_step(const float *D, int R, int E, float *b, float *slabs, float *dist, hipStream_t st) {
    if (!cvec_pca_args_ok(D, R, E) || !cvec_bufs_ok(b, slabs, dist)) return hipErrorInvalidValue;
    return cvec_slabs_finish(D, R, E, nullptr, 1.0f / (float)R, b, 0, slabs, dist, st);
}

hipError_t launch_cvec_orient(const float *D, int R, int E, float *b, float *y, hipStream_t st) {
    if (!cvec_pca_args_ok(D, R, E) || !b || ((uintptr_t)b & 15) || !y) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cvec_row_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, D, b, R, E, y);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cvec_orient_kernel, dim3(1), dim3(CV_FIN), 0, st, y, R, b, E);
    return hipGetLastError();
}

}  // namespace mi355
