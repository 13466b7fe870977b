// imatrix.hip — the importance-matrix collector (what upstream's llama-imatrix records): for the f32 rows a projection consumes,
//   sum2[m][j] += sum over the rows r of matrix m of v[r][j]^2,   count[m] += rows of m,      j < K,
// with v = x[r] or silu(x[r]) * x2[r], launch row r read from source row row_src[r] where a table is given, and the rows of a launch either all one matrix's
// or cut by expert as launch_moe_group's meta array says (counts | exclusive offsets | total), read on the device.
//
// Two launches, no atomics, every order fixed - the same bits run to run:
//   slab pass: the rows of a matrix are cut into slices of S = imatrix_slice_rows(R) rows, at most 64 slices over the whole launch.  A workgroup owns one slice
//     and 1024 columns; a thread owns four adjacent columns (one 16-byte load per row: a wave reads 1 KB of a row) and adds its rows' squares in row order,
//     then stores its four sums into the slice's f32 slab.  Every input element is read once.
//   sum pass: a thread owns one column of one matrix and adds the matrix's slabs in slice order, then adds the result to the running total.
// Per-expert launches: expert e's slices are slabs base(e) .. base(e) + ceil(count[e] / S) - 1 with base(e) = offset[e] / S + e, which never overlap (the next
// expert's base is at least that many further on) and stay below R / S + n_mat + 1.  The grid has one slot per possible slab; a workgroup finds its expert by
// a binary search of base() and leaves when its slice is past the expert's rows, so an expert without rows costs neither slab traffic nor a word of its totals.
#include <algorithm>

#include "dev_common.h"
#include "kernels.h"

namespace mi355 {

namespace {
constexpr int IMX_MAX_MAT = 256;      // (the router's and launch_moe_group's expert limit)
constexpr int IMX_TILE = 1024;        // columns of a slab-pass workgroup (256 threads x 4)
constexpr int IMX_MAX_SLICES = 64;    // slices of a launch's rows (dense); per-expert launches add at most one slab per expert

__device__ __forceinline__ void imx_add_sq(float4 &acc, const float4 v) {
    acc.x = fmaf(v.x, v.x, acc.x); acc.y = fmaf(v.y, v.y, acc.y); acc.z = fmaf(v.z, v.z, acc.z); acc.w = fmaf(v.w, v.w, acc.w);
}

template <bool GLU>
__device__ __forceinline__ float4 imx_load(const float *x, const float *x2, size_t at) {
    float4 v = *reinterpret_cast<const float4 *>(x + at);
    if (GLU) {
        const float4 u = *reinterpret_cast<const float4 *>(x2 + at);
        v = float4{swiglu_f32(v.x, u.x), swiglu_f32(v.y, u.y), swiglu_f32(v.z, u.z), swiglu_f32(v.w, u.w)};
    }
    return v;
}

// matrix m's rows of the launch: (count, first row).  meta == nullptr: one matrix, all R rows
__device__ __forceinline__ void imx_rows_of(const int32_t *meta, int n_mat, int R, int m, int &cnt, int &off) {
    if (meta) { cnt = meta[m]; off = meta[n_mat + m]; } else { cnt = R; off = 0; }
    // (a meta array that does not describe this launch must not send a read outside it)
    if (cnt < 0 || off < 0 || off > R || cnt > R - off) cnt = 0;
}

template <bool GLU>
__global__ __launch_bounds__(256) void imatrix_slab_kernel(const float *__restrict__ x, const float *__restrict__ x2, int ld, int K, int R,
                                                           const int32_t *__restrict__ row_src, const int32_t *__restrict__ meta, int n_mat, int S,
                                                           float *__restrict__ slabs) {
    const int c = blockIdx.x * IMX_TILE + (int)threadIdx.x * 4, slot = blockIdx.y;
    int m = 0;
    if (meta) {                                  // the largest m with base(m) <= slot (base(0) = 0, strictly increasing)
        int lo = 0, hi = n_mat - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            const int off = meta[n_mat + mid];
            if ((off < 0 ? 0 : off) / S + mid <= slot) lo = mid; else hi = mid - 1;
        }
        m = lo;
    }
    int cnt, off;
    imx_rows_of(meta, n_mat, R, m, cnt, off);
    const int s = slot - (off / S + m);
    if (s < 0 || (long long)s * S >= cnt || c >= K) return;
    const int r0 = off + s * S, r1 = min(r0 + S, off + cnt);
    float4 acc = float4{0.0f, 0.0f, 0.0f, 0.0f};
    int r = r0;
    for (; r + 4 <= r1; r += 4) {                // four rows in flight, added in row order
        size_t at[4];
#pragma unroll
        for (int i = 0; i < 4; i++) at[i] = (size_t)(row_src ? row_src[r + i] : r + i) * (size_t)ld + (size_t)c;
        float4 v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = imx_load<GLU>(x, x2, at[i]);
#pragma unroll
        for (int i = 0; i < 4; i++) imx_add_sq(acc, v[i]);
    }
    for (; r < r1; r++) imx_add_sq(acc, imx_load<GLU>(x, x2, (size_t)(row_src ? row_src[r] : r) * (size_t)ld + (size_t)c));
    *reinterpret_cast<float4 *>(slabs + (size_t)slot * K + c) = acc;
}

__global__ __launch_bounds__(256) void imatrix_sum_kernel(const float *__restrict__ slabs, const int32_t *__restrict__ meta, int n_mat, int K, int R, int S,
                                                          float *__restrict__ sum2, int32_t *__restrict__ count) {
    const int j = blockIdx.x * 256 + (int)threadIdx.x, m = blockIdx.y;
    int cnt, off;
    imx_rows_of(meta, n_mat, R, m, cnt, off);
    if (cnt <= 0) return;                        // an expert without rows: its totals are not touched
    if (j == 0) count[m] += cnt;
    if (j >= K) return;
    const int ns = (cnt + S - 1) / S;                // exactly the slabs the slab pass wrote: a slot past the matrix's rows was skipped there and holds stale floats
    const float *p = slabs + (size_t)(off / S + m) * K + j;
    float tot = p[0];
    for (int s = 1; s < ns; s++) tot += p[(size_t)s * K];
    sum2[(size_t)m * K + j] += tot;
}
}  // namespace

int imatrix_slice_rows(int R) { return std::max(8, (R + IMX_MAX_SLICES - 1) / IMX_MAX_SLICES); }

// slabs a launch of r rows touches: below r / S(r) + n_mat + 1 (above)
static size_t imx_launch_slabs(int r, int n_mat) { return (size_t)(r / imatrix_slice_rows(r) + n_mat + 1); }

// The slab count is not monotone in the rows (600 rows: S = 10, 60 slices; 512 rows: S = 8, 64 slices), so the scratch of "up to R rows" is the largest over
// every r <= R: r / S(r) <= r / 8 and <= IMX_MAX_SLICES, both reached at or below R.
size_t imatrix_scratch_floats(int K, int R, int n_mat) {
    if (K < 1 || R < 1 || n_mat < 1) return 0;
    return (size_t)(std::min(IMX_MAX_SLICES, (R + 7) / 8) + n_mat + 1) * (size_t)K;
}

bool imatrix_accum_ok(const float *x, const float *x2, int ld, int K, int R, const int32_t *meta, int n_mat) {
    if (!x || K < 32 || (K & 31) || ld < K || (ld & 3) || R < 1 || R > IMX_MAX_ROWS || n_mat < 1 || n_mat > IMX_MAX_MAT) return false;
    if (n_mat > 1 && !meta) return false;
    if (((uintptr_t)x & 15) || ((uintptr_t)x2 & 15)) return false;
    return true;
}

hipError_t launch_imatrix_accum(const float *x, const float *x2, int ld, int K, int R, const int32_t *row_src, const int32_t *meta, int n_mat, float *sum2,
                                int32_t *count, float *slabs, size_t slab_floats, hipStream_t st) {
    if (!imatrix_accum_ok(x, x2, ld, K, R, meta, n_mat) || !sum2 || !count || !slabs || ((uintptr_t)slabs & 15)) return hipErrorInvalidValue;
    if (imx_launch_slabs(R, n_mat) * (size_t)K > slab_floats) return hipErrorInvalidValue;      // the scratch does not hold this launch's slabs
    const int S = imatrix_slice_rows(R);
    const int slots = (R + S - 1) / S + (meta ? n_mat : 0);
    const dim3 g1((unsigned)((K + IMX_TILE - 1) / IMX_TILE), (unsigned)slots), g2((unsigned)((K + 255) / 256), (unsigned)n_mat);
    if (x2) hipLaunchKernelGGL(imatrix_slab_kernel<true>, g1, dim3(256), 0, st, x, x2, ld, K, R, row_src, meta, n_mat, S, slabs);
    else hipLaunchKernelGGL(imatrix_slab_kernel<false>, g1, dim3(256), 0, st, x, x2, ld, K, R, row_src, meta, n_mat, S, slabs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(imatrix_sum_kernel, g2, dim3(256), 0, st, slabs, meta, n_mat, K, R, S, sum2, count);
    return hipGetLastError();
}

}  // namespace mi355
