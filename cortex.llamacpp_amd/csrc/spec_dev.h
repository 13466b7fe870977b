// spec_dev.h — the row helpers the logits-row reductions share (spec.hip, logprob.hip): a row cut into SPEC_PARTS ranges, the walk over a range with 16-byte
// loads, the workgroup's and a wave's (value, index) winner, the index rule (the lowest index wins ties, a NaN never wins).  Device code only.
#pragma once
#include "kernels.h"

namespace mi355 {

constexpr int SPEC_PARTS = 64;
#define SPEC_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ void spec_take(float v, int i, float &best, int &idx) {
    if (v > best || (v == best && i < idx)) { best = v; idx = i; }
}
// a part's range as a scalar head up to the first 16-byte boundary, 16-byte loads, a scalar tail: any n, any row start
template <typename F>
__device__ __forceinline__ void spec_walk(const float *xr, int lo, int hi, int tid, F f) {
    if (lo >= hi) return;
    int head = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(xr + lo) >> 2) & 3u)) & 3u);
    if (head > hi - lo) head = hi - lo;
    const int v0 = lo + head, nv = (hi - v0) >> 2, t0 = v0 + 4 * nv;
    if (tid < head) f(xr[lo + tid], lo + tid);
    const float4 *x4 = reinterpret_cast<const float4 *>(xr + v0);
    for (int q = tid; q < nv; q += 256) {
        const float4 v = x4[q];
        const int i = v0 + 4 * q;
        f(v.x, i); f(v.y, i + 1); f(v.z, i + 2); f(v.w, i + 3);
    }
    if (tid < hi - t0) f(xr[t0 + tid], t0 + tid);
}
// the workgroup's (value, index) winner, known to EVERY thread afterwards (bv / bi: 4 words each; a barrier inside)
__device__ __forceinline__ void spec_block_argmax(float &best, int &idx, float *bv, int *bi) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    if (lane == 0) { bv[wave] = best; bi[wave] = idx; }
    __syncthreads();
    best = bv[0]; idx = bi[0];
#pragma unroll
    for (int w = 1; w < 4; w++)
        if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
}
__device__ __forceinline__ void spec_wave_argmax(float &b, int &i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(b, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (ov > b || (ov == b && oi < i)) { b = ov; i = oi; }
    }
}
__device__ __forceinline__ void spec_part_range(int n, int part, int &lo, int &hi) {
    const int chunk = (n + SPEC_PARTS - 1) / SPEC_PARTS;
    lo = part * chunk < n ? part * chunk : n;
    hi = lo + chunk < n ? lo + chunk : n;
}

}  // namespace mi355
