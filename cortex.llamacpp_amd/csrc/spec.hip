// spec.hip — the two device-side decisions of a speculative-decoding round, so that neither moves a logits row to the host:
//   argmax_prob_rows: per row the arg-max AND its softmax probability (the draft model's "am I still confident" test);
//   spec_verify:      the arg-max of every row of a verify batch and, per group of rows, how many drafted tokens the target model agrees with.
// Both are argmax_part_kernel's shape (misc.hip): grid (64 parts, rows), 256 threads, a per-row partial in scratch, the last workgroup to take a ticket on the
// row's counter finishes the row - one launch, no host round trip.  The index rule is that kernel's: the lowest index wins ties, a NaN never wins, a row of
// NaNs gives 0.
#include "spec_dev.h"

namespace mi355 {

// ---------------------------------------------------------------- arg-max and its probability
// p = 1 / sum_j exp(x_j - max) over the non-NaN entries, in f32.  A part leaves the online-softmax pair (m, s): its maximum and s = sum exp(x - m) over its
// range (thread sums, a fixed xor tree over the wave, the four waves in order).  The finisher folds the pairs in part order, 0 .. 63: the row maximum M is the
// arg-max's value, so every fold step rescales to the maximum the walk would end on, s_i * exp(m_i - M), and lane 0 adds those 64 terms in index order -
// the same bits run to run.  A row whose maximum is not finite (all NaN, all -inf, a +inf entry) gives p = 0.
__global__ __launch_bounds__(256) void argmax_prob_part_kernel(const float *x, int n, const int32_t *rows, float *pv, int *pi, float *ps, unsigned *cnt,
                                                               int32_t *idx_out, float *p_out) {
    __shared__ float bv[4], sv[4];
    __shared__ int bi[4];
    __shared__ int last_sh;
    const int row = blockIdx.y, part = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *xr = x + (size_t)(rows ? rows[row] : row) * n;
    int lo, hi;
    spec_part_range(n, part, lo, hi);
    float best = -INFINITY;
    int idx = 0x7fffffff;
    spec_walk(xr, lo, hi, tid, [&](float v, int i) { spec_take(v, i, best, idx); });
    spec_block_argmax(best, idx, bv, bi);
    const bool finite = best > -INFINITY && best < INFINITY;
    float s = 0.0f;
    if (finite) spec_walk(xr, lo, hi, tid, [&](float v, int) { if (v == v) s += expf(v - best); });      // (the range is in cache from the first walk)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) sv[wave] = s;
    __syncthreads();
    if (tid == 0) {
        s = ((sv[0] + sv[1]) + sv[2]) + sv[3];
        __hip_atomic_store(pv + row * SPEC_PARTS + part, best, SPEC_RLX_AGENT);
        __hip_atomic_store(pi + row * SPEC_PARTS + part, idx, SPEC_RLX_AGENT);
        __hip_atomic_store(ps + row * SPEC_PARTS + part, s, SPEC_RLX_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the write-through stores have left before the ticket does
        const unsigned t = __hip_atomic_fetch_add(cnt + row, 1u, SPEC_RLX_AGENT);
        last_sh = t == SPEC_PARTS - 1 ? 1 : 0;
        if (last_sh) __hip_atomic_store(cnt + row, 0u, SPEC_RLX_AGENT);   // re-armed for the next launch
    }
    __syncthreads();
    if (!last_sh || tid >= 64) return;
    const float m = __hip_atomic_load(pv + row * SPEC_PARTS + tid, SPEC_RLX_AGENT);
    const float sp = __hip_atomic_load(ps + row * SPEC_PARTS + tid, SPEC_RLX_AGENT);
    float b2 = m;
    int i2 = __hip_atomic_load(pi + row * SPEC_PARTS + tid, SPEC_RLX_AGENT);
    spec_wave_argmax(b2, i2);
    const bool ok = b2 > -INFINITY && b2 < INFINITY;
    const float term = ok && m > -INFINITY ? sp * expf(m - b2) : 0.0f;   // (a part with nothing comparable: m = -inf, s = 0)
    float sum = 0.0f;
    for (int k = 0; k < SPEC_PARTS; k++) sum += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(term), k));
    if (tid == 0) {
        idx_out[row] = i2 == 0x7fffffff ? 0 : i2;
        p_out[row] = ok ? 1.0f / sum : 0.0f;
    }
}
size_t argmax_prob_scratch_words(int cap_rows) { return (size_t)cap_rows * (1 + 3 * SPEC_PARTS); }
hipError_t launch_argmax_prob_rows(const float *x, int n, const int32_t *rows_dev, int rows, int32_t *idx_out, float *p_out, float *scratch, int cap_rows,
                                   hipStream_t st) {
    if (n < 1 || n > SPEC_MAX_N || rows < 1 || rows > cap_rows || rows > 65535) return hipErrorInvalidValue;
    unsigned *cnt = reinterpret_cast<unsigned *>(scratch);       // at the head, as in launch_argmax_rows
    float *pv = scratch + cap_rows;
    int *pi = reinterpret_cast<int *>(pv + (size_t)cap_rows * SPEC_PARTS);
    float *ps = pv + 2 * (size_t)cap_rows * SPEC_PARTS;
    hipLaunchKernelGGL(argmax_prob_part_kernel, dim3(SPEC_PARTS, rows), dim3(256), 0, st, x, n, rows_dev, pv, pi, ps, cnt, idx_out, p_out);
    return hipGetLastError();
}

// ---------------------------------------------------------------- greedy acceptance of a verify batch
// Row r of the launch is logits row rows[r] of `base`; group g owns rows group_start[g] .. group_start[g + 1] - 1: k_g + 1 rows for k_g drafted tokens, row j
// of the group being the target's answer to "what follows draft j - 1".  ids[r] = the row's arg-max; n_accept[g] = the largest a <= k_g with ids[j] == draft[j]
// for the group's first a rows (the draft entry of a group's last row is not looked at).  A row's finisher stores its id device-coherently, drains the store
// and takes a ticket on ONE counter over all R rows; whoever draws the last ticket therefore finds every id final and scans the groups, one lane each.
__global__ __launch_bounds__(256) void spec_verify_kernel(const float *base, int n, const int32_t *rows, int R, const int32_t *group_start, int G, const int32_t *draft,
                                                          float *pv, int *pi, unsigned *cnt, unsigned *done, int32_t *ids_dev, int32_t *ids_out, int32_t *n_accept_out) {
    __shared__ float bv[4];
    __shared__ int bi[4];
    __shared__ int last_sh;
    const int row = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const float *xr = base + (size_t)rows[row] * n;
    int lo, hi;
    spec_part_range(n, part, lo, hi);
    float best = -INFINITY;
    int idx = 0x7fffffff;
    spec_walk(xr, lo, hi, tid, [&](float v, int i) { spec_take(v, i, best, idx); });
    spec_block_argmax(best, idx, bv, bi);
    if (tid == 0) {
        __hip_atomic_store(pv + row * SPEC_PARTS + part, best, SPEC_RLX_AGENT);
        __hip_atomic_store(pi + row * SPEC_PARTS + part, idx, SPEC_RLX_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(cnt + row, 1u, SPEC_RLX_AGENT);
        last_sh = t == SPEC_PARTS - 1 ? 1 : 0;
        if (last_sh) __hip_atomic_store(cnt + row, 0u, SPEC_RLX_AGENT);
    }
    __syncthreads();
    if (!last_sh || tid >= 64) return;
    float b2 = __hip_atomic_load(pv + row * SPEC_PARTS + tid, SPEC_RLX_AGENT);
    int i2 = __hip_atomic_load(pi + row * SPEC_PARTS + tid, SPEC_RLX_AGENT);
    spec_wave_argmax(b2, i2);
    int all = 0;
    if (tid == 0) {
        const int id = i2 == 0x7fffffff ? 0 : i2;
        ids_out[row] = id;
        __hip_atomic_store(ids_dev + row, id, SPEC_RLX_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the id has left before this row counts as done
        const unsigned t = __hip_atomic_fetch_add(done, 1u, SPEC_RLX_AGENT);
        all = t == (unsigned)R - 1u ? 1 : 0;
        if (all) __hip_atomic_store(done, 0u, SPEC_RLX_AGENT);
    }
    all = __shfl(all, 0, 64);
    if (!all || tid >= G) return;
    const int g0 = group_start[tid], g1 = group_start[tid + 1];
    int a = 0;
    for (int j = g0; j < g1 - 1; j++) {
        if (__hip_atomic_load(ids_dev + j, SPEC_RLX_AGENT) != draft[j]) break;
        a++;
    }
    n_accept_out[tid] = a;
}
size_t spec_verify_scratch_words(int cap_rows) { return 4 + (size_t)cap_rows * (2 + 2 * SPEC_PARTS); }
hipError_t launch_spec_verify(const float *base, int n, const int32_t *rows_dev, int R, const int32_t *group_start_dev, int G, const int32_t *draft_dev,
                              int32_t *ids_out, int32_t *n_accept_out, float *scratch, int cap_rows, hipStream_t st) {
    if (n < 1 || n > SPEC_MAX_N || R < 1 || R > cap_rows || R > SPEC_MAX_ROWS || G < 1 || G > SPEC_MAX_GROUPS) return hipErrorInvalidValue;
    unsigned *done = reinterpret_cast<unsigned *>(scratch);      // [4 words: the launch's counter | cap_rows row tickets | cap_rows ids | part values | part indices]
    unsigned *cnt = done + 4;
    int32_t *ids_dev = reinterpret_cast<int32_t *>(cnt + cap_rows);
    float *pv = scratch + 4 + 2 * (size_t)cap_rows;
    int *pi = reinterpret_cast<int *>(pv + (size_t)cap_rows * SPEC_PARTS);
    hipLaunchKernelGGL(spec_verify_kernel, dim3(SPEC_PARTS, R), dim3(256), 0, st, base, n, rows_dev, R, group_start_dev, G, draft_dev, pv, pi, cnt, done, ids_dev,
                       ids_out, n_accept_out);
    return hipGetLastError();
}

}  // namespace mi355
