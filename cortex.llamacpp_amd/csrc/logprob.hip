// logprob.hip — what a perplexity / KL-divergence run needs of a logits row, so that no row moves to the host:
//   token_logprob_rows: per row the log-probability of one target token over the whole vocabulary, and the target's rank;
//   logits_kl_rows:     per pair of rows (P, Q) the divergence KL(P || Q) and whether the two arg-maxes agree.
// Both are argmax_prob_part_kernel's shape (spec.hip): grid (64 parts, rows), 256 threads, per-part partials in scratch (agent-scope relaxed atomics, drained
// before the ticket), the workgroup that draws a row's last ticket finishes the row and re-arms the counter - one launch, no host round trip.  Everything is
// f32 and every summation order is fixed (thread sums, a fixed xor tree over the wave, the four waves in order, the 64 parts in index order on one lane).
#include "spec_dev.h"

namespace mi355 {

__device__ __forceinline__ float lp_wave_sum(float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}
// the 64 lanes' terms added in lane order, the same value on every lane
__device__ __forceinline__ float lp_fold_in_order(float term) {
    float sum = 0.0f;
    for (int k = 0; k < SPEC_PARTS; k++) sum += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(term), k));
    return sum;
}
__device__ __forceinline__ bool lp_finite(float v) { return v > -INFINITY && v < INFINITY; }

// ---------------------------------------------------------------- log-probability and rank of a target
// A part leaves (m, s, c): its maximum, s = sum exp(x - m) over its non-NaN entries and c = how many of its entries beat the target (the target logit is read
// first, so one walk gives the maximum and the count).  The finisher: M = the largest m, S = sum_k s_k exp(m_k - M) in part order, logprob = (x_t - M) - log S.
__global__ __launch_bounds__(256) void token_logprob_part_kernel(const float *x, int n, const int32_t *rows, const int32_t *targets, float *pv, float *ps, int *pc,
                                                                 unsigned *cnt, float *logprob_out, int32_t *rank_out) {
    __shared__ float bv[4], sv[4];
    __shared__ int bi[4], cv[4];
    __shared__ int last_sh;
    const int row = blockIdx.y, part = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *xr = x + (size_t)(rows ? rows[row] : row) * n;
    const int t = targets[row];
    const bool t_ok = t >= 0 && t < n;                          // (the callers check; never read outside the row)
    const float xt = t_ok ? xr[t] : __int_as_float(0x7fc00000);
    int lo, hi;
    spec_part_range(n, part, lo, hi);
    float best = -INFINITY;
    int idx = 0x7fffffff, c = 0;
    spec_walk(xr, lo, hi, tid, [&](float v, int i) {
        spec_take(v, i, best, idx);
        c += (v > xt || (v == xt && i < t)) ? 1 : 0;
    });
    spec_block_argmax(best, idx, bv, bi);
    float s = 0.0f;
    if (lp_finite(best)) spec_walk(xr, lo, hi, tid, [&](float v, int) { if (v == v) s += expf(v - best); });
    s = lp_wave_sum(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) { sv[wave] = s; cv[wave] = c; }
    __syncthreads();
    if (tid == 0) {
        s = ((sv[0] + sv[1]) + sv[2]) + sv[3];
        c = cv[0] + cv[1] + cv[2] + cv[3];
        __hip_atomic_store(pv + row * SPEC_PARTS + part, best, SPEC_RLX_AGENT);
        __hip_atomic_store(ps + row * SPEC_PARTS + part, s, SPEC_RLX_AGENT);
        __hip_atomic_store(pc + row * SPEC_PARTS + part, c, SPEC_RLX_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the write-through stores have left before the ticket does
        const unsigned tk = __hip_atomic_fetch_add(cnt + row, 1u, SPEC_RLX_AGENT);
        last_sh = tk == SPEC_PARTS - 1 ? 1 : 0;
        if (last_sh) __hip_atomic_store(cnt + row, 0u, SPEC_RLX_AGENT);   // re-armed for the next launch
    }
    __syncthreads();
    if (!last_sh || tid >= 64) return;
    const float m = __hip_atomic_load(pv + row * SPEC_PARTS + tid, SPEC_RLX_AGENT);
    const float sp = __hip_atomic_load(ps + row * SPEC_PARTS + tid, SPEC_RLX_AGENT);
    int c2 = __hip_atomic_load(pc + row * SPEC_PARTS + tid, SPEC_RLX_AGENT);
    float M = m;
    int iM = tid;
    spec_wave_argmax(M, iM);
    const bool ok = lp_finite(M) && xt == xt;
    const float S = lp_fold_in_order(ok && m > -INFINITY ? sp * expf(m - M) : 0.0f);   // (a part with nothing comparable: m = -inf, s = 0)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c2 += __shfl_xor(c2, o, 64);
    if (tid == 0) {
        logprob_out[row] = ok ? (xt - M) - logf(S) : __int_as_float(0x7fc00000);
        rank_out[row] = ok ? c2 : -1;
    }
}
size_t token_logprob_scratch_words(int cap_rows) { return (size_t)cap_rows * (1 + 3 * SPEC_PARTS); }
hipError_t launch_token_logprob_rows(const float *base, int n, const int32_t *rows_dev, const int32_t *targets_dev, int R, float *logprob_out, int32_t *rank_out,
                                     float *scratch, int cap_rows, hipStream_t st) {
    if (n < 1 || n > SPEC_MAX_N || R < 1 || R > cap_rows || R > 65535 || !targets_dev) return hipErrorInvalidValue;
    unsigned *cnt = reinterpret_cast<unsigned *>(scratch);       // [cap_rows ticket words | part maxima | part sums | part counts]
    float *pv = scratch + cap_rows;
    float *ps = pv + (size_t)cap_rows * SPEC_PARTS;
    int *pc = reinterpret_cast<int *>(ps + (size_t)cap_rows * SPEC_PARTS);
    hipLaunchKernelGGL(token_logprob_part_kernel, dim3(SPEC_PARTS, R), dim3(256), 0, st, base, n, rows_dev, targets_dev, pv, ps, pc, cnt, logprob_out, rank_out);
    return hipGetLastError();
}

// ---------------------------------------------------------------- KL(P || Q) of two rows
// With p = softmax(x), q = softmax(y): KL = sum_j p_j (log p_j - log q_j) = sum_j p_j (x_j - y_j) - (lse_p - lse_q) = A / S_p - (lse_p - lse_q),
// A = sum_j exp(x_j - M_p) (x_j - y_j), lse = M + log S.  A part leaves, rescaled to ITS maxima, the triple (m_p, s_p, a) and the pair (m_q, s_q), both
// (value, index) winners and whether it met a non-finite entry; the finisher rescales to the row maxima and adds in part order.  lse_p and lse_q come out of
// one operation sequence each on its own row, so identical rows give bit-equal values, A = 0 and KL = 0.0f exactly.
__global__ __launch_bounds__(256) void logits_kl_part_kernel(const float *xb, const float *yb, int n, const int32_t *rows_p, const int32_t *rows_q, float *part,
                                                             unsigned *cnt, int cap_rows, float *kl_out, int32_t *same_top_out) {
    __shared__ float bvx[4], bvy[4], sv[3][4];
    __shared__ int bix[4], biy[4], badv[4];
    __shared__ int last_sh;
    const int row = blockIdx.y, part_i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *xr = xb + (size_t)(rows_p ? rows_p[row] : row) * n;
    const float *yr = yb + (size_t)(rows_q ? rows_q[row] : row) * n;
    int lo, hi;
    spec_part_range(n, part_i, lo, hi);
    float bx = -INFINITY, by = -INFINITY;
    int ix = 0x7fffffff, iy = 0x7fffffff, bad = 0;
    spec_walk(xr, lo, hi, tid, [&](float v, int i) { spec_take(v, i, bx, ix); bad |= lp_finite(v) ? 0 : 1; });
    spec_walk(yr, lo, hi, tid, [&](float v, int i) { spec_take(v, i, by, iy); bad |= lp_finite(v) ? 0 : 1; });
    spec_block_argmax(bx, ix, bvx, bix);
    spec_block_argmax(by, iy, bvy, biy);
    bad = __any(bad) ? 1 : 0;
    if (lane == 0) badv[wave] = bad;
    __syncthreads();
    bad = badv[0] | badv[1] | badv[2] | badv[3];
    float sp = 0.0f, a = 0.0f, sq = 0.0f;
    if (!bad) spec_walk(xr, lo, hi, tid, [&](float v, int i) {     // (both ranges are in cache from the first walks; an empty part walks nothing)
        const float w = yr[i], e = expf(v - bx);
        sp += e;
        a += e * (v - w);
        sq += expf(w - by);
    });
    sp = lp_wave_sum(sp); a = lp_wave_sum(a); sq = lp_wave_sum(sq);
    if (lane == 0) { sv[0][wave] = sp; sv[1][wave] = a; sv[2][wave] = sq; }
    __syncthreads();
    // the row's words: 8 planes of cap_rows * 64
    const size_t plane = (size_t)cap_rows * SPEC_PARTS, at = (size_t)row * SPEC_PARTS;
    if (tid == 0) {
        sp = ((sv[0][0] + sv[0][1]) + sv[0][2]) + sv[0][3];
        a = ((sv[1][0] + sv[1][1]) + sv[1][2]) + sv[1][3];
        sq = ((sv[2][0] + sv[2][1]) + sv[2][2]) + sv[2][3];
        int *parti = reinterpret_cast<int *>(part);
        __hip_atomic_store(part + 0 * plane + at + part_i, bx, SPEC_RLX_AGENT);
        __hip_atomic_store(parti + 1 * plane + at + part_i, ix, SPEC_RLX_AGENT);
        __hip_atomic_store(part + 2 * plane + at + part_i, sp, SPEC_RLX_AGENT);
        __hip_atomic_store(part + 3 * plane + at + part_i, a, SPEC_RLX_AGENT);
        __hip_atomic_store(part + 4 * plane + at + part_i, by, SPEC_RLX_AGENT);
        __hip_atomic_store(parti + 5 * plane + at + part_i, iy, SPEC_RLX_AGENT);
        __hip_atomic_store(part + 6 * plane + at + part_i, sq, SPEC_RLX_AGENT);
        __hip_atomic_store(parti + 7 * plane + at + part_i, bad, SPEC_RLX_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the write-through stores have left before the ticket does
        const unsigned tk = __hip_atomic_fetch_add(cnt + row, 1u, SPEC_RLX_AGENT);
        last_sh = tk == SPEC_PARTS - 1 ? 1 : 0;
        if (last_sh) __hip_atomic_store(cnt + row, 0u, SPEC_RLX_AGENT);   // re-armed for the next launch
    }
    __syncthreads();
    if (!last_sh || tid >= 64) return;
    const int *parti = reinterpret_cast<const int *>(part);
    const float mp = __hip_atomic_load(part + 0 * plane + at + tid, SPEC_RLX_AGENT);
    int ip = __hip_atomic_load(parti + 1 * plane + at + tid, SPEC_RLX_AGENT);
    const float sp_k = __hip_atomic_load(part + 2 * plane + at + tid, SPEC_RLX_AGENT);
    const float a_k = __hip_atomic_load(part + 3 * plane + at + tid, SPEC_RLX_AGENT);
    const float mq = __hip_atomic_load(part + 4 * plane + at + tid, SPEC_RLX_AGENT);
    int iq = __hip_atomic_load(parti + 5 * plane + at + tid, SPEC_RLX_AGENT);
    const float sq_k = __hip_atomic_load(part + 6 * plane + at + tid, SPEC_RLX_AGENT);
    const int bad_k = __hip_atomic_load(parti + 7 * plane + at + tid, SPEC_RLX_AGENT);
    float Mp = mp, Mq = mq;
    spec_wave_argmax(Mp, ip);
    spec_wave_argmax(Mq, iq);
    const bool ok = !__any(bad_k) && lp_finite(Mp) && lp_finite(Mq);
    const float wp = ok && mp > -INFINITY ? expf(mp - Mp) : 0.0f, wq = ok && mq > -INFINITY ? expf(mq - Mq) : 0.0f;   // (an empty part: m = -inf, sums 0)
    const float Sp = lp_fold_in_order(sp_k * wp);
    const float Sq = lp_fold_in_order(sq_k * wq);
    const float A = lp_fold_in_order(a_k * wp);
    if (tid == 0) {
        const float lse_p = Mp + logf(Sp), lse_q = Mq + logf(Sq);
        kl_out[row] = ok ? A / Sp - (lse_p - lse_q) : __int_as_float(0x7fc00000);
        same_top_out[row] = ok ? (ip == iq ? 1 : 0) : -1;
    }
}
size_t logits_kl_scratch_words(int cap_rows) { return (size_t)cap_rows * (1 + 8 * SPEC_PARTS); }
hipError_t launch_logits_kl_rows(const float *base_p, const float *base_q, int n, const int32_t *rows_p_dev, const int32_t *rows_q_dev, int R, float *kl_out,
                                 int32_t *same_top_out, float *scratch, int cap_rows, hipStream_t st) {
    if (n < 1 || n > SPEC_MAX_N || R < 1 || R > cap_rows || R > 65535) return hipErrorInvalidValue;
    unsigned *cnt = reinterpret_cast<unsigned *>(scratch);       // [cap_rows ticket words | 8 planes of cap_rows * 64: m_p, i_p, s_p, a, m_q, i_q, s_q, non-finite]
    hipLaunchKernelGGL(logits_kl_part_kernel, dim3(SPEC_PARTS, R), dim3(256), 0, st, base_p, base_q, n, rows_p_dev, rows_q_dev, scratch + cap_rows, cnt, cap_rows,
                       kl_out, same_top_out);
    return hipGetLastError();
}

}  // namespace mi355
