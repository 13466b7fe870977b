// sample.hip — the tail of the sampler chain and the draw, on the device: what Sampler::finish (host/sampling.cc) does with the k <= 128
// candidates of launch_topk_rows, for many rows in one launch, so that a sampled step brings one token per row to the host instead of k pairs per call.
//   work split: one wave64 per row, SAMPLE_WAVES waves per workgroup, grid = ceil(R / SAMPLE_WAVES); a row's wave never talks to another: no LDS, no atomics,
//               no barrier, no scratch.  Lane l holds the candidates of rank l and l + 64 in registers (k <= 64: the second set stays empty).
//   sums:       xor butterflies (every lane gets the total) and shift-up prefix sums over the two register sets, rank order = set 0's lanes, then set 1's.
//   typical-p:  an in-wave bitonic sort of 128 keys (|-log p - H| as f32 bits) << 8 | rank, two keys per lane: strides below 64 exchange by shuffle, stride
//               64 is the lane's own pair.  Only keys move: a sorted position fetches its probability from the rank's owner by shuffle, and a lane learns
//               whether its rank survived by comparing its own key with the key at the cut (the keys are distinct).
//   arithmetic: f64.  The candidates' weights stay unnormalised, w_i = exp(l_i - l_0): a cut compares a prefix sum with threshold * total, min_p compares
//               weights, and the temperature's p^(1/T) is exp((l_i - l_first) / T) - so a probability that leaves here has seen one exp, one sum of at most
//               128 terms and one division, whatever cuts were on (the host renormalises after each cut; the same real numbers).
//   draw:       Philox4x32-10 from its published round function (Salmon et al., SC'11), every lane the same words.
#include "kernels.h"
#include "philox.h"

namespace mi355 {

constexpr int SAMPLE_WAVES = 4;

// ---------------------------------------------------------------- Philox4x32-10 (philox.h)
__global__ void philox_u_kernel(unsigned long long seed, unsigned long long counter0, unsigned stream, int n, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = philox_u(seed, counter0 + (unsigned long long)i, stream);
}

// ---------------------------------------------------------------- wave helpers over the two register sets
__device__ __forceinline__ double smp_sum2(double a, double b) {               // the 128 values' sum, on every lane
    double s = a + b;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}
// inclusive prefix sums in rank order; returns the total
__device__ __forceinline__ double smp_scan2(double &a, double &b, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double ta = __shfl_up(a, o, 64), tb = __shfl_up(b, o, 64);
        if (lane >= o) { a += ta; b += tb; }
    }
    b += __shfl(a, 63, 64);
    return __shfl(b, 63, 64);
}
// the value rank r's owner holds (r in [0, 128); the same r or not on every lane)
__device__ __forceinline__ double smp_at(double a, double b, int r) {
    const double x = __shfl(a, r & 63, 64), y = __shfl(b, r & 63, 64);
    return (r & 64) ? y : x;
}
__device__ __forceinline__ unsigned long long smp_at(unsigned long long a, unsigned long long b, int r) {
    const unsigned long long x = __shfl(a, r & 63, 64), y = __shfl(b, r & 63, 64);
    return (r & 64) ? y : x;
}
// the lowest rank whose flag is set (128: none), the same on every lane
__device__ __forceinline__ int smp_first(bool fa, bool fb) {
    const unsigned long long ma = __ballot(fa), mb = __ballot(fb);
    return ma ? __ffsll((long long)ma) - 1 : mb ? 64 + __ffsll((long long)mb) - 1 : 128;
}
// how many set flags precede this lane's two ranks; n: how many are set at all
__device__ __forceinline__ void smp_index2(bool fa, bool fb, int lane, int &ia, int &ib, int &n) {
    const unsigned long long ma = __ballot(fa), mb = __ballot(fb), below = (1ull << lane) - 1ull;
    ia = __popcll(ma & below);
    ib = __popcll(ma) + __popcll(mb & below);
    n = __popcll(ma) + __popcll(mb);
}
// ascending bitonic sort of the 128 keys (position = set * 64 + lane)
__device__ __forceinline__ void smp_sort2(unsigned long long &a, unsigned long long &b, int lane) {
#pragma unroll
    for (int size = 2; size <= 128; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (stride == 64) {                                                  // (size 128 only: every pair ascends)
                const unsigned long long lo = a < b ? a : b, hi = a < b ? b : a;
                a = lo; b = hi;
            } else {
                const unsigned long long pa = __shfl_xor(a, stride, 64), pb = __shfl_xor(b, stride, 64);
                const bool low = (lane & stride) == 0;                           // this lane holds the lower position of its pairs
                const bool up_a = (lane & size) == 0, up_b = ((lane + 64) & size) == 0;
                a = (low == up_a) ? (a < pa ? a : pa) : (a < pa ? pa : a);
                b = (low == up_b) ? (b < pb ? b : pb) : (b < pb ? pb : b);
            }
        }
    }
}

// ---------------------------------------------------------------- the chain
__global__ __launch_bounds__(64 * SAMPLE_WAVES) void sample_rows_kernel(const unsigned long long *keys, int R, int k, const SampleParams *params, const double *u_in,
                                                                        int32_t *tokens_out, float *probs_out, int32_t *n_kept_out, int32_t *kept_tok, float *kept_p) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * SAMPLE_WAVES + (threadIdx.x >> 6);
    if (row >= R) return;                                                        // (a whole wave: nothing below waits for another wave)
    const SampleParams sp = params[row];
    const int mk = sp.min_keep > 1 ? sp.min_keep : 1;
    // 1. the top_k cut (the front already kept max(top_k, min_keep) where it was asked to; a launch serves its largest row)
    int n = k;
    if (sp.top_k > 0) { const int want = sp.top_k > mk ? sp.top_k : mk; n = want < k ? want : k; }
    const bool va = lane < n, vb = lane + 64 < n;
    const unsigned long long *kr = keys + (size_t)row * TOPK_MAX_K;
    const unsigned long long ka = va ? kr[lane] : 0ull, kb = vb ? kr[lane + 64] : 0ull;
    auto logit_of = [](unsigned long long key) {
        unsigned u = (unsigned)(key >> 32);
        u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;                              // inverse of the order-preserving image
        return __uint_as_float(u);
    };
    const int ta = (int)(0xffffffffu - (unsigned)ka), tb = (int)(0xffffffffu - (unsigned)kb);
    const float la = va ? logit_of(ka) : -INFINITY, lb = vb ? logit_of(kb) : -INFINITY;
    const float best = __shfl(la, 0, 64);
    int *kt = kept_tok ? kept_tok + (size_t)row * TOPK_MAX_K : nullptr;
    float *kp = kept_tok ? kept_p + (size_t)row * TOPK_MAX_K : nullptr;
    if (!(best > -INFINITY && best < INFINITY)) {
        if (lane == 0) { tokens_out[row] = -1; probs_out[row] = 0.0f; if (n_kept_out) n_kept_out[row] = 0; }
        return;
    }
    if (sp.temp <= 0.0f) {                                                       // the front's arg-max rule; no draw
        if (lane == 0) { tokens_out[row] = ta; probs_out[row] = 1.0f; if (n_kept_out) n_kept_out[row] = 1; if (kt) { kt[0] = ta; kp[0] = 1.0f; } }
        return;
    }
    const double ea = va ? exp((double)la - (double)best) : 0.0, eb = vb ? exp((double)lb - (double)best) : 0.0;
    bool fa = va, fb = vb;                                                       // kept
    // 2. typical-p: the shortest prefix, in order of |-log p - H| (ties: the rank), whose mass exceeds typ_p
    if (sp.typ_p < 1.0f && n > 1) {
        const double s0 = smp_sum2(ea, eb), pa = ea / s0, pb = eb / s0;
        const double h = smp_sum2(pa > 0.0 ? -pa * log(pa) : 0.0, pb > 0.0 ? -pb * log(pb) : 0.0);
        const double tiny = (double)1e-30f;
        const float da = (float)fabs(-log(pa > tiny ? pa : tiny) - h), db = (float)fabs(-log(pb > tiny ? pb : tiny) - h);
        const unsigned long long mine_a = va ? ((unsigned long long)__float_as_uint(da) << 8) | (unsigned)lane : ~0ull;
        const unsigned long long mine_b = vb ? ((unsigned long long)__float_as_uint(db) << 8) | (unsigned)(lane + 64) : ~0ull;
        unsigned long long sa = mine_a, sb = mine_b;
        smp_sort2(sa, sb, lane);
        double ca = smp_at(pa, pb, (int)(sa & 127u)), cb = smp_at(pa, pb, (int)(sb & 127u));
        if (sa == ~0ull) ca = 0.0;
        if (sb == ~0ull) cb = 0.0;
        smp_scan2(ca, cb, lane);
        const int first = smp_first(va && ca > (double)sp.typ_p && lane + 1 >= mk, vb && cb > (double)sp.typ_p && lane + 65 >= mk);   // (positions < n are valid keys)
        const int last = first < 128 ? first + 1 : n;
        const unsigned long long cut = smp_at(sa, sb, last - 1);
        fa = va && mine_a <= cut; fb = vb && mine_b <= cut;
    }
    const int head = smp_first(fa, fb);                                          // the best kept candidate: the cuts below keep a prefix of the kept, so it stays
    int ia, ib, n_kept;
    // 3. top_p over the kept candidates' renormalised probabilities: the first whose running mass reaches top_p is the last kept
    if (sp.top_p < 1.0f) {
        double ca = fa ? ea : 0.0, cb = fb ? eb : 0.0;
        const double s1 = smp_scan2(ca, cb, lane);
        smp_index2(fa, fb, lane, ia, ib, n_kept);
        const int first = smp_first(fa && ca / s1 >= (double)sp.top_p && ia + 1 >= mk, fb && cb / s1 >= (double)sp.top_p && ib + 1 >= mk);
        fa = fa && lane <= first; fb = fb && lane + 64 <= first;
    }
    // 4. min_p against the best kept probability: the first candidate below it, past min_keep, and everything behind it go
    if (sp.min_p > 0.0f) {
        const double thr = smp_at(ea, eb, head) * (double)sp.min_p;
        smp_index2(fa, fb, lane, ia, ib, n_kept);
        const int first = smp_first(fa && ea < thr && ia >= mk, fb && eb < thr && ib >= mk);
        fa = fa && lane < first; fb = fb && lane + 64 < first;
    }
    // 5. temperature and 6. the final softmax
    const double l_head = (double)((head & 64) ? __shfl(lb, head & 63, 64) : __shfl(la, head & 63, 64)), inv_t = 1.0 / (double)sp.temp;
    const double wa = fa ? exp(((double)la - l_head) * inv_t) : 0.0, wb = fb ? exp(((double)lb - l_head) * inv_t) : 0.0;
    double ca = wa, cb = wb;
    const double total = smp_scan2(ca, cb, lane);
    smp_index2(fa, fb, lane, ia, ib, n_kept);
    // the draw: the first kept candidate whose inclusive prefix sum exceeds u * total; the last kept one if rounding leaves none
    const double u = u_in ? u_in[row] : (double)philox_u(sp.seed, sp.counter, sp.stream);
    const double target = u * total;
    int pick = smp_first(fa && ca > target, fb && cb > target);
    if (pick == 128) {
        const unsigned long long ma = __ballot(fa), mb = __ballot(fb);
        pick = mb ? 127 - __clzll((long long)mb) : 63 - __clzll((long long)ma);
    }
    if (kt) {
        if (fa) { kt[ia] = ta; kp[ia] = (float)(wa / total); }
        if (fb) { kt[ib] = tb; kp[ib] = (float)(wb / total); }
    }
    if (lane == (pick & 63)) {
        tokens_out[row] = (pick & 64) ? tb : ta;
        probs_out[row] = (float)(((pick & 64) ? wb : wa) / total);
        if (n_kept_out) n_kept_out[row] = n_kept;
    }
}

// ---------------------------------------------------------------- launchers
const char *sample_rows_refusal(int R, int k, const SampleParams *p) {
    if (R < 1) return "R";
    if (k < 1 || k > TOPK_MAX_K) return "k";
    auto unit = [](float v) { return v >= 0.0f && v <= 1.0f; };                  // (false for NaN)
    for (int r = 0; p && r < R; r++) {
        if (!unit(p[r].top_p)) return "top_p";
        if (!unit(p[r].min_p)) return "min_p";
        if (!unit(p[r].typ_p)) return "typ_p";
        if (p[r].min_keep < 0) return "min_keep";
    }
    return nullptr;
}

hipError_t launch_sample_rows(const unsigned long long *keys, int R, int k, const SampleParams *params_host, const SampleParams *params_dev, const double *u_dev,
                              int32_t *tokens_out, float *probs_out, int32_t *n_kept_out, int32_t *kept_tok, float *kept_p, hipStream_t st) {
    if (!keys || !params_host || !params_dev || !tokens_out || !probs_out || (kept_tok == nullptr) != (kept_p == nullptr)) return hipErrorInvalidValue;
    if (sample_rows_refusal(R, k, params_host)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_rows_kernel, dim3((unsigned)((R + SAMPLE_WAVES - 1) / SAMPLE_WAVES)), dim3(64 * SAMPLE_WAVES), 0, st, keys, R, k, params_dev, u_dev,
                       tokens_out, probs_out, n_kept_out, kept_tok, kept_p);
    return hipGetLastError();
}

hipError_t launch_philox_u(unsigned long long seed, unsigned long long counter0, unsigned stream, int n, float *out, hipStream_t st) {
    if (n < 1 || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(philox_u_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, seed, counter0, stream, n, out);
    return hipGetLastError();
}

}  // namespace mi355
