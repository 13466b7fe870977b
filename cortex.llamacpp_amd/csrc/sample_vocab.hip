// sample_vocab.hip — the sampler chain and the draw over a WHOLE vocabulary row: top_k off or above the front's 128 candidates, and mirostat 2.
// Nothing is sorted and the row never leaves the device.  Every cut of these chains keeps a prefix of one order - higher adjusted logit first, lower token id
// among equal logits - and the draw is a selection by mass in that order, so the kernel is a radix SELECTION: it finds the prefix boundary by count or by mass.
//   work split: one workgroup of 1024 threads (16 waves) per row, grid = R.  The row (<= 1 MiB) is read from L2 once per pass, four logits per lane
//               (n % 4 == 0; else one), 4096 per round of the workgroup; a pass is "every element -> one LDS histogram bin" or "every element -> a fold".
//   the order:  o = (~image(logit) << 18) | token, 50 bits, ascending = best first (image: the front's order-preserving u32 of the f32, -0.0 read as +0.0).
//               A prefix of the order is "o <= boundary": one compare per element.
//   levels:     six, 1024 bins each (one bin per thread for the scan).  Level 0 buckets by distance from the best logit, floor((best - l) * 16) capped at
//               1023 - monotone in the order and spread over real logits, where the image's top bits (sign, exponent) would put a whole row into a few bins.
//               Levels 1..5 are the five 10-bit digits of o among the elements of the chosen bucket.  After level 5 the element is known: logit and token.
//   masses:     44-bit fixed point, q = rint(exp((l - best) / T) * 2^44) from an f64 exp, added into u64 LDS bins with integer atomics: the sum does not
//               depend on the order of the adds, so every call gives the same bits.  2^18 elements of at most 2^44 stay below 2^62.  A bin's count rides along.
//   selection:  an inclusive scan over the 1024 bins (shift-up in the wave, 16 wave totals through LDS); the one thread whose bin crosses the target (a rank, or
//               an integer mass T: "running mass >= top_p * total" is T = ceil, "> u * total" is T = floor + 1) names the bin; the next level looks inside it.
//   adjustments: at most 192 (token, bias, count) entries, the front's arithmetic, computed once into LDS.  A 32 KiB LDS bitmap marks their tokens: the
//               row's pass skips a marked token and thread j < adj_n offers entry j's value instead - the context's logits row is never written.
#include "kernels.h"
#include "philox.h"

namespace mi355 {

constexpr int SV_THREADS = 1024, SV_BINS = 1024, SV_WAVES = SV_THREADS / 64, SV_LEVELS = 6, SV_TOK_BITS = 18;
constexpr double SV_ONE = 17592186044416.0;                                       // 2^44
static_assert(SAMPLE_VOCAB_MAX_N == 1 << SV_TOK_BITS, "the order keeps 18 bits for the token");
typedef unsigned long long sv_u64;

struct SvShared {
    unsigned bitmap[SAMPLE_VOCAB_MAX_N / 32];                                     // adjusted tokens
    unsigned cnt[SV_BINS];
    sv_u64 mass[SV_BINS];
    int a_tok[TOPK_MAX_ADJ];                                                      // -1: not offered (out of the row, or a later entry of a token already listed)
    float a_val[TOPK_MAX_ADJ];
    unsigned w_cnt[SV_WAVES];
    sv_u64 w_a[SV_WAVES], w_b[SV_WAVES];
    int sel_bin;
    unsigned sel_cnt;
    sv_u64 sel_mass;
};
struct SvRow { const float *x; int n, n_adj; float best; };

__device__ __forceinline__ sv_u64 sv_order(float l, int tok) {
    unsigned b = __float_as_uint(l == 0.0f ? 0.0f : l);
    b ^= (b >> 31) ? 0xffffffffu : 0x80000000u;
    return ((sv_u64)(~b) << SV_TOK_BITS) | (unsigned)tok;
}
__device__ __forceinline__ float sv_logit_of(sv_u64 o) {
    unsigned b = ~(unsigned)(o >> SV_TOK_BITS);
    b ^= (b >> 31) ? 0x80000000u : 0xffffffffu;
    return __uint_as_float(b);
}
__device__ __forceinline__ int sv_bucket(float best, float l) { return (int)fminf((best - l) * 16.0f, (float)(SV_BINS - 1)); }
__device__ __forceinline__ sv_u64 sv_weight(float best, float l, double inv_t) { return (sv_u64)rint(exp(((double)l - (double)best) * inv_t) * SV_ONE); }

// f(token, adjusted logit) once for every token of the row, in no particular order
template <class F> __device__ __forceinline__ void sv_each(const SvShared &s, const SvRow &r, F f) {
    const int tid = threadIdx.x;
    if ((r.n & 3) == 0) {                                                         // (every row starts on 16 bytes then)
        for (int i = tid * 4; i < r.n; i += SV_THREADS * 4) {
            const float4 v = *reinterpret_cast<const float4 *>(r.x + i);
            const unsigned m = r.n_adj ? (s.bitmap[i >> 5] >> (i & 31)) & 15u : 0u;
            if (!(m & 1u)) f(i, v.x);
            if (!(m & 2u)) f(i + 1, v.y);
            if (!(m & 4u)) f(i + 2, v.z);
            if (!(m & 8u)) f(i + 3, v.w);
        }
    } else {
        for (int i = tid; i < r.n; i += SV_THREADS)
            if (!(r.n_adj && ((s.bitmap[i >> 5] >> (i & 31)) & 1u))) f(i, r.x[i]);
    }
    if (tid < r.n_adj && s.a_tok[tid] >= 0) f(s.a_tok[tid], s.a_val[tid]);
}

// (sum of cnt, max of a, sum of b) over the workgroup, on every thread
__device__ __forceinline__ void sv_reduce(SvShared &s, unsigned &cnt, sv_u64 &a, sv_u64 &b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        const sv_u64 oa = __shfl_xor(a, o, 64);
        a = oa > a ? oa : a;
        b += __shfl_xor(b, o, 64);
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { s.w_cnt[w] = cnt; s.w_a[w] = a; s.w_b[w] = b; }
    __syncthreads();
    cnt = 0; a = 0; b = 0;
#pragma unroll
    for (int i = 0; i < SV_WAVES; i++) { cnt += s.w_cnt[i]; a = s.w_a[i] > a ? s.w_a[i] : a; b += s.w_b[i]; }
}

struct SvPick { sv_u64 o; unsigned rank; sv_u64 total; bool found; };            // the element, how many precede it, the prefix's whole mass (2^-44 units)

// Among the elements with o <= bound: by_mass ? the first whose inclusive running mass (weights exp((l - best) * inv_t)) reaches T, T = gt ? floor(frac *
// total) + 1 : ceil(frac * total), at least 1 : the one at rank `want`.  found = false: no element does (rounding, or want past the end).  Uniform.
__device__ SvPick sv_select(SvShared &s, const SvRow &r, sv_u64 bound, bool by_mass, double inv_t, double frac, bool gt, unsigned want) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned cnt_before = 0;
    sv_u64 mass_before = 0, target = 0, prefix = 0;
    int b0 = -1;
    SvPick out{0, 0, 0, false};
    for (int lev = 0; lev < SV_LEVELS; lev++) {
        s.cnt[tid] = 0; s.mass[tid] = 0;
        if (tid == 0) s.sel_bin = -1;
        __syncthreads();
        const int shift = 50 - 10 * lev;                                          // (levels 1..5: digits at 40, 30, 20, 10, 0)
        sv_each(s, r, [&](int tok, float l) {
            const sv_u64 o = sv_order(l, tok);
            if (o > bound) return;
            int bin = sv_bucket(r.best, l);
            if (lev > 0) {
                if (bin != b0 || (lev > 1 && (o >> (shift + 10)) != prefix)) return;
                bin = (int)(o >> shift) & (SV_BINS - 1);
            }
            atomicAdd(&s.cnt[bin], 1u);
            if (by_mass) atomicAdd(&s.mass[bin], sv_weight(r.best, l, inv_t));
        });
        __syncthreads();
        const unsigned own_c = s.cnt[tid];
        const sv_u64 own_m = s.mass[tid];
        unsigned ic = own_c;
        sv_u64 im = own_m;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned tc = __shfl_up(ic, o, 64);
            const sv_u64 tm = __shfl_up(im, o, 64);
            if (lane >= o) { ic += tc; im += tm; }
        }
        if (lane == 63) { s.w_cnt[w] = ic; s.w_a[w] = im; }
        __syncthreads();
        sv_u64 all_m = 0;
#pragma unroll
        for (int i = 0; i < SV_WAVES; i++) {
            if (i < w) { ic += s.w_cnt[i]; im += s.w_a[i]; }
            all_m += s.w_a[i];
        }
        if (lev == 0) {
            out.total = all_m;
            if (by_mass) {
                const double x = frac * (double)all_m;
                target = gt ? (sv_u64)floor(x) + 1ull : (sv_u64)ceil(x);
                if (target < 1ull) target = 1ull;
            }
        }
        const bool hit = by_mass ? (mass_before + im >= target && mass_before + im - own_m < target)
                                 : (cnt_before + ic > want && cnt_before + ic - own_c <= want);
        if (hit) { s.sel_bin = tid; s.sel_cnt = cnt_before + ic - own_c; s.sel_mass = mass_before + im - own_m; }
        __syncthreads();
        const int b = s.sel_bin;
        if (b < 0) return out;
        cnt_before = s.sel_cnt; mass_before = s.sel_mass;
        if (lev == 0) b0 = b; else prefix = (prefix << 10) | (sv_u64)b;
        __syncthreads();
    }
    out.o = prefix; out.rank = cnt_before; out.found = true;
    return out;
}

__global__ __launch_bounds__(SV_THREADS) void sample_vocab_kernel(const float *base, int n, const int *rows, const TopkAdj *adjs, const SampleParams *params,
                                                                  const float *mu_in, const double *u_in, int32_t *tokens_out, float *probs_out, int32_t *n_kept_out) {
    __shared__ SvShared s;
    const int tid = threadIdx.x, row = blockIdx.x;
    const SampleParams sp = params[row];
    const TopkAdj &adj = adjs[row];
    SvRow r{base + (size_t)(rows ? rows[row] : row) * n, n, adj.n, 0.0f};
    // the adjusted tokens: entry j's value is the front's loop over every entry of its token, in order; the first entry of a token offers it
    if (r.n_adj) {
        for (int i = tid; i < (n + 31) / 32; i += SV_THREADS) s.bitmap[i] = 0u;
        __syncthreads();
        if (tid < r.n_adj) {
            const int tok = adj.tok[tid];
            bool first = tok >= 0 && tok < n;
            for (int a = 0; a < tid && first; a++) first = adj.tok[a] != tok;
            s.a_tok[tid] = first ? tok : -1;
            if (first) {
                float l = r.x[tok];
                for (int a = tid; a < r.n_adj; a++) {
                    if (adj.tok[a] != tok) continue;
                    l = l + adj.bias[a];
                    if (adj.cnt[a] > 0) {
                        if (l <= 0.0f) l *= adj.repeat; else l /= adj.repeat;
                        l -= (float)adj.cnt[a] * adj.freq + adj.present;
                    }
                }
                s.a_val[tid] = l;
                atomicOr(&s.bitmap[tok >> 5], 1u << (tok & 31));
            }
        }
        __syncthreads();
    }
    // the best candidate: the smallest o
    unsigned c0 = 0;
    sv_u64 top = 0, z0 = 0;
    sv_each(s, r, [&](int tok, float l) { const sv_u64 v = ~sv_order(l, tok); top = v > top ? v : top; });
    sv_reduce(s, c0, top, z0);
    const sv_u64 o_best = ~top & ((1ull << 50) - 1ull);
    r.best = sv_logit_of(o_best);
    auto leave = [&](int tok, float p, int kept) {
        if (tid == 0) { tokens_out[row] = tok; probs_out[row] = p; if (n_kept_out) n_kept_out[row] = kept; }
    };
    if (!(r.best > -INFINITY && r.best < INFINITY)) { leave(-1, 0.0f, 0); return; }
    if (sp.temp <= 0.0f) { leave((int)(o_best & ((1u << SV_TOK_BITS) - 1u)), 1.0f, 1); return; }
    const double inv_t = 1.0 / (double)sp.temp;
    const unsigned mk = sp.min_keep > 1 ? (unsigned)sp.min_keep : 1u;
    sv_u64 bound = ~0ull;                                                         // the kept prefix: o <= bound, len elements
    unsigned len = (unsigned)n;
    // (count, last of them in the order) of the kept elements that pass `keep`, then the prefix cut to max(count, floor) of them
    auto cut_where = [&](auto keep, unsigned floor_len) {
        unsigned c = 0;
        sv_u64 last = 0, z = 0;
        sv_each(s, r, [&](int tok, float l) {
            const sv_u64 o = sv_order(l, tok);
            if (o <= bound && keep(l)) { c++; last = o > last ? o : last; }
        });
        sv_reduce(s, c, last, z);
        const unsigned want = c > floor_len ? c : floor_len;
        if (want >= len) return;
        if (want == c) bound = last;
        else bound = sv_select(s, r, bound, false, 1.0, 0.0, false, want - 1u).o;
        len = want;
    };
    const bool miro = mu_in && mu_in[row] == mu_in[row] && fabsf(mu_in[row]) < INFINITY;
    if (miro) {
        // mirostat 2: temperature and softmax over the whole row, then the prefix whose surprise -log2 p does not exceed mu (p floored at 1e-37)
        unsigned c = 0;
        sv_u64 z = 0, sum = 0;
        sv_each(s, r, [&](int, float l) { sum += sv_weight(r.best, l, inv_t); });
        sv_reduce(s, c, z, sum);
        const double log2_s = log2((double)sum / SV_ONE), cap = -log2((double)1e-37f), mu = (double)mu_in[row];
        cut_where([&](float l) { return fmin(log2_s - ((double)l - (double)r.best) * inv_t * 1.4426950408889634, cap) <= mu; }, 1u);
    } else {
        // 1. top_k
        if (sp.top_k > 0) {
            const unsigned want = (unsigned)sp.top_k > mk ? (unsigned)sp.top_k : mk;
            if (want < len) { bound = sv_select(s, r, bound, false, 1.0, 0.0, false, want - 1u).o; len = want; }
        }
        // 2. top_p over the survivors: the first whose running mass reaches it is the last kept
        if (sp.top_p < 1.0f) {
            SvPick p = sv_select(s, r, bound, true, 1.0, (double)sp.top_p, false, 0u);
            const unsigned need = (mk < len ? mk : len) - 1u;
            if (p.found && p.rank < need) p = sv_select(s, r, bound, false, 1.0, 0.0, false, need);
            if (p.found) { bound = p.o; len = p.rank + 1u; }
        }
        // 3. min_p against the best kept probability (the best of the row: it is always kept)
        if (sp.min_p > 0.0f) {
            const double lim = log((double)sp.min_p);
            cut_where([&](float l) { return (double)l - (double)r.best >= lim; }, mk);
        }
    }
    // temperature, softmax and the draw: the first kept candidate whose inclusive prefix mass exceeds u * total; the last kept one if rounding leaves none
    const double u = u_in ? u_in[row] : (double)philox_u(sp.seed, sp.counter, sp.stream);
    SvPick p = sv_select(s, r, bound, true, inv_t, u, true, 0u);
    const sv_u64 total = p.total;
    if (!p.found) p = sv_select(s, r, bound, false, 1.0, 0.0, false, len - 1u);
    const double wt = exp(((double)sv_logit_of(p.o) - (double)r.best) * inv_t);
    leave((int)(p.o & ((1u << SV_TOK_BITS) - 1u)), (float)(wt / ((double)total / SV_ONE)), (int)len);
}

// ---------------------------------------------------------------- launcher
const char *sample_vocab_refusal(int R, int n, const SampleParams *p) {
    if (R < 1) return "R";
    if (n < 1 || n > SAMPLE_VOCAB_MAX_N) return "n";
    auto unit = [](float v) { return v >= 0.0f && v <= 1.0f; };                  // (false for NaN)
    for (int r = 0; p && r < R; r++) {
        if (!unit(p[r].top_p)) return "top_p";
        if (!unit(p[r].min_p)) return "min_p";
        if (!(p[r].typ_p == 1.0f)) return "typ_p";
        if (p[r].min_keep < 0) return "min_keep";
    }
    return nullptr;
}

hipError_t launch_sample_vocab(const float *base, int n, int R, const int *rows_dev, const TopkAdj *adjs_dev, const SampleParams *params_host,
                               const SampleParams *params_dev, const float *mu_dev, const double *u_dev, int32_t *tokens_out, float *probs_out, int32_t *n_kept_out,
                               hipStream_t st) {
    if (!base || !adjs_dev || !params_host || !params_dev || !tokens_out || !probs_out) return hipErrorInvalidValue;
    if (sample_vocab_refusal(R, n, params_host)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_vocab_kernel, dim3((unsigned)R), dim3(SV_THREADS), 0, st, base, n, rows_dev, adjs_dev, params_dev, mu_dev, u_dev, tokens_out, probs_out,
                       n_kept_out);
    return hipGetLastError();
}

}  // namespace mi355
