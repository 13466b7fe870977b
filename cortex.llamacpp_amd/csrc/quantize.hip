// quantize.hip — the quantiser (what upstream's ggml_quantize_chunk does for the types of the published mixes): f32 / f16 / bf16 rows ->
// ggml-layout blocks of Q8_0, Q5_0, Q5_1, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, with or without an importance matrix.  The arithmetic is tests/quantize_ref.py's, step
// for step: that file is the specification, this one follows it (same products, same summation trees, IEEE division and square root, no contraction).
//
// Shape of the work.  The rows are one flat run of elements (a row is a whole number of blocks).  A wave owns 256 adjacent elements: one super-block of a K
// type, eight blocks of a 32-element type.  Lane l holds elements 4 l .. 4 l + 3 (one 16-byte load of f32; of f16 / bf16 the 16 bytes it shares with its
// neighbour), so a 32-element sub-block is the 8 lanes 8 g .. 8 g + 7 and a 16-element one the 4 lanes 4 g .. 4 g + 3.  A sum over a sub-block is the lane's
// four terms left to right, then a butterfly over the group (l ^ 1, l ^ 2, l ^ 4: DPP); every lane of the group ends with the same bits, so the search's
// choices are uniform inside a group and need no vote.  The super-block step (the maxima of the scales, their quantisation, the recomputed codes) continues
// the butterfly over the wave.  The codes then meet in LDS, where lanes assemble the block's bytes, and leave as 16-bit stores.
// No atomics; a non-finite source value is computed as 0 and raises *nonfinite_flag (every writer stores the same 1).
#include "dev_common.h"
#include "kernels.h"

namespace mi355 {

namespace {
constexpr float Q_GROUP_MAX_EPS = 1e-15f;
constexpr int QZ_WAVES = 4;              // waves (256-element chunks) of a workgroup
constexpr int QZ_OUT_MAX = 272;          // bytes a chunk leaves: eight Q8_0 blocks

// ---- group reductions: G = 4 or 8 adjacent lanes (aligned), 64 = the wave
template <int G> __device__ __forceinline__ float gsum(float v) {
    v += dpp_f<DPP_QP_1032>(v);
    v += dpp_f<DPP_QP_2301>(v);
    if (G >= 8) v += dpp_f<DPP_HALF_MIRROR>(v);          // (groups of four are uniform by now: i <-> 7 - i adds the two of them, as l ^ 4 would)
    if (G >= 64) {
        v += dpp_f<DPP_MIRROR>(v);
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
    }
    return v;
}
template <int G> __device__ __forceinline__ float gmax(float v) {
    v = fmaxf(v, dpp_f<DPP_QP_1032>(v));
    v = fmaxf(v, dpp_f<DPP_QP_2301>(v));
    if (G >= 8) v = fmaxf(v, dpp_f<DPP_HALF_MIRROR>(v));
    if (G >= 64) {
        v = fmaxf(v, dpp_f<DPP_MIRROR>(v));
        v = fmaxf(v, __shfl_xor(v, 16));
        v = fmaxf(v, __shfl_xor(v, 32));
    }
    return v;
}
template <int G> __device__ __forceinline__ float gmin(float v) { return -gmax<G>(-v); }
template <int G> __device__ __forceinline__ float lsum(float a, float b, float c, float d) { return gsum<G>(((a + b) + c) + d); }
template <int G> __device__ __forceinline__ float lmax(const float x[4]) { return gmax<G>(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]))); }
template <int G> __device__ __forceinline__ float lmin(const float x[4]) { return gmin<G>(fminf(fminf(x[0], x[1]), fminf(x[2], x[3]))); }
// the element of largest magnitude with its sign; +a where +a and -a tie
template <int G> __device__ __forceinline__ float lextreme(const float x[4]) {
    const float mx = lmax<G>(x), mn = lmin<G>(x);
    return -mn > mx ? mn : mx;
}
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// ---- the lane's four source elements (first element e0, a multiple of 4)
template <int ST> __device__ __forceinline__ void load4(const void *src, size_t e0, float x[4]) {
    if (ST == T_F32) {
        const float4 v = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(src) + e0);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
        const uint4 v = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint16_t *>(src) + (e0 & ~(size_t)7));
        const uint32_t a = (e0 & 4) ? v.z : v.x, b = (e0 & 4) ? v.w : v.y;
        if (ST == T_F16) {
            x[0] = h2f((uint16_t)(a & 0xffffu)); x[1] = h2f((uint16_t)(a >> 16)); x[2] = h2f((uint16_t)(b & 0xffffu)); x[3] = h2f((uint16_t)(b >> 16));
        } else {
            x[0] = __uint_as_float(a << 16); x[1] = __uint_as_float(a & 0xffff0000u); x[2] = __uint_as_float(b << 16); x[3] = __uint_as_float(b & 0xffff0000u);
        }
    }
}

// ---- make_qkx2_quants over a group of G lanes: codes L in [0, nmax], scale, the_min >= 0
template <int G, bool MAD> __device__ __forceinline__ float qkx_err(const float x[4], const float w[4], float sc, float m, const float L[4]) {
    float t[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float d = (sc * L[i] + m) - x[i];
        t[i] = w[i] * (MAD ? fabsf(d) : d * d);
    }
    return lsum<G>(t[0], t[1], t[2], t[3]);
}

template <int G, bool MAD>
__device__ __forceinline__ void qkx_search(const float x[4], const float w[4], float nmax, float rmin, float rdelta, int nstep, float L[4], float &scale_out,
                                           float &min_out) {
    const float mn = fminf(lmin<G>(x), 0.0f) + 0.0f, mx = lmax<G>(x);
    const float sum_w = lsum<G>(w[0], w[1], w[2], w[3]), sum_x = lsum<G>(w[0] * x[0], w[1] * x[1], w[2] * x[2], w[3] * x[3]);
    const bool flat = mx == mn;
    const float rng = flat ? 1.0f : mx - mn;
    const float iscale = nmax / rng;
    float scale = 1.0f / iscale, m_out = mn;
#pragma unroll
    for (int i = 0; i < 4; i++) L[i] = clampf(rintf(iscale * (x[i] - mn)), 0.0f, nmax);
    float best = qkx_err<G, MAD>(x, w, scale, mn, L);
    for (int s = 0; s <= nstep; s++) {
        const float isc = ((rmin + rdelta * (float)s) + nmax) / rng;
        float l[4], wl[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { l[i] = clampf(rintf(isc * (x[i] - mn)), 0.0f, nmax); wl[i] = w[i] * l[i]; }
        const float sum_l = lsum<G>(wl[0], wl[1], wl[2], wl[3]);
        const float sum_l2 = lsum<G>(wl[0] * l[0], wl[1] * l[1], wl[2] * l[2], wl[3] * l[3]);
        const float sum_xl = lsum<G>(wl[0] * x[0], wl[1] * x[1], wl[2] * x[2], wl[3] * x[3]);
        const float D = sum_w * sum_l2 - sum_l * sum_l;
        float t_scale = (sum_w * sum_xl - sum_x * sum_l) / D;
        float t_min = (sum_l2 * sum_x - sum_l * sum_xl) / D;
        if (t_min > 0.0f) { t_min = 0.0f; t_scale = sum_xl / sum_l2; }
        const float mad = qkx_err<G, MAD>(x, w, t_scale, t_min, l);
        if (D > 0.0f && mad < best && !flat) {
            best = mad; scale = t_scale; m_out = t_min;
#pragma unroll
            for (int i = 0; i < 4; i++) L[i] = l[i];
        }
    }
    if (flat) {
        scale = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; i++) L[i] = 0.0f;
    }
    scale_out = scale;
    min_out = 0.0f - m_out;
}

// ---- make_qx_quants with weights w over a group of G lanes: codes l in [-nmax, nmax - 1], scale.  REFINE (G = 4): make_q3_quants' sweeps on top
template <int G> __device__ __forceinline__ void sym_sums(const float x[4], const float w[4], const float wx[4], float isc, float nmax, float l[4], float &slx,
                                                          float &sl2) {
#pragma unroll
    for (int i = 0; i < 4; i++) l[i] = clampf(rintf(isc * x[i]), -nmax, nmax - 1.0f);
    slx = lsum<G>(wx[0] * l[0], wx[1] * l[1], wx[2] * l[2], wx[3] * l[3]);
    sl2 = lsum<G>((w[0] * l[0]) * l[0], (w[1] * l[1]) * l[1], (w[2] * l[2]) * l[2], (w[3] * l[3]) * l[3]);
}

template <int G, bool REFINE>
__device__ __forceinline__ void sym_search(const float x[4], const float w[4], float nmax, float L[4], float &scale_out) {
    const float ext = lextreme<G>(x);
    const bool tiny = fabsf(ext) < Q_GROUP_MAX_EPS;
    const float mxs = tiny ? 1.0f : ext;
    float wx[4];
#pragma unroll
    for (int i = 0; i < 4; i++) wx[i] = w[i] * x[i];
    float sumlx, suml2;
    sym_sums<G>(x, w, wx, -nmax / mxs, nmax, L, sumlx, suml2);
    float scale = suml2 != 0.0f ? sumlx / suml2 : 0.0f;
    float best = scale * sumlx;
    for (int s = -9; s <= 9; s++) {
        if (s == 0) continue;
        float l[4], slx, sl2;
        sym_sums<G>(x, w, wx, -(nmax + 0.1f * (float)s) / mxs, nmax, l, slx, sl2);
        if (sl2 > 0.0f && slx * slx > best * sl2) {
            scale = slx / sl2; best = scale * slx; sumlx = slx; suml2 = sl2;
#pragma unroll
            for (int i = 0; i < 4; i++) L[i] = l[i];
        }
    }
    if (REFINE) {
        // every lane of the group takes the whole sub-block and runs the sweeps on its own copy: the same bits in all four, no exchange inside the loop
        static_assert(!REFINE || G == 4, "the sweeps hold 16 elements per lane");
        float xs[16], ws[16], Ls[16];
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int j = 0; j < 4; j++) { xs[4 * k + j] = __shfl(x[j], k, 4); ws[4 * k + j] = __shfl(w[j], k, 4); Ls[4 * k + j] = __shfl(L[j], k, 4); }
        for (int itry = 0; itry < 5; itry++) {
            bool changed = false;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const float wxi = ws[i] * xs[i];
                const float slx = sumlx - wxi * Ls[i];
                const float sl2 = suml2 - (ws[i] * Ls[i]) * Ls[i];
                const float nl = clampf(rintf((xs[i] * sl2) / slx), -nmax, nmax - 1.0f);
                const float slx2 = slx + wxi * nl;
                const float sl22 = sl2 + (ws[i] * nl) * nl;
                if (slx > 0.0f && nl != Ls[i] && sl22 > 0.0f && (slx2 * slx2) * suml2 > (sumlx * sumlx) * sl22) {
                    Ls[i] = nl; sumlx = slx2; suml2 = sl22; changed = true;
                }
            }
            if (!changed) break;
        }
        scale = suml2 != 0.0f ? sumlx / suml2 : 0.0f;
        const int gl = (int)(threadIdx.x & 3);
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int j = 0; j < 4; j++) if (k == gl) L[j] = Ls[4 * k + j];
    }
    if (tiny) {
        scale = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; i++) L[i] = -nmax;
    }
    scale_out = scale;
}

// qw * sqrt(sigma2 + x^2), sigma2 = factor * (sum of x^2 over the super-block) / 256
__device__ __forceinline__ void weights_sigma(const float x[4], const float qw[4], float factor, float w[4]) {
    const float s2 = lsum<64>(x[0] * x[0], x[1] * x[1], x[2] * x[2], x[3] * x[3]);
    const float sigma2 = factor * s2 / 256.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = qw[i] * sqrtf(sigma2 + x[i] * x[i]);
}
// av_x + |x|, av_x = sqrt(sum of x^2 over the sub-block / n)
template <int G> __device__ __forceinline__ void weights_av(const float x[4], float w[4]) {
    const float av = sqrtf(lsum<G>(x[0] * x[0], x[1] * x[1], x[2] * x[2], x[3] * x[3]) / (float)(4 * G));
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = av + fabsf(x[i]);
}

__device__ __forceinline__ void put_codes(uint8_t *codes, int lane, const float L[4], float bias) {
    const uint32_t c0 = (uint32_t)(int)(L[0] + bias), c1 = (uint32_t)(int)(L[1] + bias), c2 = (uint32_t)(int)(L[2] + bias), c3 = (uint32_t)(int)(L[3] + bias);
    reinterpret_cast<uint32_t *>(codes)[lane] = (c0 & 255u) | (c1 & 255u) << 8 | (c2 & 255u) << 16 | c3 << 24;
}
__device__ __forceinline__ void put_u16(uint8_t *out, int at, uint16_t v) { *reinterpret_cast<uint16_t *>(out + at) = v; }
// 2-bit codes: byte 32 h + l holds elements 128 h + l + 32 k at bits 2 k (Q2_K's and Q3_K's qs)
__device__ __forceinline__ uint8_t pack2(const uint8_t *codes, int b) {
    const uint8_t *c = codes + 128 * (b >> 5) + (b & 31);
    return (uint8_t)((c[0] & 3) | (c[32] & 3) << 2 | (c[64] & 3) << 4 | (c[96] & 3) << 6);
}

template <int DT, int ST>
__global__ __launch_bounds__(QZ_WAVES * 64) void quantize_kernel(const void *__restrict__ src, const float *__restrict__ imatrix, int64_t n_per_row,
                                                                 int64_t n_total, uint8_t *__restrict__ dst, int32_t *__restrict__ nonfinite_flag) {
    __shared__ __attribute__((aligned(16))) uint8_t s_codes[QZ_WAVES][256];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[QZ_WAVES][QZ_OUT_MAX];
    __shared__ __attribute__((aligned(16))) uint8_t s_sub[QZ_WAVES][32];
    constexpr int BB = ggml_block_bytes(DT), BE = ggml_block_elems(DT);
    constexpr int CHUNK_BYTES = 256 / BE * BB;
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const int64_t chunk = (int64_t)blockIdx.x * QZ_WAVES + wv;
    const int64_t e0 = chunk * 256 + 4 * lane;
    const bool have = e0 < n_total;            // (a block of 32 is inside or outside as a whole, and so is the 16-byte load of two lanes)
    uint8_t *codes = s_codes[wv], *out = s_out[wv], *sub = s_sub[wv];

    float x[4] = {0.0f, 0.0f, 0.0f, 0.0f}, qw[4] = {1.0f, 1.0f, 1.0f, 1.0f};
    if (have) {
        load4<ST>(src, (size_t)e0, x);
        if (imatrix) load4<T_F32>(imatrix, (size_t)(e0 % n_per_row), qw);
        bool bad = false;
#pragma unroll
        for (int i = 0; i < 4; i++) if (!(fabsf(x[i]) <= 3.4028234664e38f)) { bad = true; x[i] = 0.0f; }
        if (bad) *nonfinite_flag = 1;
    }
    const bool imx = imatrix != nullptr;

    if (DT == T_Q8_0) {
        const float d = gmax<8>(fmaxf(fmaxf(fabsf(x[0]), fabsf(x[1])), fmaxf(fabsf(x[2]), fabsf(x[3])))) / 127.0f;
        const float id = d != 0.0f ? 1.0f / d : 0.0f;
        uint8_t *b = out + 34 * (lane >> 3);
        if ((lane & 7) == 0) put_u16(b, 0, f2h(d));
#pragma unroll
        for (int i = 0; i < 4; i++) b[2 + 4 * (lane & 7) + i] = (uint8_t)(int8_t)(int)roundf(x[i] * id);
        __syncthreads();
    } else if (DT == T_Q5_0 || DT == T_Q5_1) {
        float L[4], d, mn = 0.0f;
        if (DT == T_Q5_0) {
            d = lextreme<8>(x) / -16.0f + 0.0f;
            const float id = d != 0.0f ? 1.0f / d : 0.0f;
#pragma unroll
            for (int i = 0; i < 4; i++) L[i] = fminf(31.0f, truncf(x[i] * id + 16.5f));
        } else {
            mn = lmin<8>(x) + 0.0f;
            d = (lmax<8>(x) - mn) / 31.0f + 0.0f;
            const float id = d != 0.0f ? 1.0f / d : 0.0f;
#pragma unroll
            for (int i = 0; i < 4; i++) L[i] = fminf(31.0f, truncf((x[i] - mn) * id + 0.5f));
        }
        put_codes(codes, lane, L, 0.0f);
        uint32_t hb = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) hb |= (((uint32_t)(int)L[i] >> 4) & 1u) << (4 * (lane & 7) + i);
        hb |= (uint32_t)__shfl_xor((int)hb, 1); hb |= (uint32_t)__shfl_xor((int)hb, 2); hb |= (uint32_t)__shfl_xor((int)hb, 4);
        constexpr int HDR = DT == T_Q5_0 ? 2 : 4;
        uint8_t *b = out + BB * (lane >> 3);
        if ((lane & 7) == 0) {
            put_u16(b, 0, f2h(d));
            if (DT == T_Q5_1) put_u16(b, 2, f2h(mn));
            put_u16(b, HDR, (uint16_t)(hb & 0xffffu)); put_u16(b, HDR + 2, (uint16_t)(hb >> 16));
        }
        __syncthreads();
        const uint8_t *c = codes + 32 * (lane >> 3);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int j = 2 * (lane & 7) + k;
            b[HDR + 4 + j] = (uint8_t)((c[j] & 15) | (c[16 + j] & 15) << 4);
        }
        __syncthreads();
    } else if (DT == T_Q4_K || DT == T_Q5_K) {
        constexpr float nmax = DT == T_Q4_K ? 15.0f : 31.0f;
        float w[4], L[4], scale, the_min;
        if (imx) {
            weights_sigma(x, qw, 2.0f, w);
            qkx_search<8, false>(x, w, nmax, -0.9f, 0.05f, 36, L, scale, the_min);
        } else {
            weights_av<8>(x, w);
            if (DT == T_Q4_K) qkx_search<8, false>(x, w, nmax, -1.0f, 0.1f, 20, L, scale, the_min);
            else qkx_search<8, false>(x, w, nmax, -0.5f, 0.1f, 15, L, scale, the_min);
        }
        const float max_scale = gmax<64>(scale), max_min = gmax<64>(the_min);
        const float inv_scale = max_scale > 0.0f ? 63.0f / max_scale : 0.0f, inv_min = max_min > 0.0f ? 63.0f / max_min : 0.0f;
        const float ls = clampf(rintf(inv_scale * scale), 0.0f, 63.0f), lm = clampf(rintf(inv_min * the_min), 0.0f, 63.0f);
        const uint16_t dh = f2h(max_scale / 63.0f), dmh = f2h(max_min / 63.0f);
        const float d = h2f(dh) * ls, dm = h2f(dmh) * lm;
        if (d != 0.0f) {
#pragma unroll
            for (int i = 0; i < 4; i++) L[i] = clampf(rintf((x[i] + dm) / d), 0.0f, nmax);
        }
        put_codes(codes, lane, L, 0.0f);
        if ((lane & 7) == 0) { sub[lane >> 3] = (uint8_t)(int)ls; sub[8 + (lane >> 3)] = (uint8_t)(int)lm; }
        __syncthreads();
        if (lane == 0) { put_u16(out, 0, dh); put_u16(out, 2, dmh); }
        if (lane < 4) {
            out[4 + lane] = (uint8_t)(sub[lane] | (sub[4 + lane] >> 4) << 6);
            out[8 + lane] = (uint8_t)(sub[8 + lane] | (sub[12 + lane] >> 4) << 6);
            out[12 + lane] = (uint8_t)((sub[4 + lane] & 15) | (sub[12 + lane] & 15) << 4);
        }
        constexpr int QS = DT == T_Q4_K ? 16 : 48;
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int b = lane + 64 * k;
            const uint8_t *c = codes + 64 * (b >> 5) + (b & 31);
            out[QS + b] = (uint8_t)((c[0] & 15) | (c[32] & 15) << 4);
        }
        if (DT == T_Q5_K && lane < 32) {
            uint32_t h = 0;
#pragma unroll
            for (int j = 0; j < 8; j++) h |= (uint32_t)(codes[32 * j + lane] >> 4) << j;
            out[16 + lane] = (uint8_t)h;
        }
        __syncthreads();
    } else if (DT == T_Q2_K) {
        float w[4], L[4], scale, the_min;
        if (imx) {
            weights_sigma(x, qw, 1.0f, w);
            qkx_search<4, false>(x, w, 3.0f, -0.9f, 0.05f, 36, L, scale, the_min);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) w[i] = fabsf(x[i]);
            qkx_search<4, true>(x, w, 3.0f, -0.5f, 0.1f, 15, L, scale, the_min);
        }
        const float max_scale = gmax<64>(scale), max_min = gmax<64>(the_min);
        const float is_ = max_scale > 0.0f ? 15.0f / max_scale : 0.0f, im_ = max_min > 0.0f ? 15.0f / max_min : 0.0f;
        const float ls = clampf(rintf(is_ * scale), 0.0f, 15.0f), lm = clampf(rintf(im_ * the_min), 0.0f, 15.0f);
        const uint16_t dh = f2h(max_scale > 0.0f ? max_scale / 15.0f : 0.0f), dmh = f2h(max_min > 0.0f ? max_min / 15.0f : 0.0f);
        const float d = h2f(dh) * ls, dm = h2f(dmh) * lm;
        if (d != 0.0f) {
#pragma unroll
            for (int i = 0; i < 4; i++) L[i] = clampf(rintf((x[i] + dm) / d), 0.0f, 3.0f);
        }
        put_codes(codes, lane, L, 0.0f);
        if ((lane & 3) == 0) out[lane >> 2] = (uint8_t)((int)ls | (int)lm << 4);
        if (lane == 0) { put_u16(out, 80, dh); put_u16(out, 82, dmh); }
        __syncthreads();
        out[16 + lane] = pack2(codes, lane);
        __syncthreads();
    } else if (DT == T_Q6_K || DT == T_Q3_K) {
        constexpr float nmax = DT == T_Q6_K ? 32.0f : 4.0f, smax = DT == T_Q6_K ? 128.0f : 32.0f;
        float w[4], L[4], scale;
        if (DT == T_Q6_K) {
#pragma unroll
            for (int i = 0; i < 4; i++) w[i] = imx ? qw[i] : x[i] * x[i];
            sym_search<4, false>(x, w, nmax, L, scale);
        } else {
            if (imx) weights_sigma(x, qw, 2.0f, w); else weights_av<4>(x, w);
            sym_search<4, true>(x, w, nmax, L, scale);
        }
        const float smx = gmax<64>(scale), smn = gmin<64>(scale);
        const float ms = -smn > smx ? smn : smx;
        const bool zero = fabsf(ms) < Q_GROUP_MAX_EPS;
        const float iscale = -smax / (zero ? 1.0f : ms);
        const uint16_t dh = f2h(1.0f / iscale);
        const float sc = clampf(rintf(iscale * scale), -smax, smax - 1.0f);
        const float d = h2f(dh) * sc;
        if (d != 0.0f) {
#pragma unroll
            for (int i = 0; i < 4; i++) L[i] = clampf(rintf(x[i] / d), -nmax, nmax - 1.0f);
        }
        put_codes(codes, lane, L, nmax);
        if (DT == T_Q6_K) {
            if ((lane & 3) == 0) out[192 + (lane >> 2)] = zero ? (uint8_t)0 : (uint8_t)(int8_t)(int)sc;
            if (lane == 0) put_u16(out, 208, zero ? (uint16_t)0 : dh);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int b = lane + 64 * k;
                const uint8_t *c = codes + 128 * (b >> 6) + 32 * ((b >> 5) & 1) + (b & 31);
                out[b] = zero ? (uint8_t)0 : (uint8_t)((c[0] & 15) | (c[64] & 15) << 4);
            }
            const uint8_t *c = codes + 128 * (lane >> 5) + (lane & 31);
            out[128 + lane] = zero ? (uint8_t)0 : (uint8_t)((c[0] >> 4) | (c[32] >> 4) << 2 | (c[64] >> 4) << 4 | (c[96] >> 4) << 6);
        } else {
            if ((lane & 3) == 0) sub[lane >> 2] = (uint8_t)((int)sc + 32);
            if (lane == 0) put_u16(out, 108, zero ? (uint16_t)0 : dh);
            __syncthreads();
            if (lane < 32) {
                uint32_t h = 0;
#pragma unroll
                for (int j = 0; j < 8; j++) h |= (uint32_t)(codes[32 * j + lane] >> 2) << j;
                out[lane] = zero ? (uint8_t)0 : (uint8_t)h;
            }
            out[32 + lane] = zero ? (uint8_t)0 : pack2(codes, lane);
            if (lane < 8) out[96 + lane] = zero ? (uint8_t)0 : (uint8_t)((sub[lane] & 15) | (sub[8 + lane] & 15) << 4);
            else if (lane < 12) {
                const int k = lane - 8;
                out[96 + lane] = zero ? (uint8_t)0 : (uint8_t)((sub[k] >> 4) | (sub[4 + k] >> 4) << 2 | (sub[8 + k] >> 4) << 4 | (sub[12 + k] >> 4) << 6);
            }
        }
        __syncthreads();
    }

    // the chunk's bytes leave: 16-bit words (a block's size is even; a Q3_K / Q6_K block is not a multiple of four)
    const int64_t left = n_total - chunk * 256;
    const int n_bytes = left >= 256 ? CHUNK_BYTES : left > 0 ? (int)(left / BE) * BB : 0;
    uint16_t *dst16 = reinterpret_cast<uint16_t *>(dst + (size_t)chunk * CHUNK_BYTES);
    const uint16_t *out16 = reinterpret_cast<const uint16_t *>(out);
    for (int k = lane; k < n_bytes / 2; k += 64) dst16[k] = out16[k];
}

template <int DT> hipError_t launch_dt(int src_type, const void *src, int64_t n_per_row, int64_t n_total, const float *imatrix, void *dst, int32_t *flag,
                                       hipStream_t st) {
    const int64_t chunks = (n_total + 255) / 256;
    const dim3 grid((unsigned)((chunks + QZ_WAVES - 1) / QZ_WAVES)), block(QZ_WAVES * 64);
    uint8_t *d = reinterpret_cast<uint8_t *>(dst);
    switch (src_type) {
        case T_F32: hipLaunchKernelGGL((quantize_kernel<DT, T_F32>), grid, block, 0, st, src, imatrix, n_per_row, n_total, d, flag); break;
        case T_F16: hipLaunchKernelGGL((quantize_kernel<DT, T_F16>), grid, block, 0, st, src, imatrix, n_per_row, n_total, d, flag); break;
        case T_BF16: hipLaunchKernelGGL((quantize_kernel<DT, T_BF16>), grid, block, 0, st, src, imatrix, n_per_row, n_total, d, flag); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
}  // namespace

bool quantize_dst_supported(int dst_type) {
    switch (dst_type) {
        case T_Q8_0: case T_Q5_0: case T_Q5_1: case T_Q2_K: case T_Q3_K: case T_Q4_K: case T_Q5_K: case T_Q6_K: return true;
        default: return false;
    }
}
bool quantize_src_supported(int src_type) { return src_type == T_F32 || src_type == T_F16 || src_type == T_BF16; }

hipError_t launch_quantize_rows(int dst_type, int src_type, const void *src, int64_t n_per_row, int64_t n_rows, const float *imatrix, void *dst,
                                int32_t *nonfinite_flag, hipStream_t st) {
    if (!quantize_dst_supported(dst_type) || !quantize_src_supported(src_type) || !src || !dst || !nonfinite_flag || n_per_row < 1 || n_rows < 1 ||
        n_per_row % ggml_block_elems(dst_type) || n_rows > ((int64_t)1 << 40) / n_per_row) return hipErrorInvalidValue;
    if (((uintptr_t)src & 15) || ((uintptr_t)imatrix & 15) || ((uintptr_t)dst & 1)) return hipErrorInvalidValue;
    const int64_t n_total = n_per_row * n_rows;
    if ((n_total + 255) / 256 > (int64_t)0x7fffffff * QZ_WAVES) return hipErrorInvalidValue;
    switch (dst_type) {
        case T_Q8_0: return launch_dt<T_Q8_0>(src_type, src, n_per_row, n_total, imatrix, dst, nonfinite_flag, st);
        case T_Q5_0: return launch_dt<T_Q5_0>(src_type, src, n_per_row, n_total, imatrix, dst, nonfinite_flag, st);
        case T_Q5_1: return launch_dt<T_Q5_1>(src_type, src, n_per_row, n_total, imatrix, dst, nonfinite_flag, st);
        case T_Q2_K: return launch_dt<T_Q2_K>(src_type, src, n_per_row, n_total, imatrix, dst, nonfinite_flag, st);
        case T_Q3_K: return launch_dt<T_Q3_K>(src_type, src, n_per_row, n_total, imatrix, dst, nonfinite_flag, st);
        case T_Q4_K: return launch_dt<T_Q4_K>(src_type, src, n_per_row, n_total, imatrix, dst, nonfinite_flag, st);
        case T_Q5_K: return launch_dt<T_Q5_K>(src_type, src, n_per_row, n_total, imatrix, dst, nonfinite_flag, st);
        default: return launch_dt<T_Q6_K>(src_type, src, n_per_row, n_total, imatrix, dst, nonfinite_flag, st);
    }
}

}  // namespace mi355
