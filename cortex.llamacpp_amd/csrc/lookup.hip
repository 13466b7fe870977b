// lookup.hip — prompt-lookup drafting (DESIGN.md §4.9 "Prompt-lookup drafting"): the producer of drafts for speculative decoding without a draft model.
//   ngram_draft:   per history h[0 .. len) the most recent, longest repeat of its tail and the up-to-k tokens that followed it;
//   lookup_append: a history grows by tokens that are already on the device (the verify launch's ids) or were uploaded (the prompt).
// The rule, integers only.  For an end position e, 1 <= e < len, m(e) = how many tokens agree walking backwards from h[e - 1] against h[len - 1], at most
// ngram_max of them, the walk ending at index 0.  The winner is the e of the largest m, the largest such e; a candidate is the 64-bit key (m << 32) | e and
// every reduction is a maximum over keys, so the answer does not depend on the order anything arrives in.  m >= ngram_min: the draft is h[e .. min(e + k, len)).
//
// The split.  Token index i = e - 1 is what a lane owns: a tile is NG_TILE adjacent indices, a lane takes NG_PER_LANE adjacent ones of it (one 16-byte LDS
// read), a part is tiles_per_part adjacent tiles, the grid is (parts, sequences).  A tile sits in LDS behind a halo of NG_HALO = 16 tokens, the longest walk,
// so a repeat that straddles a tile or a part boundary is walked whole from LDS.  The tail's 16 tokens are in LDS once per workgroup; its last token is in a
// register, and a lane compares that one first: the common miss costs one compare per index.  Parts meet through one scratch slot each and a ticket
// (spec.hip's pattern): the last workgroup to arrive reduces the slots, applies ngram_min, copies the draft out of the history and re-arms the counter.
#include "spec_dev.h"

namespace mi355 {

constexpr int NG_THREADS = 256, NG_PER_LANE = 4, NG_TILE = NG_THREADS * NG_PER_LANE, NG_HALO = 16;
constexpr int NG_PART_MIN_TILES = 2;           // a part is worth a workgroup from two tiles on: a history up to 2048 tokens is one workgroup
static_assert(NG_HALO == NG_MAX_NGRAM && NG_MAX_DRAFT == SPEC_MAX_DRAFT, "the halo holds the longest walk; a draft is a verify group");

__device__ __forceinline__ unsigned long long ng_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
// the wave's largest key, in every lane: the two halves of the key go through the cross-lane network separately
__device__ __forceinline__ unsigned long long ng_wave_max(unsigned long long key) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = __shfl_xor((unsigned)(key >> 32), o, 64), lo = __shfl_xor((unsigned)key, o, 64);
        key = ng_max(key, ((unsigned long long)hi << 32) | lo);
    }
    return key;
}

// hist [n_seq][cap], cap % 4 == 0 and the base 16-byte aligned (the launcher's check): every row starts on a 16-byte boundary.  slots [n_seq][NG_MAX_PARTS]
// keys, cnt [n_seq] tickets (zero between launches).  draft_out [n_seq][16] (-1 behind n_draft), n_draft_out [n_seq], match_out [n_seq][2] = (m, e).
__global__ __launch_bounds__(NG_THREADS) void ngram_draft_kernel(const int32_t *hist, int cap, const int32_t *len_dev, int ngram_min, int ngram_max, int k,
                                                                 int tiles_per_part, unsigned long long *slots, unsigned *cnt, int32_t *draft_out,
                                                                 int32_t *n_draft_out, int32_t *match_out) {
    __shared__ __attribute__((aligned(16))) int32_t sh[NG_HALO + NG_TILE];
    __shared__ int32_t tail[NG_HALO];
    __shared__ unsigned long long wkey[NG_THREADS / 64];
    __shared__ int last_sh;
    const int row = blockIdx.y, part = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t *h = hist + (size_t)row * cap;
    const int len = min(max(len_dev[row], 0), cap);
    const int n_idx = len - 1;                           // token indices 0 .. len - 2 end a candidate (e = i + 1 < len)
    unsigned long long best = 0;
    if ((size_t)part * tiles_per_part * NG_TILE < (size_t)max(n_idx, 0)) {
        if (tid < NG_HALO) tail[tid] = len - 1 - tid >= 0 ? h[len - 1 - tid] : 0;      // tail[j] = h[len - 1 - j]
        const int lim = (n_idx + 3) & ~3;                // the 16-byte loads stop at the first one that holds no candidate (<= cap: cap % 4 == 0)
        for (int t = 0; t < tiles_per_part; t++) {
            const int t0 = (part * tiles_per_part + t) * NG_TILE;
            if (t0 >= n_idx) break;
            __syncthreads();                             // the previous tile has been read (the first pass: nothing to wait for but the tail's stores)
            for (int q = tid; q < (NG_HALO + NG_TILE) / 4; q += NG_THREADS) {
                const int v = t0 - NG_HALO + 4 * q;
                int4 w = make_int4(0, 0, 0, 0);          // in front of index 0 and behind the candidates: never compared (the walk's bounds), defined anyway
                if (v >= 0 && v < lim) w = *reinterpret_cast<const int4 *>(h + v);
                *reinterpret_cast<int4 *>(sh + 4 * q) = w;
            }
            __syncthreads();
            const int last = tail[0];
            const int i0 = t0 + NG_PER_LANE * tid;
            const int4 w = *reinterpret_cast<const int4 *>(sh + NG_HALO + NG_PER_LANE * tid);
            const int own[NG_PER_LANE] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < NG_PER_LANE; j++) {
                const int i = i0 + j;
                if (i >= n_idx || own[j] != last) continue;
                const int32_t *p = sh + NG_HALO + (i - t0);                       // p[-m] = h[i - m], m <= 15: inside the halo
                int m = 1;
                while (m < ngram_max && i - m >= 0 && p[-m] == tail[m]) m++;
                best = ng_max(best, ((unsigned long long)m << 32) | (unsigned)(i + 1));
            }
        }
    }
    best = ng_wave_max(best);
    if (lane == 0) wkey[wave] = best;
    __syncthreads();
    if (tid == 0) {
        best = ng_max(ng_max(wkey[0], wkey[1]), ng_max(wkey[2], wkey[3]));
        __hip_atomic_store(slots + (size_t)row * NG_MAX_PARTS + part, best, SPEC_RLX_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the slot has left before the ticket does
        const unsigned tk = __hip_atomic_fetch_add(cnt + row, 1u, SPEC_RLX_AGENT);
        last_sh = tk == gridDim.x - 1 ? 1 : 0;
        if (last_sh) __hip_atomic_store(cnt + row, 0u, SPEC_RLX_AGENT);   // re-armed for the next launch
    }
    __syncthreads();
    if (!last_sh || tid >= 64) return;
    // the finisher: one wave, one slot per lane (parts <= 64)
    unsigned long long key = tid < (int)gridDim.x ? __hip_atomic_load(slots + (size_t)row * NG_MAX_PARTS + tid, SPEC_RLX_AGENT) : 0ull;
    key = ng_wave_max(key);
    const int m = (int)(key >> 32);
    const int e = key ? (int)(unsigned)key : (len >= 2 ? len - 1 : 0);    // nothing agrees anywhere: m = 0 at every e, and the largest e is len - 1
    const int n_draft = m >= ngram_min && m > 0 ? min(k, len - e) : 0;
    if (tid < NG_MAX_DRAFT) draft_out[row * NG_MAX_DRAFT + tid] = tid < n_draft ? h[e + tid] : -1;
    if (tid == 0) {
        n_draft_out[row] = n_draft;
        match_out[2 * row] = m;
        match_out[2 * row + 1] = e;
    }
}

size_t ngram_draft_scratch_words() { return (size_t)NG_MAX_SEQ * NG_MAX_PARTS * 2 + NG_MAX_SEQ; }
void ngram_draft_grid(int max_len, int &parts, int &tiles_per_part) {
    const int n_idx = max_len > 1 ? max_len - 1 : 1;
    parts = std::min(NG_MAX_PARTS, (n_idx + NG_PART_MIN_TILES * NG_TILE - 1) / (NG_PART_MIN_TILES * NG_TILE));
    const int per_part = (n_idx + parts - 1) / parts;
    tiles_per_part = (per_part + NG_TILE - 1) / NG_TILE;
}
hipError_t launch_ngram_draft(const int32_t *hist, int n_seq, int cap, const int32_t *len_dev, int max_len, int ngram_min, int ngram_max, int k,
                              int32_t *draft_out, int32_t *n_draft_out, int32_t *match_out, float *scratch, hipStream_t st) {
    if (!hist || !len_dev || !draft_out || !n_draft_out || !match_out || !scratch) return hipErrorInvalidValue;
    if (n_seq < 1 || n_seq > NG_MAX_SEQ || cap < 4 || cap % 4 || cap > NG_MAX_CAP || max_len < 0 || max_len > cap) return hipErrorInvalidValue;
    if (ngram_min < 1 || ngram_min > ngram_max || ngram_max > NG_HALO || k < 1 || k > NG_MAX_DRAFT) return hipErrorInvalidValue;
    if (((uintptr_t)hist & 15) || ((uintptr_t)scratch & 7)) return hipErrorInvalidValue;
    int parts, tiles_per_part;
    ngram_draft_grid(max_len, parts, tiles_per_part);
    unsigned long long *slots = reinterpret_cast<unsigned long long *>(scratch);           // [slots | tickets]
    unsigned *cnt = reinterpret_cast<unsigned *>(slots + (size_t)NG_MAX_SEQ * NG_MAX_PARTS);
    hipLaunchKernelGGL(ngram_draft_kernel, dim3(parts, n_seq), dim3(NG_THREADS), 0, st, hist, cap, len_dev, ngram_min, ngram_max, k, tiles_per_part, slots, cnt,
                       draft_out, n_draft_out, match_out);
    return hipGetLastError();
}

// ---------------------------------------------------------------- a history grows
// hist[seq][base + i] = src[i], i < n, with base = at (at >= 0: the history is cut or reset to `at` tokens first) or the device-side length (at < 0); the
// new length is written back.  What does not fit under cap is not written: the length stops at cap and *overflow is set (pinned host memory, or a device
// word), which the host turns into an error.  One workgroup: the length is read by every thread before one of them replaces it.
__global__ __launch_bounds__(1024) void lookup_append_kernel(int32_t *hist, int cap, int32_t *len_dev, int seq, const int32_t *src, int n, int at, int32_t *overflow) {
    __shared__ int base_sh;
    if (threadIdx.x == 0) base_sh = min(max(at >= 0 ? at : len_dev[seq], 0), cap);
    __syncthreads();
    const int base = base_sh, room = cap - base, fit = n < room ? n : room;
    int32_t *dst = hist + (size_t)seq * cap + base;
    for (int i = threadIdx.x; i < fit; i += 1024) dst[i] = src[i];
    if (threadIdx.x == 0) {
        len_dev[seq] = base + fit;
        if (fit < n) *overflow = 1;
    }
}
hipError_t launch_lookup_append(int32_t *hist, int n_seq, int cap, int32_t *len_dev, int seq, const int32_t *src, int n, int at, int32_t *overflow, hipStream_t st) {
    if (!hist || !len_dev || !overflow || (n > 0 && !src) || n_seq < 1 || n_seq > NG_MAX_SEQ || cap < 1 || cap > NG_MAX_CAP) return hipErrorInvalidValue;
    if (seq < 0 || seq >= n_seq || n < 0 || n > NG_MAX_CAP || at > cap) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lookup_append_kernel, dim3(1), dim3(1024), 0, st, hist, cap, len_dev, seq, src, n, at, overflow);
    return hipGetLastError();
}

}  // namespace mi355
