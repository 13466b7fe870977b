// host/attn_chunks.h — per-token chunk lists of a batched single-token step (AttnArgs::tok_chunks / tok_nchunks, kernels.h).
// Host code only, no HIP: Context::decode_ubatch builds the lists with it before every step that uses them, the attention test entries (csrc/op_entries_attn.cc, through
// op_support.h ChunkLists) build the lists they launch with, and tests/host/host_tests.cc checks it against a restatement.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace mi355 {

constexpr int ATTN_CHUNK_CELLS = 64;   // the lists count 64-cell chunks (attn_decode_dev.h C, attn_out.hip with lists)

// For each of the n_tok tokens, the ascending list of the 64-cell chunks of cells [0, n_kv) that hold at least one occupied cell (pos >= 0) carrying the
// token's sequence bit: lists[t * stride + i], i < counts[t].  A chunk is listed whatever the positions of its cells are - the kernel applies the causal bound.
// cell(i, pos, seqs) reads cell i (0 <= i < n_have; cells from n_have on count as empty); stride >= (n_kv + 63) / 64.
// Returns the longest list's length, at least 1 (the grid's y size must not be 0): a token whose sequence has no cell gets counts[t] = 0.
template <class CellAt>
inline int build_attn_chunk_lists(int n_kv, int n_have, CellAt cell, const int32_t *tok_seq, int n_tok, int stride, int32_t *lists, int32_t *counts) {
    const int nch = (n_kv + ATTN_CHUNK_CELLS - 1) / ATTN_CHUNK_CELLS;
    std::vector<uint64_t> seq_of_chunk((size_t)std::max(nch, 0), 0ull);
    for (int i = 0; i < n_kv && i < n_have; i++) {
        int32_t pos = -1;
        uint64_t seqs = 0;
        cell(i, pos, seqs);
        if (pos >= 0) seq_of_chunk[(size_t)(i / ATTN_CHUNK_CELLS)] |= seqs;
    }
    int lmax = 0;
    for (int t = 0; t < n_tok; t++) {
        int32_t *lst = lists + (size_t)t * stride;
        int c = 0;
        const uint64_t bit = 1ull << (tok_seq[t] & 63);
        for (int ch = 0; ch < nch; ch++) if (seq_of_chunk[(size_t)ch] & bit) lst[c++] = ch;
        counts[t] = c;
        lmax = std::max(lmax, c);
    }
    return lmax < 1 ? 1 : lmax;
}

// Chunk slots the attention grid gets for lists whose longest one has lmax entries: steps of 4 (one captured graph serves four lengths), never more than the stride.
inline int attn_chunk_grid(int lmax, int stride) { return std::min(stride, (lmax + 3) & ~3); }

}  // namespace mi355
