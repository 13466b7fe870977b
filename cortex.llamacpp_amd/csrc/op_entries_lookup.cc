// op_entries_lookup.cc — the per-op test entry of prompt-lookup drafting (csrc/lookup.hip).  Scaffolding: op_support.h.
#include "op_support.h"

using namespace mi355;

extern "C" {

// host pointers: upload, one launch, download.  The caller's rows are `cap` tokens apart; on the device they start on 16-byte boundaries (cap rounded up to 4).
int mi355_op_ngram_draft(const int32_t *hist, int32_t n_seq, int32_t cap, const int32_t *len, int32_t ngram_min, int32_t ngram_max, int32_t k,
                         int32_t *draft_out, int32_t *n_draft_out, int32_t *match_out) { return op_entry([&]() -> int {
    if (!hist || !len || !draft_out || !n_draft_out || !match_out) { fail("ngram_draft: null pointer"); return MI355_ERR_ARG; }
    if (n_seq < 1 || n_seq > NG_MAX_SEQ) { fail("ngram_draft: n_seq " + std::to_string(n_seq) + " outside [1, 64]"); return MI355_ERR_ARG; }
    if (cap < 1 || cap > NG_MAX_CAP - 3) { fail("ngram_draft: cap " + std::to_string(cap) + " outside [1, 2^24 - 3]"); return MI355_ERR_ARG; }
    if (ngram_max < 1 || ngram_max > NG_MAX_NGRAM) { fail("ngram_draft: ngram_max " + std::to_string(ngram_max) + " outside [1, 16]"); return MI355_ERR_ARG; }
    if (ngram_min < 1 || ngram_min > ngram_max) { fail("ngram_draft: ngram_min " + std::to_string(ngram_min) + " outside [1, ngram_max]"); return MI355_ERR_ARG; }
    if (k < 1 || k > NG_MAX_DRAFT) { fail("ngram_draft: k " + std::to_string(k) + " outside [1, 16]"); return MI355_ERR_ARG; }
    int max_len = 0;
    for (int s = 0; s < n_seq; s++) {
        if (len[s] < 0 || len[s] > cap) { fail("ngram_draft: length " + std::to_string(len[s]) + " of sequence " + std::to_string(s) + " outside [0, cap]"); return MI355_ERR_ARG; }
        max_len = std::max(max_len, len[s]);
    }
    const int capd = (cap + 3) & ~3;
    OpBufs b;
    int32_t *dh = b.alloc<int32_t>((size_t)n_seq * capd * 4);
    const int32_t *dl = b.upload(len, (size_t)n_seq * 4);
    int32_t *dd = b.alloc<int32_t>((size_t)n_seq * NG_MAX_DRAFT * 4), *dn = b.alloc<int32_t>((size_t)n_seq * 4), *dm = b.alloc<int32_t>((size_t)n_seq * 8);
    float *ds = b.alloc<float>(ngram_draft_scratch_words() * 4);
    if (!b.ok()) return oom();
    if (!b.check(hipMemcpy2D(dh, (size_t)capd * 4, hist, (size_t)cap * 4, (size_t)cap * 4, (size_t)n_seq, hipMemcpyHostToDevice) == hipSuccess)) return oom();
    if (const int rc = finish(launch_ngram_draft(dh, n_seq, capd, dl, max_len, ngram_min, ngram_max, k, dd, dn, dm, ds, nullptr), "ngram_draft")) return rc;
    return b.down(draft_out, dd, (size_t)n_seq * NG_MAX_DRAFT * 4).down(n_draft_out, dn, (size_t)n_seq * 4).down(match_out, dm, (size_t)n_seq * 8).done("ngram_draft");
}); }

}  // extern "C"
