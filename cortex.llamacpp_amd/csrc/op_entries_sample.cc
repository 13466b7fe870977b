// op_entries_sample.cc — per-op test entries of the device samplers: the tail's chain and draw over given candidates (csrc/sample.hip), the whole-row chain over
// given rows (csrc/sample_vocab.hip), and the device's Philox sequence.  Scaffolding: op_support.h.
#include "op_support.h"

using namespace mi355;

extern "C" {

int mi355_op_sample_rows(const int32_t *cand_tok, const float *cand_logit, int32_t R, int32_t k, const mi355_sampler_params *params, const double *u,
                         int32_t *tokens_out, int32_t *n_kept_out, float *probs_out, int32_t *kept_tok_out, float *kept_p_out) { return op_entry([&]() -> int {
    if (!cand_tok || !cand_logit || !params || !tokens_out || !n_kept_out || !probs_out || (kept_tok_out == nullptr) != (kept_p_out == nullptr)) {
        fail("sample_rows: null pointer"); return MI355_ERR_ARG;
    }
    if (R > 65535 * 4) { fail("sample_rows: R above 262140"); return MI355_ERR_ARG; }
    std::vector<SampleParams> sp((size_t)std::max(R, 0));
    for (int r = 0; r < R; r++) {
        const mi355_sampler_params &p = params[r];
        sp[(size_t)r] = SampleParams{p.top_k, p.min_keep, p.top_p, p.min_p, p.typ_p, p.temp, p.stream, 0u, p.seed, 0ull};
    }
    if (const char *word = sample_rows_refusal(R, k, sp.data())) { fail(std::string("sample_rows: ") + word + " outside what the launcher takes"); return MI355_ERR_ARG; }
    // the candidates as the front leaves them: [R][TOPK_MAX_K] keys
    std::vector<unsigned long long> keys((size_t)R * TOPK_MAX_K, 0ull);
    for (int r = 0; r < R; r++)
        for (int j = 0; j < k; j++) {
            unsigned b;
            memcpy(&b, &cand_logit[(size_t)r * k + j], 4);
            b ^= (b >> 31) ? 0xffffffffu : 0x80000000u;
            keys[(size_t)r * TOPK_MAX_K + j] = ((unsigned long long)b << 32) | (0xffffffffu - (unsigned)cand_tok[(size_t)r * k + j]);
        }
    const size_t nr = (size_t)R * 4, nk = (size_t)R * TOPK_MAX_K * 4;
    OpBufs b;
    const unsigned long long *dk = b.upload(keys.data(), keys.size() * 8);  const SampleParams *dp = b.upload(sp.data(), sp.size() * sizeof(SampleParams));
    const double *du = u ? b.upload(u, (size_t)R * 8) : nullptr;
    int32_t *dt = b.alloc<int32_t>(nr), *dn = b.alloc<int32_t>(nr), *dkt = kept_tok_out ? b.alloc<int32_t>(nk) : nullptr;
    float *dpr = b.alloc<float>(nr), *dkp = kept_tok_out ? b.alloc<float>(nk) : nullptr;
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_sample_rows(dk, R, k, sp.data(), dp, du, dt, dpr, dn, dkt, dkp, nullptr), "sample_rows")) return rc;
    if (kept_tok_out) b.down(kept_tok_out, dkt, nk).down(kept_p_out, dkp, nk);
    return b.down(tokens_out, dt, nr).down(n_kept_out, dn, nr).down(probs_out, dpr, nr).done("sample_rows");
}); }

int mi355_op_sample_vocab(const float *rows, int64_t n, int32_t R, const int32_t *adj_n, const int32_t *adj_tok, const float *adj_bias, const int32_t *adj_cnt,
                          const mi355_sampler_params *params, const double *u, const float *mirostat_mu, int32_t *tokens_out, int32_t *n_kept_out, float *probs_out) {
    return op_entry([&]() -> int {
    if (!rows || !params || !tokens_out || !n_kept_out || !probs_out || (adj_n && (!adj_tok || !adj_bias || !adj_cnt))) { fail("sample_vocab: null pointer"); return MI355_ERR_ARG; }
    if (R > 65535) { fail("sample_vocab: R above 65535"); return MI355_ERR_ARG; }
    std::vector<SampleParams> sp((size_t)std::max(R, 0));
    std::vector<TopkAdj> adjs(sp.size());
    for (int r = 0; r < R; r++) {
        const mi355_sampler_params &p = params[r];
        sp[(size_t)r] = SampleParams{p.top_k, p.min_keep, p.top_p, p.min_p, p.typ_p, p.temp, p.stream, 0u, p.seed, 0ull};
        TopkAdj &a = adjs[(size_t)r];
        memset(&a, 0, sizeof a);
        a.n = adj_n ? adj_n[r] : 0; a.repeat = p.penalty_repeat; a.freq = p.penalty_freq; a.present = p.penalty_present;
        if (a.n < 0 || a.n > TOPK_MAX_ADJ) { fail("sample_vocab: adj_n[" + std::to_string(r) + "] outside [0, " + std::to_string(TOPK_MAX_ADJ) + "]"); return MI355_ERR_ARG; }
        const size_t o = (size_t)r * TOPK_MAX_ADJ;
        for (int j = 0; j < a.n; j++) { a.tok[j] = adj_tok[o + j]; a.bias[j] = adj_bias[o + j]; a.cnt[j] = adj_cnt[o + j]; }
    }
    if (const char *word = sample_vocab_refusal(R, n > SAMPLE_VOCAB_MAX_N ? 0 : (int)n, sp.data())) {
        fail(std::string("sample_vocab: ") + word + " outside what the launcher takes"); return MI355_ERR_ARG;
    }
    const size_t nr = (size_t)R * 4;
    OpBufs b;
    const float *dx = b.upload(rows, (size_t)R * (size_t)n * 4);  const SampleParams *dp = b.upload(sp.data(), sp.size() * sizeof(SampleParams));
    const TopkAdj *da = b.upload(adjs.data(), adjs.size() * sizeof(TopkAdj));
    const double *du = u ? b.upload(u, (size_t)R * 8) : nullptr;  const float *dm = mirostat_mu ? b.upload(mirostat_mu, nr) : nullptr;
    int32_t *dt = b.alloc<int32_t>(nr), *dn = b.alloc<int32_t>(nr);
    float *dpr = b.alloc<float>(nr);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_sample_vocab(dx, (int)n, R, nullptr, da, sp.data(), dp, dm, du, dt, dpr, dn, nullptr), "sample_vocab")) return rc;
    return b.down(tokens_out, dt, nr).down(n_kept_out, dn, nr).down(probs_out, dpr, nr).done("sample_vocab");
}); }

int mi355_op_philox_u(uint64_t seed, uint64_t counter0, uint32_t stream, int32_t n, float *out) { return op_entry([&]() -> int {
    if (!out || n < 1 || n > (1 << 24)) { fail("philox_u: bad arguments"); return MI355_ERR_ARG; }
    OpBufs b;
    float *d = b.alloc<float>((size_t)n * 4);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_philox_u(seed, counter0, stream, n, d, nullptr), "philox_u")) return rc;
    return b.down(out, d, (size_t)n * 4).done("philox_u");
}); }

}  // extern "C"
