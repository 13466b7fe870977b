// sampling.h — host sampler chain the slot loop applies to one logits row.  Stands in for common_sampler_{init,reset,
// accept,sample,get_candidates} (reference call sites src/llama_server_context.cc:626-628,886,1487,1495,1553,1680-1690);
// chain order per SURVEY.md §A.6: logit_bias -> penalties(last_n, repeat, freq, presence) -> top_k -> typical_p -> top_p
// -> min_p -> temperature (entropy-driven when dynatemp_range > 0; <= 0 => greedy) -> seeded draw.  mirostat 1 / 2 replace
// everything after the penalties by temperature -> the mirostat truncation -> draw, as common_sampler_init chains them
// (upstream common/sampling.cpp, llama-sampling.cpp: llama_sampler_temp_ext / _mirostat / _mirostat_v2).  A grammar (grammar.h) constrains the
// draw the way common_sampler_sample does with grammar_first = false: the chain runs unconstrained, the drawn token is checked against the grammar,
// and only if it is refused the row is masked to the admissible tokens and the chain runs again.  Not carried over: DRY, XTC.
#pragma once

#include <cstdint>
#include <memory>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "grammar.h"

namespace mi355 {

struct SamplingParams {            // defaults of chat_completion_request.h:60-92 / common_params_sampling
    uint32_t seed = 0xFFFFFFFFu;   // -1 => random
    int32_t n_probs = 0;
    int32_t min_keep = 0;
    int32_t top_k = 40;
    float top_p = 0.95f;
    float min_p = 0.05f;
    float typ_p = 1.0f;
    float temp = 0.8f;
    float dynatemp_range = 0.0f, dynatemp_exponent = 1.0f;
    int32_t penalty_last_n = 64;   // 0 = penalties off, -1 = the whole context (penalty_n_ctx tokens)
    int32_t penalty_n_ctx = 0;     // what -1 stands for: the slot's context size
    float penalty_repeat = 1.0f, penalty_freq = 0.0f, penalty_present = 0.0f;
    int32_t mirostat = 0;
    float mirostat_tau = 5.0f, mirostat_eta = 0.1f;
    bool ignore_eos = false;
    std::vector<std::pair<int32_t, float>> logit_bias;
};

struct TokenProb { int32_t tok; float p; };

class Sampler {
  public:
    explicit Sampler(const SamplingParams &p = SamplingParams());
    void reset();
    void accept(int32_t token, bool advance_grammar = true);     // (prompt tokens are accepted without the grammar: src/llama_server_context.cc:1493-1495)
    int32_t sample(const float *logits, int n_vocab);
    // grammar-constrained sampling: `pieces[token]` = the bytes of the token's text ("" for tokens without text), eog[token] != 0 for the end tokens;
    // both belong to the caller and outlive the sampler
    void set_grammar(std::shared_ptr<const Grammar> g, const std::vector<std::string> *pieces, const std::vector<uint8_t> *eog);
    bool has_grammar() const { return gm_ != nullptr; }
    bool grammar_admits(int32_t token) const;
    // the token finish() / the device arg-max produced was refused by the grammar: mask the whole row and run the chain again
    int32_t resample_with_grammar(const float *logits, int n_vocab);
    // sample() = head (logit_bias -> penalties -> top_k over the whole row) + finish().  The head can run on the device instead (SURVEY.md §8f.1,
    // mi355_get_topk_ith): plan_front says whether this sampler's state allows it (false: take sample()) and what to send; finish() then runs the rest
    // of the chain on the (token, adjusted logit) candidates, best first - the same token and the same candidates() as sample() on the whole row
    struct FrontPlan { int k = 0; std::vector<int32_t> tok; std::vector<float> bias; std::vector<int32_t> cnt; };
    bool plan_front(int n_vocab, int max_k, int max_adj, FrontPlan &pl) const;
    int32_t finish(std::vector<TokenProb> &c);
    // true when sample() would return the plain argmax of the raw logits (greedy, nothing modifies them, no probabilities
    // asked for): the caller may then take the device-side argmax instead of reading the row
    bool is_plain_greedy() const;
    void set_greedy_result(int32_t tok) { cand_.assign(1, TokenProb{tok, 1.0f}); }
    // the device sampler (csrc/sample.hip) can run the rest of the chain and the draw as well: no grammar, mirostat, n_probs or dynatemp,
    // top_k within [1, max_k], and top_p, min_p and typ_p inside [0, 1] (the launcher refuses a whole call for one value outside; the host chain reads such a
    // value as "off", so that request alone stays there).  Its RNG is the device's: device_seed() is the Philox key (the request's seed; a random one for
    // seed -1, fixed at reset) and device_draw() the draw counter, which set_device_result() advances: one per token the device sampled.
    bool device_tail_ok(int max_k) const {
        const auto unit = [](float v) { return v >= 0.0f && v <= 1.0f; };   // (false for NaN)
        return !gm_ && p_.mirostat != 1 && p_.mirostat != 2 && p_.n_probs <= 0 && !(p_.dynatemp_range > 0.0f) && p_.top_k >= 1 && p_.top_k <= max_k && p_.min_keep <= max_k &&
               unit(p_.top_p) && unit(p_.min_p) && unit(p_.typ_p);
    }
    // ... and the whole-row kernel (csrc/sample_vocab.hip) the chains the front cannot serve: temp > 0, no grammar, n_probs, dynatemp or
    // typical-p, and either mirostat 2 or a plain chain whose top_k is off (<= 0) or above max_k.  plan_adjust says what to send (false: more than max_adj
    // adjusted tokens, or two biases on one token).  A mirostat-2 row goes with device_mu(); set_device_result_mirostat() takes the token and its probability
    // under the kept distribution and moves mu as the host branch does.
    bool device_vocab_ok(int max_k) const {
        const auto unit = [](float v) { return v >= 0.0f && v <= 1.0f; };
        if (gm_ || !(p_.temp > 0.0f) || p_.mirostat == 1 || p_.n_probs > 0 || p_.dynatemp_range > 0.0f || !(p_.typ_p == 1.0f)) return false;
        if (p_.mirostat == 2) return true;
        return (p_.top_k <= 0 || p_.top_k > max_k) && unit(p_.top_p) && unit(p_.min_p);
    }
    bool plan_adjust(int n_vocab, int max_adj, FrontPlan &pl) const;
    bool device_mirostat() const { return p_.mirostat == 2; }
    float device_mu() const { return mu_; }
    void set_device_result_mirostat(int32_t tok, float p);
    uint64_t device_seed() const { return dev_seed_; }
    uint64_t device_draw() const { return n_draws_; }
    void set_device_result(int32_t tok, float p) { cand_.assign(1, TokenProb{tok, p}); n_draws_++; }
    // candidates of the last sample(), sorted by probability (descending), probabilities after the chain
    const std::vector<TokenProb> &candidates() const { return cand_; }
    const SamplingParams &params() const { return p_; }

  private:
    size_t front_k(int n_vocab) const;
    int32_t sample_chain(const float *logits, int n_vocab);
    SamplingParams p_;
    std::unique_ptr<GrammarMatcher> gm_;
    const std::vector<std::string> *pieces_ = nullptr;
    const std::vector<uint8_t> *eog_ = nullptr;
    std::vector<int32_t> prev_;     // ring of accepted tokens (penalty window)
    std::vector<TokenProb> cand_;
    std::mt19937 rng_;
    uint64_t dev_seed_ = 0, n_draws_ = 0;
    std::vector<float> probs_;       // (scratch of the draw)
    float mu_ = 0.0f;               // mirostat: running surprise target (starts at 2 tau)
};

}  // namespace mi355
