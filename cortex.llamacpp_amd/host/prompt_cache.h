// prompt_cache.h — the slot loop's host-RAM prompt cache (/loadmodel key "cache_ram", upstream's --cache-ram): KV states of conversations that lost their slot,
// kept as the blobs IBackend::state_seq_get gives, found again by the longest common prefix with a new prompt.  Host logic only; the blobs are opaque here.
// Whole class in the header: everything that compiles server_context.cc gets it without another translation unit.
//
// One thread (the slot loop) calls everything but stats(), which any thread may call.
#pragma once

#include <atomic>
#include <cstdint>
#include <utility>
#include <vector>

namespace mi355 {

class PromptCache {
  public:
    // The loop saves a slot's sequence when a new prompt would drop at least kMinSave of its cached tokens, and restores an entry when it holds at least kMinGain
    // more of the prompt than the slot itself.  Measured (tools/kv_state_time.py, profiles/kv_state_time.json; Llama-3-8B Q4_K_M, q8_0 cache): a restore plus the
    // last token beats the prefill at every length tried, 64 tokens (1.7 ms against 5.2 ms) being the shortest - so 64, a multiple of 16, is the threshold; below
    // it nothing was measured and a prefill costs a few milliseconds anyway.
    static constexpr int kMinSave = 64, kMinGain = 64;

    struct Entry {
        std::vector<int32_t> tokens;
        std::vector<uint8_t> blob;
        uint64_t last_used = 0;
        size_t bytes() const { return blob.size() + tokens.size() * sizeof(int32_t); }
    };
    enum { ENTRIES = 0, BYTES = 1, SAVES = 2, RESTORES = 3, TOKENS_RESTORED = 4, EVICTIONS = 5, N_STATS = 6 };

    // budget_mib: 0 = off, < 0 = no limit
    explicit PromptCache(int64_t budget_mib) : budget_(budget_mib < 0 ? -1 : budget_mib * 1024 * 1024) { for (auto &s : stats_) s = 0; }
    bool enabled() const { return budget_ != 0; }

    static size_t common_part(const std::vector<int32_t> &a, const std::vector<int32_t> &b) {
        size_t i = 0;
        while (i < a.size() && i < b.size() && a[i] == b[i]) i++;
        return i;
    }
    // the entry with the longest common prefix with `prompt` (the most recently used of equals), -1 when no entry shares a token; best = that length
    int lookup(const std::vector<int32_t> &prompt, size_t &best) const {
        int idx = -1;
        best = 0;
        for (size_t i = 0; i < entries_.size(); i++) {
            const size_t c = common_part(entries_[i].tokens, prompt);
            if (c > best || (c == best && c > 0 && idx >= 0 && entries_[i].last_used > entries_[(size_t)idx].last_used)) { best = c; idx = (int)i; }
        }
        return idx;
    }
    // an entry already holds these tokens (they are a prefix of its own): saving them again adds nothing
    bool covers(const std::vector<int32_t> &tokens) const {
        for (const Entry &e : entries_)
            if (e.tokens.size() >= tokens.size() && common_part(e.tokens, tokens) == tokens.size()) return true;
        return false;
    }
    const Entry &entry(int i) const { return entries_[(size_t)i]; }
    size_t size() const { return entries_.size(); }
    void touch(int i) { entries_[(size_t)i].last_used = ++clock_; }
    void drop(int i) { entries_.erase(entries_.begin() + i); publish(); }
    void restored(size_t n_tokens) { stats_[RESTORES]++; stats_[TOKENS_RESTORED] += (int64_t)n_tokens; }
    // Takes the state of `tokens`.  Entries whose tokens are a prefix of the new ones are replaced by it; the least recently used entries leave until the budget
    // holds it.  false (nothing stored, nothing evicted): the entry alone is larger than the whole budget.
    bool store(std::vector<int32_t> tokens, std::vector<uint8_t> blob) {
        Entry e;
        e.tokens = std::move(tokens); e.blob = std::move(blob); e.last_used = ++clock_;
        if (budget_ > 0 && (int64_t)e.bytes() > budget_) return false;
        for (size_t i = 0; i < entries_.size();) {
            if (entries_[i].tokens.size() <= e.tokens.size() && common_part(entries_[i].tokens, e.tokens) == entries_[i].tokens.size()) entries_.erase(entries_.begin() + (long)i);
            else i++;
        }
        while (budget_ > 0 && !entries_.empty() && (int64_t)(held() + e.bytes()) > budget_) {
            size_t lru = 0;
            for (size_t i = 1; i < entries_.size(); i++) if (entries_[i].last_used < entries_[lru].last_used) lru = i;
            entries_.erase(entries_.begin() + (long)lru);
            stats_[EVICTIONS]++;
        }
        entries_.push_back(std::move(e));
        stats_[SAVES]++;
        publish();
        return true;
    }
    void clear() { entries_.clear(); publish(); }
    void stats(int64_t out[N_STATS]) const { for (int i = 0; i < N_STATS; i++) out[i] = stats_[i].load(); }

  private:
    size_t held() const { size_t b = 0; for (const Entry &e : entries_) b += e.bytes(); return b; }
    void publish() { stats_[ENTRIES] = (int64_t)entries_.size(); stats_[BYTES] = (int64_t)held(); }
    int64_t budget_;
    uint64_t clock_ = 0;
    std::vector<Entry> entries_;
    std::atomic<int64_t> stats_[N_STATS];
};

}  // namespace mi355
