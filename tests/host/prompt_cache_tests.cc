// tests/host/prompt_cache_tests.cc — CPU tests of the host-RAM prompt cache (host/prompt_cache.h) and of what the slot loop does with it (server_context.cc
// PromptCacheVisit), against a fake arithmetic backend whose sequence states are blobs derived from the tokens it was given.  Built with the address and
// undefined-behaviour sanitizers and run by tests/test_prompt_cache_cpu.py (g++, no HIP, no GPU).
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../cortex.llamacpp_amd/host/prompt_cache.h"
#include "../../cortex.llamacpp_amd/host/server_context.h"
#include "../../cortex.llamacpp_amd/host/vocab.h"

using namespace mi355;

static int g_fail = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); g_fail++; } \
    } while (0)

static Vocab make_vocab() {
    std::vector<std::string> toks = {"<unk>", "<s>", "</s>"};
    std::vector<float> sc = {0, 0, 0};
    std::vector<int> ty = {TT_UNKNOWN, TT_CONTROL, TT_CONTROL};
    for (int b = 0; b < 256; b++) { char buf[8]; snprintf(buf, sizeof buf, "<0x%02X>", b); toks.push_back(buf); sc.push_back(0); ty.push_back(TT_BYTE); }
    for (int i = 0; i < 64; i++) { toks.push_back("w" + std::to_string(i)); sc.push_back(1.0f); ty.push_back(TT_NORMAL); }
    Vocab v;
    v.init_spm(toks, sc, ty, 1, 2, 0, true);
    return v;
}
constexpr int FIRST = 259, N_WORDS = 64;
constexpr int N_PROMPT = 100;                       // tokens of a conversation's prompt: more than PromptCache::kMinGain / kMinSave, fewer than a batch
static_assert(N_PROMPT >= PromptCache::kMinGain + 16 && N_PROMPT >= PromptCache::kMinSave + 16, "the prompts must be long enough for the save / restore rules to apply");

// sequences are maps position -> token; a state blob is {n, pad, (position, token) x n, pad bytes}: what a set gives back is exactly what a get took
struct FakeBackend : IBackend {
    Vocab voc = make_vocab();
    std::map<int, std::map<int, int>> kv;
    std::vector<std::vector<int32_t>> calls_tokens, calls_pos;
    std::vector<std::vector<float>> last_logits;
    std::vector<int> last_flag_index;
    int n_size = 0, n_get = 0, n_set = 0;
    bool refuse_set = false, has_state = true;
    size_t pad = 0;                      // extra bytes per blob (the budget is counted in MiB)
    bool embd_on = false;
    std::vector<float> embd_row;

    int n_ctx() const override { return 256; }
    int n_batch() const override { return 128; }
    int n_ubatch() const override { return 128; }
    int n_vocab() const override { return voc.n_tokens(); }
    int n_embd() const override { return 8; }
    const Vocab &vocab() const override { return voc; }
    int decode(const BatchView &b) override {
        calls_tokens.emplace_back(b.token, b.token + b.n_tokens);
        calls_pos.emplace_back(b.pos, b.pos + b.n_tokens);
        last_logits.clear(); last_flag_index.assign((size_t)b.n_tokens, -1);
        for (int i = 0; i < b.n_tokens; i++) {
            kv[b.seq_id[i]][b.pos[i]] = b.token[i];
            if (!b.logits[i]) continue;
            std::vector<float> lg((size_t)n_vocab(), 0.0f);
            lg[(size_t)(FIRST + (b.token[i] * 31 + b.pos[i] * 7 + 11) % N_WORDS)] = 12.0f;
            last_flag_index[(size_t)i] = (int)last_logits.size();
            last_logits.push_back(std::move(lg));
        }
        return 0;
    }
    const float *logits_ith(int i) override { return (i >= 0 && i < (int)last_flag_index.size() && last_flag_index[(size_t)i] >= 0) ? last_logits[(size_t)last_flag_index[(size_t)i]].data() : nullptr; }
    void set_embeddings(bool on) override { embd_on = on; }
    const float *embeddings_ith(int i) override {
        if (!embd_on || i < 0 || i >= (int)last_flag_index.size() || last_flag_index[(size_t)i] < 0) return nullptr;
        embd_row.assign((size_t)n_embd(), 0.5f);
        return embd_row.data();
    }
    void kv_clear() override { kv.clear(); }
    bool kv_seq_rm(int seq, int p0, int p1) override {
        auto &m = kv[seq];
        for (auto it = m.begin(); it != m.end();) { if (it->first >= (p0 < 0 ? 0 : p0) && (p1 < 0 || it->first < p1)) it = m.erase(it); else ++it; }
        return true;
    }
    void kv_seq_add(int, int, int, int) override {}
    void kv_seq_cp(int, int, int, int) override {}
    size_t state_seq_size(int seq) override { n_size++; return has_state ? 8 + 8 * kv[seq].size() + pad : 0; }
    size_t state_seq_get(int seq, uint8_t *dst, size_t cap) override {
        n_get++;
        const auto &m = kv[seq];
        const size_t need = 8 + 8 * m.size() + pad;
        if (!has_state || cap < need) return 0;
        memset(dst, 0, need);
        const uint32_t n = (uint32_t)m.size();
        memcpy(dst, &n, 4);
        size_t o = 8;
        for (const auto &e : m) { const int32_t pt[2] = {e.first, e.second}; memcpy(dst + o, pt, 8); o += 8; }
        return need;
    }
    size_t state_seq_set(int seq, const uint8_t *src, size_t len) override {
        n_set++;
        if (!has_state || refuse_set || len < 8) return 0;
        uint32_t n = 0;
        memcpy(&n, src, 4);
        if (len < 8 + 8 * (size_t)n) return 0;
        std::map<int, int> m;
        for (uint32_t i = 0; i < n; i++) { int32_t pt[2]; memcpy(pt, src + 8 + 8 * (size_t)i, 8); m[pt[0]] = pt[1]; }
        kv[seq] = m;
        return len;
    }
};

static Json prompt_of(int salt, int n) {
    Json a = Json::array();
    for (int i = 0; i < n; i++) a.push_back(Json((int64_t)(FIRST + (i * (2 * salt + 1) + 3 * salt) % N_WORDS)));
    return a;
}
static Json request(int salt, int n, bool cache_prompt = true) {
    Json d = Json::object();
    d["prompt"] = prompt_of(salt, n); d["n_predict"] = 3; d["temperature"] = 0.0; d["cache_prompt"] = cache_prompt;
    return d;
}
static TaskResult run(LlamaServerContext &ctx, const Json &d, bool embedding = false) { return ctx.NextResult(ctx.RequestCompletion(d, false, embedding, -1)); }
struct Stats { int64_t v[6]; int64_t entries() const { return v[0]; } int64_t bytes() const { return v[1]; } int64_t saves() const { return v[2]; }
               int64_t restores() const { return v[3]; } int64_t tokens_restored() const { return v[4]; } int64_t evictions() const { return v[5]; } };
static Stats stats_of(const LlamaServerContext &ctx) { Stats s; ctx.PromptCacheStats(s.v); return s; }

// ---------------------------------------------------------------- the store on its own
static std::vector<int32_t> seq_tokens(int salt, int n) { std::vector<int32_t> t; for (int i = 0; i < n; i++) t.push_back(salt * 1000 + i); return t; }

static void test_store_lru_by_bytes() {
    PromptCache pc(1);                                                  // 1 MiB: two entries of 400 KiB, not three
    const size_t blob = 400 * 1024;
    CHECK(pc.enabled() && !PromptCache(0).enabled() && PromptCache(-1).enabled());
    CHECK(pc.store(seq_tokens(1, 20), std::vector<uint8_t>(blob, 1)));
    CHECK(pc.store(seq_tokens(2, 20), std::vector<uint8_t>(blob, 2)));
    size_t best = 0;
    int idx = pc.lookup(seq_tokens(1, 30), best);
    CHECK(idx >= 0 && best == 20 && pc.entry(idx).blob[0] == 1);
    pc.touch(idx);                                                      // entry 1 is now the most recently used: entry 2 leaves first
    CHECK(pc.store(seq_tokens(3, 20), std::vector<uint8_t>(blob, 3)));
    int64_t s[6];
    pc.stats(s);
    CHECK(s[PromptCache::ENTRIES] == 2 && s[PromptCache::EVICTIONS] == 1 && s[PromptCache::SAVES] == 3);
    CHECK(s[PromptCache::BYTES] == (int64_t)(2 * (blob + 20 * 4)));
    CHECK(pc.lookup(seq_tokens(2, 20), best) == -1 && best == 0);
    CHECK(pc.lookup(seq_tokens(1, 20), best) >= 0 && best == 20);
    CHECK(pc.lookup(seq_tokens(3, 5), best) >= 0 && best == 5);
    // larger than the whole budget: not stored, nothing evicted
    CHECK(!pc.store(seq_tokens(4, 20), std::vector<uint8_t>(2 * 1024 * 1024, 4)));
    pc.stats(s);
    CHECK(s[PromptCache::ENTRIES] == 2 && s[PromptCache::EVICTIONS] == 1 && s[PromptCache::SAVES] == 3);
    // no limit
    PromptCache big(-1);
    for (int i = 0; i < 5; i++) CHECK(big.store(seq_tokens(10 + i, 8), std::vector<uint8_t>(blob, 0)));
    big.stats(s);
    CHECK(s[PromptCache::ENTRIES] == 5 && s[PromptCache::EVICTIONS] == 0);
    big.clear();
    big.stats(s);
    CHECK(s[PromptCache::ENTRIES] == 0 && s[PromptCache::BYTES] == 0 && s[PromptCache::SAVES] == 5);
}

static void test_store_entry_replaced_by_one_that_extends_it() {
    PromptCache pc(-1);
    CHECK(pc.store(seq_tokens(1, 20), std::vector<uint8_t>(100, 1)));
    CHECK(pc.store(seq_tokens(2, 20), std::vector<uint8_t>(100, 2)));
    CHECK(pc.covers(seq_tokens(1, 20)) && pc.covers(seq_tokens(1, 12)) && !pc.covers(seq_tokens(1, 21)));
    CHECK(pc.store(seq_tokens(1, 35), std::vector<uint8_t>(150, 3)));   // the same conversation, further along
    int64_t s[6];
    pc.stats(s);
    CHECK(s[PromptCache::ENTRIES] == 2 && s[PromptCache::EVICTIONS] == 0 && s[PromptCache::BYTES] == 100 + 20 * 4 + 150 + 35 * 4);
    size_t best = 0;
    const int idx = pc.lookup(seq_tokens(1, 40), best);
    CHECK(idx >= 0 && best == 35 && pc.entry(idx).blob.size() == 150 && pc.entry(idx).blob[0] == 3);
    CHECK(pc.covers(seq_tokens(1, 35)));
    CHECK(pc.store(seq_tokens(1, 10), std::vector<uint8_t>(50, 4)));    // a shorter one replaces nothing (the loop asks covers() first and does not store it)
    pc.stats(s);
    CHECK(s[PromptCache::ENTRIES] == 3);
}

// ---------------------------------------------------------------- the slot loop
static void test_cache_ram_zero_makes_no_state_call() {
    FakeBackend be;
    ServerParams sp;                                                    // cache_ram_mib 0
    LlamaServerContext ctx(&be, sp);
    ctx.Initialize();
    for (int salt : {1, 2, 1}) { TaskResult r = run(ctx, request(salt, N_PROMPT)); CHECK(r.stop && !r.error); }
    ctx.ReleaseResources();
    CHECK(be.n_size == 0 && be.n_get == 0 && be.n_set == 0);
    const Stats s = stats_of(ctx);
    for (int i = 0; i < 6; i++) CHECK(s.v[i] == 0);
}

static void test_a_b_a_on_one_slot() {
    FakeBackend be;
    ServerParams sp;
    sp.cache_ram_mib = 64;
    LlamaServerContext ctx(&be, sp);
    ctx.Initialize();
    TaskResult ra1 = run(ctx, request(1, N_PROMPT));
    CHECK(ra1.stop && stats_of(ctx).saves() == 0 && be.n_get == 0 && be.n_set == 0);      // nothing to drop yet
    TaskResult rb = run(ctx, request(2, N_PROMPT));
    Stats s = stats_of(ctx);
    CHECK(rb.stop && s.saves() == 1 && s.restores() == 0 && s.entries() == 1 && be.n_get == 1 && be.n_set == 0);   // B drops A: A is saved
    const size_t ncalls = be.calls_tokens.size();
    TaskResult ra2 = run(ctx, request(1, N_PROMPT));
    s = stats_of(ctx);
    CHECK(ra2.stop && s.saves() == 2 && s.restores() == 1 && s.entries() == 2 && be.n_get == 2 && be.n_set == 1);  // A drops B: B is saved, A comes back
    CHECK(s.tokens_restored() == N_PROMPT && s.evictions() == 0);
    // n_past = the prompt's length minus 1: one prompt token was evaluated, the last one, at the last position
    CHECK(be.calls_tokens.size() > ncalls && be.calls_tokens[ncalls].size() == 1 && be.calls_pos[ncalls][0] == N_PROMPT - 1);
    CHECK(be.calls_tokens[ncalls][0] == (int32_t)prompt_of(1, N_PROMPT).items()[(size_t)N_PROMPT - 1].as_int());
    CHECK(ra2.result_json["tokens_evaluated"].as_int() == N_PROMPT);
    CHECK(ra2.result_json["content"].as_string() == ra1.result_json["content"].as_string());
    // the same conversation once more: the slot's own cache serves it, no state call
    TaskResult ra3 = run(ctx, request(1, N_PROMPT));
    s = stats_of(ctx);
    CHECK(ra3.stop && s.saves() == 2 && s.restores() == 1 && be.n_get == 2 && be.n_set == 1);
    ctx.ReleaseResources();
    CHECK(stats_of(ctx).entries() == 0 && stats_of(ctx).bytes() == 0);                      // the store goes with the model
}

static void test_refused_restore_falls_back_and_drops_the_entry() {
    FakeBackend be;
    ServerParams sp;
    sp.cache_ram_mib = -1;
    LlamaServerContext ctx(&be, sp);
    ctx.Initialize();
    // A, then B, then A with restores refused
    CHECK(run(ctx, request(1, N_PROMPT)).stop);
    CHECK(run(ctx, request(2, N_PROMPT)).stop);
    CHECK(stats_of(ctx).entries() == 1);
    be.refuse_set = true;
    const size_t ncalls = be.calls_tokens.size();
    TaskResult r = run(ctx, request(1, N_PROMPT));
    const Stats s = stats_of(ctx);
    CHECK(r.stop && !r.error && be.n_set == 1 && s.restores() == 0 && s.tokens_restored() == 0);
    CHECK(s.entries() == 1 && s.saves() == 2);                          // B's entry stays, A's was dropped
    // the slot's own common part with A is 0 tokens: the whole prompt was evaluated
    CHECK(be.calls_tokens.size() > ncalls && be.calls_tokens[ncalls].size() == (size_t)N_PROMPT && be.calls_pos[ncalls][0] == 0);
    be.refuse_set = false;
    const int n_set = be.n_set;
    CHECK(run(ctx, request(2, N_PROMPT)).stop && be.n_set == n_set + 1 && stats_of(ctx).restores() == 1);   // B's entry is still good
    ctx.ReleaseResources();
}

static void test_embedding_and_uncached_requests_touch_nothing() {
    FakeBackend be;
    ServerParams sp;
    sp.cache_ram_mib = 64;
    LlamaServerContext ctx(&be, sp);
    ctx.Initialize();
    CHECK(run(ctx, request(1, N_PROMPT)).stop);
    const int n_size = be.n_size;
    TaskResult e = run(ctx, request(2, N_PROMPT), true);                      // an embedding request (cache_prompt set)
    CHECK(!e.error && e.result_json["embedding"].is_array());
    TaskResult u = run(ctx, request(3, N_PROMPT, false));                     // cache_prompt false
    CHECK(u.stop && !u.error);
    ctx.ReleaseResources();
    CHECK(be.n_size == n_size && be.n_get == 0 && be.n_set == 0);
    const Stats s = stats_of(ctx);
    CHECK(s.saves() == 0 && s.restores() == 0);
}

static void test_backend_without_state_keeps_the_cache_off() {
    FakeBackend be;
    be.has_state = false;
    ServerParams sp;
    sp.cache_ram_mib = 64;
    LlamaServerContext ctx(&be, sp);
    ctx.Initialize();
    for (int salt : {1, 2, 1}) CHECK(run(ctx, request(salt, N_PROMPT)).stop);
    ctx.ReleaseResources();
    CHECK(be.n_size == 1 && be.n_get == 0 && be.n_set == 0);            // asked once, at start-up
}

static void test_loop_evicts_under_a_budget_of_two() {
    FakeBackend be;
    be.pad = 400 * 1024;
    ServerParams sp;
    sp.cache_ram_mib = 1;
    LlamaServerContext ctx(&be, sp);
    ctx.Initialize();
    for (int salt : {1, 2, 3, 4}) CHECK(run(ctx, request(salt, N_PROMPT)).stop);      // saves 1, 2, 3: the third evicts conversation 1
    Stats s = stats_of(ctx);
    CHECK(s.saves() == 3 && s.entries() == 2 && s.evictions() == 1 && s.bytes() <= 1024 * 1024);
    const size_t ncalls = be.calls_tokens.size();
    CHECK(run(ctx, request(1, N_PROMPT)).stop);                                        // conversation 1 is gone: a whole prefill (and 4 is saved, evicting 2)
    s = stats_of(ctx);
    CHECK(s.restores() == 0 && s.saves() == 4 && s.evictions() == 2 && be.calls_tokens[ncalls].size() == (size_t)N_PROMPT);
    CHECK(run(ctx, request(3, N_PROMPT)).stop);                                        // conversation 3 is still there
    CHECK(stats_of(ctx).restores() == 1);
    ctx.ReleaseResources();
}

int main() {
    test_store_lru_by_bytes();
    test_store_entry_replaced_by_one_that_extends_it();
    test_cache_ram_zero_makes_no_state_call();
    test_a_b_a_on_one_slot();
    test_refused_restore_falls_back_and_drops_the_entry();
    test_embedding_and_uncached_requests_touch_nothing();
    test_backend_without_state_keeps_the_cache_off();
    test_loop_evicts_under_a_budget_of_two();
    if (g_fail) { printf("%d prompt-cache checks FAILED\n", g_fail); return 1; }
    printf("all prompt-cache checks passed\n");
    return 0;
}
