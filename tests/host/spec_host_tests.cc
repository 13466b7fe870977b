// tests/host/spec_host_tests.cc — CPU tests of speculative decoding in the slot loop (server_context.cc UpdateSlots) against a fake arithmetic backend whose
// next token is a function of (token, position) and whose draft model is scripted: proposals all right, all wrong or mixed.  What a request emits must not
// depend on the draft.  Built and run by tests/test_spec_host.py (g++, no HIP, no GPU), once more with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

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
    for (int i = 0; i < 64; i++) { toks.push_back("w" + std::to_string(i) + "."); sc.push_back(1.0f); ty.push_back(TT_NORMAL); }
    Vocab v;
    v.init_spm(toks, sc, ty, 1, 2, 0, true);
    return v;
}
constexpr int FIRST = 259, N_WORDS = 64, EOS = 2;
enum DraftMode { NONE, RIGHT, WRONG, MIXED };

struct FakeBackend : IBackend {
    Vocab voc = make_vocab();
    DraftMode mode = NONE;
    bool device_verify = true;           // spec_verify answers (plain greedy takes it); false: the loop walks the rows itself
    int ctx_len = 256, eos_pos = -1;     // eos_pos: the token that follows position eos_pos is </s>
    std::map<int, std::map<int, int>> kv;
    std::vector<std::vector<float>> last_logits;
    std::vector<int> last_flag_index;
    std::vector<int> rm_calls_p0;        // kv_seq_rm(seq, p0, -1) calls with p0 > 0
    int n_draft_calls = 0, n_draft_rm = 0, n_verify_calls = 0, max_spec_seqs_in_a_batch = 0, max_rows = 0;
    bool embd_on = false;

    int next_of(int tok, int pos) const { return pos == eos_pos ? EOS : FIRST + (tok * 31 + pos * 7 + 11) % N_WORDS; }
    int n_ctx() const override { return ctx_len; }
    int n_batch() const override { return 128; }
    int n_ubatch() const override { return 128; }
    int n_vocab() const override { return voc.n_tokens(); }
    int n_embd() const override { return 8; }
    const Vocab &vocab() const override { return voc; }
    int decode(const BatchView &b) override {
        last_logits.clear(); last_flag_index.assign((size_t)b.n_tokens, -1);
        std::map<int, int> rows_of_seq, first_pos;
        for (int i = 0; i < b.n_tokens; i++) first_pos.emplace(b.seq_id[i], b.pos[i]);
        for (const auto &e : first_pos) { const auto &m = kv[e.first]; if (!m.empty() && m.rbegin()->first >= e.second) n_stale++; }
        for (int i = 0; i < b.n_tokens; i++) {
            kv[b.seq_id[i]][b.pos[i]] = b.token[i];
            if (!b.logits[i]) continue;
            rows_of_seq[b.seq_id[i]]++;
            std::vector<float> lg((size_t)n_vocab(), 0.0f);
            lg[(size_t)next_of(b.token[i], b.pos[i])] = 12.0f;
            last_flag_index[(size_t)i] = (int)last_logits.size();
            last_logits.push_back(std::move(lg));
        }
        int spec_seqs = 0;
        for (const auto &e : rows_of_seq) { if (e.second > 1) spec_seqs++; max_rows = std::max(max_rows, e.second); }
        max_spec_seqs_in_a_batch = std::max(max_spec_seqs_in_a_batch, spec_seqs);
        return 0;
    }
    const float *logits_ith(int i) override { return (i >= 0 && i < (int)last_flag_index.size() && last_flag_index[(size_t)i] >= 0) ? last_logits[(size_t)last_flag_index[(size_t)i]].data() : nullptr; }
    void set_embeddings(bool on) override { embd_on = on; }
    const float *embeddings_ith(int) override { return nullptr; }
    std::map<int, std::map<int, int>> kv_at_clear;   // what the loop's clean-up of an idle cache (KvCacheClear) found
    int n_stale = 0;                                 // decodes that found cells of their sequence at or behind the first position they write
    void kv_clear() override { if (!kv.empty()) kv_at_clear = kv; kv.clear(); }
    bool kv_seq_rm(int seq, int p0, int p1) override {
        if (p0 > 0 && p1 < 0) rm_calls_p0.push_back(p0);
        auto &m = kv[seq];
        for (auto it = m.begin(); it != m.end();) { if (it->first >= (p0 < 0 ? 0 : p0) && (p1 < 0 || it->first < p1)) it = m.erase(it); else ++it; }
        return true;
    }
    void kv_seq_add(int seq, int p0, int p1, int delta) override {       // positions [p0, p1) move by delta
        std::map<int, int> m;
        for (const auto &e : kv[seq]) m[e.first >= p0 && e.first < p1 ? e.first + delta : e.first] = e.second;
        kv[seq] = m;
    }
    void kv_seq_cp(int, int, int, int) override {}
    // ---- images: "IMG" + a byte n = an image of n embedding rows (the fake of tests/host/host_tests.cc)
    bool mm = false;
    int n_embd_calls = 0;
    bool multimodal() const override { return mm; }
    bool image_check(const uint8_t *b, size_t n, std::string &err) override { if (n == 4 && !memcmp(b, "IMG", 3) && b[3] > 0) return true; err = "not an image"; return false; }
    int image_embed(const uint8_t *b, size_t n, std::vector<float> &rows, std::string &err) override {
        if (!image_check(b, n, err)) return -1;
        rows.assign((size_t)b[3] * (size_t)n_embd(), (float)b[3]);
        return (int)b[3];
    }
    int decode_embd(const float *, int n, int pos0, int seq) override {
        n_embd_calls++;
        for (int i = 0; i < n; i++) kv[seq][pos0 + i] = -1;
        return 0;
    }
    // ---- the scripted draft
    bool has_draft() const override { return mode != NONE; }
    int spec_draft(int seq, const int32_t *tokens, int n_tokens, int n_max, float, int32_t *out) override {
        (void)seq;
        n_draft_calls++;
        int t = tokens[n_tokens - 1], pos = n_tokens - 1;
        const int n_right = mode == RIGHT ? n_max : mode == WRONG ? 0 : n_draft_calls % 4;      // mixed: 1, 2, 3, 0 right ones, then a wrong one
        const int n = mode == MIXED ? std::min(n_max, 1 + n_draft_calls % 5) : n_max;
        for (int j = 0; j < n; j++) {
            int nx = next_of(t, pos);
            if (j >= n_right) nx = nx == EOS ? FIRST : FIRST + (nx - FIRST + 1) % N_WORDS;
            out[j] = nx; t = nx; pos++;
        }
        return n;
    }
    bool spec_verify(int n_groups, const int32_t *gs, const int32_t *draft, int32_t *ids, int32_t *n_accept) override {
        if (!device_verify) return false;
        n_verify_calls++;
        for (int r = gs[0]; r < gs[n_groups]; r++) {
            const float *row = logits_ith(r);
            if (!row) return false;
            int best = 0;
            for (int v = 1; v < n_vocab(); v++) if (row[v] > row[best]) best = v;
            ids[r - gs[0]] = best;
        }
        for (int g = 0; g < n_groups; g++) {
            int a = 0;
            for (int r = gs[g]; r < gs[g + 1] - 1 && ids[r - gs[0]] == draft[r - gs[0]]; r++) a++;
            n_accept[g] = a;
        }
        return true;
    }
    void draft_seq_rm(int, int) override { n_draft_rm++; }
};

static Json prompt_of(int salt, int n) {
    Json a = Json::array();
    for (int i = 0; i < n; i++) a.push_back(Json((int64_t)(FIRST + (i * (2 * salt + 1) + 3 * salt) % N_WORDS)));
    return a;
}
static Json request(int salt, int n_prompt, int n_predict, double temp = 0.0) {
    Json d = Json::object();
    d["prompt"] = prompt_of(salt, n_prompt); d["n_predict"] = n_predict; d["temperature"] = temp; d["seed"] = 42; d["cache_prompt"] = true; d["stream"] = false;
    return d;
}
struct Run { std::string content; int predicted = 0, cached = 0; int64_t stats[4] = {0, 0, 0, 0}; bool ok = false, truncated = false; };
// one request on a fresh context; the fake is left as the request left it
static Run run_one(FakeBackend &be, const Json &d, int draft_max = 4) {
    ServerParams sp;
    sp.draft_max = draft_max;
    LlamaServerContext ctx(&be, sp);
    ctx.Initialize();
    const TaskResult r = ctx.NextResult(ctx.RequestCompletion(d, false, false, -1));
    Run out;
    out.ok = r.stop && !r.error;
    if (out.ok) {
        out.content = r.result_json["content"].as_string();
        out.predicted = (int)r.result_json["tokens_predicted"].as_int();
        out.cached = (int)r.result_json["tokens_cached"].as_int();
        out.truncated = r.result_json["truncated"].is_bool() && r.result_json["truncated"].as_bool();
    }
    ctx.SpecStats(out.stats);
    ctx.ReleaseResources();
    return out;
}
// the target's cache holds positions 0 .. tokens_cached - 1 and nothing behind them
static bool kv_is_exact(FakeBackend &be, const Run &r) {
    const auto &m = be.kv[0].empty() ? be.kv_at_clear[0] : be.kv[0];
    return be.n_stale == 0 && (int)m.size() == r.cached && !m.empty() && m.rbegin()->first == r.cached - 1;
}

static void test_text_does_not_depend_on_the_draft() {
    for (double temp : {0.0, 0.8})
        for (bool device_verify : {true, false}) {
            FakeBackend base;
            const Run want = run_one(base, request(1, 20, 24, temp));
            CHECK(want.ok && want.predicted >= 24 && base.n_draft_calls == 0 && kv_is_exact(base, want));
            for (DraftMode m : {RIGHT, WRONG, MIXED}) {
                FakeBackend be;
                be.mode = m; be.device_verify = device_verify;
                const Run got = run_one(be, request(1, 20, 24, temp));
                CHECK(got.ok && got.content == want.content && got.predicted == want.predicted && got.cached == want.cached);
                CHECK(kv_is_exact(be, got));
                CHECK(be.n_draft_calls > 0 && be.max_rows > 1 && be.n_draft_rm > 0);
                CHECK((be.n_verify_calls > 0) == (device_verify && temp == 0.0));                // plain greedy: the device call; any other sampler walks its rows
                // the counters: accepted <= drafted, at least one drafted token per round; all wrong: none accepted; all right (greedy): all but the cut
                // the counters add up: every round emits the target's own token and its accepted drafts; a drafted token is accepted or not
                CHECK(got.predicted == got.stats[0] + got.stats[2]);
                CHECK(got.stats[0] > 0 && got.stats[1] >= got.stats[2] && got.stats[1] >= got.stats[0] - got.stats[3]);
                if (m == WRONG) CHECK(got.stats[2] == 0);
                if (m == RIGHT) CHECK(got.stats[2] == got.stats[1] && got.stats[2] > 0 && got.stats[3] == 0);      // (k is capped by what may still be emitted: none is cut)
                if (m == MIXED) CHECK(got.stats[2] > 0 && got.stats[2] < got.stats[1]);
                if (m == WRONG) CHECK(!be.rm_calls_p0.empty());                                  // rejected rows were rolled back
            }
        }
}

static void test_n_predict_stop_string_and_eos_cut_inside_an_accepted_run() {
    // n_predict: every count from 1 on, so that the cut falls on every place of a round
    for (int n_predict = 1; n_predict <= 9; n_predict++) {
        FakeBackend base, be;
        be.mode = RIGHT;
        const Run want = run_one(base, request(2, 16, n_predict)), got = run_one(be, request(2, 16, n_predict));
        CHECK(want.ok && got.ok && got.content == want.content && got.predicted == want.predicted && got.cached == want.cached);
        CHECK(kv_is_exact(base, want) && kv_is_exact(be, got));
        CHECK(got.predicted == got.stats[0] + got.stats[2] && got.stats[2] <= got.stats[1]);
    }
    // a stop string in the middle of the text
    {
        FakeBackend base0;
        const Run full = run_one(base0, request(3, 16, 20));
        CHECK(full.ok && full.content.size() > 30);
        const std::string stop = full.content.substr(full.content.size() / 2, 5);
        Json d = request(3, 16, 20);
        Json stops = Json::array(); stops.push_back(Json(stop));
        d["stop"] = stops;
        FakeBackend base, be;
        be.mode = RIGHT;
        const Run want = run_one(base, d), got = run_one(be, d, 8);
        CHECK(want.ok && got.ok && want.content.size() < full.content.size());
        CHECK(got.content == want.content && got.predicted == want.predicted && got.cached == want.cached && kv_is_exact(be, got));
    }
    // </s> as the fifth generated token, inside a run of eight right drafts
    {
        FakeBackend base, be;
        base.eos_pos = be.eos_pos = 16 + 3;
        be.mode = RIGHT;
        const Run want = run_one(base, request(4, 16, 20)), got = run_one(be, request(4, 16, 20), 8);
        CHECK(want.ok && got.ok && want.predicted < 10);
        CHECK(got.content == want.content && got.predicted == want.predicted && got.cached == want.cached && kv_is_exact(be, got));
    }
}

static void test_grammar_and_n_probs_requests_never_ask_the_draft() {
    {
        FakeBackend be;
        be.mode = RIGHT;
        Json d = request(5, 16, 8);
        d["n_probs"] = 2;
        const Run r = run_one(be, d);
        CHECK(r.ok && be.n_draft_calls == 0 && be.max_rows == 1 && r.stats[0] == 0 && r.stats[3] == 0);
    }
    {
        FakeBackend be;
        be.mode = RIGHT;
        Json d = request(5, 16, 8);
        d["grammar"] = "root ::= [w0-9.]*";
        const Run r = run_one(be, d);
        CHECK(r.ok && be.n_draft_calls == 0 && be.max_rows == 1);
    }
}

static std::string b64(const std::string &in) {
    static const char *tbl = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
    std::string out;
    for (size_t i = 0; i < in.size(); i += 3) {
        const unsigned n = (unsigned)(uint8_t)in[i] << 16 | (i + 1 < in.size() ? (unsigned)(uint8_t)in[i + 1] << 8 : 0) | (i + 2 < in.size() ? (unsigned)(uint8_t)in[i + 2] : 0);
        out += tbl[n >> 18 & 63]; out += tbl[n >> 12 & 63];
        out += i + 1 < in.size() ? tbl[n >> 6 & 63] : '=';
        out += i + 2 < in.size() ? tbl[n & 63] : '=';
    }
    return out;
}
// a request with a picture on a multimodal context that also has a draft model: the rows reach the model, the draft is never asked, every tick is one row
static void test_image_requests_never_ask_the_draft() {
    Json d = Json::object();
    d["prompt"] = "see [img-1] now"; d["n_predict"] = 8; d["temperature"] = 0.0; d["stream"] = false; d["cache_prompt"] = true;
    Json im = Json::object(), imgs = Json::array();
    im["id"] = 1; im["data"] = b64(std::string("IMG") + (char)5);
    imgs.push_back(im);
    d["image_data"] = imgs;
    FakeBackend base, be;
    base.mm = be.mm = true;
    be.mode = RIGHT;
    const Run want = run_one(base, d), got = run_one(be, d);
    CHECK(want.ok && got.ok && want.predicted >= 8 && base.n_embd_calls == 1 && be.n_embd_calls == 1);
    CHECK(got.content == want.content && got.predicted == want.predicted && got.cached == want.cached);
    CHECK(be.n_draft_calls == 0 && be.max_rows == 1 && be.n_verify_calls == 0);
    for (int i = 0; i < 4; i++) CHECK(got.stats[i] == 0);
    // the same context then serves a text request with drafts: the guard is the request's, not the context's
    FakeBackend be2;
    be2.mm = true; be2.mode = RIGHT;
    const Run text = run_one(be2, request(5, 16, 8));
    CHECK(text.ok && be2.n_draft_calls > 0 && be2.max_rows > 1);
}

static void test_two_slots_speculate_in_one_tick() {
    FakeBackend base1, base2;
    const Run want1 = run_one(base1, request(6, 16, 40)), want2 = run_one(base2, request(7, 18, 40));
    FakeBackend be;
    be.mode = MIXED;
    ServerParams sp;
    sp.n_parallel = 2; sp.draft_max = 4;
    LlamaServerContext ctx(&be, sp);
    ctx.Initialize();
    const int t1 = ctx.RequestCompletion(request(6, 16, 40), false, false, -1), t2 = ctx.RequestCompletion(request(7, 18, 40), false, false, -1);
    const TaskResult r1 = ctx.NextResult(t1), r2 = ctx.NextResult(t2);
    ctx.ReleaseResources();
    CHECK(r1.stop && !r1.error && r2.stop && !r2.error);
    CHECK(r1.result_json["content"].as_string() == want1.content && r2.result_json["content"].as_string() == want2.content);
    CHECK(be.max_spec_seqs_in_a_batch == 2);
}

static void test_context_shift_still_fires() {
    FakeBackend base, be;
    base.ctx_len = be.ctx_len = 48;
    be.mode = RIGHT;
    const Run want = run_one(base, request(8, 20, 60)), got = run_one(be, request(8, 20, 60));
    CHECK(want.ok && got.ok && want.truncated && got.truncated);
    CHECK(got.content == want.content && got.predicted == want.predicted && got.cached == want.cached);
    CHECK(be.n_draft_calls > 0 && got.stats[2] > 0 && got.predicted == got.stats[0] + got.stats[2]);
}

int main() {
    test_text_does_not_depend_on_the_draft();
    test_n_predict_stop_string_and_eos_cut_inside_an_accepted_run();
    test_grammar_and_n_probs_requests_never_ask_the_draft();
    test_image_requests_never_ask_the_draft();
    test_two_slots_speculate_in_one_tick();
    test_context_shift_still_fires();
    if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
    printf("all speculative-decoding host checks passed\n");
    return 0;
}
