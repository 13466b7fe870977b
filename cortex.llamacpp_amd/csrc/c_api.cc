// c_api.cc — the C-ABI declared in include/mi355_llama.h, over host/runtime.{h,cc}.
#include "../../include/mi355_llama.h"

#include <atomic>
#include <memory>
#include <new>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../host/clip.h"
#include "../host/engine.h"
#include "../host/hip_backend.h"
#include "../host/log.h"
#include "../host/runtime.h"
#include "../host/attn_chunks.h"
#include "../host/tp_comm.h"
#include "../host/tp_split.h"
#include "../host/vocab.h"

namespace mi355 {
const std::string &last_error_string();
void set_state_stage_max(size_t bytes);       // host/runtime.cc: the staging bound of Context::state_seq_get / set (tests)
}

using namespace mi355;

struct mi355_model {
    Model *m;
    Vocab vocab;            // loaded on first tokenizer call
    bool vocab_tried = false, vocab_ok = false;
};
typedef void (*mi355_release_fn)(void *);
struct mi355_engine {
    LlamaEngine eng{make_hip_backend};
    std::atomic<mi355_release_fn> release{nullptr};     // mi355_engine_set_release_callback
};
struct mi355_clip { ClipModel m; };
struct mi355_adapter_lora { LoraAdapter *a; };
struct mi355_context {
    Context *c;
    std::vector<const char *> prof_names;
};

static thread_local std::string t_err;
static int g_op_mmq_planes = 1, g_op_mmq_ksplit = 1;
static bool g_backend_ok = false;

static void fail(const std::string &s) { t_err = s; }

// No C++ exception may cross the C ABI (the reference's own rule for its plugin boundary, enginei.h): allocation failures
// and anything else thrown below an entry point become that entry point's error return and a last_error message.
#define MI355_GUARD(on_error, ...)                                              \
    try { __VA_ARGS__ }                                                         \
    catch (const std::bad_alloc &) { fail("out of host memory"); on_error; }    \
    catch (const std::exception &ex) { fail(std::string("internal error: ") + ex.what()); on_error; } \
    catch (...) { fail("internal error"); on_error; }

extern "C" {

int mi355_backend_init(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        fail("no HIP device visible: this backend has no CPU fallback");
        g_backend_ok = false;
        return MI355_ERR_NO_DEVICE;
    }
    g_backend_ok = true;
    return MI355_OK;
}
void mi355_backend_free(void) { g_backend_ok = false; }
int mi355_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
const char *mi355_last_error(void) {
    if (t_err.empty() && !last_error_string().empty()) return last_error_string().c_str();
    return t_err.c_str();
}
int64_t mi355_time_us(void) {
    using namespace std::chrono;
    return duration_cast<microseconds>(steady_clock::now().time_since_epoch()).count();
}
const char *mi355_print_system_info(void) {
    static std::string s;
    int n = mi355_device_count();
    s = "mi355-llama | HIP devices = " + std::to_string(n);
    if (n > 0) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, 0) == hipSuccess)
            s += std::string(" | ") + p.name + " | " + p.gcnArchName + " | CUs = " + std::to_string(p.multiProcessorCount) +
                 " | HBM = " + std::to_string(p.totalGlobalMem >> 30) + " GiB";
    }
    return s.c_str();
}

mi355_model_params mi355_model_default_params(void) {
    mi355_model_params p{};
    p.n_gpu_layers = 300; p.main_gpu = 0; p.use_mmap = 1; p.use_mlock = 0; p.tp_rank = 0; p.tp_size = 1; p.prefill_planes = -1;
    return p;
}

mi355_model *mi355_model_load_from_file(const char *path, mi355_model_params params) {
    if (!path) { fail("null path"); return nullptr; }
    if (!g_backend_ok && mi355_backend_init() != MI355_OK) return nullptr;
    if (params.n_gpu_layers <= 0) { fail("ngl=0 requested: this backend is device-only (no CPU path)"); return nullptr; }
    if (params.tp_size > 1 && (tp_size() != params.tp_size || tp_rank() != params.tp_rank)) {
        fail("tp_size > 1 needs the process's row-split group first (mi355_tp_init with the same rank / size)");
        return nullptr;
    }
    MI355_GUARD(return nullptr,
        std::string err;
        int status = 0;
        Model *m = model_load(path, params.main_gpu, err, status, params.prefill_planes, params.tp_rank, params.tp_size);
        if (!m) { fail(err); return nullptr; }
        mi355_model *h = new (std::nothrow) mi355_model;
        if (!h) { delete m; fail("out of host memory"); return nullptr; }
        h->m = m;
        return h;
    )
}
void mi355_model_free(mi355_model *model) {
    if (!model) return;
    delete model->m;
    delete model;
}
int32_t mi355_model_n_vocab(const mi355_model *m) { return m->m->hp.n_vocab; }
int32_t mi355_model_n_embd(const mi355_model *m) { return m->m->hp.n_embd; }
int32_t mi355_model_n_layer(const mi355_model *m) { return m->m->hp.n_layer; }
int32_t mi355_model_n_head(const mi355_model *m) { return m->m->hp.n_head; }
int32_t mi355_model_n_head_kv(const mi355_model *m) { return m->m->hp.n_head_kv; }
int32_t mi355_model_n_ctx_train(const mi355_model *m) { return m->m->hp.n_ctx_train; }
uint64_t mi355_model_size(const mi355_model *m) { return m->m->file_tensor_bytes; }
uint64_t mi355_model_cpu_buffer(const mi355_model *m) { return m->m->host_bytes; }
uint64_t mi355_model_other_buffer(const mi355_model *m) { return m->m->device_bytes; }
uint64_t mi355_model_bytes_per_token(const mi355_model *m) { return m->m->bytes_per_token; }
uint64_t mi355_model_planes_bytes(const mi355_model *m) { return m->m->planes_bytes; }
const char *mi355_model_desc(const mi355_model *m) { return m->m->desc.c_str(); }
int mi355_model_meta_str(const mi355_model *m, const char *key, char *buf, size_t buf_size) {
    if (!m || !key || !buf || !buf_size) return 0;
    const GGUFValue *v = m->m->file->find(key);
    if (!v || v->type == GV_ARR) return 0;
    std::string s;
    if (v->type == GV_STR) s = v->s;
    else if (v->type == GV_F32 || v->type == GV_F64) { char t[64]; snprintf(t, sizeof t, "%g", v->f); s = t; }
    else if (v->type == GV_BOOL) s = v->u ? "true" : "false";
    else s = std::to_string((long long)(int64_t)v->u);
    snprintf(buf, buf_size, "%s", s.c_str());
    return 1;
}

mi355_context_params mi355_context_default_params(void) {
    mi355_context_params p{};
    p.n_ctx = 2048; p.n_batch = 2048; p.n_ubatch = 512; p.n_seq_max = 1;
    p.type_k = MI355_TYPE_F16; p.type_v = MI355_TYPE_F16; p.flash_attn = 1; p.embeddings = 0; p.use_graphs = 1; p.logits_to_host = 1;
    return p;
}

mi355_context *mi355_context_new(mi355_model *model, mi355_context_params params) {
    if (!model) { fail("null model"); return nullptr; }
    ContextParams cp;
    cp.n_ctx = params.n_ctx; cp.n_batch = params.n_batch; cp.n_ubatch = params.n_ubatch ? params.n_ubatch : params.n_batch;
    cp.n_seq_max = params.n_seq_max ? params.n_seq_max : 1;
    cp.type_k = params.type_k; cp.type_v = params.type_v;
    cp.flash_attn = params.flash_attn != 0 || params.type_k != MI355_TYPE_F16 || params.type_v != MI355_TYPE_F16;
    cp.embeddings = params.embeddings != 0;
    cp.use_graphs = params.use_graphs != 0;
    cp.logits_to_host = params.logits_to_host != 0;
    if (cp.n_ctx == 0 || cp.n_batch == 0 || cp.n_seq_max > 64) { fail("bad context parameters (n_ctx and n_batch must be positive, n_seq_max at most 64)"); return nullptr; }
    MI355_GUARD(return nullptr,
        std::unique_ptr<Context> c(new Context(model->m, cp));
        std::string err;
        if (!c->init(err)) { fail(err); return nullptr; }
        mi355_context *h = new mi355_context{c.get(), {}};
        c.release();
        return h;
    )
}
void mi355_context_free(mi355_context *ctx) {
    if (!ctx) return;
    delete ctx->c;
    delete ctx;
}
uint32_t mi355_n_ctx(const mi355_context *ctx) { return ctx->c->cp.n_ctx; }
uint32_t mi355_n_batch(const mi355_context *ctx) { return ctx->c->cp.n_batch; }
uint32_t mi355_n_ubatch(const mi355_context *ctx) { return ctx->c->cp.n_ubatch; }
uint64_t mi355_context_device_bytes(const mi355_context *ctx) { return ctx->c->device_bytes; }

mi355_batch mi355_batch_init(int32_t n_tokens, int32_t embd, int32_t n_seq_max) {
    mi355_batch b{};
    // llama_batch_init: embd != 0 allocates n_tokens x embd floats and NO token array
    if (embd > 0) b.embd = (float *)calloc((size_t)n_tokens * (size_t)embd, sizeof(float));
    else b.token = (mi355_token *)calloc((size_t)n_tokens, sizeof(mi355_token));
    b.pos = (mi355_pos *)calloc((size_t)n_tokens, sizeof(mi355_pos));
    b.n_seq_id = (int32_t *)calloc((size_t)n_tokens, sizeof(int32_t));
    b.seq_id = (mi355_seq_id **)calloc((size_t)n_tokens + 1, sizeof(mi355_seq_id *));
    for (int i = 0; i < n_tokens; i++) b.seq_id[i] = (mi355_seq_id *)calloc((size_t)(n_seq_max > 0 ? n_seq_max : 1), sizeof(mi355_seq_id));
    b.seq_id[n_tokens] = nullptr;
    b.logits = (int8_t *)calloc((size_t)n_tokens, 1);
    return b;
}
void mi355_batch_free(mi355_batch b) {
    free(b.token); free(b.embd); free(b.pos); free(b.n_seq_id); free(b.logits);
    if (b.seq_id) {
        for (int i = 0; b.seq_id[i]; i++) free(b.seq_id[i]);
        free(b.seq_id);
    }
}

int32_t mi355_decode(mi355_context *ctx, mi355_batch batch) {
    if (!ctx) return MI355_ERR_ARG;
    MI355_GUARD(return MI355_ERR_ARG,
        // (llama_batch: token ids, or - image embeddings - rows of n_embd floats in embd with token == NULL)
        const int rc = ctx->c->decode(batch.n_tokens, batch.embd ? nullptr : batch.token, batch.pos, batch.n_seq_id, batch.seq_id, batch.logits, batch.embd);
        if (rc < 0) fail(ctx->c->last_error);
        return rc;
    )
}
// n greedy single-token steps in one call: llama_decode, the logits row made host-visible (llama_get_logits_ith), the arg-max fed back - the inner loop of a
// generation as the reference's C++ slot loop runs it, without a scripting caller's per-call overhead in every step
int32_t mi355_greedy_steps(mi355_context *ctx, mi355_token first, mi355_pos pos0, mi355_seq_id seq, int32_t n, mi355_token *out_tokens) {
    if (!ctx || n < 0) return MI355_ERR_ARG;
    MI355_GUARD(return MI355_ERR_ARG,
        int32_t tok = first, one = 1, sid = seq;
        int32_t *sp = &sid;
        const int8_t flag = 1;
        for (int32_t i = 0; i < n; i++) {
            int32_t pos = pos0 + i;
            const int rc = ctx->c->decode(1, &tok, &pos, &one, &sp, &flag);
            if (rc != 0) { if (rc < 0) fail(ctx->c->last_error); return i; }
            if (!ctx->c->logits_ith(0)) { fail("no logits row"); return i; }
            tok = ctx->c->argmax_ith(0);
            if (tok < 0) { fail(ctx->c->last_error.empty() ? "arg-max failed" : ctx->c->last_error); return i; }
            if (out_tokens) out_tokens[i] = tok;
        }
        return n;
    )
}
float *mi355_get_logits_ith(mi355_context *ctx, int32_t i) {
    float *p = ctx->c->logits_ith(i);
    if (!p) fail(ctx->c->last_error.empty() ? "no logits for that batch row" : ctx->c->last_error);      // (why: a step an in-kernel wait gave up on says so here)
    return p;
}
int32_t mi355_get_argmax_ith(mi355_context *ctx, int32_t i) { return ctx->c->argmax_ith(i); }

// ---- speculative decoding: the device-side decisions (csrc/spec.hip) and the round built on them
static int no_context(const char *what) {
    if (!g_backend_ok && mi355_backend_init() != MI355_OK) return MI355_ERR_NO_DEVICE;
    fail(std::string(what) + ": null context or argument");
    return MI355_ERR_ARG;
}
int32_t mi355_get_argmax_prob_ith(mi355_context *ctx, int32_t i, float *p) {
    if (!ctx) return no_context("get_argmax_prob_ith");
    MI355_GUARD(return MI355_ERR_ARG,
        const int32_t t = ctx->c->argmax_prob_ith(i, p);
        if (t < 0) fail(ctx->c->last_error.empty() ? "arg-max failed" : ctx->c->last_error);
        return t;
    )
}
int32_t mi355_spec_verify(mi355_context *ctx, int32_t n_groups, const int32_t *group_start, const mi355_token *draft, mi355_token *ids_out, int32_t *n_accept_out) {
    if (!ctx) return no_context("spec_verify");
    MI355_GUARD(return MI355_ERR_ARG,
        const int r = ctx->c->spec_verify(n_groups, group_start, draft, ids_out, n_accept_out);
        if (r < 0) { fail(ctx->c->last_error.empty() ? "spec_verify failed" : ctx->c->last_error); return MI355_ERR_ARG; }
        return r;
    )
}
// ---- perplexity and KL divergence (csrc/logprob.hip)
int32_t mi355_get_token_logprobs(mi355_context *ctx, int32_t n, const int32_t *batch_rows, const mi355_token *targets, float *logprob_out, int32_t *rank_out) {
    if (!ctx) return no_context("get_token_logprobs");
    MI355_GUARD(return MI355_ERR_ARG,
        const int r = ctx->c->token_logprobs(n, batch_rows, targets, logprob_out, rank_out);
        if (r < 0) { fail(ctx->c->last_error.empty() ? "token_logprobs failed" : ctx->c->last_error); return MI355_ERR_ARG; }
        return r;
    )
}
int32_t mi355_logits_kl(mi355_context *ctx, mi355_context *ctx_base, int32_t n, const int32_t *rows_base, const int32_t *rows, float *kl_out, int32_t *same_top_out) {
    if (!ctx || !ctx_base) return no_context("logits_kl");
    MI355_GUARD(return MI355_ERR_ARG,
        const int r = ctx->c->logits_kl(*ctx_base->c, n, rows_base, rows, kl_out, same_top_out);
        if (r < 0) { fail(ctx->c->last_error.empty() ? "logits_kl failed" : ctx->c->last_error); return MI355_ERR_ARG; }
        return r;
    )
}
// ---- importance matrix (Context::imatrix_*)
int32_t mi355_imatrix_begin(mi355_context *ctx, int32_t process_output) {
    if (!ctx) return no_context("imatrix_begin");
    MI355_GUARD(return MI355_ERR_ARG,
        if (ctx->c->imatrix_begin(process_output != 0) != 0) { fail(ctx->c->last_error.empty() ? "imatrix_begin failed" : ctx->c->last_error); return MI355_ERR_ARG; }
        return MI355_OK;
    )
}
int32_t mi355_imatrix_end(mi355_context *ctx) {
    if (!ctx) return no_context("imatrix_end");
    MI355_GUARD(return MI355_ERR_ARG,
        if (ctx->c->imatrix_end() != 0) { fail(ctx->c->last_error); return MI355_ERR_ARG; }
        return MI355_OK;
    )
}
int32_t mi355_imatrix_clear(mi355_context *ctx) {
    if (!ctx) return no_context("imatrix_clear");
    MI355_GUARD(return MI355_ERR_ARG,
        if (ctx->c->imatrix_clear() != 0) { fail(ctx->c->last_error); return MI355_ERR_ARG; }
        return MI355_OK;
    )
}
int32_t mi355_imatrix_n_entries(const mi355_context *ctx) { return ctx ? ctx->c->imatrix_n_entries() : 0; }
int32_t mi355_imatrix_entry(const mi355_context *ctx, int32_t i, char *name_buf, int32_t cap, int32_t *ne0, int32_t *n_mat) {
    if (!ctx) return no_context("imatrix_entry");
    MI355_GUARD(return MI355_ERR_ARG,
        std::string name;
        int k = 0, m = 0;
        if (!ctx->c->imatrix_entry(i, name, k, m)) { fail("imatrix_entry: no entry " + std::to_string(i)); return MI355_ERR_ARG; }
        if (name_buf && cap > 0) { snprintf(name_buf, (size_t)cap, "%s", name.c_str()); }
        if (ne0) *ne0 = k;
        if (n_mat) *n_mat = m;
        return (int32_t)name.size();
    )
}
int32_t mi355_imatrix_get(mi355_context *ctx, int32_t i, float *sum2, int32_t *counts) {
    if (!ctx) return no_context("imatrix_get");
    MI355_GUARD(return MI355_ERR_ARG,
        if (ctx->c->imatrix_get(i, sum2, counts) != 0) { fail(ctx->c->last_error.empty() ? "imatrix_get failed" : ctx->c->last_error); return MI355_ERR_ARG; }
        return MI355_OK;
    )
}
namespace {
struct PplCallback { mi355_ppl_callback cb; void *user; };
void ppl_stats_out(const Context::PplStats &s, mi355_ppl_stats *o) {
    o->n_chunks = s.n_chunks; o->count = s.count; o->top1 = s.top1; o->dead = s.dead; o->same_top = s.same_top;
    o->has_base = s.has_base; o->stopped = s.stopped;
    o->nll = s.nll; o->nll2 = s.nll2; o->nll_base = s.nll_base; o->nll2_base = s.nll2_base; o->kl = s.kl; o->kl2 = s.kl2;
}
int ppl_trampoline(const Context::PplStats &s, void *p) {
    const PplCallback *c = static_cast<const PplCallback *>(p);
    mi355_ppl_stats o;
    ppl_stats_out(s, &o);
    return c->cb(&o, c->user);
}
}  // namespace
int32_t mi355_perplexity(mi355_context *ctx, mi355_context *ctx_base, const mi355_token *tokens, int64_t n_tokens, int32_t n_chunk, mi355_token bos, mi355_seq_id seq,
                         float *logprob_out, float *kl_out, mi355_ppl_callback cb, void *user, mi355_ppl_stats *stats) {
    if (!ctx || !tokens || !stats) return no_context("perplexity");
    MI355_GUARD(return MI355_ERR_ARG,
        PplCallback pc{cb, user};
        Context::PplStats st;
        const int r = ctx->c->perplexity(tokens, n_tokens, n_chunk, bos, seq, ctx_base ? ctx_base->c : nullptr, logprob_out, kl_out, cb ? ppl_trampoline : nullptr, &pc, st);
        ppl_stats_out(st, stats);
        if (r < 0) { fail(ctx->c->last_error.empty() ? "perplexity failed" : ctx->c->last_error); return MI355_ERR_ARG; }
        return MI355_OK;
    )
}
// The greedy loop with a draft model beside the target (the round: DESIGN.md §4.9).  `p` is the position of `last`, the newest emitted token, which neither
// context has decoded yet; the draft context holds [0, dpos) and `pend` is what it has still to see (positions dpos .. p).
int32_t mi355_speculative_steps(mi355_context *ctx_tgt, mi355_context *ctx_dft, mi355_token first, mi355_pos pos0, mi355_seq_id seq, int32_t n, int32_t n_max,
                                int32_t n_min, float p_min, mi355_token *out_tokens, int64_t *stats) {
    if (!ctx_tgt || !ctx_dft) return no_context("speculative_steps");
    if (n < 0 || pos0 < 0 || n_max < 1 || n_max > SPEC_MAX_DRAFT || n_min < 0 || ctx_tgt == ctx_dft) {
        fail("speculative_steps: n >= 0, pos0 >= 0, 1 <= n_max <= 16, n_min >= 0 and two different contexts"); return MI355_ERR_ARG;
    }
    if (ctx_tgt->c->model->hp.n_vocab != ctx_dft->c->model->hp.n_vocab) { fail("speculative_steps: the two models have different vocabulary sizes"); return MI355_ERR_ARG; }
    MI355_GUARD(return MI355_ERR_ARG,
        Context *T = ctx_tgt->c, *D = ctx_dft->c;
        int64_t st[4] = {0, 0, 0, 0};                                  // rounds, drafted, accepted, plain steps
        if (stats) memcpy(stats, st, sizeof st);
        int32_t sid = seq;
        int32_t *sp = &sid;
        int32_t n_seq[SPEC_MAX_DRAFT + 2], pos[SPEC_MAX_DRAFT + 2], toks[SPEC_MAX_DRAFT + 2], ids[SPEC_MAX_DRAFT + 1], draft[SPEC_MAX_DRAFT + 1];
        int32_t *seqs[SPEC_MAX_DRAFT + 2];
        int8_t flags[SPEC_MAX_DRAFT + 2];
        for (int j = 0; j < SPEC_MAX_DRAFT + 2; j++) { n_seq[j] = 1; seqs[j] = sp; }
        auto decode = [&](Context *c, int cnt, bool all_rows) -> bool {
            for (int j = 0; j < cnt; j++) flags[j] = all_rows || j == cnt - 1;
            const int rc = c->decode(cnt, toks, pos, n_seq, seqs, flags);
            if (rc != 0) fail(rc < 0 ? c->last_error : std::string("speculative_steps: no KV cells left for the batch"));
            return rc == 0;
        };
        const int room = (int)std::min(T->cp.n_ctx / T->cp.n_seq_max, D->cp.n_ctx / D->cp.n_seq_max);
        std::vector<int32_t> pend;
        int32_t last = first, p = pos0, dpos = pos0, done = 0;
        while (done < n) {
            const int k_cap = std::max(0, std::min((int)n_max, room - p - 1));
            int k = 0;
            pend.push_back(last);                                      // positions dpos .. p
            if (k_cap > 0) {
                // 1. the draft context catches up; 2. it drafts while it is sure enough
                if (pend.size() > (size_t)SPEC_MAX_DRAFT + 2) { fail("speculative_steps: the draft context fell behind"); break; }
                for (size_t j = 0; j < pend.size(); j++) { toks[j] = pend[j]; pos[j] = dpos + (int32_t)j; }
                if (!decode(D, (int)pend.size(), false)) break;
                dpos = p + 1;
                pend.clear();
                bool bad = false;
                for (;;) {
                    float pr = 0.0f;
                    const int32_t t = D->argmax_prob_ith(-1, &pr);
                    if (t < 0) { fail(D->last_error); bad = true; break; }
                    if (pr < p_min) break;
                    draft[k++] = t;
                    if (k == k_cap) break;
                    toks[0] = t; pos[0] = dpos;
                    if (!decode(D, 1, false)) { bad = true; break; }
                    dpos++;
                }
                if (bad) break;
                if (k < n_min) k = 0;                                  // 3. too short a draft is not worth a batch
            }
            // 4. the target decodes the last token and the drafts as one batch, every row flagged
            int a = 0;
            toks[0] = last; pos[0] = p;
            for (int j = 0; j < k; j++) { toks[j + 1] = draft[j]; pos[j + 1] = p + 1 + j; }
            if (!decode(T, k + 1, true)) break;
            if (k > 0) {
                const int32_t gs[2] = {0, k + 1};
                draft[k] = -1;
                if (T->spec_verify(1, gs, draft, ids, &a) < 0) { fail(T->last_error); break; }
            } else {
                ids[0] = T->argmax_ith(0);
                if (ids[0] < 0) { fail(T->last_error.empty() ? "arg-max failed" : T->last_error); break; }
                st[3]++;
            }
            // 5. emit ids[0 .. a], cut at n; 6. both caches keep what was emitted and nothing behind it
            const int m = std::min(a + 1, (int)(n - done));
            st[0]++; st[1] += k; st[2] += m - 1;                      // accepted: the drafts that were emitted (the cut of the last round takes its share)
            for (int j = 0; j < m; j++) if (out_tokens) out_tokens[done + j] = ids[j];
            done += m;
            const int32_t keep = p + m;                                // the new last token's position: not decoded anywhere yet
            if (k + 1 > m) T->kv_seq_rm(seq, keep, -1);               // (a context that holds nothing there is left alone: its cell table stays clean)
            if (dpos > keep) { D->kv_seq_rm(seq, keep, -1); dpos = keep; }
            for (int32_t q = dpos + (int32_t)pend.size(); q < keep; q++) pend.push_back(q == p ? last : ids[q - p - 1]);     // accepted drafts the draft context has not decoded
            last = ids[m - 1];
            p = keep;
        }
        if (stats) memcpy(stats, st, sizeof st);
        return done;
    )
}
int32_t mi355_get_topk_ith(mi355_context *ctx, int32_t i, int32_t k, int32_t n_adj, const int32_t *adj_tok, const float *adj_bias, const int32_t *adj_count,
                           float penalty_repeat, float penalty_freq, float penalty_present, int32_t *toks_out, float *logits_out) {
    if (!ctx || !toks_out || !logits_out || n_adj < 0 || n_adj > TOPK_MAX_ADJ || (n_adj > 0 && (!adj_tok || !adj_bias || !adj_count))) { fail("bad arguments"); return -1; }
    TopkAdj a{};
    a.n = n_adj; a.repeat = penalty_repeat; a.freq = penalty_freq; a.present = penalty_present;
    for (int j = 0; j < n_adj; j++) { a.tok[j] = adj_tok[j]; a.bias[j] = adj_bias[j]; a.cnt[j] = adj_count[j]; }
    const int r = ctx->c->topk_ith(i, k, a, toks_out, logits_out);
    if (r < 0) fail(ctx->c->last_error.empty() ? "top-k failed" : ctx->c->last_error);
    return r;
}
int64_t mi355_debug_mega_steps(const mi355_context *ctx) { return ctx->c->mega_steps; }
int64_t mi355_debug_engine_steps(const mi355_context *ctx) { return ctx->c->engine_steps; }
int64_t mi355_debug_fused_skipped_steps(const mi355_context *ctx) { return ctx->c->fused_skipped_steps; }
int64_t mi355_debug_qkv_attn_launches(const mi355_context *ctx) { return ctx->c->qkv_attn_launches; }
int64_t mi355_debug_qkv_attn_plan(int32_t type_q, int32_t type_k, int32_t type_v, int32_t type_o, int32_t n_embd, int32_t n_head, int32_t n_head_kv, int32_t head_dim,
                                  int32_t type_kv, int32_t n_kv, int32_t *slots_out) {
    int slots = 0;
    const size_t lds = qkv_attn_out_plan_lds(type_q, type_k, type_v, type_o, n_embd, n_head, n_head_kv, head_dim, type_kv, n_kv, &slots);
    if (slots_out) *slots_out = slots;
    return (int64_t)lds;
}
void mi355_set_embeddings(mi355_context *ctx, int32_t enabled) { ctx->c->embeddings_enabled = enabled != 0 || ctx->c->model->hp.encoder; }
float *mi355_get_embeddings_ith(mi355_context *ctx, int32_t i) { return ctx->c->embeddings_ith(i); }
void mi355_synchronize(mi355_context *ctx) { ctx->c->synchronize(); }

// ---- LoRA adapters (llama_adapter_lora_init / llama_set_adapter_lora and their kin)
mi355_adapter_lora *mi355_adapter_lora_init(mi355_model *model, const char *path) {
    if (!model || !path) { fail("null model or path"); return nullptr; }
    MI355_GUARD(return nullptr,
        std::string err;
        int status = 0;
        LoraAdapter *a = lora_load(model->m, path, err, status);
        if (!a) { fail(err); return nullptr; }
        mi355_adapter_lora *h = new (std::nothrow) mi355_adapter_lora;
        if (!h) { lora_free(a); fail("out of host memory"); return nullptr; }
        h->a = a;
        return h;
    )
}
void mi355_adapter_lora_free(mi355_adapter_lora *adapter) {
    if (!adapter) return;
    lora_free(adapter->a);
    delete adapter;
}
float mi355_adapter_lora_alpha(const mi355_adapter_lora *adapter) { return adapter ? adapter->a->alpha : 0.0f; }
int32_t mi355_adapter_lora_n_pairs(const mi355_adapter_lora *adapter) { return adapter ? (int32_t)adapter->a->pairs.size() : 0; }
int32_t mi355_set_adapter_lora(mi355_context *ctx, mi355_adapter_lora *adapter, float scale) {
    if (!ctx || !adapter) { fail("null context or adapter"); return MI355_ERR_ARG; }
    MI355_GUARD(return MI355_ERR_ARG,
        if (ctx->c->set_adapter_lora(adapter->a, scale) != 0) { fail(ctx->c->last_error); return MI355_ERR_ARG; }
        return MI355_OK;
    )
}
int32_t mi355_rm_adapter_lora(mi355_context *ctx, mi355_adapter_lora *adapter) {
    if (!ctx || !adapter) { fail("null context or adapter"); return MI355_ERR_ARG; }
    if (ctx->c->rm_adapter_lora(adapter->a) != 0) { fail(ctx->c->last_error); return -1; }
    return MI355_OK;
}
void mi355_clear_adapter_lora(mi355_context *ctx) { if (ctx) ctx->c->clear_adapter_lora(); }

// ---- LLaVA image path (host/clip.h)
mi355_clip *mi355_clip_model_load(const char *path, int32_t main_gpu) {
    if (!path) { fail("clip_model_load: no path"); return nullptr; }
    MI355_GUARD(return nullptr,
        std::unique_ptr<mi355_clip> c(new mi355_clip);
        const std::string err = c->m.load(path, main_gpu < 0 ? 0 : main_gpu);
        if (!err.empty()) { fail(err); return nullptr; }
        return c.release();
    )
}
void mi355_clip_free(mi355_clip *clip) { delete clip; }
int32_t mi355_clip_n_mmproj_embd(const mi355_clip *clip) { return clip ? clip->m.proj_dim : 0; }
int32_t mi355_clip_n_patches(const mi355_clip *clip) { return clip ? clip->m.n_patches() : 0; }
int32_t mi355_clip_image_size(const mi355_clip *clip) { return clip ? clip->m.image_size : 0; }
int32_t mi355_clip_max_image_rows(const mi355_clip *clip) { return clip ? clip->m.max_image_rows() : 0; }
int32_t mi355_clip_image_preprocess_grid(const mi355_clip *clip, const uint8_t *rgb, int32_t nx, int32_t ny, float *out, size_t out_floats, int32_t *grid_w, int32_t *grid_h) {
    if (!clip || !rgb || !out || nx <= 0 || ny <= 0) { fail("clip_image_preprocess_grid: bad arguments"); return MI355_ERR_ARG; }
    MI355_GUARD(return MI355_ERR_ARG,
        ClipImageU8 img;
        img.nx = nx; img.ny = ny; img.rgb.assign(rgb, rgb + (size_t)3 * nx * ny);
        std::vector<std::vector<float>> imgs;
        int gw = 0, gh = 0;
        clip->m.preprocess_all(img, imgs, gw, gh);
        const size_t per = (size_t)3 * clip->m.image_size * clip->m.image_size;
        if (out_floats < per * imgs.size()) { fail("clip_image_preprocess_grid: output buffer too small"); return MI355_ERR_ARG; }
        for (size_t i = 0; i < imgs.size(); i++) memcpy(out + i * per, imgs[i].data(), per * sizeof(float));
        if (grid_w) *grid_w = gw;
        if (grid_h) *grid_h = gh;
        return (int32_t)imgs.size();
    )
}
int32_t mi355_clip_image_load_from_bytes(const uint8_t *bytes, size_t n_bytes, int32_t *nx, int32_t *ny, uint8_t *rgb_out, size_t rgb_cap) {
    MI355_GUARD(return MI355_ERR_ARG,
        ClipImageU8 img;
        const std::string err = clip_image_load_from_bytes(bytes, n_bytes, img);
        if (!err.empty()) { fail(err); return MI355_ERR_ARG; }
        if (nx) *nx = img.nx;
        if (ny) *ny = img.ny;
        if (rgb_out) {
            if (rgb_cap < img.rgb.size()) { fail("clip_image_load_from_bytes: rgb_cap too small"); return MI355_ERR_ARG; }
            memcpy(rgb_out, img.rgb.data(), img.rgb.size());
        }
        return MI355_OK;
    )
}
int32_t mi355_clip_image_preprocess(const mi355_clip *clip, const uint8_t *rgb, int32_t nx, int32_t ny, float *out) {
    if (!clip || !rgb || !out || nx <= 0 || ny <= 0) { fail("clip_image_preprocess: bad arguments"); return MI355_ERR_ARG; }
    MI355_GUARD(return MI355_ERR_ARG,
        ClipImageU8 img;
        img.nx = nx; img.ny = ny; img.rgb.assign(rgb, rgb + (size_t)3 * nx * ny);
        std::vector<float> f;
        clip->m.preprocess(img, f);
        memcpy(out, f.data(), f.size() * sizeof(float));
        return MI355_OK;
    )
}
int32_t mi355_clip_image_encode(mi355_clip *clip, const float *img, float *out) {
    if (!clip || !img || !out) { fail("clip_image_encode: bad arguments"); return MI355_ERR_ARG; }
    MI355_GUARD(return MI355_ERR_ARG,
        const std::string err = clip->m.encode(img, out);
        if (!err.empty()) { fail(err); return MI355_ERR_ARG; }
        return MI355_OK;
    )
}
int32_t mi355_llava_image_embed_from_bytes(mi355_clip *clip, const uint8_t *bytes, size_t n_bytes, float *out, size_t out_floats) {
    if (!clip || !bytes || !out) { fail("llava_image_embed: bad arguments"); return MI355_ERR_ARG; }
    MI355_GUARD(return MI355_ERR_ARG,
        ClipImageU8 img;
        std::string err = clip_image_load_from_bytes(bytes, n_bytes, img);
        if (!err.empty()) { fail(err); return MI355_ERR_ARG; }
        std::vector<float> rows;
        int n_rows = 0;
        err = clip->m.embed(img, rows, n_rows);
        if (!err.empty()) { fail(err); return MI355_ERR_ARG; }
        if (out_floats < rows.size()) { fail("llava_image_embed: output buffer too small (" + std::to_string(n_rows) + " rows; size it with mi355_clip_max_image_rows)"); return MI355_ERR_ARG; }
        memcpy(out, rows.data(), rows.size() * sizeof(float));
        return n_rows;
    )
}

void mi355_kv_cache_clear(mi355_context *ctx) { ctx->c->kv_clear(); }
// sequence ids index a 64-bit mask per cell: anything outside [0, 64) is refused here (seq < 0 = "every sequence" only
// where upstream defines it: seq_rm)
static bool seq_in_range(const mi355_context *, mi355_seq_id seq) { return seq >= 0 && seq < 64; }
int32_t mi355_kv_cache_seq_rm(mi355_context *ctx, mi355_seq_id seq, mi355_pos p0, mi355_pos p1) {
    if (!ctx) return 0;
    if (seq >= 0 && !seq_in_range(ctx, seq)) { fail("seq_rm: sequence id out of range"); return 0; }
    return ctx->c->kv_seq_rm(seq, p0, p1) ? 1 : 0;
}
void mi355_kv_cache_seq_cp(mi355_context *ctx, mi355_seq_id src, mi355_seq_id dst, mi355_pos p0, mi355_pos p1) {
    if (!ctx) return;
    if (!seq_in_range(ctx, src) || !seq_in_range(ctx, dst)) { fail("seq_cp: sequence id out of range"); return; }
    ctx->c->kv_seq_cp(src, dst, p0, p1);
}
void mi355_kv_cache_seq_add(mi355_context *ctx, mi355_seq_id seq, mi355_pos p0, mi355_pos p1, mi355_pos delta) {
    if (!ctx) return;
    if (!seq_in_range(ctx, seq)) { fail("seq_add: sequence id out of range"); return; }
    ctx->c->kv_seq_add(seq, p0, p1, delta);
}
int32_t mi355_kv_cache_used_cells(const mi355_context *ctx) { return ctx->c->kv_used_cells(); }

// ---- a sequence's KV state (llama_state_seq_*): the blob is Context::state_seq_get's (host/runtime.h); 0 = refused, the reason in mi355_last_error
size_t mi355_state_seq_get_size(mi355_context *ctx, mi355_seq_id seq) {
    if (!ctx || !ctx->c) { fail("state_seq_get_size: null context"); return 0; }
    return ctx->c->state_seq_size(seq);
}
size_t mi355_state_seq_get_data(mi355_context *ctx, uint8_t *dst, size_t cap, mi355_seq_id seq) {
    if (!ctx || !ctx->c) { fail("state_seq_get_data: null context"); return 0; }
    MI355_GUARD(return 0,
        const size_t n = ctx->c->state_seq_get(seq, dst, cap);
        if (!n) fail(ctx->c->last_error);
        return n;
    )
}
size_t mi355_state_seq_set_data(mi355_context *ctx, const uint8_t *src, size_t len, mi355_seq_id dst) {
    if (!ctx || !ctx->c) { fail("state_seq_set_data: null context"); return 0; }
    MI355_GUARD(return 0,
        const size_t n = ctx->c->state_seq_set(dst, src, len);
        if (!n) fail(ctx->c->last_error);
        return n;
    )
}
// the file: 4 words {magic "M5KF", version, n_tokens, 0}, the blob's length (8 bytes), the tokens, the blob
static const uint32_t STATE_FILE_MAGIC = 0x464b354du, STATE_FILE_VERSION = 1;
static const size_t STATE_FILE_HEADER = 24;
size_t mi355_state_seq_save_file(mi355_context *ctx, const char *path, mi355_seq_id seq, const mi355_token *tokens, size_t n_tokens) {
    if (!ctx || !ctx->c) { fail("state_seq_save_file: null context"); return 0; }
    if (!path || (n_tokens && !tokens) || n_tokens > 0x7fffffffu) { fail("state_seq_save_file: null path / tokens"); return 0; }
    MI355_GUARD(return 0,
        const size_t blob = ctx->c->state_seq_size(seq);
        std::vector<uint8_t> buf(STATE_FILE_HEADER + n_tokens * 4 + blob);
        const size_t got = blob ? ctx->c->state_seq_get(seq, buf.data() + STATE_FILE_HEADER + n_tokens * 4, blob) : 0;
        if (!got) { fail(blob ? ctx->c->last_error : std::string("state_seq_save_file: this context has no sequence state")); return 0; }
        const uint32_t head[4] = {STATE_FILE_MAGIC, STATE_FILE_VERSION, (uint32_t)n_tokens, 0};
        const uint64_t blob_len = got;
        memcpy(buf.data(), head, 16);
        memcpy(buf.data() + 16, &blob_len, 8);
        if (n_tokens) memcpy(buf.data() + STATE_FILE_HEADER, tokens, n_tokens * 4);
        buf.resize(STATE_FILE_HEADER + n_tokens * 4 + got);
        // a reader never sees a half-written file: the bytes go to a temporary name beside the target, which is then renamed over it
        const std::string tmp = std::string(path) + ".tmp";
        FILE *f = fopen(tmp.c_str(), "wb");
        if (!f) { fail("state_seq_save_file: cannot create " + tmp); return 0; }
        const bool ok = fwrite(buf.data(), 1, buf.size(), f) == buf.size();
        if (fclose(f) != 0 || !ok) { remove(tmp.c_str()); fail("state_seq_save_file: write to " + tmp + " failed"); return 0; }
        if (rename(tmp.c_str(), path) != 0) { remove(tmp.c_str()); fail(std::string("state_seq_save_file: cannot rename to ") + path); return 0; }
        return buf.size();
    )
}
size_t mi355_state_seq_load_file(mi355_context *ctx, const char *path, mi355_seq_id dst_seq, mi355_token *tokens_out, size_t cap, size_t *n_tokens_out) {
    if (!ctx || !ctx->c) { fail("state_seq_load_file: null context"); return 0; }
    if (!path) { fail("state_seq_load_file: null path"); return 0; }
    if (n_tokens_out) *n_tokens_out = 0;
    MI355_GUARD(return 0,
        FILE *f = fopen(path, "rb");
        if (!f) { fail(std::string("state_seq_load_file: cannot open ") + path); return 0; }
        struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
        uint8_t hb[STATE_FILE_HEADER];
        if (fread(hb, 1, sizeof hb, f) != sizeof hb) { fail("state_seq_load_file: truncated file: no header"); return 0; }
        uint32_t head[4];
        uint64_t blob_len = 0;
        memcpy(head, hb, 16); memcpy(&blob_len, hb + 16, 8);
        if (head[0] != STATE_FILE_MAGIC) { fail("state_seq_load_file: magic mismatch: the file has " + std::to_string(head[0]) + ", a state file has " + std::to_string(STATE_FILE_MAGIC)); return 0; }
        if (head[1] != STATE_FILE_VERSION) { fail("state_seq_load_file: version mismatch: the file has " + std::to_string(head[1]) + ", this build reads " + std::to_string(STATE_FILE_VERSION)); return 0; }
        const size_t n_tok = head[2];
        if (fseek(f, 0, SEEK_END) != 0) { fail("state_seq_load_file: seek failed"); return 0; }
        const long flen = ftell(f);
        const uint64_t want = (uint64_t)STATE_FILE_HEADER + (uint64_t)n_tok * 4 + blob_len;
        if (flen < 0 || (uint64_t)flen != want) { fail("state_seq_load_file: file length mismatch: the file has " + std::to_string(flen) + " bytes, its header asks for " + std::to_string(want)); return 0; }
        if (n_tok > cap || (n_tok && !tokens_out)) { fail("state_seq_load_file: token buffer of " + std::to_string(cap) + ", the file holds " + std::to_string(n_tok)); return 0; }
        if (fseek(f, (long)STATE_FILE_HEADER, SEEK_SET) != 0) { fail("state_seq_load_file: seek failed"); return 0; }
        std::vector<mi355_token> toks(n_tok);
        std::vector<uint8_t> blob((size_t)blob_len);
        if ((n_tok && fread(toks.data(), 4, n_tok, f) != n_tok) || fread(blob.data(), 1, blob.size(), f) != blob.size()) { fail("state_seq_load_file: read failed"); return 0; }
        if (!ctx->c->state_seq_set(dst_seq, blob.data(), blob.size())) { fail(ctx->c->last_error); return 0; }
        if (n_tok) memcpy(tokens_out, toks.data(), n_tok * 4);
        if (n_tokens_out) *n_tokens_out = n_tok;
        return (size_t)want;
    )
}
void mi355_debug_state_seq_timing(mi355_context *ctx, float out_ms[3]) {
    if (!ctx || !ctx->c) return;
    ctx->c->state_timing = true;
    if (out_ms) { out_ms[0] = ctx->c->state_ms_pack; out_ms[1] = ctx->c->state_ms_copy; out_ms[2] = ctx->c->state_ms_unpack; }
}

void mi355_debug_enable_taps(mi355_context *ctx, int32_t enabled) { ctx->c->set_debug_taps(enabled != 0); }
int32_t mi355_debug_layer_out(mi355_context *ctx, int32_t il, float *dst, size_t dst_floats) { return ctx->c->debug_layer_out(il, dst, dst_floats); }

void mi355_profile_enable(mi355_context *ctx, int32_t enabled) { ctx->c->set_profile(enabled != 0); }
int32_t mi355_profile_last_decode(mi355_context *ctx, const char **names, float *us, int32_t cap) {
    const auto &p = ctx->c->last_profile();
    int n = 0;
    for (const auto &e : p) {
        if (n >= cap) break;
        names[n] = e.name.c_str();
        us[n] = e.us;
        n++;
    }
    return n;
}
int mi355_debug_force_moe_ids(mi355_context *ctx, const int32_t *ids, int32_t n_layer, int32_t n_tokens, int32_t k) {
    if (!ctx || !ctx->c) return MI355_ERR_ARG;
    if (ctx->c->force_moe_ids(ids, n_layer, n_tokens, k) != 0) { fail(ctx->c->last_error.empty() ? "force_moe_ids failed" : ctx->c->last_error); return MI355_ERR_ARG; }
    return MI355_OK;
}
double mi355_bench_weight_sweep(mi355_context *ctx, int iters, uint64_t *bytes_per_sweep) { return ctx->c->bench_weight_sweep(iters, bytes_per_sweep); }
double mi355_bench_weight_sweep2(mi355_context *ctx, int iters, uint64_t *bytes_per_sweep, int32_t *launches_per_sweep) {
    int n = 0;
    const double us = ctx->c->bench_weight_sweep(iters, bytes_per_sweep, &n);
    if (launches_per_sweep) *launches_per_sweep = n;
    return us;
}

}  // extern "C"

// ------------------------------------------------------------------ per-op wrappers
namespace {
struct DevBuf {
    void *p = nullptr;
    size_t n = 0;
    explicit DevBuf(size_t bytes) : n(bytes) { if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) p = nullptr; else (void)hipMemset(p, 0, bytes ? bytes : 16); }
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <typename T> T *as() { return reinterpret_cast<T *>(p); }
    bool up(const void *src, size_t bytes) { return p && hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) == hipSuccess; }
    bool down(void *dst, size_t bytes) { return p && hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost) == hipSuccess; }
};
bool need_device() {
    if (g_backend_ok) return true;
    return mi355_backend_init() == MI355_OK;
}
struct ActBufs {
    DevBuf qs, d, bs, qs0, d0;
    ActQuant q;
    ActBufs(size_t K, size_t T) : qs(T * K), d(T * (K / 256 + 1) * 4), bs(T * (K / 16 + 1) * 2), qs0(T * K), d0(T * (K / 32 + 1) * 2) {
        q.qs = qs.as<int8_t>(); q.d = d.as<float>(); q.bsums = bs.as<int16_t>(); q.qs0 = qs0.as<int8_t>(); q.d0 = d0.as<uint16_t>();
    }
    bool ok() const { return qs.p && d.p && bs.p && qs0.p && d0.p; }
};
// The quantiser hooks give the planes one row more than they ask for, filled with a pattern first and checked afterwards: a kernel that walks past the end
// of a row (its partial last 256-group) or of the last row lands there.
const int Q80_GUARD = 0xA5;
bool q80_guard_set(ActBufs &ab, size_t n, size_t rows) {
    return hipMemset(ab.q.qs0 + rows * n, Q80_GUARD, n) == hipSuccess && hipMemset(ab.q.d0 + rows * (n / 32), Q80_GUARD, (n / 32) * 2) == hipSuccess;
}
bool q80_guard_intact(ActBufs &ab, size_t n, size_t rows) {
    std::vector<uint8_t> g(n + (n / 32) * 2);
    if (hipMemcpy(g.data(), ab.q.qs0 + rows * n, n, hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (hipMemcpy(g.data() + n, ab.q.d0 + rows * (n / 32), (n / 32) * 2, hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (uint8_t b : g) if (b != Q80_GUARD) return false;
    return true;
}
int hip_fail(hipError_t e, const char *what) {
    fail(std::string(what) + ": " + hipGetErrorString(e));
    return MI355_ERR_HIP;
}
// ggml-layout cache rows [n_cells][G * D] (f16, q8_0 or q4_0 blocks) -> the device's head-major planes: codes [G][n_cells][...] and f16 block scales
void cache_planes_from_rows(int type, const void *rows, int G, int D, int n_cells, std::vector<uint8_t> &codes, std::vector<uint16_t> &scales) {
    const uint8_t *src = (const uint8_t *)rows;
    const size_t rb = ggml_row_bytes(type, (int64_t)G * D);
    if (type == T_F16) {
        codes.resize((size_t)G * n_cells * D * 2);
        for (int c = 0; c < n_cells; c++)
            for (int g = 0; g < G; g++) memcpy(&codes[(((size_t)g * n_cells + c) * D) * 2], src + (size_t)c * rb + (size_t)g * D * 2, (size_t)D * 2);
    } else {
        const int bb = ggml_block_bytes(type), cb = bb - 2;
        codes.resize((size_t)G * n_cells * (D / 32) * cb);
        scales.resize((size_t)G * n_cells * (D / 32));
        for (int c = 0; c < n_cells; c++)
            for (int g = 0; g < G; g++)
                for (int b = 0; b < D / 32; b++) {
                    const uint8_t *blk = src + (size_t)c * rb + ((size_t)g * (D / 32) + b) * bb;
                    memcpy(&scales[((size_t)g * n_cells + c) * (D / 32) + b], blk, 2);
                    memcpy(&codes[(((size_t)g * n_cells + c) * (D / 32) + b) * cb], blk + 2, (size_t)cb);
                }
    }
}
// ... and back: the cache row at `cell` in ggml block layout (dst: G * D elements' worth; null: nothing to do)
bool cache_row_to_ggml(int type, DevBuf &codes, DevBuf &scales, int G, int D, int n_cells, int cell, void *dst) {
    if (!dst) return true;
    uint8_t *o8 = (uint8_t *)dst;
    for (int g = 0; g < G; g++) {
        const size_t rowi = (size_t)g * n_cells + cell;
        if (type == T_F16) {
            if (hipMemcpy(o8 + (size_t)g * D * 2, (uint8_t *)codes.p + rowi * D * 2, (size_t)D * 2, hipMemcpyDeviceToHost) != hipSuccess) return false;
        } else {
            const int bb = ggml_block_bytes(type), cb = bb - 2;
            std::vector<uint8_t> c((size_t)(D / 32) * cb);
            std::vector<uint16_t> sc((size_t)D / 32);
            if (hipMemcpy(c.data(), (uint8_t *)codes.p + rowi * (D / 32) * cb, c.size(), hipMemcpyDeviceToHost) != hipSuccess) return false;
            if (hipMemcpy(sc.data(), (uint8_t *)scales.p + rowi * (D / 32) * 2, sc.size() * 2, hipMemcpyDeviceToHost) != hipSuccess) return false;
            for (int b = 0; b < D / 32; b++) {
                uint8_t *blk = o8 + ((size_t)g * (D / 32) + b) * bb;
                memcpy(blk, &sc[(size_t)b], 2);
                memcpy(blk + 2, &c[(size_t)b * cb], (size_t)cb);
            }
        }
    }
    return true;
}
// ... and the whole cache: every cell of the device's planes back into ggml-layout rows [n_cells][G * D] (the inverse of cache_planes_from_rows)
bool cache_rows_from_planes(int type, DevBuf &codes, DevBuf &scales, int G, int D, int n_cells, void *rows) {
    uint8_t *dst = (uint8_t *)rows;
    const size_t rb = ggml_row_bytes(type, (int64_t)G * D);
    const int cb = type == T_F16 ? 64 : type == T_Q8_0 ? 32 : 16, bb = type == T_F16 ? 64 : cb + 2;   // code bytes of 32 elements; bytes of their ggml block
    std::vector<uint8_t> c((size_t)G * n_cells * (D / 32) * cb);
    std::vector<uint16_t> sc(type == T_F16 ? 0 : (size_t)G * n_cells * (D / 32));
    if (!codes.down(c.data(), c.size()) || (!sc.empty() && !scales.down(sc.data(), sc.size() * 2))) return false;
    for (int cell = 0; cell < n_cells; cell++)
        for (int g = 0; g < G; g++)
            for (int b = 0; b < D / 32; b++) {
                const size_t bi = ((size_t)g * n_cells + cell) * (D / 32) + b;
                uint8_t *blk = dst + (size_t)cell * rb + ((size_t)g * (D / 32) + b) * bb;
                if (type != T_F16) { memcpy(blk, &sc[bi], 2); blk += 2; }
                memcpy(blk, &c[bi * cb], (size_t)cb);
            }
    return true;
}
// The per-token chunk lists of a test entry's step, built by the function the runtime builds its own with (host/attn_chunks.h) and laid out as Context keeps
// them: [64][stride] lists, then [64] counts.  grid: the chunk slots the launch gets (a.splits).
struct ChunkLists {
    std::unique_ptr<DevBuf> dev;
    int stride = 0, lmax = 0, grid = 0;
    bool make(int n_kv, int n_cells, const int32_t *cell_pos, const uint64_t *cell_seq, const int32_t *tok_seq, int T) {
        stride = (n_cells + ATTN_CHUNK_CELLS - 1) / ATTN_CHUNK_CELLS;
        std::vector<int32_t> h((size_t)64 * (stride + 1), 0);
        lmax = build_attn_chunk_lists(n_kv, n_cells, [&](int i, int32_t &p, uint64_t &m) { p = cell_pos[i]; m = cell_seq[i]; }, tok_seq, T, stride, h.data(),
                                      h.data() + (size_t)64 * stride);
        grid = attn_chunk_grid(lmax, stride);
        dev.reset(new DevBuf(h.size() * 4));
        return dev->up(h.data(), h.size() * 4);
    }
    void apply(AttnArgs &a) const {
        a.tok_chunks = dev->as<int32_t>(); a.tok_nchunks = dev->as<int32_t>() + (size_t)64 * stride; a.chunk_stride = stride;
        a.splits = grid;
    }
};
int op_ffn_gate_up_nib32(int32_t type, const void *Wg, const void *Wu, int64_t N, int64_t K, const float *x, int64_t T, float *y);
}  // namespace

extern "C" double hbm_read_probe(size_t bytes, int iters);

extern "C" {

int mi355_op_quantize_act(int32_t act_type, const float *x, int64_t n, int64_t rows, void *out_blocks) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    // Q8_0: any whole number of 32-element blocks; a Q8_K block is 256 elements
    if ((act_type != MI355_TYPE_Q8_K && act_type != MI355_TYPE_Q8_0) || n <= 0 || rows <= 0 || n % (act_type == MI355_TYPE_Q8_K ? 256 : 32)) { fail("bad args"); return MI355_ERR_ARG; }
    DevBuf dx((size_t)n * rows * 4);
    ActBufs ab((size_t)n, (size_t)rows + 1);
    const size_t ob = act_type == MI355_TYPE_Q8_K ? ggml_row_bytes(T_Q8_K, n) * rows : ggml_row_bytes(T_Q8_0, n) * rows;
    DevBuf dout(ob);
    if (!dx.up(x, (size_t)n * rows * 4) || !ab.ok() || !dout.p || !q80_guard_set(ab, (size_t)n, (size_t)rows)) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    hipError_t e = launch_quantize(dx.as<float>(), (int)n, (int)rows, ab.q, act_type == MI355_TYPE_Q8_K, act_type == MI355_TYPE_Q8_0, nullptr);
    if (e == hipSuccess) e = act_type == MI355_TYPE_Q8_K ? launch_pack_q8k_blocks(ab.q, (int)n, (int)rows, dout.as<uint8_t>(), nullptr)
                                                         : launch_pack_q80_blocks(ab.q, (int)n, (int)rows, dout.as<uint8_t>(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "quantize_act");
    if (act_type == MI355_TYPE_Q8_0 && !q80_guard_intact(ab, (size_t)n, (size_t)rows)) { fail("quantize_act: the quantiser wrote past the last row"); return MI355_ERR_HIP; }
    return dout.down(out_blocks, ob) ? MI355_OK : MI355_ERR_HIP;
}

// RMSNorm * weight and the Q8_0 quantisation of its rows in one launch, as a layer's norm_quant step runs it: the per-row kernel, from 32 rows on the wide
// prompt-batch one.  out_blocks: T rows of n / 32 ggml block_q8_0; y_f32 (optional): the f32 rows the blocks were made from.  n: any multiple of 32.
int mi355_op_rms_norm_quant(const float *x, const float *w, int64_t n, int64_t T, float eps, float *y_f32, void *out_blocks) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!x || !w || !out_blocks || n <= 0 || T <= 0 || n % 32) { fail("bad args"); return MI355_ERR_ARG; }
    DevBuf dx((size_t)n * T * 4), dw((size_t)n * 4), dy((size_t)n * T * 4), dout(ggml_row_bytes(T_Q8_0, n) * T);
    ActBufs ab((size_t)n, (size_t)T + 1);
    if (!dx.up(x, (size_t)n * T * 4) || !dw.up(w, (size_t)n * 4) || !dy.p || !dout.p || !ab.ok() || !q80_guard_set(ab, (size_t)n, (size_t)T)) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    hipError_t e = launch_rmsnorm_quant(dx.as<float>(), dw.as<float>(), (int)n, (int)T, eps, y_f32 ? dy.as<float>() : nullptr, &ab.q, false, true, nullptr);
    if (e == hipSuccess) e = launch_pack_q80_blocks(ab.q, (int)n, (int)T, dout.as<uint8_t>(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "rms_norm_quant");
    if (!q80_guard_intact(ab, (size_t)n, (size_t)T)) { fail("rms_norm_quant: the quantiser wrote past the last row"); return MI355_ERR_HIP; }
    if (y_f32 && !dy.down(y_f32, (size_t)n * T * 4)) return MI355_ERR_HIP;
    return dout.down(out_blocks, ggml_row_bytes(T_Q8_0, n) * T) ? MI355_OK : MI355_ERR_HIP;
}

// silu(gate) * up and the Q8_0 quantisation of the result in one launch (a prompt batch's step between ffn_gate | ffn_up and ffn_down).  n: any multiple of 32.
int mi355_op_swiglu_quant(const float *gate, const float *up, int64_t n, int64_t T, void *out_blocks) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!gate || !up || !out_blocks || n <= 0 || T <= 0 || n % 32) { fail("bad args"); return MI355_ERR_ARG; }
    DevBuf dg((size_t)n * T * 4), du((size_t)n * T * 4), dout(ggml_row_bytes(T_Q8_0, n) * T);
    ActBufs ab((size_t)n, (size_t)T + 1);
    if (!dg.up(gate, (size_t)n * T * 4) || !du.up(up, (size_t)n * T * 4) || !dout.p || !ab.ok() || !q80_guard_set(ab, (size_t)n, (size_t)T)) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    hipError_t e = launch_swiglu_quant(dg.as<float>(), du.as<float>(), (int)n, (int)T, ab.q, false, true, nullptr, nullptr, nullptr);
    if (e == hipSuccess) e = launch_pack_q80_blocks(ab.q, (int)n, (int)T, dout.as<uint8_t>(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "swiglu_quant");
    if (!q80_guard_intact(ab, (size_t)n, (size_t)T)) { fail("swiglu_quant: the quantiser wrote past the last row"); return MI355_ERR_HIP; }
    return dout.down(out_blocks, ggml_row_bytes(T_Q8_0, n) * T) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_ffn_gate_up(int32_t type, const void *Wg, const void *Wu, int64_t N, int64_t K, const float *x, int64_t T, float *y) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    // the 32-element formats: any whole number of blocks (the K-quants below: their plane sets, whole 256-blocks); f16 as two products and the SwiGLU pass
    if (act_is_q80(type) || type == T_F16) return op_ffn_gate_up_nib32(type, Wg, Wu, N, K, x, T, y);
    const size_t grow = ggml_row_bytes(type, K), drow = dev_row_bytes(type, K);
    const size_t pb = mmq_planes_bytes(type, N, (int)K);
    if (!grow || K % 256 || !pb || N % 32) { fail("bad type / K / N"); return MI355_ERR_ARG; }
    if (!mmq_planes_swiglu_ok(type, type, (int)N, (int)K, (int)T)) { fail("shape does not take the SwiGLU launch (set mmq_tiles = 4 to force it)"); return MI355_ERR_ARG; }
    DevBuf wsrc(grow * N), wdev(drow * N), pg(pb), pu(pb), dx((size_t)K * T * 4), dy((size_t)N * T * 4);
    ActBufs ab((size_t)K, (size_t)T);
    if (!wsrc.p || !wdev.p || !pg.p || !pu.p || !dx.up(x, (size_t)K * T * 4) || !dy.p || !ab.ok()) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; i++) {
        if (!wsrc.up(i ? Wu : Wg, grow * N)) { fail("device copy failed"); return MI355_ERR_OOM; }
        e = launch_repack_rows(type, wsrc.as<uint8_t>(), wdev.as<uint8_t>(), K, N, nullptr);
        if (e == hipSuccess) e = launch_mmq_expand(type, wdev.as<uint8_t>(), drow, (int)N, (int)K, (i ? pu : pg).as<uint8_t>(), nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (e == hipSuccess) e = launch_quantize(dx.as<float>(), (int)K, (int)T, ab.q, true, false, nullptr);
    if (e == hipSuccess) e = launch_mmq_planes_swiglu(type, pg.as<uint8_t>(), pu.as<uint8_t>(), (int)N, (int)K, (int)T, ab.q, dy.as<float>(), (int)N, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "ffn_gate_up");
    return dy.down(y, (size_t)N * T * 4) ? MI355_OK : MI355_ERR_HIP;
}

}  // extern "C"

namespace {
int op_mul_mat(int32_t type, const void *W, int64_t N, int64_t K, const float *x, int64_t T, const float *resid, float *y, int32_t *isum, int32_t *msum) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    const size_t grow = ggml_row_bytes(type, K), drow = dev_row_bytes(type, K);
    // the K-quants, IQ4_XS, TQ1_0 and TQ2_0: whole 256-blocks; the 32-element formats and f16 take any whole number of 32-element blocks
    if (!grow || K <= 0 || ((act_is_q80(type) || type == T_F16) ? K % 32 : K % 256)) { fail("bad type / K"); return MI355_ERR_ARG; }
    DevBuf wsrc(grow * N), wdev(drow * N), dx((size_t)K * T * 4), dy((size_t)N * T * 4), dres(resid ? (size_t)N * T * 4 : 16);
    ActBufs ab((size_t)K, (size_t)T);
    if (!wsrc.up(W, grow * N) || !wdev.p || !dx.up(x, (size_t)K * T * 4) || !dy.p || !ab.ok() || !dres.p || (resid && !dres.up(resid, (size_t)N * T * 4))) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    const float *rs = resid ? dres.as<float>() : nullptr;
    hipError_t e = launch_repack_rows(type, wsrc.as<uint8_t>(), wdev.as<uint8_t>(), K, N, nullptr);
    if (e != hipSuccess) return hip_fail(e, "repack");
    const bool quant = type_is_quant(type);
    if (resid && !(quant && ((mmq_q80_applicable(type, (int)K, (int)T)) || (mmq_q80_copy_bytes(type, N, (int)K) && mmq_q80_applicable(T_Q8_0, (int)K, (int)T) && g_op_mmq_planes)))) {
        fail("resid: only the Q8_0 prompt kernel's launches take one here"); return MI355_ERR_ARG;
    }
    if (quant) {
        e = launch_quantize(dx.as<float>(), (int)K, (int)T, ab.q, !act_is_q80(type), act_is_q80(type), nullptr);
        if (e != hipSuccess) return hip_fail(e, "quantize");
        if (mmq_q80_applicable(type, (int)K, (int)T)) {
            e = launch_mmq_q80(wdev.as<uint8_t>(), drow, (int)N, (int)K, (int)T, ab.q, dy.as<float>(), (int)N, rs, nullptr);
            if (e == hipSuccess) e = hipDeviceSynchronize();
            if (e != hipSuccess) return hip_fail(e, "mmq_q80");
        } else
        if (mmq_q80_copy_bytes(type, N, (int)K) && mmq_q80_applicable(T_Q8_0, (int)K, (int)T) && g_op_mmq_planes) {   // Q4_0 / Q5_0 / IQ4_NL / Q4_1 / Q5_1 / MXFP4 prompt batches: exact Q8_0-layout copy
            DevBuf cp(mmq_q80_copy_bytes(type, N, (int)K));
            if (!cp.p) return MI355_ERR_OOM;
            e = launch_expand_q80_copy(type, wdev.as<uint8_t>(), drow, (int)N, (int)K, cp.as<uint8_t>(), nullptr);
            if (e == hipSuccess) e = launch_mmq_q80(cp.as<uint8_t>(), mmq_q80_copy_row_bytes(type, (int)K), (int)N, (int)K, (int)T, ab.q, dy.as<float>(), (int)N, rs, nullptr, mmq_q80_copy_form(type));
            if (e == hipSuccess) e = hipDeviceSynchronize();
            if (e != hipSuccess) return hip_fail(e, "mmq_q80 (copy)");
        } else
        if (g_op_mmq_ksplit && mmq_ksplit_applicable(type, (int)K, (int)T)) {
            DevBuf bh(mmq_prep_bytes((int)K, (int)T)), bl(mmq_prep_bytes((int)K, (int)T));
            if (!bh.p || !bl.p) return MI355_ERR_OOM;
            e = launch_mmq_prep(ab.q, (int)K, (int)T, bh.as<int8_t>(), bl.as<int8_t>(), nullptr);
            if (e == hipSuccess) e = launch_mmq_ksplit(type, wdev.as<uint8_t>(), drow, (int)N, (int)K, (int)T, ab.q, bh.as<int8_t>(), bl.as<int8_t>(), dy.as<float>(), (int)N, nullptr, nullptr);
            if (e == hipSuccess) e = hipDeviceSynchronize();
            if (e != hipSuccess) return hip_fail(e, "mmq_ksplit");
        } else
        if (mmq_applicable(type, (int)K, (int)T) || (type_is_planes_only(type) && T >= 32 && g_op_mmq_planes)) {   // (Q2_K / Q3_K / IQ4_XS / TQ1_0 / TQ2_0: planes only)
            DevBuf bh(mmq_prep_bytes((int)K, (int)T)), bl(mmq_prep_bytes((int)K, (int)T));
            if (!bh.p || !bl.p) return MI355_ERR_OOM;
            e = launch_mmq_prep(ab.q, (int)K, (int)T, bh.as<int8_t>(), bl.as<int8_t>(), nullptr);
            if (g_op_mmq_planes) {
                DevBuf pl(mmq_planes_bytes(type, N, (int)K));
                if (!pl.p) return MI355_ERR_OOM;
                if (e == hipSuccess) e = launch_mmq_expand(type, wdev.as<uint8_t>(), drow, (int)N, (int)K, pl.as<uint8_t>(), nullptr);
                // K-split partial sums: only tensors with few rows split (a large N x T never does, and gets no workspace)
                const size_t ws_bytes = (size_t)4 * T * N * sizeof(float) <= ((size_t)256 << 20) ? (size_t)4 * T * N * sizeof(float) : 0;
                DevBuf wsb(ws_bytes ? ws_bytes : 16);
                if (!wsb.p) return MI355_ERR_OOM;
                MMQWorkspace wsp; wsp.p = ws_bytes ? wsb.as<float>() : nullptr; wsp.bytes = ws_bytes;
                if (e == hipSuccess) e = launch_mmq_planes(type, pl.as<uint8_t>(), (int)N, (int)K, (int)T, ab.q, bh.as<int8_t>(), bl.as<int8_t>(), dy.as<float>(), (int)N, nullptr, nullptr, wsp);
                if (e == hipSuccess) e = hipDeviceSynchronize();
                if (e == hipSuccess) e = hipDeviceSynchronize();
            } else
            if (e == hipSuccess) e = launch_mmq(type, wdev.as<uint8_t>(), drow, (int)N, (int)K, (int)T, ab.q, bh.as<int8_t>(), bl.as<int8_t>(), dy.as<float>(), (int)N, nullptr, nullptr);
            if (e == hipSuccess) e = hipDeviceSynchronize();
            if (e != hipSuccess) return hip_fail(e, "mmq");
        } else
        for (int64_t t0 = 0; t0 < T;) {
            const int64_t rem = T - t0;
            const int nt = rem >= 16 ? 16 : rem >= 8 ? 8 : rem >= 4 ? 4 : rem >= 2 ? 2 : 1;
            MMVQArgs a{};
            a.n_seg = 1; a.K = (int)K; a.T = nt; a.epi = EPI_STORE;
            a.seg[0].W = wdev.as<uint8_t>(); a.seg[0].out = dy.as<float>() + t0 * N; a.seg[0].type = type; a.seg[0].n_rows = (int)N;
            a.seg[0].ld_out = (int)N; a.seg[0].row_bytes = drow;
            a.aq = ab.q.qs + t0 * K; a.ad = ab.q.d + t0 * (K / 256); a.abs = ab.q.bsums + t0 * (K / 16);
            a.aq0 = ab.q.qs0 + t0 * K; a.ad0 = ab.q.d0 + t0 * (K / 32);
            // Q4_1 / Q5_1 / MXFP4, one token: quantised in the mat-vec's prologue, as a decode step's ffn_down and head are - the weight stream takes Q8_0-activation
            // types only in that form (row pairs, single rows), the register ring with "mmvq_stream" 0; the same blocks, so the same result
            if (nt == 1 && (nib32_has_min(type) || nib32_has_e8(type)) && (K % 256) == 0) { a.fuse_mode = 2; a.nx = dx.as<float>() + t0 * K; }
            e = launch_mmvq(a, nullptr);
            if (e != hipSuccess) return hip_fail(e, "mmvq");
            t0 += nt;
        }
        if (isum && msum) {
            const int64_t nblk = act_is_q80(type) ? K / 32 : K / 256;
            DevBuf di((size_t)N * nblk * 4), dm((size_t)N * nblk * 4);
            for (int64_t t = 0; t < T; t++) {
                MMVQArgs a{};
                a.n_seg = 1; a.K = (int)K; a.T = 1; a.epi = EPI_STORE;
                a.seg[0].W = wdev.as<uint8_t>(); a.seg[0].type = type; a.seg[0].n_rows = (int)N; a.seg[0].row_bytes = drow;
                a.aq = ab.q.qs + t * K; a.ad = ab.q.d + t * (K / 256); a.abs = ab.q.bsums + t * (K / 16);
                a.aq0 = ab.q.qs0 + t * K; a.ad0 = ab.q.d0 + t * (K / 32);
                e = launch_mmvq_ints(a, di.as<int32_t>(), dm.as<int32_t>(), nullptr);
                if (e == hipSuccess) e = hipDeviceSynchronize();
                if (e != hipSuccess) return hip_fail(e, "mmvq_ints");
                di.down(isum + t * N * nblk, (size_t)N * nblk * 4);
                dm.down(msum + t * N * nblk, (size_t)N * nblk * 4);
            }
        }
    } else {
        if (type == T_BF16) {
            // (the model path's choice for a bf16 tensor: the rows rounded to bf16 once, then the matrix cores from 8 tokens on, else the weight stream)
            DevBuf xb((size_t)K * T * 2);
            if (!xb.p) return MI355_ERR_OOM;
            e = launch_f32_to_bf16(dx.as<float>(), xb.p, (size_t)K * T, nullptr);
            if (e == hipSuccess) {
                if (mmbf16_applicable(type, (int)N, (int)K, (int)T, wdev.p, xb.p, dy.p) && (N & 3) == 0)
                    e = launch_mmbf16(wdev.as<uint8_t>(), (int)N, (int)K, xb.p, (int)T, dy.as<float>(), (int)N, nullptr, nullptr, 1.0f, false, nullptr);
                else {
                    MMVBF16Args a{};
                    a.n_seg = 1; a.K = (int)K; a.epi = EPI_STORE; a.xb = xb.as<uint16_t>();
                    a.seg[0] = MMVBF16Seg{wdev.as<uint8_t>(), dy.as<float>(), nullptr, (int)N, (int)N, drow};
                    e = launch_mmv_bf16_tokens(a, (int)T, nullptr);
                }
            }
            if (e == hipSuccess) e = hipDeviceSynchronize();
            if (e != hipSuccess) return hip_fail(e, "mul_mat (bf16)");
        } else
        // (the model path's choice: batches against f16 tensors on the matrix cores, everything else one wave per row and token)
        if (mmf16_applicable(type, (int)N, (int)K, (int)T, wdev.p, dx.p, dy.p) && (N & 3) == 0)
            e = launch_mmf16(wdev.as<uint8_t>(), (int)N, (int)K, dx.as<float>(), (int)T, dy.as<float>(), (int)N, nullptr, nullptr);
        else
            e = launch_mmv_float(type, wdev.as<uint8_t>(), (int)N, (int)K, dx.as<float>(), (int)T, dy.as<float>(), (int)N, nullptr, nullptr);
        if (e != hipSuccess) return hip_fail(e, "mmv_float");
    }
    e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "mul_mat");
    return dy.down(y, (size_t)N * T * 4) ? MI355_OK : MI355_ERR_HIP;
}

// ffn_gate | ffn_up of a Q4_1 / Q5_1 / MXFP4 layer with SwiGLU, as Context::ffn_gate_up runs them: prompt batches through the two tensors' Q8_0-layout copies
// and the SwiGLU pass ("mmq_planes" 1, T >= 32), else the mat-vec with SwiGLU in its epilogue in chunks of 16, 8, 4, 2, 1 tokens
int op_ffn_gate_up_nib32(int32_t type, const void *Wg, const void *Wu, int64_t N, int64_t K, const float *x, int64_t T, float *y) {
    const size_t grow = ggml_row_bytes(type, K), drow = dev_row_bytes(type, K);
    if (!grow || K <= 0 || K % 32 || N <= 0 || T <= 0) { fail("bad type / K"); return MI355_ERR_ARG; }
    DevBuf wsrc(grow * N), wg(drow * N), wu(drow * N), dx((size_t)K * T * 4), dy((size_t)N * T * 4), du((size_t)N * T * 4);
    ActBufs ab((size_t)K, (size_t)T);
    if (!wsrc.p || !wg.p || !wu.p || !dx.up(x, (size_t)K * T * 4) || !dy.p || !du.p || !ab.ok()) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; i++) {
        if (!wsrc.up(i ? Wu : Wg, grow * N)) { fail("device copy failed"); return MI355_ERR_OOM; }
        e = launch_repack_rows(type, wsrc.as<uint8_t>(), (i ? wu : wg).as<uint8_t>(), K, N, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (type == T_F16) {                                          // (Context::ffn_dense_gate_up's float branch: two products, then SwiGLU)
        for (int i = 0; i < 2 && e == hipSuccess; i++) {
            const uint8_t *w = (i ? wu : wg).as<uint8_t>();
            float *o = (i ? du : dy).as<float>();
            if (mmf16_applicable(type, (int)N, (int)K, (int)T, w, dx.p, o) && (N & 3) == 0) e = launch_mmf16(w, (int)N, (int)K, dx.as<float>(), (int)T, o, (int)N, nullptr, nullptr);
            else e = launch_mmv_float(type, w, (int)N, (int)K, dx.as<float>(), (int)T, o, (int)N, nullptr, nullptr);
        }
        if (e == hipSuccess) e = launch_swiglu(dy.as<float>(), du.as<float>(), dy.as<float>(), N * T, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) return hip_fail(e, "ffn_gate_up (f16)");
        return dy.down(y, (size_t)N * T * 4) ? MI355_OK : MI355_ERR_HIP;
    }
    if (e == hipSuccess) e = launch_quantize(dx.as<float>(), (int)K, (int)T, ab.q, false, true, nullptr);
    if (e != hipSuccess) return hip_fail(e, "ffn_gate_up (set-up)");
    if (type == T_Q8_0 && mmq_q80_applicable(type, (int)K, (int)T)) {      // the prompt kernel on the weights themselves
        e = launch_mmq_q80(wg.as<uint8_t>(), drow, (int)N, (int)K, (int)T, ab.q, dy.as<float>(), (int)N, nullptr, nullptr);
        if (e == hipSuccess) e = launch_mmq_q80(wu.as<uint8_t>(), drow, (int)N, (int)K, (int)T, ab.q, du.as<float>(), (int)N, nullptr, nullptr);
        if (e == hipSuccess) e = launch_swiglu(dy.as<float>(), du.as<float>(), dy.as<float>(), N * T, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    } else
    if (type != T_Q8_0 && g_op_mmq_planes && mmq_q80_applicable(T_Q8_0, (int)K, (int)T)) {
        const size_t cb = mmq_q80_copy_bytes(type, N, (int)K), crow = mmq_q80_copy_row_bytes(type, (int)K);
        DevBuf cg(cb), cu(cb);
        if (!cg.p || !cu.p) return MI355_ERR_OOM;
        e = launch_expand_q80_copy(type, wg.as<uint8_t>(), drow, (int)N, (int)K, cg.as<uint8_t>(), nullptr);
        if (e == hipSuccess) e = launch_expand_q80_copy(type, wu.as<uint8_t>(), drow, (int)N, (int)K, cu.as<uint8_t>(), nullptr);
        if (e == hipSuccess) e = launch_mmq_q80(cg.as<uint8_t>(), crow, (int)N, (int)K, (int)T, ab.q, dy.as<float>(), (int)N, nullptr, nullptr, mmq_q80_copy_form(type));
        if (e == hipSuccess) e = launch_mmq_q80(cu.as<uint8_t>(), crow, (int)N, (int)K, (int)T, ab.q, du.as<float>(), (int)N, nullptr, nullptr, mmq_q80_copy_form(type));
        if (e == hipSuccess) e = launch_swiglu(dy.as<float>(), du.as<float>(), dy.as<float>(), N * T, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    } else {
        for (int64_t t0 = 0; t0 < T && e == hipSuccess;) {
            const int64_t rem = T - t0;
            const int nt = rem >= 16 ? 16 : rem >= 8 ? 8 : rem >= 4 ? 4 : rem >= 2 ? 2 : 1;
            MMVQArgs a{};
            a.n_seg = 2; a.K = (int)K; a.T = nt; a.epi = EPI_SWIGLU;
            for (int i = 0; i < 2; i++) {
                a.seg[i].W = (i ? wu : wg).as<uint8_t>(); a.seg[i].out = (i ? du : dy).as<float>() + t0 * N; a.seg[i].type = type; a.seg[i].n_rows = (int)N;
                a.seg[i].ld_out = (int)N; a.seg[i].row_bytes = drow;
            }
            a.aq0 = ab.q.qs0 + t0 * K; a.ad0 = ab.q.d0 + t0 * (K / 32);
            e = launch_mmvq(a, nullptr);
            t0 += nt;
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (e != hipSuccess) return hip_fail(e, "ffn_gate_up");
    return dy.down(y, (size_t)N * T * 4) ? MI355_OK : MI355_ERR_HIP;
}
}  // namespace

extern "C" {

int mi355_op_mul_mat(int32_t type, const void *W, int64_t N, int64_t K, const float *x, int64_t T, float *y, int32_t *isum, int32_t *msum) {
    return op_mul_mat(type, W, N, K, x, T, nullptr, y, isum, msum);
}
int mi355_op_mul_mat_add(int32_t type, const void *W, int64_t N, int64_t K, const float *x, int64_t T, const float *resid, float *y) {
    if (!resid) { fail("mul_mat_add: resid is null"); return MI355_ERR_ARG; }
    return op_mul_mat(type, W, N, K, x, T, resid, y, nullptr, nullptr);
}

// One token's mat-vec with the activation made in the launch's prologue, as a decode step's launches take it: norm_w set - RMSNorm(x) * norm_w, then Q8_0
// (fuse mode 1: Q | K | V, ffn_gate | ffn_up, the head); norm_w null - Q8_0 of x (mode 2: ffn_down).  The 32-element weight formats, K any multiple of 32 up
// to 8192.  The result has the bits of the quantiser's launch followed by mi355_op_mul_mat's.
int mi355_op_mul_mat_fused(int32_t type, const void *W, int64_t N, int64_t K, const float *x, const float *norm_w, float eps, float *y) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    const size_t grow = ggml_row_bytes(type, K), drow = dev_row_bytes(type, K);
    if (!act_is_q80(type) || !grow || !W || !x || !y || N <= 0 || K <= 0 || K % 32 || K > 8192) { fail("bad type / K"); return MI355_ERR_ARG; }
    DevBuf wsrc(grow * N), wdev(drow * N), dx((size_t)K * 4), dw((size_t)K * 4), dy((size_t)N * 4);
    if (!wsrc.up(W, grow * N) || !wdev.p || !dx.up(x, (size_t)K * 4) || !dw.p || !dy.p || (norm_w && !dw.up(norm_w, (size_t)K * 4))) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    hipError_t e = launch_repack_rows(type, wsrc.as<uint8_t>(), wdev.as<uint8_t>(), K, N, nullptr);
    MMVQArgs a{};
    a.n_seg = 1; a.K = (int)K; a.T = 1; a.epi = EPI_STORE;
    a.seg[0].W = wdev.as<uint8_t>(); a.seg[0].out = dy.as<float>(); a.seg[0].type = type; a.seg[0].n_rows = (int)N; a.seg[0].ld_out = (int)N; a.seg[0].row_bytes = drow;
    a.fuse_mode = norm_w ? 1 : 2; a.nx = dx.as<float>(); a.nw = norm_w ? dw.as<float>() : nullptr; a.neps = eps;
    if (e == hipSuccess) e = launch_mmvq(a, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "mul_mat_fused");
    return dy.down(y, (size_t)N * 4) ? MI355_OK : MI355_ERR_HIP;
}

// A decode step's mat-vec launch as the model issues it (make_seg / single_token_desc / mmvq_tokens of host/runtime.cc): up to three weight tensors over one
// activation, the epilogue, the prologue, the host copy, the selected-experts form.  Every output buffer is 0xFF bytes before the launch and comes back whole.
int mi355_op_mat_vec_step(int32_t n_seg, const int32_t *types, const void *const *W, const int64_t *N, int64_t K, const float *x, int64_t T, int32_t epi,
                          const float *resid, int32_t fuse, const float *norm_w, float eps, int32_t want_host_copy, int32_t n_sel, int32_t n_expert,
                          const int32_t *expert_ids, int64_t ld_pad, float *const *y, float *y_host, int32_t *path) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    const bool sel = n_sel > 0;
    if (n_seg < 1 || n_seg > 3 || !types || !W || !N || !x || !y || !path || K <= 0 || T < 1 || T > 17 || ld_pad < 0 || ld_pad > 64 || fuse < 0 || fuse > 2 ||
        (epi != EPI_STORE && epi != EPI_ADD && epi != EPI_SWIGLU) || (epi == EPI_ADD && (n_seg != 1 || !resid)) || (epi == EPI_SWIGLU && (n_seg != 2 || N[0] != N[1])) ||
        (fuse != 0 && T != 1) || (fuse == 1 && !norm_w) || (want_host_copy && (!y_host || T != 1)) ||
        (sel && (n_sel < 2 || n_sel > 8 || n_expert < 1 || !expert_ids || T != 1 || epi == EPI_ADD || want_host_copy || (epi == EPI_SWIGLU ? 1 : n_seg) != 1))) {
        fail("mat_vec_step: bad arguments"); return MI355_ERR_ARG;
    }
    for (int j = 0; j < n_sel; j++) if (expert_ids[j] < 0 || expert_ids[j] >= n_expert) { fail("mat_vec_step: expert id out of range"); return MI355_ERR_ARG; }
    const int64_t NE = sel ? n_expert : 1;
    const int64_t R = sel ? n_sel : T;                            // rows of every out buffer
    const int64_t XR = sel && fuse == 2 ? n_sel : T;              // rows of x: the selected experts' ffn_down quantises one row per expert
    bool need_q8k = false, need_q80 = false;
    std::vector<std::unique_ptr<DevBuf>> dw, dy;
    std::vector<DevTensor> wt((size_t)n_seg);
    for (int s = 0; s < n_seg; s++) {
        const size_t grow = ggml_row_bytes(types[s], K), drow = dev_row_bytes(types[s], K);
        if (!type_is_quant(types[s]) || !grow || N[s] < 1 || !W[s] || (!y[s] && !(epi == EPI_SWIGLU && s == 1)) || ((act_is_q80(types[s]) ? K % 32 : K % 256) != 0)) { fail("mat_vec_step: bad segment"); return MI355_ERR_ARG; }
        (act_is_q80(types[s]) ? need_q80 : need_q8k) = true;
        const int64_t rows = N[s] * NE;
        DevBuf wsrc(grow * rows);
        dw.emplace_back(new DevBuf(drow * rows));
        dy.emplace_back(new DevBuf((size_t)R * (N[s] + ld_pad) * 4));
        if (!wsrc.up(W[s], grow * rows) || !dw.back()->p || !dy.back()->p) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
        hipError_t e = launch_repack_rows(types[s], wsrc.as<uint8_t>(), dw.back()->as<uint8_t>(), K, rows, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemset(dy.back()->p, 0xFF, (size_t)R * (N[s] + ld_pad) * 4);
        if (e != hipSuccess) return hip_fail(e, "mat_vec_step (set-up)");
        DevTensor &w = wt[(size_t)s];
        w.type = types[s]; w.K = K; w.N = N[s]; w.n_expert = NE; w.data = dw.back()->as<uint8_t>(); w.row_bytes = drow; w.bytes = drow * (size_t)rows;
    }
    const int64_t ld0 = N[0] + ld_pad;
    DevBuf dx((size_t)K * XR * 4), dnw((size_t)K * 4), dres(resid ? (size_t)R * ld0 * 4 : 16), dids(sel ? (size_t)n_sel * 4 : 16);
    ActBufs ab((size_t)K, (size_t)T);
    if (!dx.up(x, (size_t)K * XR * 4) || !dnw.p || (norm_w && !dnw.up(norm_w, (size_t)K * 4)) || !dres.p || (resid && !dres.up(resid, (size_t)R * ld0 * 4)) || !dids.p ||
        (sel && !dids.up(expert_ids, (size_t)n_sel * 4)) || !ab.ok()) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    float *host = nullptr;
    if (want_host_copy) {
        if (hipHostMalloc((void **)&host, (size_t)N[0] * 4, hipHostMallocDefault) != hipSuccess) { fail("pinned alloc failed"); return MI355_ERR_OOM; }
        memset(host, 0xFF, (size_t)N[0] * 4);
    }
    hipDeviceProp_t prop;
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) set_num_cu(prop.multiProcessorCount);
    unsigned *ew = install_stream_error_word();
    hipError_t e = hipSuccess;
    if (fuse == 0) e = launch_quantize(dx.as<float>(), (int)K, (int)T, ab.q, need_q8k, need_q80, nullptr);
    MMVQTrace trace;
    const int32_t *esel = sel ? dids.as<int32_t>() : nullptr;
    MMVQSeg segs[3];
    for (int s = 0; s < n_seg; s++) segs[s] = make_seg(wt[(size_t)s], dy[(size_t)s]->as<float>(), (int)(N[s] + ld_pad), s == 0 && resid ? dres.as<float>() : nullptr, esel);
    if (e == hipSuccess) {
        if (sel) {                                                // (the two descriptions of Context::moe_selected_desc)
            MMVQArgs a = single_token_desc(n_seg, (int)K, epi, fuse, fuse ? dx.as<float>() : nullptr, fuse == 1 ? dnw.as<float>() : nullptr, fuse == 1 ? eps : 0.0f, ab.q);
            a.n_sel = n_sel; a.sel_out_stride = (int)ld0;
            if (fuse == 2) a.sel_nx_stride = (int)K;
            for (int s = 0; s < n_seg; s++) a.seg[s] = segs[s];
            trace.note(a);
            e = launch_mmvq(a, nullptr);
        } else {
            Fuse fz;
            fz.mode = fuse; fz.x = fuse ? dx.as<float>() : nullptr; fz.w = fuse == 1 ? dnw.as<float>() : nullptr; fz.eps = eps; fz.out_host = host;
            e = mmvq_tokens(segs, n_seg, (int)K, (int)T, epi, ab.q, nullptr, fz, &trace);
        }
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    int rc = MI355_OK;
    if (e != hipSuccess) rc = hip_fail(e, "mat_vec_step");
    if (rc == MI355_OK && ew && __atomic_exchange_n(ew, 0u, __ATOMIC_RELAXED)) { fail("mat_vec_step: a weight-stream kernel raised the stream error word"); rc = MI355_ERR_HIP; }
    for (int i = 0; i < 40; i++) path[i] = 0;
    for (size_t i = 0; i < trace.recs.size() && i < 5; i++) {
        const MMVQTrace::Rec &r = trace.recs[i];
        int32_t *p = path + i * 8;
        p[0] = r.T; p[1] = r.kernel;
        if (r.kernel == MMVQ_KERNEL_STREAM) { p[2] = r.form.role; p[3] = r.form.kb; p[4] = r.form.fast_ok; p[5] = r.form.down_early; p[6] = r.form.moe; p[7] = r.form.ternary; }
    }
    const int n_out = epi == EPI_SWIGLU ? 1 : n_seg;
    for (int s = 0; s < n_out && rc == MI355_OK; s++)
        if (!dy[(size_t)s]->down(y[s], (size_t)R * (N[s] + ld_pad) * 4)) rc = MI355_ERR_HIP;
    if (host) {
        if (rc == MI355_OK) memcpy(y_host, host, (size_t)N[0] * 4);
        (void)hipHostFree(host);
    }
    return rc;
}

// One mat-mul launch of a dense prompt batch or a batched decode step as the model issues it (Context::linear, linear_multi and the gate | up block of
// host/runtime.cc): the producer of the activation and of its bh / bl planes, the launcher, the epilogue, the residual in place.  Every out buffer is 0xFF bytes
// before the launch and comes back whole; a refused launch leaves them so and launches nothing.
int mi355_op_prompt_mul_mat(int32_t n_seg, const int32_t *types, const void *const *W, const int64_t *N, int64_t K, const float *x, int64_t T, int32_t epi,
                            const float *resid, int32_t in_place, int32_t prologue, const float *norm_w, float eps, int32_t form, int64_t ld_pad,
                            float *const *y, int32_t *path) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (n_seg < 1 || n_seg > 3 || !types || !W || !N || !x || !y || !path || K <= 0 || K % 256 || K > 65536 || T < 3 || T > 600 || ld_pad < 0 || ld_pad > 64) {
        fail("prompt_mul_mat: bad arguments"); return MI355_ERR_ARG;
    }
    const int n_out = epi == EPI_SWIGLU ? 1 : n_seg;
    for (int s = 0; s < n_seg; s++) if (N[s] < 1 || N[s] > (1 << 20) || !W[s] || (s < n_out && !y[s])) { fail("prompt_mul_mat: bad segment"); return MI355_ERR_ARG; }
    for (int i = 0; i < 8; i++) path[i] = 0;
    for (int s = 0; s < n_out; s++) memset(y[s], 0xFF, (size_t)T * (N[s] + ld_pad) * 4);       // what a refusal or a failure hands back
    auto refuse = [](const char *why) { fail(std::string("prompt_mul_mat: ") + why); return MI355_ERR_ARG; };
    if (epi != EPI_STORE && epi != EPI_ADD && epi != EPI_SWIGLU) return refuse("epi outside 0..2");
    if (epi == EPI_ADD && n_seg != 1) return refuse("a residual takes one tensor");
    if (epi == EPI_ADD && !resid) return refuse("epi 1 without resid");
    if (epi != EPI_ADD && (resid || in_place)) return refuse("resid / in_place without epi 1");
    if (epi == EPI_SWIGLU && (n_seg != 2 || N[0] != N[1])) return refuse("the SwiGLU pair is two tensors of one N");
    if (epi == EPI_SWIGLU && types[0] != types[1]) return refuse("the SwiGLU pair is two tensors of one type");
    if (prologue < 0 || prologue > 3 || (prologue == 1 && !norm_w)) return refuse("bad prologue");
    if (form < 0 || form > 3) return refuse("form outside 0..3");
    if (form == 3 && n_seg != 1) return refuse("the expansion on the fly takes one tensor");
    int64_t n_all = 0;
    for (int s = 0; s < n_seg; s++) {
        const int t = types[s];
        const bool kq = t == T_Q4_K || t == T_Q5_K || t == T_Q6_K, small = t == T_Q2_K || t == T_Q3_K || t == T_IQ4_XS;
        if (!kq && !(small && n_seg == 1 && (form == 0 || form == 2))) return refuse("a tensor type this launcher has no form for");
        n_all += N[s];
    }
    hipDeviceProp_t prop;
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) set_num_cu(prop.multiProcessorCount);
    // ---- device copies: rows in the device layout, the plane sets back to back in one arena (forms 0 and 2), out buffers, activation, workspace
    const bool want_planes = form == 0 || form == 2;
    size_t arena_bytes = 0;
    std::vector<size_t> poff((size_t)n_seg, 0);
    for (int s = 0; s < n_seg; s++) { poff[(size_t)s] = arena_bytes; arena_bytes += mmq_planes_bytes(types[s], N[s], (int)K); }
    DevBuf arena(want_planes ? arena_bytes : 16);
    std::vector<std::unique_ptr<DevBuf>> dw, dy;
    std::vector<DevTensor> wt((size_t)n_seg);
    const size_t ws_bytes = (size_t)4 * T * n_all * sizeof(float);     // (the K-split partial sums: up to four splits of every segment)
    DevBuf wsb(ws_bytes), dx((size_t)K * T * 4 * (prologue == 2 ? 2 : 1)), dnw((size_t)K * 4), bh(mmq_prep_bytes((int)K, (int)T)), bl(mmq_prep_bytes((int)K, (int)T));
    ActBufs ab((size_t)K, (size_t)T);
    if (!arena.p || !wsb.p || !dx.up(x, dx.n) || !dnw.p || (norm_w && !dnw.up(norm_w, (size_t)K * 4)) || !bh.p || !bl.p || !ab.ok() ||
        hipMemset(bh.p, 0xFF, bh.n) != hipSuccess || hipMemset(bl.p, 0xFF, bl.n) != hipSuccess) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    for (int s = 0; s < n_seg; s++) {
        const size_t grow = ggml_row_bytes(types[s], K), drow = dev_row_bytes(types[s], K);
        dw.emplace_back(new DevBuf(drow * N[s]));
        dy.emplace_back(new DevBuf((size_t)T * (N[s] + ld_pad) * 4));
        if (!grow || !dw.back()->p || !dy.back()->p) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
        DevTensor &w = wt[(size_t)s];
        w.type = types[s]; w.K = K; w.N = N[s]; w.n_expert = 1; w.data = dw.back()->as<uint8_t>(); w.row_bytes = drow; w.bytes = drow * (size_t)N[s];
        if (want_planes) { w.planes = arena.as<uint8_t>() + poff[(size_t)s]; w.planes_bytes = mmq_planes_bytes(types[s], N[s], (int)K); }
    }
    MMQWorkspace wsp; wsp.p = wsb.as<float>(); wsp.bytes = ws_bytes;
    // ---- which launch: the model's choice (form 0), or the launcher named; what the launcher would refuse is refused here, before anything is launched
    int rows[3], lds[3], tys[3];
    float *outs[3];
    const DevTensor *wp[3];
    for (int s = 0; s < n_seg; s++) { rows[s] = (int)N[s]; lds[s] = (int)(N[s] + ld_pad); tys[s] = types[s]; outs[s] = dy[(size_t)s]->as<float>(); wp[s] = &wt[(size_t)s]; }
    int kind = form, n_fused = n_seg;
    bool swiglu = epi == EPI_SWIGLU;
    if (form == 0) {
        const PromptMatmul pm = prompt_mul_mat_choice(epi == EPI_SWIGLU ? PM_ROLE_GATE_UP : n_seg == 1 ? PM_ROLE_ONE : PM_ROLE_MULTI, wp, n_seg, (int)K, (int)T, wsp);
        if (pm.form == PM_NONE) return refuse("the model has no MFMA launch for these tensors and this batch");
        if (epi == EPI_SWIGLU && !pm.swiglu) return refuse("the model runs SwiGLU behind this launch, in a pass of its own");
        kind = pm.form; n_fused = pm.n_fused;
    }
    MMQPlanesForm pf{};
    if (kind == PM_KSPLIT) {
        for (int s = 0; s < n_seg; s++) if (!mmq_ksplit_applicable(types[s], (int)K, (int)T)) return refuse("the K-split kernel does not take this type or batch");
    } else if (kind == PM_PLANES) {
        for (int s = 0; s < n_seg; s++) if (!mmq_applicable(types[s], (int)K, (int)T) && !(type_is_planes_only(types[s]) && T >= 32)) return refuse("the plane kernels take batches of 32 tokens and more");
        if (swiglu) {
            if (!mmq_planes_swiglu_ok(types[0], types[1], rows[0], (int)K, (int)T)) return refuse("launch_mmq_planes_swiglu does not take this shape");
            pf.kernel = MMQ_PLANES_LDS; pf.n_split = 1; pf.mixed = false;
        } else {
            if (form == 0 && n_fused < 2) n_fused = 1;              // (no two plane sets fuse: every tensor on its own, path describes the first)
            if (!mmq_planes_form(types[0], rows, n_fused, (int)K, (int)T, epi == EPI_ADD, wsp, tys, &pf)) return refuse("launch_mmq_planes_multi refuses these segments");
        }
    } else {
        if (!mmq_applicable(types[0], (int)K, (int)T)) return refuse("launch_mmq does not take this type or batch");
    }
    // ---- set-up: the rows in the device layout, their plane sets, the out buffers 0xFF
    for (int s = 0; s < n_seg; s++) {
        const size_t grow = ggml_row_bytes(types[s], K);
        DevTensor &w = wt[(size_t)s];
        DevBuf wsrc(grow * N[s]);
        if (!wsrc.up(W[s], grow * N[s])) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
        hipError_t e = launch_repack_rows(types[s], wsrc.as<uint8_t>(), w.data, K, N[s], nullptr);
        if (e == hipSuccess && want_planes) e = launch_mmq_expand(types[s], w.data, w.row_bytes, (int)N[s], (int)K, w.planes, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemset(dy[(size_t)s]->p, 0xFF, dy[(size_t)s]->n);
        if (e != hipSuccess) return hip_fail(e, "prompt_mul_mat (set-up)");
    }
    // ---- the residual: in place it sits in the out buffer, as attn_output and ffn_down have it
    const size_t rbytes = (size_t)T * (N[0] + ld_pad) * 4;
    DevBuf dres(epi == EPI_ADD && !in_place ? rbytes : 16);
    const float *rs = nullptr;
    if (epi == EPI_ADD) {
        DevBuf &rb = in_place ? *dy[0] : dres;
        if (!rb.up(resid, rbytes)) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
        rs = rb.as<float>();
    }
    // ---- the activation and its block-sum planes
    hipError_t e;
    if (prologue == 0) {
        e = launch_quantize(dx.as<float>(), (int)K, (int)T, ab.q, true, false, nullptr);
        if (e == hipSuccess) e = launch_mmq_prep(ab.q, (int)K, (int)T, bh.as<int8_t>(), bl.as<int8_t>(), nullptr);
    } else if (prologue == 1) e = launch_rmsnorm_quant(dx.as<float>(), dnw.as<float>(), (int)K, (int)T, eps, nullptr, &ab.q, true, false, nullptr, bh.as<int8_t>(), bl.as<int8_t>());
    else if (prologue == 2) e = launch_swiglu_quant(dx.as<float>(), dx.as<float>() + (size_t)T * K, (int)K, (int)T, ab.q, true, false, nullptr, bh.as<int8_t>(), bl.as<int8_t>());
    else e = launch_quantize(dx.as<float>(), (int)K, (int)T, ab.q, true, false, nullptr, bh.as<int8_t>(), bl.as<int8_t>());
    if (e != hipSuccess) return hip_fail(e, "prompt_mul_mat (activation)");
    // ---- the launch
    const int8_t *pbh = bh.as<int8_t>(), *pbl = bl.as<int8_t>();
    if (kind == PM_KSPLIT) {
        MMQSeg sg[3];
        for (int s = 0; s < n_seg; s++) sg[s] = MMQSeg{wt[(size_t)s].data, wt[(size_t)s].row_bytes, rows[s], types[s], outs[s], lds[s], s == 0 ? rs : nullptr, 0};
        e = launch_mmq_ksplit_multi(sg, n_seg, (int)K, (int)T, ab.q, pbh, pbl, swiglu, nullptr);
        path[0] = 1; path[1] = mmq_ksplit_token_tiles((int)T); path[2] = 1;
    } else if (kind == PM_PLANES && swiglu) {
        e = launch_mmq_planes_swiglu(types[0], wt[0].planes, wt[1].planes, rows[0], (int)K, (int)T, ab.q, outs[0], lds[0], nullptr);
        path[0] = pf.kernel; path[2] = 1;
    } else if (kind == PM_PLANES) {
        e = launch_mmq_planes_multi(types[0], wt[0].planes, rows, outs, lds, n_fused, (int)K, (int)T, ab.q, pbh, pbl, rs, nullptr, wsp, tys);
        for (int s = n_fused; s < n_seg && e == hipSuccess; s++)     // (form 0: the tensors the fused launch left out, each on its plane set as Context::linear_multi runs them)
            e = launch_mmq_planes(types[s], wt[(size_t)s].planes, rows[s], (int)K, (int)T, ab.q, pbh, pbl, outs[s], lds[s], nullptr, nullptr, wsp);
        path[0] = pf.kernel; path[2] = pf.n_split; path[3] = pf.mixed ? 1 : 0;
    } else {
        e = launch_mmq(types[0], wt[0].data, wt[0].row_bytes, rows[0], (int)K, (int)T, ab.q, pbh, pbl, outs[0], lds[0], rs, nullptr);
        path[0] = 5; path[2] = 1;
    }
    path[4] = swiglu ? 1 : 0; path[5] = prologue == 0 ? 1 : 0;
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "prompt_mul_mat");
    for (int s = 0; s < n_out; s++)
        if (!dy[(size_t)s]->down(y[s], (size_t)T * (N[s] + ld_pad) * 4)) return MI355_ERR_HIP;
    return MI355_OK;
}

// One producer of the MFMA kernels' activation, with Q8_K and the bh / bl planes as the model calls it; launch_mmq_prep's planes of the same rows beside them
int mi355_op_act_q8k_planes(int32_t producer, const float *x, const float *x2, const float *norm_w, float eps, int64_t n, int64_t T, void *out_blocks,
                            int8_t *out_bh, int8_t *out_bl, int8_t *prep_bh, int8_t *prep_bl, float *y_f32) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (producer < 0 || producer > 2 || !x || (producer == 1 && !norm_w) || (producer == 2 && !x2) || (producer != 1 && y_f32) || !out_blocks || !out_bh || !out_bl ||
        !prep_bh || !prep_bl || n <= 0 || n % 256 || n > (1 << 20) || T <= 0 || T > 4096) { fail("act_q8k_planes: bad arguments"); return MI355_ERR_ARG; }
    const size_t xb = (size_t)n * T * 4, pb = mmq_prep_bytes((int)n, (int)T), ob = ggml_row_bytes(T_Q8_K, n) * T;
    DevBuf dx(xb), dx2(producer == 2 ? xb : 16), dw((size_t)n * 4), dyf(y_f32 ? xb : 16), dout(ob), bh(pb), bl(pb), ph(pb), pl(pb);
    ActBufs ab((size_t)n, (size_t)T);
    if (!dx.up(x, xb) || !dx2.p || (producer == 2 && !dx2.up(x2, xb)) || !dw.p || (producer == 1 && !dw.up(norm_w, (size_t)n * 4)) || !dyf.p || !dout.p || !bh.p || !bl.p ||
        !ph.p || !pl.p || !ab.ok() || hipMemset(bh.p, 0xFF, pb) != hipSuccess || hipMemset(bl.p, 0xFF, pb) != hipSuccess) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    hipError_t e;
    if (producer == 0) e = launch_quantize(dx.as<float>(), (int)n, (int)T, ab.q, true, false, nullptr, bh.as<int8_t>(), bl.as<int8_t>());
    else if (producer == 1) e = launch_rmsnorm_quant(dx.as<float>(), dw.as<float>(), (int)n, (int)T, eps, y_f32 ? dyf.as<float>() : nullptr, &ab.q, true, false, nullptr, bh.as<int8_t>(), bl.as<int8_t>());
    else e = launch_swiglu_quant(dx.as<float>(), dx2.as<float>(), (int)n, (int)T, ab.q, true, false, nullptr, bh.as<int8_t>(), bl.as<int8_t>());
    if (e == hipSuccess) e = launch_mmq_prep(ab.q, (int)n, (int)T, ph.as<int8_t>(), pl.as<int8_t>(), nullptr);
    if (e == hipSuccess) e = launch_pack_q8k_blocks(ab.q, (int)n, (int)T, dout.as<uint8_t>(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "act_q8k_planes");
    if (y_f32 && !dyf.down(y_f32, xb)) return MI355_ERR_HIP;
    return dout.down(out_blocks, ob) && bh.down(out_bh, pb) && bl.down(out_bl, pb) && ph.down(prep_bh, pb) && pl.down(prep_bl, pb) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_f32_to_bf16(const float *x, int64_t n, uint16_t *out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (n <= 0 || n % 8) { fail("f32_to_bf16: n must be a positive multiple of 8"); return MI355_ERR_ARG; }
    DevBuf dx((size_t)n * 4), dy((size_t)n * 2);
    if (!dx.up(x, (size_t)n * 4) || !dy.p) return MI355_ERR_OOM;
    hipError_t e = launch_f32_to_bf16(dx.as<float>(), dy.p, (size_t)n, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "f32_to_bf16");
    return dy.down(out, (size_t)n * 2) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_mul_mat_bf16(int32_t n_seg, const void *const *W, const int64_t *N, int64_t K, const float *x, int64_t T, const float *const *bias, const float *resid,
                          int32_t epi, int32_t path, int32_t tokens_per_launch, int32_t use_graph, float *const *y) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (n_seg < 1 || n_seg > 3 || !W || !N || !x || !y || K < 8 || K % 8 || (path == 2 && K % 16) || T < 1 || (epi != EPI_STORE && epi != EPI_ADD && epi != EPI_SWIGLU) || path < 0 || path > 2 ||
        (epi == EPI_ADD && (n_seg != 1 || !resid)) || (epi == EPI_SWIGLU && (n_seg != 2 || N[0] != N[1])) ||
        (tokens_per_launch != 0 && tokens_per_launch != 1 && tokens_per_launch != 2 && tokens_per_launch != 4 && tokens_per_launch != 8 && tokens_per_launch != 16)) {
        fail("mul_mat_bf16: bad arguments"); return MI355_ERR_ARG;
    }
    const size_t row = (size_t)K * 2;
    const int n_out = epi == EPI_SWIGLU ? 1 : n_seg;
    std::vector<std::unique_ptr<DevBuf>> dw, db, dy;
    for (int s = 0; s < n_seg; s++) {
        if (N[s] < 1 || !W[s]) { fail("mul_mat_bf16: bad segment"); return MI355_ERR_ARG; }
        dw.emplace_back(new DevBuf(row * (size_t)N[s]));
        db.emplace_back(new DevBuf(bias && bias[s] ? (size_t)N[s] * 4 : 16));
        dy.emplace_back(new DevBuf((size_t)N[s] * T * 4));
        if (!dw.back()->up(W[s], row * (size_t)N[s]) || !dy.back()->p || !db.back()->p) return MI355_ERR_OOM;
        if (bias && bias[s] && !db.back()->up(bias[s], (size_t)N[s] * 4)) return MI355_ERR_OOM;
    }
    DevBuf dx((size_t)K * T * 4), xb((size_t)K * T * 2), dr(resid ? (size_t)N[0] * T * 4 : 16);
    if (!dx.up(x, (size_t)K * T * 4) || !xb.p || !dr.p || (resid && !dr.up(resid, (size_t)N[0] * T * 4))) return MI355_ERR_OOM;
    hipStream_t st = nullptr;
    if (hipStreamCreate(&st) != hipSuccess) return MI355_ERR_HIP;
    auto run = [&]() -> hipError_t {
        hipError_t e = launch_f32_to_bf16(dx.as<float>(), xb.p, (size_t)K * T, st);
        if (e != hipSuccess) return e;
        bool mfma = path == 2;
        if (path == 0) {                                      // the model path's choice (Context::linear_bf16)
            mfma = true;
            for (int s = 0; s < n_seg; s++) mfma = mfma && mmbf16_applicable(T_BF16, (int)N[s], (int)K, (int)T, dw[(size_t)s]->p, xb.p, dy[(size_t)s]->p) && (N[s] & 3) == 0;
        }
        if (mfma) {
            for (int s = 0; s < n_seg && e == hipSuccess; s++)
                e = launch_mmbf16(dw[(size_t)s]->as<uint8_t>(), (int)N[s], (int)K, xb.p, (int)T, dy[(size_t)s]->as<float>(), (int)N[s], epi == EPI_ADD ? dr.as<float>() : nullptr,
                                  bias && bias[s] ? db[(size_t)s]->as<float>() : nullptr, 1.0f, false, st);
            if (e == hipSuccess && epi == EPI_SWIGLU) e = launch_swiglu(dy[0]->as<float>(), dy[1]->as<float>(), dy[0]->as<float>(), (int64_t)T * N[0], st);
            return e;
        }
        MMVBF16Args a{};
        a.n_seg = n_seg; a.K = (int)K; a.epi = epi; a.resid = epi == EPI_ADD ? dr.as<float>() : nullptr; a.xb = xb.as<uint16_t>();
        for (int s = 0; s < n_seg; s++)
            a.seg[s] = MMVBF16Seg{dw[(size_t)s]->as<uint8_t>(), dy[(size_t)s]->as<float>(), bias && bias[s] ? db[(size_t)s]->as<float>() : nullptr, (int)N[s], (int)N[s], row};
        if (tokens_per_launch == 0) return launch_mmv_bf16_tokens(a, (int)T, st);
        for (int64_t t0 = 0; t0 < T && e == hipSuccess; t0 += tokens_per_launch) {       // (tests: a fixed launch width; T must be a multiple of it)
            if (T - t0 < tokens_per_launch) return hipErrorInvalidValue;
            MMVBF16Args c = a;
            c.T = tokens_per_launch; c.xb = a.xb + t0 * K;
            if (a.resid) c.resid = a.resid + t0 * N[0];
            for (int s = 0; s < n_seg; s++) c.seg[s].out = a.seg[s].out + t0 * N[s];
            e = launch_mmv_bf16(c, st);
        }
        return e;
    };
    hipError_t e = hipSuccess;
    if (use_graph) {                                          // captured once, replayed twice: what a decode step's graph does with these launches
        hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr;
        e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
        if (e == hipSuccess) {
            const hipError_t er = run();
            const hipError_t ec = hipStreamEndCapture(st, &g);
            e = er != hipSuccess ? er : ec;
        }
        if (e == hipSuccess) e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipGraphLaunch(ge, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (ge) (void)hipGraphExecDestroy(ge);
        if (g) (void)hipGraphDestroy(g);
    } else {
        e = run();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    (void)hipStreamDestroy(st);
    if (e != hipSuccess) return hip_fail(e, "mul_mat_bf16");
    for (int s = 0; s < n_out; s++)
        if (!dy[(size_t)s]->down(y[s], (size_t)N[s] * T * 4)) return MI355_ERR_HIP;
    return MI355_OK;
}

// launch_lora_delta once: out[s][t][n] += scale[s] * B[s][n] . (A[s] x[t]) for n_seg segments over the rows x [T][K]; out[s] is [T][ld_out[s]], read and written
// back whole (the columns beyond N[s] come back as they went in unless the kernel wrote there)
int mi355_op_lora_delta(int32_t n_seg, const int32_t *type, const void *const *A, const void *const *B, const int32_t *r, const int64_t *N, const float *scale,
                        const float *x, int64_t K, int64_t T, const int64_t *ld_out, float *const *out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (n_seg < 1 || n_seg > 3 || !type || !A || !B || !r || !N || !scale || !x || !ld_out || !out || K < 32 || K % 32 || K > (1 << 20) || T < 1 || T > 65536) { fail("bad args"); return MI355_ERR_ARG; }
    for (int s = 0; s < n_seg; s++)
        if ((type[s] != T_F32 && type[s] != T_F16) || r[s] < 1 || r[s] > LORA_MAX_R || N[s] < 1 || N[s] > (1 << 24) || ld_out[s] < N[s] || !A[s] || !B[s] || !out[s]) {
            fail("bad segment (F32 / F16 pairs, rank 1 .. 512, ld_out >= N)");
            return MI355_ERR_ARG;
        }
    std::vector<std::unique_ptr<DevBuf>> bufs;
    auto dev = [&](const void *src, size_t bytes) -> void * {
        bufs.emplace_back(new DevBuf(bytes));
        return bufs.back()->up(src, bytes) ? bufs.back()->p : nullptr;
    };
    LoraSeg segs[3];
    float *xd = (float *)dev(x, (size_t)T * K * 4);
    bool ok = xd != nullptr;
    for (int s = 0; s < n_seg && ok; s++) {
        const size_t es = type[s] == T_F16 ? 2 : 4;
        segs[s] = LoraSeg{dev(A[s], (size_t)r[s] * K * es), dev(B[s], (size_t)N[s] * r[s] * es), type[s], r[s], (int)N[s], scale[s],
                          (float *)dev(out[s], (size_t)T * ld_out[s] * 4), (int)ld_out[s]};
        ok = segs[s].A && segs[s].B && segs[s].out;
    }
    DevBuf scratch(lora_scratch_floats((int)T) * 4);
    if (!ok || !scratch.p) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    hipError_t e = launch_lora_delta(segs, n_seg, xd, (int)K, (int)K, (int)T, scratch.as<float>(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "lora_delta");
    for (int s = 0; s < n_seg; s++)
        if (hipMemcpy(out[s], segs[s].out, (size_t)T * ld_out[s] * 4, hipMemcpyDeviceToHost) != hipSuccess) return MI355_ERR_HIP;
    return MI355_OK;
}

int mi355_op_rms_norm_mul(const float *x, const float *w, int64_t n, int64_t T, float eps, float *y) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (n <= 0 || T <= 0 || n % 32) { fail("n must be a multiple of 32"); return MI355_ERR_ARG; }
    DevBuf dx((size_t)n * T * 4), dw((size_t)n * 4), dy((size_t)n * T * 4);
    if (!dx.up(x, (size_t)n * T * 4) || !dw.up(w, (size_t)n * 4) || !dy.p) return MI355_ERR_OOM;
    hipError_t e = launch_rmsnorm_quant(dx.as<float>(), dw.as<float>(), (int)n, (int)T, eps, dy.as<float>(), nullptr, false, false, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "rms_norm");
    return dy.down(y, (size_t)n * T * 4) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_rope(float *x, int32_t n_head, int32_t head_dim, int32_t n_rot, const int32_t *pos, int64_t T,
                  float freq_base, float freq_scale, const float *freq_factors, int32_t neox) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    const size_t nb = (size_t)T * n_head * head_dim * 4;
    DevBuf dx(nb), dp((size_t)T * 4), dff(freq_factors ? (size_t)n_rot * 2 : 16);
    if (!dx.up(x, nb) || !dp.up(pos, (size_t)T * 4)) return MI355_ERR_OOM;
    if (freq_factors) dff.up(freq_factors, (size_t)(n_rot / 2) * 4);
    RopeArgs ra{n_rot, freq_base, freq_scale, freq_factors ? dff.as<float>() : nullptr, neox};
    hipError_t e = launch_rope_inplace(dx.as<float>(), (int)T, n_head, head_dim, dp.as<int32_t>(), ra, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "rope");
    return dx.down(x, nb) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_rope_yarn(float *x, int32_t n_head, int32_t head_dim, int32_t n_rot, const int32_t *pos, int64_t T,
                       float freq_base, float freq_scale, const float *freq_factors, int32_t neox,
                       float ext_factor, float attn_factor, float corr_lo, float corr_hi) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    const size_t nb = (size_t)T * n_head * head_dim * 4;
    DevBuf dx(nb), dp((size_t)T * 4), dff(freq_factors ? (size_t)n_rot * 2 : 16);
    if (!dx.up(x, nb) || !dp.up(pos, (size_t)T * 4)) return MI355_ERR_OOM;
    if (freq_factors) dff.up(freq_factors, (size_t)(n_rot / 2) * 4);
    RopeArgs ra{n_rot, freq_base, freq_scale, freq_factors ? dff.as<float>() : nullptr, neox};
    ra.ext_factor = ext_factor; ra.attn_factor = attn_factor; ra.corr_lo = corr_lo; ra.corr_hi = corr_hi;
    hipError_t e = launch_rope_inplace(dx.as<float>(), (int)T, n_head, head_dim, dp.as<int32_t>(), ra, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "rope_yarn");
    return dx.down(x, nb) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_get_rows(int32_t type, const void *table, int64_t K, int64_t n_rows, const int32_t *ids, int64_t n_ids, float *dst) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    const size_t grow = ggml_row_bytes(type, K), drow = dev_row_bytes(type, K);
    if (!grow) return MI355_ERR_ARG;
    DevBuf src(grow * n_rows), dev(drow * n_rows), di((size_t)n_ids * 4), dd((size_t)n_ids * K * 4);
    if (!src.up(table, grow * n_rows) || !dev.p || !di.up(ids, (size_t)n_ids * 4) || !dd.p) return MI355_ERR_OOM;
    hipError_t e = launch_repack_rows(type, src.as<uint8_t>(), dev.as<uint8_t>(), K, n_rows, nullptr);
    if (e == hipSuccess) e = launch_get_rows(type, dev.as<uint8_t>(), K, di.as<int32_t>(), (int)n_ids, dd.as<float>(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "get_rows");
    return dd.down(dst, (size_t)n_ids * K * 4) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_repack_rows(int32_t type, const void *src_rows, int64_t K, int64_t n_rows, void *dst) {
    const int be = ggml_block_elems(type);
    if (be == 0 || K <= 0 || n_rows <= 0 || K % be) return MI355_ERR_ARG;
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    const size_t grow = ggml_row_bytes(type, K), drow = dev_row_bytes(type, K);
    DevBuf src(grow * n_rows), dev(drow * n_rows);
    if (!src.up(src_rows, grow * n_rows) || !dev.p) return MI355_ERR_OOM;
    hipError_t e = hipMemset(dev.p, Q80_GUARD, drow * n_rows);
    if (e == hipSuccess) e = launch_repack_rows(type, src.as<uint8_t>(), dev.as<uint8_t>(), K, n_rows, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "repack_rows");
    return dev.down(dst, drow * n_rows) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_swiglu(const float *gate, const float *up, int64_t n, float *y) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    DevBuf g((size_t)n * 4), u((size_t)n * 4), o((size_t)n * 4);
    if (!g.up(gate, (size_t)n * 4) || !u.up(up, (size_t)n * 4) || !o.p) return MI355_ERR_OOM;
    hipError_t e = launch_swiglu(g.as<float>(), u.as<float>(), o.as<float>(), n, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "swiglu");
    return o.down(y, (size_t)n * 4) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_soft_max(const float *x, const float *mask, int64_t n, int64_t rows, float scale, float *y) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    const size_t nb = (size_t)n * rows * 4;
    DevBuf dx(nb), dm(nb), dy(nb);
    if (!dx.up(x, nb) || !dy.p) return MI355_ERR_OOM;
    if (mask) dm.up(mask, nb);
    hipError_t e = launch_soft_max(dx.as<float>(), mask ? dm.as<float>() : nullptr, dy.as<float>(), (int)n, (int)rows, scale, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "soft_max");
    return dy.down(y, nb) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_moe_route(const float *logits, int64_t T, int32_t n_expert, int32_t k, int32_t *ids, float *w) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (T <= 0 || n_expert <= 0 || n_expert > 256 || k <= 0 || k > 64 || k > n_expert) { fail("moe_route: bad shape"); return MI355_ERR_ARG; }
    DevBuf dl((size_t)T * n_expert * 4), di((size_t)T * k * 4), dw((size_t)T * k * 4);
    if (!dl.up(logits, (size_t)T * n_expert * 4) || !di.p || !dw.p) return MI355_ERR_OOM;
    hipError_t e = launch_moe_route(dl.as<float>(), (int)T, n_expert, k, di.as<int32_t>(), dw.as<float>(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "moe_route");
    return di.down(ids, (size_t)T * k * 4) && dw.down(w, (size_t)T * k * 4) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_moe_router(int32_t type, const void *gate_inp, int32_t n_expert, int64_t K, const float *x, int64_t T, int32_t k, int32_t fused,
                        const int32_t *forced, float *logits, int32_t *ids, float *w) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if ((type != T_F32 && type != T_F16) || T <= 0 || K <= 0 || n_expert <= 0 || n_expert > 256 || k <= 0 || k > 64 || k > n_expert) {
        fail("moe_router: bad type or shape"); return MI355_ERR_ARG;
    }
    const size_t wb = (size_t)n_expert * K * (type == T_F32 ? 4 : 2), nl = (size_t)T * n_expert * 4, ns = (size_t)T * k * 4;
    DevBuf dW(wb), dx((size_t)T * K * 4), dl(nl), di(ns), dw(ns), df(forced ? ns : 16);
    if (!dW.up(gate_inp, wb) || !dx.up(x, (size_t)T * K * 4) || !dl.p || !di.p || !dw.p) return MI355_ERR_OOM;
    if (forced && !df.up(forced, ns)) return MI355_ERR_OOM;
    const int32_t *fd = forced ? df.as<int32_t>() : nullptr;
    // fused: the one-launch router the single-token and prompt steps take for f32 / f16 gate_inp; else mmv_float, then the selection on its logits
    hipError_t e = fused ? launch_moe_router(type, dW.as<uint8_t>(), n_expert, (int)K, dx.as<float>(), (int)T, k, dl.as<float>(), di.as<int32_t>(), dw.as<float>(), nullptr, fd)
                         : launch_mmv_float(type, dW.as<uint8_t>(), n_expert, (int)K, dx.as<float>(), (int)T, dl.as<float>(), n_expert, nullptr, nullptr);
    if (!fused && e == hipSuccess) e = launch_moe_route(dl.as<float>(), (int)T, n_expert, k, di.as<int32_t>(), dw.as<float>(), nullptr, fd);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "moe_router");
    if (logits && !dl.down(logits, nl)) return MI355_ERR_HIP;
    return di.down(ids, ns) && dw.down(w, ns) ? MI355_OK : MI355_ERR_HIP;
}

// ---- the kernels that produce indices (csrc/misc.hip), one test entry each
int mi355_op_argmax_rows(const float *x, int64_t n, const int32_t *launches, int32_t n_launch, int32_t cap_rows, int32_t *out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (n < 1 || n > INT32_MAX || n_launch < 1 || cap_rows < 1 || cap_rows > 65535) { fail("argmax_rows: bad shape"); return MI355_ERR_ARG; }
    size_t rows = 0;
    for (int i = 0; i < n_launch; i++) {
        if (launches[i] < 1 || launches[i] > cap_rows) { fail("argmax_rows: launch " + std::to_string(i) + " outside [1, cap_rows]"); return MI355_ERR_ARG; }
        rows += (size_t)launches[i];
    }
    DevBuf dx(rows * (size_t)n * 4), dout(rows * 4), ds((size_t)cap_rows * 129 * 4);      // (DevBuf zero-fills: the ticket words start at 0, once)
    if (!dx.up(x, rows * (size_t)n * 4) || !dout.p || !ds.p) return MI355_ERR_OOM;
    hipError_t e = hipSuccess;
    size_t r0 = 0;
    for (int i = 0; i < n_launch && e == hipSuccess; i++) {                               // back to back on one scratch: no synchronisation in between
        e = launch_argmax_rows(dx.as<float>() + r0 * (size_t)n, (int)n, launches[i], dout.as<int32_t>() + r0, ds.as<float>(), cap_rows, nullptr);
        r0 += (size_t)launches[i];
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "argmax_rows");
    return dout.down(out, rows * 4) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_argmax_prob_rows(const float *x, int64_t n, int32_t rows, int32_t *idx_out, float *p_out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!x || !idx_out || !p_out || n < 1 || n > SPEC_MAX_N || rows < 1 || rows > 65535) { fail("argmax_prob_rows: bad shape"); return MI355_ERR_ARG; }
    const size_t nb = (size_t)rows * (size_t)n * 4;
    DevBuf dx(nb), di((size_t)rows * 4), dp((size_t)rows * 4), ds(argmax_prob_scratch_words(rows) * 4);
    if (!dx.up(x, nb) || !di.p || !dp.p || !ds.p) return MI355_ERR_OOM;
    hipError_t e = launch_argmax_prob_rows(dx.as<float>(), (int)n, nullptr, rows, di.as<int32_t>(), dp.as<float>(), ds.as<float>(), rows, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "argmax_prob_rows");
    return di.down(idx_out, (size_t)rows * 4) && dp.down(p_out, (size_t)rows * 4) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_spec_verify(const float *logits, int64_t n, int32_t n_base_rows, const int32_t *rows, int32_t R, const int32_t *group_start, int32_t G,
                         const int32_t *draft, int32_t *ids_out, int32_t *n_accept_out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!logits || !rows || !group_start || !draft || !ids_out || !n_accept_out || n < 1 || n > SPEC_MAX_N || n_base_rows < 1 || R < 1 || R > SPEC_MAX_ROWS || G < 1 ||
        G > SPEC_MAX_GROUPS) { fail("spec_verify: bad shape (R <= 1088, G <= 64)"); return MI355_ERR_ARG; }
    for (int r = 0; r < R; r++)
        if (rows[r] < 0 || rows[r] >= n_base_rows) { fail("spec_verify: rows[" + std::to_string(r) + "] outside the base"); return MI355_ERR_ARG; }
    if (group_start[0] != 0 || group_start[G] != R) { fail("spec_verify: the groups do not cover rows 0 .. R - 1"); return MI355_ERR_ARG; }
    for (int g = 0; g < G; g++) {
        const int k1 = group_start[g + 1] - group_start[g];
        if (k1 < 1 || k1 > SPEC_MAX_DRAFT + 1) { fail("spec_verify: group " + std::to_string(g) + " outside 1 .. 17 rows"); return MI355_ERR_ARG; }
    }
    const size_t nb = (size_t)n_base_rows * (size_t)n * 4;
    DevBuf db(nb), dr((size_t)R * 4), dg((size_t)(G + 1) * 4), dd((size_t)R * 4), di((size_t)R * 4), da((size_t)G * 4), ds(spec_verify_scratch_words(R) * 4);
    if (!db.up(logits, nb) || !dr.up(rows, (size_t)R * 4) || !dg.up(group_start, (size_t)(G + 1) * 4) || !dd.up(draft, (size_t)R * 4) || !di.p || !da.p || !ds.p) return MI355_ERR_OOM;
    hipError_t e = launch_spec_verify(db.as<float>(), (int)n, dr.as<int32_t>(), R, dg.as<int32_t>(), G, dd.as<int32_t>(), di.as<int32_t>(), da.as<int32_t>(), ds.as<float>(), R,
                                      nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "spec_verify");
    return di.down(ids_out, (size_t)R * 4) && da.down(n_accept_out, (size_t)G * 4) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_token_logprob_rows(const float *base, int64_t n, int32_t n_base_rows, const int32_t *rows, const int32_t *targets, int32_t R, float *logprob_out,
                                int32_t *rank_out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!base || !targets || !logprob_out || !rank_out || n < 1 || n > SPEC_MAX_N || n_base_rows < 1 || R < 1 || R > 65535 || (!rows && R > n_base_rows)) {
        fail("token_logprob_rows: bad shape"); return MI355_ERR_ARG;
    }
    for (int r = 0; r < R; r++) {
        if (rows && (rows[r] < 0 || rows[r] >= n_base_rows)) { fail("token_logprob_rows: rows[" + std::to_string(r) + "] outside the base"); return MI355_ERR_ARG; }
        if (targets[r] < 0 || targets[r] >= n) { fail("token_logprob_rows: targets[" + std::to_string(r) + "] outside [0, n)"); return MI355_ERR_ARG; }
    }
    const size_t nb = (size_t)n_base_rows * (size_t)n * 4;
    DevBuf db(nb), dr((size_t)R * 4), dt((size_t)R * 4), dl((size_t)R * 4), dk((size_t)R * 4), ds(token_logprob_scratch_words(R) * 4);
    if (!db.up(base, nb) || (rows && !dr.up(rows, (size_t)R * 4)) || !dt.up(targets, (size_t)R * 4) || !dr.p || !dl.p || !dk.p || !ds.p) return MI355_ERR_OOM;
    hipError_t e = launch_token_logprob_rows(db.as<float>(), (int)n, rows ? dr.as<int32_t>() : nullptr, dt.as<int32_t>(), R, dl.as<float>(), dk.as<int32_t>(), ds.as<float>(),
                                             R, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "token_logprob_rows");
    return dl.down(logprob_out, (size_t)R * 4) && dk.down(rank_out, (size_t)R * 4) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_logits_kl_rows(const float *p, int32_t n_p_rows, const float *q, int32_t n_q_rows, int64_t n, const int32_t *rows_p, const int32_t *rows_q, int32_t R,
                            float *kl_out, int32_t *same_top_out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!p || !q || !kl_out || !same_top_out || n < 1 || n > SPEC_MAX_N || n_p_rows < 1 || n_q_rows < 1 || R < 1 || R > 65535 || (!rows_p && R > n_p_rows) ||
        (!rows_q && R > n_q_rows)) { fail("logits_kl_rows: bad shape"); return MI355_ERR_ARG; }
    for (int r = 0; r < R; r++)
        if ((rows_p && (rows_p[r] < 0 || rows_p[r] >= n_p_rows)) || (rows_q && (rows_q[r] < 0 || rows_q[r] >= n_q_rows))) {
            fail("logits_kl_rows: row " + std::to_string(r) + " outside its base"); return MI355_ERR_ARG;
        }
    const size_t nbp = (size_t)n_p_rows * (size_t)n * 4, nbq = (size_t)n_q_rows * (size_t)n * 4;
    DevBuf dp(nbp), dq(nbq), drp((size_t)R * 4), drq((size_t)R * 4), dk((size_t)R * 4), dt((size_t)R * 4), ds(logits_kl_scratch_words(R) * 4);
    if (!dp.up(p, nbp) || !dq.up(q, nbq) || (rows_p && !drp.up(rows_p, (size_t)R * 4)) || (rows_q && !drq.up(rows_q, (size_t)R * 4)) || !drp.p || !drq.p || !dk.p || !dt.p ||
        !ds.p) return MI355_ERR_OOM;
    hipError_t e = launch_logits_kl_rows(dp.as<float>(), dq.as<float>(), (int)n, rows_p ? drp.as<int32_t>() : nullptr, rows_q ? drq.as<int32_t>() : nullptr, R, dk.as<float>(),
                                         dt.as<int32_t>(), ds.as<float>(), R, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "logits_kl_rows");
    return dk.down(kl_out, (size_t)R * 4) && dt.down(same_top_out, (size_t)R * 4) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_imatrix_accum(const float *x, const float *x2, int64_t ld, int64_t K, int32_t R, const int32_t *row_src, int32_t n_src_rows, const int32_t *counts_per_mat,
                           int32_t n_mat, float *sum2_io, int32_t *count_io) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!x || !sum2_io || !count_io || K < 32 || (K & 31) || K > INT32_MAX / 2 || ld < K || (ld & 3) || ld > INT32_MAX / 2 || R < 1 || R > IMX_MAX_ROWS || n_src_rows < 1 ||
        n_mat < 1 || n_mat > 256 || (n_mat > 1 && !counts_per_mat) || (!row_src && R > n_src_rows)) { fail("imatrix_accum: bad shape"); return MI355_ERR_ARG; }
    for (int r = 0; row_src && r < R; r++)
        if (row_src[r] < 0 || row_src[r] >= n_src_rows) { fail("imatrix_accum: row_src[" + std::to_string(r) + "] outside the source rows"); return MI355_ERR_ARG; }
    // meta as launch_moe_group leaves it: counts | exclusive offsets | total
    std::vector<int32_t> meta;
    if (counts_per_mat) {
        meta.assign((size_t)2 * n_mat + 1, 0);
        int64_t run = 0;
        for (int m = 0; m < n_mat; m++) {
            if (counts_per_mat[m] < 0) { fail("imatrix_accum: negative count"); return MI355_ERR_ARG; }
            meta[(size_t)m] = counts_per_mat[m]; meta[(size_t)n_mat + m] = (int32_t)std::min<int64_t>(run, R);
            run += counts_per_mat[m];
        }
        if (run != R) { fail("imatrix_accum: the counts do not add up to R"); return MI355_ERR_ARG; }
        meta[(size_t)2 * n_mat] = R;
    }
    const size_t nx = (size_t)n_src_rows * (size_t)ld * 4, ns = (size_t)(n_mat + 1) * (size_t)K * 4;
    const size_t slab_floats = imatrix_scratch_floats((int)K, R, n_mat);
    DevBuf dx(nx), dx2(x2 ? nx : 16), dr((size_t)R * 4), dm(meta.empty() ? 16 : meta.size() * 4), dsum(ns), dcnt((size_t)n_mat * 4), dslab(slab_floats * 4);
    if (!dx.up(x, nx) || (x2 && !dx2.up(x2, nx)) || (row_src && !dr.up(row_src, (size_t)R * 4)) || (!meta.empty() && !dm.up(meta.data(), meta.size() * 4)) ||
        !dsum.up(sum2_io, ns) || !dcnt.up(count_io, (size_t)n_mat * 4) || !dx2.p || !dr.p || !dm.p || !dslab.p) return MI355_ERR_OOM;
    hipError_t e = launch_imatrix_accum(dx.as<float>(), x2 ? dx2.as<float>() : nullptr, (int)ld, (int)K, R, row_src ? dr.as<int32_t>() : nullptr,
                                        meta.empty() ? nullptr : dm.as<int32_t>(), n_mat, dsum.as<float>(), dcnt.as<int32_t>(), dslab.as<float>(), slab_floats, nullptr);
    if (e == hipErrorInvalidValue) { fail("imatrix_accum: the launcher refuses this shape"); return MI355_ERR_ARG; }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "imatrix_accum");
    return dsum.down(sum2_io, ns) && dcnt.down(count_io, (size_t)n_mat * 4) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_quantize_supported(int32_t dst_type) { return quantize_dst_supported(dst_type) ? 1 : 0; }

// what the last mi355_quantize_chunk of this thread spent: upload and download by the host's clock (the copies block), the launch between two events
static thread_local float t_quant_ms[3] = {-1.0f, -1.0f, -1.0f};
int mi355_quantize_last_times(float *upload_ms, float *kernel_ms, float *download_ms) {
    if (t_quant_ms[0] < 0.0f) { fail("quantize_last_times: no completed mi355_quantize_chunk on this thread"); return MI355_ERR_ARG; }
    if (upload_ms) *upload_ms = t_quant_ms[0];
    if (kernel_ms) *kernel_ms = t_quant_ms[1];
    if (download_ms) *download_ms = t_quant_ms[2];
    return MI355_OK;
}

int mi355_quantize_chunk(int32_t dst_type, int32_t src_type, const void *src, int64_t n_per_row, int64_t n_rows, const float *imatrix, void *dst) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!quantize_dst_supported(dst_type)) { fail("quantize_chunk: destination type " + std::to_string(dst_type) + " is not built"); return MI355_ERR_ARG; }
    if (!quantize_src_supported(src_type)) { fail("quantize_chunk: source type " + std::to_string(src_type) + " is not F32, F16 or BF16"); return MI355_ERR_ARG; }
    if (!src || !dst) { fail("quantize_chunk: null pointer"); return MI355_ERR_ARG; }
    if (n_rows < 1) { fail("quantize_chunk: n_rows < 1"); return MI355_ERR_ARG; }
    if (n_per_row < 1 || n_per_row % ggml_block_elems(dst_type)) {
        fail("quantize_chunk: n_per_row " + std::to_string(n_per_row) + " is not a whole number of " + ggml_type_name(dst_type) + " blocks of " +
             std::to_string(ggml_block_elems(dst_type)));
        return MI355_ERR_ARG;
    }
    if (n_rows > ((int64_t)1 << 36) / n_per_row) { fail("quantize_chunk: more than 2^36 elements in one call"); return MI355_ERR_ARG; }
    for (int64_t j = 0; imatrix && j < n_per_row; j++)
        if (!(imatrix[j] >= 0.0f) || std::isinf(imatrix[j])) { fail("quantize_chunk: imatrix[" + std::to_string(j) + "] is negative or not finite"); return MI355_ERR_ARG; }
    const size_t es = src_type == T_F32 ? 4 : 2, n = (size_t)n_per_row * (size_t)n_rows, rb = ggml_row_bytes(dst_type, n_per_row), nb = rb * (size_t)n_rows;
    DevBuf dsrc(n * es), dim((size_t)n_per_row * 4), dout(nb + rb), dflag(16);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess) { if (ev0) (void)hipEventDestroy(ev0); return MI355_ERR_HIP; }
    struct EvGuard { hipEvent_t a, b; ~EvGuard() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev_guard{ev0, ev1};
    const auto c0 = std::chrono::steady_clock::now();
    if (!dsrc.up(src, n * es) || (imatrix && !dim.up(imatrix, (size_t)n_per_row * 4)) || !dim.p || !dout.p || !dflag.p) return MI355_ERR_OOM;
    if (hipMemset(dout.as<uint8_t>() + nb, Q80_GUARD, rb) != hipSuccess) return MI355_ERR_HIP;
    const auto c1 = std::chrono::steady_clock::now();
    (void)hipEventRecord(ev0, nullptr);
    hipError_t e = launch_quantize_rows(dst_type, src_type, dsrc.p, n_per_row, n_rows, imatrix ? dim.as<float>() : nullptr, dout.p, dflag.as<int32_t>(), nullptr);
    if (e == hipErrorInvalidValue) { fail("quantize_chunk: the launcher refuses this shape"); return MI355_ERR_ARG; }
    (void)hipEventRecord(ev1, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "quantize_chunk");
    float kernel_ms = 0.0f;
    (void)hipEventElapsedTime(&kernel_ms, ev0, ev1);
    const auto c2 = std::chrono::steady_clock::now();
    int32_t flag = 0;
    std::vector<uint8_t> guard(rb);
    if (!dflag.down(&flag, 4) || hipMemcpy(guard.data(), dout.as<uint8_t>() + nb, rb, hipMemcpyDeviceToHost) != hipSuccess) return MI355_ERR_HIP;
    for (uint8_t b : guard)
        if (b != Q80_GUARD) { fail("quantize_chunk: the guard row behind the output was written"); return MI355_ERR_HIP; }
    if (flag) {                                  // which row: the host looks, the error path can afford it
        int64_t row = -1;
        for (int64_t i = 0; i < (int64_t)n && row < 0; i++) {
            uint32_t u;
            if (src_type == T_F32) memcpy(&u, (const uint8_t *)src + (size_t)i * 4, 4);
            else { uint16_t h; memcpy(&h, (const uint8_t *)src + (size_t)i * 2, 2); u = src_type == T_F16 ? ((uint32_t)(h & 0x7c00u) == 0x7c00u ? 0x7f800000u : 0u) : (uint32_t)h << 16; }
            if ((u & 0x7f800000u) == 0x7f800000u) row = i / n_per_row;
        }
        fail("quantize_chunk: row " + std::to_string(row) + " holds a non-finite value");
        return MI355_ERR_ARG;
    }
    if (!dout.down(dst, nb)) return MI355_ERR_HIP;
    const auto c3 = std::chrono::steady_clock::now();
    t_quant_ms[0] = std::chrono::duration<float, std::milli>(c1 - c0).count();
    t_quant_ms[1] = kernel_ms;
    t_quant_ms[2] = std::chrono::duration<float, std::milli>(c3 - c2).count();
    return MI355_OK;
}

int mi355_op_topk_rows(const float *base, int64_t n, int32_t n_base_rows, const int32_t *rows, int32_t n_rows, int32_t k, const int32_t *adj_n,
                       const int32_t *adj_tok, const float *adj_bias, const int32_t *adj_cnt, const float *repeat, const float *freq, const float *present,
                       uint64_t *keys_out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (n < 1 || n > INT32_MAX || n_base_rows < 1 || n_rows < 1 || n_rows > 65535) { fail("topk_rows: bad shape"); return MI355_ERR_ARG; }
    if (k < 1 || k > TOPK_MAX_K || k > n) { fail("topk_rows: k outside [1, min(n, " + std::to_string(TOPK_MAX_K) + ")]"); return MI355_ERR_ARG; }
    std::vector<TopkAdj> adjs((size_t)n_rows);
    for (int r = 0; r < n_rows; r++) {
        if (rows[r] < 0 || rows[r] >= n_base_rows) { fail("topk_rows: rows[" + std::to_string(r) + "] outside the base"); return MI355_ERR_ARG; }
        if (adj_n[r] < 0 || adj_n[r] > TOPK_MAX_ADJ) { fail("topk_rows: adj_n[" + std::to_string(r) + "] outside [0, " + std::to_string(TOPK_MAX_ADJ) + "]"); return MI355_ERR_ARG; }
        TopkAdj &a = adjs[(size_t)r];
        memset(&a, 0, sizeof a);
        a.n = adj_n[r]; a.repeat = repeat[r]; a.freq = freq[r]; a.present = present[r];
        const size_t o = (size_t)r * TOPK_MAX_ADJ;
        memcpy(a.tok, adj_tok + o, (size_t)a.n * sizeof(int)); memcpy(a.bias, adj_bias + o, (size_t)a.n * sizeof(float)); memcpy(a.cnt, adj_cnt + o, (size_t)a.n * sizeof(int));
    }
    const size_t nb = (size_t)n_base_rows * (size_t)n * 4, nk = (size_t)n_rows * TOPK_MAX_K * 8;
    DevBuf db(nb), dr((size_t)n_rows * 4), da((size_t)n_rows * sizeof(TopkAdj)), ds(topk_scratch_bytes((int)n) * (size_t)n_rows), dk(nk);
    if (!db.up(base, nb) || !dr.up(rows, (size_t)n_rows * 4) || !da.up(adjs.data(), (size_t)n_rows * sizeof(TopkAdj)) || !ds.p || !dk.p) return MI355_ERR_OOM;
    hipError_t e = launch_topk_rows(db.as<float>(), (int)n, n_rows, dr.as<int>(), k, da.as<TopkAdj>(), ds.p, dk.as<unsigned long long>(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "topk_rows");
    std::vector<uint64_t> keys((size_t)n_rows * TOPK_MAX_K);
    if (!dk.down(keys.data(), nk)) return MI355_ERR_HIP;
    for (int r = 0; r < n_rows; r++) memcpy(keys_out + (size_t)r * k, keys.data() + (size_t)r * TOPK_MAX_K, (size_t)k * 8);
    return MI355_OK;
}

int mi355_op_moe_group(const int32_t *ids, int64_t T, int32_t k, int32_t n_expert, int32_t *meta, int32_t *slot_of, int32_t *tok_of) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (n_expert < 1 || n_expert > 256) { fail("moe_group: n_expert outside [1, 256]"); return MI355_ERR_ARG; }
    if (T < 1 || k < 1 || T * (int64_t)k > 60 * 1024) { fail("moe_group: T * k outside [1, 61440]"); return MI355_ERR_ARG; }
    const size_t ns = (size_t)T * k;
    for (size_t i = 0; i < ns; i++)
        if (ids[i] < 0 || ids[i] >= n_expert) { fail("moe_group: ids[" + std::to_string(i) + "] outside [0, n_expert)"); return MI355_ERR_ARG; }
    DevBuf di(ns * 4), dm(((size_t)2 * n_expert + 1) * 4), dslot(ns * 4), dtok(ns * 4);
    if (!di.up(ids, ns * 4) || !dm.p || !dslot.p || !dtok.p) return MI355_ERR_OOM;
    hipError_t e = launch_moe_group(di.as<int32_t>(), (int)T, k, n_expert, dm.as<int32_t>(), dslot.as<int32_t>(), dtok.as<int32_t>(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "moe_group");
    return dm.down(meta, ((size_t)2 * n_expert + 1) * 4) && dslot.down(slot_of, ns * 4) && dtok.down(tok_of, ns * 4) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_moe_gather_act(const int8_t *qs, const float *d, const int16_t *bsums, const int8_t *qs0, const uint16_t *d0, int64_t T, int64_t K,
                            const int32_t *tok_of, int64_t n_rows, int8_t *qs_out, float *d_out, int16_t *bsums_out, int8_t *qs0_out, uint16_t *d0_out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (T < 1 || n_rows < 1 || K < 1 || K > INT32_MAX || n_rows > INT32_MAX) { fail("moe_gather_act: bad shape"); return MI355_ERR_ARG; }
    if (K % 256) { fail("moe_gather_act: K is not a multiple of 256"); return MI355_ERR_ARG; }
    const bool q8k = qs != nullptr, q80 = qs0 != nullptr;
    if ((!q8k && !q80) || (q8k && (!d || !bsums || !qs_out || !d_out || !bsums_out)) || (q80 && (!d0 || !qs0_out || !d0_out))) {
        fail("moe_gather_act: an activation form needs all its planes, in and out"); return MI355_ERR_ARG;
    }
    for (int64_t r = 0; r < n_rows; r++)
        if (tok_of[r] < 0 || tok_of[r] >= T) { fail("moe_gather_act: tok_of[" + std::to_string(r) + "] outside [0, T)"); return MI355_ERR_ARG; }
    // plane p: bytes per row, source rows, destination rows (+ the guard row the caller filled)
    const size_t rb[5] = {(size_t)K, (size_t)(K / 256) * 4, (size_t)(K / 16) * 2, (size_t)K, (size_t)(K / 32) * 2};
    const void *in[5] = {qs, d, bsums, qs0, d0};
    void *out[5] = {qs_out, d_out, bsums_out, qs0_out, d0_out};
    const bool on[5] = {q8k, q8k, q8k, q80, q80};
    std::unique_ptr<DevBuf> s[5], o[5];
    for (int p = 0; p < 5; p++) {
        if (!on[p]) continue;
        s[p].reset(new DevBuf(rb[p] * (size_t)T));
        o[p].reset(new DevBuf(rb[p] * (size_t)(n_rows + 1)));
        if (!s[p]->up(in[p], rb[p] * (size_t)T) || !o[p]->up(out[p], rb[p] * (size_t)(n_rows + 1))) return MI355_ERR_OOM;
    }
    DevBuf dt((size_t)n_rows * 4);
    if (!dt.up(tok_of, (size_t)n_rows * 4)) return MI355_ERR_OOM;
    ActQuant src, dst;
    if (q8k) { src.qs = s[0]->as<int8_t>(); src.d = s[1]->as<float>(); src.bsums = s[2]->as<int16_t>(); dst.qs = o[0]->as<int8_t>(); dst.d = o[1]->as<float>(); dst.bsums = o[2]->as<int16_t>(); }
    if (q80) { src.qs0 = s[3]->as<int8_t>(); src.d0 = s[4]->as<uint16_t>(); dst.qs0 = o[3]->as<int8_t>(); dst.d0 = o[4]->as<uint16_t>(); }
    hipError_t e = launch_moe_gather_act(src, dt.as<int32_t>(), (int)n_rows, (int)K, dst, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "moe_gather_act");
    for (int p = 0; p < 5; p++)
        if (on[p] && !o[p]->down(out[p], rb[p] * (size_t)(n_rows + 1))) return MI355_ERR_HIP;
    return MI355_OK;
}

int mi355_op_moe_combine(const float *x, const float *eo, const float *w, int64_t T, int32_t E, int32_t k, int32_t grouped, const int32_t *slot_of, float *y_out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (T < 1 || E < 1 || k < 1 || T * (int64_t)E > INT32_MAX || T * (int64_t)k > INT32_MAX) { fail("moe_combine: bad shape"); return MI355_ERR_ARG; }
    if (grouped && !slot_of) { fail("moe_combine: the grouped form needs slot_of"); return MI355_ERR_ARG; }
    const size_t ns = (size_t)T * k, nx = (size_t)T * E * 4;
    if (grouped)
        for (size_t i = 0; i < ns; i++)
            if (slot_of[i] < 0 || (size_t)slot_of[i] >= ns) { fail("moe_combine: slot_of[" + std::to_string(i) + "] outside [0, T * k)"); return MI355_ERR_ARG; }
    DevBuf dx(nx), de(nx * (size_t)k), dw(ns * 4), dslot(ns * 4);
    if (!dx.up(x, nx) || !de.up(eo, nx * (size_t)k) || !dw.up(w, ns * 4) || !dslot.p) return MI355_ERR_OOM;
    if (grouped && !dslot.up(slot_of, ns * 4)) return MI355_ERR_OOM;
    hipError_t e = grouped ? launch_moe_scatter_combine(dx.as<float>(), de.as<float>(), dw.as<float>(), dslot.as<int32_t>(), (int)T, E, k, nullptr)
                           : launch_moe_combine(dx.as<float>(), de.as<float>(), dw.as<float>(), (int)T, E, k, (size_t)T * E, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "moe_combine");
    return dx.down(y_out, nx) ? MI355_OK : MI355_ERR_HIP;
}

// One grouped-expert launch of a prompt batch as Context::moe_grouped_planes / moe_grouped_q80 issue it (host/runtime.cc): the weights expanded expert by expert
// at the loader's stride (expand_prefill_planes), the grouped rows quantised, meta in moe_group_kernel's layout, rows_max = R.  Every out buffer is 0xFF bytes
// before the launch and comes back whole, guard rows included.
int mi355_op_moe_mul_mat_grouped(int32_t type, int32_t form, const void *W0, const void *W1, int32_t n_expert, int64_t N, int64_t K, const float *x,
                                 const int32_t *counts, int64_t R, int64_t ld_out, int64_t guard_rows, float *y0, float *y1) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    const bool planes = form == 0 || form == 1, two_w = form == 1 || form == 3, two_y = form == 3;
    if (form < 0 || form > 3 || !W0 || (two_w && !W1) || !x || !counts || !y0 || (two_y && !y1) || n_expert < 1 || n_expert > 256 || N < 1 || K < 1 || R < 1 ||
        R > 60 * 1024 || N > INT32_MAX || K > INT32_MAX || ld_out < N || ld_out > INT32_MAX || guard_rows < 0 || guard_rows > 1024) {
        fail("moe_mul_mat_grouped: bad arguments"); return MI355_ERR_ARG;
    }
    if (planes ? !mmq_planes_moe_ok(type, (int)N, (int)K) : !mmq_q80_moe_ok(type, (int)N, (int)K)) {
        fail(planes ? "moe_mul_mat_grouped: the grouped plane launch takes Q4_K / Q5_K / Q6_K / IQ4_XS / TQ1_0 / TQ2_0, N % 128 == 0, K % 256 == 0"
                    : "moe_mul_mat_grouped: the grouped Q8_0-copy launch takes MXFP4, N % 128 == 0, K % 32 == 0, 32 <= K <= 16384");
        return MI355_ERR_ARG;
    }
    std::vector<int32_t> meta((size_t)2 * n_expert + 1);
    int64_t sum = 0;
    for (int e = 0; e < n_expert; e++) {
        if (counts[e] < 0) { fail("moe_mul_mat_grouped: counts[" + std::to_string(e) + "] is negative"); return MI355_ERR_ARG; }
        meta[(size_t)e] = counts[e];
        meta[(size_t)n_expert + e] = (int32_t)sum;
        sum += counts[e];
        if (sum > R) break;
    }
    if (sum != R) { fail("moe_mul_mat_grouped: the counts do not add up to R"); return MI355_ERR_ARG; }
    meta[(size_t)2 * n_expert] = (int32_t)R;
    const size_t grow = ggml_row_bytes(type, K), drow = dev_row_bytes(type, K);
    const size_t pb = planes ? mmq_planes_bytes(type, N, (int)K) : mmq_q80_copy_bytes(type, N, (int)K);
    const size_t stride = (pb + 255) & ~(size_t)255;             // (the loader's: every expert's set starts on 256 bytes)
    const int n_w = two_w ? 2 : 1, n_y = two_y ? 2 : 1;
    const size_t yb = (size_t)(R + guard_rows) * (size_t)ld_out * 4;
    std::unique_ptr<DevBuf> pl[2], dy[2];
    {
        DevBuf wsrc(grow * (size_t)N * n_expert), wdev(drow * (size_t)N * n_expert);
        if (!wsrc.p || !wdev.p) { fail("device alloc failed"); return MI355_ERR_OOM; }
        for (int i = 0; i < n_w; i++) {
            pl[i].reset(new DevBuf(stride * (size_t)n_expert));
            if (!pl[i]->p || !wsrc.up(i ? W1 : W0, grow * (size_t)N * n_expert)) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
            hipError_t e = launch_repack_rows(type, wsrc.as<uint8_t>(), wdev.as<uint8_t>(), K, N * n_expert, nullptr);
            for (int64_t ex = 0; ex < n_expert && e == hipSuccess; ex++) {
                const uint8_t *src = wdev.as<uint8_t>() + (size_t)ex * drow * (size_t)N;
                uint8_t *dst = pl[i]->as<uint8_t>() + (size_t)ex * stride;
                e = planes ? launch_mmq_expand(type, src, drow, (int)N, (int)K, dst, nullptr) : launch_expand_q80_copy(type, src, drow, (int)N, (int)K, dst, nullptr);
            }
            if (e == hipSuccess) e = hipDeviceSynchronize();
            if (e != hipSuccess) return hip_fail(e, "moe_mul_mat_grouped (weights)");
        }
    }
    DevBuf dx((size_t)K * R * 4), dmeta(meta.size() * 4);
    ActBufs ab((size_t)K, (size_t)R);
    if (!dx.up(x, (size_t)K * R * 4) || !dmeta.up(meta.data(), meta.size() * 4) || !ab.ok()) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    for (int i = 0; i < n_y; i++) {
        dy[i].reset(new DevBuf(yb));
        if (!dy[i]->p || hipMemset(dy[i]->p, 0xFF, yb) != hipSuccess) { fail("device alloc failed"); return MI355_ERR_OOM; }
    }
    hipError_t e = launch_quantize(dx.as<float>(), (int)K, (int)R, ab.q, planes, !planes, nullptr);
    if (e == hipSuccess) {
        if (form == 0) e = launch_mmq_planes_moe(type, pl[0]->as<uint8_t>(), stride, n_expert, dmeta.as<int32_t>(), (int)N, (int)K, (int)R, ab.q, dy[0]->as<float>(), (int)ld_out, nullptr);
        else if (form == 1) e = launch_mmq_planes_swiglu_moe(type, pl[0]->as<uint8_t>(), pl[1]->as<uint8_t>(), stride, n_expert, dmeta.as<int32_t>(), (int)N, (int)K, (int)R, ab.q,
                                                             dy[0]->as<float>(), (int)ld_out, nullptr);
        else {
            const uint8_t *w[2] = {pl[0]->as<uint8_t>(), two_w ? pl[1]->as<uint8_t>() : nullptr};
            float *o[2] = {dy[0]->as<float>(), two_y ? dy[1]->as<float>() : nullptr};
            e = launch_mmq_q80_moe(type, w, o, n_w, stride, n_expert, dmeta.as<int32_t>(), (int)N, (int)K, (int)R, ab.q, (int)ld_out, nullptr);
        }
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "moe_mul_mat_grouped");
    if (!dy[0]->down(y0, yb) || (two_y && !dy[1]->down(y1, yb))) return MI355_ERR_HIP;
    return MI355_OK;
}

int mi355_op_gather_rows_f32(const float *src, int64_t n_src_rows, int64_t n, const int32_t *rows, int64_t n_rows, float *dst) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (n_src_rows < 1 || n < 1 || n_rows < 1 || n > INT32_MAX || n_rows > 65535) { fail("gather_rows_f32: bad shape"); return MI355_ERR_ARG; }
    for (int64_t r = 0; r < n_rows; r++)
        if (rows[r] < 0 || rows[r] >= n_src_rows) { fail("gather_rows_f32: rows[" + std::to_string(r) + "] outside the source"); return MI355_ERR_ARG; }
    const size_t nsrc = (size_t)n_src_rows * (size_t)n * 4, nd = (size_t)n_rows * (size_t)n * 4;
    DevBuf ds(nsrc), dr((size_t)n_rows * 4), dd(nd);
    if (!ds.up(src, nsrc) || !dr.up(rows, (size_t)n_rows * 4) || !dd.p) return MI355_ERR_OOM;
    hipError_t e = launch_gather_rows_f32(ds.as<float>(), dr.as<int32_t>(), (int)n_rows, (int)n, dd.as<float>(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "gather_rows_f32");
    return dd.down(dst, nd) ? MI355_OK : MI355_ERR_HIP;
}

// flash_attn_ext over a caller-supplied cache and cell table (test entry): launch_flash_attn as a prompt batch or a generic step runs it.  cell_seq: the cells'
// sequence bit masks, q_seq: each query's sequence (0 .. 63); a query sees cell c < n_kv where cell_pos[c] >= 0, cell_pos[c] <= q_pos and bit q_seq of
// cell_seq[c] is set.  n_kv (1 .. n_cells) is what the kernels read from the device as the number of cells to scan; the grid, the splits and the workspace
// are sized for n_cells, as a step of a context whose high-water mark lies below the bound its launches were sized for.
int mi355_op_flash_attn_seq(const float *q, int64_t T, int32_t H, int32_t G, int32_t D, int32_t type_k, const void *k, int32_t type_v, const void *v,
                            int32_t n_cells, const int32_t *cell_pos, const uint64_t *cell_seq, const int32_t *q_pos, const int32_t *q_seq, int32_t n_kv,
                            float scale, float *out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if ((D != 64 && D != 128) || G < 1 || H < 1 || H % G || T < 1 || n_cells < 1) { fail("unsupported head geometry"); return MI355_ERR_ARG; }
    if ((type_k != T_F16 && type_k != T_Q8_0 && type_k != T_Q4_0) || (type_v != T_F16 && type_v != T_Q8_0 && type_v != T_Q4_0)) { fail("bad cache type"); return MI355_ERR_ARG; }
    if (!q || !k || !v || !cell_pos || !cell_seq || !q_pos || !q_seq || !out) { fail("flash_attn: null argument"); return MI355_ERR_ARG; }
    if (n_kv < 1 || n_kv > n_cells) { fail("flash_attn: n_kv outside [1, n_cells]"); return MI355_ERR_ARG; }
    for (int64_t t = 0; t < T; t++)
        if (q_seq[t] < 0 || q_seq[t] > 63) { fail("flash_attn: q_seq[" + std::to_string(t) + "] outside [0, 63]"); return MI355_ERR_ARG; }
    std::vector<uint8_t> kc, vc;
    std::vector<uint16_t> ks, vs;
    cache_planes_from_rows(type_k, k, G, D, n_cells, kc, ks);
    cache_planes_from_rows(type_v, v, G, D, n_cells, vc, vs);
    DevBuf dk(kc.size()), dks(ks.size() * 2 + 16), dv(vc.size()), dvs(vs.size() * 2 + 16);
    DevBuf dq((size_t)T * H * D * 4), dout((size_t)T * H * D * 4), dcp((size_t)n_cells * 4), dcs((size_t)n_cells * 8), dtp((size_t)T * 4), dts((size_t)T * 4), dn(16);
    if (!dk.up(kc.data(), kc.size()) || !dv.up(vc.data(), vc.size()) || !dq.up(q, (size_t)T * H * D * 4) || !dout.p || !dks.p || !dvs.p) return MI355_ERR_OOM;
    if (!ks.empty()) dks.up(ks.data(), ks.size() * 2);
    if (!vs.empty()) dvs.up(vs.data(), vs.size() * 2);
    if (!dcp.up(cell_pos, (size_t)n_cells * 4) || !dcs.up(cell_seq, (size_t)n_cells * 8) || !dtp.up(q_pos, (size_t)T * 4) || !dts.up(q_seq, (size_t)T * 4) ||
        !dn.up(&n_kv, 4)) return MI355_ERR_OOM;
    AttnArgs a{};
    a.q = dq.as<float>(); a.out = dout.as<float>();
    a.kv.k = dk.as<uint8_t>(); a.kv.kd = dks.as<uint16_t>(); a.kv.v = dv.as<uint8_t>(); a.kv.vd = dvs.as<uint16_t>();
    a.type_k = type_k; a.type_v = type_v; a.T = (int)T; a.H = H; a.G = G; a.D = D; a.n_ctx = n_cells;
    a.cell_pos = dcp.as<int32_t>(); a.cell_seq = dcs.as<uint64_t>(); a.tok_pos = dtp.as<int32_t>(); a.tok_seq = dts.as<int32_t>();
    a.n_kv_dev = dn.as<int32_t>(); a.n_kv_max = n_cells; a.scale = scale;
    a.splits = flash_attn_pick_splits((int)T, G, n_cells);
    a.pf_splits = flash_attn_prefill_splits((int)T, H, G, D, n_cells);
    DevBuf part(flash_attn_workspace_floats((int)T, H, D, std::max(a.splits, a.pf_splits)) * 4);
    if (!part.p) return MI355_ERR_OOM;
    a.part = part.as<float>();
    hipError_t e = launch_flash_attn(a, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "flash_attn");
    return dout.down(out, (size_t)T * H * D * 4) ? MI355_OK : MI355_ERR_HIP;
}

// ... with one sequence: every cell in sequence 0, every query of sequence 0, the whole table scanned
int mi355_op_flash_attn(const float *q, int64_t T, int32_t H, int32_t G, int32_t D, int32_t type_k, const void *k, int32_t type_v,
                        const void *v, int32_t n_cells, const int32_t *cell_pos, const int32_t *q_pos, float scale, float *out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (T < 1 || n_cells < 1) { fail("unsupported head geometry"); return MI355_ERR_ARG; }
    std::vector<uint64_t> seqm((size_t)n_cells, 1ull);
    std::vector<int32_t> tseq((size_t)T, 0);
    return mi355_op_flash_attn_seq(q, T, H, G, D, type_k, k, type_v, v, n_cells, cell_pos, seqm.data(), q_pos, tseq.data(), n_cells, scale, out);
}

// How launch_flash_attn would split the keys of such a call: out[0] = flash_attn_pick_splits (the split kernel), out[1] = flash_attn_prefill_splits (the
// matrix-core prompt kernel), out[2] = 1 where the prompt kernel takes the call (test entry: a test states which splits its case runs with through this)
int mi355_op_flash_attn_plan(int64_t T, int32_t H, int32_t G, int32_t D, int32_t type_k, int32_t type_v, int32_t n_cells, int32_t *out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if ((D != 64 && D != 128) || G < 1 || H < 1 || H % G || T < 1 || T > INT32_MAX || n_cells < 1 || !out) { fail("unsupported head geometry"); return MI355_ERR_ARG; }
    AttnArgs a{};
    a.type_k = type_k; a.type_v = type_v; a.T = (int)T; a.H = H; a.G = G; a.D = D; a.n_ctx = n_cells; a.n_kv_max = n_cells;
    out[0] = flash_attn_pick_splits((int)T, G, n_cells);
    out[1] = flash_attn_prefill_splits((int)T, H, G, D, n_cells);
    out[2] = flash_attn_prefill_applicable(a) && !(fa_v_acc_f16_enabled() && type_k == T_F16 && type_v == T_F16) ? 1 : 0;
    return MI355_OK;
}

// The attention block of ONE single-token step exactly as the decode path launches it (test entry): rope of q
// and of the token's K row, the K / V row quantised into the cache, attention over the visible cells, merge of the chunk partials, Q8_K quantisation and the
// attn_output mat-vec with its residual.  fused = 1: attn_out.hip (one launch); 0: the single-launch decode attention + the weight-stream mat-vec.
// k / v: the cache BEFORE the step as ggml-layout rows [n_cells][G * D] (the row at tok_cell is overwritten); cell_pos[tok_cell] must already be tok_pos.
// cell_seq (null: every cell in sequence 0 only) / tok_seq: the cells' sequence bit masks and the token's sequence, so that the cache may hold other sequences'
// cells; use_lists: the launch walks the token's chunk list (host/attn_chunks.h) as a step of a context with several sequences does.
int mi355_op_attn_step_seq(const float *q, const float *k_new, const float *v_new, int32_t H, int32_t G, int32_t D, int32_t type_k, const void *k, int32_t type_v,
                           const void *v, int32_t n_cells, const int32_t *cell_pos, const uint64_t *cell_seq, int32_t tok_pos, int32_t tok_seq, int32_t tok_cell,
                           int32_t use_lists, float rope_base, int32_t n_rot, float scale, int32_t type_o, const void *W_o, int64_t E, const float *resid,
                           int32_t fused, float *att_out, float *out, void *k_row_out, void *v_row_out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if ((D != 64 && D != 128) || G < 1 || H % G || n_cells < 1 || tok_cell < 0 || tok_cell >= n_cells) { fail("bad geometry"); return MI355_ERR_ARG; }
    if (tok_seq < 0 || tok_seq > 63) { fail("tok_seq outside [0, 63]"); return MI355_ERR_ARG; }
    const int64_t K = (int64_t)H * D;
    const size_t kv_dim = (size_t)G * D;
    auto fill = [&](int type, const void *rows, std::vector<uint8_t> &codes, std::vector<uint16_t> &scales) { cache_planes_from_rows(type, rows, G, D, n_cells, codes, scales); };
    if ((type_k != T_F16 && type_k != T_Q8_0 && type_k != T_Q4_0) || (type_v != T_F16 && type_v != T_Q8_0 && type_v != T_Q4_0)) { fail("bad cache type"); return MI355_ERR_ARG; }
    std::vector<uint8_t> kc, vc;
    std::vector<uint16_t> ks, vs;
    fill(type_k, k, kc, ks);
    fill(type_v, v, vc, vs);
    const size_t grow = ggml_row_bytes(type_o, K), drow = dev_row_bytes(type_o, K);
    if (!grow || K % 256) { fail("bad attn_output type / K"); return MI355_ERR_ARG; }
    DevBuf dk(kc.size()), dks(ks.size() * 2 + 16), dv(vc.size()), dvs(vs.size() * 2 + 16);
    DevBuf dq((size_t)K * 4), dkn(kv_dim * 4), dvn(kv_dim * 4), datt((size_t)K * 4), dcp((size_t)n_cells * 4), dcs((size_t)n_cells * 8), dtp(16), dts(16), dn(16), dcell(16);
    DevBuf wsrc(grow * E), wdev(drow * E), dres((size_t)E * 4), dout((size_t)E * 4), dcnt(64 * ATT_SYNC_STRIDE * 4), dflags(64 * ATT_SYNC_STRIDE * 4), dserial(64), dcsb((size_t)std::max(n_rot, 4) * 4 + 64);
    ActBufs ab((size_t)K, 1);
    if (!dk.up(kc.data(), kc.size()) || !dv.up(vc.data(), vc.size()) || !dq.up(q, (size_t)K * 4) || !dkn.up(k_new, kv_dim * 4) || !dvn.up(v_new, kv_dim * 4) ||
        !wsrc.up(W_o, grow * E) || !wdev.p || !dres.up(resid, (size_t)E * 4) || !dout.p || !ab.ok() || !datt.p) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    if (!ks.empty()) dks.up(ks.data(), ks.size() * 2);
    if (!vs.empty()) dvs.up(vs.data(), vs.size() * 2);
    std::vector<uint64_t> seqm((size_t)n_cells, 1ull);
    if (cell_seq) seqm.assign(cell_seq, cell_seq + n_cells);
    const int32_t tseq = tok_seq, nkv = n_cells;
    const unsigned one = 1u;
    ChunkLists cl;
    if (use_lists && !cl.make(n_cells, n_cells, cell_pos, seqm.data(), &tseq, 1)) return MI355_ERR_OOM;
    dcp.up(cell_pos, (size_t)n_cells * 4); dcs.up(seqm.data(), (size_t)n_cells * 8); dtp.up(&tok_pos, 4); dts.up(&tseq, 4); dn.up(&nkv, 4); dcell.up(&tok_cell, 4);
    dserial.up(&one, 4);
    hipError_t e = launch_repack_rows(type_o, wsrc.as<uint8_t>(), wdev.as<uint8_t>(), K, E, nullptr);
    if (e != hipSuccess) return hip_fail(e, "repack");
    RopeArgs ra{};
    ra.n_rot = n_rot; ra.freq_base = rope_base; ra.freq_scale = 1.0f; ra.freq_factors = nullptr; ra.neox = 0;
    e = launch_rope_table(dtp.as<int32_t>(), 1, ra, dcsb.as<float>(), nullptr);
    if (e != hipSuccess) return hip_fail(e, "rope_table");
    AttnArgs a{};
    a.q = dq.as<float>(); a.out = datt.as<float>();
    a.kv.k = dk.as<uint8_t>(); a.kv.kd = dks.as<uint16_t>(); a.kv.v = dv.as<uint8_t>(); a.kv.vd = dvs.as<uint16_t>();
    a.type_k = type_k; a.type_v = type_v; a.T = 1; a.H = H; a.G = G; a.D = D; a.n_ctx = n_cells;
    a.cell_pos = dcp.as<int32_t>(); a.cell_seq = dcs.as<uint64_t>(); a.tok_pos = dtp.as<int32_t>(); a.tok_seq = dts.as<int32_t>();
    a.n_kv_dev = dn.as<int32_t>(); a.n_kv_max = n_cells; a.scale = scale;
    a.out_q = &ab.q; a.out_q8k = true; a.out_q80 = false;
    MMVQSeg so{};
    so.W = wdev.as<uint8_t>(); so.out = dout.as<float>(); so.resid = dres.as<float>(); so.type = type_o; so.n_rows = (int)E; so.ld_out = (int)E; so.row_bytes = drow;
    if (fused) {
        a.splits = attn_out_fused_splits(a);
        if (use_lists) cl.apply(a);
        DevBuf part(flash_attn_workspace_floats(1, H, D, a.splits) * 4);
        a.part = part.as<float>();
        if (!attn_out_fused_applicable(a, ra, so, (int)K, EPI_ADD)) { fail("attn_out.hip has no form for this shape"); return MI355_ERR_ARG; }
        DevBuf dgran(attn_out_granule_words((int)K) * 8);
        if (!dgran.p) return MI355_ERR_OOM;
        e = launch_attn_out_fused(a, dcsb.as<float>(), ra, dkn.as<float>(), dvn.as<float>(), dcell.as<int32_t>(), dcnt.as<unsigned>(), dflags.as<unsigned>(),
                                  dgran.as<unsigned long long>(), 3, dserial.as<unsigned>(), so, (int)K, EPI_ADD, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) return hip_fail(e, "attn_out_fused");
    } else {
        a.splits = flash_attn_decode_splits(n_cells);
        if (use_lists) cl.apply(a);
        DevBuf part(flash_attn_workspace_floats(1, H, D, a.splits) * 4);
        a.part = part.as<float>();
        if (!flash_attn_decode_fused_applicable(a, ra)) { fail("the single-launch decode attention has no form for this shape"); return MI355_ERR_ARG; }
        e = launch_flash_attn_decode_fused(a, dcsb.as<float>(), ra, dkn.as<float>(), dvn.as<float>(), dcell.as<int32_t>(), dcnt.as<unsigned>(), nullptr);
        if (e != hipSuccess) return hip_fail(e, "flash_attn_decode_fused");
        MMVQArgs m{};
        m.n_seg = 1; m.K = (int)K; m.T = 1; m.epi = EPI_ADD; m.seg[0] = so;
        m.aq = ab.q.qs; m.ad = ab.q.d; m.abs = ab.q.bsums; m.aq0 = ab.q.qs0; m.ad0 = ab.q.d0;
        e = launch_mmvq(m, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) return hip_fail(e, "attn_output mat-vec");
    }
    if (att_out && !datt.down(att_out, (size_t)K * 4)) return MI355_ERR_HIP;
    if (out && !dout.down(out, (size_t)E * 4)) return MI355_ERR_HIP;
    // the cache row the step wrote, back in ggml block layout
    auto row_back = [&](int type, DevBuf &codes, DevBuf &scales, void *dst) -> bool { return cache_row_to_ggml(type, codes, scales, G, D, n_cells, tok_cell, dst); };
    if (!row_back(type_k, dk, dks, k_row_out) || !row_back(type_v, dv, dvs, v_row_out)) return MI355_ERR_HIP;
    return MI355_OK;
}

int mi355_op_attn_step(const float *q, const float *k_new, const float *v_new, int32_t H, int32_t G, int32_t D, int32_t type_k, const void *k, int32_t type_v,
                       const void *v, int32_t n_cells, const int32_t *cell_pos, int32_t tok_pos, int32_t tok_cell, float rope_base, int32_t n_rot, float scale,
                       int32_t type_o, const void *W_o, int64_t E, const float *resid, int32_t fused, float *att_out, float *out, void *k_row_out, void *v_row_out) {
    return mi355_op_attn_step_seq(q, k_new, v_new, H, G, D, type_k, k, type_v, v, n_cells, cell_pos, nullptr, tok_pos, 0, tok_cell, 0, rope_base, n_rot, scale, type_o,
                                  W_o, E, resid, fused, att_out, out, k_row_out, v_row_out);
}

// The decode attention of ONE token of a qwen2 / qwen3 file as the decode path launches it (test entry): NEOX rope of q and of the token's K row - each head
// RMS-normalised and multiplied by q_norm / k_norm first where they are given (qwen3; null: no norm, the qwen2 path) - the K / V row quantised into the cache,
// attention over the visible cells and the merge of the chunk partials.  mode 1: the single-launch form of a single-token step (tickets, the last workgroup
// merges); 0: the store-fused form of a batched step (K / V stored inside the attention launch, merged by its own launch); 2: the generic path of prompt
// batches (rope_kv_store, then the split attention on the rotated q).  Cache arguments and outputs as mi355_op_attn_step.
// cell_seq (null: every cell in sequence 0 only), tok_seq, use_lists (modes 0 and 1 only): as mi355_op_attn_step_seq.
int mi355_op_attn_decode_neox_seq(const float *q, const float *k_new, const float *v_new, int32_t H, int32_t G, int32_t D, int32_t type_k, const void *k, int32_t type_v,
                                  const void *v, int32_t n_cells, const int32_t *cell_pos, const uint64_t *cell_seq, int32_t tok_pos, int32_t tok_seq, int32_t tok_cell,
                                  int32_t use_lists, float rope_base, float scale, const float *q_norm, const float *k_norm, float eps, int32_t mode, float *att_out,
                                  void *k_row_out, void *v_row_out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if ((D != 64 && D != 128) || G < 1 || H % G || n_cells < 1 || tok_cell < 0 || tok_cell >= n_cells || mode < 0 || mode > 2) { fail("bad geometry / mode"); return MI355_ERR_ARG; }
    if (tok_seq < 0 || tok_seq > 63 || (use_lists && mode == 2)) { fail("tok_seq outside [0, 63], or chunk lists asked of the generic path"); return MI355_ERR_ARG; }
    if ((type_k != T_F16 && type_k != T_Q8_0 && type_k != T_Q4_0) || (type_v != T_F16 && type_v != T_Q8_0 && type_v != T_Q4_0)) { fail("bad cache type"); return MI355_ERR_ARG; }
    const size_t K = (size_t)H * D, kv_dim = (size_t)G * D;
    std::vector<uint8_t> kc, vc;
    std::vector<uint16_t> ks, vs;
    cache_planes_from_rows(type_k, k, G, D, n_cells, kc, ks);
    cache_planes_from_rows(type_v, v, G, D, n_cells, vc, vs);
    DevBuf dk(kc.size()), dks(ks.size() * 2 + 16), dv(vc.size()), dvs(vs.size() * 2 + 16), dqn((size_t)D * 4), dkn_w((size_t)D * 4);
    DevBuf dq(K * 4), dkn(kv_dim * 4), dvn(kv_dim * 4), datt(K * 4), dcp((size_t)n_cells * 4), dcs((size_t)n_cells * 8), dtp(16), dts(16), dn(16), dcell(16);
    DevBuf dcnt(64 * ATT_SYNC_STRIDE * 4), dcsb((size_t)D * 4 + 64);
    if (!dk.up(kc.data(), kc.size()) || !dv.up(vc.data(), vc.size()) || !dq.up(q, K * 4) || !dkn.up(k_new, kv_dim * 4) || !dvn.up(v_new, kv_dim * 4) || !datt.p ||
        (q_norm && !dqn.up(q_norm, (size_t)D * 4)) || (k_norm && !dkn_w.up(k_norm, (size_t)D * 4))) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    if (!ks.empty()) dks.up(ks.data(), ks.size() * 2);
    if (!vs.empty()) dvs.up(vs.data(), vs.size() * 2);
    std::vector<uint64_t> seqm((size_t)n_cells, 1ull);
    if (cell_seq) seqm.assign(cell_seq, cell_seq + n_cells);
    const int32_t tseq = tok_seq, nkv = n_cells;
    ChunkLists cl;
    if (use_lists && !cl.make(n_cells, n_cells, cell_pos, seqm.data(), &tseq, 1)) return MI355_ERR_OOM;
    dcp.up(cell_pos, (size_t)n_cells * 4); dcs.up(seqm.data(), (size_t)n_cells * 8); dtp.up(&tok_pos, 4); dts.up(&tseq, 4); dn.up(&nkv, 4); dcell.up(&tok_cell, 4);
    RopeArgs ra{};
    ra.n_rot = D; ra.freq_base = rope_base; ra.freq_scale = 1.0f; ra.freq_factors = nullptr; ra.neox = 1;
    ra.q_norm = q_norm ? dqn.as<float>() : nullptr; ra.k_norm = k_norm ? dkn_w.as<float>() : nullptr; ra.qk_eps = eps;
    hipError_t e = launch_rope_table(dtp.as<int32_t>(), 1, ra, dcsb.as<float>(), nullptr);
    if (e != hipSuccess) return hip_fail(e, "rope_table");
    AttnArgs a{};
    a.q = dq.as<float>(); a.out = datt.as<float>();
    a.kv.k = dk.as<uint8_t>(); a.kv.kd = dks.as<uint16_t>(); a.kv.v = dv.as<uint8_t>(); a.kv.vd = dvs.as<uint16_t>();
    a.type_k = type_k; a.type_v = type_v; a.T = 1; a.H = H; a.G = G; a.D = D; a.n_ctx = n_cells;
    a.cell_pos = dcp.as<int32_t>(); a.cell_seq = dcs.as<uint64_t>(); a.tok_pos = dtp.as<int32_t>(); a.tok_seq = dts.as<int32_t>();
    a.n_kv_dev = dn.as<int32_t>(); a.n_kv_max = n_cells; a.scale = scale;
    if (mode == 2) {
        e = launch_rope_kv_store(dq.as<float>(), dkn.as<float>(), dvn.as<float>(), 1, H, G, D, dtp.as<int32_t>(), dcell.as<int32_t>(), ra, a.kv, type_k, type_v, n_cells,
                                 dcsb.as<float>(), nullptr);
        if (e != hipSuccess) return hip_fail(e, "rope_kv_store");
        a.splits = flash_attn_pick_splits(1, G, n_cells);
        a.pf_splits = flash_attn_prefill_splits(1, H, G, D, n_cells);
        DevBuf part(flash_attn_workspace_floats(1, H, D, std::max(a.splits, a.pf_splits)) * 4);
        a.part = part.as<float>();
        e = launch_flash_attn(a, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) return hip_fail(e, "flash_attn");
    } else {
        a.splits = flash_attn_decode_splits(n_cells);
        if (use_lists) cl.apply(a);
        DevBuf part(flash_attn_workspace_floats(1, H, D, a.splits) * 4);
        a.part = part.as<float>();
        if (!flash_attn_decode_applicable(a, ra) || (mode == 1 && !flash_attn_decode_fused_applicable(a, ra))) { fail("the decode attention has no form for this shape"); return MI355_ERR_ARG; }
        if (mode == 1) e = launch_flash_attn_decode_fused(a, dcsb.as<float>(), ra, dkn.as<float>(), dvn.as<float>(), dcell.as<int32_t>(), dcnt.as<unsigned>(), nullptr);
        else e = launch_flash_attn_decode(a, dcsb.as<float>(), ra, nullptr, dkn.as<float>(), dvn.as<float>(), dcell.as<int32_t>());
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) return hip_fail(e, "flash_attn_decode");
    }
    if (att_out && !datt.down(att_out, K * 4)) return MI355_ERR_HIP;
    if (!cache_row_to_ggml(type_k, dk, dks, G, D, n_cells, tok_cell, k_row_out) || !cache_row_to_ggml(type_v, dv, dvs, G, D, n_cells, tok_cell, v_row_out)) return MI355_ERR_HIP;
    return MI355_OK;
}

int mi355_op_attn_decode_neox(const float *q, const float *k_new, const float *v_new, int32_t H, int32_t G, int32_t D, int32_t type_k, const void *k, int32_t type_v,
                              const void *v, int32_t n_cells, const int32_t *cell_pos, int32_t tok_pos, int32_t tok_cell, float rope_base, float scale,
                              const float *q_norm, const float *k_norm, float eps, int32_t mode, float *att_out, void *k_row_out, void *v_row_out) {
    return mi355_op_attn_decode_neox_seq(q, k_new, v_new, H, G, D, type_k, k, type_v, v, n_cells, cell_pos, nullptr, tok_pos, 0, tok_cell, 0, rope_base, scale, q_norm,
                                         k_norm, eps, mode, att_out, k_row_out, v_row_out);
}

// The K / V cache write of a batch on its own (test entry): the four launches that rotate K and write K / V rows into the cache,
// on a caller-supplied cache that crosses the boundary whole, in and out, as ggml-layout rows.  form 0: launch_rope_kv_store computing its angles, 1: on the
// table of launch_rope_table, 2: launch_rope_q_kv_store_fast, 3: launch_kv_store_fast.  A form that has no kernel for the arguments is refused, never launched.
int mi355_op_kv_store(int32_t form, float *q, const float *k, const float *v, int64_t T, int32_t H, int32_t G, int32_t D, int32_t n_rot, int32_t neox,
                      int32_t type_k, int32_t type_v, int32_t n_cells, const int32_t *tok_pos, const int32_t *tok_cell, float rope_base, float freq_scale,
                      const float *freq_factors, const float *q_norm, const float *k_norm, float eps, void *k_cache, void *v_cache) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (form < 0 || form > 3 || !k || !v || !tok_pos || !tok_cell || !k_cache || !v_cache || (form != 3 && !q)) { fail("bad form / null argument"); return MI355_ERR_ARG; }
    if (T < 1 || T > 4096 || H < 1 || G < 1 || D < 32 || D % 32 || n_rot < 2 || n_rot > D || n_rot % 2 || n_cells < 1) { fail("bad geometry"); return MI355_ERR_ARG; }
    if ((type_k != T_F16 && type_k != T_Q8_0 && type_k != T_Q4_0) || (type_v != T_F16 && type_v != T_Q8_0 && type_v != T_Q4_0)) { fail("bad cache type"); return MI355_ERR_ARG; }
    for (int64_t t = 0; t < T; t++)
        if (tok_cell[t] < 0 || tok_cell[t] >= n_cells) { fail("tok_cell outside the cache"); return MI355_ERR_ARG; }
    const size_t q_dim = (size_t)H * D, kv_dim = (size_t)G * D;
    if (form < 2 && ((size_t)n_rot + kv_dim) * 4 > 48 * 1024) { fail("n_head_kv * head_dim too wide for the generic kernel's LDS"); return MI355_ERR_ARG; }
    if (form < 2 && (q_norm || k_norm) && (n_rot != D || (D != 64 && D != 128))) { fail("the q / k norm works on whole heads of 64 or 128"); return MI355_ERR_ARG; }
    std::vector<uint8_t> kc, vc;
    std::vector<uint16_t> ks, vs;
    cache_planes_from_rows(type_k, k_cache, G, D, n_cells, kc, ks);
    cache_planes_from_rows(type_v, v_cache, G, D, n_cells, vc, vs);
    DevBuf dk(kc.size()), dks(ks.size() * 2 + 16), dv(vc.size()), dvs(vs.size() * 2 + 16), dqn((size_t)D * 4), dkn_w((size_t)D * 4), dff((size_t)n_rot * 2 + 16);
    DevBuf dq((size_t)T * q_dim * 4), dkn((size_t)T * kv_dim * 4), dvn((size_t)T * kv_dim * 4), dtp((size_t)T * 4), dcell((size_t)T * 4), dcsb((size_t)T * n_rot * 4 + 64);
    if (!dk.up(kc.data(), kc.size()) || !dv.up(vc.data(), vc.size()) || !dks.p || !dvs.p || !dq.p || (q && !dq.up(q, (size_t)T * q_dim * 4)) ||
        !dkn.up(k, (size_t)T * kv_dim * 4) || !dvn.up(v, (size_t)T * kv_dim * 4) || !dtp.up(tok_pos, (size_t)T * 4) || !dcell.up(tok_cell, (size_t)T * 4) || !dcsb.p ||
        (q_norm && !dqn.up(q_norm, (size_t)D * 4)) || (k_norm && !dkn_w.up(k_norm, (size_t)D * 4)) ||
        (freq_factors && !dff.up(freq_factors, (size_t)(n_rot / 2) * 4))) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    if (!ks.empty() && !dks.up(ks.data(), ks.size() * 2)) return MI355_ERR_OOM;
    if (!vs.empty() && !dvs.up(vs.data(), vs.size() * 2)) return MI355_ERR_OOM;
    RopeArgs ra{};
    ra.n_rot = n_rot; ra.freq_base = rope_base; ra.freq_scale = freq_scale; ra.freq_factors = freq_factors ? dff.as<float>() : nullptr; ra.neox = neox ? 1 : 0;
    ra.q_norm = q_norm ? dqn.as<float>() : nullptr; ra.k_norm = k_norm ? dkn_w.as<float>() : nullptr; ra.qk_eps = eps;
    if (form == 2 && !rope_q_kv_store_fast_applicable(H, G, D, type_k, type_v, ra)) { fail("the vectorised prompt store has no form for these arguments"); return MI355_ERR_ARG; }
    if (form == 3 && !kv_store_fast_applicable(G, D, type_k, type_v, ra)) { fail("the small-batch decode store has no form for these arguments"); return MI355_ERR_ARG; }
    KVLayerView kv{};
    kv.k = dk.as<uint8_t>(); kv.kd = dks.as<uint16_t>(); kv.v = dv.as<uint8_t>(); kv.vd = dvs.as<uint16_t>();
    hipError_t e = hipSuccess;
    if (form != 0) e = launch_rope_table(dtp.as<int32_t>(), (int)T, ra, dcsb.as<float>(), nullptr);
    if (e != hipSuccess) return hip_fail(e, "rope_table");
    if (form < 2)
        e = launch_rope_kv_store(dq.as<float>(), dkn.as<float>(), dvn.as<float>(), (int)T, H, G, D, dtp.as<int32_t>(), dcell.as<int32_t>(), ra, kv, type_k, type_v, n_cells,
                                 form == 1 ? dcsb.as<float>() : nullptr, nullptr);
    else if (form == 2)
        e = launch_rope_q_kv_store_fast(dq.as<float>(), dkn.as<float>(), dvn.as<float>(), (int)T, H, G, D, dcsb.as<float>(), ra, dcell.as<int32_t>(), kv, type_k, type_v,
                                        n_cells, nullptr);
    else
        e = launch_kv_store_fast(dkn.as<float>(), dvn.as<float>(), (int)T, G, D, dcsb.as<float>(), ra, dcell.as<int32_t>(), kv, type_k, type_v, n_cells, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "kv_store");
    if (form != 3 && !dq.down(q, (size_t)T * q_dim * 4)) return MI355_ERR_HIP;
    if (!cache_rows_from_planes(type_k, dk, dks, G, D, n_cells, k_cache) || !cache_rows_from_planes(type_v, dv, dvs, G, D, n_cells, v_cache)) return MI355_ERR_HIP;
    return MI355_OK;
}

// The attention of ONE batched single-token step - T tokens, up to 64, as a continuous-batching step holds them - in each form Context::attn_core launches it
// (test entry).  q [T][H * D] un-rotated, k_new / v_new [T][G * D]; k_cache / v_cache: the whole cache as ggml-layout rows [n_cells][G * D], in and out;
// cell_pos / cell_seq [n_cells] with the new cells already set (cell_pos[tok_cell[t]] = tok_pos[t], bit tok_seq[t] of cell_seq[tok_cell[t]]); n_kv: cells to
// scan (what the device reads), every launch is sized for n_cells.
//   mode 0: K rope + K / V store inside the attention launch (launch_flash_attn_decode with the new rows), every chunk of the cache scanned;
//   mode 1: the same launch on the per-token chunk lists of host/attn_chunks.h;
//   mode 2: launch_kv_store_fast, then launch_flash_attn_decode without the store, on the lists;
//   mode 3: the generic path, launch_rope_kv_store + launch_flash_attn.
// att_out [T][H * D]; q8k_out (nullable; H * D a multiple of 256): the Q8_K blocks of the T rows that the merge wrote for attn_output, as ggml block_q8_K.
// A shape or mode without a kernel is refused before anything is launched: more than 64 tokens, a token in several or in another token's sequence (modes 0
// and 1: no token may read another's new cell), what flash_attn_decode_applicable (modes 0 - 2) or kv_store_fast_applicable (the lists, mode 2) reject.
int mi355_op_attn_batch_step(const float *q, const float *k_new, const float *v_new, int64_t T, int32_t H, int32_t G, int32_t D, int32_t type_k, void *k_cache,
                             int32_t type_v, void *v_cache, int32_t n_cells, int32_t n_kv, const int32_t *cell_pos, const uint64_t *cell_seq, const int32_t *tok_pos,
                             const int32_t *tok_seq, const int32_t *tok_cell, float rope_base, int32_t n_rot, int32_t neox, float scale, int32_t mode,
                             float *att_out, void *q8k_out) {
    return mi355_op_attn_batch_step_planes(q, k_new, v_new, T, H, G, D, type_k, k_cache, type_v, v_cache, n_cells, n_kv, cell_pos, cell_seq, tok_pos, tok_seq, tok_cell,
                                           rope_base, n_rot, neox, scale, mode, att_out, q8k_out, nullptr, nullptr);
}
// bh_out / bl_out (both or neither, with q8k_out): the merge also writes the block sums of its Q8_K rows as the int8 planes of the MFMA kernels (AttnArgs out_bh /
// out_bl, what Context::attn_core sets for a K-quant attn_output); the planes are 0xFF bytes before the launch
int mi355_op_attn_batch_step_planes(const float *q, const float *k_new, const float *v_new, int64_t T, int32_t H, int32_t G, int32_t D, int32_t type_k, void *k_cache,
                                    int32_t type_v, void *v_cache, int32_t n_cells, int32_t n_kv, const int32_t *cell_pos, const uint64_t *cell_seq, const int32_t *tok_pos,
                                    const int32_t *tok_seq, const int32_t *tok_cell, float rope_base, int32_t n_rot, int32_t neox, float scale, int32_t mode,
                                    float *att_out, void *q8k_out, int8_t *bh_out, int8_t *bl_out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if ((bh_out != nullptr) != (bl_out != nullptr) || (bh_out && !q8k_out)) { fail("attn_batch_step: bh_out / bl_out come together and with q8k_out"); return MI355_ERR_ARG; }
    if (!q || !k_new || !v_new || !k_cache || !v_cache || !cell_pos || !cell_seq || !tok_pos || !tok_seq || !tok_cell || !att_out) { fail("attn_batch_step: null argument"); return MI355_ERR_ARG; }
    if (mode < 0 || mode > 3) { fail("attn_batch_step: mode outside [0, 3]"); return MI355_ERR_ARG; }
    if (T < 1 || T > 64) { fail("attn_batch_step: a batched step holds 1 .. 64 tokens"); return MI355_ERR_ARG; }
    if ((D != 64 && D != 128) || G < 1 || H < 1 || H % G || H / G > 8 || n_cells < 1 || n_kv < 1 || n_kv > n_cells || n_rot < 2 || n_rot > D || n_rot % 2) { fail("attn_batch_step: bad geometry"); return MI355_ERR_ARG; }
    if ((type_k != T_F16 && type_k != T_Q8_0 && type_k != T_Q4_0) || (type_v != T_F16 && type_v != T_Q8_0 && type_v != T_Q4_0)) { fail("attn_batch_step: bad cache type"); return MI355_ERR_ARG; }
    const size_t K = (size_t)H * D, kv_dim = (size_t)G * D;
    if (q8k_out && K % 256) { fail("attn_batch_step: Q8_K rows need n_head * head_dim to be a multiple of 256"); return MI355_ERR_ARG; }
    uint64_t seen = 0;
    for (int64_t t = 0; t < T; t++) {
        if (tok_seq[t] < 0 || tok_seq[t] > 63) { fail("attn_batch_step: tok_seq[" + std::to_string(t) + "] outside [0, 63]"); return MI355_ERR_ARG; }
        if (tok_cell[t] < 0 || tok_cell[t] >= n_kv) { fail("attn_batch_step: tok_cell[" + std::to_string(t) + "] outside the scanned cells"); return MI355_ERR_ARG; }
        const uint64_t bit = 1ull << tok_seq[t];
        if (mode < 2 && ((seen & bit) || cell_seq[tok_cell[t]] != bit)) { fail("attn_batch_step: the store-fused launch needs every token in one sequence of its own"); return MI355_ERR_ARG; }
        seen |= bit;
    }
    RopeArgs ra{};
    ra.n_rot = n_rot; ra.freq_base = rope_base; ra.freq_scale = 1.0f; ra.freq_factors = nullptr; ra.neox = neox ? 1 : 0;
    AttnArgs a{};
    a.type_k = type_k; a.type_v = type_v; a.T = (int)T; a.H = H; a.G = G; a.D = D; a.n_ctx = n_cells; a.n_kv_max = n_cells; a.scale = scale;
    if (mode < 3 && !flash_attn_decode_applicable(a, ra)) { fail("attn_batch_step: the decode attention has no form for this shape"); return MI355_ERR_ARG; }
    if ((mode == 1 || mode == 2) && !kv_store_fast_applicable(G, D, type_k, type_v, ra)) { fail("attn_batch_step: the small-batch store has no form for these arguments (no chunk lists either)"); return MI355_ERR_ARG; }
    if (mode == 3 && ((size_t)n_rot + kv_dim) * 4 > 48 * 1024) { fail("attn_batch_step: n_head_kv * head_dim too wide for the generic store's LDS"); return MI355_ERR_ARG; }
    std::vector<uint8_t> kc, vc;
    std::vector<uint16_t> ks, vs;
    cache_planes_from_rows(type_k, k_cache, G, D, n_cells, kc, ks);
    cache_planes_from_rows(type_v, v_cache, G, D, n_cells, vc, vs);
    DevBuf dk(kc.size()), dks(ks.size() * 2 + 16), dv(vc.size()), dvs(vs.size() * 2 + 16);
    DevBuf dq((size_t)T * K * 4), dkn((size_t)T * kv_dim * 4), dvn((size_t)T * kv_dim * 4), datt((size_t)T * K * 4), dcp((size_t)n_cells * 4), dcs((size_t)n_cells * 8);
    DevBuf dtp((size_t)T * 4), dts((size_t)T * 4), dcell((size_t)T * 4), dn(16), dcsb((size_t)T * n_rot * 4 + 64), dblk(q8k_out ? ggml_row_bytes(T_Q8_K, (int64_t)K) * T : 16);
    ActBufs ab(q8k_out ? K : 256, (size_t)T + 1);
    const size_t pb = bh_out ? (size_t)T * (K / 16) : 0;
    DevBuf dbh(pb ? pb : 16), dbl(pb ? pb : 16);
    if (!dbh.p || !dbl.p || hipMemset(dbh.p, 0xFF, dbh.n) != hipSuccess || hipMemset(dbl.p, 0xFF, dbl.n) != hipSuccess) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    if (!dk.up(kc.data(), kc.size()) || !dv.up(vc.data(), vc.size()) || !dks.p || !dvs.p || !dq.up(q, (size_t)T * K * 4) || !dkn.up(k_new, (size_t)T * kv_dim * 4) ||
        !dvn.up(v_new, (size_t)T * kv_dim * 4) || !datt.p || !dcp.up(cell_pos, (size_t)n_cells * 4) || !dcs.up(cell_seq, (size_t)n_cells * 8) ||
        !dtp.up(tok_pos, (size_t)T * 4) || !dts.up(tok_seq, (size_t)T * 4) || !dcell.up(tok_cell, (size_t)T * 4) || !dn.up(&n_kv, 4) || !dcsb.p || !dblk.p || !ab.ok()) {
        fail("device alloc/copy failed"); return MI355_ERR_OOM;
    }
    if (!ks.empty() && !dks.up(ks.data(), ks.size() * 2)) return MI355_ERR_OOM;
    if (!vs.empty() && !dvs.up(vs.data(), vs.size() * 2)) return MI355_ERR_OOM;
    ChunkLists cl;
    if ((mode == 1 || mode == 2) && !cl.make(n_kv, n_cells, cell_pos, cell_seq, tok_seq, (int)T)) return MI355_ERR_OOM;
    a.q = dq.as<float>(); a.out = datt.as<float>();
    a.kv.k = dk.as<uint8_t>(); a.kv.kd = dks.as<uint16_t>(); a.kv.v = dv.as<uint8_t>(); a.kv.vd = dvs.as<uint16_t>();
    a.cell_pos = dcp.as<int32_t>(); a.cell_seq = dcs.as<uint64_t>(); a.tok_pos = dtp.as<int32_t>(); a.tok_seq = dts.as<int32_t>(); a.n_kv_dev = dn.as<int32_t>();
    if (q8k_out) { a.out_q = &ab.q; a.out_q8k = true; a.out_q80 = false; }
    if (bh_out) { a.out_bh = dbh.as<int8_t>(); a.out_bl = dbl.as<int8_t>(); }
    if (mode == 3) {
        a.splits = flash_attn_pick_splits((int)T, G, n_cells);
        a.pf_splits = flash_attn_prefill_splits((int)T, H, G, D, n_cells);
    } else {
        a.splits = flash_attn_decode_splits(n_cells);
        if (mode != 0) cl.apply(a);
    }
    DevBuf part(flash_attn_workspace_floats((int)T, H, D, std::max(a.splits, a.pf_splits)) * 4);
    if (!part.p) return MI355_ERR_OOM;
    a.part = part.as<float>();
    hipError_t e = launch_rope_table(dtp.as<int32_t>(), (int)T, ra, dcsb.as<float>(), nullptr);
    if (e != hipSuccess) return hip_fail(e, "rope_table");
    if (mode == 3) {
        e = launch_rope_kv_store(dq.as<float>(), dkn.as<float>(), dvn.as<float>(), (int)T, H, G, D, dtp.as<int32_t>(), dcell.as<int32_t>(), ra, a.kv, type_k, type_v, n_cells,
                                 dcsb.as<float>(), nullptr);
        if (e == hipSuccess) e = launch_flash_attn(a, nullptr);
    } else if (mode == 2) {
        e = launch_kv_store_fast(dkn.as<float>(), dvn.as<float>(), (int)T, G, D, dcsb.as<float>(), ra, dcell.as<int32_t>(), a.kv, type_k, type_v, n_cells, nullptr);
        if (e == hipSuccess) e = launch_flash_attn_decode(a, dcsb.as<float>(), ra, nullptr);
    } else {
        e = launch_flash_attn_decode(a, dcsb.as<float>(), ra, nullptr, dkn.as<float>(), dvn.as<float>(), dcell.as<int32_t>());
    }
    if (e == hipSuccess && q8k_out) e = launch_pack_q8k_blocks(ab.q, (int)K, (int)T, dblk.as<uint8_t>(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "attn_batch_step");
    if (!datt.down(att_out, (size_t)T * K * 4)) return MI355_ERR_HIP;
    if (q8k_out && !dblk.down(q8k_out, ggml_row_bytes(T_Q8_K, (int64_t)K) * T)) return MI355_ERR_HIP;
    if (bh_out && (!dbh.down(bh_out, pb) || !dbl.down(bl_out, pb))) return MI355_ERR_HIP;
    if (!cache_rows_from_planes(type_k, dk, dks, G, D, n_cells, k_cache) || !cache_rows_from_planes(type_v, dv, dvs, G, D, n_cells, v_cache)) return MI355_ERR_HIP;
    return MI355_OK;
}

// The K-shift on its own (test entry): one launch_k_shift over a caller-supplied K cache that crosses the boundary whole, in and out.
int mi355_op_k_shift(int32_t type_k, int32_t G, int32_t D, int32_t n_rot, int32_t neox, int32_t n_cells, const int32_t *delta, float rope_base, float freq_scale,
                     const float *freq_factors, float ext_factor, float attn_factor, float corr_lo, float corr_hi, void *k_cache) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!delta || !k_cache || G < 1 || D < 32 || D % 32 || n_rot < 2 || n_rot > D || n_rot % 2 || n_cells < 1) { fail("bad geometry / null argument"); return MI355_ERR_ARG; }
    if (type_k != T_F16 && type_k != T_Q8_0 && type_k != T_Q4_0) { fail("bad cache type"); return MI355_ERR_ARG; }
    if (((size_t)n_rot + (size_t)G * D) * 4 > 48 * 1024) { fail("n_head_kv * head_dim too wide for the kernel's LDS"); return MI355_ERR_ARG; }
    std::vector<uint8_t> kc;
    std::vector<uint16_t> ks;
    cache_planes_from_rows(type_k, k_cache, G, D, n_cells, kc, ks);
    DevBuf dk(kc.size()), dks(ks.size() * 2 + 16), dd((size_t)n_cells * 4), dff((size_t)n_rot * 2 + 16);
    if (!dk.up(kc.data(), kc.size()) || !dks.p || !dd.up(delta, (size_t)n_cells * 4) || (freq_factors && !dff.up(freq_factors, (size_t)(n_rot / 2) * 4))) {
        fail("device alloc/copy failed"); return MI355_ERR_OOM;
    }
    if (!ks.empty() && !dks.up(ks.data(), ks.size() * 2)) return MI355_ERR_OOM;
    RopeArgs ra{};
    ra.n_rot = n_rot; ra.freq_base = rope_base; ra.freq_scale = freq_scale; ra.freq_factors = freq_factors ? dff.as<float>() : nullptr; ra.neox = neox ? 1 : 0;
    ra.ext_factor = ext_factor; ra.attn_factor = attn_factor; ra.corr_lo = corr_lo; ra.corr_hi = corr_hi;
    KVLayerView kv{};
    kv.k = dk.as<uint8_t>(); kv.kd = dks.as<uint16_t>();
    hipError_t e = launch_k_shift(kv, type_k, G, D, n_cells, dd.as<int32_t>(), ra, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "k_shift");
    return cache_rows_from_planes(type_k, dk, dks, G, D, n_cells, k_cache) ? MI355_OK : MI355_ERR_HIP;
}

// The gather / scatter kernels of a sequence's state on their own (test entries): a cache of n_layer layers crosses the boundary as ggml-layout rows per layer and is
// uploaded into device planes; `cells` is checked here, as Context::state_seq_get / set check their own lists before they launch.
namespace {
struct StateOpCache {
    std::vector<std::unique_ptr<DevBuf>> bufs;       // per layer: K codes, K scales, V codes, V scales
    std::vector<KVLayerView> views;
    std::unique_ptr<DevBuf> table, cells, rows;
    size_t row_bytes = 0;
    int init(int type_k, int type_v, int n_layer, int G, int D, int n_cells, const void *const *k_rows, const void *const *v_rows, const int32_t *cell_list, int n, bool distinct) {
        if (!k_rows || !v_rows || !cell_list || n_layer < 1 || n_layer > 1024 || G < 1 || D < 32 || D % 32 || n_cells < 1 || n < 1 || n > n_cells) { fail("kv_state: bad geometry / null argument"); return MI355_ERR_ARG; }
        if ((type_k != T_F16 && type_k != T_Q8_0 && type_k != T_Q4_0) || (type_v != T_F16 && type_v != T_Q8_0 && type_v != T_Q4_0)) { fail("kv_state: bad cache type"); return MI355_ERR_ARG; }
        std::vector<char> seen((size_t)n_cells, 0);
        for (int i = 0; i < n; i++) {
            if (cell_list[i] < 0 || cell_list[i] >= n_cells) { fail("kv_state: cells[" + std::to_string(i) + "] outside the cache"); return MI355_ERR_ARG; }
            if (distinct && seen[(size_t)cell_list[i]]) { fail("kv_state: cells[" + std::to_string(i) + "] listed twice"); return MI355_ERR_ARG; }
            seen[(size_t)cell_list[i]] = 1;
        }
        views.resize((size_t)n_layer);
        for (int il = 0; il < n_layer; il++) {
            if (!k_rows[il] || !v_rows[il]) { fail("kv_state: null layer"); return MI355_ERR_ARG; }
            std::vector<uint8_t> kc, vc;
            std::vector<uint16_t> ks, vs;
            cache_planes_from_rows(type_k, k_rows[il], G, D, n_cells, kc, ks);
            cache_planes_from_rows(type_v, v_rows[il], G, D, n_cells, vc, vs);
            DevBuf *b[4] = {new DevBuf(kc.size()), new DevBuf(ks.size() * 2 + 16), new DevBuf(vc.size()), new DevBuf(vs.size() * 2 + 16)};
            for (DevBuf *p : b) bufs.emplace_back(p);
            if (!b[0]->up(kc.data(), kc.size()) || !b[2]->up(vc.data(), vc.size()) || !b[1]->p || !b[3]->p || (!ks.empty() && !b[1]->up(ks.data(), ks.size() * 2)) ||
                (!vs.empty() && !b[3]->up(vs.data(), vs.size() * 2))) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
            views[(size_t)il].k = b[0]->as<uint8_t>(); views[(size_t)il].kd = b[1]->as<uint16_t>(); views[(size_t)il].v = b[2]->as<uint8_t>(); views[(size_t)il].vd = b[3]->as<uint16_t>();
        }
        row_bytes = (size_t)n_layer * n * (kv_state_row_bytes(type_k, G, D) + kv_state_row_bytes(type_v, G, D));
        table.reset(new DevBuf(views.size() * sizeof(KVLayerView)));
        cells.reset(new DevBuf((size_t)n * 4));
        rows.reset(new DevBuf(row_bytes));
        if (!table->up(views.data(), views.size() * sizeof(KVLayerView)) || !cells->up(cell_list, (size_t)n * 4) || !rows->p) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
        return MI355_OK;
    }
};
}  // namespace

int mi355_op_kv_state_pack(int32_t type_k, int32_t type_v, int32_t n_layer, int32_t G, int32_t D, int32_t n_cells, const void *const *k_rows, const void *const *v_rows,
                           const int32_t *cells, int32_t n, void *out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!out) { fail("kv_state_pack: null output"); return MI355_ERR_ARG; }
    StateOpCache c;
    if (const int rc = c.init(type_k, type_v, n_layer, G, D, n_cells, k_rows, v_rows, cells, n, false)) return rc;
    hipError_t e = launch_kv_state_pack(c.table->as<KVLayerView>(), n_layer, type_k, type_v, G, D, n_cells, c.cells->as<int32_t>(), n, c.rows->as<uint8_t>(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "kv_state_pack");
    return c.rows->down(out, c.row_bytes) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_kv_state_unpack(int32_t type_k, int32_t type_v, int32_t n_layer, int32_t G, int32_t D, int32_t n_cells, const void *in, const int32_t *cells, int32_t n,
                             void *const *k_rows, void *const *v_rows) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!in) { fail("kv_state_unpack: null input"); return MI355_ERR_ARG; }
    StateOpCache c;
    if (const int rc = c.init(type_k, type_v, n_layer, G, D, n_cells, k_rows, v_rows, cells, n, true)) return rc;
    if (!c.rows->up(in, c.row_bytes)) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    hipError_t e = launch_kv_state_unpack(c.table->as<KVLayerView>(), n_layer, type_k, type_v, G, D, n_cells, c.cells->as<int32_t>(), n, c.rows->as<uint8_t>(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "kv_state_unpack");
    for (int il = 0; il < n_layer; il++)
        if (!cache_rows_from_planes(type_k, *c.bufs[(size_t)il * 4], *c.bufs[(size_t)il * 4 + 1], G, D, n_cells, k_rows[il]) ||
            !cache_rows_from_planes(type_v, *c.bufs[(size_t)il * 4 + 2], *c.bufs[(size_t)il * 4 + 3], G, D, n_cells, v_rows[il])) return MI355_ERR_HIP;
    return MI355_OK;
}

// ------------------------------------------------------------------ the LLaVA image encoder's launches, one at a time (tests/test_gpu_clip_ops.py)
// The tower's attention.  The kernel is named by the function the launcher asks (clip_attn_choice): a refusal returns here, before anything is launched.
int mi355_op_clip_attn(const float *q, const float *k, const float *v, int64_t T, int32_t H, int32_t D, int32_t n_img, float *out, uint16_t *out_h, int32_t *path) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!q || !k || !v || !out || !path || T < 1 || T > (1 << 20) || H < 1 || D < 4 || D % 4 || n_img < 1) { fail("clip_attn: bad args"); return MI355_ERR_ARG; }
    const ClipAttnChoice ch = clip_attn_choice((int)T, D);
    *path = ch.path;
    if (ch.path == CLIP_ATTN_REFUSED) { fail("clip_attn: no kernel for this head size and row count"); return MI355_ERR_ARG; }
    const size_t n = (size_t)n_img * T * H * D;
    DevBuf dq(n * 4), dk(n * 4), dv(n * 4), dout(n * 4), dh(n * 2);
    if (!dq.up(q, n * 4) || !dk.up(k, n * 4) || !dv.up(v, n * 4) || !dout.p || !dh.p) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    hipError_t e = launch_clip_attn(dq.as<float>(), dk.as<float>(), dv.as<float>(), (int)T, H, D, dout.as<float>(), out_h ? dh.p : nullptr, n_img, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "clip_attn");
    if (out_h && !dh.down(out_h, n * 2)) return MI355_ERR_HIP;
    return dout.down(out, n * 4) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_mul_mat_f16_xh(const uint16_t *W, int64_t N, int64_t K, const float *x, int64_t T, int64_t ld_out, const float *bias, float scale, int32_t do_scale,
                            const float *resid, int32_t in_place, int32_t form, float *y_io) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!W || !x || !y_io || N < 1 || K < 8 || K % 8 || T < 1 || ld_out < N || (form != 0 && form != 1) || (in_place && resid) ||
        (form == 1 && (ld_out != N || (do_scale && !bias)))) { fail("mul_mat_f16_xh: bad args"); return MI355_ERR_ARG; }
    const size_t yb = (size_t)T * ld_out * 4;
    DevBuf dw((size_t)N * K * 2), dx((size_t)T * K * 4), dxh((size_t)T * K * 2), dy(yb), dr(resid ? yb : 0), db(bias ? (size_t)N * 4 : 0), tmp(form == 1 ? yb : 0);
    if (!dw.up(W, (size_t)N * K * 2) || !dx.up(x, (size_t)T * K * 4) || !dxh.p || !dy.up(y_io, yb) || (resid && !dr.up(resid, yb)) || (bias && !db.up(bias, (size_t)N * 4)) || !tmp.p) {
        fail("device alloc/copy failed");
        return MI355_ERR_OOM;
    }
    const float *rs = in_place ? dy.as<float>() : resid ? dr.as<float>() : nullptr, *bs = bias ? db.as<float>() : nullptr;
    hipError_t e = hipSuccess;
    if (form == 0) {
        e = launch_f32_to_f16(dx.as<float>(), dxh.p, (size_t)T * K, nullptr);
        if (e == hipSuccess) e = launch_mmf16_xh(dw.as<uint8_t>(), (int)N, (int)K, dxh.p, (int)T, dy.as<float>(), (int)ld_out, rs, bs, scale, do_scale != 0, nullptr);
    } else {                                                    // host/clip.cc, MI355_CLIP_XH=0: the product into scratch when a residual follows
        float *dst = rs ? tmp.as<float>() : dy.as<float>();
        e = launch_mmf16(dw.as<uint8_t>(), (int)N, (int)K, dx.as<float>(), (int)T, dst, (int)N, nullptr, nullptr);
        if (e == hipSuccess && bs) e = launch_clip_bias(dst, bs, (int)N, (int)T, scale, do_scale != 0, nullptr);
        if (e == hipSuccess && rs) e = launch_add(rs, dst, dy.as<float>(), (int64_t)T * N, nullptr);
    }
    const hipError_t es = hipDeviceSynchronize();
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return hip_fail(e, "mul_mat_f16_xh");
    return dy.down(y_io, yb) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_layer_norm(const float *x, const float *w, const float *b, int64_t n, int64_t T, float eps, int32_t in_place, float *y, uint16_t *y_h) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!x || !w || !b || !y || n < 1 || T < 1) { fail("layer_norm: bad args"); return MI355_ERR_ARG; }
    const size_t nb = (size_t)n * T * 4;
    DevBuf dx(nb), dw((size_t)n * 4), db((size_t)n * 4), dy(in_place ? 0 : nb), dh(nb / 2);
    if (!dx.up(x, nb) || !dw.up(w, (size_t)n * 4) || !db.up(b, (size_t)n * 4) || !dy.p || !dh.p) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    float *o = in_place ? dx.as<float>() : dy.as<float>();
    hipError_t e = y_h ? launch_layer_norm_h(dx.as<float>(), dw.as<float>(), db.as<float>(), (int)n, (int)T, eps, o, dh.p, nullptr)
                       : launch_layer_norm(dx.as<float>(), dw.as<float>(), db.as<float>(), (int)n, (int)T, eps, o, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "layer_norm");
    if (y_h && !dh.down(y_h, nb / 2)) return MI355_ERR_HIP;
    return hipMemcpy(y, o, nb, hipMemcpyDeviceToHost) == hipSuccess ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_clip_gelu(const float *x, int64_t n, int32_t quick, float *y, uint16_t *y_h) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!x || !y || n < 1) { fail("clip_gelu: bad args"); return MI355_ERR_ARG; }
    DevBuf dx((size_t)n * 4), dh((size_t)n * 2);
    if (!dx.up(x, (size_t)n * 4) || !dh.p) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    hipError_t e = launch_clip_gelu(dx.as<float>(), (size_t)n, quick != 0, y_h ? dh.p : nullptr, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "clip_gelu");
    if (y_h && !dh.down(y_h, (size_t)n * 2)) return MI355_ERR_HIP;
    return dx.down(y, (size_t)n * 4) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_clip_im2col(const float *img, int32_t S, int32_t P, int32_t ld, float *patches_io) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!img || !patches_io || P < 1 || S < P || S % P || ld < 3 * P * P) { fail("clip_im2col: bad args"); return MI355_ERR_ARG; }
    const size_t ib = (size_t)3 * S * S * 4, pb = (size_t)(S / P) * (S / P) * ld * 4;
    DevBuf di(ib), dp(pb);
    if (!di.up(img, ib) || !dp.up(patches_io, pb)) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    hipError_t e = launch_clip_im2col(di.as<float>(), S, P, ld, dp.as<float>(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "clip_im2col");
    return dp.down(patches_io, pb) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_clip_embed(const float *patch, const float *cls, const float *pos, int32_t E, int32_t T, float *emb) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!patch || !cls || !pos || !emb || E < 1 || T < 2) { fail("clip_embed: bad args"); return MI355_ERR_ARG; }
    const size_t rb = (size_t)E * 4;
    DevBuf dpa(rb * (T - 1)), dc(rb), dpo(rb * T), de(rb * T);
    if (!dpa.up(patch, rb * (T - 1)) || !dc.up(cls, rb) || !dpo.up(pos, rb * T) || !de.p) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    hipError_t e = launch_clip_embed(dpa.as<float>(), dc.as<float>(), dpo.as<float>(), E, T, de.as<float>(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "clip_embed");
    return de.down(emb, rb * T) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_clip_bias(float *x_io, const float *b, int32_t n, int32_t T, float scale, int32_t do_scale) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!x_io || !b || n < 1 || T < 1) { fail("clip_bias: bad args"); return MI355_ERR_ARG; }
    const size_t nb = (size_t)n * T * 4;
    DevBuf dx(nb), db((size_t)n * 4);
    if (!dx.up(x_io, nb) || !db.up(b, (size_t)n * 4)) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    hipError_t e = launch_clip_bias(dx.as<float>(), db.as<float>(), n, T, scale, do_scale != 0, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "clip_bias");
    return dx.down(x_io, nb) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_f32_to_f16(const float *x, int64_t n, uint16_t *out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (!x || !out || n < 4 || n % 4) { fail("f32_to_f16: n must be a positive multiple of 4"); return MI355_ERR_ARG; }
    DevBuf dx((size_t)n * 4), dy((size_t)n * 2);
    if (!dx.up(x, (size_t)n * 4) || !dy.p) { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
    hipError_t e = launch_f32_to_f16(dx.as<float>(), dy.p, (size_t)n, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "f32_to_f16");
    return dy.down(out, (size_t)n * 2) ? MI355_OK : MI355_ERR_HIP;
}

int mi355_op_add_qkv_bias(float *q_io, float *k_io, float *v_io, const float *bq, const float *bk, const float *bv, int32_t nq, int32_t nkv, int32_t T) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (nq < 1 || nkv < 0 || T < 1 || (bq && !q_io) || (bk && !k_io) || (bv && !v_io) || ((bk || bv) && nkv < 1)) { fail("add_qkv_bias: bad args"); return MI355_ERR_ARG; }
    float *const xs[3] = {q_io, k_io, v_io};
    const float *const bs[3] = {bq, bk, bv};
    std::unique_ptr<DevBuf> dx[3], db[3];
    for (int s = 0; s < 3; s++) {
        const size_t n = s == 0 ? (size_t)nq : (size_t)nkv;
        if (xs[s]) { dx[s].reset(new DevBuf(n * T * 4)); if (!dx[s]->up(xs[s], n * T * 4)) { fail("device alloc/copy failed"); return MI355_ERR_OOM; } }
        if (bs[s]) { db[s].reset(new DevBuf(n * 4)); if (!db[s]->up(bs[s], n * 4)) { fail("device alloc/copy failed"); return MI355_ERR_OOM; } }
    }
    auto xp = [&](int s) { return dx[s] ? dx[s]->as<float>() : nullptr; };
    auto bp = [&](int s) { return db[s] ? db[s]->as<float>() : nullptr; };
    hipError_t e = launch_add_qkv_bias(xp(0), xp(1), xp(2), bp(0), bp(1), bp(2), nq, nkv, T, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "add_qkv_bias");
    for (int s = 0; s < 3; s++)
        if (xs[s] && !dx[s]->down(xs[s], (s == 0 ? (size_t)nq : (size_t)nkv) * T * 4)) return MI355_ERR_HIP;
    return MI355_OK;
}

int mi355_debug_set_option(const char *name, int32_t value) {
    if (!name) return MI355_ERR_ARG;
    if (!strcmp(name, "mmq_planes")) { g_op_mmq_planes = value != 0; return MI355_OK; }
    if (!strcmp(name, "mmq_tiles")) { mmq_set_tiles(value); return MI355_OK; }
    if (!strcmp(name, "mmq_q80_tiles")) { mmq_q80_set_tiles(value); return MI355_OK; }
    if (!strcmp(name, "mmq_split")) { mmq_set_split(value); return MI355_OK; }
    if (!strcmp(name, "mmq_lds_form")) { mmq_set_lds_form(value); return MI355_OK; }
    if (!strcmp(name, "mmq_ksplit")) { g_op_mmq_ksplit = value != 0; return MI355_OK; }
    if (!strcmp(name, "attn_store_fuse")) { set_attn_store_fuse(value != 0); return MI355_OK; }
    if (!strcmp(name, "rope_fast")) { set_rope_fast(value != 0); return MI355_OK; }
    if (!strcmp(name, "decode_mega") || !strcmp(name, "decode_engine")) {
        // the whole-step kernel and the layer engine are experiments that lost their A/Bs: only a library built with MI355_BUILD_EXPERIMENTS=1 holds them
        if (value > 0 && !experiments_built()) { fail(std::string(name) + ": the experiment kernels are not in this build (MI355_BUILD_EXPERIMENTS=1 python cortex.llamacpp_amd/build.py --force)"); return MI355_ERR_ARG; }
        if (name[7] == 'm') set_decode_mega(value != 0); else set_decode_engine(value);
        return MI355_OK;
    }
    if (!strcmp(name, "tp_p2p")) { tp_p2p_use(value != 0); return MI355_OK; }
    if (!strcmp(name, "tp_p2p_prompt")) { tp_p2p_use_prompt(value != 0); return MI355_OK; }
    if (!strcmp(name, "mmvq_stream")) { mmvq_set_stream(value != 0); return MI355_OK; }
    if (!strcmp(name, "attn_out_fused")) { set_attn_out_fused(value); return MI355_OK; }     // (contexts created afterwards)
    if (!strcmp(name, "qkv_attn_fused")) { set_qkv_attn_fused(value); return MI355_OK; }     // Q | K | V inside the attention launch (applies from the next step's launches on; graphs captured earlier keep their form)
    if (!strcmp(name, "moe_group_min")) { set_moe_group_min(value); return MI355_OK; }
    if (!strcmp(name, "moe_q80_grouped")) { set_moe_q80_grouped(value != 0); return MI355_OK; }
    if (!strcmp(name, "fa_v_acc_f16")) { set_fa_v_acc_f16(value); return MI355_OK; }              // f16 cache: the CPU path's fp16 V accumulation (parity mode)
    if (!strcmp(name, "raise_stream_error")) { debug_raise_stream_error((unsigned)value); return MI355_OK; }   // tests: what a timed-out in-kernel wait does
    if (!strcmp(name, "state_stage_kib")) { set_state_stage_max((size_t)(value > 0 ? value : 0) * 1024); return MI355_OK; }   // tests: sequence states through a small staging block, in chunks (0: the default 64 MiB; contexts that have not moved a state yet)
    if (!strcmp(name, "tp_null_group")) { tp_set_null_group(0, value); return MI355_OK; }
    fail(std::string("unknown option ") + name);
    return MI355_ERR_ARG;
}

// simple read-bandwidth probe: sum-reduce `bytes` of device memory
// ---------------------------------------------------------------- row split group
int mi355_tp_unique_id(void *id_out, size_t cap) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    std::string err;
    const int n = tp_unique_id(id_out, cap, err);
    if (n < 0) { fail(err); return MI355_ERR_ARG; }
    return n;
}
int mi355_tp_init(int32_t device, int32_t rank, int32_t size, const void *id, size_t id_len) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) { fail("hipSetDevice failed"); return MI355_ERR_ARG; }
    std::string err;
    if (tp_init(rank, size, id, id_len, err) != 0) { fail(err); return MI355_ERR_ARG; }
    return MI355_OK;
}
void mi355_tp_shutdown(void) { tp_shutdown(); }
int mi355_tp_worker_main(int sock_fd) {
    try {
        if (!g_backend_ok && mi355_backend_init() != MI355_OK) return 66;
        return tp_split_worker_main(sock_fd);
    } catch (const std::exception &e) {
        fprintf(stderr, "mi355_tp_worker: %s\n", e.what());
        return 70;
    } catch (...) { return 70; }
}
int32_t mi355_tp_rank(void) { return tp_rank(); }
int32_t mi355_tp_size(void) { return tp_size(); }
int mi355_tp_set_host_exchange(mi355_tp_host_exchange fn, void *user, int32_t rank, int32_t size) {
    if (fn && (size < 1 || rank < 0 || rank >= size)) { fail("bad rank / size"); return MI355_ERR_ARG; }
    tp_set_host_exchange(reinterpret_cast<tp_host_exchange_fn>(fn), user, rank, size);
    return MI355_OK;
}

int mi355_tp_p2p_local_handle2(void *out, size_t cap, size_t max_floats, size_t prompt_floats) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    std::string err;
    const int n = tp_p2p_local_handle(out, cap, max_floats, prompt_floats, err);
    if (n < 0) { fail(err); return MI355_ERR_ARG; }
    return n;
}
int mi355_tp_p2p_local_handle(void *out, size_t cap, size_t max_floats) { return mi355_tp_p2p_local_handle2(out, cap, max_floats, 0); }
int mi355_tp_p2p_enable(const void *handles, size_t len) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    std::string err;
    if (tp_p2p_enable(handles, len, err) != 0) { fail(err); return MI355_ERR_HIP; }
    return MI355_OK;
}
int64_t mi355_tp_p2p_exchanges(void) { return tp_p2p_exchanges(); }
int64_t mi355_tp_p2p_prompt_exchanges(void) { return tp_p2p_prompt_exchanges(); }

double mi355_bench_hbm_read(size_t bytes, int iters) {
    if (!need_device()) return -1.0;
    return hbm_read_probe(bytes, iters);
}

// ---------------------------------------------------------------- tokenizer
static Vocab *model_vocab(mi355_model *m) {
    if (!m) { fail("null model"); return nullptr; }
    if (!m->vocab_tried) {
        m->vocab_tried = true;
        std::string err;
        m->vocab_ok = m->vocab.load(*m->m->file, err);
        if (!m->vocab_ok) fail("tokenizer: " + err);
    }
    return m->vocab_ok ? &m->vocab : nullptr;
}
int32_t mi355_tokenize(mi355_model *m, const char *text, int32_t text_len, mi355_token *out, int32_t cap, int32_t add_special, int32_t parse_special) {
    MI355_GUARD(return INT32_MIN,
        Vocab *v = model_vocab(m);
        if (!v || !text || text_len < 0) return INT32_MIN;
        const std::vector<int32_t> ids = v->tokenize(std::string(text, (size_t)text_len), add_special != 0, parse_special != 0);
        if ((int64_t)ids.size() > cap || !out) return -(int32_t)ids.size();
        memcpy(out, ids.data(), ids.size() * sizeof(int32_t));
        return (int32_t)ids.size();
    )
}
int32_t mi355_token_to_piece(mi355_model *m, mi355_token tok, char *buf, int32_t cap, int32_t special) {
    MI355_GUARD(return INT32_MIN,
        Vocab *v = model_vocab(m);
        if (!v) return INT32_MIN;
        const std::string p = v->token_to_piece(tok, special != 0);
        if ((int64_t)p.size() > cap || !buf) return -(int32_t)p.size();
        memcpy(buf, p.data(), p.size());
        return (int32_t)p.size();
    )
}
mi355_token mi355_token_bos(mi355_model *m) { Vocab *v = model_vocab(m); return v ? v->bos() : -1; }
mi355_token mi355_token_eos(mi355_model *m) { Vocab *v = model_vocab(m); return v ? v->eos() : -1; }
int32_t mi355_token_is_eog(mi355_model *m, mi355_token tok) { Vocab *v = model_vocab(m); return v && v->is_eog(tok) ? 1 : 0; }

// ---------------------------------------------------------------- engine
static bool parse_body(const char *txt, Json &j, mi355_engine_callback cb, void *user) {
    std::string err;
    if (txt && Json::parse(txt, j, &err)) return true;
    if (cb) {
        Json st = Json::object(), body = Json::object();
        st["is_done"] = true; st["has_error"] = true; st["is_stream"] = false; st["status_code"] = 400;
        body["message"] = "Malformed JSON body: " + err;
        cb(st.dump().c_str(), body.dump().c_str(), user);
    }
    return false;
}
// The engine copies the callback into whatever outlives the call (a queued stream task); every copy shares `guard`, so the host's release function runs
// exactly once per request, after the last callback the request will ever make - also for a request that ends without a terminal callback (a stream
// cancelled by StopInferencing: src/llama_engine.cc:950-955 breaks out of the loop without one)
static LlamaEngine::Callback wrap_cb(mi355_engine *e, mi355_engine_callback cb, void *user) {
    const mi355_release_fn rel = e->release.load();
    std::shared_ptr<void> guard(user, [rel](void *u) { if (rel) rel(u); });
    return [cb, user, guard](Json &&st, Json &&body) {
        if (!cb) return;
        const std::string s = st.dump(), b = body.dump();
        cb(s.c_str(), b.c_str(), user);
    };
}
// an exception below an engine entry point: answered in the reference's error shape (status 500), never thrown at the host
static void engine_exception(mi355_engine_callback cb, void *user, const char *what) {
    fail(std::string("internal error: ") + what);
    if (!cb) return;
    try {
        Json st = Json::object(), body = Json::object();
        st["is_done"] = true; st["has_error"] = true; st["is_stream"] = false; st["status_code"] = 500;
        body["message"] = std::string("Internal error: ") + what;
        cb(st.dump().c_str(), body.dump().c_str(), user);
    } catch (...) {}
}
mi355_engine *mi355_engine_create(void) {
    if (!g_backend_ok && mi355_backend_init() != MI355_OK) return nullptr;
    MI355_GUARD(return nullptr, return new mi355_engine;)
}
void mi355_engine_destroy(mi355_engine *e) { delete e; }
#define MI355_ENGINE_FWD(cname, Method)                                                                     \
    void cname(mi355_engine *e, const char *body_json, mi355_engine_callback cb, void *user) {              \
        try {                                                                                               \
            Json j;                                                                                         \
            if (!e) return;                                                                                 \
            LlamaEngine::Callback w = wrap_cb(e, cb, user);   /* from here on `user` is released with w */   \
            if (!parse_body(body_json, j, cb, user)) return;                                                \
            e->eng.Method(j, std::move(w));                                                                 \
        } catch (const std::exception &ex) {                                                                \
            engine_exception(cb, user, ex.what());                                                          \
        } catch (...) {                                                                                     \
            engine_exception(cb, user, "unknown exception");                                                \
        }                                                                                                   \
    }
MI355_ENGINE_FWD(mi355_engine_load_model, LoadModel)
MI355_ENGINE_FWD(mi355_engine_unload_model, UnloadModel)
MI355_ENGINE_FWD(mi355_engine_get_model_status, GetModelStatus)
MI355_ENGINE_FWD(mi355_engine_get_models, GetModels)
MI355_ENGINE_FWD(mi355_engine_handle_chat_completion, HandleChatCompletion)
MI355_ENGINE_FWD(mi355_engine_handle_embedding, HandleEmbedding)
#undef MI355_ENGINE_FWD
void mi355_engine_set_release_callback(mi355_engine *e, void (*release)(void *user)) { if (e) e->release.store(release); }
int32_t mi355_engine_is_supported(mi355_engine *e, const char *feature) { return e && feature && e->eng.IsSupported(feature) ? 1 : 0; }
void mi355_engine_stop_inferencing(mi355_engine *e, const char *model_id) { if (e && model_id) e->eng.StopInferencing(model_id); }
int mi355_engine_prompt_cache_stats(mi355_engine *e, const char *model_id, int64_t out[6]) {
    if (!e || !model_id || !out) { fail("prompt_cache_stats: null argument"); return MI355_ERR_ARG; }
    MI355_GUARD(return MI355_ERR_ARG,
        if (!e->eng.PromptCacheStats(model_id, out)) { fail(std::string("prompt_cache_stats: no model ") + model_id); return MI355_ERR_ARG; }
        return MI355_OK;
    )
}
int mi355_engine_spec_stats(mi355_engine *e, const char *model_id, int64_t out[4]) {
    if (!e || !model_id || !out) { fail("spec_stats: null argument"); return MI355_ERR_ARG; }
    MI355_GUARD(return MI355_ERR_ARG,
        if (!e->eng.SpecStats(model_id, out)) { fail(std::string("spec_stats: no model ") + model_id); return MI355_ERR_ARG; }
        return MI355_OK;
    )
}
void mi355_engine_load(mi355_engine *e, const char *engine_path, const char *deps_path, int32_t is_custom_engine_path, const char *log_path, int32_t max_log_lines,
                       int32_t log_level) {
    if (!e) return;
    MI355_GUARD(return, {
        LlamaEngine::EngineLoadOption o;
        o.engine_path = engine_path ? engine_path : ""; o.deps_path = deps_path ? deps_path : ""; o.is_custom_engine_path = is_custom_engine_path != 0;
        o.log_path = log_path ? log_path : ""; o.max_log_lines = max_log_lines; o.log_level = log_level;
        e->eng.Load(o);
        return;
    })
}
void mi355_engine_unload(mi355_engine *e) { if (e) { MI355_GUARD(return, { e->eng.Unload(); return; }) } }
void mi355_engine_set_file_logger(mi355_engine *e, int32_t max_log_lines, const char *log_path) {
    if (e) { MI355_GUARD(return, { e->eng.SetFileLogger(max_log_lines, log_path ? log_path : ""); return; }) }
}
void mi355_engine_set_log_level(mi355_engine *e, int32_t log_level) { if (e) e->eng.SetLogLevel(log_level); }
void mi355_engine_set_log_callback(mi355_engine *e, mi355_log_callback cb, void *user) { (void)e; log_set_callback(cb, user); }

}  // extern "C"
