// c_api.cc — the product C-ABI declared in include/mi355_llama.h, over host/runtime.{h,cc}.  The per-op test entries (mi355_op_*) are in op_entries_*.cc.
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

#include "op_support.h"
#include "../host/clip.h"
#include "../host/cvec.h"
#include "../host/engine.h"
#include "../host/hip_backend.h"
#include "../host/log.h"
#include "../host/runtime.h"
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
static bool g_backend_ok = false;

// what op_support.h declares for the per-op test entries (op_entries_*.cc): the error string, the device check, the switches of mi355_debug_set_option
int mi355::g_op_mmq_planes = 1, mi355::g_op_mmq_ksplit = 1;
void mi355::fail(const std::string &s) { t_err = s; }
bool mi355::need_device() { return g_backend_ok || mi355_backend_init() == MI355_OK; }

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

// ---- control vectors (llama_apply_adapter_cvec, common_control_vector_load)
int32_t mi355_apply_adapter_cvec(mi355_context *ctx, const float *data, size_t len, int32_t n_embd, int32_t il_start, int32_t il_end) {
    if (!ctx) return no_context("apply_adapter_cvec");
    MI355_GUARD(return MI355_ERR_ARG,
        if (ctx->c->apply_cvec(data, len, n_embd, il_start, il_end) != 0) { fail(ctx->c->last_error.empty() ? "apply_adapter_cvec failed" : ctx->c->last_error); return MI355_ERR_ARG; }
        return MI355_OK;
    )
}
int64_t mi355_control_vector_load(const char *const *paths, const float *scales, int32_t n, float *out, size_t cap_floats, int32_t *n_embd_out) {
    if (!paths || n < 1) { fail("control_vector_load: no file given"); return MI355_ERR_ARG; }
    MI355_GUARD(return MI355_ERR_OOM,
        std::vector<ControlVectorFile> files;
        for (int32_t i = 0; i < n; i++) {
            if (!paths[i]) { fail("control_vector_load: null path"); return MI355_ERR_ARG; }
            files.push_back({paths[i], scales ? scales[i] : 1.0f});
        }
        std::vector<float> data;
        int n_embd = 0;
        std::string err;
        if (!control_vector_load(files, data, n_embd, err)) { fail("control_vector_load: " + err); return MI355_ERR_FORMAT; }
        if (n_embd_out) *n_embd_out = n_embd;
        if (out && cap_floats >= data.size()) memcpy(out, data.data(), data.size() * sizeof(float));
        return (int64_t)data.size();
    )
}

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

extern "C" double hbm_read_probe(size_t bytes, int iters);

extern "C" {

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
    OpBufs b;
    uint8_t *dsrc = b.alloc(n * es), *dout = b.alloc(nb + rb);
    float *dim = b.alloc<float>((size_t)n_per_row * 4);
    int32_t *dflag = b.alloc<int32_t>(16);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess) { if (ev0) (void)hipEventDestroy(ev0); fail("quantize_chunk: no timing events"); return MI355_ERR_HIP; }
    struct EvGuard { hipEvent_t a, b; ~EvGuard() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } ev_guard{ev0, ev1};
    const auto c0 = std::chrono::steady_clock::now();
    b.copy_in(dsrc, src, n * es);
    if (imatrix) b.copy_in(dim, imatrix, (size_t)n_per_row * 4);
    b.check(dout && hipMemset(dout + nb, Q80_GUARD, rb) == hipSuccess);
    if (!b.ok()) return oom();
    const auto c1 = std::chrono::steady_clock::now();
    (void)hipEventRecord(ev0, nullptr);
    hipError_t e = launch_quantize_rows(dst_type, src_type, dsrc, n_per_row, n_rows, imatrix ? dim : nullptr, dout, dflag, nullptr);
    if (e == hipErrorInvalidValue) { fail("quantize_chunk: the launcher refuses this shape"); return MI355_ERR_ARG; }
    (void)hipEventRecord(ev1, nullptr);
    if (const int rc = finish(e, "quantize_chunk")) return rc;
    float kernel_ms = 0.0f;
    (void)hipEventElapsedTime(&kernel_ms, ev0, ev1);
    const auto c2 = std::chrono::steady_clock::now();
    int32_t flag = 0;
    std::vector<uint8_t> guard(rb);
    if (!b.down(&flag, dflag, 4).down(guard.data(), dout + nb, rb).ok()) return b.done("quantize_chunk");
    for (uint8_t g : guard)
        if (g != Q80_GUARD) { fail("quantize_chunk: the guard row behind the output was written"); return MI355_ERR_HIP; }
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
    if (!b.down(dst, dout, nb).ok()) return b.done("quantize_chunk");
    const auto c3 = std::chrono::steady_clock::now();
    t_quant_ms[0] = std::chrono::duration<float, std::milli>(c1 - c0).count();
    t_quant_ms[1] = kernel_ms;
    t_quant_ms[2] = std::chrono::duration<float, std::milli>(c3 - c2).count();
    return MI355_OK;
}

// The direction of a layer's difference rows (csrc/cvec.hip): upload, iterate, download.  Every refusal comes before dir_out is written.
int mi355_cvec_direction(int32_t method, const float *rows, int64_t n_rows, int32_t n_embd, const float *init, int32_t n_iter, int32_t n_batch, float tol,
                         float *dir_out, int32_t *iters_out, float *dist_out) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    const bool pca = method == 0;
    if (method != 0 && method != 1) { fail("cvec_direction: method " + std::to_string(method) + " is neither 0 (pca) nor 1 (mean)"); return MI355_ERR_ARG; }
    if (!rows || !dir_out || (pca && !init)) { fail("cvec_direction: null pointer"); return MI355_ERR_ARG; }
    if (n_rows < 1 || n_rows > CVEC_MAX_ROWS) { fail("cvec_direction: n_rows " + std::to_string(n_rows) + " is outside 1 .. 2^20"); return MI355_ERR_ARG; }
    if (n_embd < 32 || n_embd % 32 || n_embd > CVEC_MAX_E) { fail("cvec_direction: n_embd " + std::to_string(n_embd) + " is not a multiple of 32 in 32 .. 65536"); return MI355_ERR_ARG; }
    if (pca && (n_iter < 1 || n_batch < 1)) { fail("cvec_direction: n_iter and n_batch must be at least 1"); return MI355_ERR_ARG; }
    if (pca && std::isnan(tol)) { fail("cvec_direction: tol is not a number"); return MI355_ERR_ARG; }
    const int R = (int)n_rows, E = n_embd;
    const size_t n = (size_t)R * (size_t)E;
    bool any = false;
    for (size_t i = 0; i < n; i++) {
        if (!std::isfinite(rows[i])) { fail("cvec_direction: row " + std::to_string(i / (size_t)E) + " holds a non-finite value"); return MI355_ERR_ARG; }
        any = any || rows[i] != 0.0f;
    }
    if (!any) { fail("cvec_direction: every row is zero"); return MI355_ERR_ARG; }
    if (pca) {
        bool init_any = false;
        for (int j = 0; j < E; j++) {
            if (!std::isfinite(init[j])) { fail("cvec_direction: init holds a non-finite value"); return MI355_ERR_ARG; }
            init_any = init_any || init[j] != 0.0f;
        }
        if (!init_any) { fail("cvec_direction: init is the zero vector"); return MI355_ERR_ARG; }
    }
    MI355_GUARD(return MI355_ERR_OOM,
        const size_t eb = (size_t)E * 4;
        OpBufs b;
        const float *dD = b.upload(rows, n * 4);
        float *db = b.alloc<float>(2 * eb), *dy = b.alloc<float>((size_t)R * 4), *dslab = b.alloc<float>(cvec_scratch_floats(R, E) * 4), *ddist = b.alloc<float>(64);
        if (pca) b.copy_in(db, init, eb);
        b.check(db && hipMemset((uint8_t *)db + eb, Q80_GUARD, eb) == hipSuccess);          // the guard rows behind the direction and the distance word
        b.check(ddist && hipMemset((uint8_t *)ddist + 4, Q80_GUARD, 60) == hipSuccess);
        if (!b.ok()) return oom();
        int iters = 0;
        float dist = 0.0f;
        auto read_dist = [&]() -> int {
            if (const int rc = finish(hipSuccess, "cvec_direction")) return rc;
            if (!b.down(&dist, ddist, 4).ok()) return b.done("cvec_direction");
            if (dist == -1.0f) { fail(pca ? "cvec_direction: the iteration reached the zero vector (the start vector is orthogonal to every row)" : "cvec_direction: the rows' mean is the zero vector"); return MI355_ERR_ARG; }
            if (dist < 0.0f) { fail("cvec_direction: the rows are too large for f32 sums of squares"); return MI355_ERR_ARG; }
            return MI355_OK;
        };
        if (pca) {
            while (iters < n_iter) {
                const hipError_t e = launch_cvec_pca_step(dD, R, E, db, dy, dslab, ddist, nullptr);
                if (e != hipSuccess) return e == hipErrorInvalidValue ? (fail("cvec_direction: the launcher refuses this shape"), (int)MI355_ERR_ARG) : hip_fail(e, "cvec_direction");
                iters++;
                if (iters % n_batch == 0 || iters == n_iter) {
                    if (const int rc = read_dist()) return rc;
                    if (dist < tol) break;
                }
            }
        } else {
            const hipError_t e = launch_cvec_mean_step(dD, R, E, db, dslab, ddist, nullptr);
            if (e != hipSuccess) return e == hipErrorInvalidValue ? (fail("cvec_direction: the launcher refuses this shape"), (int)MI355_ERR_ARG) : hip_fail(e, "cvec_direction");
            if (const int rc = read_dist()) return rc;
        }
        if (const int rc = finish(launch_cvec_orient(dD, R, E, db, dy, nullptr), "cvec_direction")) return rc;
        std::vector<float> res((size_t)E);
        std::vector<uint8_t> guard(eb + 60);
        if (!b.down(res.data(), db, eb).down(guard.data(), (uint8_t *)db + eb, eb).down(guard.data() + eb, (uint8_t *)ddist + 4, 60).ok()) return b.done("cvec_direction");
        for (uint8_t g : guard)
            if (g != Q80_GUARD) { fail("cvec_direction: the guard region behind the outputs was written"); return MI355_ERR_HIP; }
        for (float v : res)
            if (!std::isfinite(v)) { fail("cvec_direction: the direction holds a non-finite value"); return MI355_ERR_HIP; }
        memcpy(dir_out, res.data(), eb);
        if (iters_out) *iters_out = iters;
        if (dist_out) *dist_out = dist;
        return MI355_OK;
    )
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
