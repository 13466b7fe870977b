// runtime.cc — GGUF -> HBM residency, KV cells, and the per-batch executor for the `llama` architecture
// (op order of upstream llm_build_llama / build_attn / build_ffn / build_moe_ffn).
// Reference caller: LlamaServerContext::UpdateSlots -> llama_decode (src/llama_server_context.cc:1628-1635).
#include "runtime.h"

#include <dlfcn.h>
#include "tp_comm.h"
#include "attn_chunks.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace mi355 {

unsigned stream_error_epoch();           // error epochs opened so far in this process (Context::stream_check)
static unsigned *stream_error_word();   // pinned, one per process: raised by a weight-stream / engine kernel whose bounded wait gave up

static thread_local std::string g_err;
void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}
const std::string &last_error_string() { return g_err; }

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) {                                                           \
            set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return e_;                                                                    \
        }                                                                                 \
    } while (0)

// ------------------------------------------------------------------------------------------ model
Model::~Model() {
    while (!adapters.empty()) lora_free(adapters.back());
    for (uint8_t *p : arenas) (void)hipFree(p);
}

// ---- LoRA adapters: the file is checked on the host (lora.cc), then every pair is copied to the device as the file holds it
LoraAdapter *lora_load(Model *m, const std::string &path, std::string &err, int &status) {
    status = 0;
    GGUFFile f;
    err = f.open(path);
    if (!err.empty()) { status = err.rfind("cannot", 0) == 0 ? -101 : -102; return nullptr; }
    LoraPlan plan;
    if (!plan_lora(f, *m, plan, err, status)) return nullptr;
    std::unique_ptr<LoraAdapter> a(new LoraAdapter());
    a->model = m; a->path = path; a->alpha = plan.alpha;
    a->index.assign((size_t)(m->hp.n_layer + 1) * LORA_N_TARGETS, -1);
    size_t total = 0;
    for (const LoraPairPlan &p : plan.pairs) total += ((p.a->bytes + 255) & ~(size_t)255) + ((p.b->bytes + 255) & ~(size_t)255);
    if (hipSetDevice(m->device) != hipSuccess) { err = "hipSetDevice failed"; status = -100; return nullptr; }
    if (hipMalloc(&a->arena, total) != hipSuccess) { err = "hipMalloc of " + std::to_string(total) + " adapter bytes failed"; status = -104; return nullptr; }
    size_t off = 0;
    for (const LoraPairPlan &p : plan.pairs) {
        LoraPair d{p.layer, p.target, p.type, p.r, p.K, p.N, a->arena + off, nullptr};
        off += (p.a->bytes + 255) & ~(size_t)255;
        d.B = a->arena + off;
        off += (p.b->bytes + 255) & ~(size_t)255;
        if (hipMemcpy(const_cast<uint8_t *>(d.A), p.a->data, p.a->bytes, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(const_cast<uint8_t *>(d.B), p.b->data, p.b->bytes, hipMemcpyHostToDevice) != hipSuccess) {
            err = "upload of adapter pair " + p.base + " failed"; status = -105;
            (void)hipFree(a->arena);
            return nullptr;
        }
        a->index[(size_t)(p.layer + 1) * LORA_N_TARGETS + (size_t)p.target] = (int)a->pairs.size();
        a->pairs.push_back(d);
    }
    a->device_bytes = total;
    m->device_bytes += total;
    m->adapters.push_back(a.get());
    return a.release();
}

void lora_free(LoraAdapter *a) {
    if (!a) return;
    if (Model *m = a->model) {
        m->adapters.erase(std::remove(m->adapters.begin(), m->adapters.end(), a), m->adapters.end());
        m->device_bytes -= a->device_bytes;
    }
    if (a->arena) (void)hipFree(a->arena);
    delete a;
}

// the rotary parameters every kernel that rotates takes (with_ff: the per-pair frequency factors of rope_freqs.weight, when the file has them)
static RopeArgs rope_args(const Model &m, bool with_ff) {
    const HParams &hp = m.hp;
    RopeArgs ra{hp.n_rot, hp.rope_base, hp.rope_scale, with_ff && m.rope_freqs.valid() ? (const float *)m.rope_freqs.data : nullptr, hp.rope_neox};
    ra.ext_factor = hp.yarn_ext; ra.attn_factor = hp.yarn_attn; ra.corr_lo = hp.yarn_lo; ra.corr_hi = hp.yarn_hi;
    return ra;
}

// ... and those of one layer: qwen3 layers add their per-head q / k RMSNorm weights (null: none - every other file)
static RopeArgs layer_rope(const RopeArgs &ra, const LayerWeights &L, float eps) {
    RopeArgs r = ra;
    r.q_norm = L.q_norm.valid() ? (const float *)L.q_norm.data : nullptr;
    r.k_norm = L.k_norm.valid() ? (const float *)L.k_norm.data : nullptr;
    r.qk_eps = eps;
    return r;
}

// ---- model_load: plan on the host (model_plan.cc), then upload, then the views and the tied output, then the prefill planes
static bool upload_tensors(Model &m, const LoadPlan &plan, std::string &err, int &status) {
    uint8_t *arena = nullptr, *stage = nullptr;
    if (hipMalloc(&arena, plan.total) != hipSuccess) { err = "hipMalloc of " + std::to_string(plan.total) + " weight bytes failed"; status = -104; return false; }
    m.arenas.push_back(arena);
    if (plan.max_stage && hipMalloc(&stage, plan.max_stage) != hipSuccess) { err = "hipMalloc of staging buffer failed"; status = -104; return false; }
    hipStream_t st = nullptr;
    (void)hipStreamCreate(&st);
    bool ok = true;
    for (const TensorPlan &pl : plan.tensors) {
        DevTensor &d = *pl.dst;
        d.data = arena + pl.off;
        const bool direct = !type_is_repacked(d.type) && (pl.ti->n_dims == 1 || d.row_bytes == ggml_row_bytes(d.type, d.K));
        hipError_t e;
        const uint8_t *src = (const uint8_t *)pl.ti->data + pl.src_off;
        uint8_t *to = direct ? d.data : stage;
        if (pl.src_width == pl.src_pitch) e = hipMemcpyAsync(to, src, pl.src_bytes, hipMemcpyHostToDevice, st);
        else e = hipMemcpy2DAsync(to, pl.src_width, src, pl.src_pitch, pl.src_width, (size_t)pl.src_rows, hipMemcpyHostToDevice, st);
        if (!direct && e == hipSuccess) e = launch_repack_rows(d.type, stage, d.data, d.K, d.N * d.n_expert, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            err = std::string("upload of ") + d.name + " failed: " + hipGetErrorString(e);
            status = -105;
            ok = false;
            break;
        }
    }
    if (stage) (void)hipFree(stage);
    (void)hipStreamDestroy(st);
    return ok;
}

// tied embeddings: the output head is the embedding table.  Encoder files: Q, K and V are row ranges of the fused projection - views into its device
// rows (one launch each; the rows are contiguous per output)
static void alias_tensors(Model &m) {
    const HParams &hp = m.hp;
    if (!m.output.valid()) m.output = m.tok_embd;
    if (!hp.encoder) return;
    for (auto &L : m.layers) {
        const int64_t qw = (int64_t)hp.n_head * hp.head_dim, kvw = (int64_t)hp.n_head_kv * hp.head_dim;
        auto view = [&](DevTensor &v, int64_t row0, int64_t rows, const char *what) {
            v = L.wqkv;
            v.name = L.wqkv.name + "[" + what + "]";
            v.N = rows;
            v.data = L.wqkv.data + (size_t)row0 * L.wqkv.row_bytes;
            v.bytes = (size_t)rows * L.wqkv.row_bytes;
            v.planes = nullptr; v.planes_bytes = 0;
        };
        view(L.wq, 0, qw, "q"); view(L.wk, qw, kvw, "k"); view(L.wv, qw + kvw, kvw, "v");
    }
}

// prompt-processing copy of the per-layer projection weights: both int8 MFMA operand planes of every K-step,
// expanded once here (2 B per weight) so that the prefill kernel spends nothing per weight (mmq.hip).  288 GB of HBM
// is what makes this the default; it is skipped (the prefill kernel then expands on the fly) when memory is short.
static bool expand_prefill_planes(Model &m, int prefill_planes, std::string &err, int &status) {
    if (const char *e = getenv("MI355_PREFILL_PLANES")) prefill_planes = atoi(e);
    if (prefill_planes == 0) return true;
    std::vector<DevTensor *> want;
    for (auto &L : m.layers)
        for (DevTensor *d : {&L.wq, &L.wk, &L.wv, &L.wo, &L.gate, &L.up, &L.down, &L.gate_exps, &L.up_exps, &L.down_exps})
            if (d->valid() && (mmq_planes_bytes(d->type, d->N, (int)d->K) || mmq_q80_copy_bytes(d->type, d->N, (int)d->K))) want.push_back(d);
    // (an *_exps tensor holds one plane set per expert, back to back: a prompt batch runs one contraction per expert)
    // (K-quants: the two int8 MFMA planes; Q4_0 / Q5_0 / IQ4_NL / Q4_1 / Q5_1 / MXFP4: an exact Q8_0-layout copy for the Q8_0 prompt kernel, with a min plane for Q4_1 / Q5_1 and E8M0 scale bytes for MXFP4)
    auto planes_of = [](const DevTensor *d) {
        const size_t b = mmq_planes_bytes(d->type, d->N, (int)d->K);
        return ((b ? b : mmq_q80_copy_bytes(d->type, d->N, (int)d->K)) + 255) & ~(size_t)255;
    };
    size_t need = 0;
    for (DevTensor *d : want) need += planes_of(d) * (size_t)d->n_expert;
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    const size_t reserve = (size_t)24 << 30;             // KV cache, activations, other contexts
    const bool fits = need > 0 && free_b > need + reserve;
    if (need > 0 && !fits && prefill_planes == 1) { err = "not enough device memory for the prefill planes (" + std::to_string(need >> 20) + " MiB)"; status = -104; return false; }
    if (!fits) return true;
    uint8_t *parena = nullptr;
    if (hipMalloc(&parena, need) != hipSuccess) { err = "hipMalloc of the prefill planes failed"; status = -104; return false; }
    m.arenas.push_back(parena);
    size_t off = 0;
    for (DevTensor *d : want) {
        d->planes = parena + off;
        d->planes_bytes = planes_of(d) * (size_t)d->n_expert;
        off += d->planes_bytes;
        for (int64_t x = 0; x < d->n_expert; x++) {
            const uint8_t *src = d->data + (size_t)x * d->row_bytes * (size_t)d->N;
            uint8_t *dst = d->planes + (size_t)x * planes_of(d);
            const hipError_t e = mmq_planes_bytes(d->type, d->N, (int)d->K) ? launch_mmq_expand(d->type, src, d->row_bytes, (int)d->N, (int)d->K, dst, nullptr)
                                                                           : launch_expand_q80_copy(d->type, src, d->row_bytes, (int)d->N, (int)d->K, dst, nullptr);
            if (e != hipSuccess) { err = std::string("plane expansion of ") + d->name + " failed: " + hipGetErrorString(e); status = -105; return false; }
        }
    }
    if (hipDeviceSynchronize() != hipSuccess) { err = "plane expansion failed"; status = -105; return false; }
    m.planes_bytes = need;
    m.device_bytes += need;
    return true;
}

Model *model_load(const std::string &path, int main_gpu, std::string &err, int &status, int prefill_planes, int tp_rank, int tp_size) {
    status = 0;
    std::unique_ptr<Model> m(new Model());
    m->file.reset(new GGUFFile());
    m->path = path;
    err = m->file->open(path);
    if (!err.empty()) { status = err.rfind("cannot", 0) == 0 ? -101 : -102; return nullptr; }
    // every refusal of a file and the whole arena layout: host arithmetic (model_plan.cc), so a malformed file fails the same way with and without a GPU
    const int P = tp_size > 1 ? tp_size : 1, R = tp_size > 1 ? tp_rank : 0;
    LoadPlan plan;
    if (!plan_model(*m->file, tp_rank, tp_size, tp_active() && mi355::tp_size() == P && mi355::tp_rank() == R, *m, plan, err, status)) return nullptr;
    if (hipSetDevice(main_gpu) != hipSuccess) { err = "hipSetDevice failed"; status = -100; return nullptr; }
    m->device = main_gpu;
    if (!upload_tensors(*m, plan, err, status)) return nullptr;
    alias_tensors(*m);
    m->file_tensor_bytes = plan.file_tensor_bytes;
    m->device_bytes = plan.total;
    m->host_bytes = 0;
    if (!expand_prefill_planes(*m, prefill_planes, err, status)) return nullptr;
    m->bytes_per_token = plan.bytes_per_token;
    const HParams &hp = m->hp;
    char desc[256];
    snprintf(desc, sizeof desc, "%s %dL E%d H%d/%d FF%d V%d%s", hp.arch.c_str(), hp.n_layer, hp.n_embd, hp.n_head, hp.n_head_kv, hp.n_ff,
             hp.n_vocab, hp.n_expert ? " MoE" : "");
    m->desc = desc;
    return m.release();
}

// ------------------------------------------------------------------------------------------ context
Context::Context(Model *m, const ContextParams &p) : model(m), cp(p) {}

// the dispatches' own begin / end timestamps, by role (kernels.h KernelTimer): events are created on demand and reused from step to step
struct Context::KTimer : KernelTimer {
    struct Rec { const char *role; hipEvent_t a, b; };
    std::vector<Rec> pool;
    size_t used = 0;
    bool next(const char *role, hipEvent_t *start, hipEvent_t *stop) override {
        if (used == pool.size()) {
            Rec r{role, nullptr, nullptr};
            if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return false;
            pool.push_back(r);
        }
        Rec &r = pool[used++];
        r.role = role; *start = r.a; *stop = r.b;
        return true;
    }
    ~KTimer() override { for (auto &r : pool) { if (r.a) (void)hipEventDestroy(r.a); if (r.b) (void)hipEventDestroy(r.b); } }
};
Context::~Context() {
    if (holds_fused_) { (void)hipStreamSynchronize(stream_); fused_release(); }
    if (ktimer_) { if (kernel_timer() == ktimer_) set_kernel_timer(nullptr); delete ktimer_; ktimer_ = nullptr; }
    attn_probe_report();
    attn_out_probe_report();
    if (d_engine_probe_) {                                     // diagnosis: time line of the probed layer's last engine launch
        const int ncu = num_cu(), NW = 10, NS = 48;
        std::vector<unsigned long long> t((size_t)ncu * NW * NS);
        (void)hipDeviceSynchronize();
        if (hipMemcpy(t.data(), d_engine_probe_, t.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            if (const char *pf = getenv("MI355_ENGINE_PROBE_FILE")) {          // raw stamps [workgroup][wave][32] for tools/engine_probe.py
                if (FILE *f = fopen(pf, "wb")) { fwrite(t.data(), 8, t.size(), f); fclose(f); }
            }
            unsigned long long base = ~0ull;
            for (int w = 0; w < ncu * NW; w++) { const unsigned long long v = t[(size_t)w * NS]; if (v && v < base) base = v; }
            // kind 0: wall-clock stamp relative to the first wave; 1: a duration (10 ns ticks); 2: a count
            auto stat = [&](bool loader, int idx, const char *name, int kind = 0) {
                std::vector<double> v;
                for (int w = 0; w < ncu * NW; w++) {
                    if (loader != ((w % NW) < 2)) continue;
                    const unsigned long long x = t[(size_t)w * NS + idx];
                    if (kind == 0) { if (x) v.push_back((double)(long long)(x - base) * 0.01); }
                    else v.push_back(kind == 1 ? (double)x * 0.01 : (double)x);
                }
                if (v.empty()) return;
                std::sort(v.begin(), v.end());
                fprintf(stderr, "  %-52s n=%4zu  min %8.2f  med %8.2f  max %8.2f %s\n", name, v.size(), v.front(), v[v.size() / 2], v.back(), kind == 2 ? "" : "us");
            };
            fprintf(stderr, "engine probe, layer %d (us since the first wave entered):\n", engine_probe_layer_);
            stat(true, 0, "loader: enter"); stat(true, 1, "loader: go (consumers' requests queued)"); stat(true, 2, "loader: attn_output issued");
            stat(true, 3, "loader: gate|up issued"); stat(true, 4, "loader: down issued"); stat(true, 5, "loader: qkv issued"); stat(true, 6, "loader: all landed");
            stat(true, 12, "loader: attn_output polls waiting for landings", 2); stat(true, 13, "loader: attn_output polls waiting for ring space", 2);
            stat(true, 14, "loader: gate|up polls waiting for landings", 2); stat(true, 15, "loader: gate|up polls waiting for ring space", 2);
            stat(true, 16, "loader: down polls waiting for landings", 2); stat(true, 17, "loader: down polls waiting for ring space", 2);
            stat(true, 18, "loader: qkv polls waiting for landings", 2); stat(true, 19, "loader: qkv polls waiting for ring space", 2);
            stat(false, 0, "consumer: enter"); stat(false, 20, "consumer: attn_output activation ready"); stat(false, 21, "consumer: attn_output waiting for slots", 1);
            stat(false, 22, "consumer: attn_output decoding", 1); stat(false, 1, "consumer: attn_output decoded");
            stat(false, 32, "consumer: next described, norm weights requested");
            stat(false, 2, "consumer: x' gather starts"); stat(false, 3, "consumer: x' in LDS");
            stat(false, 34, "consumer: sum of squares done"); stat(false, 35, "consumer: rendezvous 1 passed"); stat(false, 36, "consumer: scale known");
            stat(false, 37, "consumer: blocks quantised");
            stat(false, 23, "consumer: gate|up activation ready"); stat(false, 24, "consumer: gate|up waiting for slots", 1); stat(false, 25, "consumer: gate|up decoding", 1);
            stat(false, 4, "consumer: gate|up decoded"); stat(false, 5, "last arriver: swiglu hand-over starts"); stat(false, 6, "last arriver: own blocks quantised + published");
            stat(false, 7, "consumer: codes in LDS"); stat(false, 26, "consumer: down activation ready"); stat(false, 27, "consumer: down waiting for slots", 1);
            stat(false, 28, "consumer: down decoding", 1); stat(false, 8, "consumer: down decoded"); stat(false, 9, "consumer: x'' gather starts");
            stat(false, 10, "consumer: x'' in LDS"); stat(false, 29, "consumer: qkv activation ready"); stat(false, 30, "consumer: qkv waiting for slots", 1);
            stat(false, 31, "consumer: qkv decoding", 1); stat(false, 11, "consumer: qkv decoded");
        }
    }
    if (d_mega_probe_) {                                       // diagnosis: where the last whole-step launch spent its time
        const int nl = model->hp.n_layer, np = 1 + MEGA_PROBES_PER_LAYER * nl;
        std::vector<unsigned long long> t((size_t)np);
        (void)hipDeviceSynchronize();
        if (hipMemcpy(t.data(), d_mega_probe_, (size_t)np * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            const char *names[MEGA_PROBES_PER_LAYER] = {"wait", "qkv", "wait", "attention", "wait", "wo", "wait", "gate_up", "wait", "down"};
            double sum[MEGA_PROBES_PER_LAYER] = {0};
            for (int il = 0; il < nl; il++)
                for (int k = 0; k < MEGA_PROBES_PER_LAYER; k++)
                    sum[k] += (double)(t[(size_t)(1 + il * MEGA_PROBES_PER_LAYER + k)] - t[(size_t)(il * MEGA_PROBES_PER_LAYER + k)]) * 0.01;
            fprintf(stderr, "mega probe (workgroup 0, us per layer):");
            for (int k = 0; k < MEGA_PROBES_PER_LAYER; k++) fprintf(stderr, " %s %.2f", names[k], sum[k] / nl);
            fprintf(stderr, " | total %.1f us\n", (double)(t[(size_t)np - 1] - t[0]) * 0.01);
        }
    }
    for (auto &ge : graphs_) (void)hipGraphExecDestroy(ge.second);
    if (stage_event_) (void)hipEventDestroy(stage_event_);
    for (auto &pe : prof_events_) (void)hipEventDestroy(pe.second);
    for (void *p : allocs_) (void)hipFree(p);
    if (h_stage_) (void)hipHostFree(h_stage_);
    if (h_logits_) (void)hipHostFree(h_logits_);
    if (h_argmax_) (void)hipHostFree(h_argmax_);
    if (h_embd_) (void)hipHostFree(h_embd_);
    if (h_chunks_) (void)hipHostFree(h_chunks_);
    if (h_mega_flag_) (void)hipHostFree(h_mega_flag_);
    if (h_topk_) (void)hipHostFree(h_topk_);
    if (h_topk_adj_) (void)hipHostFree(h_topk_adj_);
    if (h_spec_) (void)hipHostFree(h_spec_);
    if (h_lp_) (void)hipHostFree(h_lp_);
    if (d_topk_adj_) (void)hipFree(d_topk_adj_);
    if (topk_scratch_) { (void)hipFree(topk_scratch_); topk_scratch_ = nullptr; }
    if (h_moe_meta_) (void)hipHostFree(h_moe_meta_);
    if (stream_) (void)hipStreamDestroy(stream_);
}

void *Context::dalloc(size_t bytes) {
    void *p = nullptr;
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes == 0) bytes = 256;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    (void)hipMemset(p, 0, bytes);
    allocs_.push_back(p);
    device_bytes += bytes;
    return p;
}

static void alloc_actq(ActQuant &q, size_t K, size_t T, bool k, bool z, std::vector<void *> &track, uint64_t &tot, bool &ok) {
    auto al = [&](size_t b) -> void * {
        void *p = nullptr;
        b = (b + 255) & ~(size_t)255;
        if (hipMalloc(&p, b) != hipSuccess) { ok = false; return nullptr; }
        track.push_back(p);
        tot += b;
        return p;
    };
    if (k) {
        q.qs = (int8_t *)al(T * K);
        q.d = (float *)al(T * ((K + 255) / 256) * 4);         // (rounded up: a width that ends inside a 256-group never shrinks a plane)
        q.bsums = (int16_t *)al(T * ((K + 15) / 16) * 2);
    }
    if (z) {
        q.qs0 = (int8_t *)al(T * K);
        q.d0 = (uint16_t *)al(T * (K / 32) * 2);
    }
}

bool Context::init(std::string &err) {
    const HParams &hp = model->hp;
    if (hipSetDevice(model->device) != hipSuccess) { err = "hipSetDevice failed"; return false; }
    if (cp.n_ubatch > cp.n_batch) cp.n_ubatch = cp.n_batch;
    if (const char *ng = getenv("MI355_NO_GRAPHS")) { if (ng[0] == '1') cp.use_graphs = false; }   // e.g. under rocprofv3
    if (cp.n_ubatch == 0 || cp.n_ctx == 0) { err = "n_ctx / n_ubatch must be > 0"; return false; }
    if (cp.n_seq_max > 64) { err = "n_seq_max > 64 unsupported"; return false; }
    auto kv_ok = [](int t) { return t == T_F16 || t == T_Q8_0 || t == T_Q4_0; };
    if (!kv_ok(cp.type_k) || !kv_ok(cp.type_v)) { err = "unsupported KV cache type"; return false; }
    if (hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking) != hipSuccess) { err = "hipStreamCreate failed"; return false; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, model->device) == hipSuccess) set_num_cu(prop.multiProcessorCount);
    err_epoch_seen_ = stream_error_epoch();
    (void)install_stream_error_word();

    const size_t T = cp.n_ubatch, E = hp.n_embd, FF = hp.n_ff, G = hp.n_head_kv, D = hp.head_dim, NC = cp.n_ctx;
    cells_.assign(NC, KVCell());
    kv_.resize((size_t)hp.n_layer);
    auto plane_bytes = [&](int type, size_t &codes, size_t &scales) {
        if (type == T_F16) { codes = G * NC * D * 2; scales = 0; }
        else if (type == T_Q8_0) { codes = G * NC * D; scales = G * NC * (D / 32) * 2; }
        else { codes = G * NC * D / 2; scales = G * NC * (D / 32) * 2; }
    };
    for (int il = 0; il < hp.n_layer; il++) {
        size_t c, s;
        plane_bytes(cp.type_k, c, s);
        kv_[(size_t)il].k = (uint8_t *)dalloc(c);
        kv_[(size_t)il].kd = s ? (uint16_t *)dalloc(s) : nullptr;
        plane_bytes(cp.type_v, c, s);
        kv_[(size_t)il].v = (uint8_t *)dalloc(c);
        kv_[(size_t)il].vd = s ? (uint16_t *)dalloc(s) : nullptr;
        if (!kv_[(size_t)il].k || !kv_[(size_t)il].v) { err = "KV cache allocation failed"; return false; }
    }
    d_cell_pos_ = (int32_t *)dalloc(NC * 4);
    d_cell_seq_ = (uint64_t *)dalloc(NC * 8);
    d_delta_ = (int32_t *)dalloc(NC * 4);
    // token staging block: [nkv x4][tok][pos][seq][cell][outrow][seqmask]
    const size_t Tp = (T + 1) & ~(size_t)1;   // keeps the u64 seqmask array 8-byte aligned
    stage_bytes_ = 16 + Tp * 4 * 5 + Tp * 8;
    stage_bytes_ = (stage_bytes_ + 15) & ~(size_t)15;
    d_stage_ = (uint8_t *)dalloc(stage_bytes_);
    if (hipHostMalloc((void **)&h_stage_, stage_bytes_, hipHostMallocDefault) != hipSuccess) { err = "pinned alloc failed"; return false; }
    d_nkv_ = (int32_t *)d_stage_;
    d_tok_ = (int32_t *)(d_stage_ + 16);
    d_pos_ = d_tok_ + Tp;
    d_seq_ = d_pos_ + Tp;
    d_cell_ = d_seq_ + Tp;
    d_outrow_ = d_cell_ + Tp;
    d_seqmask_ = (uint64_t *)(d_outrow_ + Tp);

    // rows that hold Q or the attention output are H * D wide, which is n_embd for llama / qwen2 files, less on a row-split rank, and may be more for qwen3
    // (Qwen3-0.6B: 2048 against 1024; Qwen3-4B: 4096 against 2560).  q_ also takes E-wide results (the encoder's attn_output / ffn_down).
    const size_t QA = std::max(E, (size_t)hp.n_head * D);
    x_ = (float *)dalloc(T * E * 4);
    xn_ = (float *)dalloc(T * E * 4);
    q_ = (float *)dalloc(T * QA * 4);
    k_ = (float *)dalloc(T * G * D * 4);
    v_ = (float *)dalloc(T * G * D * 4);
    att_ = (float *)dalloc(T * QA * 4);
    ffn_ = (float *)dalloc(T * FF * 4);
    ffn_u_ = (float *)dalloc(T * FF * 4);
    xo_ = (float *)dalloc(T * E * 4);
    xb_ = (uint16_t *)dalloc(T * std::max({E, FF, QA}) * 2);     // the rows of a contraction against a bf16 tensor, rounded to bf16 (widest: n_embd, n_ff or H * D)
    if (hp.tp_exchange) {
        if (!tp_active() || tp_size() != hp.tp_size || tp_rank() != hp.tp_rank) { err = "model was loaded as rank " + std::to_string(hp.tp_rank) + " of " + std::to_string(hp.tp_size) + " but the process has no matching row-split group (mi355_tp_init)"; return false; }
        tp_part_ = (float *)dalloc(T * E * 4);
        if (tp_uses_host()) cp.use_graphs = false;     // the host transport drains the stream inside the step
        if (const char *tg = getenv("MI355_TP_GRAPHS")) { if (tg[0] == '0') cp.use_graphs = false; }
    }
    if (hp.n_expert > 0) {
        router_ = (float *)dalloc(T * hp.n_expert * 4);
        moe_ids_ = (int32_t *)dalloc(T * hp.n_expert_used * 4);
        moe_w_ = (float *)dalloc(T * hp.n_expert_used * 4);
        moe_out_ = (float *)dalloc((size_t)hp.n_expert_used * T * E * 4);
        if (T >= 8) {                                              // grouped-by-expert batches of a prompt (run_layers)
            const size_t GR = (size_t)hp.n_expert_used * T;
            bool okg = true;
            alloc_actq(aq_eg_, E, GR, true, true, allocs_, device_bytes, okg);
            alloc_actq(aq_ffg_, FF, GR, true, true, allocs_, device_bytes, okg);
            ffn_g_ = (float *)dalloc(GR * FF * 4);
            ffn_ug_ = (float *)dalloc(GR * FF * 4);
            y_g_ = (float *)dalloc(GR * E * 4);
            moe_meta_ = (int32_t *)dalloc((size_t)(2 * hp.n_expert + 1) * 4);
            moe_slot_ = (int32_t *)dalloc(GR * 4);
            moe_tok_ = (int32_t *)dalloc(GR * 4);
            if (!okg || !ffn_g_ || !ffn_ug_ || !y_g_ || !moe_tok_ ||
                hipHostMalloc((void **)&h_moe_meta_, (size_t)(2 * hp.n_expert + 1) * 4, hipHostMallocDefault) != hipSuccess) { err = "MoE batch buffers allocation failed"; return false; }
        }
    }
    bool ok = true;
    alloc_actq(aq_e_, E, T, true, true, allocs_, device_bytes, ok);
    alloc_actq(aq_o_, QA, T, true, true, allocs_, device_bytes, ok);      // (the attention output's codes: attn_output contracts over H * D)
    alloc_actq(aq_ff_, FF, T, true, true, allocs_, device_bytes, ok);
    const int prep_rows = (int)T * (hp.n_expert > 0 ? std::max(1, (int)hp.n_expert_used) : 1);   // (expert batches: every (token, rank) pair is a row)
    mmq_bh_ = (int8_t *)dalloc(mmq_prep_bytes((int)std::max({E, FF, QA}), prep_rows));     // (block sums of the widest contraction: n_embd, n_ff or H * D)
    mmq_bl_ = (int8_t *)dalloc(mmq_prep_bytes((int)std::max({E, FF, QA}), prep_rows));
    // partial sums of the K-split prompt contraction: only tensors with few rows split (Q | K | V, attention output, FFN down),
    // up to four ways; tensors that do not fit fall back to an unsplit kernel
    // A launch only splits while its 128 x 256 tiles number fewer than 3/4 of the CUs, and then into ceil(CUs / tiles) <= 4 parts (mmq.hip planes2_split):
    // n_split * tiles < CUs + tiles < 7/4 CUs, i.e. never more than 7/4 * CUs tiles' worth of partial sums whatever the model (58.7 MB on 256 CUs;
    // sized by the widest tensor instead it was 335 MB per context for Llama-3-70B at n_ubatch 2048)
    mmq_ws_.bytes = std::min((size_t)4 * T * std::max<size_t>(QA, (size_t)(hp.n_head + 2 * hp.n_head_kv) * D) * sizeof(float),
                             (size_t)(num_cu() * 7 / 4) * 128 * 256 * sizeof(float));
    mmq_ws_.p = T >= 128 ? (float *)dalloc(mmq_ws_.bytes) : nullptr;
    if (!mmq_ws_.p) mmq_ws_.bytes = 0;
    if (!ok || !x_ || !ffn_u_ || !xb_) { err = "activation buffer allocation failed"; return false; }

    size_t ws = 0;
    for (int t = 1; t <= (int)T; t++) {
        const int sp = flash_attn_pick_splits(t, (int)G, (int)NC);
        ws = std::max(ws, flash_attn_workspace_floats(t, hp.n_head, (int)D, sp));
    }
    ws = std::max(ws, flash_attn_workspace_floats(std::min<int>((int)T, 64), hp.n_head, (int)D, flash_attn_decode_splits((int)NC)));
    for (int t = 32; t <= (int)T; t += 32)                       // key splits of a prompt batch (fewer tokens take more splits)
        ws = std::max(ws, flash_attn_workspace_floats(t, hp.n_head, (int)D, flash_attn_prefill_splits(t, hp.n_head, (int)G, (int)D, (int)NC)));
    att_part_ = (float *)dalloc(ws * 4);
    att_part_floats_ = ws;
    att_counters_ = (unsigned *)dalloc(64 * ATT_SYNC_STRIDE * sizeof(unsigned));
    if (!att_part_ || !att_counters_) { err = "attention workspace allocation failed"; return false; }
    if (hipMemset(att_counters_, 0, 64 * ATT_SYNC_STRIDE * sizeof(unsigned)) != hipSuccess) { err = "hipMemset failed"; return false; }
    d_step_serial_ = (unsigned *)dalloc(64);
    d_ao_flags_ = (unsigned *)dalloc((size_t)std::max(1, hp.n_layer) * 64 * ATT_SYNC_STRIDE * sizeof(unsigned));
    d_ao_gran_ = (unsigned long long *)dalloc(attn_out_granule_words((int)(hp.n_head * D)) * 8);
    d_qkv_gran_ = (unsigned long long *)dalloc(qkv_attn_granule_words((int)(hp.n_head * D), (int)(hp.n_head_kv * D)) * 8);
    if (!d_step_serial_ || !d_ao_flags_ || !d_ao_gran_ || !d_qkv_gran_) { err = "step serial / flag allocation failed"; return false; }
    d_argmax_ = (int32_t *)dalloc(T * 4);
    argmax_scratch_ = (float *)dalloc(T * 129 * 4);     // T ticket words at the head, then per row 64 part values and 64 part indices (zero-filled: dalloc)
    rope_cs_ = (float *)dalloc(T * (size_t)hp.n_rot * 4);
    chunk_stride_ = (int)((NC + 63) / 64);
    d_chunks_ = (int32_t *)dalloc((size_t)64 * (chunk_stride_ + 1) * 4);
    if (hipHostMalloc((void **)&h_chunks_, (size_t)64 * (chunk_stride_ + 1) * 4, hipHostMallocDefault) != hipSuccess) { err = "pinned alloc failed"; return false; }
    d_embd_ = (float *)dalloc(T * E * 4);
    if (hipHostMalloc((void **)&h_embd_, T * E * 4, hipHostMallocDefault) != hipSuccess) { err = "pinned alloc failed"; return false; }
    if (hipHostMalloc((void **)&h_argmax_, T * 4, hipHostMallocDefault) != hipSuccess) { err = "pinned alloc failed"; return false; }
    embeddings_enabled = cp.embeddings || model->hp.encoder;      // an encoder has nothing but embeddings to give
    if (model->hp.encoder) {
        d_pos_open_ = (int32_t *)dalloc(T * 4);
        std::vector<int32_t> open((size_t)T, 0x7fffffff);
        if (!d_pos_open_ || hipMemcpy(d_pos_open_, open.data(), T * 4, hipMemcpyHostToDevice) != hipSuccess) { err = "encoder position buffer allocation failed"; return false; }
    }
    kv_clear();
    // the zero-fills above ran on the null stream, which the context's non-blocking stream does not wait for: drain them
    // before any kernel can touch these buffers (a late fill would wipe live KV rows; seen under rocprofv3 --pmc)
    if (hipDeviceSynchronize() != hipSuccess) { err = "device synchronise failed"; return false; }
    return true;
}

// ------------------------------------------------------------------------------------------ KV cells
// ---- the active adapters.  A change of the set or of a scale changes what the captured steps would have to launch: the stream is drained and they are dropped.
void Context::drop_captured_steps() {
    (void)hipSetDevice(model->device);
    (void)hipStreamSynchronize(stream_);
    if (holds_fused_) fused_release();
    for (auto &ge : graphs_) (void)hipGraphExecDestroy(ge.second);
    graphs_.clear();
    graph_exec_ = nullptr;
}

bool Context::lora_changed() {
    drop_captured_steps();
    if (!lora_.empty() && !lora_t_ && lora_scratch_floats((int)cp.n_ubatch) > 0) {
        lora_t_ = (float *)dalloc(lora_scratch_floats((int)cp.n_ubatch) * sizeof(float));
        if (!lora_t_) { lora_.clear(); last_error = "out of device memory for the adapter scratch"; return false; }
    }
    return true;
}

int Context::set_adapter_lora(LoraAdapter *a, float scale) {
    if (!a || a->model != model) { last_error = "the adapter was not loaded onto this context's model"; return -1; }
    bool found = false;
    for (ActiveLora &al : lora_) if (al.a == a) { al.scale = scale; found = true; }
    if (!found) lora_.push_back({a, scale});
    return lora_changed() ? 0 : -1;
}

int Context::rm_adapter_lora(LoraAdapter *a) {
    for (size_t i = 0; i < lora_.size(); i++)
        if (lora_[i].a == a) {
            lora_.erase(lora_.begin() + (long)i);
            (void)lora_changed();
            return 0;
        }
    last_error = "the adapter is not set on this context";
    return -1;
}

void Context::clear_adapter_lora() {
    if (lora_.empty()) return;
    lora_.clear();
    (void)lora_changed();
}

bool Context::lora_on(int layer, int target) const {
    for (const ActiveLora &al : lora_) if (al.a->find(layer, target)) return true;
    return false;
}

hipError_t Context::lora_add(int layer, const int *targets, float *const *outs, const int *lds, int n, const float *x, int ld_x, int K, int T) {
    bool any = false;
    for (const ActiveLora &al : lora_) {
        LoraSeg segs[3];
        int ns = 0;
        for (int i = 0; i < n && i < 3; i++)
            if (const LoraPair *p = al.a->find(layer, targets[i]))
                segs[ns++] = LoraSeg{p->A, p->B, p->type, p->r, (int)p->N, lora_scale(al.scale, al.a->alpha, p->r), outs[i], lds[i]};
        if (ns == 0) continue;
        HIP_TRY(launch_lora_delta(segs, ns, x, ld_x, K, T, lora_t_, stream_));
        any = true;
    }
    if (any) prof_mark("lora");
    return hipSuccess;
}

// ---- the control vector (runtime.h).  Every refusal comes before the first change: a refused call leaves the context as it was.
int Context::apply_cvec(const float *data, size_t len, int n_embd, int il_start, int il_end) {
    const HParams &hp = model->hp;
    if (hp.encoder) { last_error = "apply_cvec: an encoder model takes no control vector"; return -1; }
    if (hp.tp_size > 1) { last_error = "apply_cvec: not on a rank of a row split (load the model on one device)"; return -1; }
    if (!data) {                                                       // clear
        if (!cvec_on_) return 0;
        drop_captured_steps();
        cvec_on_ = false;
        std::fill(cvec_present_.begin(), cvec_present_.end(), (uint8_t)0);
        return 0;
    }
    if (n_embd != hp.n_embd) { last_error = "apply_cvec: n_embd " + std::to_string(n_embd) + " is not the model's " + std::to_string(hp.n_embd); return -1; }
    if (len % (size_t)n_embd) { last_error = "apply_cvec: len " + std::to_string(len) + " is not a multiple of n_embd " + std::to_string(n_embd); return -1; }
    if (il_start > il_end) { last_error = "apply_cvec: il_start " + std::to_string(il_start) + " > il_end " + std::to_string(il_end); return -1; }
    if (n_embd % 32) { last_error = "apply_cvec: n_embd is no multiple of 32"; return -1; }
    const size_t E = (size_t)n_embd, n_have = std::min(len / E, (size_t)std::max(0, hp.n_layer - 1));      // vectors of layers 1 .. n_have
    for (size_t i = 0; i < len; i++)
        if (!std::isfinite(data[i])) { last_error = "apply_cvec: the vector of layer " + std::to_string(i / E + 1) + " holds a non-finite value"; return -1; }
    if (hipSetDevice(model->device) != hipSuccess) { last_error = "apply_cvec: cannot select the device"; return -1; }
    drop_captured_steps();
    if (!cvec_) {
        cvec_ = (float *)dalloc((size_t)hp.n_layer * E * sizeof(float));       // (zero-filled)
        if (!cvec_) { last_error = "apply_cvec: out of device memory for the vectors"; return -1; }
        (void)hipDeviceSynchronize();                                          // the null-stream zero-fill (see init)
    }
    if (n_have && hipMemcpy(cvec_ + E, data, n_have * E * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        cvec_on_ = false; last_error = "apply_cvec: the copy to the device failed"; return -1;
    }
    cvec_present_.assign((size_t)hp.n_layer, (uint8_t)0);
    for (size_t il = 1; il <= n_have; il++) cvec_present_[il] = 1;
    cvec_start_ = il_start; cvec_end_ = il_end;
    cvec_on_ = true;
    return 0;
}

// layer il's vector onto its completed rows, where it has one inside the range
hipError_t Context::cvec_add(int il, int T) {
    if (!cvec_on_ || il < 1 || il < cvec_start_ || il > cvec_end_ || !cvec_present_[(size_t)il]) return hipSuccess;
    HIP_TRY(launch_add_row_vec(x_, cvec_ + (size_t)il * model->hp.n_embd, model->hp.n_embd, T, stream_));
    prof_mark("cvec");
    return hipSuccess;
}

// ---- importance-matrix collection (runtime.h).  begin lays out one device block: every accumulator's f32 [n_mat][K] rows, then every
// int32 [n_mat] count, then a slab scratch that holds any launch of up to a micro-batch's rows (imatrix_scratch_floats: the largest batch does not need the most slabs).
int Context::imatrix_begin(bool process_output) {
    const HParams &hp = model->hp;
    if (imx_on_) { last_error = "imatrix_begin: collection is already on (imatrix_end first)"; return -1; }
    if (hp.encoder) { last_error = "imatrix_begin: an encoder model is not collected (its blocks have no route that keeps the f32 rows)"; return -1; }
    if (hp.tp_size > 1) { last_error = "imatrix_begin: not on a rank of a row split (a rank sees a slice of every contraction)"; return -1; }
    const bool moe = hp.n_expert > 0;
    const int E = hp.n_embd, FF = hp.n_ff, NE = hp.n_expert, T = (int)cp.n_ubatch, GR = T * std::max(1, hp.n_expert_used);
    if (moe) {
        const LayerWeights &L0 = model->layers[0];
        if (!aq_eg_.qs || !moe_meta_ || !moe_tok_) { last_error = "imatrix_begin: this context has no grouped-expert buffers (n_ubatch < 8): the per-expert rows exist only on the grouped route"; return -1; }
        if (!(type_is_quant(L0.gate_exps.type) && type_is_quant(L0.up_exps.type) && type_is_quant(L0.down_exps.type))) { last_error = "imatrix_begin: float expert tensors never take the grouped route the collector reads"; return -1; }
        if (NE > 256 || GR > IMX_MAX_ROWS) { last_error = "imatrix_begin: more experts or grouped rows than the collector takes"; return -1; }
    }
    if (hipSetDevice(model->device) != hipSuccess) { last_error = "imatrix_begin: cannot select the device"; return -1; }
    std::vector<ImxAcc> acc((size_t)hp.n_layer * IMX_SLOTS + 1);
    std::vector<ImxName> names;
    size_t slab_floats = 0;
    bool widths_ok = true;
    auto site = [&](int idx, int K, int n_mat, int rows, std::initializer_list<const DevTensor *> ws) {
        acc[(size_t)idx].K = K; acc[(size_t)idx].n_mat = n_mat;
        if (K < 32 || (K & 31)) widths_ok = false;
        slab_floats = std::max(slab_floats, imatrix_scratch_floats(K, rows, n_mat));
        for (const DevTensor *w : ws) names.push_back({w->name, idx});
    };
    for (int il = 0; il < hp.n_layer; il++) {
        const LayerWeights &L = model->layers[(size_t)il];
        const int b = il * IMX_SLOTS;
        site(b + IMX_QKV, E, 1, T, {&L.wq, &L.wk, &L.wv});
        site(b + IMX_O, (int)L.wo.K, 1, T, {&L.wo});
        if (moe) {
            site(b + IMX_ROUTER, E, 1, T, {&L.gate_inp});
            site(b + IMX_FFN_IN, E, NE, GR, {&L.gate_exps, &L.up_exps});
            site(b + IMX_FFN_DOWN, FF, NE, GR, {&L.down_exps});
        } else {
            site(b + IMX_FFN_IN, E, 1, T, {&L.gate, &L.up});
            site(b + IMX_FFN_DOWN, FF, 1, T, {&L.down});
        }
    }
    if (process_output) site(hp.n_layer * IMX_SLOTS, E, 1, T, {!model->output.name.empty() ? &model->output : &model->tok_embd});
    if (!widths_ok) { last_error = "imatrix_begin: a projection's row length is no multiple of 32"; return -1; }
    size_t sum_floats = 0, n_counts = 0;
    for (const ImxAcc &a : acc) { sum_floats += (size_t)a.K * a.n_mat; n_counts += (size_t)a.n_mat; }
    const size_t acc_bytes = (sum_floats * 4 + n_counts * 4 + 255) & ~(size_t)255;
    drop_captured_steps();                                             // (as a change of the adapter set does: no captured step outlives a change of routes)
    const uint64_t before = device_bytes;
    imx_block_ = (uint8_t *)dalloc(acc_bytes + slab_floats * 4);       // (zero-filled)
    if (!imx_block_) { last_error = "imatrix_begin: out of device memory for the accumulators"; return -1; }
    (void)hipDeviceSynchronize();                                      // the null-stream zero-fill (see init)
    imx_block_bytes_ = (size_t)(device_bytes - before);
    imx_acc_bytes_ = acc_bytes;
    float *fp = reinterpret_cast<float *>(imx_block_);
    int32_t *ip = reinterpret_cast<int32_t *>(imx_block_ + sum_floats * 4);
    for (ImxAcc &a : acc) {
        if (a.K == 0) continue;
        a.sum2 = fp; fp += (size_t)a.K * a.n_mat;
        a.count = ip; ip += a.n_mat;
    }
    imx_slabs_ = reinterpret_cast<float *>(imx_block_ + acc_bytes);
    imx_slab_floats_ = slab_floats;
    imx_acc_ = std::move(acc);
    imx_names_ = std::move(names);
    imx_output_ = process_output;
    imx_on_ = true;
    return 0;
}

int Context::imatrix_end() {
    if (!imx_on_) { last_error = "imatrix_end: collection is not on"; return -1; }
    (void)hipSetDevice(model->device);
    (void)hipStreamSynchronize(stream_);
    (void)hipFree(imx_block_);
    allocs_.erase(std::find(allocs_.begin(), allocs_.end(), (void *)imx_block_));
    device_bytes -= imx_block_bytes_;
    imx_block_ = nullptr; imx_slabs_ = nullptr; imx_block_bytes_ = imx_acc_bytes_ = imx_slab_floats_ = 0;
    imx_acc_.clear(); imx_names_.clear();
    imx_on_ = imx_output_ = false;
    return 0;
}

int Context::imatrix_clear() {
    if (!imx_on_) { last_error = "imatrix_clear: collection is not on"; return -1; }
    if (hipSetDevice(model->device) != hipSuccess || hipMemsetAsync(imx_block_, 0, imx_acc_bytes_, stream_) != hipSuccess ||
        hipStreamSynchronize(stream_) != hipSuccess) { last_error = "imatrix_clear: zero-fill failed"; return -1; }
    return 0;
}

bool Context::imatrix_entry(int i, std::string &name, int &ne0, int &n_mat) const {
    if (i < 0 || i >= (int)imx_names_.size()) return false;
    const ImxAcc &a = imx_acc_[(size_t)imx_names_[(size_t)i].acc];
    name = imx_names_[(size_t)i].name; ne0 = a.K; n_mat = a.n_mat;
    return true;
}

int Context::imatrix_get(int i, float *sum2, int32_t *counts) {
    if (!imx_on_ || i < 0 || i >= (int)imx_names_.size() || !sum2 || !counts) { last_error = "imatrix_get: collection is not on, or no such entry"; return -1; }
    const ImxAcc &a = imx_acc_[(size_t)imx_names_[(size_t)i].acc];
    const size_t n = (size_t)a.K * a.n_mat;
    if (hipSetDevice(model->device) != hipSuccess || hipStreamSynchronize(stream_) != hipSuccess || !mega_check() || !stream_check()) return -1;
    if (hipMemcpy(sum2, a.sum2, n * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(counts, a.count, (size_t)a.n_mat * 4, hipMemcpyDeviceToHost) != hipSuccess) {
        last_error = "imatrix_get: copy failed"; return -1;
    }
    for (size_t j = 0; j < n; j++)
        if (!(sum2[j] >= 0.0f && sum2[j] < INFINITY)) {      // (llama-imatrix aborts on it: the file would poison a quantisation)
            last_error = "imatrix_get: non-finite sum in " + imx_names_[(size_t)i].name + " (matrix " + std::to_string(j / (size_t)a.K) + ", column " + std::to_string(j % (size_t)a.K) + ")";
            return -1;
        }
    return 0;
}

hipError_t Context::imx_collect(int il, int slot, const float *x, const float *x2, int K, int R, const int32_t *row_src, const int32_t *meta) {
    const ImxAcc &a = imx_acc_[il < 0 ? (size_t)model->hp.n_layer * IMX_SLOTS : (size_t)il * IMX_SLOTS + (size_t)slot];
    if (a.K != K || !a.sum2) return hipErrorInvalidValue;
    prof_mark("rows");                                // (the launches since the last mark produced the rows: their time is not the collector's)
    HIP_TRY(launch_imatrix_accum(x, x2, K, K, R, row_src, meta, a.n_mat, a.sum2, a.count, imx_slabs_, imx_slab_floats_, stream_));
    prof_mark(x2 ? "imatrix_glu" : "imatrix");       // (the producer form has a role of its own: it tells which grouped-expert form fed ffn_down_exps)
    return hipSuccess;
}

void Context::kv_clear() {
    for (auto &c : cells_) c = KVCell();
    head_ = 0;
    has_shift_ = false;
    meta_dirty_ = true;
    region_next_.clear();
}
bool Context::kv_seq_rm(int seq, int p0, int p1) {
    if (seq >= 64) return false;                                   // (the cell masks are 64 bits wide)
    if (p0 < 0) p0 = 0;
    if (p1 < 0) p1 = 0x7fffffff;
    int new_head = (int)cells_.size();
    for (int i = 0; i < (int)cells_.size(); i++) {
        KVCell &c = cells_[(size_t)i];
        if (c.pos < p0 || c.pos >= p1) continue;
        if (seq < 0) c.seqs = 0;
        else if (c.seqs & (1ull << seq)) c.seqs &= ~(1ull << seq);
        else continue;
        if (!c.seqs) { c.pos = -1; c.delta = 0; if (i < new_head) new_head = i; }
    }
    if (new_head < (int)cells_.size() && new_head < head_) head_ = new_head;
    if (new_head < (int)cells_.size()) region_next_.clear();   // cells came free: the next allocation starts at its region's lowest free cell
    meta_dirty_ = true;
    return true;
}
void Context::kv_seq_cp(int src, int dst, int p0, int p1) {
    if (src == dst || src < 0 || dst < 0 || src >= 64 || dst >= 64) return;
    if (p0 < 0) p0 = 0;
    if (p1 < 0) p1 = 0x7fffffff;
    for (auto &c : cells_)
        if ((c.seqs & (1ull << src)) && c.pos >= p0 && c.pos < p1) c.seqs |= 1ull << dst;
    meta_dirty_ = true;
}
void Context::kv_seq_add(int seq, int p0, int p1, int delta) {
    if (seq < 0 || seq >= 64) return;
    if (p0 < 0) p0 = 0;
    if (p1 < 0) p1 = 0x7fffffff;
    if (p0 == p1 || delta == 0) return;
    for (auto &c : cells_) {
        if (!(c.seqs & (1ull << seq)) || c.pos < p0 || c.pos >= p1) continue;
        has_shift_ = true;
        c.pos += delta;
        c.delta += delta;
        if (c.pos < 0) { c.pos = -1; c.seqs = 0; c.delta = 0; region_next_.clear(); }
    }
    meta_dirty_ = true;
}
int Context::kv_used_cells() const {
    int n = 0;
    for (const auto &c : cells_) n += c.pos >= 0;
    return n;
}

int Context::find_slot(int n) {
    const int NC = (int)cells_.size();
    if (n > NC) return -1;
    int head = head_, tested = 0;
    while (true) {
        if (head + n > NC) { tested += NC - head; head = 0; if (tested >= NC) return -1; continue; }
        bool ok = true;
        for (int i = 0; i < n; i++)
            if (cells_[(size_t)(head + i)].pos >= 0) { ok = false; head += i + 1; tested += i + 1; break; }
        if (ok) return head;
        if (tested >= NC) return -1;
    }
}

bool Context::alloc_cells(int n, const uint64_t *seqmask, std::vector<int> &out) {
    out.assign((size_t)n, -1);
    const int NC = (int)cells_.size();
    const int NS = (int)cp.n_seq_max;
    if (NS <= 1) {                                              // one sequence: a contiguous run, as before
        const int slot = find_slot(n);
        if (slot < 0) return false;
        for (int i = 0; i < n; i++) out[(size_t)i] = slot + i;
        head_ = slot + n;
        if (head_ >= NC) head_ = 0;
        return true;
    }
    // every sequence owns a region of the cache, a whole number of 64-cell attention chunks where the cache allows it: a
    // sequence then sees the same chunk partition whichever region it lives in (results do not depend on the slot), and
    // the hint below always points at the region's lowest free cell, so allocation is a pure function of the cell table
    int R = std::max(1, NC / NS);
    if (R >= 64) R &= ~63;
    if ((int)region_next_.size() != NS) { region_next_.assign((size_t)NS, 0); for (int s = 0; s < NS; s++) region_next_[(size_t)s] = s * R; }
    std::vector<char> taken((size_t)NC, 0);                    // cells handed out within this call
    auto is_free = [&](int c) { return cells_[(size_t)c].pos < 0 && !taken[(size_t)c]; };
    for (int i = 0; i < n; i++) {
        int s = seqmask[i] ? __builtin_ctzll(seqmask[i]) : 0;
        if (s >= NS) s = NS - 1;
        const int lo = s * R, hi = (s == NS - 1) ? NC : lo + R;
        int c = -1;
        int start = region_next_[(size_t)s];
        if (start < lo || start >= hi) start = lo;
        for (int k = 0; k < hi - lo; k++) {                    // own region first, from where the last cell went
            int cand = start + k;
            if (cand >= hi) cand -= hi - lo;
            if (is_free(cand)) { c = cand; break; }
        }
        if (c < 0) for (int cand = 0; cand < NC; cand++) if (is_free(cand)) { c = cand; break; }   // region full: anywhere
        if (c < 0) return false;
        taken[(size_t)c] = 1;
        out[(size_t)i] = c;
        if (c >= lo && c < hi) region_next_[(size_t)s] = c + 1;
    }
    return true;
}

void Context::apply_k_shift() {
    const HParams &hp = model->hp;
    std::vector<int32_t> delta(cells_.size());
    for (size_t i = 0; i < cells_.size(); i++) { delta[i] = cells_[i].delta; cells_[i].delta = 0; }
    (void)hipMemcpyAsync(d_delta_, delta.data(), delta.size() * 4, hipMemcpyHostToDevice, stream_);
    (void)hipStreamSynchronize(stream_);
    RopeArgs ra = rope_args(*model, true);
    for (int il = 0; il < hp.n_layer; il++)
        (void)launch_k_shift(kv_[(size_t)il], cp.type_k, hp.n_head_kv, hp.head_dim, (int)cp.n_ctx, d_delta_, ra, stream_);
    has_shift_ = false;
}

// ------------------------------------------------------------------------------------------ a sequence's state (llama_state_seq_*; runtime.h)
namespace {
size_t g_state_stage_max = (size_t)64 << 20;             // device staging of the portable rows: a long sequence goes through it in chunks of cells
struct EventPair {                                        // state_timing: one launch / copy between two events of its own
    hipEvent_t a = nullptr, b = nullptr;
    bool on;
    explicit EventPair(bool enable) : on(enable) { if (on && (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess)) on = false; }
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    void begin(hipStream_t st) { if (on) (void)hipEventRecord(a, st); }
    void end(hipStream_t st, float &acc) {
        if (!on) return;
        float ms = 0.0f;
        if (hipEventRecord(b, st) == hipSuccess && hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess) acc += ms;
    }
};
}  // namespace

void set_state_stage_max(size_t bytes) { g_state_stage_max = bytes ? bytes : (size_t)64 << 20; }   // tests: contexts that have not moved a state yet chunk at this size

const char *Context::state_refusal() const {
    if (model->hp.encoder) return "an encoder context has no KV cache, so no sequence state";
    if (model->hp.tp_size > 1) return "a rank of a row split holds a slice of every KV row, so no sequence state (load the model on one device)";
    return nullptr;
}
size_t Context::state_cell_bytes() const {
    const HParams &hp = model->hp;
    return (size_t)hp.n_layer * (kv_state_row_bytes(cp.type_k, hp.n_head_kv, hp.head_dim) + kv_state_row_bytes(cp.type_v, hp.n_head_kv, hp.head_dim));
}
size_t Context::state_seq_size(int seq) const {
    if (state_refusal() || seq < 0 || seq >= 64) return 0;
    size_t n = 0;
    for (const KVCell &c : cells_) n += (c.pos >= 0 && (c.seqs & (1ull << seq))) ? 1 : 0;
    return STATE_HEADER_BYTES + 4 * n + n * state_cell_bytes();
}
bool Context::state_prepare() {
    if (d_state_stage_) return true;
    const size_t per = state_cell_bytes();
    state_stage_bytes_ = std::max(per, std::min(g_state_stage_max, per * (size_t)cp.n_ctx));
    uint8_t *stage = (uint8_t *)dalloc(state_stage_bytes_);
    d_state_cells_ = (int32_t *)dalloc((size_t)cp.n_ctx * 4);
    d_state_layers_ = (KVLayerView *)dalloc(kv_.size() * sizeof(KVLayerView));
    if (!stage || !d_state_cells_ || !d_state_layers_ ||
        hipMemcpy(d_state_layers_, kv_.data(), kv_.size() * sizeof(KVLayerView), hipMemcpyHostToDevice) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {               // (the zero-fills of dalloc ran on the null stream: see init)
        last_error = "sequence state: staging allocation failed";
        return false;
    }
    d_state_stage_ = stage;
    return true;
}

size_t Context::state_seq_get(int seq, uint8_t *dst, size_t cap) {
    if (const char *why = state_refusal()) { last_error = std::string("state_seq_get: ") + why; return 0; }
    if (seq < 0 || seq >= 64) { last_error = "state_seq_get: seq id " + std::to_string(seq) + " out of range [0, 64)"; return 0; }
    if (hipSetDevice(model->device) != hipSuccess) { last_error = "state_seq_get: hipSetDevice failed"; return 0; }
    if (has_shift_) apply_k_shift();                           // the blob holds K as rotated for the positions it records
    const HParams &hp = model->hp;
    std::vector<std::pair<int32_t, int32_t>> pc;               // (position, cell)
    for (size_t i = 0; i < cells_.size(); i++)
        if (cells_[i].pos >= 0 && (cells_[i].seqs & (1ull << seq))) pc.emplace_back(cells_[i].pos, (int32_t)i);
    std::sort(pc.begin(), pc.end());
    const size_t n = pc.size(), per = state_cell_bytes(), need = STATE_HEADER_BYTES + 4 * n + n * per;
    if (!dst || cap < need) { last_error = "state_seq_get: a buffer of " + std::to_string(cap) + " bytes, sequence " + std::to_string(seq) + " needs " + std::to_string(need); return 0; }
    const uint32_t head[8] = {STATE_MAGIC, STATE_VERSION, (uint32_t)cp.type_k, (uint32_t)cp.type_v, (uint32_t)hp.n_layer, (uint32_t)hp.n_head_kv, (uint32_t)hp.head_dim, (uint32_t)n};
    memcpy(dst, head, sizeof head);
    std::vector<int32_t> cells(n);
    for (size_t i = 0; i < n; i++) { memcpy(dst + STATE_HEADER_BYTES + 4 * i, &pc[i].first, 4); cells[i] = pc[i].second; }
    if (n == 0) return need;
    if (!state_prepare()) return 0;
    const size_t rbk = kv_state_row_bytes(cp.type_k, hp.n_head_kv, hp.head_dim), rbv = kv_state_row_bytes(cp.type_v, hp.n_head_kv, hp.head_dim);
    uint8_t *rows = dst + STATE_HEADER_BYTES + 4 * n;
    state_ms_pack = state_ms_copy = 0.0f;
    EventPair ev(state_timing);
    hipError_t e = hipMemcpyAsync(d_state_cells_, cells.data(), n * 4, hipMemcpyHostToDevice, stream_);
    const size_t chunk = std::max<size_t>(1, state_stage_bytes_ / per);
    for (size_t off = 0; off < n && e == hipSuccess; off += chunk) {
        const size_t nc = std::min(chunk, n - off);
        ev.begin(stream_);
        e = launch_kv_state_pack(d_state_layers_, hp.n_layer, cp.type_k, cp.type_v, hp.n_head_kv, hp.head_dim, (int)cp.n_ctx, d_state_cells_ + off, (int)nc, d_state_stage_, stream_);
        ev.end(stream_, state_ms_pack);
        ev.begin(stream_);
        if (e == hipSuccess && nc == n) e = hipMemcpyAsync(rows, d_state_stage_, n * per, hipMemcpyDeviceToHost, stream_);     // one chunk: the staging block IS the row section
        else
            for (int il = 0; il < hp.n_layer && e == hipSuccess; il++) {
                const uint8_t *s = d_state_stage_ + (size_t)il * nc * (rbk + rbv);
                uint8_t *d = rows + (size_t)il * n * (rbk + rbv);
                e = hipMemcpyAsync(d + off * rbk, s, nc * rbk, hipMemcpyDeviceToHost, stream_);
                if (e == hipSuccess) e = hipMemcpyAsync(d + n * rbk + off * rbv, s + nc * rbk, nc * rbv, hipMemcpyDeviceToHost, stream_);
            }
        ev.end(stream_, state_ms_copy);
        if (e == hipSuccess) e = hipStreamSynchronize(stream_);          // the next chunk packs into the same block
    }
    if (e == hipSuccess) fused_release();                  // (the stream has just been drained)
    if (e != hipSuccess) { last_error = std::string("state_seq_get: ") + hipGetErrorString(e); return 0; }
    return need;
}

size_t Context::state_seq_set(int seq, const uint8_t *src, size_t len) {
    if (const char *why = state_refusal()) { last_error = std::string("state_seq_set: ") + why; return 0; }
    if (seq < 0 || seq >= 64) { last_error = "state_seq_set: seq id " + std::to_string(seq) + " out of range [0, 64)"; return 0; }
    if (!src || len < STATE_HEADER_BYTES) { last_error = "state_seq_set: truncated blob: " + std::to_string(src ? len : 0) + " bytes, the header alone has " + std::to_string(STATE_HEADER_BYTES); return 0; }
    const HParams &hp = model->hp;
    uint32_t head[8];
    memcpy(head, src, sizeof head);
    const char *names[7] = {"magic", "version", "type_k", "type_v", "n_layer", "n_head_kv", "head_dim"};
    const uint32_t want[7] = {STATE_MAGIC, STATE_VERSION, (uint32_t)cp.type_k, (uint32_t)cp.type_v, (uint32_t)hp.n_layer, (uint32_t)hp.n_head_kv, (uint32_t)hp.head_dim};
    for (int i = 0; i < 7; i++)
        if (head[i] != want[i]) { last_error = std::string("state_seq_set: ") + names[i] + " mismatch: the blob has " + std::to_string(head[i]) + ", the context has " + std::to_string(want[i]); return 0; }
    const size_t n = head[7], per = state_cell_bytes();
    // the sequence's region (alloc_cells): the whole cache for a single-sequence context
    const int NC = (int)cells_.size(), NS = (int)cp.n_seq_max;
    size_t region = (size_t)NC;
    if (NS > 1) {
        int R = std::max(1, NC / NS);
        if (R >= 64) R &= ~63;
        const int s = std::min(seq, NS - 1);
        region = (size_t)(s == NS - 1 ? NC - s * R : R);
    }
    if (n > region) { last_error = "state_seq_set: n mismatch: the blob has " + std::to_string(n) + " cells, the region of sequence " + std::to_string(seq) + " has " + std::to_string(region); return 0; }
    const size_t need = STATE_HEADER_BYTES + 4 * n + n * per;
    if (len < need) { last_error = "state_seq_set: truncated blob: " + std::to_string(len) + " bytes, its header asks for " + std::to_string(need); return 0; }
    std::vector<int32_t> pos(n);
    if (n) memcpy(pos.data(), src + STATE_HEADER_BYTES, 4 * n);
    for (size_t i = 0; i < n; i++) {
        if (pos[i] < 0) { last_error = "state_seq_set: negative position " + std::to_string(pos[i]) + " at index " + std::to_string(i); return 0; }
        if (i && pos[i] <= pos[i - 1]) { last_error = "state_seq_set: positions not ascending at index " + std::to_string(i) + ": " + std::to_string(pos[i - 1]) + " then " + std::to_string(pos[i]); return 0; }
    }
    const uint64_t bit = 1ull << seq;
    size_t avail = 0;                                          // free cells, and cells nothing but this sequence holds
    for (const KVCell &c : cells_) avail += (c.pos < 0 || c.seqs == bit) ? 1 : 0;
    if (n > avail) { last_error = "state_seq_set: no cells: the blob has " + std::to_string(n) + ", the cache can free " + std::to_string(avail); return 0; }
    if (hipSetDevice(model->device) != hipSuccess) { last_error = "state_seq_set: hipSetDevice failed"; return 0; }
    // from here on the destination is rewritten: whatever goes wrong leaves it empty
    kv_seq_rm(seq, -1, -1);
    region_next_.clear();                                      // the region's lowest free cells first: a pure function of the cell table
    meta_dirty_ = true;
    if (n == 0) return need;
    std::vector<uint64_t> masks(n, bit);
    std::vector<int> got;
    if (!alloc_cells((int)n, masks.data(), got)) { last_error = "state_seq_set: no cells: the cache has no room for " + std::to_string(n); return 0; }
    if (!state_prepare()) return 0;
    const size_t rbk = kv_state_row_bytes(cp.type_k, hp.n_head_kv, hp.head_dim), rbv = kv_state_row_bytes(cp.type_v, hp.n_head_kv, hp.head_dim);
    const uint8_t *rows = src + STATE_HEADER_BYTES + 4 * n;
    std::vector<int32_t> cells(got.begin(), got.end());
    state_ms_unpack = 0.0f;
    EventPair ev(state_timing);
    hipError_t e = hipMemcpyAsync(d_state_cells_, cells.data(), n * 4, hipMemcpyHostToDevice, stream_);
    const size_t chunk = std::max<size_t>(1, state_stage_bytes_ / per);
    for (size_t off = 0; off < n && e == hipSuccess; off += chunk) {
        const size_t nc = std::min(chunk, n - off);
        if (nc == n) e = hipMemcpyAsync(d_state_stage_, rows, n * per, hipMemcpyHostToDevice, stream_);
        else
            for (int il = 0; il < hp.n_layer && e == hipSuccess; il++) {
                uint8_t *d = d_state_stage_ + (size_t)il * nc * (rbk + rbv);
                const uint8_t *s = rows + (size_t)il * n * (rbk + rbv);
                e = hipMemcpyAsync(d, s + off * rbk, nc * rbk, hipMemcpyHostToDevice, stream_);
                if (e == hipSuccess) e = hipMemcpyAsync(d + nc * rbk, s + n * rbk + off * rbv, nc * rbv, hipMemcpyHostToDevice, stream_);
            }
        ev.begin(stream_);
        if (e == hipSuccess)
            e = launch_kv_state_unpack(d_state_layers_, hp.n_layer, cp.type_k, cp.type_v, hp.n_head_kv, hp.head_dim, (int)cp.n_ctx, d_state_cells_ + off, (int)nc, d_state_stage_, stream_);
        ev.end(stream_, state_ms_unpack);
        if (e == hipSuccess) e = hipStreamSynchronize(stream_);          // the next chunk is copied into the same block
    }
    if (e == hipSuccess) fused_release();                  // (the stream has just been drained)
    if (e != hipSuccess) { last_error = std::string("state_seq_set: ") + hipGetErrorString(e); return 0; }
    for (size_t i = 0; i < n; i++) {
        KVCell &c = cells_[(size_t)got[i]];
        c.pos = pos[i]; c.seqs = bit; c.delta = 0;
    }
    meta_dirty_ = true;
    return need;
}

// ------------------------------------------------------------------------------------------ profiling
void Context::prof_begin() {
    if (!profile_) return;
    for (auto &pe : prof_events_) (void)hipEventDestroy(pe.second);
    prof_events_.clear();
    if (!ktimer_) ktimer_ = new KTimer;
    ktimer_->used = 0;
    set_kernel_timer(ktimer_);
    prof_mark("begin");
}
void Context::prof_mark(const char *name) {
    if (!profile_) return;
    hipEvent_t ev;
    if (hipEventCreate(&ev) != hipSuccess) return;
    (void)hipEventRecord(ev, stream_);
    prof_events_.emplace_back(name, ev);
}
void Context::prof_end() {
    if (!profile_) return;
    set_kernel_timer(nullptr);
    (void)hipStreamSynchronize(stream_);
    last_profile_.clear();
    if (ktimer_) {     // "k:<role>" = sum of the role's kernel durations in this step, "n:<role>" = its launches
        for (size_t i = 0; i < ktimer_->used; i++) {
            const KTimer::Rec &r = ktimer_->pool[i];
            float ms = 0;
            if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) continue;
            const std::string kn = std::string("k:") + r.role, nn = std::string("n:") + r.role;
            bool fk = false, fn = false;
            for (auto &e : last_profile_) { if (e.name == kn) { e.us += ms * 1000.0f; fk = true; } else if (e.name == nn) { e.us += 1.0f; fn = true; } }
            if (!fk) last_profile_.push_back({kn, ms * 1000.0f});
            if (!fn) last_profile_.push_back({nn, 1.0f});
        }
    }
    for (size_t i = 1; i < prof_events_.size(); i++) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, prof_events_[i - 1].second, prof_events_[i].second);
        bool found = false;
        for (auto &e : last_profile_)
            if (e.name == prof_events_[i].first) { e.us += ms * 1000.0f; found = true; break; }
        if (!found) last_profile_.push_back({prof_events_[i].first, ms * 1000.0f});
    }
}

// ------------------------------------------------------------------------------------------ linear layers

MMVQSeg make_seg(const DevTensor &w, float *out, int ld_out, const float *resid, const int32_t *esel) {
    MMVQSeg s{};
    s.W = w.data; s.out = out; s.resid = resid; s.type = w.type; s.n_rows = (int)w.N; s.ld_out = ld_out; s.row_bytes = w.row_bytes;
    s.expert_sel = esel; s.expert_stride = w.row_bytes * (size_t)w.N;
    return s;
}

static void chunk_act(MMVQArgs &a, const ActQuant &aq, int K, int t0) {
    a.aq = aq.qs ? aq.qs + (size_t)t0 * K : nullptr;
    a.ad = aq.d ? aq.d + (size_t)t0 * (K / 256) : nullptr;
    a.abs = aq.bsums ? aq.bsums + (size_t)t0 * (K / 16) : nullptr;
    a.aq0 = aq.qs0 ? aq.qs0 + (size_t)t0 * K : nullptr;
    a.ad0 = aq.d0 ? aq.d0 + (size_t)t0 * (K / 32) : nullptr;
}

// a single-token mat-vec launch's description without its segments: the activation codes, the epilogue, the fused activation prologue (Fuse::mode)
MMVQArgs single_token_desc(int n_seg, int K, int epi, int fuse, const float *nx, const float *nw, float eps, const ActQuant &aq) {
    MMVQArgs a{};
    a.n_seg = n_seg; a.K = K; a.T = 1; a.epi = epi;
    a.fuse_mode = fuse; a.nx = nx; a.nw = nw; a.neps = eps;
    chunk_act(a, aq, K, 0);
    return a;
}

// up to 3 quantised weight tensors sharing one activation (fused Q/K/V), or one tensor with an epilogue
// (any whole number of super-blocks: the prologues of the register ring and of the weight stream stop at the row's end inside the last pass, so hidden sizes
// like Qwen2-7B's 3584 and Llama-30B's 6656 - 14 and 26 super-blocks - stream too: mmvq_stream_applicable, tests/test_gpu_matvec_step.py k3584_* / k6656_*)
// (a width that is no multiple of 256 - whole 32-element blocks, so every quantised tensor over it takes Q8_0 activations - goes to the generic mat-vec,
// whose prologue takes a row that ends inside a 256-group: a step of such a file has as many launches as any other on that path)
static bool can_fuse(int K, int T) { return T == 1 && K <= 8192 && (K & 31) == 0; }

void MMVQTrace::note(const MMVQArgs &a) {
    Rec r{};
    r.T = a.T; r.kernel = mmvq_kernel_choice(a);
    if (r.kernel == MMVQ_KERNEL_STREAM) r.form = mmvq_stream_form(a);
    recs.push_back(r);
}

hipError_t mmvq_tokens(MMVQSeg *segs, int n_seg, int K, int T, int epi, const ActQuant &aq, hipStream_t st, const Fuse &fz, MMVQTrace *trace) {
    for (int t0 = 0; t0 < T;) {
        const int rem = T - t0, nt = rem >= 16 ? 16 : rem >= 8 ? 8 : rem >= 4 ? 4 : rem >= 2 ? 2 : 1;
        MMVQArgs a{};
        a.n_seg = n_seg; a.K = K; a.T = nt; a.epi = epi;
        a.fuse_mode = fz.mode; a.nx = fz.x; a.nw = fz.w; a.neps = fz.eps;
        a.out_host = nt == 1 && T == 1 ? fz.out_host : nullptr;
        for (int s = 0; s < n_seg; s++) {
            a.seg[s] = segs[s];
            a.seg[s].out = segs[s].out + (size_t)t0 * segs[s].ld_out;
            if (segs[s].resid) a.seg[s].resid = segs[s].resid + (size_t)t0 * segs[s].ld_out;
        }
        chunk_act(a, aq, K, t0);
        if (trace) trace->note(a);
        hipError_t e = launch_mmvq(a, st);
        if (e != hipSuccess) return e;
        t0 += nt;
    }
    return hipSuccess;
}

hipError_t Context::ensure_prep(const ActQuant &aq, int K, int T) {
    if (prep_owner_ == aq.qs && prep_K_ == K && prep_T_ == T && aq.qs) return hipSuccess;
    HIP_TRY(launch_mmq_prep(aq, K, T, mmq_bh_, mmq_bl_, stream_));
    prep_written(aq, K, T);
    return hipSuccess;
}

// Q2_K / Q3_K / IQ4_XS / TQ1_0 / TQ2_0 tensors reach the matrix cores only through their plane sets (no expand-on-the-fly kernel): prompt batches of 32 tokens and more
// (the types with an exact Q8_0-layout copy: act_is_q80 without Q8_0 itself, which needs none)
static bool q80_copy(const DevTensor &w, int K, int T) {
    return type_has_q80_copy(w.type) && w.planes && w.n_expert == 1 && mmq_q80_applicable(T_Q8_0, K, T);
}
static bool planes_small(const DevTensor &w, int K, int T) { return type_is_planes_only(w.type) && w.planes && T >= 32 && (K % 256) == 0; }

PromptMatmul prompt_mul_mat_choice(int role, const DevTensor *const *ws, int n, int K, int T, MMQWorkspace wsp) {
    PromptMatmul pm;
    if (role == PM_ROLE_ONE) {
        const DevTensor &w = *ws[0];
        if (mmq_ksplit_preferred(w.type, (int)w.N, K, T, w.planes != nullptr)) {   // batched decode steps, short prompts, expert batches: MFMA, K split
            pm.form = PM_KSPLIT; pm.n_fused = 1; pm.need_prep = w.type != T_Q6_K;
        } else if (mmq_applicable(w.type, K, T)) {                                  // prompt processing: MFMA path
            pm.form = w.planes ? PM_PLANES : PM_FLY; pm.n_fused = 1; pm.need_prep = w.type != T_Q6_K || !w.planes;
        } else if (planes_small(w, K, T)) {
            // prompt processing of Q2_K / Q3_K / IQ4_XS / TQ1_0 / TQ2_0 tensors: their plane sets (expanded at load in the Q4_K / Q6_K plane formats, mmq.hip) on the same kernels
            pm.form = PM_PLANES; pm.n_fused = 1; pm.planes_only = true; pm.need_prep = w.type == T_Q2_K;
        }
        return pm;
    }
    if (role == PM_ROLE_MULTI) {
        bool all_mmq = true, all_ks = true;
        // (IQ4_XS, TQ1_0, TQ2_0: through their plane sets, the signed format - Q | K | V of those mixes run as one launch like the K-quants')
        auto signed_planes_only = [](int t) { return t == T_IQ4_XS || type_is_ternary(t); };
        for (int i = 0; i < n; i++) { all_mmq &= mmq_applicable(ws[i]->type, K, T) || (signed_planes_only(ws[i]->type) && planes_small(*ws[i], K, T)); all_ks &= mmq_ksplit_applicable(ws[i]->type, K, T); }
        if (all_ks && n <= 3) {                                  // batched decode step: Q, K, V in one launch
            pm.form = PM_KSPLIT; pm.n_fused = n; pm.need_prep = true;
            return pm;
        }
        if (!all_mmq) return pm;
        // Q | K | V (or Q | K) as one launch over the concatenated rows where their plane sets are adjacent in the arena and
        // of one plane format (Q4_K and Q5_K share it; the Q6_K attn_v of the "more bits" layers runs on its own)
        auto mins = [&](int t) { return t != T_Q6_K && !signed_planes_only(t); };
        auto adjacent = [&](int i) { return ws[i]->planes && ws[i - 1]->planes && ws[i]->planes == ws[i - 1]->planes + ws[i - 1]->planes_bytes &&
                                            (ws[i - 1]->N % 32) == 0 && ws[i]->n_expert == 1; };
        int nf = 1;
        while (nf < n && nf < 3 && adjacent(nf) && mins(ws[nf]->type) == mins(ws[0]->type)) nf++;
        // the "more bits" layers (Q6_K attn_v beside Q4_K / Q5_K attn_q, attn_k): still one launch where the 128 x 256 kernel takes it
        int nm = nf;
        while (nm < n && nm < 3 && adjacent(nm)) nm++;
        if (nm > nf) {
            int rows[3];
            for (int i = 0; i < nm; i++) rows[i] = (int)ws[i]->N;
            if (mmq_planes_mixed_ok(rows, nm, K, T, wsp)) nf = nm;
        }
        pm.form = PM_PLANES; pm.n_fused = nf >= 2 ? nf : 0; pm.need_prep = true;
        return pm;
    }
    // PM_ROLE_GATE_UP: ws = {ffn_gate, ffn_up}
    const DevTensor &g = *ws[0], &u = *ws[1];
    if (mmq_ksplit_preferred(g.type, (int)g.N, K, T, g.planes != nullptr, true) && mmq_ksplit_preferred(u.type, (int)u.N, K, T, u.planes != nullptr, true)) {
        pm.form = PM_KSPLIT; pm.n_fused = 2; pm.need_prep = g.type != T_Q6_K || u.type != T_Q6_K;     // batched decode step: gate and up in one launch
        pm.swiglu = T <= 32 && g.type == u.type && g.N == u.N;   // SwiGLU in the epilogue
    } else if (g.planes && u.planes && g.N == u.N && (mmq_applicable(g.type, K, T) || planes_small(g, K, T)) && mmq_planes_swiglu_ok(g.type, u.type, (int)g.N, K, T)) {
        pm.form = PM_PLANES; pm.n_fused = 2; pm.swiglu = true;   // prompt batch on the LDS kernel: gate and up in one launch, SwiGLU in the epilogue
    }
    return pm;
}

hipError_t Context::linear(const DevTensor &w, const ActQuant &aq, const float *x_f32, int K, int T, float *out, int ld_out,
                           const float *resid, int epi) {
    if (type_is_quant(w.type)) {
        if (mmq_q80_applicable(w.type, K, T) && pending_fuse_.mode == 0 && epi != EPI_SWIGLU && aq.qs0)   // prompt processing, Q8_0 weights
            return launch_mmq_q80(w.data, w.row_bytes, (int)w.N, K, T, aq, out, ld_out, epi == EPI_ADD ? resid : nullptr, stream_);
        // (bh_over_ / bl_over_: the caller prepared the block-sum planes of a larger batch that aq's rows are a slice of - the expert loop)
        const int8_t *bh = bh_over_ ? bh_over_ : mmq_bh_, *bl = bh_over_ ? bl_over_ : mmq_bl_;
        // the K-quants' MFMA launches: the K-split kernel, the plane sets, the expansion on the fly (prompt_mul_mat_choice; the planes-only types want Q8_K rows)
        const DevTensor *w1 = &w;
        const PromptMatmul pm = pending_fuse_.mode == 0 && epi != EPI_SWIGLU ? prompt_mul_mat_choice(PM_ROLE_ONE, &w1, 1, K, T, mmq_ws_) : PromptMatmul();
        if (pm.form != PM_NONE && !(pm.planes_only && !aq.qs)) {
            if (pm.need_prep && !bh_over_) HIP_TRY(ensure_prep(aq, K, T));
            if (pm.form == PM_KSPLIT) return launch_mmq_ksplit(w.type, w.data, w.row_bytes, (int)w.N, K, T, aq, bh, bl, out, ld_out, epi == EPI_ADD ? resid : nullptr, stream_);
            if (pm.form == PM_PLANES) return launch_mmq_planes(w.type, w.planes, (int)w.N, K, T, aq, bh, bl, out, ld_out, epi == EPI_ADD ? resid : nullptr, stream_, mmq_ws_);
            return launch_mmq(w.type, w.data, w.row_bytes, (int)w.N, K, T, aq, bh, bl, out, ld_out, epi == EPI_ADD ? resid : nullptr, stream_);
        }
        if (q80_copy(w, K, T) && pending_fuse_.mode == 0 && epi != EPI_SWIGLU && aq.qs0)      // prompt processing of Q4_0 / Q5_0 / IQ4_NL / Q4_1 / Q5_1 / MXFP4 tensors: their exact Q8_0-layout copy
            return launch_mmq_q80(w.planes, mmq_q80_copy_row_bytes(w.type, K), (int)w.N, K, T, aq, out, ld_out, epi == EPI_ADD ? resid : nullptr, stream_, mmq_q80_copy_form(w.type));
        MMVQSeg s = make_seg(w, out, ld_out, resid, nullptr);
        return mmvq_tokens(&s, 1, K, T, epi, aq, stream_, pending_fuse_);
    }
    if (w.type == T_BF16) {                                      // the activation rows rounded to bf16 once, then the weight stream or the matrix cores
        const DevTensor *ws1[1] = {&w};
        float *outs1[1] = {out};
        HIP_TRY(launch_f32_to_bf16(x_f32, xb_, (size_t)T * K, stream_));
        return linear_bf16(ws1, outs1, nullptr, 1, K, T, ld_out, resid, epi);
    }
    if (mmf16_applicable(w.type, (int)w.N, K, T, w.data, x_f32, out) && w.n_expert == 1 && (ld_out & 3) == 0)      // a batch against an f16 tensor: matrix cores
        return launch_mmf16(w.data, (int)w.N, K, x_f32, T, out, ld_out, epi == EPI_ADD ? resid : nullptr, stream_);
    return launch_mmv_float(w.type, w.data, (int)w.N, K, x_f32, T, out, ld_out, epi == EPI_ADD ? resid : nullptr, stream_);
}

// up to three bf16 tensors over the activation rows in xb_ (already rounded): fewer than 8 tokens and narrow tensors take the weight stream - all segments in
// one launch, bias / residual / SwiGLU in its epilogue - the rest the matrix cores, one launch per tensor.  EPI_SWIGLU: ws = {gate, up}, outs[0] gets silu(g) * u
// (outs[1] is scratch for the matrix-core form).  ld_out: of outs[0] when there is one tensor, else every tensor's own row count.
// (the one place that decides between the two bf16 kernels: every tensor of the launch must take the matrix cores, else all take the stream)
static bool bf16_takes_mfma(const DevTensor *const *ws, float *const *outs, int n, int K, int T, int ld_out, const void *xb) {
    bool mfma = true;
    for (int i = 0; i < n; i++) mfma &= mmbf16_applicable(T_BF16, (int)ws[i]->N, K, T, ws[i]->data, xb, outs[i]) && ws[i]->n_expert == 1 && ((n == 1 ? ld_out : (int)ws[i]->N) & 3) == 0;
    return mfma;
}

hipError_t Context::linear_bf16(const DevTensor *const *ws, float *const *outs, const float *const *bias, int n, int K, int T, int ld_out, const float *resid, int epi) {
    if (bf16_takes_mfma(ws, outs, n, K, T, ld_out, xb_)) {
        for (int i = 0; i < n; i++)
            HIP_TRY(launch_mmbf16(ws[i]->data, (int)ws[i]->N, K, xb_, T, outs[i], n == 1 ? ld_out : (int)ws[i]->N, epi == EPI_ADD ? resid : nullptr, bias ? bias[i] : nullptr, 1.0f, false, stream_));
        if (epi == EPI_SWIGLU) HIP_TRY(launch_swiglu(outs[0], outs[1], outs[0], (int64_t)T * ws[0]->N, stream_));
        return hipSuccess;
    }
    MMVBF16Args a{};
    a.n_seg = n; a.K = K; a.epi = epi; a.resid = epi == EPI_ADD ? resid : nullptr; a.xb = xb_;
    for (int i = 0; i < n; i++) a.seg[i] = MMVBF16Seg{ws[i]->data, outs[i], bias ? bias[i] : nullptr, (int)ws[i]->N, n == 1 ? ld_out : (int)ws[i]->N, ws[i]->row_bytes};
    return launch_mmv_bf16_tokens(a, T, stream_);
}

hipError_t Context::linear_multi(const DevTensor *const *ws, float *const *outs, int n, const ActQuant &aq, const float *x_f32, int T, const float *const *bias, bool *bias_done) {
    bool all_q = true, all_bf = n <= 3;
    for (int i = 0; i < n; i++) { all_q &= type_is_quant(ws[i]->type); all_bf &= ws[i]->type == T_BF16 && ws[i]->n_expert == 1; }
    const int K = (int)ws[0]->K;
    if (all_bf) {                                                // Q | K | V of a bf16 layer: one rounding of the rows, one launch, the qwen2 biases in its epilogue
        HIP_TRY(launch_f32_to_bf16(x_f32, xb_, (size_t)T * K, stream_));
        HIP_TRY(linear_bf16(ws, outs, bias, n, K, T, 0, nullptr, EPI_STORE));
        if (bias_done) *bias_done = true;
        return hipSuccess;
    }
    // Q | K | V of a batched decode step in one K-split launch; of a prompt batch as one launch over the concatenated plane sets where those are adjacent
    // (prompt_mul_mat_choice), the rest each on its own
    const PromptMatmul pm = pending_fuse_.mode == 0 ? prompt_mul_mat_choice(PM_ROLE_MULTI, ws, n, K, T, mmq_ws_) : PromptMatmul();
    if (pm.form == PM_KSPLIT) {
        HIP_TRY(ensure_prep(aq, K, T));
        MMQSeg sg[3];
        for (int i = 0; i < n; i++) sg[i] = MMQSeg{ws[i]->data, ws[i]->row_bytes, (int)ws[i]->N, ws[i]->type, outs[i], (int)ws[i]->N, nullptr, 0};
        return launch_mmq_ksplit_multi(sg, n, K, T, aq, mmq_bh_, mmq_bl_, false, stream_);
    }
    if (pm.form == PM_PLANES) {
        HIP_TRY(ensure_prep(aq, K, T));
        const int nf = pm.n_fused;
        if (nf >= 2) {
            int rows[3], ldo[3], types[3];
            float *o[3];
            for (int i = 0; i < nf; i++) { rows[i] = (int)ws[i]->N; ldo[i] = (int)ws[i]->N; o[i] = outs[i]; types[i] = ws[i]->type; }
            HIP_TRY(launch_mmq_planes_multi(ws[0]->type, ws[0]->planes, rows, o, ldo, nf, K, T, aq, mmq_bh_, mmq_bl_, nullptr, stream_, mmq_ws_, types));
        }
        for (int i = nf; i < n; i++) {
            if (ws[i]->planes) HIP_TRY(launch_mmq_planes(ws[i]->type, ws[i]->planes, (int)ws[i]->N, K, T, aq, mmq_bh_, mmq_bl_, outs[i], (int)ws[i]->N, nullptr, stream_, mmq_ws_));
            else HIP_TRY(launch_mmq(ws[i]->type, ws[i]->data, ws[i]->row_bytes, (int)ws[i]->N, K, T, aq, mmq_bh_, mmq_bl_, outs[i], (int)ws[i]->N, nullptr, stream_));
        }
        return hipSuccess;
    }
    bool any_mmq = false;
    for (int i = 0; i < n; i++) any_mmq |= mmq_applicable(ws[i]->type, K, T) || mmq_q80_applicable(ws[i]->type, K, T) || planes_small(*ws[i], K, T) || q80_copy(*ws[i], K, T);
    if (all_q && n <= 3 && !(any_mmq && pending_fuse_.mode == 0)) {
        MMVQSeg segs[3];
        for (int i = 0; i < n; i++) segs[i] = make_seg(*ws[i], outs[i], (int)ws[i]->N, nullptr, nullptr);
        return mmvq_tokens(segs, n, K, T, EPI_STORE, aq, stream_, pending_fuse_);
    }
    // a prompt batch with mixed types (8-expert files keep attn_k / attn_v in Q8_0): every tensor takes its own best path
    for (int i = 0; i < n; i++) {
        hipError_t e = linear(*ws[i], aq, x_f32, K, T, outs[i], (int)ws[i]->N, nullptr, EPI_STORE);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ------------------------------------------------------------------------------------------ whole-step kernel
// Off by default: measured on MI355X (tools/bench_gridbar.hip) a device-wide barrier costs ~4 us where a
// launch boundary inside a graph costs ~2.7 us, so the whole-step kernel is ~10 % slower than one launch per operation.
// MI355_MEGA=1 or mi355_debug_set_option("decode_mega", 1) turns it on for contexts created afterwards.
// Batches of at least this many tokens run a mixture-of-experts feed-forward grouped by expert (ggml_mul_mat_id as one
// batched contraction per expert); fewer tokens loop over (token, expert) with the mat-vec.  Tests move it to compare both.
static int g_moe_group_min = getenv("MI355_MOE_GROUP_MIN") ? atoi(getenv("MI355_MOE_GROUP_MIN")) : 8;
void set_moe_group_min(int t) { g_moe_group_min = t < 1 ? 1 : t; }
// MXFP4 expert tensors, prompt batches: every expert's batch in one launch (false: a launch per expert, the same bits; the variable is for the benchmark's A/B)
static bool g_moe_q80_grouped = !(getenv("MI355_MOE_Q80_GROUPED") && getenv("MI355_MOE_Q80_GROUPED")[0] == '0');
void set_moe_q80_grouped(bool on) { g_moe_q80_grouped = on; }
static int g_decode_mega = -1;           // -1: take the environment
static bool g_store_fuse = true;
void set_attn_store_fuse(bool on) { g_store_fuse = on; }
static bool store_fuse_enabled() {
    static const bool env_off = getenv("MI355_ATTN_STORE_FUSE") && getenv("MI355_ATTN_STORE_FUSE")[0] == '0';
    return g_store_fuse && !env_off;
}
static bool g_rope_fast = true;
void set_rope_fast(bool on) { g_rope_fast = on; }
void set_decode_mega(bool on) { g_decode_mega = on ? 1 : 0; }

// Builds the per-layer phase descriptors of decode_mega.hip: the same MMVQArgs the per-launch path passes to
// launch_mmvq_fast for Q/K/V, attn_output, gate/up and down of a single token, planned for the mega grid.
bool Context::mega_prepare() {
    if (mega_state_ != 0) return mega_state_ > 0;
    mega_state_ = -1;
    static const bool mega_env_on = getenv("MI355_MEGA") && getenv("MI355_MEGA")[0] == '1';
    const bool mega_env = g_decode_mega < 0 ? mega_env_on : g_decode_mega > 0;
    const HParams &hp = model->hp;
    const int E = hp.n_embd, FF = hp.n_ff, H = hp.n_head, G = hp.n_head_kv, D = hp.head_dim;
    if (!mega_env || hp.n_expert > 0 || G <= 0 || H % G != 0 || H * D != E) return false;
    const int kb_e = (E + 2047) >> 11, kb_ff = (FF + 2047) >> 11;
    if ((E % 2048) != 0 || (FF % 256) != 0 || !decode_mega_applicable(kb_e, kb_ff, H / G, cp.type_k, cp.type_v, hp.qk_norm)) return false;
    RopeArgs ra = rope_args(*model, false);
    if (ra.neox || (ra.n_rot % 4) != 0 || D != 128 || !kv_store_fast_applicable(G, D, cp.type_k, cp.type_v, ra)) return false;
    std::vector<MegaLayer> ml((size_t)hp.n_layer);
    const int blocks = mega_blocks();
    size_t lds = 0;
    for (int il = 0; il < hp.n_layer; il++) {
        const LayerWeights &L = model->layers[(size_t)il];
        if (!type_is_kq456(L.wq.type) || !type_is_kq456(L.wk.type) || !type_is_kq456(L.wv.type) || !type_is_kq456(L.wo.type) || !type_is_kq456(L.gate.type) || !type_is_kq456(L.up.type) || !type_is_kq456(L.down.type)) return false;
        if (L.gate.type != L.up.type || L.gate.N != L.up.N || L.bq.valid() || L.bk.valid() || L.bv.valid()) return false;
        if ((int)L.wq.K != E || (int)L.wo.K != E || (int)L.gate.K != E || (int)L.down.K != FF) return false;
        MegaLayer &m = ml[(size_t)il];
        m.qkv = single_token_desc(3, E, EPI_STORE, 1, x_, (const float *)L.attn_norm.data, hp.eps, aq_e_);
        m.qkv.seg[0] = make_seg(L.wq, q_, (int)L.wq.N, nullptr, nullptr);
        m.qkv.seg[1] = make_seg(L.wk, k_, (int)L.wk.N, nullptr, nullptr);
        m.qkv.seg[2] = make_seg(L.wv, v_, (int)L.wv.N, nullptr, nullptr);
        m.wo = single_token_desc(1, E, EPI_ADD, 0, nullptr, nullptr, hp.eps, aq_o_);
        m.wo.seg[0] = make_seg(L.wo, x_, E, x_, nullptr);
        m.gate_up = single_token_desc(2, E, EPI_SWIGLU, 1, x_, (const float *)L.ffn_norm.data, hp.eps, aq_e_);
        m.gate_up.seg[0] = make_seg(L.gate, ffn_, FF, nullptr, nullptr);
        m.gate_up.seg[1] = make_seg(L.up, ffn_u_, FF, nullptr, nullptr);
        m.down = single_token_desc(1, FF, EPI_ADD, 2, ffn_, nullptr, hp.eps, aq_ff_);
        m.down.seg[0] = make_seg(L.down, x_, E, x_, nullptr);
        for (MMVQArgs *a : {&m.qkv, &m.wo, &m.gate_up, &m.down}) {
            if (!mmvq_fast_applicable(*a)) return false;
            const size_t l = mmvq_fast_plan(*a, blocks, 4);
            if (!l) return false;
            lds = std::max(lds, l);
        }
        m.kv = kv_[(size_t)il];
    }
    d_mega_layers_ = (MegaLayer *)dalloc(ml.size() * sizeof(MegaLayer));
    // the barrier words are polled through the scalar cache path: they must never be cached in an XCD's L2
    if (hipExtMallocWithFlags((void **)&d_mega_sync_, MEGA_SYNC_WORDS * sizeof(unsigned), hipDeviceMallocUncached) != hipSuccess) { d_mega_sync_ = nullptr; return false; }
    allocs_.push_back(d_mega_sync_);
    if (!d_mega_layers_ || !d_mega_sync_) return false;
    if (!h_mega_flag_ && hipHostMalloc((void **)&h_mega_flag_, sizeof(int), hipHostMallocDefault) != hipSuccess) return false;
    *h_mega_flag_ = 0;
    if (hipMemcpy(d_mega_layers_, ml.data(), ml.size() * sizeof(MegaLayer), hipMemcpyHostToDevice) != hipSuccess) return false;
    if (hipMemset(d_mega_sync_, 0, MEGA_SYNC_WORDS * sizeof(unsigned)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return false;
    if (getenv("MI355_MEGA_PROBE") && getenv("MI355_MEGA_PROBE")[0] == '1')
        d_mega_probe_ = (unsigned long long *)dalloc((size_t)(1 + MEGA_PROBES_PER_LAYER * hp.n_layer) * 8);
    mega_lds_ = lds;
    mega_state_ = 1;
    return true;
}

bool Context::mega_check() {
    if (mega_state_ <= 0 || !h_mega_flag_ || *h_mega_flag_ == 0) return true;
    // a device-wide barrier gave up: the step's results are not valid.  Fall back to one launch per operation from here on.
    *h_mega_flag_ = 0;
    (void)hipMemset(d_mega_sync_, 0, MEGA_SYNC_WORDS * sizeof(unsigned));
    (void)hipDeviceSynchronize();
    mega_state_ = -1;
    for (auto &ge : graphs_) (void)hipGraphExecDestroy(ge.second);
    graphs_.clear();
    graph_exec_ = nullptr;
    last_error = "whole-step kernel: device-wide barrier timed out (workgroups not co-resident?); results of the step discarded";
    return false;
}

// ------------------------------------------------------------------------------------------ layer engine
// Opt-in (MI355_ENGINE=1 or mi355_debug_set_option("decode_engine", 1)): measured on MI355X the layer launch takes 42 us against 38.7 us for the four
// launches it replaces (545 vs 570 tok/s on Llama-3-8B Q4_K_M; DESIGN.md 4.8 has the per-phase time line and what bounds it), so one launch per mat-vec
// stays the default; the bitwise test turns the engine on explicitly.
static int g_decode_engine = -1;         // -1: take the environment
void set_decode_engine(int on) { g_decode_engine = on < 0 ? -1 : on ? 1 : 0; }

// the sticky error word of the weight-stream / engine kernels: one pinned word per process, raised by a bounded wait that gave up
static unsigned *stream_error_word() {
    static unsigned *w = [] { unsigned *p = nullptr; if (hipHostMalloc((void **)&p, 64, hipHostMallocDefault) != hipSuccess) p = nullptr; if (p) *p = 0u; return p; }();
    return w;
}

unsigned *install_stream_error_word() {
    unsigned *ew = stream_error_word();
    if (ew) { mmvq_stream_set_error_word(ew); decode_engine_set_error_word(ew); attn_out_set_error_word(ew); tp_p2p_set_error_word(ew); }   // (per device: the pointer lives in device globals)
    return ew;
}

// The word is one per process (the kernels find it through a device global), but a process may hold several contexts (the engine's server_map_): the
// context that happens to read a raised word first is not necessarily the one whose kernel raised it.  So a raised word opens a new ERROR EPOCH, and every
// live context fails its next check once per epoch: the step that really timed out is never returned as valid, at the price of one discarded step in the
// bystanders.
static std::atomic<unsigned> g_stream_err_epoch{0}, g_stream_err_code{0};
// who can have raised it: every step launch of the process takes a serial; an epoch remembers the last serial handed out when it was opened; a context is a
// suspect if it has an unchecked launch from before that moment
static std::atomic<unsigned long long> g_launch_serial{0}, g_epoch_launch_serial{0};
unsigned long long next_launch_serial() { return g_launch_serial.fetch_add(1) + 1; }
unsigned stream_error_epoch() { return g_stream_err_epoch.load(); }
// tests (mi355_debug_set_option("raise_stream_error", code)): what a kernel's bounded wait does when it gives up
void debug_raise_stream_error(unsigned code) {
    unsigned *w = stream_error_word();
    if (w && code) __atomic_fetch_or(w, code, __ATOMIC_RELAXED);
}

static std::atomic<int> g_fused_owner_count[64];      // per device: 1 while a context holds the cross-workgroup-wait launches
static bool fused_gate_on() { static const bool off = getenv("MI355_FUSED_GATE") && getenv("MI355_FUSED_GATE")[0] == '0'; return !off; }
bool Context::fused_acquire() {
    if (!fused_gate_on() || holds_fused_) return true;
    int expected = 0;
    if (g_fused_owner_count[model->device & 63].compare_exchange_strong(expected, 1)) { holds_fused_ = true; return true; }
    return false;
}
void Context::fused_release() {
    if (holds_fused_) { holds_fused_ = false; g_fused_owner_count[model->device & 63].store(0); }
}

bool Context::stream_check() {
    fused_release();                                     // (every caller has just synchronised the context's stream)
    unsigned *w = stream_error_word();
    if (!w) return true;
    const unsigned raised = __atomic_exchange_n(w, 0u, __ATOMIC_RELAXED);
    if (raised) { g_stream_err_code.store(raised); g_epoch_launch_serial.store(g_launch_serial.load()); g_stream_err_epoch.fetch_add(1); }
    const unsigned epoch = g_stream_err_epoch.load();
    const unsigned long long first = first_unchecked_launch_;
    first_unchecked_launch_ = 0;                         // (every caller has just synchronised the context's stream: nothing of this context is in flight)
    if (epoch == err_epoch_seen_) return true;
    err_epoch_seen_ = epoch;
    // The word is raised by SOME kernel of the process.  A context with no unchecked launch from before the epoch was opened cannot be the one: it takes note
    // of the epoch and carries on - a time-out in one model's kernel then does not abort the requests of the other models a server holds, unless they were in
    // flight at the same moment (those discard one step each: the word cannot say whose kernel raised it).
    if (first == 0 || first > g_epoch_launch_serial.load()) return true;
    const unsigned code = g_stream_err_code.load();
    // a wait inside a kernel that waits for OTHER workgroups gave up (debugger, time-slicing, a workgroup that was not resident): the step's results are not
    // valid.  Two kernels wait that way - the layer engine and the one-launch attention + attn_output (attn_out.hip) - and both are left from here on: this
    // context takes one launch per mat-vec and the wait-free attention launch + linear(attn_output), so that a cause that persists (CU oversubscription from a
    // second stream, a debugger) cannot make every later step time out the same way.  The weight-stream kernels' own waits are inside one workgroup.
    engine_state_ = -1;
    attn_out_off_ = true;
    for (auto &ge : graphs_) (void)hipGraphExecDestroy(ge.second);
    graphs_.clear();
    graph_exec_ = nullptr;
    char buf[240];
    snprintf(buf, sizeof buf, "weight-stream / attention kernel: a bounded wait gave up in this process (code 0x%x); results of the step discarded, this context "
                              "continues on the wait-free launches", code);
    last_error = buf;
    return false;
}

// Builds the per-layer descriptors of decode_engine.hip: the same MMVQArgs the per-launch path passes to launch_mmvq_stream for attn_output, gate | up,
// down and the next layer's Q | K | V of a single token, planned for one workgroup per CU.
bool Context::engine_prepare() {
    if (engine_state_ != 0) return engine_state_ > 0;
    engine_state_ = -1;
    static const bool env_on = getenv("MI355_ENGINE") && getenv("MI355_ENGINE")[0] == '1';
    const bool on = g_decode_engine < 0 ? env_on : g_decode_engine > 0;
    const HParams &hp = model->hp;
    const int E = hp.n_embd, FF = hp.n_ff;
    if (!on || hp.n_expert > 0 || hp.tp_exchange || cp.n_ubatch < 1) return false;
    std::vector<EngineLayer> el((size_t)hp.n_layer);
    for (int il = 0; il < hp.n_layer; il++) {
        const LayerWeights &L = model->layers[(size_t)il];
        if (L.bq.valid() || L.bk.valid() || L.bv.valid()) return false;
        if (!type_is_quant(L.wo.type) || act_is_q80(L.wo.type)) return false;
        for (const DevTensor *t : {&L.wq, &L.wk, &L.wv, &L.wo, &L.gate, &L.up, &L.down}) if (t->type == T_BF16) return false;   // (the engine has no bf16 form)
        EngineLayer &m = el[(size_t)il];
        m.qk_norm = L.q_norm.valid() || L.k_norm.valid() || (il + 1 < hp.n_layer && (model->layers[(size_t)il + 1].q_norm.valid() || model->layers[(size_t)il + 1].k_norm.valid()));
        m.wo = single_token_desc(1, E, EPI_ADD, 0, nullptr, nullptr, hp.eps, aq_o_);
        m.wo.seg[0] = make_seg(L.wo, x_, E, x_, nullptr);
        m.gu = single_token_desc(2, E, EPI_SWIGLU, 1, x_, (const float *)L.ffn_norm.data, hp.eps, aq_e_);
        m.gu.seg[0] = make_seg(L.gate, ffn_, FF, nullptr, nullptr);
        m.gu.seg[1] = make_seg(L.up, ffn_u_, FF, nullptr, nullptr);
        m.dn = single_token_desc(1, FF, EPI_ADD, 2, ffn_, nullptr, hp.eps, aq_ff_);
        m.dn.seg[0] = make_seg(L.down, x_, E, x_, nullptr);
        m.has_qkv = il + 1 < hp.n_layer ? 1 : 0;
        m.qkv = MMVQArgs{};
        if (m.has_qkv) {
            const LayerWeights &N = model->layers[(size_t)il + 1];
            m.qkv = single_token_desc(3, E, EPI_STORE, 1, x_, (const float *)N.attn_norm.data, hp.eps, aq_e_);
            m.qkv.seg[0] = make_seg(N.wq, q_, (int)N.wq.N, nullptr, nullptr);
            m.qkv.seg[1] = make_seg(N.wk, k_, (int)N.wk.N, nullptr, nullptr);
            m.qkv.seg[2] = make_seg(N.wv, v_, (int)N.wv.N, nullptr, nullptr);
        }
        if ((int)L.wo.K != E || (int)L.gate.K != E || (int)L.down.K != FF || (int)L.gate.N != FF || (int)L.up.N != FF) return false;
        if (!decode_engine_applicable(m, E, FF)) return false;
        decode_engine_plan(m);
    }
    unsigned *ew = stream_error_word();
    if (!ew) return false;
    mmvq_stream_set_error_word(ew);
    decode_engine_set_error_word(ew);
    d_engine_layers_ = (EngineLayer *)dalloc(el.size() * sizeof(EngineLayer));
    const size_t gw = decode_engine_granule_words(E, FF);
    d_engine_gran_ = (unsigned long long *)dalloc(gw * 8);
    d_engine_epoch_ = d_step_serial_;     // the step serial every set-up launch increments
    if (!d_engine_layers_ || !d_engine_gran_ || !d_engine_epoch_) return false;
    if (hipMemcpy(d_engine_layers_, el.data(), el.size() * sizeof(EngineLayer), hipMemcpyHostToDevice) != hipSuccess) return false;
    if (hipMemset(d_engine_gran_, 0, gw * 8) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return false;
    if (const char *pl = getenv("MI355_ENGINE_PROBE")) {
        engine_probe_layer_ = atoi(pl);
        const size_t np = (size_t)num_cu() * 10 * 48;
        d_engine_probe_ = (unsigned long long *)dalloc(np * 8);
        if (d_engine_probe_) (void)hipMemset(d_engine_probe_, 0, np * 8);
        (void)hipDeviceSynchronize();
    }
    engine_state_ = 1;
    return true;
}

// ------------------------------------------------------------------------------------------ the forward pass
// nomic-bert (llm_build_bert, the NOMIC_BERT branches): token + type-0 embeddings -> LayerNorm; per layer the fused Q | K | V projection, NEOX rope on Q and K,
// attention over ALL cells of the token's sequence (bidirectional: the attention kernels get INT_MAX as every token's position, so their causal test always
// passes), attn_output (+ bias), residual, LayerNorm, SwiGLU feed-forward, residual, LayerNorm.  The output is the last layer's hidden state; there is no head.
// K / V rows go through the context's cache like a prompt batch's (the whole sequence is one micro-batch: Context::decode checks that).
hipError_t Context::run_layers_encoder(int T, int n_kv_cap) {
    cur_T_ = T;
    const HParams &hp = model->hp;
    const int E = hp.n_embd, FF = hp.n_ff, H = hp.n_head, G = hp.n_head_kv, D = hp.head_dim;
    RopeArgs ra = rope_args(*model, true);
    const int n_kv_max = std::max(n_kv_cap, 1);
    att_splits_ = flash_attn_pick_splits(T, G, n_kv_max);
    last_layers_mega_ = false; last_layers_engine_ = false;
    HIP_TRY(launch_step_setup_embed(d_pos_, T, ra, rope_cs_, d_cell_pos_, d_cell_seq_, d_cell_, d_seqmask_, nullptr, nullptr, model->tok_embd.type, model->tok_embd.data, E,
                                    d_tok_, x_, stream_));
    if (model->tok_types.valid())      // token types are all zero: row 0 of the table on every token
        HIP_TRY(launch_add_qkv_bias(x_, nullptr, nullptr, (const float *)model->tok_types.data, nullptr, nullptr, E, 0, T, stream_));
    HIP_TRY(launch_layer_norm(x_, (const float *)model->tok_norm.data, (const float *)model->tok_norm_b.data, E, T, hp.eps, x_, stream_));
    prof_mark("embed");
    // quantised weight tensors contract against a quantised copy of their input (Q8_K for K-quants, Q8_0 otherwise), float tensors against the f32 rows
    auto quantise_for = [&](const float *x, int K, ActQuant &aq, std::initializer_list<const DevTensor *> ws) -> hipError_t {
        bool k = false, z = false;
        for (const DevTensor *w : ws) if (type_is_quant(w->type)) { if (act_is_q80(w->type)) z = true; else k = true; }
        if (!k && !z) return hipSuccess;
        prep_owner_ = nullptr;
        return launch_quantize(x, K, T, aq, k, z, stream_);
    };
    for (int il = 0; il < hp.n_layer; il++) {
        const LayerWeights &L = model->layers[(size_t)il];
        HIP_TRY(quantise_for(x_, E, aq_e_, {&L.wq, &L.wk, &L.wv}));
        const DevTensor *ws[3] = {&L.wq, &L.wk, &L.wv};
        float *outs[3] = {q_, k_, v_};
        HIP_TRY(linear_multi(ws, outs, 3, aq_e_, x_, T));
        prof_mark("qkv");
        HIP_TRY(launch_rope_kv_store(q_, k_, v_, T, H, G, D, d_pos_, d_cell_, ra, kv_[(size_t)il], cp.type_k, cp.type_v, (int)cp.n_ctx, rope_cs_, stream_));
        prof_mark("rope_kv");
        AttnArgs aa = attn_args(il, T, n_kv_max, d_pos_open_);    // (no quantised copy of the output: out_q stays null)
        aa.splits = att_splits_;
        aa.pf_splits = flash_attn_prefill_splits(T, H, G, D, n_kv_max);
        while (aa.pf_splits > 1 && flash_attn_workspace_floats(T, H, D, aa.pf_splits) > att_part_floats_) aa.pf_splits >>= 1;
        HIP_TRY(launch_flash_attn(aa, stream_));
        prof_mark("attn");
        HIP_TRY(quantise_for(att_, H * D, aq_o_, {&L.wo}));
        HIP_TRY(linear(L.wo, aq_o_, att_, H * D, T, q_, E, nullptr, EPI_STORE));
        if (L.bo.valid()) HIP_TRY(launch_add_qkv_bias(q_, nullptr, nullptr, (const float *)L.bo.data, nullptr, nullptr, E, 0, T, stream_));
        HIP_TRY(launch_add(q_, x_, xn_, (int64_t)T * E, stream_));                       // re-add the layer input
        HIP_TRY(launch_layer_norm(xn_, (const float *)L.attn_out_norm.data, (const float *)L.attn_out_norm_b.data, E, T, hp.eps, xn_, stream_));
        prof_mark("attn_out");
        HIP_TRY(quantise_for(xn_, E, aq_e_, {&L.gate, &L.up}));
        HIP_TRY(linear(L.gate, aq_e_, xn_, E, T, ffn_, FF, nullptr, EPI_STORE));
        HIP_TRY(linear(L.up, aq_e_, xn_, E, T, ffn_u_, FF, nullptr, EPI_STORE));
        HIP_TRY(launch_swiglu(ffn_, ffn_u_, ffn_, (int64_t)T * FF, stream_));
        prof_mark("ffn_gate_up");
        HIP_TRY(quantise_for(ffn_, FF, aq_ff_, {&L.down}));
        HIP_TRY(linear(L.down, aq_ff_, ffn_, FF, T, q_, E, nullptr, EPI_STORE));
        HIP_TRY(launch_add(q_, xn_, x_, (int64_t)T * E, stream_));                       // the attention output bypasses the feed-forward block
        HIP_TRY(launch_layer_norm(x_, (const float *)L.layer_out_norm.data, (const float *)L.layer_out_norm_b.data, E, T, hp.eps, x_, stream_));
        prof_mark("ffn_down");
        if (debug_taps_ && dbg_) HIP_TRY(hipMemcpyAsync(dbg_ + (size_t)il * cp.n_ubatch * E, x_, (size_t)T * E * 4, hipMemcpyDeviceToDevice, stream_));
    }
    return hipSuccess;
}

// ---- the llama-graph layer, block by block.  run_layers (below) is the loop; every choice of launch form is stated once, in the block that makes it, and
// bench_weight_sweep asks the same functions.

// what one run_layers call fixes for all its layers (the environment is read once per process)
Context::Step Context::step_constants(int T, int n_kv_cap) const {
    static const int attn_mode = getenv("MI355_ATTN_MODE") ? atoi(getenv("MI355_ATTN_MODE")) : 2;
    static const bool rope_fast_env = !(getenv("MI355_ROPE_FAST") && getenv("MI355_ROPE_FAST")[0] == '0');
    static const bool fuse_down_env = !(getenv("MI355_FUSE_DOWN") && getenv("MI355_FUSE_DOWN")[0] == '0');
    const HParams &hp = model->hp;
    Step st;
    st.T = T;
    st.n_kv_max = std::max(n_kv_cap, 1);   // upper bound of occupied cells the kernels are sized for
    st.ra_step = rope_args(*model, true);  // (each layer's: layer_rope)
    st.tp = hp.tp_exchange;
    st.chunk_lists = chunk_lmax_ > 0;
    st.attn_mode = attn_mode; st.rope_fast = rope_fast_env && g_rope_fast; st.fuse_down_env = fuse_down_env;
    // attn_output and ffn_down add their result to the residual stream in place; under a row split they leave this rank's partial sum (rank 0 carries the
    // residual) for the exchange: x = sum over ranks
    st.out = st.tp ? tp_part_ : x_;
    st.resid = !st.tp || hp.tp_rank == 0 ? x_ : nullptr;
    return st;
}

// the fields of an attention launch's description that no launch form changes (tok_pos: d_pos_; the encoder's open positions)
AttnArgs Context::attn_args(int il, int T, int n_kv_max, const int32_t *tok_pos) const {
    const HParams &hp = model->hp;
    AttnArgs aa{};
    aa.q = q_; aa.out = att_; aa.kv = kv_[(size_t)il]; aa.type_k = cp.type_k; aa.type_v = cp.type_v;
    aa.T = T; aa.H = hp.n_head; aa.G = hp.n_head_kv; aa.D = hp.head_dim; aa.n_ctx = (int)cp.n_ctx;
    aa.cell_pos = d_cell_pos_; aa.cell_seq = d_cell_seq_; aa.tok_pos = tok_pos; aa.tok_seq = d_seq_;
    aa.n_kv_dev = d_nkv_; aa.n_kv_max = n_kv_max; aa.scale = 1.0f / sqrtf((float)hp.head_dim); aa.part = att_part_;
    return aa;
}
// per-token chunk lists (decode_ubatch): batched steps, or regions in use
void Context::attn_chunk_lists(AttnArgs &aa) const {
    aa.tok_chunks = d_chunks_; aa.tok_nchunks = d_chunks_ + (size_t)64 * chunk_stride_; aa.chunk_stride = chunk_stride_;
    aa.splits = std::max(chunk_cap_, chunk_lmax_);
}

// Which launches run layer il's attention block.  Launches nothing.
Context::AttnPlan Context::plan_attn(int il, const Step &st) const {
    const HParams &hp = model->hp;
    const LayerWeights &L = model->layers[(size_t)il];
    const int E = hp.n_embd, T = st.T;
    AttnPlan p{};
    p.ra = layer_rope(st.ra_step, L, hp.eps);   // (qwen3: with the layer's q / k norm weights; every kernel either applies them or refuses)
    p.qkv_float = !type_is_quant(L.wq.type) || !type_is_quant(L.wk.type) || !type_is_quant(L.wv.type);
    // an adapter on attn_q / attn_k / attn_v: the norm runs as a launch of its own and leaves its f32 rows in xn_ for the deltas; one on attn_output: the
    // projection runs as a launch of its own behind the attention, which leaves its f32 rows in att_
    p.qkv_lora = f32_rows(il, LORA_Q) || f32_rows(il, LORA_K) || f32_rows(il, LORA_V);     // (or the importance-matrix collector reads them)
    p.qkv_prologue = !p.qkv_float && can_fuse(E, T) && !p.qkv_lora;
    AttnArgs &aa = p.aa;
    aa = attn_args(il, T, st.n_kv_max, d_pos_);
    const bool o_q = type_is_quant(L.wo.type);
    aa.out_q = o_q ? &aq_o_ : nullptr; aa.out_q8k = !act_is_q80(L.wo.type); aa.out_q80 = act_is_q80(L.wo.type);   // merged + quantised in one pass
    p.o_planes = o_q && aa.out_q8k && T >= 3;             // the batched kernels will want the block-sum planes: the merge writes them too
    if (p.o_planes) { aa.out_bh = mmq_bh_; aa.out_bl = mmq_bl_; }
    // (parity mode for an f16 cache: the generic launch dispatches to the cell-by-cell kernel with fp16 V accumulation)
    const bool v16 = fa_v_acc_f16_enabled() && cp.type_k == T_F16 && cp.type_v == T_F16;
    p.decode_attn = !v16 && flash_attn_decode_applicable(aa, p.ra);
    if (p.decode_attn) {
        aa.splits = flash_attn_decode_splits(st.n_kv_max);
        if (st.chunk_lists) attn_chunk_lists(aa);
        p.fused_step = st.attn_mode > 0 && flash_attn_decode_fused_applicable(aa, p.ra);
    }
    // single-token step: attention + attn_output in one launch (attn_out.hip) where it has a form for the shape
    // (not where the ranks of a row split exchange through the host callback - the transport of a rig whose ranks SHARE one device: this kernel's
    // workgroups wait for each other (consumers for the item workgroups' flags), and two processes' copies placed on the same CUs at the same time can
    // hold each other's item workgroups out - every wait then runs into its bound (round 6: 0x8 on three of eight ranks behind one MI355X at the first
    // single-token step, profiles/r6_tp_shared_device_trace.txt).  A rank that owns its GPU has the chip to itself.)
    p.ao_seg = make_seg(L.wo, st.out, E, st.resid, nullptr);
    p.ao_epi = st.resid ? EPI_ADD : EPI_STORE;
    p.af = aa;
    if (p.decode_attn && p.fused_step && st.attn_mode == 2 && !st.engine && il < 255 && !attn_out_off_ && !attn_out_skip_step_ && !(st.tp && tp_uses_host()) && !f32_rows(il, LORA_O)) {
        p.af.splits = attn_out_fused_splits(p.af);
        if (st.chunk_lists) p.af.splits = aa.splits;
        p.ao_form = attn_out_fused_applicable(p.af, p.ra, p.ao_seg, (int)L.wo.K, p.ao_epi);
    }
    // ... and the layer's Q | K | V in front of it in that launch: the RMSNorm -> Q8_K prologue, the three mat-vecs, rope, KV store, attention, merge,
    // Q8_K and attn_output + residual are ONE launch per layer (outputs bit-identical to the two launches)
    if (p.ao_form && p.qkv_prologue && !st.tp && d_qkv_gran_ && !(L.bq.valid() || L.bk.valid() || L.bv.valid())) {
        QKVFuse &qf = p.qf;
        qf.seg[0] = make_seg(L.wq, q_, (int)L.wq.N, nullptr, nullptr);
        qf.seg[1] = make_seg(L.wk, k_, (int)L.wk.N, nullptr, nullptr);
        qf.seg[2] = make_seg(L.wv, v_, (int)L.wv.N, nullptr, nullptr);
        qf.nx = x_; qf.nw = (const float *)L.attn_norm.data; qf.neps = hp.eps; qf.K = E; qf.gran = d_qkv_gran_;
        p.qkv_in_attn = qkv_attn_out_applicable(p.af, p.ra, p.ao_seg, (int)L.wo.K, p.ao_epi, qf);
    }
    return p;
}

// Q | K | V as launches of their own: q_, k_, v_ from the layer input (nothing where the plan has them inside the attention launch, or the engine made them)
hipError_t Context::attn_qkv(int il, const Step &st, const AttnPlan &p) {
    const HParams &hp = model->hp;
    const LayerWeights &L = model->layers[(size_t)il];
    const int E = hp.n_embd, T = st.T;
    if (p.qkv_in_attn) return hipSuccess;
    if (st.engine && il > 0) return hipSuccess;               // computed at the end of the previous layer's engine launch
    if (p.qkv_prologue) {
        pending_fuse_.mode = 1; pending_fuse_.x = x_; pending_fuse_.w = (const float *)L.attn_norm.data; pending_fuse_.eps = hp.eps;
    } else {
        const bool need_k = (type_is_quant(L.wq.type) && !act_is_q80(L.wq.type)) || (type_is_quant(L.wk.type) && !act_is_q80(L.wk.type)) || (type_is_quant(L.wv.type) && !act_is_q80(L.wv.type));
        const bool need_0 = act_is_q80(L.wq.type) || act_is_q80(L.wk.type) || act_is_q80(L.wv.type);
        const bool pl = need_k && T >= 3;                      // the batched kernels will want the block-sum planes
        HIP_TRY(launch_rmsnorm_quant(x_, (const float *)L.attn_norm.data, E, T, hp.eps, p.qkv_float || p.qkv_lora ? xn_ : nullptr, &aq_e_, need_k, need_0, stream_,
                                     pl ? mmq_bh_ : nullptr, pl ? mmq_bl_ : nullptr));
        prep_owner_ = nullptr;
        if (pl) prep_written(aq_e_, E, T);
        prof_mark("norm_quant");
        if (imx_on_) HIP_TRY(imx_collect(il, IMX_QKV, xn_, nullptr, E, T, nullptr, nullptr));
    }
    const DevTensor *ws[3] = {&L.wq, &L.wk, &L.wv};
    float *outs[3] = {q_, k_, v_};
    const float *bias[3] = {L.bq.valid() ? (const float *)L.bq.data : nullptr, L.bk.valid() ? (const float *)L.bk.data : nullptr, L.bv.valid() ? (const float *)L.bv.data : nullptr};
    bool bias_done = false;                                      // (a bf16 layer adds the biases in its launch's epilogue: the same f32 add)
    HIP_TRY(linear_multi(ws, outs, 3, aq_e_, xn_, T, bias, &bias_done));
    pending_fuse_ = Fuse();
    if (p.qkv_lora) {                                            // before the biases, the rope, the q / k norm and the KV store read q_, k_, v_
        const int targets[3] = {LORA_Q, LORA_K, LORA_V}, lds[3] = {(int)L.wq.N, (int)L.wk.N, (int)L.wv.N};
        HIP_TRY(lora_add(il, targets, outs, lds, 3, xn_, E, E, T));
    }
    if (!bias_done && (bias[0] || bias[1] || bias[2]))          // qwen2-style attention biases: all T rows of the three projections in one launch
        HIP_TRY(launch_add_qkv_bias(q_, k_, v_, bias[0], bias[1], bias[2], hp.n_head * hp.head_dim, hp.n_head_kv * hp.head_dim, T, stream_));
    prof_mark("qkv");
    return hipSuccess;
}

// rope, KV store and the attention itself in the plan's launch form: att_ (and its quantised copy for attn_output) - or, with p.ao_form, attn_output as well
hipError_t Context::attn_core(int il, const Step &st, const AttnPlan &p) {
    const HParams &hp = model->hp;
    const LayerWeights &L = model->layers[(size_t)il];
    const int H = hp.n_head, G = hp.n_head_kv, D = hp.head_dim, T = st.T;
    const KVLayerView &kv = kv_[(size_t)il];
    unsigned *ao_flags = d_ao_flags_ + (size_t)il * 64 * ATT_SYNC_STRIDE;
    if (p.qkv_in_attn) {
        HIP_TRY(launch_qkv_attn_out(p.af, rope_cs_, p.ra, d_cell_, att_counters_, ao_flags, d_ao_gran_, il, d_step_serial_, p.ao_seg, (int)L.wo.K, p.ao_epi, p.qf, stream_));
        qkv_attn_launches++;
        prof_mark("qkv");
    } else if (p.fused_step) {
        // single-token step: K rope + KV store + attention + split merge + quantise in ONE launch - and, where attn_out.hip has a form for the shape,
        // the attn_output mat-vec with its residual add in that launch too
        if (p.ao_form)
            HIP_TRY(launch_attn_out_fused(p.af, rope_cs_, p.ra, k_, v_, d_cell_, att_counters_, ao_flags, d_ao_gran_, il, d_step_serial_, p.ao_seg, (int)L.wo.K, p.ao_epi, stream_));
        else
            HIP_TRY(launch_flash_attn_decode_fused(p.aa, rope_cs_, p.ra, k_, v_, d_cell_, st.attn_mode == 2 ? att_counters_ : nullptr, stream_));
    } else if (p.decode_attn && batch_distinct_ && store_fuse_enabled()) {
        // batched step, every token of a different sequence: K rope + KV store inside the attention launch (no token reads another's new cell)
        HIP_TRY(launch_flash_attn_decode(p.aa, rope_cs_, p.ra, stream_, k_, v_, d_cell_));
    } else if (p.decode_attn && kv_store_fast_applicable(G, D, cp.type_k, cp.type_v, p.ra)) {
        // small-batch step: K rope + KV store in one small kernel; q is rotated inside the attention kernel
        HIP_TRY(launch_kv_store_fast(k_, v_, T, G, D, rope_cs_, p.ra, d_cell_, kv, cp.type_k, cp.type_v, (int)cp.n_ctx, stream_));
        prof_mark("rope_kv");
        HIP_TRY(launch_flash_attn_decode(p.aa, rope_cs_, p.ra, stream_));
    } else {
        if (st.rope_fast && rope_cs_ && rope_q_kv_store_fast_applicable(H, G, D, cp.type_k, cp.type_v, p.ra))
            HIP_TRY(launch_rope_q_kv_store_fast(q_, k_, v_, T, H, G, D, rope_cs_, p.ra, d_cell_, kv, cp.type_k, cp.type_v, (int)cp.n_ctx, stream_));
        else
            HIP_TRY(launch_rope_kv_store(q_, k_, v_, T, H, G, D, d_pos_, d_cell_, p.ra, kv, cp.type_k, cp.type_v, (int)cp.n_ctx, rope_cs_, stream_));
        prof_mark("rope_kv");
        AttnArgs aa = p.aa;
        aa.splits = att_splits_;
        // (splits balance the causal tiles of ONE long sequence: sized by what a query of this batch can see - its position + 1 -
        // not by the cache's high-water mark: 32 sequences of 50-token prompts in a 32000-cell cache need none, and every
        // extra workgroup would scan the whole cell table)
        aa.pf_splits = flash_attn_prefill_splits(T, H, G, D, std::min(st.n_kv_max, cur_max_pos_ + 1));
        while (aa.pf_splits > 1 && flash_attn_workspace_floats(T, H, D, aa.pf_splits) > att_part_floats_) aa.pf_splits >>= 1;
        HIP_TRY(launch_flash_attn(aa, stream_));
    }
    prof_mark("attn");
    if (p.o_planes) prep_written(aq_o_, (int)L.wo.K, T);       // the attention just re-quantised its output, planes included
    else if (prep_owner_ == aq_o_.qs) prep_owner_ = nullptr;
    return hipSuccess;
}

// attn_output + residual into st.out (nothing where it ran inside the attention launch)
hipError_t Context::attn_output(int il, const Step &st, const AttnPlan &p) {
    const LayerWeights &L = model->layers[(size_t)il];
    if (p.ao_form) return hipSuccess;
    HIP_TRY(linear(L.wo, aq_o_, att_, (int)L.wo.K, st.T, st.out, model->hp.n_embd, st.resid, p.ao_epi));
    if (imx_on_) HIP_TRY(imx_collect(il, IMX_O, att_, nullptr, (int)L.wo.K, st.T, nullptr, nullptr));
    if (lora_on(il, LORA_O)) {                                   // onto the rows that already hold the residual
        const int target = LORA_O, ld = model->hp.n_embd;
        float *out = st.out;
        HIP_TRY(lora_add(il, &target, &out, &ld, 1, att_, (int)L.wo.K, (int)L.wo.K, st.T));
    }
    return hipSuccess;
}

// "SwiGLU, then quantise for a quantised ffn_down", in one pass: aq_ff_ from gate | up's result.  combined: ffn_ already holds silu(gate) * up (the
// planes-SwiGLU launch's epilogue), only the quantisation is left.  The block-sum planes the batched ffn_down kernels take are written with the codes from
// 3 tokens on - planes_any_T: also below that (the K-split branch has always written them with every batch it runs for).
hipError_t Context::quantise_for_down(int il, int T, bool combined, bool planes_any_T) {
    const int FF = model->hp.n_ff;
    const bool k = !act_is_q80(model->layers[(size_t)il].down.type), pl = k && (planes_any_T || T >= 3);
    int8_t *bh = pl ? mmq_bh_ : nullptr, *bl = pl ? mmq_bl_ : nullptr;
    if (combined) HIP_TRY(launch_quantize(ffn_, FF, T, aq_ff_, k, !k, stream_, bh, bl));
    else HIP_TRY(launch_swiglu_quant(ffn_, ffn_u_, FF, T, aq_ff_, k, !k, stream_, bh, bl));
    prep_owner_ = nullptr;
    if (pl) prep_written(aq_ff_, FF, T);
    return hipSuccess;
}

// dense feed-forward, first half: ffn_ = silu(gate x') * (up x') with x' = RMSNorm(x).  quantised: aq_ff_ already holds it quantised for ffn_down
hipError_t Context::ffn_dense_gate_up(int il, const Step &st, bool &quantised) {
    const HParams &hp = model->hp;
    const LayerWeights &L = model->layers[(size_t)il];
    const int E = hp.n_embd, FF = hp.n_ff, T = st.T;
    quantised = false;
    const bool gq = type_is_quant(L.gate.type), uq = type_is_quant(L.up.type);
    const bool fk = (gq && !act_is_q80(L.gate.type)) || (uq && !act_is_q80(L.up.type));
    const bool f0 = act_is_q80(L.gate.type) || act_is_q80(L.up.type);
    // an adapter on ffn_gate / ffn_up: both projections store their rows (the last branch below), the deltas are added from xn_, then SwiGLU; one on ffn_down:
    // ffn_ must hold silu(gate) * up in f32 - the same branch, without the quantising shortcut
    const bool lora_gu = f32_rows(il, LORA_GATE) || f32_rows(il, LORA_UP), lora_any = lora_gu || f32_rows(il, LORA_DOWN);      // (an adapter, or the collector)
    const bool fuse_ffn = gq && uq && L.gate.type == L.up.type && can_fuse(E, T) && !lora_any;
    Fuse fz;
    if (fuse_ffn) {
        fz.mode = 1; fz.x = x_; fz.w = (const float *)L.ffn_norm.data; fz.eps = hp.eps;
    } else {
        const bool pl = fk && T >= 3;
        HIP_TRY(launch_rmsnorm_quant(x_, (const float *)L.ffn_norm.data, E, T, hp.eps, (!gq || !uq || lora_gu) ? xn_ : nullptr, &aq_e_, fk, f0, stream_,
                                     pl ? mmq_bh_ : nullptr, pl ? mmq_bl_ : nullptr));
        prep_owner_ = nullptr;
        if (pl) prep_written(aq_e_, E, T);
        prof_mark("norm_quant");
        if (imx_on_) HIP_TRY(imx_collect(il, IMX_FFN_IN, xn_, nullptr, E, T, nullptr, nullptr));
    }
    const bool down_q = type_is_quant(L.down.type) && (FF % 32) == 0;      // SwiGLU and the quantisation for ffn_down can share a pass
    const bool ffn_mmq = (mmq_q80_applicable(L.gate.type, E, T) && mmq_q80_applicable(L.up.type, E, T)) ||
                         (mmq_applicable(L.gate.type, E, T) && mmq_applicable(L.up.type, E, T)) ||
                         (mmq_ksplit_applicable(L.gate.type, E, T) && mmq_ksplit_applicable(L.up.type, E, T)) ||
                         (planes_small(L.gate, E, T) && planes_small(L.up, E, T)) || (q80_copy(L.gate, E, T) && q80_copy(L.up, E, T));
    // gate | up as one MFMA launch: the K-split pair, or the plane sets with SwiGLU in the epilogue (prompt_mul_mat_choice)
    const DevTensor *gu_w[2] = {&L.gate, &L.up};
    const PromptMatmul gu_pm = fuse_ffn ? PromptMatmul() : prompt_mul_mat_choice(PM_ROLE_GATE_UP, gu_w, 2, E, T, mmq_ws_);
    const bool ffn_ks = gu_pm.form == PM_KSPLIT;
    if (lora_any) {
        HIP_TRY(linear(L.gate, aq_e_, xn_, E, T, ffn_, FF, nullptr, EPI_STORE));
        HIP_TRY(linear(L.up, aq_e_, xn_, E, T, ffn_u_, FF, nullptr, EPI_STORE));
        if (lora_gu) {
            const int targets[2] = {LORA_GATE, LORA_UP}, lds[2] = {FF, FF};
            float *outs[2] = {ffn_, ffn_u_};
            HIP_TRY(lora_add(il, targets, outs, lds, 2, xn_, E, E, T));
        }
        quantised = T > 1 && down_q && !f32_rows(il, LORA_DOWN);
        if (quantised) HIP_TRY(quantise_for_down(il, T, false, false));
        else HIP_TRY(launch_swiglu(ffn_, ffn_u_, ffn_, (int64_t)T * FF, stream_));
        if (imx_on_) HIP_TRY(imx_collect(il, IMX_FFN_DOWN, ffn_, nullptr, FF, T, nullptr, nullptr));      // ffn_ holds silu(gate) * up in f32
    } else if (gq && uq && L.gate.type == L.up.type && !ffn_mmq) {
        MMVQSeg segs[2] = {make_seg(L.gate, ffn_, FF, nullptr, nullptr), make_seg(L.up, ffn_u_, FF, nullptr, nullptr)};
        HIP_TRY(mmvq_tokens(segs, 2, E, T, EPI_SWIGLU, aq_e_, stream_, fz));
    } else if (L.gate.type == T_BF16 && L.up.type == T_BF16 && L.gate.N == L.up.N) {
        // bf16 gate | up: one rounding of the rows; the weight stream computes both in one launch with SwiGLU in its epilogue, a prompt batch runs the
        // two matrix-core products and the SwiGLU pass
        const DevTensor *gu[2] = {&L.gate, &L.up};
        float *go[2] = {ffn_, ffn_u_};
        HIP_TRY(launch_f32_to_bf16(xn_, xb_, (size_t)T * E, stream_));
        quantised = T > 1 && down_q && bf16_takes_mfma(gu, go, 2, E, T, 0, xb_);
        HIP_TRY(linear_bf16(gu, go, nullptr, 2, E, T, 0, nullptr, quantised ? EPI_STORE : EPI_SWIGLU));
        if (quantised) HIP_TRY(quantise_for_down(il, T, false, false));
    } else if (ffn_ks) {                                   // batched decode step: gate and up in one launch
        if (gu_pm.need_prep) HIP_TRY(ensure_prep(aq_e_, E, T));
        MMQSeg sg[2] = {{L.gate.data, L.gate.row_bytes, (int)L.gate.N, L.gate.type, ffn_, FF, nullptr, 0},
                        {L.up.data, L.up.row_bytes, (int)L.up.N, L.up.type, ffn_u_, FF, nullptr, 0}};
        const bool pair = gu_pm.swiglu;                          // SwiGLU in the epilogue
        HIP_TRY(launch_mmq_ksplit_multi(sg, 2, E, T, aq_e_, mmq_bh_, mmq_bl_, pair, stream_));
        quantised = !pair && down_q;
        if (quantised) HIP_TRY(quantise_for_down(il, T, false, true));
        else if (!pair) HIP_TRY(launch_swiglu(ffn_, ffn_u_, ffn_, (int64_t)T * FF, stream_));
    } else if (T > 1 && gu_pm.form == PM_PLANES) {
        // prompt batch on the LDS kernel: gate and up in one launch, 64 rows of each per workgroup, SwiGLU in the epilogue (one
        // f32 result of T x FF instead of two); the quantiser for the down projection then reads half as much
        HIP_TRY(launch_mmq_planes_swiglu(L.gate.type, L.gate.planes, L.up.planes, (int)L.gate.N, E, T, aq_e_, ffn_, FF, stream_));
        quantised = down_q;
        if (quantised) HIP_TRY(quantise_for_down(il, T, true, false));
    } else {
        HIP_TRY(linear(L.gate, aq_e_, xn_, E, T, ffn_, FF, nullptr, EPI_STORE));
        HIP_TRY(linear(L.up, aq_e_, xn_, E, T, ffn_u_, FF, nullptr, EPI_STORE));
        // prompt batch: SwiGLU and the quantisation for the down projection in one pass (no f32 round trip of T x FF)
        quantised = T > 1 && down_q;
        if (quantised) HIP_TRY(quantise_for_down(il, T, false, false));
        else HIP_TRY(launch_swiglu(ffn_, ffn_u_, ffn_, (int64_t)T * FF, stream_));
    }
    prof_mark("ffn_gate_up");
    return hipSuccess;
}

// dense feed-forward, second half: ffn_down + residual into st.out.  n_matvec (optional): the mat-vec launches it took (2: the column halves)
hipError_t Context::ffn_down(int il, const Step &st, bool quantised, int *n_matvec) {
    const HParams &hp = model->hp;
    const LayerWeights &L = model->layers[(size_t)il];
    const int E = hp.n_embd, FF = hp.n_ff, T = st.T;
    const int epi = st.resid ? EPI_ADD : EPI_STORE;
    // quantise inside the down-projection's prologue (once per CU, overlapped with its first weight loads)
    // (the widths listed are the ones the register-ring and weight-stream kernels take; the generic mat-vec's fused prologue would refuse others)
    // (... and an n_ff that ends inside a 256-group: the generic mat-vec's prologue, Q8_0 activations)
    const bool lora_down = f32_rows(il, LORA_DOWN);              // ffn_ holds f32 rows: the projection quantises them in a launch of its own, the delta is added behind it
    const bool fuse_down = !lora_down && st.fuse_down_env && T == 1 && type_is_quant(L.down.type) &&
                           (((FF % 256) == 0 && mmvq_fast_kb_ok((FF + 2047) / 2048)) || ((FF % 256) != 0 && (FF % 32) == 0 && FF <= 8192 && act_is_q80(L.down.type)));
    if (fuse_down && !st.tp && L.down_lo.valid() && L.down_hi.valid()) {
        // the column halves of ffn_down, each quantising its half of the SwiGLU output in its prologue: x += W_lo a_lo; x += W_hi a_hi
        const int Kh = (int)L.down_lo.K;
        pending_fuse_.mode = 2; pending_fuse_.x = ffn_;
        HIP_TRY(linear(L.down_lo, aq_ff_, ffn_, Kh, T, st.out, E, st.resid, epi));
        pending_fuse_.mode = 2; pending_fuse_.x = ffn_ + Kh;
        HIP_TRY(linear(L.down_hi, aq_ff_, ffn_ + Kh, Kh, T, st.out, E, st.out, EPI_ADD));
        pending_fuse_ = Fuse();
        if (n_matvec) *n_matvec = 2;
        return hipSuccess;
    }
    if (n_matvec) *n_matvec = 1;
    if (fuse_down) {
        pending_fuse_.mode = 2; pending_fuse_.x = ffn_;
    } else if (type_is_quant(L.down.type) && !quantised) {
        HIP_TRY(launch_quantize(ffn_, FF, T, aq_ff_, !act_is_q80(L.down.type), act_is_q80(L.down.type), stream_));
        prep_owner_ = nullptr;
        prof_mark("quant");
    }
    HIP_TRY(linear(L.down, aq_ff_, ffn_, FF, T, st.out, E, st.resid, epi));
    pending_fuse_ = Fuse();
    if (lora_down) {
        const int target = LORA_DOWN;
        float *out = st.out;
        HIP_TRY(lora_add(il, &target, &out, &E, 1, ffn_, FF, FF, T));
    }
    return hipSuccess;
}

// single-token step of a mixture-of-experts layer: the token's selected experts share one launch per projection (the workgroups are divided among them;
// each reads its own expert index on the device): gate | up with SwiGLU (a), then down with the Q8_K quantisation of its own expert's activation in the
// prologue (d).  False where the layer has no such form.
bool Context::moe_selected_desc(int il, MMVQArgs &a, MMVQArgs &d) const {
    const HParams &hp = model->hp;
    const LayerWeights &L = model->layers[(size_t)il];
    const int E = hp.n_embd, FF = hp.n_ff, KU = hp.n_expert_used;
    if (KU < 2 || KU > 8 || (int)cp.n_ubatch < KU || L.gate_exps.type != L.up_exps.type) return false;
    // (RMSNorm + quantise again in the launch's prologue - the same arithmetic as the norm_quant launch that fed the router, so the same codes: the
    // weight stream's gate | up form takes its activation that way, and with it the selected experts stream like the dense feed-forward does)
    const bool prologue = can_fuse(E, 1) && !act_is_q80(L.gate_exps.type);
    a = single_token_desc(2, E, EPI_SWIGLU, prologue ? 1 : 0, prologue ? x_ : nullptr, prologue ? (const float *)L.ffn_norm.data : nullptr, prologue ? hp.eps : 0.0f, aq_e_);
    a.n_sel = KU; a.sel_out_stride = FF;
    a.seg[0] = make_seg(L.gate_exps, ffn_, FF, nullptr, moe_ids_);
    a.seg[1] = make_seg(L.up_exps, ffn_u_, FF, nullptr, moe_ids_);
    d = single_token_desc(1, FF, EPI_STORE, 2, ffn_, nullptr, 0.0f, aq_ff_);
    d.n_sel = KU; d.sel_nx_stride = FF; d.sel_out_stride = E;
    d.seg[0] = make_seg(L.down_exps, moe_out_, E, nullptr, moe_ids_);
    return mmvq_fast_applicable(a) && mmvq_fast_applicable(d);
}

// mixture-of-experts feed-forward, prompt batch on plane sets: every expert's batch in ONE launch per projection (the workgroups find their expert and
// token tile from the counts on the device): no host synchronisation in the layer, and ~128-token batches that half-fill a launch each become one launch
// that fills the chip
hipError_t Context::moe_grouped_one_launch(int il, int T) {
    const HParams &hp = model->hp;
    const LayerWeights &L = model->layers[(size_t)il];
    const int E = hp.n_embd, FF = hp.n_ff, KU = hp.n_expert_used, NE = hp.n_expert, GR = T * KU;
    HIP_TRY(launch_moe_gather_act(aq_e_, moe_tok_, GR, E, aq_eg_, stream_));
    prep_owner_ = nullptr;
    const size_t ps_gu = L.gate_exps.planes_bytes / (size_t)L.gate_exps.n_expert, ps_d = L.down_exps.planes_bytes / (size_t)L.down_exps.n_expert;
    HIP_TRY(launch_mmq_planes_swiglu_moe(L.gate_exps.type, L.gate_exps.planes, L.up_exps.planes, ps_gu, NE, moe_meta_, (int)L.gate_exps.N, E, GR, aq_eg_, ffn_g_, FF, stream_));
    if (imx_on_) HIP_TRY(imx_collect(il, IMX_FFN_DOWN, ffn_g_, nullptr, FF, GR, nullptr, moe_meta_));     // the epilogue left silu(gate) * up
    HIP_TRY(launch_quantize(ffn_g_, FF, GR, aq_ffg_, true, false, stream_));
    HIP_TRY(launch_mmq_planes_moe(L.down_exps.type, L.down_exps.planes, ps_d, NE, moe_meta_, (int)L.down_exps.N, FF, GR, aq_ffg_, y_g_, E, stream_));
    return launch_moe_scatter_combine(x_, y_g_, moe_w_, moe_slot_, T, E, KU, stream_);
}

// ... the same for expert tensors with Q8_0-layout copies (MXFP4): gather, gate | up in one launch of two segments, SwiGLU + Q8_0 quantisation, down,
// scatter-combine - five launches a layer whatever the number of experts, no host synchronisation
hipError_t Context::moe_grouped_q80(int il, int T) {
    const HParams &hp = model->hp;
    const LayerWeights &L = model->layers[(size_t)il];
    const int E = hp.n_embd, FF = hp.n_ff, KU = hp.n_expert_used, NE = hp.n_expert, GR = T * KU;
    HIP_TRY(launch_moe_gather_act(aq_e_, moe_tok_, GR, E, aq_eg_, stream_));
    prep_owner_ = nullptr;
    const uint8_t *w_gu[2] = {L.gate_exps.planes, L.up_exps.planes}, *w_d[1] = {L.down_exps.planes};
    float *o_gu[2] = {ffn_g_, ffn_ug_}, *o_d[1] = {y_g_};
    HIP_TRY(launch_mmq_q80_moe(L.gate_exps.type, w_gu, o_gu, 2, L.gate_exps.planes_bytes / (size_t)L.gate_exps.n_expert, NE, moe_meta_, (int)L.gate_exps.N, E, GR, aq_eg_, FF, stream_));
    if (imx_on_) HIP_TRY(imx_collect(il, IMX_FFN_DOWN, ffn_g_, ffn_ug_, FF, GR, nullptr, moe_meta_));
    HIP_TRY(launch_swiglu_quant(ffn_g_, ffn_ug_, FF, GR, aq_ffg_, false, true, stream_, nullptr, nullptr));
    HIP_TRY(launch_mmq_q80_moe(L.down_exps.type, w_d, o_d, 1, L.down_exps.planes_bytes / (size_t)L.down_exps.n_expert, NE, moe_meta_, (int)L.down_exps.N, FF, GR, aq_ffg_, E, stream_));
    return launch_moe_scatter_combine(x_, y_g_, moe_w_, moe_slot_, T, E, KU, stream_);
}

// ... grouped, one batched contraction per expert and projection through linear(): the batch sizes come back to the host first (prompt batches only: never
// inside a graph)
// q80_any: the layer qualifies for moe_grouped_q80 and the "moe_q80_grouped" switch is off - every expert's batch, also one below 32 tokens, then runs the Q8_0
// prompt kernel on the expert's copy, so that the two settings of the switch give the same bits
hipError_t Context::moe_grouped_per_expert(int il, int T, bool q80_any) {
    const HParams &hp = model->hp;
    const LayerWeights &L = model->layers[(size_t)il];
    const int E = hp.n_embd, FF = hp.n_ff, KU = hp.n_expert_used, NE = hp.n_expert, GR = T * KU;
    HIP_TRY(hipMemcpyAsync(h_moe_meta_, moe_meta_, (size_t)(2 * NE + 1) * 4, hipMemcpyDeviceToHost, stream_));
    HIP_TRY(launch_moe_gather_act(aq_e_, moe_tok_, GR, E, aq_eg_, stream_));
    prep_owner_ = nullptr;                             // the grouped rows were just rewritten
    HIP_TRY(hipStreamSynchronize(stream_));            // the batch sizes size the launches
    auto view = [](const DevTensor &w, int e) {
        DevTensor v = w;
        v.data = w.data + (size_t)e * w.row_bytes * (size_t)w.N;
        v.n_expert = 1;
        v.planes = w.planes ? w.planes + (size_t)e * (w.planes_bytes / (size_t)w.n_expert) : nullptr;
        return v;
    };
    auto rows = [](const ActQuant &q, int r0, int K) {
        ActQuant v;
        if (q.qs) { v.qs = q.qs + (size_t)r0 * K; v.d = q.d + (size_t)r0 * (K / 256); v.bsums = q.bsums + (size_t)r0 * (K / 16); }
        if (q.qs0) { v.qs0 = q.qs0 + (size_t)r0 * K; v.d0 = q.d0 + (size_t)r0 * (K / 32); }
        return v;
    };
    auto copy_batch = [&](const DevTensor &w, int e, const ActQuant &q, int K, int n_e, float *out, int ld_out) {
        return launch_mmq_q80(w.planes + (size_t)e * (w.planes_bytes / (size_t)w.n_expert), mmq_q80_copy_row_bytes(w.type, K), (int)w.N, K, n_e, q, out, ld_out, nullptr, stream_,
                              mmq_q80_copy_form(w.type), true);
    };
    // the block-sum planes of ALL grouped rows in one launch (they were one launch per expert and projection: 16 a layer);
    // an expert's batch takes its slice of them
    const bool pl_gu = !act_is_q80(L.gate_exps.type) || !act_is_q80(L.up_exps.type), pl_d = !act_is_q80(L.down_exps.type);
    if (pl_gu) HIP_TRY(launch_mmq_prep(aq_eg_, E, GR, mmq_bh_, mmq_bl_, stream_));
    hipError_t e_exp = hipSuccess;
    for (int e = 0; e < NE && e_exp == hipSuccess; e++) {
        const int n_e = h_moe_meta_[e], r0 = h_moe_meta_[NE + e];
        if (n_e <= 0) continue;
        if (pl_gu) { bh_over_ = mmq_bh_ + (size_t)r0 * (E >> 4); bl_over_ = mmq_bl_ + (size_t)r0 * (E >> 4); }
        if (q80_any) {
            e_exp = copy_batch(L.gate_exps, e, rows(aq_eg_, r0, E), E, n_e, ffn_g_ + (size_t)r0 * FF, FF);
            if (e_exp == hipSuccess) e_exp = copy_batch(L.up_exps, e, rows(aq_eg_, r0, E), E, n_e, ffn_ug_ + (size_t)r0 * FF, FF);
            continue;
        }
        e_exp = linear(view(L.gate_exps, e), rows(aq_eg_, r0, E), nullptr, E, n_e, ffn_g_ + (size_t)r0 * FF, FF, nullptr, EPI_STORE);
        if (e_exp == hipSuccess) e_exp = linear(view(L.up_exps, e), rows(aq_eg_, r0, E), nullptr, E, n_e, ffn_ug_ + (size_t)r0 * FF, FF, nullptr, EPI_STORE);
    }
    bh_over_ = bl_over_ = nullptr;
    HIP_TRY(e_exp);
    if (imx_on_) HIP_TRY(imx_collect(il, IMX_FFN_DOWN, ffn_g_, ffn_ug_, FF, GR, nullptr, moe_meta_));
    HIP_TRY(launch_swiglu_quant(ffn_g_, ffn_ug_, FF, GR, aq_ffg_, !act_is_q80(L.down_exps.type), act_is_q80(L.down_exps.type), stream_,
                                pl_d ? mmq_bh_ : nullptr, pl_d ? mmq_bl_ : nullptr));
    prep_owner_ = nullptr;
    for (int e = 0; e < NE && e_exp == hipSuccess; e++) {
        const int n_e = h_moe_meta_[e], r0 = h_moe_meta_[NE + e];
        if (n_e <= 0) continue;
        if (pl_d) { bh_over_ = mmq_bh_ + (size_t)r0 * (FF >> 4); bl_over_ = mmq_bl_ + (size_t)r0 * (FF >> 4); }
        if (q80_any) { e_exp = copy_batch(L.down_exps, e, rows(aq_ffg_, r0, FF), FF, n_e, y_g_ + (size_t)r0 * E, E); continue; }
        e_exp = linear(view(L.down_exps, e), rows(aq_ffg_, r0, FF), nullptr, FF, n_e, y_g_ + (size_t)r0 * E, E, nullptr, EPI_STORE);
    }
    bh_over_ = bl_over_ = nullptr;
    HIP_TRY(e_exp);
    return launch_moe_scatter_combine(x_, y_g_, moe_w_, moe_slot_, T, E, KU, stream_);
}

// ... and a few tokens: the selected experts of a single token in one launch per projection (moe_selected_desc), else a mat-vec per (token, expert)
hipError_t Context::moe_selected(int il, int T) {
    const HParams &hp = model->hp;
    const LayerWeights &L = model->layers[(size_t)il];
    const int E = hp.n_embd, FF = hp.n_ff, KU = hp.n_expert_used;
    MMVQArgs a{}, d{};
    if (T == 1 && moe_selected_desc(il, a, d)) {
        HIP_TRY(launch_mmvq(a, stream_));          // the weight stream where it has a form for the shape, else the register ring (bit-identical)
        HIP_TRY(launch_mmvq(d, stream_));
        return launch_moe_combine(x_, moe_out_, moe_w_, T, E, KU, (size_t)T * E, stream_);
    }
    // quantise inside the down projection's prologue where the persistent mat-vec takes this shape (as the dense feed-forward does), else as its own launch
    const bool fuse_q = type_is_kq456(L.down_exps.type) && (FF % 256) == 0 && mmvq_fast_kb_ok((FF + 2047) / 2048);
    for (int t = 0; t < T; t++) {
        for (int j = 0; j < KU; j++) {
            const int32_t *esel = moe_ids_ + (size_t)t * KU + j;
            a = MMVQArgs{};
            a.n_seg = 2; a.K = E; a.T = 1; a.epi = EPI_SWIGLU;
            a.seg[0] = make_seg(L.gate_exps, ffn_ + (size_t)t * FF, FF, nullptr, esel);
            a.seg[1] = make_seg(L.up_exps, ffn_u_ + (size_t)t * FF, FF, nullptr, esel);
            chunk_act(a, aq_e_, E, t);
            if (L.gate_exps.type == L.up_exps.type) {
                HIP_TRY(launch_mmvq(a, stream_));
            } else {
                a.epi = EPI_STORE;
                HIP_TRY(launch_mmvq(a, stream_));
                HIP_TRY(launch_swiglu(ffn_ + (size_t)t * FF, ffn_u_ + (size_t)t * FF, ffn_ + (size_t)t * FF, FF, stream_));
            }
            if (!fuse_q) { HIP_TRY(launch_quantize(ffn_ + (size_t)t * FF, FF, 1, aq_ff_, !act_is_q80(L.down_exps.type), act_is_q80(L.down_exps.type), stream_)); prep_owner_ = nullptr; }
            d = MMVQArgs{};
            d.n_seg = 1; d.K = FF; d.T = 1; d.epi = EPI_STORE;
            if (fuse_q) { d.fuse_mode = 2; d.nx = ffn_ + (size_t)t * FF; }
            d.seg[0] = make_seg(L.down_exps, moe_out_ + ((size_t)j * T + t) * E, E, nullptr, esel);
            chunk_act(d, aq_ff_, FF, 0);
            HIP_TRY(launch_mmvq(d, stream_));
        }
    }
    return launch_moe_combine(x_, moe_out_, moe_w_, T, E, KU, (size_t)T * E, stream_);
}

// mixture-of-experts feed-forward: RMSNorm, router, then the experts in the form the batch size picks (the result is added to x_ by the combine launch)
hipError_t Context::ffn_moe(int il, const Step &st) {
    const HParams &hp = model->hp;
    const LayerWeights &L = model->layers[(size_t)il];
    const int E = hp.n_embd, FF = hp.n_ff, T = st.T, KU = hp.n_expert_used;
    HIP_TRY(launch_rmsnorm_quant(x_, (const float *)L.ffn_norm.data, E, T, hp.eps, xn_, &aq_e_,
                                 !act_is_q80(L.gate_exps.type) || !act_is_q80(L.up_exps.type), act_is_q80(L.gate_exps.type) || act_is_q80(L.up_exps.type), stream_));
    prep_owner_ = nullptr;
    prof_mark("norm_quant");
    const int32_t *forced = moe_forced_T_ == T ? d_moe_forced_ + (size_t)il * T * KU : nullptr;
    // the fused router computes a token's logits in ONE workgroup: the fastest form at 8 experts (4.9 us against 7.0 for the two launches below,
    // one token, K 2048), the slowest from 64 on (22 / 42 / 82 us at 64 / 128 / 256 experts against 9.4 / 9.5 / 13.2); the two give the same bits
    if ((L.gate_inp.type == T_F32 || L.gate_inp.type == T_F16) && hp.n_expert <= 8) {
        HIP_TRY(launch_moe_router(L.gate_inp.type, L.gate_inp.data, hp.n_expert, E, xn_, T, KU, router_, moe_ids_, moe_w_, stream_, forced));
    } else {
        HIP_TRY(launch_mmv_float(L.gate_inp.type, L.gate_inp.data, hp.n_expert, E, xn_, T, router_, hp.n_expert, nullptr, stream_));
        HIP_TRY(launch_moe_route(router_, T, hp.n_expert, KU, moe_ids_, moe_w_, stream_, forced));
    }
    prof_mark("moe_route");
    const bool exps_q = type_is_quant(L.gate_exps.type) && type_is_quant(L.up_exps.type) && type_is_quant(L.down_exps.type);
    if (imx_on_) HIP_TRY(imx_collect(il, IMX_ROUTER, xn_, nullptr, E, T, nullptr, nullptr));
    if (exps_q && (T >= g_moe_group_min || imx_on_) && aq_eg_.qs) {       // (the collector reads the grouped rows: grouped at every T)
        // ggml_mul_mat_id on a batch: group the (token, rank) pairs by expert, one contiguous activation batch per
        // expert (its weights are read once per batch, through the same batched kernels as the dense projections)
        HIP_TRY(launch_moe_group(moe_ids_, T, KU, hp.n_expert, moe_meta_, moe_slot_, moe_tok_, stream_));
        if (imx_on_) HIP_TRY(imx_collect(il, IMX_FFN_IN, xn_, nullptr, E, T * KU, moe_tok_, moe_meta_));    // a grouped row's token's row, per expert
        const bool one_launch = T >= 32 && L.gate_exps.planes && L.up_exps.planes && L.down_exps.planes && L.gate_exps.type == L.up_exps.type &&
                                L.gate_exps.N == L.up_exps.N && mmq_planes_moe_ok(L.gate_exps.type, (int)L.gate_exps.N, E) &&
                                mmq_planes_moe_ok(L.down_exps.type, (int)L.down_exps.N, FF) && (L.gate_exps.N % 64) == 0;
        // MXFP4 expert tensors (Q8_0-layout copies, Q8_0 activations): the grouped-expert form of the Q8_0 prompt kernel
        const bool q80_ok = T >= 32 && L.gate_exps.planes && L.up_exps.planes && L.down_exps.planes && L.gate_exps.type == T_MXFP4 && L.up_exps.type == T_MXFP4 &&
                            L.down_exps.type == T_MXFP4 && L.gate_exps.N == L.up_exps.N && mmq_q80_moe_ok(T_MXFP4, (int)L.gate_exps.N, E) &&
                            mmq_q80_moe_ok(T_MXFP4, (int)L.down_exps.N, FF) && aq_eg_.qs0 && aq_ffg_.qs0;
        if (q80_ok && g_moe_q80_grouped) HIP_TRY(moe_grouped_q80(il, T));
        else HIP_TRY(one_launch ? moe_grouped_one_launch(il, T) : moe_grouped_per_expert(il, T, q80_ok));
    } else {
        HIP_TRY(moe_selected(il, T));
    }
    prof_mark("moe_ffn");
    return hipSuccess;
}

hipError_t Context::ffn_block(int il, const Step &st) {
    if (model->hp.n_expert > 0) return ffn_moe(il, st);
    bool quantised = false;
    HIP_TRY(ffn_dense_gate_up(il, st, quantised));
    HIP_TRY(ffn_down(il, st, quantised));
    if (st.tp) HIP_TRY(tp_reduce_into_x(st.T));
    prof_mark("ffn_down");
    return hipSuccess;
}

// debug taps: the layer's output rows
hipError_t Context::tap_layer(int il, int T) {
    if (!debug_taps_ || !dbg_) return hipSuccess;
    return hipMemcpyAsync(dbg_ + (size_t)il * cp.n_ubatch * model->hp.n_embd, x_, (size_t)T * model->hp.n_embd * 4, hipMemcpyDeviceToDevice, stream_);
}

hipError_t Context::run_layers(int T, int n_kv_cap) {
    if (model->hp.encoder) return run_layers_encoder(T, n_kv_cap);
    cur_T_ = T;
    const HParams &hp = model->hp;
    const int E = hp.n_embd, FF = hp.n_ff;
    Step st = step_constants(T, n_kv_cap);
    att_splits_ = flash_attn_pick_splits(T, hp.n_head_kv, st.n_kv_max);

    // single-token step on a dense K-quant model: all layers in one launch (decode_mega.hip)
    bool mega = T == 1 && !profile_ && !debug_taps_ && !ub_embd_ && lora_.empty() && !imx_on_ && !cvec_on_ && mega_prepare();
    AttnArgs ma{};
    if (mega) {
        ma = attn_args(0, 1, st.n_kv_max, d_pos_);             // (the kernel takes each layer's cache from its own descriptor)
        ma.out_q = &aq_o_; ma.out_q8k = !act_is_q80(model->layers[0].wo.type); ma.out_q80 = false;
        ma.splits = flash_attn_decode_splits(st.n_kv_max);
        if (st.chunk_lists) attn_chunk_lists(ma);
        mega = flash_attn_decode_fused_applicable(ma, st.ra_step);      // (more than 64 chunks: the per-launch path merges them)
    }
    // ... or one persistent launch per layer for the mat-vecs between two attention calls (decode_engine.hip)
    st.engine = T == 1 && !mega && !profile_ && !debug_taps_ && !ub_embd_ && lora_.empty() && !imx_on_ && !cvec_on_ && engine_prepare();
    last_layers_engine_ = st.engine;
    // cos / sin table, cell metadata and the tokens' embedding rows: one launch
    HIP_TRY(launch_step_setup_embed(d_pos_, T, st.ra_step, rope_cs_, d_cell_pos_, d_cell_seq_, d_cell_, d_seqmask_, mega ? d_mega_sync_ : nullptr,
                                    d_step_serial_, model->tok_embd.type, model->tok_embd.data, E, d_tok_, x_, stream_));
    // an embeddings batch: the caller's rows take the place of the looked-up ones (never inside a captured graph: decode_ubatch)
    if (ub_embd_) HIP_TRY(hipMemcpyAsync(x_, ub_embd_, (size_t)T * E * sizeof(float), hipMemcpyHostToDevice, stream_));
    prof_mark("embed");
    last_layers_mega_ = mega;
    if (mega)
        return launch_decode_mega(d_mega_layers_, hp.n_layer, (E + 2047) >> 11, (FF + 2047) >> 11, ma, rope_cs_, st.ra_step.n_rot, k_, v_, d_cell_,
                                  att_counters_, d_mega_sync_, h_mega_flag_, d_mega_probe_, mega_lds_, stream_);

    for (int il = 0; il < hp.n_layer; il++) {
        const AttnPlan ap = plan_attn(il, st);
        HIP_TRY(attn_qkv(il, st, ap));
        HIP_TRY(attn_core(il, st, ap));
        if (st.engine) {   // attn_output, gate | up, down and the next layer's Q | K | V in one launch
            HIP_TRY(launch_decode_engine(d_engine_layers_ + il, E, FF, d_engine_gran_, d_engine_epoch_, il, il == engine_probe_layer_ ? d_engine_probe_ : nullptr, stream_));
        } else {
            HIP_TRY(attn_output(il, st, ap));
            if (st.tp) HIP_TRY(tp_reduce_into_x(T));
            prof_mark("attn_out");
            HIP_TRY(ffn_block(il, st));
        }
        HIP_TRY(cvec_add(il, T));
        HIP_TRY(tap_layer(il, T));
    }
    return hipSuccess;
}

hipError_t Context::tp_reduce_into_x(int T) {
    return tp_all_reduce_sum(tp_part_, x_, (size_t)T * model->hp.n_embd, stream_);
}

hipError_t Context::run_output(int n_out, int out_base) {
    logits_on_host_ = false;
    if (n_out <= 0) return hipSuccess;
    const HParams &hp = model->hp;
    const int E = hp.n_embd, V = hp.n_vocab;
    // (a single-token step has one row and it is the flagged one: no gather launch)
    float *const xo = cur_T_ == 1 && n_out == 1 ? x_ : xo_;
    if (xo != x_) HIP_TRY(launch_gather_rows_f32(x_, d_outrow_, n_out, E, xo_, stream_));
    if (hp.encoder) {                                        // the embeddings ARE the last layer's rows (t_embd of llm_build_bert): no final norm, no head
        HIP_TRY(hipMemcpyAsync(d_embd_ + (size_t)out_base * E, xo, (size_t)n_out * E * 4, hipMemcpyDeviceToDevice, stream_));
        prof_mark("embd");
        return hipSuccess;
    }
    if (embeddings_enabled) {
        // embeddings mode (llama_set_embeddings): output = result_norm rows, no lm-head (pooling NONE on this architecture)
        HIP_TRY(launch_rmsnorm_quant(xo, (const float *)model->out_norm.data, E, n_out, hp.eps, d_embd_ + (size_t)out_base * E, nullptr, false, false, stream_));
        prof_mark("embd");
        return hipSuccess;
    }
    const bool oq = type_is_quant(model->output.type);
    const bool imx_head = imx_on_ && imx_output_;
    const bool lora_head = lora_on(-1, LORA_OUTPUT);              // the delta is added onto the device row
    const bool head_rows = lora_head || imx_head;                 // either reads the norm's f32 rows: the norm as a launch of its own, its rows in xn_
    // a single-token step whose logits row is wanted on the host: the head's launch stores it into the pinned row itself (the row crosses PCIe under the
    // launch; a copy node behind it cost 9 - 12 us of every step, tools/host_gap.py)
    static const bool zc_env = !(getenv("MI355_LOGITS_ZERO_COPY") && getenv("MI355_LOGITS_ZERO_COPY")[0] == '0');
    logits_on_host_ = zc_env && oq && cur_T_ == 1 && n_out == 1 && cp.logits_to_host && !hp.tp_exchange && h_logits_ != nullptr && !head_rows;
    if (oq && can_fuse(E, n_out) && !head_rows) {
        pending_fuse_.mode = 1; pending_fuse_.x = xo; pending_fuse_.w = (const float *)model->out_norm.data; pending_fuse_.eps = hp.eps;
    } else {
        prep_owner_ = nullptr;
        HIP_TRY(launch_rmsnorm_quant(xo, (const float *)model->out_norm.data, E, n_out, hp.eps, oq && !head_rows ? nullptr : xn_, &aq_e_,
                                     oq && !act_is_q80(model->output.type), act_is_q80(model->output.type), stream_));
        prof_mark("norm_quant");
        if (imx_head) HIP_TRY(imx_collect(-1, IMX_QKV, xn_, nullptr, E, n_out, nullptr, nullptr));
    }
    float *lg = d_logits_ + (size_t)out_base * V;
    const int VL = hp.n_vocab_local, P = hp.tp_size;
    if (hp.tp_exchange && VL * P == V) {
        // vocabulary rows are cut across the ranks: each computes its slice of every flagged row, the slices are gathered
        // rank-major and copied into place (for a single row the gathered buffer already is the logits row)
        if (n_out > 1 && (size_t)n_out > tp_logits_rows_) {      // (never inside a capture: graphs carry single-row steps only)
            HIP_TRY(hipStreamSynchronize(stream_));
            tp_logits_ = (float *)dalloc((size_t)n_out * V * 4);
            if (!tp_logits_) return hipErrorOutOfMemory;
            tp_logits_rows_ = (size_t)n_out;
            HIP_TRY(hipDeviceSynchronize());
        }
        float *gathered = n_out == 1 ? lg : tp_logits_;
        float *part = gathered + (size_t)hp.tp_rank * n_out * VL;
        HIP_TRY(linear(model->output, aq_e_, xn_, E, n_out, part, VL, nullptr, EPI_STORE));
        pending_fuse_ = Fuse();
        HIP_TRY(tp_all_gather(part, gathered, (size_t)n_out * VL, stream_));
        for (int r = 0; r < P && n_out > 1; r++)
            HIP_TRY(hipMemcpy2DAsync(lg + (size_t)r * VL, (size_t)V * 4, tp_logits_ + (size_t)r * n_out * VL, (size_t)VL * 4, (size_t)VL * 4, (size_t)n_out,
                                     hipMemcpyDeviceToDevice, stream_));
    } else {
        if (logits_on_host_) pending_fuse_.out_host = h_logits_ + (size_t)out_base * V;
        HIP_TRY(linear(model->output, aq_e_, xn_, E, n_out, lg, V, nullptr, EPI_STORE));
        if (lora_head) {
            const int target = LORA_OUTPUT;
            HIP_TRY(lora_add(-1, &target, &lg, &V, 1, xn_, E, E, n_out));
        }
    }
    pending_fuse_ = Fuse();
    prof_mark("lm_head");
    for (int r0 = 0; r0 < n_out; r0 += (int)cp.n_ubatch) {
        const int nr = std::min((int)cp.n_ubatch, n_out - r0);
        // the winner goes straight into pinned host memory (visible once the stream has drained): no copy node
        HIP_TRY(launch_argmax_rows(lg + (size_t)r0 * V, V, nr, h_argmax_ + out_base + r0, argmax_scratch_, (int)cp.n_ubatch, stream_));
    }
    prof_mark("argmax");
    return hipSuccess;
}

int Context::decode_ubatch(int n, const int32_t *tokens, const int32_t *pos, const int32_t *seq, const uint64_t *seqmask,
                           const int8_t *flags, int out_base) {
    { const unsigned long long ls = next_launch_serial(); if (!first_unchecked_launch_) first_unchecked_launch_ = ls; }   // (stream_check: who is a suspect)
    cur_max_pos_ = 0;
    for (int i = 0; i < n; i++) cur_max_pos_ = std::max(cur_max_pos_, (int)pos[i]);
    std::vector<int> tcell;
    if (!alloc_cells(n, seqmask, tcell)) return 1;
    for (int i = 0; i < n; i++) {
        KVCell &c = cells_[(size_t)tcell[(size_t)i]];
        c.pos = pos[i]; c.seqs = seqmask[i]; c.delta = 0;
    }
    int hi = 0;
    for (int i = (int)cells_.size() - 1; i >= 0; i--) if (cells_[(size_t)i].pos >= 0) { hi = i + 1; break; }
    n_kv_ = std::min((int)cp.n_ctx, (hi + 31) & ~31);

    if (meta_dirty_) {   // sequence ops since the last batch: re-upload the whole cell table
        std::vector<int32_t> cpos(cells_.size());
        std::vector<uint64_t> cseq(cells_.size());
        for (size_t i = 0; i < cells_.size(); i++) { cpos[i] = cells_[i].pos; cseq[i] = cells_[i].seqs; }
        if (hipMemcpyAsync(d_cell_pos_, cpos.data(), cpos.size() * 4, hipMemcpyHostToDevice, stream_) != hipSuccess ||
            hipMemcpyAsync(d_cell_seq_, cseq.data(), cseq.size() * 8, hipMemcpyHostToDevice, stream_) != hipSuccess ||
            hipStreamSynchronize(stream_) != hipSuccess) { last_error = "cell table upload failed"; return -1; }
        meta_dirty_ = false;
    }
    // stage token arrays (the pinned block may still be in flight from the previous micro-batch)
    if (stage_event_) (void)hipEventSynchronize(stage_event_);
    const size_t T = ((size_t)cp.n_ubatch + 1) & ~(size_t)1;
    int32_t *h_nkv = (int32_t *)h_stage_;
    int32_t *h_tok = (int32_t *)(h_stage_ + 16), *h_pos = h_tok + T, *h_seq = h_pos + T, *h_cell = h_seq + T, *h_out = h_cell + T;
    uint64_t *h_mask = (uint64_t *)(h_out + T);
    h_nkv[0] = n_kv_;
    int n_out = 0;
    for (int i = 0; i < n; i++) {
        h_tok[i] = tokens[i]; h_pos[i] = pos[i]; h_seq[i] = seq[i]; h_cell[i] = tcell[(size_t)i]; h_mask[i] = seqmask[i];
        if (flags[i]) h_out[n_out++] = i;
    }
    if (hipMemcpyAsync(d_stage_, h_stage_, stage_bytes_, hipMemcpyHostToDevice, stream_) != hipSuccess) { last_error = "token upload failed"; return -1; }
    // continuous-batching steps (a few tokens, usually one per sequence): each token scans only the 64-cell chunks that
    // hold cells of its own sequence instead of the whole cache
    chunk_lmax_ = 0;
    batch_distinct_ = n >= 2 && n <= 64;                       // every token in exactly one sequence, no two in the same one (a continuous-batching step)
    {
        uint64_t seen = 0;
        for (int i = 0; i < n && batch_distinct_; i++) {
            const uint64_t mk = seqmask[i];
            if (mk == 0 || (mk & (mk - 1)) != 0 || (seen & mk) != 0) batch_distinct_ = false;
            seen |= mk;
        }
    }
    bool lists_usable = false;                                 // only the split-per-chunk attention kernels walk the lists
    {
        const HParams &hp = model->hp;
        RopeArgs ra = rope_args(*model, false);
        AttnArgs aa{};
        aa.T = n; aa.H = hp.n_head; aa.G = hp.n_head_kv; aa.D = hp.head_dim; aa.n_kv_max = n_kv_; aa.type_k = cp.type_k; aa.type_v = cp.type_v;
        lists_usable = n <= 64 && flash_attn_decode_applicable(aa, ra) && kv_store_fast_applicable(aa.G, aa.D, cp.type_k, cp.type_v, ra);
    }
    if ((n >= 2 || cp.n_seq_max > 1) && lists_usable) {
        chunk_lmax_ = build_attn_chunk_lists(n_kv_, (int)cells_.size(), [&](int i, int32_t &p, uint64_t &m) { p = cells_[(size_t)i].pos; m = cells_[(size_t)i].seqs; },
                                             seq, n, chunk_stride_, h_chunks_, h_chunks_ + (size_t)64 * chunk_stride_);
        if (hipMemcpyAsync(d_chunks_, h_chunks_, (size_t)64 * (chunk_stride_ + 1) * 4, hipMemcpyHostToDevice, stream_) != hipSuccess) { last_error = "chunk list upload failed"; return -1; }
    }
    // rocprofv3 --pmc does not keep copy-engine transfers ordered with the kernels it serialises (observed: kernels reading
    // the previous step's token / position block); MI355_PROFILER_SAFE=1 drains the stream around the transfers
    static const bool profiler_safe = getenv("MI355_PROFILER_SAFE") && getenv("MI355_PROFILER_SAFE")[0] == '1';
    if (profiler_safe) (void)hipStreamSynchronize(stream_);
    if (!stage_event_) (void)hipEventCreateWithFlags(&stage_event_, hipEventDisableTiming);
    if (stage_event_) (void)hipEventRecord(stage_event_, stream_);

    const int V = model->hp.n_vocab;
    if (n == 1 && !model->hp.encoder && !ub_embd_) { (void)mega_prepare(); (void)engine_prepare(); }   // allocate and upload on first use: must not happen inside a stream capture
    // a single-token step would launch the attention + attn_output kernel whose workgroups wait for each other: only while no other context of this device has
    // such a step in flight (runtime.h fused_acquire); otherwise this step takes the wait-free launches, eagerly (the captured graphs hold the fused kernel)
    attn_out_skip_step_ = n == 1 && !attn_out_off_ && !model->hp.encoder && !fused_acquire();
    if (attn_out_skip_step_) fused_skipped_steps++;
    bool graph_ok = cp.use_graphs && n == 1 && n_out == 1 && out_base == 0 && !profile_ && !debug_taps_ && !embeddings_enabled && moe_forced_T_ == 0 && !ub_embd_ && !attn_out_skip_step_ && !imx_on_;
    hipError_t e = hipSuccess;
    if (graph_ok) {
        // the attention grid is sized for an upper bound of occupied cells; one captured graph per 256-cell bucket
        int bucket = std::min((int)cp.n_ctx, (n_kv_ + 255) & ~255);
        chunk_cap_ = 0;
        if (chunk_lmax_ > 0) {                                 // chunk lists: the grid is sized by the list length, in steps of 4
            chunk_cap_ = attn_chunk_grid(chunk_lmax_, chunk_stride_);
            bucket = -chunk_cap_;                              // separate key space from the cell-count buckets
        }
        auto git = graphs_.find(bucket);
        graph_exec_ = git == graphs_.end() ? nullptr : git->second;
        if (!graph_exec_) {
            hipGraph_t g = nullptr;
            std::string inner;                                  // which launch refused, when one did (HIP_TRY's message)
            e = hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal);
            if (e == hipSuccess) {
                last_error.clear();
                hipError_t e2 = run_layers(1, bucket > 0 ? bucket : std::min((int)cp.n_ctx, chunk_cap_ * 64));
                if (e2 == hipSuccess) e2 = run_output(1, 0);
                if (e2 == hipSuccess && cp.logits_to_host && !logits_on_host_) e2 = hipMemcpyAsync(h_logits_, d_logits_, (size_t)V * 4, hipMemcpyDeviceToHost, stream_);
                if (e2 != hipSuccess) inner = last_error;
                e = hipStreamEndCapture(stream_, &g);
                if (e2 != hipSuccess) e = e2;
            }
            if (e == hipSuccess) e = hipGraphInstantiate(&graph_exec_, g, nullptr, nullptr, 0);
            if (g) (void)hipGraphDestroy(g);
            if (e != hipSuccess && model->hp.tp_exchange) {
                // a collective that cannot be captured on this RCCL / driver pair: every rank fails the same way, so all
                // of them continue with eager launches from here on (nothing was executed during the failed capture)
                (void)hipGetLastError();
                cp.use_graphs = false;
                graph_ok = false;
                graph_exec_ = nullptr;
                e = hipSuccess;
            } else {
                if (e != hipSuccess) { last_error = std::string("graph capture failed: ") + hipGetErrorString(e) + (inner.empty() ? "" : " / " + inner); return -1; }
                graphs_[bucket] = graph_exec_;
                graph_is_mega_[graph_exec_] = last_layers_mega_;
                graph_is_engine_[graph_exec_] = last_layers_engine_;
            }
        }
        if (graph_ok) e = hipGraphLaunch(graph_exec_, stream_);
    }
    if (!graph_ok) {
        prof_begin();
        chunk_cap_ = chunk_lmax_;
        e = run_layers(n, n_kv_);
        if (e == hipSuccess) e = run_output(n_out, out_base);
        if (profiler_safe) (void)hipStreamSynchronize(stream_);
        if (e == hipSuccess && n_out > 0 && cp.logits_to_host && !embeddings_enabled && !logits_on_host_)
            e = hipMemcpyAsync(h_logits_ + (size_t)out_base * V, d_logits_ + (size_t)out_base * V, (size_t)n_out * V * 4, hipMemcpyDeviceToHost, stream_);
        prof_end();
    }
    if (e != hipSuccess) { last_error = std::string("decode failed: ") + hipGetErrorString(e) + " / " + last_error_string(); return -1; }
    if (n == 1 && (graph_ok ? graph_is_mega_[graph_exec_] : last_layers_mega_)) mega_steps++;
    if (n == 1 && (graph_ok ? graph_is_engine_[graph_exec_] : last_layers_engine_)) engine_steps++;
    dbg_tokens_ = n;
    return 0;
}

// GPU-side trace ranges (tracing row): with MI355_ROCTX=1 every decode call is a roctx range - "mi355_decode prompt n=512" / "mi355_decode step
// n=1" - so a rocprofv3 --marker-trace run shows where the batches begin and end between the kernels.  The marker library is looked up at run time
// (librocprofiler-sdk-roctx, then the legacy libroctx64); absent or switched off, a range costs one branch.
namespace {
struct RoctxApi {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    RoctxApi() {
        const char *ev = getenv("MI355_ROCTX");
        if (!ev || ev[0] != '1') return;
        for (const char *n : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
            if (void *h = dlopen(n, RTLD_NOW | RTLD_GLOBAL)) {
                push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
                pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
                if (push && pop) return;
                push = nullptr; pop = nullptr;
            }
        }
    }
};
struct TraceRange {
    static RoctxApi &api() { static RoctxApi a; return a; }
    bool on = false;
    TraceRange(const char *what, int n) {
        if (!api().push) return;
        char buf[96];
        snprintf(buf, sizeof buf, "mi355_decode %s n=%d", what, n);
        api().push(buf);
        on = true;
    }
    ~TraceRange() { if (on) api().pop(); }
};
}  // namespace

int Context::decode(int n_tokens, const int32_t *tokens, const int32_t *pos, const int32_t *n_seq_id, int32_t *const *seq_id,
                    const int8_t *logits_flags, const float *embd) {
    if (n_tokens <= 0) { last_error = "empty batch"; return -1; }
    const TraceRange trace_range(embd ? "embeddings" : n_tokens == 1 ? "step" : n_tokens <= 64 ? "steps" : "prompt", n_tokens);
    // llama_batch.embd: the rows ARE the layer stack's input (the image embeddings of a LLaVA request, llama_server_context.cc:1093-1107); no token ids then
    std::vector<int32_t> no_tokens;
    if (embd) {
        if (model->hp.encoder) { last_error = "an encoder model takes token ids, not embeddings"; return -1; }
        if (tokens) { last_error = "a batch carries token ids or embeddings, not both"; return -1; }
        if (!pos) { last_error = "an embeddings batch needs positions"; return -1; }
        no_tokens.assign((size_t)n_tokens, 0);
        tokens = no_tokens.data();
    } else if (!tokens) { last_error = "batch without tokens"; return -1; }
    if (hipSetDevice(model->device) != hipSuccess) return -1;
    const HParams &hp = model->hp;
    // bidirectional attention: every token of a sequence must see all the others, so a batch is never cut into micro-batches (llama.cpp asks the same: n_ubatch >= n_tokens)
    if (hp.encoder && (size_t)n_tokens > cp.n_ubatch) { last_error = "encoder model: a batch of " + std::to_string(n_tokens) + " tokens does not fit one micro-batch (n_ubatch " + std::to_string(cp.n_ubatch) + ")"; return -1; }
    if (has_shift_) apply_k_shift();
    if (debug_taps_ && !dbg_) dbg_ = (float *)dalloc((size_t)hp.n_layer * cp.n_ubatch * hp.n_embd * 4);

    std::vector<int32_t> seq((size_t)n_tokens);
    std::vector<uint64_t> mask((size_t)n_tokens);
    std::vector<int8_t> flags((size_t)n_tokens);
    int n_out = 0;
    out_row_of_batch_.assign((size_t)n_tokens, -1);
    for (int i = 0; i < n_tokens; i++) {
        if (tokens[i] < 0 || tokens[i] >= hp.n_vocab) { last_error = "token id " + std::to_string(tokens[i]) + " out of range [0, " + std::to_string(hp.n_vocab) + ")"; return -1; }
        // a negative position would mark the cell it is written to as free although its KV row was stored
        if (pos && pos[i] < 0) { last_error = "negative position " + std::to_string(pos[i]) + " for token " + std::to_string(i); return -1; }
        uint64_t mk = 0;
        const int ns = n_seq_id ? n_seq_id[i] : 1;
        for (int j = 0; j < ns; j++) {
            const int s = seq_id ? seq_id[i][j] : 0;
            if (s < 0 || s >= 64) { last_error = "seq id " + std::to_string(s) + " out of range [0, 64)"; return -1; }   // (the cell masks are 64 bits wide)
            mk |= 1ull << s;
        }
        seq[(size_t)i] = seq_id ? seq_id[i][0] : 0;
        mask[(size_t)i] = mk;
        // llama_decode: logits == NULL -> only the last token
        flags[(size_t)i] = logits_flags ? (logits_flags[i] != 0) : (i == n_tokens - 1);
        if (flags[(size_t)i]) out_row_of_batch_[(size_t)i] = n_out++;
    }
    // logits buffers
    if ((size_t)n_out > logits_cap_rows_) {
        (void)hipStreamSynchronize(stream_);
        if (d_logits_) { (void)hipFree(d_logits_); allocs_.erase(std::find(allocs_.begin(), allocs_.end(), (void *)d_logits_)); }
        if (h_logits_) (void)hipHostFree(h_logits_);
        if (d_argmax_) { /* sized n_ubatch; regrow below if needed */ }
        const size_t rows = std::max<size_t>((size_t)n_out, 1);
        d_logits_ = (float *)dalloc(rows * hp.n_vocab * 4);
        if (!d_logits_ || hipHostMalloc((void **)&h_logits_, rows * hp.n_vocab * 4, hipHostMallocDefault) != hipSuccess) { last_error = "logits alloc failed"; return -1; }
        if (rows > cp.n_ubatch) {
            d_argmax_ = (int32_t *)dalloc(rows * 4);
            (void)hipHostFree(h_argmax_);
            if (hipHostMalloc((void **)&h_argmax_, rows * 4, hipHostMallocDefault) != hipSuccess) return -1;
        }
        logits_cap_rows_ = rows;
        (void)hipDeviceSynchronize();                  // null-stream zero-fills of the new buffers (see init)
        for (auto &ge : graphs_) (void)hipGraphExecDestroy(ge.second);
        graphs_.clear();
        graph_exec_ = nullptr;
    }
    n_out_last_ = n_out;
    logits_fetched_ = false;
    embd_fetched_ = false;
    last_was_embd_ = embeddings_enabled;
    if (embeddings_enabled && (size_t)n_out > cp.n_ubatch) { last_error = "embeddings: more flagged rows than n_ubatch"; return -1; }
    argmax_fetched_ = false;

    const std::vector<KVCell> saved = cells_;
    const int saved_head = head_;
    int out_base = 0;
    for (int i0 = 0; i0 < n_tokens; i0 += (int)cp.n_ubatch) {
        const int n = std::min((int)cp.n_ubatch, n_tokens - i0);
        ub_embd_ = embd ? embd + (size_t)i0 * (size_t)hp.n_embd : nullptr;
        const int rc = decode_ubatch(n, tokens + i0, pos + i0, seq.data() + i0, mask.data() + i0, flags.data() + i0, out_base);
        ub_embd_ = nullptr;
        if (rc != 0) {
            cells_ = saved; head_ = saved_head; meta_dirty_ = true; region_next_.clear();
            return rc;
        }
        for (int i = 0; i < n; i++) out_base += flags[(size_t)(i0 + i)] ? 1 : 0;
    }
    moe_forced_T_ = 0;      // (force_moe_ids arms one call)
    return 0;
}

void Context::synchronize() { (void)hipStreamSynchronize(stream_); fused_release(); }

int Context::force_moe_ids(const int32_t *ids, int n_layer, int T, int k) {
    const HParams &hp = model->hp;
    if (!ids || hp.n_expert <= 0 || n_layer != hp.n_layer || k != hp.n_expert_used || T < 1 || T > (int)cp.n_ubatch) { last_error = "force_moe_ids: shape does not match the model"; return -1; }
    const int n = n_layer * T * k;
    if (hipSetDevice(model->device) != hipSuccess) return -1;
    if (n > moe_forced_cap_) {
        (void)hipStreamSynchronize(stream_);
        d_moe_forced_ = (int32_t *)dalloc((size_t)n * 4);
        if (!d_moe_forced_) { moe_forced_cap_ = 0; return -1; }
        moe_forced_cap_ = n;
    }
    if (hipMemcpyAsync(d_moe_forced_, ids, (size_t)n * 4, hipMemcpyHostToDevice, stream_) != hipSuccess || hipStreamSynchronize(stream_) != hipSuccess) return -1;
    moe_forced_T_ = T;
    return 0;
}

float *Context::logits_ith(int i) {
    if (last_was_embd_) return nullptr;            // embeddings mode computes no logits
    if (i < 0) i += (int)out_row_of_batch_.size();
    if (i < 0 || i >= (int)out_row_of_batch_.size() || out_row_of_batch_[(size_t)i] < 0) return nullptr;
    if (!logits_fetched_) {
        if (!cp.logits_to_host &&
            hipMemcpyAsync(h_logits_, d_logits_, (size_t)n_out_last_ * model->hp.n_vocab * 4, hipMemcpyDeviceToHost, stream_) != hipSuccess) return nullptr;
        if (hipStreamSynchronize(stream_) != hipSuccess || !mega_check() || !stream_check()) return nullptr;
        logits_fetched_ = true;
    }
    return h_logits_ + (size_t)out_row_of_batch_[(size_t)i] * model->hp.n_vocab;
}

float *Context::embeddings_ith(int i) {
    if (!last_was_embd_) return nullptr;
    if (i < 0) i += (int)out_row_of_batch_.size();
    if (i < 0 || i >= (int)out_row_of_batch_.size() || out_row_of_batch_[(size_t)i] < 0) return nullptr;
    const int E = model->hp.n_embd;
    if (!embd_fetched_) {
        if (hipMemcpyAsync(h_embd_, d_embd_, (size_t)n_out_last_ * E * 4, hipMemcpyDeviceToHost, stream_) != hipSuccess) return nullptr;
        if (hipStreamSynchronize(stream_) != hipSuccess) return nullptr;
        embd_fetched_ = true;
    }
    return h_embd_ + (size_t)out_row_of_batch_[(size_t)i] * E;
}

int32_t Context::argmax_ith(int i) {
    if (i < 0) i += (int)out_row_of_batch_.size();
    if (i < 0 || i >= (int)out_row_of_batch_.size() || out_row_of_batch_[(size_t)i] < 0) return -1;
    if (!argmax_fetched_) {
        if (hipStreamSynchronize(stream_) != hipSuccess || !mega_check() || !stream_check()) return -1;
        argmax_fetched_ = true;
    }
    return h_argmax_[out_row_of_batch_[(size_t)i]];
}

// ---- speculative decoding (csrc/spec.hip): both read d_logits_, which every decode fills whatever logits_to_host says (the head's launch stores the device
// row also when it writes the pinned one itself, logits_on_host_), and leave their few words in pinned memory: one launch, one synchronisation
bool Context::spec_prepare() {
    if (spec_scratch_) return true;
    if (hipSetDevice(model->device) != hipSuccess) return false;
    const size_t words = argmax_prob_scratch_words(1) + spec_verify_scratch_words(SPEC_MAX_ROWS), in_words = 2 * (size_t)SPEC_MAX_ROWS + SPEC_MAX_GROUPS + 1;
    const size_t host_words = in_words + SPEC_MAX_ROWS + SPEC_MAX_GROUPS + 2;
    (void)hipStreamSynchronize(stream_);
    // each block is allocated once: a failure leaves what succeeded in place (dalloc's blocks are the context's) and the next call asks only for the rest;
    // spec_scratch_ is set last, so it says that all three are there
    if (!h_spec_ && hipHostMalloc((void **)&h_spec_, host_words * 4, hipHostMallocDefault) != hipSuccess) { h_spec_ = nullptr; last_error = "speculative-decoding workspace allocation failed"; return false; }
    if (!d_spec_in_) d_spec_in_ = (int32_t *)dalloc(in_words * 4);
    float *scratch = d_spec_in_ ? (float *)dalloc(words * 4) : nullptr;   // (zero-filled: the ticket words)
    if (!scratch) { last_error = "speculative-decoding workspace allocation failed"; return false; }
    spec_scratch_ = scratch;
    (void)hipDeviceSynchronize();                                      // the null-stream zero-fills (see init)
    return true;
}

int32_t Context::argmax_prob_ith(int i, float *p) {
    if (last_was_embd_) { last_error = "argmax_prob: embeddings mode computes no logits"; return -1; }
    if (i < 0) i += (int)out_row_of_batch_.size();
    if (i < 0 || i >= (int)out_row_of_batch_.size() || out_row_of_batch_[(size_t)i] < 0) { last_error = "argmax_prob: no logits for that batch row"; return -1; }
    if (!spec_prepare()) return -1;
    const int V = model->hp.n_vocab;
    int32_t *h_idx = h_spec_ + 2 * SPEC_MAX_ROWS + SPEC_MAX_GROUPS + 1 + SPEC_MAX_ROWS + SPEC_MAX_GROUPS;
    float *h_p = reinterpret_cast<float *>(h_idx + 1);
    if (launch_argmax_prob_rows(d_logits_ + (size_t)out_row_of_batch_[(size_t)i] * V, V, nullptr, 1, h_idx, h_p, spec_scratch_, 1, stream_) != hipSuccess) {
        last_error = "argmax_prob launch failed"; return -1;
    }
    if (hipStreamSynchronize(stream_) != hipSuccess || !mega_check() || !stream_check()) return -1;
    argmax_fetched_ = true;
    if (p) *p = *h_p;
    return *h_idx;
}

int Context::spec_verify(int n_groups, const int32_t *group_start, const int32_t *draft, int32_t *ids_out, int32_t *n_accept_out) {
    if (last_was_embd_) { last_error = "spec_verify: embeddings mode computes no logits"; return -1; }
    if (model->hp.tp_size > 1) { last_error = "spec_verify: not on a rank of a row split"; return -1; }
    if (n_groups < 1 || n_groups > SPEC_MAX_GROUPS || !group_start || !draft || !ids_out || !n_accept_out) { last_error = "spec_verify: bad arguments (1 .. 64 groups)"; return -1; }
    const int b0 = group_start[0], R = group_start[n_groups] - b0;
    if (b0 < 0 || R < 1 || R > SPEC_MAX_ROWS || group_start[n_groups] > (int)out_row_of_batch_.size()) { last_error = "spec_verify: the groups do not lie inside the last batch"; return -1; }
    for (int g = 0; g < n_groups; g++) {
        const int rows = group_start[g + 1] - group_start[g];
        if (rows < 1 || rows > SPEC_MAX_DRAFT + 1) { last_error = "spec_verify: group " + std::to_string(g) + " has " + std::to_string(rows) + " rows (1 .. 17)"; return -1; }
    }
    for (int r = 0; r < R; r++)
        if (out_row_of_batch_[(size_t)(b0 + r)] < 0) { last_error = "spec_verify: batch row " + std::to_string(b0 + r) + " was not flagged for logits"; return -1; }
    if (!spec_prepare()) return -1;
    // rows | group starts (relative to the launch's first row) | drafts: one staged copy
    int32_t *h_rows = h_spec_, *h_gs = h_rows + R, *h_draft = h_gs + n_groups + 1;
    for (int r = 0; r < R; r++) { h_rows[r] = out_row_of_batch_[(size_t)(b0 + r)]; h_draft[r] = draft[r]; }
    for (int g = 0; g <= n_groups; g++) h_gs[g] = group_start[g] - b0;
    int32_t *h_ids = h_spec_ + 2 * SPEC_MAX_ROWS + SPEC_MAX_GROUPS + 1, *h_acc = h_ids + SPEC_MAX_ROWS;
    const size_t in_words = 2 * (size_t)R + (size_t)n_groups + 1;
    if (hipMemcpyAsync(d_spec_in_, h_spec_, in_words * 4, hipMemcpyHostToDevice, stream_) != hipSuccess) { last_error = "spec_verify staging failed"; return -1; }
    if (launch_spec_verify(d_logits_, model->hp.n_vocab, d_spec_in_, R, d_spec_in_ + R, n_groups, d_spec_in_ + R + n_groups + 1, h_ids, h_acc,
                           spec_scratch_ + argmax_prob_scratch_words(1), SPEC_MAX_ROWS, stream_) != hipSuccess) { last_error = "spec_verify launch failed"; return -1; }
    if (hipStreamSynchronize(stream_) != hipSuccess || !mega_check() || !stream_check()) return -1;
    argmax_fetched_ = true;
    memcpy(ids_out, h_ids, (size_t)R * 4);
    memcpy(n_accept_out, h_acc, (size_t)n_groups * 4);
    return R;
}

// ---- perplexity and KL divergence (csrc/logprob.hip): d_logits_ again; a launch takes at most n_ubatch rows (the scratch's size), a call
// queues as many launches as its rows need, the kernels write their two words per row straight into pinned memory, and ONE synchronisation ends the call
bool Context::logprob_prepare(int n) {
    if (hipSetDevice(model->device) != hipSuccess) { last_error = "logprob: cannot select the device"; return false; }
    const int cap = (int)std::min<uint32_t>(std::max<uint32_t>(cp.n_ubatch, 1), 65535);
    if (!lp_scratch_) {
        (void)hipStreamSynchronize(stream_);
        lp_scratch_ = (float *)dalloc((token_logprob_scratch_words(cap) + logits_kl_scratch_words(cap)) * 4);   // (zero-filled: the ticket words)
        (void)hipDeviceSynchronize();                                  // the null-stream zero-fill (see init)
        if (!lp_scratch_) { last_error = "logprob workspace allocation failed"; return false; }
    }
    if (n > lp_cap_) {
        (void)hipStreamSynchronize(stream_);
        const int want = std::max(n, cap);
        if (h_lp_) { (void)hipHostFree(h_lp_); h_lp_ = nullptr; }
        lp_cap_ = 0;
        if (d_lp_in_) {                                                // (the stream is idle: the block it outgrew goes back, as decode does with d_logits_)
            (void)hipFree(d_lp_in_);
            allocs_.erase(std::find(allocs_.begin(), allocs_.end(), (void *)d_lp_in_));
            d_lp_in_ = nullptr;
        }
        d_lp_in_ = (int32_t *)dalloc((size_t)want * 2 * 4);
        if (!d_lp_in_ || hipHostMalloc((void **)&h_lp_, (size_t)want * 4 * 4, hipHostMallocDefault) != hipSuccess) { h_lp_ = nullptr; last_error = "logprob workspace allocation failed"; return false; }
        lp_cap_ = want;
        (void)hipDeviceSynchronize();
    }
    return true;
}

// batch rows -> rows of d_logits_, every one flagged
bool Context::logprob_rows(const char *what, int n, const int32_t *batch_rows, int32_t *dst) {
    const int nb = (int)out_row_of_batch_.size();
    for (int r = 0; r < n; r++) {
        int i = batch_rows[r];
        if (i < 0) i += nb;
        if (i < 0 || i >= nb || out_row_of_batch_[(size_t)i] < 0) { last_error = std::string(what) + ": batch row " + std::to_string(batch_rows[r]) + " was not flagged for logits"; return false; }
        dst[r] = out_row_of_batch_[(size_t)i];
    }
    return true;
}

int Context::token_logprobs(int n, const int32_t *batch_rows, const int32_t *targets, float *logprob_out, int32_t *rank_out) {
    if (last_was_embd_) { last_error = "token_logprobs: embeddings mode computes no logits"; return -1; }
    if (model->hp.tp_size > 1) { last_error = "token_logprobs: not on a rank of a row split"; return -1; }
    if (n < 1 || !batch_rows || !targets || !logprob_out) { last_error = "token_logprobs: bad arguments"; return -1; }
    const int V = model->hp.n_vocab;
    for (int r = 0; r < n; r++)
        if (targets[r] < 0 || targets[r] >= V) { last_error = "token_logprobs: target " + std::to_string(targets[r]) + " outside [0, " + std::to_string(V) + ")"; return -1; }
    std::vector<int32_t> rows((size_t)n);
    if (!logprob_rows("token_logprobs", n, batch_rows, rows.data())) return -1;
    if (!logprob_prepare(n)) return -1;
    // pinned: rows | targets, then logprob | rank
    int32_t *h_rows = h_lp_, *h_tgt = h_lp_ + n, *h_rank = h_lp_ + 2 * (size_t)lp_cap_ + n;
    float *h_out = reinterpret_cast<float *>(h_lp_ + 2 * (size_t)lp_cap_);
    memcpy(h_rows, rows.data(), (size_t)n * 4);
    memcpy(h_tgt, targets, (size_t)n * 4);
    if (hipMemcpyAsync(d_lp_in_, h_lp_, (size_t)n * 2 * 4, hipMemcpyHostToDevice, stream_) != hipSuccess) { last_error = "token_logprobs staging failed"; return -1; }
    const int cap = (int)std::min<uint32_t>(std::max<uint32_t>(cp.n_ubatch, 1), 65535);
    for (int r0 = 0; r0 < n; r0 += cap) {
        const int R = std::min(cap, n - r0);
        if (launch_token_logprob_rows(d_logits_, V, d_lp_in_ + r0, d_lp_in_ + n + r0, R, h_out + r0, h_rank + r0, lp_scratch_, cap, stream_) != hipSuccess) {
            (void)hipStreamSynchronize(stream_);
            last_error = "token_logprobs launch failed"; return -1;
        }
    }
    if (hipStreamSynchronize(stream_) != hipSuccess || !mega_check() || !stream_check()) return -1;
    argmax_fetched_ = true;
    memcpy(logprob_out, h_out, (size_t)n * 4);
    if (rank_out) memcpy(rank_out, h_rank, (size_t)n * 4);
    return n;
}

int Context::logits_kl(Context &base, int n, const int32_t *rows_base, const int32_t *rows_self, float *kl_out, int32_t *same_top_out) {
    if (&base == this) { last_error = "logits_kl: the base and the model under test are the same context"; return -1; }
    if (last_was_embd_ || base.last_was_embd_) { last_error = "logits_kl: embeddings mode computes no logits"; return -1; }
    if (model->hp.tp_size > 1 || base.model->hp.tp_size > 1) { last_error = "logits_kl: not on a rank of a row split"; return -1; }
    if (base.model->hp.n_vocab != model->hp.n_vocab) {
        last_error = "logits_kl: n_vocab differs (base " + std::to_string(base.model->hp.n_vocab) + ", this " + std::to_string(model->hp.n_vocab) + ")"; return -1;
    }
    if (base.model->device != model->device) { last_error = "logits_kl: the two contexts are on different devices"; return -1; }
    if (n < 1 || !rows_base || !rows_self || !kl_out) { last_error = "logits_kl: bad arguments"; return -1; }
    std::vector<int32_t> rp((size_t)n), rq((size_t)n);
    if (!base.logprob_rows("logits_kl (base)", n, rows_base, rp.data())) { last_error = base.last_error; return -1; }
    if (!logprob_rows("logits_kl", n, rows_self, rq.data())) return -1;
    if (!logprob_prepare(n)) return -1;
    // the base's rows are final before this stream reads them; its step is checked like any of its own reads would
    if (hipStreamSynchronize(base.stream_) != hipSuccess || !base.mega_check() || !base.stream_check()) { last_error = base.last_error.empty() ? "logits_kl: the base context's step failed" : base.last_error; return -1; }
    int32_t *h_top = h_lp_ + 2 * (size_t)lp_cap_ + n;
    float *h_out = reinterpret_cast<float *>(h_lp_ + 2 * (size_t)lp_cap_);
    memcpy(h_lp_, rp.data(), (size_t)n * 4);
    memcpy(h_lp_ + n, rq.data(), (size_t)n * 4);
    if (hipMemcpyAsync(d_lp_in_, h_lp_, (size_t)n * 2 * 4, hipMemcpyHostToDevice, stream_) != hipSuccess) { last_error = "logits_kl staging failed"; return -1; }
    const int cap = (int)std::min<uint32_t>(std::max<uint32_t>(cp.n_ubatch, 1), 65535);
    float *scratch = lp_scratch_ + token_logprob_scratch_words(cap);
    for (int r0 = 0; r0 < n; r0 += cap) {
        const int R = std::min(cap, n - r0);
        if (launch_logits_kl_rows(base.d_logits_, d_logits_, model->hp.n_vocab, d_lp_in_ + r0, d_lp_in_ + n + r0, R, h_out + r0, h_top + r0, scratch, cap, stream_) != hipSuccess) {
            (void)hipStreamSynchronize(stream_);
            last_error = "logits_kl launch failed"; return -1;
        }
    }
    if (hipStreamSynchronize(stream_) != hipSuccess || !mega_check() || !stream_check()) return -1;
    argmax_fetched_ = true;
    memcpy(kl_out, h_out, (size_t)n * 4);
    if (same_top_out) memcpy(same_top_out, h_top, (size_t)n * 4);
    return n;
}

int Context::perplexity(const int32_t *tokens, int64_t n_tokens, int n_chunk, int32_t bos, int seq, Context *base, float *logprob_out, float *kl_out,
                        int (*cb)(const PplStats &, void *), void *user, PplStats &st) {
    st = PplStats();
    st.has_base = base ? 1 : 0;
    if (!tokens || n_tokens < 0) { last_error = "perplexity: bad arguments"; return -1; }
    if (seq < 0 || seq >= 64) { last_error = "perplexity: seq id " + std::to_string(seq) + " out of range [0, 64)"; return -1; }
    if (n_chunk < 2 || (uint32_t)n_chunk > cp.n_ctx || (base && (uint32_t)n_chunk > base->cp.n_ctx)) {
        last_error = "perplexity: n_chunk " + std::to_string(n_chunk) + " outside [2, n_ctx " + std::to_string(base ? std::min(cp.n_ctx, base->cp.n_ctx) : cp.n_ctx) + "]"; return -1;
    }
    if (base == this) { last_error = "perplexity: the base and the model under test are the same context"; return -1; }
    if (base && base->model->hp.n_vocab != model->hp.n_vocab) { last_error = "perplexity: n_vocab differs between the base and the model under test"; return -1; }
    if (base && base->model->device != model->device) { last_error = "perplexity: the two contexts are on different devices"; return -1; }
    if (bos >= model->hp.n_vocab) { last_error = "perplexity: bos outside the vocabulary"; return -1; }
    const int64_t n_chunks = n_tokens / n_chunk;
    const int first = n_chunk / 2, per = n_chunk - 1 - first;          // scored positions first .. n_chunk - 2
    const int piece_max = (int)std::min(cp.n_ubatch, base ? base->cp.n_ubatch : cp.n_ubatch);
    std::vector<int32_t> tk((size_t)n_chunk), pos((size_t)piece_max), nseq((size_t)piece_max, 1), rows, tgt;
    std::vector<int8_t> flags((size_t)piece_max);
    std::vector<int32_t *> seqs((size_t)piece_max);
    std::vector<float> lp, lpb, kl;
    std::vector<int32_t> rank, top;
    int32_t sid = seq;
    for (auto &p : seqs) p = &sid;
    int rc = 0;
    for (int64_t c = 0; c < n_chunks && rc == 0; c++) {
        kv_seq_rm(seq, 0, -1);
        if (base) base->kv_seq_rm(seq, 0, -1);
        memcpy(tk.data(), tokens + c * n_chunk, (size_t)n_chunk * 4);
        if (bos >= 0) tk[0] = bos;
        int64_t at = c * per;
        PplStats cur = st;                                             // a chunk enters the stats whole or not at all
        for (int i0 = 0; i0 < n_chunk && rc == 0; i0 += piece_max) {
            const int n = std::min(piece_max, n_chunk - i0);
            rows.clear(); tgt.clear();
            for (int i = 0; i < n; i++) {
                const int p = i0 + i;
                pos[(size_t)i] = p;
                flags[(size_t)i] = p >= first && p <= n_chunk - 2;
                if (flags[(size_t)i]) { rows.push_back(i); tgt.push_back(tk[(size_t)p + 1]); }
            }
            const int d = decode(n, tk.data() + i0, pos.data(), nseq.data(), seqs.data(), flags.data());
            if (d != 0) { if (d > 0) last_error = "perplexity: no KV slot for the chunk"; rc = -1; break; }
            if (base) {
                const int db = base->decode(n, tk.data() + i0, pos.data(), nseq.data(), seqs.data(), flags.data());
                if (db != 0) { last_error = db > 0 ? "perplexity: no KV slot for the chunk in the base context" : base->last_error; rc = -1; break; }
            }
            const int R = (int)rows.size();
            if (R == 0) continue;
            lp.resize((size_t)R); rank.resize((size_t)R);
            if (token_logprobs(R, rows.data(), tgt.data(), lp.data(), rank.data()) < 0) { rc = -1; break; }
            if (base) {
                lpb.resize((size_t)R); kl.resize((size_t)R); top.resize((size_t)R);
                if (base->token_logprobs(R, rows.data(), tgt.data(), lpb.data(), nullptr) < 0) { last_error = base->last_error; rc = -1; break; }
                if (logits_kl(*base, R, rows.data(), rows.data(), kl.data(), top.data()) < 0) { rc = -1; break; }
            }
            for (int r = 0; r < R; r++, at++) {
                const bool dead = lp[(size_t)r] != lp[(size_t)r] || (base && (lpb[(size_t)r] != lpb[(size_t)r] || kl[(size_t)r] != kl[(size_t)r]));
                if (logprob_out) logprob_out[at] = dead ? NAN : lp[(size_t)r];
                if (kl_out) kl_out[at] = dead || !base ? NAN : kl[(size_t)r];
                if (dead) { cur.dead++; continue; }
                const double nll = -(double)lp[(size_t)r];
                cur.count++; cur.nll += nll; cur.nll2 += nll * nll;
                cur.top1 += rank[(size_t)r] == 0 ? 1 : 0;
                if (base) {
                    const double nb = -(double)lpb[(size_t)r], k = (double)kl[(size_t)r];
                    cur.nll_base += nb; cur.nll2_base += nb * nb; cur.kl += k; cur.kl2 += k * k;
                    cur.same_top += top[(size_t)r] == 1 ? 1 : 0;
                }
            }
        }
        if (rc != 0) break;
        st = cur;
        st.n_chunks = c + 1;
        if (cb && cb(st, user) != 0) { st.stopped = 1; break; }
    }
    kv_seq_rm(seq, 0, -1);
    if (base) base->kv_seq_rm(seq, 0, -1);
    return rc;
}

// n rows of the last batch in ONE set of launches and ONE synchronisation (a scheduler tick asks for all its sampling slots together: row by row, each
// with its own launch + sync, 32 slots cost more than copying 32 rows to the host did).  toks / logits: [n][TOPK_MAX_K]; ks[r] of each row are valid.
int Context::topk_rows(int n, const int *is, const int *ks, const TopkAdj *adjs, int32_t *toks, float *logits) {
    if (last_was_embd_ || n < 1) return -1;
    const int V = model->hp.n_vocab;
    int kmax = 0;
    std::vector<int> rows((size_t)n);
    for (int r = 0; r < n; r++) {
        int i = is[r];
        if (i < 0) i += (int)out_row_of_batch_.size();
        if (i < 0 || i >= (int)out_row_of_batch_.size() || out_row_of_batch_[(size_t)i] < 0) return -1;
        if (ks[r] < 1 || ks[r] > TOPK_MAX_K || ks[r] > V || adjs[r].n < 0 || adjs[r].n > TOPK_MAX_ADJ) return -1;
        rows[(size_t)r] = out_row_of_batch_[(size_t)i];
        kmax = std::max(kmax, ks[r]);
    }
    if (hipSetDevice(model->device) != hipSuccess) return -1;
    if (n > topk_rows_cap_) {
        (void)hipStreamSynchronize(stream_);
        if (topk_scratch_) (void)hipFree(topk_scratch_);
        if (d_topk_adj_) (void)hipFree(d_topk_adj_);
        if (h_topk_) (void)hipHostFree(h_topk_);
        if (h_topk_adj_) (void)hipHostFree(h_topk_adj_);
        topk_scratch_ = nullptr; d_topk_adj_ = nullptr; h_topk_ = nullptr; h_topk_adj_ = nullptr; topk_rows_cap_ = 0;
        const int cap = std::max(n, std::min(64, (int)cp.n_seq_max));
        const size_t adj_bytes = (size_t)cap * sizeof(TopkAdj) + (size_t)cap * sizeof(int);
        if (hipMalloc(&topk_scratch_, topk_scratch_bytes(V) * (size_t)cap) != hipSuccess || hipMalloc((void **)&d_topk_adj_, adj_bytes) != hipSuccess ||
            hipHostMalloc((void **)&h_topk_, (size_t)cap * TOPK_MAX_K * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc((void **)&h_topk_adj_, adj_bytes, hipHostMallocDefault) != hipSuccess) { last_error = "top-k workspace allocation failed"; return -1; }
        topk_rows_cap_ = cap;
    }
    // adjustments and row numbers: one staged copy
    TopkAdj *ha = reinterpret_cast<TopkAdj *>(h_topk_adj_);
    int *hr = reinterpret_cast<int *>(h_topk_adj_ + (size_t)topk_rows_cap_ * sizeof(TopkAdj));
    for (int r = 0; r < n; r++) {
        TopkAdj &d = ha[r];
        const TopkAdj &a = adjs[r];
        d.n = a.n; d.repeat = a.repeat; d.freq = a.freq; d.present = a.present;
        memcpy(d.tok, a.tok, (size_t)a.n * sizeof(int)); memcpy(d.bias, a.bias, (size_t)a.n * sizeof(float)); memcpy(d.cnt, a.cnt, (size_t)a.n * sizeof(int));
        hr[r] = rows[(size_t)r];
    }
    const size_t rows_off = (size_t)topk_rows_cap_ * sizeof(TopkAdj);
    if (hipMemcpyAsync(d_topk_adj_, h_topk_adj_, (size_t)n * sizeof(TopkAdj), hipMemcpyHostToDevice, stream_) != hipSuccess ||
        hipMemcpyAsync(d_topk_adj_ + rows_off, h_topk_adj_ + rows_off, (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream_) != hipSuccess) { last_error = "top-k staging failed"; return -1; }
    if (launch_topk_rows(d_logits_, V, n, reinterpret_cast<const int *>(d_topk_adj_ + rows_off), kmax, reinterpret_cast<const TopkAdj *>(d_topk_adj_), topk_scratch_, h_topk_,
                         stream_) != hipSuccess) { last_error = "top-k launch failed"; return -1; }
    if (hipStreamSynchronize(stream_) != hipSuccess || !mega_check() || !stream_check()) return -1;
    for (int r = 0; r < n; r++)
        for (int j = 0; j < ks[r]; j++) {
            const unsigned long long key = h_topk_[(size_t)r * TOPK_MAX_K + (size_t)j];
            unsigned u = (unsigned)(key >> 32);
            u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;        // inverse of the order-preserving image
            float f;
            memcpy(&f, &u, 4);
            toks[(size_t)r * TOPK_MAX_K + (size_t)j] = (int32_t)(0xffffffffu - (unsigned)(key & 0xffffffffull));
            logits[(size_t)r * TOPK_MAX_K + (size_t)j] = f;
        }
    return n;
}

int Context::topk_ith(int i, int k, const TopkAdj &adj, int32_t *toks, float *logits) {
    int32_t t[TOPK_MAX_K];
    float l[TOPK_MAX_K];
    if (topk_rows(1, &i, &k, &adj, t, l) != 1) return -1;
    memcpy(toks, t, (size_t)k * sizeof(int32_t));
    memcpy(logits, l, (size_t)k * sizeof(float));
    return k;
}

int Context::debug_layer_out(int il, float *dst, size_t cap) {
    const HParams &hp = model->hp;
    if (!dbg_ || il < 0 || il >= hp.n_layer) return -1;
    const size_t n = (size_t)dbg_tokens_ * hp.n_embd;
    if (cap < n) return -1;
    (void)hipStreamSynchronize(stream_);
    if (hipMemcpy(dst, dbg_ + (size_t)il * cp.n_ubatch * hp.n_embd, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return dbg_tokens_;
}

// every weight tensor once, as one decoded token reads them (no attention): the dominant kernel class, issued by the functions run_layers issues it with
// launches_out: mat-vec launches per sweep.  Where the step runs attn_output (and Q | K | V) inside its attention launch (attn_out.hip) the sweep holds no
// such launch either: it times the launches of the dominant kernel class as the step issues them, and counts their bytes only.
double Context::bench_weight_sweep(int iters, uint64_t *bytes_out, int *launches_out) {
    const HParams &hp = model->hp;
    const int E = hp.n_embd;
    if (hp.encoder) return -1.0;                               // (the encoder graph has no single-token step)
    (void)hipMemsetAsync(x_, 0, (size_t)E * 4, stream_);
    uint64_t bytes = 0; int launches = 0;
    // a single-token step over 64 cells of one sequence, outside the engine; the results go to xo_ so that the layer input stays as it is, and nothing is
    // exchanged between the ranks of a row split
    // (the residual choice stays the step's own: plan_attn is asked the step's question on every rank.  Of the prep state only prep_owner_ is dropped)
    Step st = step_constants(1, 64);
    st.chunk_lists = false;
    st.out = xo_;
    struct ProfileOff { bool &p; bool was; ~ProfileOff() { p = was; } } profile_off{profile_, profile_};   // the step's functions mark profile events:
    profile_ = false;                                                                                      // none inside the sweep's capture
    auto sweep = [&](bool count) -> hipError_t {
        for (int il = 0; il < hp.n_layer; il++) {
            const LayerWeights &L = model->layers[(size_t)il];
            const AttnPlan ap = plan_attn(il, st);
            HIP_TRY(attn_qkv(il, st, ap));
            HIP_TRY(attn_output(il, st, ap));
            if (count) {
                bytes += (ap.qkv_in_attn ? 0 : L.wq.ggml_bytes + L.wk.ggml_bytes + L.wv.ggml_bytes) + (ap.ao_form ? 0 : L.wo.ggml_bytes);
                launches += (ap.qkv_in_attn ? 0 : 1) + (ap.ao_form ? 0 : 1);
            }
            if (hp.n_expert > 0) {
                // mixture of experts: the token's n_expert_used experts (indices 0..k-1 stand in for a selection; every expert has the same shape and bytes)
                const int KU = hp.n_expert_used;
                MMVQArgs a{}, d{};
                if (!moe_ids_ || !moe_selected_desc(il, a, d)) continue;
                if (count) { std::vector<int32_t> ids((size_t)KU); for (int j = 0; j < KU; j++) ids[(size_t)j] = j; HIP_TRY(hipMemcpy(moe_ids_, ids.data(), ids.size() * 4, hipMemcpyHostToDevice)); }
                HIP_TRY(launch_mmvq(a, stream_));
                HIP_TRY(launch_mmvq(d, stream_));
                if (count) {
                    bytes += (L.gate_exps.ggml_bytes + L.up_exps.ggml_bytes + L.down_exps.ggml_bytes) / (uint64_t)L.gate_exps.n_expert * (uint64_t)KU;
                    launches += 2;
                }
                continue;
            }
            bool quantised = false;
            int n_down = 0;
            HIP_TRY(ffn_dense_gate_up(il, st, quantised));
            HIP_TRY(ffn_down(il, st, quantised, &n_down));
            if (count) {
                bytes += L.gate.ggml_bytes + L.up.ggml_bytes + L.down.ggml_bytes;
                launches += 1 + n_down;
            }
        }
        if (type_is_quant(model->output.type) && can_fuse(E, 1)) { pending_fuse_.mode = 1; pending_fuse_.x = x_; pending_fuse_.w = (const float *)model->out_norm.data; pending_fuse_.eps = hp.eps; }
        HIP_TRY(linear(model->output, aq_e_, xn_, E, 1, d_logits_, (int)model->output.N, nullptr, EPI_STORE));
        pending_fuse_ = Fuse();
        if (count) { bytes += model->output.ggml_bytes; launches += 1; }
        return hipSuccess;
    };
    if (!d_logits_) { d_logits_ = (float *)dalloc((size_t)hp.n_vocab * 4); logits_cap_rows_ = 0; }
    if (sweep(true) != hipSuccess) return -1.0;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipStreamSynchronize(stream_);
    // replayed from a hipGraph, as the decode step is (eager launches are host-bound at these kernel lengths)
    hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr;
    bool graphed = cp.use_graphs && hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (graphed) {
        const hipError_t es = sweep(false);
        const hipError_t ec = hipStreamEndCapture(stream_, &g);
        graphed = es == hipSuccess && ec == hipSuccess && g && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess;
        if (graphed) { (void)hipGraphLaunch(ge, stream_); (void)hipStreamSynchronize(stream_); }
    }
    (void)hipEventRecord(e0, stream_);
    for (int i = 0; i < iters; i++) {
        if (graphed) { if (hipGraphLaunch(ge, stream_) != hipSuccess) return -1.0; }
        else if (sweep(false) != hipSuccess) return -1.0;
    }
    (void)hipEventRecord(e1, stream_);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (ge) (void)hipGraphExecDestroy(ge);
    if (g) (void)hipGraphDestroy(g);
    if (bytes_out) *bytes_out = bytes;
    if (launches_out) *launches_out = launches;
    return (double)ms * 1000.0 / iters;
}

}  // namespace mi355
