// runtime.h — model residency and the decode executor (host C++ above the HIP kernels).
//
// Plays the role of the llama.cpp objects the reference holds through common_init_result
// (src/llama_server_context.cc:207-209): llama_model (weights on device), llama_context (KV cache,
// batch execution, logits), llama_kv_cache (cells with positions and sequence sets).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../csrc/kernels.h"
#include "gguf.h"
#include "lora.h"
#include "model_plan.h"

namespace mi355 {

// the model as its file describes it (ModelLayout: hyper-parameters and tensors, model_plan.h) plus what holding it on a device adds
struct LoraAdapter;
struct Model : ModelLayout {
    std::unique_ptr<GGUFFile> file;
    std::vector<LoraAdapter *> adapters;   // loaded onto this model (lora_load); their device bytes are part of device_bytes; freed with the model at the latest
    std::string path, desc;
    int device = 0;
    std::vector<uint8_t *> arenas;      // hipMalloc'd blocks
    uint64_t device_bytes = 0, host_bytes = 0, file_tensor_bytes = 0, bytes_per_token = 0, planes_bytes = 0;
    ~Model();
};

// The file is validated and the arena laid out by plan_model (model_plan.h) before the device is touched: a malformed file fails the same way with and
// without a GPU.  What follows uploads the plan (repacking rows on the way), sets up the encoder's views and the tied output, and expands the prefill planes.
// prefill_planes: 0 = never, 1 = always (fails when memory is short), -1 = when device memory allows (default)
// tp_size > 1: load rank tp_rank's slice of every projection (rows of attn_q/k/v, ffn_gate/up and output; the matching
// super-block columns of attn_output and ffn_down), cut on head and 256-element boundaries
Model *model_load(const std::string &path, int main_gpu, std::string &err, int &status, int prefill_planes = -1, int tp_rank = 0, int tp_size = 1);

// A LoRA adapter file loaded onto a model (llama_adapter_lora_init): every pair checked by plan_lora (lora.h) and copied to the device in the file's type,
// lora_a as r rows of K, lora_b as N rows of r.  The model owns it; a context holds the active set and the scales (Context::set_adapter_lora).
struct LoraPair { int layer, target, type, r; int64_t K, N; const uint8_t *A, *B; };
struct LoraAdapter {
    Model *model = nullptr;
    std::string path;
    float alpha = 0.0f;
    std::vector<LoraPair> pairs;
    std::vector<int> index;                // [(layer + 1) * LORA_N_TARGETS + target] -> pair or -1 (layer -1: output.weight)
    uint8_t *arena = nullptr;
    uint64_t device_bytes = 0;
    const LoraPair *find(int layer, int target) const {
        const size_t i = (size_t)(layer + 1) * LORA_N_TARGETS + (size_t)target;
        return i < index.size() && index[i] >= 0 ? &pairs[(size_t)index[i]] : nullptr;
    }
};
LoraAdapter *lora_load(Model *m, const std::string &path, std::string &err, int &status);
void lora_free(LoraAdapter *a);            // (no context may still have it set)

struct KVCell {
    int32_t pos = -1;
    int32_t delta = 0;
    uint64_t seqs = 0;
};

void debug_raise_stream_error(unsigned code);        // tests: raise the sticky error word of the cross-workgroup kernels as a timed-out wait would
struct ContextParams {
    uint32_t n_ctx = 512, n_batch = 2048, n_ubatch = 512, n_seq_max = 1;
    int type_k = T_F16, type_v = T_F16;
    bool flash_attn = true, embeddings = false, use_graphs = true;
    bool logits_to_host = true;   // llama_decode contract: flagged logits rows are copied to host memory by the decode itself
};

struct ProfileEntry { std::string name; float us; };

struct Fuse {   // fused activation prologue of the single-token mat-vec (mmvq.hip stage_act)
    int mode = 0;
    const float *x = nullptr, *w = nullptr;
    float eps = 0.0f;
    float *out_host = nullptr;   // the launch also stores its results here (pinned host memory; the output head of a single-token step) - weight stream only
};

// The mat-vec launches as a step issues them, shared with the per-op test entry (csrc/op_entries_matmul.cc mi355_op_mat_vec_step) so that model and test run one piece of code:
// a weight tensor as a launch segment; a single-token launch's description without its segments; T tokens as launches of 16 / 8 / 4 / 2 / 1.
// trace (nullable): one record per launch issued - its token count and the kernel launch_mmvq takes for it (kernels.h mmvq_kernel_choice / mmvq_stream_form).
struct MMVQTrace {
    struct Rec { int T, kernel; MMVQStreamForm form; };
    std::vector<Rec> recs;
    void note(const MMVQArgs &a);
};
MMVQSeg make_seg(const DevTensor &w, float *out, int ld_out, const float *resid, const int32_t *esel);
MMVQArgs single_token_desc(int n_seg, int K, int epi, int fuse, const float *nx, const float *nw, float eps, const ActQuant &aq);
hipError_t mmvq_tokens(MMVQSeg *segs, int n_seg, int K, int T, int epi, const ActQuant &aq, hipStream_t st, const Fuse &fz = Fuse(), MMVQTrace *trace = nullptr);
// Which MFMA launch the K-quant (and planes-only) tensors of a prompt batch or a batched decode step take: the order of predicates that Context::linear
// (PM_ROLE_ONE), Context::linear_multi (PM_ROLE_MULTI) and the dense gate | up block (PM_ROLE_GATE_UP, ws = {gate, up}) test, stated once and shared with the
// per-op test entry (csrc/op_entries_matmul.cc mi355_op_prompt_mul_mat).  PM_NONE: none of them - the caller goes on to its other paths.
enum { PM_NONE = 0, PM_KSPLIT = 1, PM_PLANES = 2, PM_FLY = 3 };
enum { PM_ROLE_ONE = 0, PM_ROLE_MULTI = 1, PM_ROLE_GATE_UP = 2 };
struct PromptMatmul {
    int form = PM_NONE;        // PM_ROLE_MULTI + PM_PLANES: of the fused launch; every other tensor takes its plane set, or the expansion on the fly without one
    int n_fused = 0;           // tensors in the launch (PM_ROLE_MULTI + PM_PLANES: 0 where no two plane sets are adjacent - every tensor on its own)
    bool swiglu = false;       // SwiGLU in the launch's epilogue
    bool planes_only = false;  // a planes-only type (Q2_K, Q3_K, IQ4_XS, ternary): the launch wants Q8_K rows
    bool need_prep = false;    // the launch reads the bh / bl block-sum planes (launch_mmq_prep, or a producer that wrote them)
};
PromptMatmul prompt_mul_mat_choice(int role, const DevTensor *const *ws, int n, int K, int T, MMQWorkspace wsp);
// the process's sticky error word installed in the device globals of the current device (what Context::init does); nullptr where it could not be allocated
unsigned *install_stream_error_word();

void set_moe_q80_grouped(bool on);  // tests / tools: MXFP4 expert tensors, prompt batches: one launch for all experts (default) or one per expert - the same bits
void set_moe_group_min(int tokens);   // tests: batch size from which a mixture-of-experts feed-forward is grouped by expert
void set_attn_store_fuse(bool on);   // tests: 0 = batched steps store K / V in their own launch before the attention
void set_rope_fast(bool on);         // tests: 0 = prompt batches rotate q / store K, V with the one-workgroup-per-token kernel
void set_decode_engine(int on);  // 1 / 0: the layer engine (decode_engine.hip) for single-token steps of contexts created afterwards; -1: environment MI355_ENGINE / default (off)
void set_decode_mega(bool on);   // tests: compare the whole-step kernel with the per-launch path (read when a context first decodes one token)

class Context {
  public:
    int64_t engine_steps = 0;          // single-token steps issued through the layer engine (graph replays included)
    int64_t qkv_attn_launches = 0;     // launches that ran a layer's Q | K | V inside its attention + attn_output launch (attn_out.hip QF)
    int64_t fused_skipped_steps = 0;   // single-token steps that took the wait-free launches because another context of the device held the cross-workgroup-wait kernel
    int64_t mega_steps = 0;            // single-token steps issued as one whole-step launch (graph replays included)
    Context(Model *m, const ContextParams &p);
    ~Context();
    bool init(std::string &err);

    // llama_decode semantics: 0 ok, 1 no KV slot, <0 error
    // embd != nullptr: rows of n_embd floats in place of token ids (llama_batch.embd; tokens must then be nullptr)
    int decode(int n_tokens, const int32_t *tokens, const int32_t *pos, const int32_t *n_seq_id, int32_t *const *seq_id,
               const int8_t *logits_flags, const float *embd = nullptr);
    float *logits_ith(int i);
    // llama_get_embeddings_ith: the final-norm hidden state of batch row i (n_embd floats, host memory); rows are
    // produced for the flagged tokens of the last decode while embeddings_enabled is set (then no logits are computed)
    float *embeddings_ith(int i);
    int32_t argmax_ith(int i);
    // speculative decoding (csrc/spec.hip), both from the device logits of the last decode, whatever logits_to_host says:
    // the arg-max of batch row i and its softmax probability over the whole vocabulary (argmax_ith's preconditions; -1 with last_error set)
    int32_t argmax_prob_ith(int i, float *p);
    // greedy acceptance: group g owns batch rows group_start[g] .. group_start[g + 1] - 1 of the last decode (k_g drafted tokens -> k_g + 1 rows, every one
    // flagged); draft [R] runs parallel to those R rows (a group's last entry is ignored).  ids_out [R]: each row's arg-max; n_accept_out [n_groups]: the drafts
    // the model agrees with, from the group's first row on.  One launch, one synchronisation.  Returns R, or -1 with last_error set (a row not flagged,
    // embeddings mode, a rank of a row split).
    int spec_verify(int n_groups, const int32_t *group_start, const int32_t *draft, int32_t *ids_out, int32_t *n_accept_out);
    // perplexity and KL divergence (csrc/logprob.hip), from the device logits of the last decode like the two above; a few words per row come
    // back through pinned memory, one synchronisation per call, the rows stay where logits_ith finds them.  Each returns n, or -1 with last_error set
    // (embeddings mode, a batch row that was not flagged, a target outside the vocabulary, a rank of a row split; logits_kl also: another n_vocab, another
    // device, the same context on both sides).
    // logprob_out[r] = log softmax(row batch_rows[r])[targets[r]] over the whole vocabulary; rank_out[r] (nullable) = the entries that beat the target
    // (0: it is the arg-max).  A dead row (kernels.h) gives NaN and -1.
    int token_logprobs(int n, const int32_t *batch_rows, const int32_t *targets, float *logprob_out, int32_t *rank_out);
    // kl_out[r] = KL(P || Q), P = row rows_base[r] of `base`'s last decode, Q = row rows_self[r] of this context's; same_top_out[r] (nullable) = 1 where both
    // have the same arg-max.  A row with a non-finite entry: NaN and -1.  base's stream is drained on the host before the launch on this one's.
    int logits_kl(Context &base, int n, const int32_t *rows_base, const int32_t *rows_self, float *kl_out, int32_t *same_top_out);
    // The llama-perplexity procedure (restated from memory of llama.cpp's perplexity(): unpinned).  n_chunks = n_tokens / n_chunk, the tail is
    // dropped.  Per chunk: `seq` is cleared, the first token becomes bos (if bos >= 0), the chunk is decoded at positions 0 .. n_chunk - 1 in pieces of at most
    // n_ubatch tokens with positions n_chunk / 2 .. n_chunk - 2 flagged, and after each piece the flagged rows are scored against the tokens that follow them.
    // With a base context the same pieces run there too and every scored row also gives the base's log-probability and KL(base || this).  Sums in double; a row
    // any of whose figures is NaN is counted in `dead` and in nothing else.  logprob_out / kl_out (nullable): n_chunks * (n_chunk - 1 - n_chunk / 2) entries in
    // scoring order, NaN for dead rows.  cb (nullable) sees the running stats after every chunk; non-zero stops the run (stats.stopped = 1).  `seq` is removed
    // from both caches on return.  0, or -1 with last_error set; the stats then cover the chunks that were scored whole.
    struct PplStats {
        int64_t n_chunks = 0, count = 0, top1 = 0, dead = 0, same_top = 0;
        int32_t has_base = 0, stopped = 0;
        double nll = 0, nll2 = 0, nll_base = 0, nll2_base = 0, kl = 0, kl2 = 0;
    };
    int perplexity(const int32_t *tokens, int64_t n_tokens, int n_chunk, int32_t bos, int seq, Context *base, float *logprob_out, float *kl_out,
                   int (*cb)(const PplStats &, void *), void *user, PplStats &out);
    // importance matrix (csrc/imatrix.hip; what llama-imatrix records).  Between begin and end every micro-batch of every decode adds, for
    // every weight matrix it multiplies, the per-input-column sum of squares of the f32 rows the projection consumes and the number of rows - per expert for
    // the expert tensors.  While it is on the layer blocks take the routes that leave those rows in memory (the ones an adapter on every target forces; a
    // mixture-of-experts feed-forward is grouped at every batch size), and the single-launch step, the layer engine and the captured graphs are not used;
    // after end the steps are what they were.  Entries carry GGUF tensor names; tensors that share an input (attn_q / attn_k / attn_v, ffn_gate / ffn_up)
    // share an accumulator and report the same values.  process_output: also the output head, from the final-norm rows of the flagged tokens.
    // begin: 0, or -1 with last_error set (already on, an encoder, a rank of a row split, a width that is no multiple of 32, a mixture-of-experts context
    // without grouped buffers or with float expert tensors, out of device memory).  The accumulators, counts and slab scratch are device memory of the
    // context (device_bytes) from begin to end.
    int imatrix_begin(bool process_output);
    int imatrix_end();
    int imatrix_clear();                       // zeroes sums and counts, keeps collecting
    bool imatrix_on() const { return imx_on_; }
    int imatrix_n_entries() const { return (int)imx_names_.size(); }
    // entry i: its tensor name, row length ne0 and number of matrices (1, or n_expert); false for an index outside the list
    bool imatrix_entry(int i, std::string &name, int &ne0, int &n_mat) const;
    // sum2 [n_mat][ne0], counts [n_mat] of entry i: one synchronisation, then the copies.  0, or -1 with last_error set (a non-finite sum names the tensor)
    int imatrix_get(int i, float *sum2, int32_t *counts);
    // test hook (mixture-of-experts files): the NEXT decode call (one micro-batch of T tokens) takes these experts, ids [n_layer][T][n_expert_used], instead of
    // its router's selection; the weights stay this side's probabilities of them.  One call, then routing is free again.  No graphs while it is armed.
    int force_moe_ids(const int32_t *ids, int n_layer, int T, int k);
    // device-side sampling front end: the k best (token, logit) candidates of batch row i after the adjustments (kernels.h launch_topk_rows), best
    // first; returns the count written (k) or < 0
    int topk_ith(int i, int k, const TopkAdj &adj, int32_t *toks, float *logits);
    int topk_rows(int n, const int *is, const int *ks, const TopkAdj *adjs, int32_t *toks, float *logits);   // n rows at once; outputs [n][TOPK_MAX_K]
    void synchronize();

    // llama_set_adapter_lora / llama_rm_adapter_lora / llama_clear_adapter_lora: the adapters this context's steps apply, in the order they were first set
    // (setting one again changes its scale).  Every change drains the stream and drops the captured steps.  0, or -1 with last_error set.
    int set_adapter_lora(LoraAdapter *a, float scale);
    int rm_adapter_lora(LoraAdapter *a);
    void clear_adapter_lora();
    // llama_apply_adapter_cvec: data holds the vectors of layers 1, 2, ... back to back, layer il at n_embd * (il - 1) and present when
    // n_embd * il <= len.  From the next step on every layer il with il_start <= il <= il_end whose vector is present ends with x[t][:] += v_il[:] on all rows
    // of the batch (csrc/cvec.hip launch_add_row_vec, a launch of its own before the tap); layer 0 never has one.  While a vector is applied the single-launch
    // step and the layer engine are not used; graphs are.  data == nullptr clears: the steps are again what they were.  Both drain the stream and drop the
    // captured steps.  0, or -1 with last_error set and nothing changed (an encoder, a rank of a row split, another n_embd, len no multiple of n_embd, a
    // non-finite value, il_start > il_end, out of device memory).  The [n_layer][n_embd] f32 buffer is device memory of the context from the first apply on.
    int apply_cvec(const float *data, size_t len, int n_embd, int il_start, int il_end);
    bool cvec_applied() const { return cvec_on_; }

    void kv_clear();
    bool kv_seq_rm(int seq, int p0, int p1);
    void kv_seq_cp(int src, int dst, int p0, int p1);
    void kv_seq_add(int seq, int p0, int p1, int delta);
    int kv_used_cells() const;

    // llama_state_seq_get_size / get_data / set_data: the cells of one sequence as a blob another context of the same geometry and cache types can take.
    //   header: 8 little-endian 32-bit words - magic "M5KV", version, type_k, type_v, n_layer, n_head_kv, head_dim, n (cells)
    //   n int32 positions, ascending; then per layer K rows [n][n_head_kv * head_dim] and V rows likewise, ggml layout of the cache type (kernels.h, kv_state.hip)
    // size = 32 + 4 n + n_layer * n * (row_bytes_k + row_bytes_v), from the host's cell table alone.  get applies a pending K-shift first, so K is rotated for the
    // positions the blob records; it returns the bytes written, 0 with last_error set when refused (cap too small, an encoder, a rank of a row split).
    // set removes everything `seq` holds, allocates n cells for it (alloc_cells: the region's lowest free cells, in position order), scatters the rows and marks
    // the cell table dirty; it returns the bytes consumed, or 0 with last_error naming the field and both values - the sequence is then left empty.
    static constexpr uint32_t STATE_MAGIC = 0x564b354du, STATE_VERSION = 1, STATE_HEADER_BYTES = 32;
    size_t state_seq_size(int seq) const;
    size_t state_seq_get(int seq, uint8_t *dst, size_t cap);
    size_t state_seq_set(int seq, const uint8_t *src, size_t len);
    // measurement (profiles/): the pack launch, the copy to the host and the unpack launch of the last get / set, each from its own pair of events (ms)
    float state_ms_pack = 0, state_ms_copy = 0, state_ms_unpack = 0;
    bool state_timing = false;

    int debug_layer_out(int il, float *dst, size_t cap);
    void set_debug_taps(bool on) { debug_taps_ = on; }
    void set_profile(bool on) { profile_ = on; }
    const std::vector<ProfileEntry> &last_profile() const { return last_profile_; }
    double bench_weight_sweep(int iters, uint64_t *bytes, int *launches = nullptr);

    Model *model;
    ContextParams cp;
    uint64_t device_bytes = 0;
    std::string last_error;
    bool embeddings_enabled = false;

  private:
    struct Bufs;
    const float *ub_embd_ = nullptr;   // host rows of the micro-batch being decoded when the batch carries embeddings
    int decode_ubatch(int n, const int32_t *tokens, const int32_t *pos, const int32_t *seq, const uint64_t *seqmask,
                      const int8_t *flags, int out_base);
    int find_slot(int n);
    // one cell per token; with n_seq_max > 1 every sequence allocates from its own region of the cache
    // (n_ctx / n_seq_max cells, the reference's per-slot context), so a sequence's cells stay together
    bool alloc_cells(int n, const uint64_t *seqmask, std::vector<int> &out);
    std::vector<int> region_next_;     // per sequence: where its next cell is looked for first
    void apply_k_shift();
    // state_seq_get / set: a bounded device staging block (at most 64 MiB of portable rows, the cells of a sequence go through it in chunks), the cell list and
    // the per-layer plane table the two kernels read; allocated on first use, freed with the context
    uint8_t *d_state_stage_ = nullptr;
    size_t state_stage_bytes_ = 0;
    int32_t *d_state_cells_ = nullptr;
    KVLayerView *d_state_layers_ = nullptr;
    bool state_prepare();
    const char *state_refusal() const;
    size_t state_cell_bytes() const;      // portable bytes of one cell over all layers
    // ---- the layer forward pass: run_layers is the loop (set-up, the whole-step early return, then per layer attention block -> attn_output -> feed-forward
    // block -> tap); each block states its choice of launch form once, and bench_weight_sweep issues a step's mat-vecs through the same functions
    struct Step {                      // what one run_layers call fixes for all its layers (step_constants)
        int T = 0, n_kv_max = 0;
        RopeArgs ra_step{};            // the model's rope (a layer's own: layer_rope)
        bool engine = false;           // the layer engine runs everything between two attention launches
        bool tp = false;               // row split: partial sums are exchanged after attn_output and ffn_down
        bool chunk_lists = false;      // the attention walks per-token chunk lists (decode_ubatch)
        int attn_mode = 2;             // MI355_ATTN_MODE
        bool rope_fast = true, fuse_down_env = true;   // MI355_ROPE_FAST (and set_rope_fast), MI355_FUSE_DOWN
        float *out = nullptr;          // where attn_output and ffn_down leave their rows: x_ (in place), tp_part_ under a row split
        const float *resid = nullptr;  // ... and the residual they add: x_, or none on the ranks after the first
    };
    struct AttnPlan {                  // the launches of one layer's attention block (plan_attn: launches nothing)
        RopeArgs ra;                   // the layer's rope
        AttnArgs aa, af;               // the attention launch; the attention + attn_output launch (its own split count)
        MMVQSeg ao_seg;                // attn_output as a segment of that launch
        int ao_epi;
        QKVFuse qf;                    // Q | K | V inside it
        bool qkv_float, qkv_prologue;  // a float projection (takes xn_); RMSNorm -> Q8_K in the Q | K | V launch's prologue
        bool o_planes;                 // the attention writes the block-sum planes of its quantised output too
        bool decode_attn, fused_step;  // the decode attention kernel; its one-launch single-token form
        bool ao_form, qkv_in_attn;     // attn_output inside the attention launch; Q | K | V too
        bool qkv_lora;                 // an active adapter has a pair on attn_q, attn_k or attn_v: the deltas are added from xn_ behind the projections
    };
    Step step_constants(int T, int n_kv_cap) const;
    AttnArgs attn_args(int il, int T, int n_kv_max, const int32_t *tok_pos) const;
    void attn_chunk_lists(AttnArgs &aa) const;
    AttnPlan plan_attn(int il, const Step &st) const;
    hipError_t attn_qkv(int il, const Step &st, const AttnPlan &p);
    hipError_t attn_core(int il, const Step &st, const AttnPlan &p);
    hipError_t attn_output(int il, const Step &st, const AttnPlan &p);
    hipError_t ffn_block(int il, const Step &st);
    hipError_t ffn_moe(int il, const Step &st);
    bool moe_selected_desc(int il, MMVQArgs &a, MMVQArgs &d) const;
    hipError_t moe_grouped_one_launch(int il, int T);
    hipError_t moe_grouped_per_expert(int il, int T, bool q80_any = false);
    hipError_t moe_grouped_q80(int il, int T);
    hipError_t moe_selected(int il, int T);
    hipError_t ffn_dense_gate_up(int il, const Step &st, bool &quantised);
    hipError_t quantise_for_down(int il, int T, bool combined, bool planes_any_T);
    hipError_t ffn_down(int il, const Step &st, bool quantised, int *n_matvec = nullptr);
    hipError_t tap_layer(int il, int T);
    hipError_t run_layers(int T, int n_kv_cap);
    hipError_t run_layers_encoder(int T, int n_kv_cap);
    hipError_t run_output(int n_out, int out_base);
    hipError_t linear(const DevTensor &w, const ActQuant &aq, const float *x_f32, int K, int T, float *out, int ld_out,
                      const float *resid, int epi);
    // bias / bias_done (optional): per-tensor bias vectors a launch may add in its epilogue; *bias_done says it did (else the caller adds them)
    hipError_t linear_multi(const DevTensor *const *ws, float *const *outs, int n, const ActQuant &aq, const float *x_f32, int T, const float *const *bias = nullptr,
                            bool *bias_done = nullptr);
    hipError_t linear_bf16(const DevTensor *const *ws, float *const *outs, const float *const *bias, int n, int K, int T, int ld_out, const float *resid, int epi);
    // active adapters (set_adapter_lora): a block with an adapted tensor takes its unfused branch and adds the deltas from its f32 operand
    struct ActiveLora { LoraAdapter *a; float scale; };
    std::vector<ActiveLora> lora_;
    float *lora_t_ = nullptr;          // t = A x of a prompt micro-batch (kernels.h lora_scratch_floats(n_ubatch))
    bool lora_on(int layer, int target) const;
    bool lora_changed();
    void drop_captured_steps();        // a change of routes: the stream is drained, the fused step's hold released, every captured graph destroyed
    // the applied control vector (apply_cvec): rows [n_layer][n_embd], which of them the caller's buffer held, the layer range
    float *cvec_ = nullptr;
    std::vector<uint8_t> cvec_present_;
    int cvec_start_ = 0, cvec_end_ = -1;
    bool cvec_on_ = false;
    hipError_t cvec_add(int il, int T);
    // outs[i] (leading dimension lds[i]) += the deltas of (layer, targets[i]) from the rows x [T][ld_x], adapter by adapter in the order they were set
    hipError_t lora_add(int layer, const int *targets, float *const *outs, const int *lds, int n, const float *x, int ld_x, int K, int T);
    // importance-matrix collection (imatrix_begin): one accumulator per (layer, site) plus the head's, in one device block with the slab scratch behind them
    enum { IMX_QKV = 0, IMX_O = 1, IMX_FFN_IN = 2, IMX_FFN_DOWN = 3, IMX_ROUTER = 4, IMX_SLOTS = 5 };   // FFN_IN / FFN_DOWN: per expert on a mixture-of-experts file
    struct ImxAcc { int K = 0, n_mat = 0; float *sum2 = nullptr; int32_t *count = nullptr; };
    struct ImxName { std::string name; int acc; };
    std::vector<ImxAcc> imx_acc_;      // [n_layer * IMX_SLOTS + 1] (the last: the head); K = 0: no such site
    std::vector<ImxName> imx_names_;   // the entries, in layer order
    bool imx_on_ = false, imx_output_ = false;
    uint8_t *imx_block_ = nullptr;
    size_t imx_block_bytes_ = 0, imx_acc_bytes_ = 0;
    float *imx_slabs_ = nullptr;
    size_t imx_slab_floats_ = 0;       // the scratch's capacity: launch_imatrix_accum refuses a launch that needs more
    // "f32 rows wanted": the operand rows of (layer, target) must exist in f32 - an adapter adds its delta from them, the collector squares them
    bool f32_rows(int layer, int target) const { return imx_on_ || lora_on(layer, target); }
    // rows x (and x2: the SwiGLU producer) [..][K] into the accumulator of (il, slot) (il < 0: the head); R launch rows through row_src, cut by meta
    hipError_t imx_collect(int il, int slot, const float *x, const float *x2, int K, int R, const int32_t *row_src, const int32_t *meta);
    void prof_mark(const char *name);
    void prof_begin();
    void prof_end();
    void *dalloc(size_t bytes);

    hipStream_t stream_ = nullptr;
    int cur_T_ = 0;                    // tokens of the micro-batch run_layers last ran (run_output: a single row needs no gather)
    std::vector<void *> allocs_;
    std::vector<KVCell> cells_;
    int head_ = 0;
    bool has_shift_ = false;
    bool meta_dirty_ = true;

    // device state
    std::vector<KVLayerView> kv_;
    int32_t *d_cell_pos_ = nullptr;
    uint64_t *d_cell_seq_ = nullptr;
    int32_t *d_delta_ = nullptr;
    // per-ubatch token arrays (device) + pinned host staging
    int32_t *d_pos_open_ = nullptr;     // encoder models: INT_MAX per token - the attention kernels' "cell position <= token position" test always passes
    int32_t *d_tok_ = nullptr, *d_pos_ = nullptr, *d_seq_ = nullptr, *d_cell_ = nullptr, *d_nkv_ = nullptr, *d_outrow_ = nullptr;
    uint64_t *d_seqmask_ = nullptr;
    uint8_t *h_stage_ = nullptr;    // pinned
    size_t stage_bytes_ = 0;
    uint8_t *d_stage_ = nullptr;
    hipEvent_t stage_event_ = nullptr;
    // activations
    float *x_ = nullptr, *xn_ = nullptr, *q_ = nullptr, *k_ = nullptr, *v_ = nullptr, *att_ = nullptr, *ffn_ = nullptr, *ffn_u_ = nullptr;
    float *xo_ = nullptr, *router_ = nullptr, *moe_out_ = nullptr;
    uint16_t *xb_ = nullptr;      // activation rows rounded to bf16 for a contraction against a bf16 tensor
    float *tp_part_ = nullptr, *tp_logits_ = nullptr;   // row split: this rank's partial sums / logits slices before the exchange
    size_t tp_logits_rows_ = 0;
    hipError_t tp_reduce_into_x(int T);                 // x_ = sum over ranks of tp_part_
    int32_t *moe_ids_ = nullptr;
    float *moe_w_ = nullptr;
    // prompt batches of a mixture-of-experts model: (token, rank) pairs grouped by expert (run_layers)
    ActQuant aq_eg_, aq_ffg_;
    float *ffn_g_ = nullptr, *ffn_ug_ = nullptr, *y_g_ = nullptr;
    int32_t *moe_meta_ = nullptr, *moe_slot_ = nullptr, *moe_tok_ = nullptr, *h_moe_meta_ = nullptr;
    ActQuant aq_e_, aq_ff_, aq_o_;
    int8_t *mmq_bh_ = nullptr, *mmq_bl_ = nullptr;   // (hi, lo) planes of the 32-code block sums for the MFMA path
    MMQWorkspace mmq_ws_;                            // partial sums of the K-split prompt contraction
    // whose block sums mmq_bh_ / mmq_bl_ currently hold (code plane pointer, K, rows): the quantisers of a prompt batch write
    // the planes themselves, launch_mmq_prep runs only when they are not there (ensure_prep)
    const void *prep_owner_ = nullptr;
    int prep_K_ = 0, prep_T_ = 0;
    hipError_t ensure_prep(const ActQuant &aq, int K, int T);
    void prep_written(const ActQuant &aq, int K, int T) { prep_owner_ = aq.qs; prep_K_ = K; prep_T_ = T; }
    bool batch_distinct_ = false;                    // the micro-batch is one token each of different sequences (decode_ubatch)
    const int8_t *bh_over_ = nullptr, *bl_over_ = nullptr;   // linear(): block-sum planes prepared by the caller for a slice of a larger batch
    float *att_part_ = nullptr;
    size_t att_part_floats_ = 0;
    int cur_max_pos_ = 0;                            // largest position of the micro-batch being decoded
    float *d_embd_ = nullptr, *h_embd_ = nullptr;   // [n_ubatch][n_embd], embeddings mode
    bool embd_fetched_ = false, last_was_embd_ = false;
    // batched single-token steps: per-token lists of the 64-cell chunks that hold cells of the token's sequence
    int32_t *h_chunks_ = nullptr, *d_chunks_ = nullptr;     // [64][chunk_stride_] lists, then [64] counts
    int chunk_stride_ = 0, chunk_lmax_ = 0, chunk_cap_ = 0;   // cap = grid size used for the lists (>= lmax; rounded up for graph reuse)                 // lmax = longest list of the current batch (0 = lists not in use)
    // whole-step kernel (decode_mega.hip): per-layer descriptors in device memory, barrier words, pinned time-out flag
    MegaLayer *d_mega_layers_ = nullptr;
    unsigned *d_mega_sync_ = nullptr;
    int *h_mega_flag_ = nullptr;
    unsigned long long *d_mega_probe_ = nullptr;   // MI355_MEGA_PROBE=1: phase time stamps of the last step (printed by the destructor)
    size_t mega_lds_ = 0;
    bool last_layers_mega_ = false;      // what the last run_layers call issued
    std::map<hipGraphExec_t, bool> graph_is_mega_, graph_is_engine_;
    bool last_layers_engine_ = false;
    int mega_state_ = 0;                 // 0 = not looked at yet, 1 = descriptors built, -1 = this model / context takes the per-launch path
    bool mega_prepare();
    bool mega_check();                   // after a stream sync: false (and last_error set) if a barrier of the last step timed out
    // layer engine (decode_engine.hip): attn_output -> gate | up -> down -> next Q | K | V of a single-token step in one persistent launch per layer
    EngineLayer *d_engine_layers_ = nullptr;
    unsigned long long *d_engine_gran_ = nullptr;      // hand-over granules
    unsigned *d_engine_epoch_ = nullptr;               // step serial (incremented by step_setup)
    unsigned long long *d_engine_probe_ = nullptr;     // MI355_ENGINE_PROBE=<layer>: wall-clock stamps of that layer's launch (printed by the destructor)
    int engine_probe_layer_ = -1;
    unsigned err_epoch_seen_ = 0;                      // stream_check: the process-wide error epoch this context has already answered for
    unsigned long long first_unchecked_launch_ = 0;    // process-wide serial of this context's first step launch since its last stream_check (0: none)
    bool logits_on_host_ = false;                      // run_output: the head's launch stored the flagged row into h_logits_ itself (no copy node behind the step)
    bool attn_out_off_ = false;                        // after an answered error epoch: the two-launch attention path (nothing in it waits for another workgroup)
    int engine_state_ = 0;                             // 0 = not looked at yet, 1 = ready, -1 = this model / context takes one launch per mat-vec
    bool engine_prepare();
    // One context at a time per device may have a step with the cross-workgroup-wait attention kernel in flight: two such kernels placed on the same CUs at the
    // same time can hold each other's item workgroups out (attn_out.hip; seen between PROCESSES in round 6, profiles/r6_tp_shared_device_trace.txt - two models
    // of one server decoding concurrently are the in-process form of it).  A context that finds the device taken runs that step on the wait-free launches.
    bool fused_acquire();
    void fused_release();                              // called wherever this context has just drained its stream
    bool holds_fused_ = false, attn_out_skip_step_ = false;
    bool stream_check();                               // after a stream sync: false (and last_error set) if a bounded wait of a stream / engine kernel gave up
    int32_t *d_moe_forced_ = nullptr;    // force_moe_ids: [n_layer][T][k] on the device (armed while moe_forced_T_ > 0)
    int moe_forced_T_ = 0, moe_forced_cap_ = 0;
    unsigned *att_counters_ = nullptr;   // per-kv-head arrival tickets of the fused decode attention (zero between launches)
    unsigned *d_step_serial_ = nullptr;  // device word: serial number of the step (incremented by the step's set-up launch; the hand-over tags / flags of attn_out.hip and decode_engine.hip)
    unsigned long long *d_qkv_gran_ = nullptr;  // attn_out.hip QF (round 6): the token's q | k | v as tagged granules inside the one launch per layer's attention block
    unsigned long long *d_ao_gran_ = nullptr;   // attn_out.hip: the quantised attention output as tagged granules (shared by the layers of a step)
    unsigned *d_ao_flags_ = nullptr;     // attn_out.hip: [n_layer][64 * ATT_SYNC_STRIDE] flag words, one per merge ticket group (they hold the serial of the step that raised them)
    float *argmax_scratch_ = nullptr, *rope_cs_ = nullptr;
    void *topk_scratch_ = nullptr;                     // launch_topk_rows workspace (own allocation, sized for topk_rows_cap_ rows on first use)
    uint8_t *d_topk_adj_ = nullptr, *h_topk_adj_ = nullptr;   // [cap] TopkAdj + [cap] row numbers: device copy and its pinned staging
    int topk_rows_cap_ = 0;
    float *spec_scratch_ = nullptr;                    // argmax_prob_ith / spec_verify: part and ticket words of the two kernels (first use)
    int32_t *d_spec_in_ = nullptr, *h_spec_ = nullptr; // rows | group starts | drafts on the device; pinned: their staging, then ids | accepted | (index, p)
    bool spec_prepare();
    // token_logprobs / logits_kl: the two kernels' part and ticket words, sized for n_ubatch rows per launch (first use); rows | targets (or rows | rows) of a
    // call on the device and their pinned staging followed by the results, both grown to the largest call
    float *lp_scratch_ = nullptr;
    int32_t *d_lp_in_ = nullptr, *h_lp_ = nullptr;
    int lp_cap_ = 0;
    bool logprob_prepare(int n);
    bool logprob_rows(const char *what, int n, const int32_t *batch_rows, int32_t *dst);
    unsigned long long *h_topk_ = nullptr;             // pinned: the winning keys
    Fuse pending_fuse_;
    int att_splits_ = 1;
    float *dbg_ = nullptr;
    bool debug_taps_ = false;
    int dbg_tokens_ = 0;
    // outputs
    float *d_logits_ = nullptr, *h_logits_ = nullptr;
    int32_t *d_argmax_ = nullptr, *h_argmax_ = nullptr;
    size_t logits_cap_rows_ = 0;
    std::vector<int> out_row_of_batch_;   // batch index -> output row or -1
    int n_out_last_ = 0;
    bool logits_fetched_ = false, argmax_fetched_ = false;
    // graph for the single-token decode step
    hipGraphExec_t graph_exec_ = nullptr;
    std::map<int, hipGraphExec_t> graphs_;   // n_kv bucket -> captured decode step
    // profiling
    bool profile_ = false;
    std::vector<std::pair<std::string, hipEvent_t>> prof_events_;
    std::vector<ProfileEntry> last_profile_;
    struct KTimer;                                     // profile mode: per-kernel begin / end events of the stream and attention launches (set_kernel_timer)
    KTimer *ktimer_ = nullptr;
    int n_kv_ = 0;
};

}  // namespace mi355
