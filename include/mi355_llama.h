/*
 * include/mi355_llama.h — C-ABI of the MI355X-native GGUF inference backend.
 *
 * This is the drop-in boundary for the ONE hot path of cortex.llamacpp: everything the
 * reference's continuous-batching loop (src/llama_server_context.cc, LlamaServerContext) calls
 * in llama.cpp's `llama.h` to run a transformer forward on a GGUF model.  Each entry point
 * below names the upstream symbol it stands in for and the reference call site that consumes it
 * (file:line under /root/reference).  Plain C types, opaque handles, int status codes, no
 * exceptions, caller-owned buffers.  All arithmetic behind it is hand-written HIP for gfx950;
 * there is no CPU fallback: every call fails with MI355_ERR_NO_DEVICE when no GPU is present.
 *
 * Thread-safety: like llama.h — a context must be driven from one thread at a time (the
 * reference drives it from the single DoBackgroundTasks thread, llama_server_context.cc:280).
 */
#ifndef MI355_LLAMA_H
#define MI355_LLAMA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_API __attribute__((visibility("default")))

typedef struct mi355_model   mi355_model;
typedef struct mi355_context mi355_context;

typedef int32_t mi355_token;
typedef int32_t mi355_pos;
typedef int32_t mi355_seq_id;

enum mi355_status {
    MI355_OK            = 0,
    MI355_ERR_NO_DEVICE = -100,  /* no MI355X / HIP runtime unavailable */
    MI355_ERR_IO        = -101,
    MI355_ERR_FORMAT    = -102,  /* not a GGUF v2/v3 file, or unsupported arch / tensor type */
    MI355_ERR_ARG       = -103,
    MI355_ERR_OOM       = -104,
    MI355_ERR_HIP       = -105,
};

/* ggml type ids as stored in GGUF (upstream ggml.h enum ggml_type; used at llama_engine.cc:272-281) */
enum mi355_type {
    MI355_TYPE_F32 = 0, MI355_TYPE_F16 = 1, MI355_TYPE_Q4_0 = 2, MI355_TYPE_Q8_0 = 8,
    MI355_TYPE_Q4_K = 12, MI355_TYPE_Q5_K = 13, MI355_TYPE_Q6_K = 14, MI355_TYPE_Q8_K = 15, MI355_TYPE_IQ4_XS = 23, MI355_TYPE_BF16 = 30, MI355_TYPE_TQ1_0 = 34, MI355_TYPE_TQ2_0 = 35,
};

/* ------------------------------------------------------------------ backend */
/* llama_backend_init (llama_engine.cc:688).  Returns MI355_OK or MI355_ERR_NO_DEVICE. */
MI355_API int         mi355_backend_init(void);
MI355_API void        mi355_backend_free(void);
MI355_API int         mi355_device_count(void);
/* last error text of the calling thread ("" if none) */
MI355_API const char *mi355_last_error(void);
/* ggml_time_us (llama_client_slot.cc:57; llama_server_context.cc:417,1314,1378,1685) */
MI355_API int64_t     mi355_time_us(void);
/* llama_print_system_info (llama_engine.cc:702) */
MI355_API const char *mi355_print_system_info(void);

/* ------------------------------------------------------------------ model */
typedef struct mi355_model_params {
    int32_t n_gpu_layers;   /* `ngl` (llama_engine.cc:609-611); this backend is device-only: must be > 0 */
    int32_t main_gpu;       /* HIP device ordinal */
    int32_t use_mmap;       /* `use_mmap` (llama_engine.cc:649) */
    int32_t use_mlock;      /* `mlock` (llama_engine.cc:569-571); accepted, ignored */
    /* row split over RCCL (see mi355_tp_init below; new keys proposed in SURVEY.md §2b) */
    int32_t tp_rank;        /* 0 when tp_size <= 1 */
    int32_t tp_size;        /* 1 = whole model on this GPU */
    /* prompt-processing copy of the projection weights as pre-expanded int8 MFMA operand planes (2 B / weight):
     * -1 = keep it when device memory allows (default), 0 = never (expand on the fly), 1 = required */
    int32_t prefill_planes;
} mi355_model_params;

MI355_API mi355_model_params mi355_model_default_params(void);
/* common_init_from_params -> llama_model_load_from_file (llama_server_context.cc:207) */
MI355_API mi355_model *mi355_model_load_from_file(const char *path_gguf, mi355_model_params params);
MI355_API void         mi355_model_free(mi355_model *model);

MI355_API int32_t  mi355_model_n_vocab(const mi355_model *m);       /* llama_vocab_n_tokens (ctx.cc:512) */
MI355_API int32_t  mi355_model_n_embd(const mi355_model *m);        /* llama_n_embd (ctx.cc:218,1033,1098) */
MI355_API int32_t  mi355_model_n_layer(const mi355_model *m);
MI355_API int32_t  mi355_model_n_head(const mi355_model *m);
MI355_API int32_t  mi355_model_n_head_kv(const mi355_model *m);
MI355_API int32_t  mi355_model_n_ctx_train(const mi355_model *m);
MI355_API uint64_t mi355_model_size(const mi355_model *m);          /* llama_model_size (llama_engine.cc:482) */
/* patches/0001-Add-API-query-buffer-size.patch:14-15,46-64 (used at llama_engine.cc:475-476) */
MI355_API uint64_t mi355_model_cpu_buffer(const mi355_model *m);    /* llama_get_cpu_buffer  -> `ram`  */
MI355_API uint64_t mi355_model_other_buffer(const mi355_model *m);  /* llama_get_other_buffer -> `vram` */
/* algorithmic weight bytes one decoded token reads; for roofline reporting */
MI355_API uint64_t mi355_model_bytes_per_token(const mi355_model *m);
MI355_API uint64_t mi355_model_planes_bytes(const mi355_model *m);  /* device bytes of the prefill planes (0 = none) */
MI355_API const char *mi355_model_desc(const mi355_model *m);
/* GGUF metadata lookup: returns 1 and fills buf if `key` exists and is a string/scalar */
MI355_API int mi355_model_meta_str(const mi355_model *m, const char *key, char *buf, size_t buf_size);

/* ------------------------------------------------------------------ context */
typedef struct mi355_context_params {
    uint32_t n_ctx;        /* `ctx_len` total KV cells (llama_engine.cc:612) */
    uint32_t n_batch;      /* `n_batch` (llama_engine.cc:617) */
    uint32_t n_ubatch;     /* `n_ubatch` (llama_engine.cc:618) */
    uint32_t n_seq_max;    /* `n_parallel` (llama_engine.cc:620) */
    int32_t  type_k;       /* `cache_type` -> mi355_type {F16,Q8_0,Q4_0} (llama_engine.cc:628-637) */
    int32_t  type_v;
    int32_t  flash_attn;   /* `flash_attn`, forced on for quantised caches (llama_engine.cc:639-647) */
    int32_t  embeddings;   /* `embedding` (llama_engine.cc:613-616) */
    int32_t  use_graphs;   /* capture the single-token decode step in a hipGraph (default 1) */
    int32_t  logits_to_host; /* 1 (default): flagged logits rows are copied to host by mi355_decode itself, as llama_decode
                              * does; 0: rows stay on the device until mi355_get_logits_ith asks (device-side greedy) */
} mi355_context_params;

MI355_API mi355_context_params mi355_context_default_params(void);
/* common_init_from_params -> llama_init_from_model (llama_server_context.cc:207-209) */
MI355_API mi355_context *mi355_context_new(mi355_model *model, mi355_context_params params);
MI355_API void           mi355_context_free(mi355_context *ctx);

MI355_API uint32_t mi355_n_ctx(const mi355_context *ctx);      /* llama_n_ctx   (ctx.cc:236) */
MI355_API uint32_t mi355_n_batch(const mi355_context *ctx);    /* llama_n_batch (ctx.cc:1351) */
MI355_API uint32_t mi355_n_ubatch(const mi355_context *ctx);   /* llama_n_ubatch(ctx.cc:1352) */
MI355_API uint64_t mi355_context_device_bytes(const mi355_context *ctx); /* KV + activations on device */

/* llama_batch exactly as the reference fills it (llama_server_context.cc:265,1630-1635) */
typedef struct mi355_batch {
    int32_t        n_tokens;
    mi355_token   *token;     /* [n_tokens] */
    float         *embd;      /* NULL, or [n_tokens][n_embd] rows that take the place of the token embeddings (then token is NULL): how the
                               * reference feeds image embeddings to the model (llava_embd_batch, llama_server_context.cc:1093-1107) */
    mi355_pos     *pos;       /* [n_tokens] */
    int32_t       *n_seq_id;  /* [n_tokens] */
    mi355_seq_id **seq_id;    /* [n_tokens][n_seq_id] */
    int8_t        *logits;    /* [n_tokens] != 0 => produce logits for that row */
} mi355_batch;

MI355_API mi355_batch mi355_batch_init(int32_t n_tokens, int32_t embd, int32_t n_seq_max); /* llama_batch_init (ctx.cc:265) */
MI355_API void        mi355_batch_free(mi355_batch batch);

/* llama_decode (llama_server_context.cc:654,1085,1103,1635).
 * Returns 0 on success, 1 if no KV slot could be found for the batch (caller halves n_batch and
 * retries, ctx.cc:1636-1663), < 0 on a fatal error.  Logits rows are host-visible afterwards. */
MI355_API int32_t mi355_decode(mi355_context *ctx, mi355_batch batch);
/* n greedy steps of one sequence in one call - per step: llama_decode of the previous step's token at pos0 + i, its logits row made host-visible
 * (llama_get_logits_ith), the arg-max as the next token (the greedy end of the sampler chain): the inner loop of the reference's UpdateSlots for a temperature-0
 * request (llama_server_context.cc:1628-1707), on the C side.  out_tokens (nullable) [n].  Returns the steps done (n, or fewer with the reason in mi355_last_error). */
MI355_API int32_t mi355_greedy_steps(mi355_context *ctx, mi355_token first, mi355_pos pos0, mi355_seq_id seq, int32_t n, mi355_token *out_tokens);
/* llama_get_logits_ith as used through common_sampler_sample(ctx, idx) (ctx.cc:1679-1680).
 * i indexes the batch of the last mi355_decode; NULL if that row had logits[i] == 0, in embeddings mode, or when the step's results were discarded
 * (an in-kernel wait that gave up, a failed copy) - mi355_last_error then says which. */
MI355_API float  *mi355_get_logits_ith(mi355_context *ctx, int32_t i);
/* device-side greedy front end: argmax token of row i without copying the row */
MI355_API int32_t mi355_get_argmax_ith(mi355_context *ctx, int32_t i);
/* ---- speculative decoding (the reference's server takes a draft model as --model-draft).  Everything below reads the device logits of the
 * last mi355_decode, also with logits_to_host = 0, and moves a few words to the host, never a row.
 * The arg-max token of row i (mi355_get_argmax_ith's rule and preconditions) and, in *p, its softmax probability over the WHOLE vocabulary,
 * 1 / sum_j exp(x_j - max) in f32 (0 where the row's maximum is not finite).  < 0 on failure. */
MI355_API int32_t mi355_get_argmax_prob_ith(mi355_context *ctx, int32_t i, float *p);
/* Greedy acceptance over the rows of the last mi355_decode: group g owns batch rows group_start[g] .. group_start[g + 1] - 1, k_g + 1 rows for k_g <= 16
 * drafted tokens, all of them flagged; the groups are adjacent, R = group_start[n_groups] - group_start[0] <= 1088 rows, n_groups <= 64.  draft [R] runs
 * parallel to those rows (the entry of a group's last row is ignored).  ids_out [R]: each row's arg-max; n_accept_out [n_groups]: the largest a <= k_g with
 * ids == draft on the group's first a rows.  One launch, one synchronisation, 4 (R + n_groups) bytes back.  Returns R; < 0 with mi355_last_error set when a
 * row was not flagged, in embeddings mode, or on a rank of a row split. */
MI355_API int32_t mi355_spec_verify(mi355_context *ctx, int32_t n_groups, const int32_t *group_start, const mi355_token *draft, mi355_token *ids_out,
                                    int32_t *n_accept_out);
/* mi355_greedy_steps with a draft model's context beside the target's.  Both hold sequence `seq` over positions [0, pos0); `first` goes to pos0.  A round:
 * the draft context decodes what it has not seen (the last emitted token; two tokens after a round that accepted n_max drafts), then drafts greedily through
 * mi355_get_argmax_prob_ith until n_max <= 16 tokens or the first probability below p_min (that token is not drafted); fewer than n_min drafts are dropped; the
 * target decodes [last, drafts] with every row flagged and mi355_spec_verify says how many hold (no drafts: a plain step); the agreed drafts and the target's
 * next token are emitted and both caches forget everything behind them.  Exactly n tokens: the last round is cut, its surplus KV removed too.  The tokens
 * are those of mi355_greedy_steps on the target wherever its arg-max does not hinge on batch-size rounding.  stats (nullable) [4]: rounds, drafted, accepted
 * (drafts that were emitted: n = rounds + accepted), plain steps (rounds without a draft).  Returns the tokens written (n, or fewer with the reason in mi355_last_error). */
MI355_API int32_t mi355_speculative_steps(mi355_context *ctx_tgt, mi355_context *ctx_dft, mi355_token first, mi355_pos pos0, mi355_seq_id seq, int32_t n,
                                          int32_t n_max, int32_t n_min, float p_min, mi355_token *out_tokens, int64_t *stats);
/* ---- perplexity and KL divergence (what upstream's llama-perplexity prints).  Like the block above these read the device logits of the last
 * mi355_decode, with logits_to_host 0 or 1, and bring a few words per row to the host; a later mi355_get_logits_ith still returns the same rows.
 * logprob_out [n]: log softmax(row batch_rows[r])[targets[r]] over the WHOLE vocabulary, x_t - max - log(sum_j exp(x_j - max)) in f32; rank_out (nullable) [n]:
 * how many entries beat the target under the arg-max rule (0: the target is what mi355_get_argmax_ith returns).  A row whose maximum is not finite, or whose
 * target logit is NaN, gives NaN and -1.  Returns n; < 0 with mi355_last_error set in embeddings mode, for a row that was not flagged, a target outside
 * [0, n_vocab) or on a rank of a row split. */
MI355_API int32_t mi355_get_token_logprobs(mi355_context *ctx, int32_t n, const int32_t *batch_rows, const mi355_token *targets, float *logprob_out,
                                           int32_t *rank_out);
/* kl_out [n]: KL(P || Q) in nats, P = row rows_base[r] of ctx_base's last decode (the f16 / Q8_0 model), Q = row rows[r] of ctx's (the model under test);
 * not clamped at 0, exactly 0 for identical rows.  same_top_out (nullable) [n]: 1 where both rows have the same arg-max.  A row with a non-finite entry gives
 * NaN and -1.  Refused as above, and when the two contexts differ in n_vocab or device or are one context. */
MI355_API int32_t mi355_logits_kl(mi355_context *ctx, mi355_context *ctx_base, int32_t n, const int32_t *rows_base, const int32_t *rows, float *kl_out,
                                  int32_t *same_top_out);
/* The llama-perplexity procedure on the C side (restated from memory of llama.cpp's perplexity(): not pinned to a source line).  n_chunks = n_tokens / n_chunk
 * (2 <= n_chunk <= n_ctx of every context involved; the tail is dropped).  Per chunk: sequence `seq` is cleared, the chunk's first token is replaced by bos
 * (-1: none), the chunk is decoded in pieces of at most n_ubatch tokens with positions n_chunk / 2 .. n_chunk - 2 flagged, and every flagged row is scored
 * against the token that follows it.  With ctx_base (nullable) the same pieces are decoded there and every row also gives the base's log-probability and
 * KL(base || ctx).  A row any of whose figures is NaN counts in `dead` alone.  logprob_out / kl_out (nullable): n_chunks * (n_chunk - 1 - n_chunk / 2)
 * floats in scoring order, NaN for dead rows.  cb (nullable) receives the running stats after every chunk and stops the run by returning non-zero.  The
 * sequence is removed from both caches on return.  perplexity = exp(nll / count). */
typedef struct mi355_ppl_stats {
    int64_t n_chunks, count, top1, dead, same_top;   /* chunks scored; rows scored; rows whose target was the arg-max; rows skipped; rows with base's arg-max */
    int32_t has_base, stopped;
    double  nll, nll2;                                /* sum and sum of squares of -logprob */
    double  nll_base, nll2_base, kl, kl2;             /* with ctx_base: the same for the base model; sum and sum of squares of the per-row KL */
} mi355_ppl_stats;
typedef int32_t (*mi355_ppl_callback)(const mi355_ppl_stats *running, void *user);
MI355_API int32_t mi355_perplexity(mi355_context *ctx, mi355_context *ctx_base, const mi355_token *tokens, int64_t n_tokens, int32_t n_chunk, mi355_token bos,
                                   mi355_seq_id seq, float *logprob_out, float *kl_out, mi355_ppl_callback cb, void *user, mi355_ppl_stats *stats);
/* ---- importance matrix (what upstream's llama-imatrix records for llama-quantize --imatrix).  Between begin and end every micro-batch of
 * every mi355_decode of this context adds, for every weight matrix it multiplies, the per-input-column sum of squares of the f32 rows the projection consumes
 * and the number of rows (per expert for the *_exps tensors), on the device.  While it is on, the steps take the launches that leave those rows in memory
 * (the ones an adapter on every target forces; no whole-step launch, layer engine or captured graph; a mixture-of-experts feed-forward grouped by expert at
 * every batch size), so logits may differ from a plain run in the last digits; after end the steps are what they were before begin, bit for bit.
 * process_output != 0 also collects the output head (output.weight, or token_embd.weight for a tied head) from the final-norm rows of the flagged tokens.
 * begin returns MI355_OK, or MI355_ERR_ARG with the reason in mi355_last_error: collection already on, an encoder model, a rank of a row split, a
 * mixture-of-experts context without grouped buffers (n_ubatch < 8) or with float expert tensors, a row length that is no multiple of 32, out of memory.
 * The accumulators, counts and scratch are device memory from begin to end (counted in mi355_context_device_bytes).  clear zeroes sums and counts and keeps
 * collecting. */
MI355_API int32_t mi355_imatrix_begin(mi355_context *ctx, int32_t process_output);
MI355_API int32_t mi355_imatrix_end(mi355_context *ctx);
MI355_API int32_t mi355_imatrix_clear(mi355_context *ctx);
/* The entries while collection is on, in layer order, named after the GGUF tensor multiplied (blk.N.attn_q.weight ...).  Tensors with one input (attn_q /
 * attn_k / attn_v; ffn_gate / ffn_up; ffn_gate_exps / ffn_up_exps) are separate entries with the same values.  entry: the name into name_buf (cap bytes,
 * always terminated), the row length ne0 and the number of matrices n_mat (1, or n_expert); returns the name's length, < 0 for an index outside the list. */
MI355_API int32_t mi355_imatrix_n_entries(const mi355_context *ctx);
MI355_API int32_t mi355_imatrix_entry(const mi355_context *ctx, int32_t i, char *name_buf, int32_t cap, int32_t *ne0, int32_t *n_mat);
/* sum2 [n_mat][ne0] and counts [n_mat] of entry i: one synchronisation, then the copies.  A sum that is not finite returns MI355_ERR_ARG with the tensor's
 * name in mi355_last_error (upstream aborts on it). */
MI355_API int32_t mi355_imatrix_get(mi355_context *ctx, int32_t i, float *sum2, int32_t *counts);
/* device-side sampling front end beyond greedy (stands in for the head of common_sampler_sample's chain, reference call site
   src/llama_server_context.cc:1679-1698): the k <= 128 best candidates of row i after logit_bias and the repetition / frequency / presence penalties,
   best first (higher logit; lower token id on ties) - k (token, logit) pairs cross to the host instead of the whole row.  adj_tok / adj_bias / adj_count:
   n_adj <= 192 adjusted tokens (bias 0 = none, count = occurrences in the penalty window, 0 = not penalised).  Returns k or < 0. */
MI355_API int32_t mi355_get_topk_ith(mi355_context *ctx, int32_t i, int32_t k, int32_t n_adj, const int32_t *adj_tok, const float *adj_bias,
                                     const int32_t *adj_count, float penalty_repeat, float penalty_freq, float penalty_present,
                                     int32_t *toks_out, float *logits_out);
/* diagnosis: single-token steps this context ran as ONE launch (decode_mega.hip; see mi355_debug_set_option "decode_mega") */
MI355_API int64_t mi355_debug_mega_steps(const mi355_context *ctx);
/* diagnosis: single-token steps this context ran through the layer engine (decode_engine.hip: one persistent launch per layer for the mat-vecs between two
   attention calls; opt-in: mi355_debug_set_option "decode_engine" 1 or MI355_ENGINE=1) */
MI355_API int64_t mi355_debug_engine_steps(const mi355_context *ctx);
/* single-token steps of this context that took the wait-free launches because another context of the device had the one-launch attention + attn_output kernel
   (workgroups that wait for each other) in flight: two models of one server decoding at the same time never run that kernel beside each other */
MI355_API int64_t mi355_debug_fused_skipped_steps(const mi355_context *ctx);
/* diagnosis: launches of this context that ran a layer's Q | K | V mat-vecs INSIDE its attention + attn_output launch (csrc/attn_out.hip QF, round 6: one launch
   per layer for the whole attention block of a single-token step; "qkv_attn_fused" 0 / MI355_QKV_ATTN_FUSED=0 keeps Q | K | V a launch of its own).  Counts
   launches issued eagerly or while a graph was captured, not graph replays. */
MI355_API int64_t mi355_debug_qkv_attn_launches(const mi355_context *ctx);
/* host logic only (no GPU needed): would a single-token step of a layer with these tensor types (MI355_TYPE_*) and this geometry run its Q | K | V inside the attention
   launch at a context of n_kv cells?  Returns the launch's LDS bytes per workgroup (<= 163840) and, in *slots_out, the 4 KiB DMA slots of a workgroup's rows; 0 = the two
   launches (types without a form, n_embd != n_head * head_dim or > 4096, head_dim != 128, rows that do not fit beside W_o: Llama-2-7B) */
MI355_API int64_t mi355_debug_qkv_attn_plan(int32_t type_q, int32_t type_k, int32_t type_v, int32_t type_o, int32_t n_embd, int32_t n_head, int32_t n_head_kv, int32_t head_dim,
                                            int32_t type_kv, int32_t n_kv, int32_t *slots_out);
/* llama_set_embeddings (ctx.cc:299) */
MI355_API void    mi355_set_embeddings(mi355_context *ctx, int32_t enabled);
/* llama_get_embeddings_ith (ctx.cc:1042-1044): final-norm hidden state (n_embd floats, host memory) of batch row i of the
 * last mi355_decode issued while embeddings were enabled; NULL otherwise.  Pooling is NONE on this architecture, so
 * llama_get_embeddings_seq has no counterpart (the reference falls back to _ith, ctx.cc:1043-1045). */
MI355_API float  *mi355_get_embeddings_ith(mi355_context *ctx, int32_t i);
MI355_API void    mi355_synchronize(mi355_context *ctx);

/* ------------------------------------------------------------------ LoRA adapters
 * llama_adapter_lora_init / llama_adapter_lora_free / llama_set_adapter_lora / llama_rm_adapter_lora / llama_clear_adapter_lora (what common_init_from_params
 * does with params.lora_adapters).  A convert_lora_to_gguf.py file: general.type "adapter", adapter.type "lora", the base model's general.architecture,
 * adapter.lora.alpha, pairs <base tensor>.lora_a [K, r] / .lora_b [r, N], both F32 or both F16, r 1 .. 512, on blk.N.{attn_q,attn_k,attn_v,attn_output,
 * ffn_gate,ffn_up,ffn_down}.weight and output.weight of a decoder model held on one device.  Applied at run time, never merged:
 *   y = W x + sum over the set adapters of scale * alpha / r * B (A x)      (scale alone when alpha is 0), in the order the adapters were set.
 * init: NULL + mi355_last_error on a refusal.  The model owns the device copy (counted in mi355_model_other_buffer); free an adapter only once no context
 * has it set.  set (again: a new scale) / rm / clear drain the context and drop its captured steps.  rm: -1 when the adapter was not set. */
typedef struct mi355_adapter_lora mi355_adapter_lora;
MI355_API mi355_adapter_lora *mi355_adapter_lora_init(mi355_model *model, const char *path);
MI355_API void    mi355_adapter_lora_free(mi355_adapter_lora *adapter);
MI355_API float   mi355_adapter_lora_alpha(const mi355_adapter_lora *adapter);
MI355_API int32_t mi355_adapter_lora_n_pairs(const mi355_adapter_lora *adapter);
MI355_API int32_t mi355_set_adapter_lora(mi355_context *ctx, mi355_adapter_lora *adapter, float scale);
MI355_API int32_t mi355_rm_adapter_lora(mi355_context *ctx, mi355_adapter_lora *adapter);
MI355_API void    mi355_clear_adapter_lora(mi355_context *ctx);

/* Control vectors (unpinned: upstream's source is not in the reference tree, the semantics are llama_apply_adapter_cvec's as remembered).
 * data: the vectors of layers 1, 2, ... back to back, `len` floats; layer il is at n_embd * (il - 1) and present when n_embd * il <= len.  From the next step on
 * every layer il_start <= il <= il_end with a present vector ends with x[t][:] = fl32(x[t][:] + v_il[:]) on every row of the batch: one extra launch per steered
 * layer, inside the captured graph where the step is captured.  Layer 0 never has a vector.  data == NULL clears (the other arguments are not read): the steps
 * are bit for bit what they were before.  Apply and clear drain the context and drop its captured steps.
 * MI355_OK, or MI355_ERR_ARG with mi355_last_error naming the cause and the context unchanged: a NULL context, an encoder model, a rank of a row split, an
 * n_embd that is not the model's, len not a multiple of n_embd, a non-finite value, il_start > il_end. */
MI355_API int32_t mi355_apply_adapter_cvec(mi355_context *ctx, const float *data, size_t len, int32_t n_embd, int32_t il_start, int32_t il_end);
/* common_control_vector_load: n GGUF files of F32 one-dimensional tensors direction.N (N >= 1, one length n_embd), file i accumulated as scales[i] * tensor into
 * layer N's slot, the files summed.  Returns the number of floats of the result, n_embd * (the highest layer named), laid out as mi355_apply_adapter_cvec takes
 * it, and writes them to `out` when cap_floats holds them (out may be NULL to ask for the size); *n_embd_out (nullable) = n_embd.  MI355_ERR_ARG (a NULL list,
 * n < 1) or MI355_ERR_FORMAT with mi355_last_error naming file and tensor: a file that does not open, direction.0, a direction tensor that is not F32 or not
 * one-dimensional, different lengths within or between files, no direction tensor at all.  Host arithmetic; needs no device. */
MI355_API int64_t mi355_control_vector_load(const char *const *paths, const float *scales, int32_t n, float *out, size_t cap_floats, int32_t *n_embd_out);
/* What llama-cvector-generator computes per layer (csrc/cvec.hip), on host pointers: the direction of rows [n_rows][n_embd] (f32).  method 0 (pca): the first
 * principal direction by the power method on rows^T rows from the start vector init [n_embd], three launches an iteration with no atomics and every summation
 * order fixed by the shape, so the same arguments give the same bytes; the host reads |b_new - b_old| every n_batch iterations and stops when it is < tol or
 * after n_iter.  method 1 (mean): the normalised mean row (init, n_iter, n_batch, tol are not read).  The sign is chosen so that sum over the rows of row . dir
 * >= 0.  dir_out [n_embd] unit length; iters_out (nullable) iterations run; dist_out (nullable) the last distance read.  A guard region behind the device
 * outputs is checked.  MI355_ERR_ARG with the cause named and dir_out untouched: a NULL pointer, an unknown method, n_rows < 1 (or > 2^20), n_embd % 32
 * (or > 65536), n_iter < 1 or n_batch < 1 (pca), a non-finite input, a zero init (pca), all-zero rows, an iteration that reaches the zero vector (init is
 * orthogonal to every row; rows whose mean is zero). */
MI355_API int mi355_cvec_direction(int32_t method, const float *rows, int64_t n_rows, int32_t n_embd, const float *init, int32_t n_iter, int32_t n_batch, float tol,
                                   float *dir_out, int32_t *iters_out, float *dist_out);

/* KV cache bookkeeping (ctx.cc:287; 661,1547; 1288,1540,1542; 1290) */
MI355_API void    mi355_kv_cache_clear(mi355_context *ctx);
MI355_API int32_t mi355_kv_cache_seq_rm(mi355_context *ctx, mi355_seq_id seq, mi355_pos p0, mi355_pos p1); /* 1 = ok */
MI355_API void    mi355_kv_cache_seq_cp(mi355_context *ctx, mi355_seq_id src, mi355_seq_id dst, mi355_pos p0, mi355_pos p1);
MI355_API void    mi355_kv_cache_seq_add(mi355_context *ctx, mi355_seq_id seq, mi355_pos p0, mi355_pos p1, mi355_pos delta);
MI355_API int32_t mi355_kv_cache_used_cells(const mi355_context *ctx);

/* ------------------------------------------------------------------ a sequence's KV state
 * llama_state_seq_get_size / get_data / set_data and llama_state_seq_save_file / load_file.  The blob is this project's own format, versioned:
 *   8 little-endian 32-bit words - magic "M5KV", version 1, type_k, type_v, n_layer, n_head_kv, head_dim, n (cells) - then n int32 positions, ascending,
 *   then per layer K rows [n][n_head_kv * head_dim] and V rows likewise in the ggml layout of the cache type (f16 halves, 34-byte q8_0 / 18-byte q4_0 blocks);
 *   size = 32 + 4 n + n_layer * n * (row_bytes_k + row_bytes_v).
 * get_data applies a pending K-shift first and returns the bytes written.  set_data checks the header against the context, removes what dst holds, gives it n
 * fresh cells (its region's lowest free ones, in position order) and returns the bytes consumed.  0 = refused, mi355_last_error names the field and both
 * values; a refused set_data leaves dst as it was, or empty - never half-written.  Encoder contexts and the ranks of a row split have no sequence state.
 * The file: 4 words - magic "M5KF", version 1, n_tokens, 0 - an 8-byte blob length, the tokens, the blob; written to a temporary name and renamed; load_file
 * checks the file's length against its header before it reads a row.  Both return the file's bytes, 0 = refused. */
MI355_API size_t mi355_state_seq_get_size(mi355_context *ctx, mi355_seq_id seq);
MI355_API size_t mi355_state_seq_get_data(mi355_context *ctx, uint8_t *dst, size_t cap, mi355_seq_id seq);
MI355_API size_t mi355_state_seq_set_data(mi355_context *ctx, const uint8_t *src, size_t len, mi355_seq_id dst);
MI355_API size_t mi355_state_seq_save_file(mi355_context *ctx, const char *path, mi355_seq_id seq, const mi355_token *tokens, size_t n_tokens);
MI355_API size_t mi355_state_seq_load_file(mi355_context *ctx, const char *path, mi355_seq_id dst_seq, mi355_token *tokens_out, size_t cap, size_t *n_tokens_out);
/* measurement aid: the pack launch, the device-to-host copy and the unpack launch of the context's last get_data / set_data, from events of their own (ms);
 * timing is switched on by the first call and costs a stream synchronisation per launch from then on */
MI355_API void    mi355_debug_state_seq_timing(mi355_context *ctx, float out_ms[3]);

/* debugging taps for parity tests (enable before decode): residual stream after layer `il` for the last
 * decoded micro-batch, copied to dst[n_tokens * n_embd]; returns n_tokens or < 0 */
MI355_API void    mi355_debug_enable_taps(mi355_context *ctx, int32_t enabled);
MI355_API int32_t mi355_debug_layer_out(mi355_context *ctx, int32_t il, float *dst, size_t dst_floats);

/* ------------------------------------------------------------------ per-op entry points
 * Host-buffer wrappers around the individual HIP kernels, for parity tests and rocprof.
 * Each copies inputs to the device, runs the same kernel the decode graph uses, copies back. */

/* quantize_row_q8_K / quantize_row_q8_0 (activation side).  out receives ggml-layout blocks.  Q8_K: n_per_row % 256 == 0; Q8_0: any multiple of 32 (a row
 * may end inside a 256-group).  From 32 rows on the prompt-batch form of the kernel runs. */
MI355_API int mi355_op_quantize_act(int32_t act_type, const float *x, int64_t n_per_row, int64_t n_rows, void *out_blocks);
/* RMSNorm(x) * w and the Q8_0 quantisation of the result in one launch, as a layer's norm step runs it (n any multiple of 32; from T = 32 on the prompt-batch
 * form).  out_blocks: T rows of n / 32 block_q8_0; y_f32 (nullable): the f32 rows [T][n] the blocks were made from. */
MI355_API int mi355_op_rms_norm_quant(const float *x, const float *w, int64_t n, int64_t T, float eps, float *y_f32, void *out_blocks);
/* silu(gate) * up and its Q8_0 quantisation in one launch (gate, up: [T][n], n any multiple of 32); out_blocks as above. */
MI355_API int mi355_op_swiglu_quant(const float *gate, const float *up, int64_t n, int64_t T, void *out_blocks);
/* y[T][N] = W[N][K] . x[T][K]; W is ggml-layout blocks of `type`.  isum/msum (nullable):
 * per (token, row, block) integer partial sums for bit-exact checks.  IQ4_XS (type 23, Q8_K activations): isum is the
 * super-block's sum over sub-blocks of (ls - 32) * sum(level * q8), msum is 0.  BF16 (type 30): the rows of x are rounded to bf16
 * (ggml's f32 -> bf16) and the model path's kernel runs: the matrix cores from 8 tokens on, else the bf16 weight stream.
 * The 32-element formats (Q8_0, Q4_0, Q5_0, IQ4_NL, Q4_1, Q5_1, MXFP4: Q8_0 activations) and F16 take any K % 32 == 0, the other types K % 256 == 0.
 * Q4_1 / Q5_1 (types 3 / 7): one token with K % 256 == 0 is quantised in the mat-vec's
 * prologue, the form the weight stream takes these types in; isum is the block's sum of q * a (q the unsigned code), msum the block's
 * sum of a - the block contributes (d * d8) * isum + m * (d8 * msum).  With "mmq_planes" 1 and T >= 32 the tensor's Q8_0-layout copy runs on the
 * matrix cores, in the form "mmq_q80_tiles" forces (1 | 2 | 4 token tiles per wave; 0: the launcher's choice).
 * MXFP4 (type 39, Q8_0 activations): as Q4_1 / Q5_1 for K, the one-token form and the copy; isum is the block's sum of level * a, msum is 0 - the block
 * contributes (d * d8) * isum with d from its E8M0 byte.
 * TQ1_0 / TQ2_0 (types 34 / 35, the ternary formats, Q8_K activations, K % 256 == 0): isum is the super-block's sum of (q - 1) * a with q the code 0..2 (the
 * formats' formulas rule for every byte value: a TQ2_0 code of 3 is weight + 2 d), msum is 0 - the super-block contributes (d * d8) * isum.  One token runs on
 * the weight stream or the register ring, 2 .. 31 on the generic mat-vec, T >= 32 on the plane kernels with "mmq_planes" 1 (planes only, as Q2_K / Q3_K / IQ4_XS). */
MI355_API int mi355_op_mul_mat(int32_t type, const void *W, int64_t N, int64_t K, const float *x, int64_t T,
                               float *y, int32_t *isum, int32_t *msum);
/* Test hook: y = resid + W . x (resid, y: [T][N]) on the launches that take a residual in their epilogue through this entry point: the Q8_0 prompt kernel
 * (Q8_0 tensors, and the Q8_0-layout copies of Q4_0 / Q5_0 / IQ4_NL / Q4_1 / Q5_1 / MXFP4 tensors with "mmq_planes" 1), T >= 32; MI355_ERR_ARG otherwise. */
MI355_API int mi355_op_mul_mat_add(int32_t type, const void *W, int64_t N, int64_t K, const float *x, int64_t T, const float *resid, float *y);
/* One token's mat-vec (a 32-element format, K % 32 == 0, K <= 8192) with the activation made in the launch's prologue, as a decode step's launches take it:
 * norm_w set: RMSNorm(x) * norm_w, then Q8_0 (Q | K | V, ffn_gate | ffn_up, the head); norm_w null: Q8_0 of x (ffn_down).  y[N] has the bits of the
 * quantiser's launch followed by mi355_op_mul_mat. */
MI355_API int mi355_op_mul_mat_fused(int32_t type, const void *W, int64_t N, int64_t K, const float *x, const float *norm_w, float eps, float *y);
/* Test hook: one mat-vec launch of a decode step, issued through the code the model issues it with (host/runtime.cc make_seg, single_token_desc, mmvq_tokens).
 *   n_seg 1..3 weight tensors W[s] (ggml rows, quantised type types[s], N[s] rows of K) over the same activation x [T][K], 1 <= T <= 17 (launches of 16 / 8 / 4 / 2 / 1);
 *   epi 0: y[s][t][n] = W[s][n] . a[t];  1 (one tensor): resid + that, resid [T][N[0] + ld_pad];  2 (two tensors, ffn_gate | ffn_up): y[0] = silu(y0) * y1;
 *   fuse 0: a = the quantiser's launch over x;  1 (T == 1): RMSNorm(x, eps) * norm_w quantised in the launch's prologue;  2 (T == 1): x quantised there;
 *   want_host_copy (T == 1, one tensor): y_host[N[0]] is the launch's second copy in pinned host memory;
 *   n_sel 2..8 (T == 1; one tensor, or the SwiGLU pair): W[s] holds n_expert tensors back to back, expert_ids[n_sel] is read on the device, y[s] is
 *   [n_sel][N[s] + ld_pad], and with fuse 2 x is [n_sel][K] (every expert quantises its own row) - the two launches of a mixture-of-experts step.
 * Every y[s] is a whole out buffer, rows N[s] + ld_pad wide, filled with 0xFF bytes before the launch (y_host likewise): an unwritten result reads as NaN, a
 * write past N[s] shows in the pad columns.  path[40]: 8 words per launch issued, in order - tokens, kernel (0 generic, 1 register ring, 2 weight stream,
 * 3 tiled), and for the weight stream its role (0 any, 1 qkv, 2 gate_up, 3 ffn_down, 4 head), passes of 2048, fast_ok, down_early, moe, ternary; zero beyond.
 * MI355_ERR_HIP where a launch fails or a weight-stream kernel raises the process's stream error word. */
MI355_API int mi355_op_mat_vec_step(int32_t n_seg, const int32_t *types, const void *const *W, const int64_t *N, int64_t K, const float *x, int64_t T, int32_t epi,
                                    const float *resid, int32_t fuse, const float *norm_w, float eps, int32_t want_host_copy, int32_t n_sel, int32_t n_expert,
                                    const int32_t *expert_ids, int64_t ld_pad, float *const *y, float *y_host, int32_t *path);
/* Test hook: one mat-mul launch of a dense prompt batch (or of a batched decode step) as the model issues it: mmq.hip's K-split, plane and LDS-plane kernels.
 *   n_seg 1..3 weight tensors W[s] (ggml rows of type types[s]: Q4_K, Q5_K, Q6_K; one tensor on the plane kernels also Q2_K, Q3_K, IQ4_XS; N[s] rows of K,
 *   K % 256 == 0) over one activation of 3 <= T <= 600 rows;
 *   epi 0: y[s][t][n] = W[s][n] . a[t];  1 (one tensor): resid + that, resid [T][N[0] + ld_pad], and with in_place the residual buffer IS the out buffer, as
 *   attn_output and ffn_down run;  2 (two tensors of one type and N: ffn_gate | ffn_up): y[0] = silu(y0) * y1, y[1] is not written (may be NULL);
 *   prologue 0: a = launch_quantize(x), then launch_mmq_prep;  1: launch_rmsnorm_quant(x, norm_w, eps) writing the bh / bl block-sum planes itself;
 *   2: launch_swiglu_quant(g, u) likewise, x = g [T][K] then u [T][K];  3: launch_quantize writing bh / bl.  x is [T][K] otherwise;
 *   form 0: the launch the model chooses (host/runtime.cc prompt_mul_mat_choice; every tensor has its plane set, adjacent in one arena);  1: the K-split kernel
 *   (launch_mmq_ksplit_multi; epi 2: its SwiGLU pair);  2: the plane sets, expanded into one arena (launch_mmq_planes_multi with seg_types, the K-split
 *   workspace and the residual; epi 2: launch_mmq_planes_swiglu);  3: the expansion on the fly (launch_mmq, one tensor).  mi355_debug_set_option "mmq_tiles"
 *   1 / 2 / 4 and "mmq_split" pick the tile form and the K split as everywhere.
 * Every y[s] is a whole out buffer [T][N[s] + ld_pad], 0xFF bytes before the launch except where in_place put the residual there: an unwritten result reads as
 * NaN, a write past N[s] shows in the pad columns.  MI355_ERR_ARG where the arguments or the chosen launcher's row rules refuse the launch: nothing is launched
 * and the buffers come back as 0xFF bytes.  path[8]: [0] the kernel (1 K-split, 2 planes 256 x 32, 3 planes 128 x 128, 4 the 128 x 256 LDS kernel, 5 on the
 * fly), [1] 32-token tiles per workgroup of the K-split kernel (else 0), [2] the K split (n_split), [3] mixed plane formats, [4] SwiGLU epilogue, [5] whether
 * launch_mmq_prep was issued, [6], [7] zero.  (form 0 with tensors whose plane sets do not all fuse: path describes the fused launch, the others follow alone.) */
MI355_API int mi355_op_prompt_mul_mat(int32_t n_seg, const int32_t *types, const void *const *W, const int64_t *N, int64_t K, const float *x, int64_t T, int32_t epi,
                                      const float *resid, int32_t in_place, int32_t prologue, const float *norm_w, float eps, int32_t form, int64_t ld_pad,
                                      float *const *y, int32_t *path);
/* Test hook: one producer of the quantised activation of the MFMA kernels, called with Q8_K and the bh / bl block-sum planes (bsum = 64 * bh + bl) as the model
 * calls it: producer 0 launch_quantize(x);  1 launch_rmsnorm_quant(x, norm_w, eps);  2 launch_swiglu_quant(x, x2).  x (and x2) [T][n], n % 256 == 0.
 * out_blocks: T rows of n / 256 ggml block_q8_K;  out_bh / out_bl: [T][n / 16] int8 each, 0xFF bytes before the launch;  prep_bh / prep_bl: what launch_mmq_prep
 * makes of the same rows;  y_f32 (producer 1, may be NULL): the f32 rows the blocks were made from. */
MI355_API int mi355_op_act_q8k_planes(int32_t producer, const float *x, const float *x2, const float *norm_w, float eps, int64_t n, int64_t T, void *out_blocks,
                                      int8_t *out_bh, int8_t *out_bl, int8_t *prep_bh, int8_t *prep_bl, float *y_f32);
/* ggml's f32 -> bf16 rounding as the bf16 kernels' activation pass does it (nearest, ties to even; NaN quieted; subnormals kept); n % 8 == 0 */
MI355_API int mi355_op_f32_to_bf16(const float *x, int64_t n, uint16_t *out);
/* Up to three BF16 tensors W[s] ([N[s]][K] bf16 rows, K % 8 == 0; the matrix cores want K % 16 == 0) against the same T rows of x, as a decoder layer launches them:
 *   y[s][t][n] = W[s][n] . bf16(x[t]) + bias[s][n]                                  (bias and its entries nullable)
 *   epi 1 (one tensor): y[0] = resid + that, resid [T][N[0]];  epi 2 (two tensors of equal N: ffn_gate, ffn_up): y[0] = silu(y0) * y1, y[1] is not written.
 * path 0: the model path's choice; 1: the weight stream (all tensors in ONE launch per token chunk, the epilogue fused); 2: the matrix cores (one launch per
 * tensor, SwiGLU as its own pass).  tokens_per_launch (stream only): 0 = chunks of 16, 8, 4, 2, 1; else every launch takes that many tokens (1, 2, 4, 8, 16;
 * T a multiple of it).  use_graph 1: the launches are captured into a graph and replayed. */
MI355_API int mi355_op_mul_mat_bf16(int32_t n_seg, const void *const *W, const int64_t *N, int64_t K, const float *x, int64_t T, const float *const *bias,
                                    const float *resid, int32_t epi, int32_t path, int32_t tokens_per_launch, int32_t use_graph, float *const *y);
/* ffn_gate and ffn_up (one K-quant type, IQ4_XS, TQ1_0 or TQ2_0, N rows each, N % 32 == 0) against the same T activation rows with SwiGLU in the
 * epilogue, as the prompt path launches them (mmq_planes2_swiglu_kernel): y[t][n] = silu(Wg[n] . x[t]) * (Wu[n] . x[t]).
 * Shapes too small for that launch are refused unless the debug option "mmq_tiles" = 4 forces the kernel.
 * The 32-element formats (any N, K % 32 == 0) run as a layer of such a file does: T >= 32 on the Q8_0 prompt kernel (Q8_0 tensors directly, the others with
 * "mmq_planes" 1 through their two Q8_0-layout copies) and the SwiGLU pass, else the mat-vec with SwiGLU in its epilogue.  F16: two products and the SwiGLU pass. */
MI355_API int mi355_op_ffn_gate_up(int32_t type, const void *Wg, const void *Wu, int64_t N, int64_t K, const float *x, int64_t T, float *y);
/* The adapter kernels (csrc/lora.hip) once: out[s][t][n] += scale[s] * B[s][n] . (A[s] x[t]) for n_seg = 1 .. 3 segments that share the rows x [T][K].
 * type[s]: F32 or F16 (both halves); A[s] [r][K], B[s] [N][r]; out[s] is [T][ld_out[s]], in and out - the columns beyond N[s] must come back untouched.
 * ggml's CPU arithmetic: an F16 pair rounds x, and t = A x, to f16; every sum is f32.  T <= 8 is one launch, more tokens two.
 * MI355_ERR_ARG, nothing launched: r outside 1 .. 512, K no multiple of 32, another type, ld_out < N. */
MI355_API int mi355_op_lora_delta(int32_t n_seg, const int32_t *type, const void *const *A, const void *const *B, const int32_t *r, const int64_t *N, const float *scale,
                                  const float *x, int64_t K, int64_t T, const int64_t *ld_out, float *const *out);
MI355_API int mi355_op_rms_norm_mul(const float *x, const float *w, int64_t n, int64_t T, float eps, float *y);
MI355_API int mi355_op_rope(float *x, int32_t n_head, int32_t head_dim, int32_t n_rot, const int32_t *pos, int64_t T,
                            float freq_base, float freq_scale, const float *freq_factors, int32_t neox);
/* the same rotation with YaRN scaling ({arch}.rope.scaling.type "yarn": llama.cpp's rope_yarn; ext_factor 0 and attn_factor 1 reduce it to mi355_op_rope) */
MI355_API int mi355_op_rope_yarn(float *x, int32_t n_head, int32_t head_dim, int32_t n_rot, const int32_t *pos, int64_t T,
                                 float freq_base, float freq_scale, const float *freq_factors, int32_t neox,
                                 float ext_factor, float attn_factor, float corr_lo, float corr_hi);
MI355_API int mi355_op_get_rows(int32_t type, const void *table, int64_t row_elems, int64_t n_rows_table,
                                const int32_t *ids, int64_t n_ids, float *dst);
// the upload's regrouping alone: n_rows ggml rows of row_elems elements -> n_rows * ((row bytes + 15) & ~15) bytes of device rows in dst, whose padding
// bytes hold 0xA5.  MI355_ERR_ARG for an unknown type, a row that is not a whole number of blocks, non-positive sizes.
MI355_API int mi355_op_repack_rows(int32_t type, const void *src_rows, int64_t row_elems, int64_t n_rows, void *dst);
MI355_API int mi355_op_swiglu(const float *gate, const float *up, int64_t n, float *y);
MI355_API int mi355_op_soft_max(const float *x, const float *mask, int64_t n, int64_t rows, float scale, float *y);
/* build_moe_ffn's expert selection: softmax over n_expert router logits per token, the k largest (first index wins ties), weights
   renormalised; ids [T][k], w [T][k] */
MI355_API int mi355_op_moe_route(const float *logits, int64_t T, int32_t n_expert, int32_t k, int32_t *ids, float *w);
/* build_moe_ffn's router and selection together: logits = ggml_mul_mat(ffn_gate_inp, cur) for T tokens of x [T][K] against gate_inp [n_expert][K]
   (type f32 or f16), then the selection of mi355_op_moe_route; n_expert <= 256.  fused = 1: the one launch the decode path takes; 0: the mat-vec, then the
   selection (the same bits).  forced (nullable): [T][k] expert ids to take instead (weights: their probabilities, renormalised).  logits [T][n_expert]
   (nullable), ids [T][k], w [T][k] */
MI355_API int mi355_op_moe_router(int32_t type, const void *gate_inp, int32_t n_expert, int64_t K, const float *x, int64_t T, int32_t k, int32_t fused,
                                  const int32_t *forced, float *logits, int32_t *ids, float *w);
/* ---- test entries of the kernels that produce indices: exact by construction, so their tests compare for equality.
 * Row arg-max (the token of a greedy step): x holds sum(launches) rows of n floats; ONE scratch of cap_rows * 129 words is zeroed once, then launch i takes the
 * next launches[i] rows (1 <= launches[i] <= cap_rows) - n_launch launches back to back on that scratch, no synchronisation between them.  out[row]: the
 * lowest index of the largest value; NaN entries never win; a row without a comparable entry gives 0. */
MI355_API int mi355_op_argmax_rows(const float *x, int64_t n, const int32_t *launches, int32_t n_launch, int32_t cap_rows, int32_t *out);
/* The two kernels of a speculative round (csrc/spec.hip), the arg-max rule above in both.  x [rows][n]: idx_out [rows] and p_out [rows], the arg-max's softmax
 * probability 1 / sum_j exp(x_j - max) over the non-NaN entries (f32, a fixed summation order; 0 where the maximum is not finite). */
MI355_API int mi355_op_argmax_prob_rows(const float *x, int64_t n, int32_t rows, int32_t *idx_out, float *p_out);
/* The two kernels of csrc/logprob.hip.  base [n_base_rows][n]; launch row r = base row rows[r] (rows NULL: row r), r < R <= 65535; targets [R] in [0, n).
 * logprob_out [R], rank_out [R] as mi355_get_token_logprobs gives them. */
MI355_API int mi355_op_token_logprob_rows(const float *base, int64_t n, int32_t n_base_rows, const int32_t *rows, const int32_t *targets, int32_t R,
                                          float *logprob_out, int32_t *rank_out);
/* p [n_p_rows][n], q [n_q_rows][n]; pair r = (p row rows_p[r], q row rows_q[r]) (NULL: row r).  kl_out [R], same_top_out [R] as mi355_logits_kl gives them. */
MI355_API int mi355_op_logits_kl_rows(const float *p, int32_t n_p_rows, const float *q, int32_t n_q_rows, int64_t n, const int32_t *rows_p, const int32_t *rows_q,
                                      int32_t R, float *kl_out, int32_t *same_top_out);
/* The collector launch of csrc/imatrix.hip.  x (and x2, nullable) [n_src_rows][ld] f32, ld >= K, ld a multiple of 4, K a multiple of 32; launch row r < R reads
 * source row row_src[r] (NULL: row r) and contributes v = x, or silu(x) * x2 with x2 (mi355_op_swiglu's values).  counts_per_mat [n_mat] (NULL with n_mat = 1:
 * all rows) cuts the launch rows into consecutive runs, one per matrix, and must add up to R; the entry builds the counts | offsets | total array the model's
 * grouping launch writes.  sum2_io [n_mat + 1][K]: row m += the column sums of squares of matrix m's rows, the last row is a guard that comes back as it went
 * in; count_io [n_mat] += the counts.  A matrix without rows keeps its row and count.  R <= 61440, n_mat <= 256.  MI355_ERR_ARG, and nothing launched or
 * written, for any other shape. */
MI355_API int mi355_op_imatrix_accum(const float *x, const float *x2, int64_t ld, int64_t K, int32_t R, const int32_t *row_src, int32_t n_src_rows,
                                     const int32_t *counts_per_mat, int32_t n_mat, float *sum2_io, int32_t *count_io);
/* The quantiser (csrc/quantize.hip; the counterpart of ggml_quantize_chunk).  src: n_rows rows of n_per_row elements of src_type (0 F32, 1 F16, 30 BF16), host
 * memory; dst: n_rows rows of dst_type blocks (8 Q8_0, 6 Q5_0, 7 Q5_1, 10 Q2_K, 11 Q3_K, 12 Q4_K, 13 Q5_K, 14 Q6_K), host memory; imatrix: NULL or n_per_row
 * column weights.  One upload, one launch, one synchronisation, one download; a guard row behind the output on the device is checked after the launch.
 * MI355_ERR_ARG with mi355_last_error naming the cause: an unsupported type on either side, n_per_row not a whole number of destination blocks, n_rows < 1,
 * a negative or non-finite imatrix value, a non-finite source value (the message names the first such row; dst is not written). */
MI355_API int mi355_quantize_chunk(int32_t dst_type, int32_t src_type, const void *src, int64_t n_per_row, int64_t n_rows, const float *imatrix, void *dst);
/* 1 if mi355_quantize_chunk writes dst_type, else 0.  Needs no device. */
MI355_API int mi355_quantize_supported(int32_t dst_type);
/* Milliseconds of the calling thread's last successful mi355_quantize_chunk: the upload (allocation included) and the guard check + download by the host's
 * clock, the launch between two events on its stream.  Any pointer may be NULL.  MI355_ERR_ARG before the first such call. */
MI355_API int mi355_quantize_last_times(float *upload_ms, float *kernel_ms, float *download_ms);
/* ---- the LLaVA image encoder's launches (csrc/clip.hip, csrc/mmf.hip, csrc/act.hip), one at a time: each entry uploads its inputs, issues the one launch
 * host/clip.cc issues, and downloads the result.  Half-precision outputs are raw f16 bits; every *_h output may be NULL (the launch then gets no f16 pointer).
 *
 * The tower's full attention within each of n_img images of T rows: q (pre-scaled), k, v, out [n_img][T][H * D].  *path: the kernel launch_clip_attn's choice
 * function names for (T, D) under MI355_CLIP_ATTN_TILED / MI355_CLIP_ATTN_MFMA: 1 f32 matrix cores, 2 LDS-tiled, 3 one wave per query, 0 refused - then
 * MI355_ERR_ARG and nothing is launched (no kernel for the head size, or T past the kernel's LDS). */
MI355_API int mi355_op_clip_attn(const float *q, const float *k, const float *v, int64_t T, int32_t H, int32_t D, int32_t n_img, float *out, uint16_t *out_h,
                                 int32_t *path);
/* y = resid + (W . f16(x) + bias) * scale against an f16 tensor W [N][K] (bits), x [T][K]; bias [N], the scale (do_scale) and resid [T][ld_out] each optional.
 * y_io [T][ld_out], ld_out >= N: uploaded before the launch and read back whole, so the columns past N must come back as they went in.  in_place 1: y_io holds
 * the residual rows on entry and the launch gets the one device buffer as resid and y (resid must be NULL).
 * form 0: launch_f32_to_f16, then launch_mmf16_xh with the epilogue fused (MI355_MMF16_LDS=0: the direct kernel; MI355_MMF16_TILE=128: its large tile);
 * form 1: the unfused chain launch_mmf16, launch_clip_bias, launch_add (ld_out == N; a scale only with a bias, as host/clip.cc has it).
 * K % 16 != 0: the launchers refuse (MI355_ERR_HIP) before any matrix launch. */
MI355_API int mi355_op_mul_mat_f16_xh(const uint16_t *W, int64_t N, int64_t K, const float *x, int64_t T, int64_t ld_out, const float *bias, float scale,
                                      int32_t do_scale, const float *resid, int32_t in_place, int32_t form, float *y_io);
/* LayerNorm with weight and bias over T rows of n; in_place 1: the launch reads and writes one device buffer. */
MI355_API int mi355_op_layer_norm(const float *x, const float *w, const float *b, int64_t n, int64_t T, float eps, int32_t in_place, float *y, uint16_t *y_h);
/* ggml's f16-table GELU (quick 0) / quick-GELU (quick 1) of n values */
MI355_API int mi355_op_clip_gelu(const float *x, int64_t n, int32_t quick, float *y, uint16_t *y_h);
/* img [3][S][S] -> patches_io [(S / P)^2][ld], ld >= 3 P P: uploaded first and read back whole (the launch writes every column, zeros past 3 P P) */
MI355_API int mi355_op_clip_im2col(const float *img, int32_t S, int32_t P, int32_t ld, float *patches_io);
/* emb [T][E]: row 0 = cls + pos[0], row t = patch[t - 1] + pos[t]; patch [T - 1][E], pos [T][E] */
MI355_API int mi355_op_clip_embed(const float *patch, const float *cls, const float *pos, int32_t E, int32_t T, float *emb);
/* x_io [T][n] = (x + b) [* scale] */
MI355_API int mi355_op_clip_bias(float *x_io, const float *b, int32_t n, int32_t T, float scale, int32_t do_scale);
/* round-to-nearest-even f32 -> f16 bits, n % 4 == 0 */
MI355_API int mi355_op_f32_to_f16(const float *x, int64_t n, uint16_t *out);
/* q_io [T][nq] += bq, k_io / v_io [T][nkv] += bk / bv in one launch; a NULL bias skips its segment (its rows may then be NULL too) */
MI355_API int mi355_op_add_qkv_bias(float *q_io, float *k_io, float *v_io, const float *bq, const float *bk, const float *bv, int32_t nq, int32_t nkv, int32_t T);
/* the control vector's row-broadcast add (csrc/cvec.hip launch_add_row_vec): y [T + 1][E]; rows 0 .. T - 1 = x[t] + v, row T = the guard row that lay behind
 * them on the device, every byte 0xA5 if the launch stayed inside its rows */
MI355_API int mi355_op_add_row_vec(const float *x, const float *v, int32_t E, int32_t T, float *y);
/* logits [n_base_rows][n]; launch row r = base row rows[r], r < R <= 1088; group g < G <= 64 owns launch rows group_start[g] .. group_start[g + 1] - 1
 * (1 .. 17 rows; group_start[0] = 0, group_start[G] = R); draft [R].  ids_out [R], n_accept_out [G] as mi355_spec_verify gives them. */
MI355_API int mi355_op_spec_verify(const float *logits, int64_t n, int32_t n_base_rows, const int32_t *rows, int32_t R, const int32_t *group_start, int32_t G,
                                   const int32_t *draft, int32_t *ids_out, int32_t *n_accept_out);
/* The k best candidates of n_rows logits rows (the front end of a sampled step): row r is base row rows[r] ([n_base_rows][n] f32) after its adjustments -
 * adj_n[r] entries (0 .. 192) of the flat [n_rows][192] arrays adj_tok / adj_bias / adj_cnt, no token twice in a row's list: l = l + bias; if cnt > 0:
 * l = l <= 0 ? l * repeat[r] : l / repeat[r]; l -= cnt * freq[r] + present[r].  Order: higher logit first, lower token id among equal logits (-0.0 == +0.0).
 * keys_out [n_rows][k], k <= min(n, 128): (order-preserving image of the f32 logit) << 32 | (0xffffffff - token).  No NaN inputs. */
MI355_API int mi355_op_topk_rows(const float *base, int64_t n, int32_t n_base_rows, const int32_t *rows, int32_t n_rows, int32_t k, const int32_t *adj_n,
                                 const int32_t *adj_tok, const float *adj_bias, const int32_t *adj_cnt, const float *repeat, const float *freq,
                                 const float *present, uint64_t *keys_out);
/* Grouping of the T * k selections ids [T][k] of a prompt batch by expert (T * k <= 61440, n_expert <= 256): a counting sort, stable in (token, rank) order.
 * meta [2 * n_expert + 1]: counts | exclusive offsets | total; slot_of [T * k]: grouped row of pair t * k + j; tok_of [T * k]: token of a grouped row. */
MI355_API int mi355_op_moe_group(const int32_t *ids, int64_t T, int32_t k, int32_t n_expert, int32_t *meta, int32_t *slot_of, int32_t *tok_of);
/* grouped row r = activation row tok_of[r], plane by plane: the Q8_K triple (qs [T][K] | d [T][K / 256] | bsums [T][K / 16]) and / or the Q8_0 pair (qs0 [T][K]
 * | d0 [T][K / 32]); the planes of a form that is not wanted are NULL, in and out.  K % 256 == 0.  Every output plane holds n_rows + 1 rows: it is uploaded
 * before the launch and read back whole, so the last row is a guard that must come back as it went in. */
MI355_API int mi355_op_moe_gather_act(const int8_t *qs, const float *d, const int16_t *bsums, const int8_t *qs0, const uint16_t *d0, int64_t T, int64_t K,
                                      const int32_t *tok_of, int64_t n_rows, int8_t *qs_out, float *d_out, int16_t *bsums_out, int8_t *qs0_out,
                                      uint16_t *d0_out);
/* y = x + sum_j eo_j * w[t][j] (x [T][E], w [T][k]; the ranks added in order, then the residual).  grouped = 0: eo [k][T][E]; grouped = 1: eo [T * k][E] in
 * grouped rows, rank j of token t at row slot_of[t * k + j]. */
MI355_API int mi355_op_moe_combine(const float *x, const float *eo, const float *w, int64_t T, int32_t E, int32_t k, int32_t grouped, const int32_t *slot_of,
                                   float *y_out);
/* Test hook: ONE grouped-expert launch of a prompt batch (ggml_mul_mat_id over rows sorted by expert), issued as the model issues it.
 *   form 0: the plane sets, one projection (ffn_down):          y0[r][n] = W0[e(r)][n] . a[r]
 *   form 1: the plane sets, ffn_gate | ffn_up with SwiGLU:      y0[r][n] = silu(W0[e(r)][n] . a[r]) * (W1[e(r)][n] . a[r])
 *   form 2 / 3: the Q8_0-layout copies, one / two segments:     y0 as form 0, and y1 the same over W1
 * W0 / W1: n_expert tensors back to back in GGUF row layout, [n_expert][N][row bytes]; x [R][K] f32, the grouped rows; counts[n_expert] rows per expert in
 * expert order, R their sum (expert e owns rows [sum of counts before e, + counts[e])).  The entry repacks the rows, expands every expert at the loader's
 * stride, quantises x (Q8_K for the plane forms, Q8_0 for the copies), builds meta (counts | exclusive offsets | total) and makes the launch with rows_max = R;
 * the copy forms take the tile "mmq_q80_tiles" forces, else the launcher's choice.  Every out buffer is [R + guard_rows][ld_out] (ld_out >= N), filled with
 * 0xFF bytes before the launch and returned whole: an unwritten result reads as NaN, a write past N or past row R shows in the pad columns / guard rows.
 * MI355_ERR_ARG, nothing launched: a shape the launch's own predicate refuses (planes: Q4_K / Q5_K / Q6_K / IQ4_XS / TQ1_0 / TQ2_0, N % 128 == 0,
 * K % 256 == 0; copies: MXFP4, N % 128 == 0, K % 32 == 0, K <= 16384), n_expert outside 1 .. 256, a negative count, counts that do not add up to R. */
MI355_API int mi355_op_moe_mul_mat_grouped(int32_t type, int32_t form, const void *W0, const void *W1, int32_t n_expert, int64_t N, int64_t K, const float *x,
                                           const int32_t *counts, int64_t R, int64_t ld_out, int64_t guard_rows, float *y0, float *y1);
/* dst [n_rows][n] = src [n_src_rows][n] rows rows[0 .. n_rows) (the output rows handed to the head) */
MI355_API int mi355_op_gather_rows_f32(const float *src, int64_t n_src_rows, int64_t n, const int32_t *rows, int64_t n_rows, float *dst);
/* flash_attn_ext for T query tokens: K/V given as ggml-layout rows [n_cells][n_head_kv*head_dim] of type_k/type_v;
 * visibility: cell c is visible to token t iff cell_pos[c] >= 0 && cell_pos[c] <= q_pos[t]. */
MI355_API int mi355_op_flash_attn(const float *q, int64_t T, int32_t n_head, int32_t n_head_kv, int32_t head_dim,
                                  int32_t type_k, const void *k, int32_t type_v, const void *v, int32_t n_cells,
                                  const int32_t *cell_pos, const int32_t *q_pos, float scale, float *out);

/* The attention block of ONE single-token step as the decode path launches it (rope of q and of the token's K row, the K / V row quantised into the cache,
 * flash_attn_ext over the visible cells, Q8_K quantisation, the attn_output mat-vec + residual: the ops between two llama_decode graph nodes of
 * llm_build_llama that attn_out.hip runs as one launch; reached through llama_decode, src/llama_server_context.cc:1635).  fused = 1: the one-launch form,
 * 0: the single-launch decode attention followed by the weight-stream mat-vec.  k / v: the cache before the step as ggml-layout rows [n_cells][n_head_kv *
 * head_dim]; cell_pos[tok_cell] must already hold tok_pos.  att_out [n_head * head_dim], out [n_embd], k_row_out / v_row_out: the cache row the step wrote,
 * in ggml block layout (any of the four may be NULL). */
MI355_API int mi355_op_attn_step(const float *q, const float *k_new, const float *v_new, int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t type_k,
                                 const void *k, int32_t type_v, const void *v, int32_t n_cells, const int32_t *cell_pos, int32_t tok_pos, int32_t tok_cell,
                                 float rope_base, int32_t n_rot, float scale, int32_t type_o, const void *W_o, int64_t n_embd, const float *resid, int32_t fused,
                                 float *att_out, float *out, void *k_row_out, void *v_row_out);
/* The decode attention of ONE token of a qwen2 / qwen3 file (NEOX rope pairing, head_dim 64 or 128, the whole head rotated): q_norm / k_norm ([head_dim] f32,
 * either may be NULL = no norm) RMS-normalise every query head / the token's kv heads over their own head_dim values (eps) and multiply by the weight BEFORE the
 * rope, as llm_build_qwen3 orders it; then the K / V row is quantised into the cache and the token attends over the visible cells.  q, k_new, v_new are
 * un-rotated.  mode 1: the single-launch form of a single-token step; 0: the store-fused form of a batched step; 2: the generic path of prompt batches
 * (rope_kv_store + split attention).  k / v, cell_pos, att_out, k_row_out / v_row_out as mi355_op_attn_step. */
MI355_API int mi355_op_attn_decode_neox(const float *q, const float *k_new, const float *v_new, int32_t n_head, int32_t n_head_kv, int32_t head_dim,
                                        int32_t type_k, const void *k, int32_t type_v, const void *v, int32_t n_cells, const int32_t *cell_pos, int32_t tok_pos,
                                        int32_t tok_cell, float rope_base, float scale, const float *q_norm, const float *k_norm, float eps, int32_t mode,
                                        float *att_out, void *k_row_out, void *v_row_out);
/* The K / V cache write of a batch of T tokens on its own (test entry): q [T][n_head * head_dim] is rotated in place, k [T][n_head_kv * head_dim] is rotated
 * and quantised into k_cache at tok_cell[t], v is quantised into v_cache.  k_cache / v_cache: the whole cache as ggml-layout rows [n_cells][n_head_kv *
 * head_dim] of type_k / type_v, read before the launch and written back whole after it (cells outside tok_cell come back as they went in; tok_cell distinct).
 * form 0: the generic kernel, angles computed from tok_pos inside it; 1: the same kernel on the cos / sin table of the batch; 2: the vectorised prompt store
 * (q, k and v); 3: the small-batch decode store (k and v only; q may be NULL and is not touched).  Forms 2 and 3 take NORM rope, f16 / q8_0 caches, no q / k
 * norm and n_head_kv * head_dim % 1024 == 0 (form 2: n_head * head_dim % 1024 == 0 too): MI355_ERR_ARG otherwise, nothing is launched.  freq_factors
 * [n_rot / 2] and q_norm / k_norm [head_dim] (qwen3: n_rot == head_dim, 64 or 128) may be NULL. */
MI355_API int mi355_op_kv_store(int32_t form, float *q, const float *k, const float *v, int64_t T, int32_t n_head, int32_t n_head_kv, int32_t head_dim,
                                int32_t n_rot, int32_t neox, int32_t type_k, int32_t type_v, int32_t n_cells, const int32_t *tok_pos, const int32_t *tok_cell,
                                float rope_base, float freq_scale, const float *freq_factors, const float *q_norm, const float *k_norm, float eps,
                                void *k_cache, void *v_cache);
/* The three attention entries above with more than one sequence in the cache (test entries).  cell_seq [n_cells]: the cells' sequence bit masks (uint64, bit s =
 * sequence s); q_seq [T] / tok_seq: the query's sequence, 0 .. 63 (MI355_ERR_ARG outside).  A query sees cell c iff c < n_kv, cell_pos[c] >= 0, cell_pos[c] <=
 * its position and bit q_seq of cell_seq[c] is set.  mi355_op_flash_attn_seq: n_kv (1 .. n_cells) is the cell count the kernels read from the device, while
 * the grid, the splits and the workspace are sized for n_cells.  mi355_op_flash_attn is this call with masks of 1, sequence 0 and n_kv = n_cells.
 * mi355_op_attn_step_seq / mi355_op_attn_decode_neox_seq: cell_seq may be NULL (every cell in sequence 0); use_lists != 0 gives the launch the token's
 * chunk list - the 64-cell chunks that hold a cell of its sequence - as a context with several sequences does (not with mode 2 of the NEOX entry). */
MI355_API int mi355_op_flash_attn_seq(const float *q, int64_t T, int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t type_k, const void *k, int32_t type_v,
                                      const void *v, int32_t n_cells, const int32_t *cell_pos, const uint64_t *cell_seq, const int32_t *q_pos, const int32_t *q_seq,
                                      int32_t n_kv, float scale, float *out);
/* out[0]: the key splits the split kernel would run such a call with, out[1]: those of the matrix-core prompt kernel, out[2]: 1 where the prompt kernel takes it. */
MI355_API int mi355_op_flash_attn_plan(int64_t T, int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t type_k, int32_t type_v, int32_t n_cells, int32_t *out);
MI355_API int mi355_op_attn_step_seq(const float *q, const float *k_new, const float *v_new, int32_t n_head, int32_t n_head_kv, int32_t head_dim, int32_t type_k,
                                     const void *k, int32_t type_v, const void *v, int32_t n_cells, const int32_t *cell_pos, const uint64_t *cell_seq, int32_t tok_pos,
                                     int32_t tok_seq, int32_t tok_cell, int32_t use_lists, float rope_base, int32_t n_rot, float scale, int32_t type_o, const void *W_o,
                                     int64_t n_embd, const float *resid, int32_t fused, float *att_out, float *out, void *k_row_out, void *v_row_out);
MI355_API int mi355_op_attn_decode_neox_seq(const float *q, const float *k_new, const float *v_new, int32_t n_head, int32_t n_head_kv, int32_t head_dim,
                                            int32_t type_k, const void *k, int32_t type_v, const void *v, int32_t n_cells, const int32_t *cell_pos,
                                            const uint64_t *cell_seq, int32_t tok_pos, int32_t tok_seq, int32_t tok_cell, int32_t use_lists, float rope_base,
                                            float scale, const float *q_norm, const float *k_norm, float eps, int32_t mode, float *att_out, void *k_row_out,
                                            void *v_row_out);
/* The attention of ONE batched single-token step of T <= 64 tokens (test entry): q [T][n_head * head_dim] un-rotated, k_new / v_new [T][n_head_kv * head_dim];
 * k_cache / v_cache: the whole cache as ggml-layout rows, read before and written back whole after the step; cell_pos / cell_seq with the new cells already
 * set; n_kv: cells to scan (tok_cell < n_kv <= n_cells).  mode 0: K rope and the K / V store inside the attention launch, every chunk scanned; 1: the same on
 * per-token chunk lists; 2: the small-batch store, then the attention without the store, on the lists; 3: the generic store + attention.  att_out [T][n_head *
 * head_dim]; q8k_out (may be NULL): the ggml block_q8_K rows the merge wrote for attn_output.  MI355_ERR_ARG, and nothing launched, for a shape or mode
 * without a kernel: T > 64, tokens that share a sequence or sit in several (modes 0 and 1), a cache type, head geometry or rope the decode attention (modes
 * 0 - 2) or the small-batch store (modes 1 and 2) does not take. */
MI355_API int mi355_op_attn_batch_step(const float *q, const float *k_new, const float *v_new, int64_t T, int32_t n_head, int32_t n_head_kv, int32_t head_dim,
                                       int32_t type_k, void *k_cache, int32_t type_v, void *v_cache, int32_t n_cells, int32_t n_kv, const int32_t *cell_pos,
                                       const uint64_t *cell_seq, const int32_t *tok_pos, const int32_t *tok_seq, const int32_t *tok_cell, float rope_base,
                                       int32_t n_rot, int32_t neox, float scale, int32_t mode, float *att_out, void *q8k_out);
/* The same step, which mi355_op_attn_batch_step forwards to, with the merge also writing the block sums of its Q8_K rows as the bh / bl planes of the MFMA
 * kernels, as the model has it do for a K-quant attn_output: bh_out / bl_out (both or neither; they need q8k_out) [T][n_head * head_dim / 16] int8 each,
 * 0xFF bytes before the launch. */
MI355_API int mi355_op_attn_batch_step_planes(const float *q, const float *k_new, const float *v_new, int64_t T, int32_t n_head, int32_t n_head_kv, int32_t head_dim,
                                              int32_t type_k, void *k_cache, int32_t type_v, void *v_cache, int32_t n_cells, int32_t n_kv, const int32_t *cell_pos,
                                              const uint64_t *cell_seq, const int32_t *tok_pos, const int32_t *tok_seq, const int32_t *tok_cell, float rope_base,
                                              int32_t n_rot, int32_t neox, float scale, int32_t mode, float *att_out, void *q8k_out, int8_t *bh_out, int8_t *bl_out);
/* The K-shift of llama_kv_cache_seq_add on its own (test entry): every row of k_cache (layout as above) whose delta[cell] != 0 is dequantised, rotated by
 * delta[cell] positions and quantised again, in one launch; rows with delta 0 are not touched.  The YaRN parameters as mi355_op_rope_yarn takes them. */
MI355_API int mi355_op_k_shift(int32_t type_k, int32_t n_head_kv, int32_t head_dim, int32_t n_rot, int32_t neox, int32_t n_cells, const int32_t *delta,
                               float rope_base, float freq_scale, const float *freq_factors, float ext_factor, float attn_factor, float corr_lo,
                               float corr_hi, void *k_cache);
/* The two kernels behind mi355_state_seq_get_data / set_data on their own (test entries): a cache of n_layer layers, each given as ggml-layout rows
 * k_rows[layer] / v_rows[layer] [n_cells][n_head_kv * head_dim] (layout as above) and uploaded into device planes; cells: n indices in [0, n_cells).
 * pack: out receives, per layer, the K rows of the listed cells in list order and then their V rows - the row section of a state blob.
 * unpack: the rows `in` (that layout) are written into the listed cells (all different) and the whole cache comes back in k_rows / v_rows. */
MI355_API int mi355_op_kv_state_pack(int32_t type_k, int32_t type_v, int32_t n_layer, int32_t n_head_kv, int32_t head_dim, int32_t n_cells,
                                     const void *const *k_rows, const void *const *v_rows, const int32_t *cells, int32_t n, void *out);
MI355_API int mi355_op_kv_state_unpack(int32_t type_k, int32_t type_v, int32_t n_layer, int32_t n_head_kv, int32_t head_dim, int32_t n_cells, const void *in,
                                       const int32_t *cells, int32_t n, void *const *k_rows, void *const *v_rows);

/* ------------------------------------------------------------------ tokenizer
 * llama_tokenize / llama_token_to_piece as reached through common_tokenize / common_token_to_piece
 * (src/llama_server_context.cc:395-410, 536, 644, 720, 936, 992) and llama_vocab_bos/eos/is_eog (:512-517, 792).
 * mi355_tokenize returns the token count, or -(count needed) when `cap` is too small. */
MI355_API int32_t mi355_tokenize(mi355_model *m, const char *text, int32_t text_len, mi355_token *out, int32_t cap,
                                 int32_t add_special, int32_t parse_special);
MI355_API int32_t mi355_token_to_piece(mi355_model *m, mi355_token tok, char *buf, int32_t cap, int32_t special);
MI355_API mi355_token mi355_token_bos(mi355_model *m);
MI355_API mi355_token mi355_token_eos(mi355_model *m);
MI355_API int32_t mi355_token_is_eog(mi355_model *m, mi355_token tok);

/* ------------------------------------------------------------------ engine (the reference's plugin surface)
 * class EngineI (base/cortex-common/enginei.h:13-74) as implemented by LlamaEngine (src/llama_engine.cc): the slot
 * loop, sampler and request/response shaping run in the host library; bodies cross the boundary as UTF-8 JSON text
 * instead of std::shared_ptr<Json::Value>.  The callback receives (status, body) exactly as the reference's
 * std::function<void(Json::Value&&, Json::Value&&)> does: status = {is_done, has_error, is_stream, status_code};
 * streaming completions call it once per chunk (body = {"data": "data: {...}\n\n"}) from a worker thread. */
typedef struct mi355_engine mi355_engine;
typedef void (*mi355_engine_callback)(const char *status_json, const char *body_json, void *user);
MI355_API mi355_engine *mi355_engine_create(void);                 /* get_engine()  (src/llama_engine.cc:1300-1304) */
MI355_API void mi355_engine_destroy(mi355_engine *e);
/* Lifetime of `user`: the reference's callback is a std::function that dies with the request (it is captured by value in the queued task,
   src/llama_engine.cc:946-948); a C callback has no destructor, so a host that allocates per-request state registers one function here and the library calls
   it exactly once per request with that request's `user`, after the LAST callback the request will ever make - also when the request ends without a terminal
   (is_done / has_error) callback, as a stream stopped by StopInferencing does (:950-955).  Set it before the first request; NULL (default) = nothing is called. */
MI355_API void mi355_engine_set_release_callback(mi355_engine *e, void (*release)(void *user));
MI355_API void mi355_engine_load_model(mi355_engine *e, const char *body_json, mi355_engine_callback cb, void *user);
MI355_API void mi355_engine_unload_model(mi355_engine *e, const char *body_json, mi355_engine_callback cb, void *user);
MI355_API void mi355_engine_get_model_status(mi355_engine *e, const char *body_json, mi355_engine_callback cb, void *user);
MI355_API void mi355_engine_get_models(mi355_engine *e, const char *body_json, mi355_engine_callback cb, void *user);
MI355_API void mi355_engine_handle_chat_completion(mi355_engine *e, const char *body_json, mi355_engine_callback cb, void *user);
MI355_API void mi355_engine_handle_embedding(mi355_engine *e, const char *body_json, mi355_engine_callback cb, void *user);
MI355_API int32_t mi355_engine_is_supported(mi355_engine *e, const char *feature);
MI355_API void mi355_engine_stop_inferencing(mi355_engine *e, const char *model_id);
/* The host-RAM prompt cache of a model loaded with "cache_ram": N (MiB of host memory; 0 / absent = off, negative = no limit; upstream's --cache-ram): KV states of
   conversations that lost their slot, restored when their prompt comes back.  out: entries, bytes held, saves, restores, tokens restored, evictions - all zero
   while the cache is off.  < 0: no such model. */
MI355_API int mi355_engine_prompt_cache_stats(mi355_engine *e, const char *model_id, int64_t out[6]);
/* Speculative decoding of a model loaded with "model_draft": PATH (a draft model of the same vocabulary; "draft_max" 1 .. 16, default 16; "draft_min", default 0;
   "draft_p_min", default 0.75): requests without a grammar, n_probs or images take the draft model's proposals and check them in one batched step.  out, as
   mi355_speculative_steps counts them: rounds (ticks of a speculating slot), drafted, accepted (drafts that were emitted), plain steps (rounds without a drafted
   token) - all zero without a draft model.  < 0: no such model. */
MI355_API int mi355_engine_spec_stats(mi355_engine *e, const char *model_id, int64_t out[4]);
/* EngineI::Load(EngineLoadOption) / Unload(EngineUnloadOption) (base/cortex-common/enginei.h:14-35; LlamaEngine: src/llama_engine.cc:289-303): Load =
   SetFileLogger(max_log_lines, log_path) + SetLogLevel(log_level).  Paths as UTF-8 strings (std::filesystem::path::string()), log_level = the value of
   trantor::Logger::LogLevel (kTrace 0, kDebug 1, kInfo 2, kWarn 3, kError 4, kFatal 5). */
MI355_API void mi355_engine_load(mi355_engine *e, const char *engine_path, const char *deps_path, int32_t is_custom_engine_path, const char *log_path,
                                 int32_t max_log_lines, int32_t log_level);
MI355_API void mi355_engine_unload(mi355_engine *e);
/* EngineI::SetFileLogger / SetLogLevel (enginei.h:69-71; src/llama_engine.cc:502-548): log lines go to log_path, kept to its last max_log_lines lines
   ("" = back to stderr); messages below log_level are dropped */
MI355_API void mi355_engine_set_file_logger(mi355_engine *e, int32_t max_log_lines, const char *log_path);
MI355_API void mi355_engine_set_log_level(mi355_engine *e, int32_t log_level);
/* the bridge the other way: every log line also goes to cb (level = trantor's numbers), so an adapter can re-emit it through the host's own LOG_* macros
   (the reference routes llama.cpp's log through trantor the same way: llama_log_set, src/llama_engine.cc:313-330).  Process-wide, like trantor::Logger. */
typedef void (*mi355_log_callback)(int level, const char *line, void *user);
MI355_API void mi355_engine_set_log_callback(mi355_engine *e, mi355_log_callback cb, void *user);

/* Test / tool switches of the per-op entry points: "mmq_planes" (1: mi355_op_mul_mat with T >= 32 expands the weight
 * into MFMA planes first, as a loaded model does; 0: expands on the fly inside the kernel - Q2_K / Q3_K / IQ4_XS / TQ1_0 / TQ2_0 have
 * no on-the-fly form and take the mat-vec then), "mmq_tiles" (0 | 1 | 2
 * token tiles per wave), "mmq_q80_tiles" (test hook: 0 | 1 | 2 | 4 token tiles per wave of the Q8_0 prompt kernel whatever the shape; every form gives the same bits), "mmq_ksplit" (1: 8 <= T <= 64 uses the K-split small-batch kernel, as the runtime does; 0: the
 * kernels the other T ranges use); and of contexts created afterwards: "decode_mega" (1: single-token steps of a dense
 * K-quant model with Llama-3-8B's layer geometry run every layer in one launch; 0, the default: one launch per operation
 * — both produce the same bits; the single launch measured slower); "moe_group_min" (batches of at least
 * this many tokens run a mixture-of-experts feed-forward grouped by expert, default 8; smaller ones loop over (token,
 * expert) with the mat-vec); "moe_q80_grouped" (1, the default: a prompt batch of a file with MXFP4 expert tensors runs every
 * expert's batch of a projection in one launch; 0: one launch per expert after a host synchronisation - the same bits);
 * "tp_null_group" (measurement aid: the process becomes rank 0 of a row-split group of `value`
 * ranks whose other members do not exist — every exchange is a device copy of this rank's own part, so a model loaded with
 * tp_rank 0 / tp_size value times ONE rank's compute without communication; its outputs are not the model's).
 * Returns MI355_OK or MI355_ERR_ARG for an unknown name. */
MI355_API int mi355_debug_set_option(const char *name, int32_t value);

/* ------------------------------------------------------------------ row split across GPUs (one process per GPU)
 * Not in the reference: cortex.llamacpp never sets llama.cpp's split_mode / tensor_split (llama_engine.cc:553-658
 * writes no such field), so every visible GPU gets whole layers.  Here a model loaded with tp_size > 1 holds rank tp_rank's
 * rows of attn_q/k/v, ffn_gate/up and output and the matching columns of attn_output / ffn_down; the partial sums of those
 * two are summed across the ranks (RCCL all-reduce over xGMI on the context's stream, inside its graphs), the logits slices
 * are gathered.  Every rank must issue the same mi355_decode calls.  Order: mi355_tp_unique_id on rank 0 -> hand the 128
 * bytes to the other ranks (any side channel) -> mi355_tp_init on every rank (after selecting its device with
 * main_gpu / HIP_VISIBLE_DEVICES) -> mi355_model_load_from_file with the same tp_rank / tp_size. */
#define MI355_TP_ID_BYTES 128
MI355_API int mi355_tp_unique_id(void *id_out, size_t cap);                         /* returns bytes written or < 0 */
MI355_API int mi355_tp_init(int32_t device, int32_t rank, int32_t size, const void *id, size_t id_len);
MI355_API void mi355_tp_shutdown(void);
/* ONE /loadmodel for the row split (what a user of the reference sees: its engine drives every visible device from one call, src/llama_engine.cc:609-611).
 * A load body with "split_mode": "row" (+ "tensor_split": even shares only, "main_gpu", "split_ranks": see host/tp_split.cc) given to
 * mi355_engine_load_model makes the calling process rank 0 of a group it forms itself: it starts bin/mi355_tp_worker once per further rank, hands it the RCCL id
 * (or, where ranks share a device, a shared-memory exchange segment) over a socket pair, and steps the workers in lock-step with every batch and KV operation.
 * None of the calls above is needed then.  mi355_tp_worker_main is that worker program's body: `sock_fd` is the inherited socket; returns the exit code. */
MI355_API int mi355_tp_worker_main(int sock_fd);
MI355_API int32_t mi355_tp_rank(void);
MI355_API int32_t mi355_tp_size(void);
/* Validation transport for boxes where the ranks share one GPU (RCCL refuses that): the exchange goes through this
 * host callback instead (op 0: sum `n` floats in place over the ranks; op 1: all-gather, `n` floats per rank, the caller's
 * part already at buf + rank * n).  Graphs are off while it is set.  fn == NULL removes it. */
/* One-shot peer-to-peer all-reduce for the decode-sized exchanges (host/tp_comm.h): after mi355_tp_init (or _set_host_exchange) every
 * rank calls mi355_tp_p2p_local_handle (64 bytes out; max_floats = the largest message it should take, e.g. n_embd * 8), the handles are gathered
 * rank-major over the side channel that carried the RCCL id, and every rank calls mi355_tp_p2p_enable with all of them.  All-reduces of up to max_floats
 * floats then run as one peer-to-peer kernel (IPC-mapped buffers, xGMI peer stores, rank-order sum); larger ones keep the base transport. */
#define MI355_TP_P2P_HANDLE_BYTES 64
MI355_API int mi355_tp_p2p_local_handle(void *out, size_t cap, size_t max_floats);   /* returns bytes written or < 0 */
MI355_API int mi355_tp_p2p_enable(const void *handles, size_t len);
MI355_API int64_t mi355_tp_p2p_exchanges(void);                                      /* diagnosis: all-reduces that took the peer-to-peer kernel */
/* The same bootstrap with a second size: all-reduces of (max_floats, prompt_floats] floats - the n_embd x n_ubatch partial sums of a prompt batch - run
 * as ONE reduce-scatter + all-gather kernel over all xGMI links at once (host/tp_comm.cc p2p_rsag_kernel: the message is cut into one segment per rank,
 * every rank stores its part of segment q into rank q's buffer, the owner adds the parts in rank order and stores the sum into everybody's buffer).  A
 * ring all-reduce keeps one link direction per rank busy; the reference has no counterpart (it copies activations between peers,
 * SURVEY.md §8e).  Option "tp_p2p_prompt" = 0 (mi355_debug_set_option) routes these messages back to RCCL. */
MI355_API int mi355_tp_p2p_local_handle2(void *out, size_t cap, size_t max_floats, size_t prompt_floats);
MI355_API int64_t mi355_tp_p2p_prompt_exchanges(void);                               /* diagnosis: all-reduces that took the reduce-scatter + all-gather kernel */
typedef int (*mi355_tp_host_exchange)(void *user, float *buf, size_t n, int32_t op);
MI355_API int mi355_tp_set_host_exchange(mi355_tp_host_exchange fn, void *user, int32_t rank, int32_t size);

/* ------------------------------------------------------------------ measurement hooks (bench.py) */
/* Streams `bytes` through a read-only reduction kernel `iters` times; returns achieved GB/s (HIP events). */
MI355_API double mi355_bench_hbm_read(size_t bytes, int iters);
/* Per-kernel-class device time of the LAST decode call in microseconds, measured with HIP events on the
 * context's stream (eager mode only).  names/us arrays of capacity cap; returns count. */
MI355_API int32_t mi355_profile_last_decode(mi355_context *ctx, const char **names, float *us, int32_t cap);
MI355_API void    mi355_profile_enable(mi355_context *ctx, int32_t enabled);
/* Runs the dominant decode kernel (quantised mat-vec over every weight tensor of the model, one token)
 * `iters` times on the context's stream, timed with HIP events; returns mean microseconds per sweep and
 * writes the algorithmic bytes of one sweep. */
/* test hook for mixture-of-experts files (build_moe_ffn's top-k): the NEXT mi355_decode call (one micro-batch of n_tokens tokens) takes the
 * experts ids[layer][token][rank] instead of its own router's selection (the weights stay this side's router probabilities of those experts, renormalised).
 * Parity tests hand over the CPU restatement's selection so that a rounding flip on a near tie of the router cannot send a token to another expert on one
 * side only.  Arms one call. */
MI355_API int     mi355_debug_force_moe_ids(mi355_context *ctx, const int32_t *ids, int32_t n_layer, int32_t n_tokens, int32_t k);
MI355_API double  mi355_bench_weight_sweep(mi355_context *ctx, int iters, uint64_t *bytes_per_sweep);
/* ... and the number of mat-vec launches the sweep holds (the step's own launches of the weight-stream kernel: where attn_output runs inside the attention
 * launch - attn_out.hip - it is not among them, and its bytes are not counted) */
MI355_API double  mi355_bench_weight_sweep2(mi355_context *ctx, int iters, uint64_t *bytes_per_sweep, int32_t *launches_per_sweep);

/* ------------------------------------------------------------------ LLaVA image path (projector file "mmproj"; llama.cpp examples/llava behind the reference)
 * The reference: clip_model_load (llama_server_context.cc:187), clip_n_mmproj_embd (:217), clip_image_load_from_bytes (:568),
 * llava_image_embed_make_with_clip_img (:820, = clip_image_preprocess + clip_image_encode); the rows then enter the model as llama_batch.embd (:1093-1107).
 * LLaVA-1.5 and LLaVA-1.6 style files (CLIP ViT tower, MLP projector, f16 weights; LLaVA-1.6 = clip.vision.image_grid_pinpoints with
 * clip.vision.mm_patch_merge_type "spatial_unpad": a picture becomes an overview plus the tiles of the best-fitting canvas). */
typedef struct mi355_clip mi355_clip;
MI355_API mi355_clip *mi355_clip_model_load(const char *path, int32_t main_gpu);       /* clip_model_load; NULL + mi355_last_error on failure */
MI355_API void        mi355_clip_free(mi355_clip *clip);                                /* clip_free */
MI355_API int32_t     mi355_clip_n_mmproj_embd(const mi355_clip *clip);                 /* clip_n_mmproj_embd: must equal the model's n_embd */
MI355_API int32_t     mi355_clip_n_patches(const mi355_clip *clip);                     /* clip_n_patches: embedding rows per image */
MI355_API int32_t     mi355_clip_image_size(const mi355_clip *clip);
/* the most rows mi355_llava_image_embed_from_bytes can write for one picture: n_patches (LLaVA-1.5) or n_patches * (1 + tiles of the largest canvas) */
MI355_API int32_t     mi355_clip_max_image_rows(const mi355_clip *clip);
/* clip_image_load_from_bytes: PNG / JPEG (Huffman-coded sequential or progressive) / BMP / binary PNM bytes -> 8-bit RGB [ny][nx][3].  rgb_out may be NULL to query the size.
 * Returns 0, or < 0 with the reason in mi355_last_error (unknown format, truncated data, rgb_cap too small). */
MI355_API int32_t     mi355_clip_image_load_from_bytes(const uint8_t *bytes, size_t n_bytes, int32_t *nx, int32_t *ny, uint8_t *rgb_out, size_t rgb_cap);
/* clip_image_preprocess (LLaVA-1.5: pad to a square with the mean colour, bilinear resample, normalise): rgb [ny][nx][3] -> out [3][S][S], S = image_size */
MI355_API int32_t     mi355_clip_image_preprocess(const mi355_clip *clip, const uint8_t *rgb, int32_t nx, int32_t ny, float *out);
/* clip_image_preprocess, every image the encoder sees for one picture: one (as above) without an image grid; with one, the overview (bicubic resize of the whole
 * picture to S x S) then the S x S tiles, row-major, of the picture fitted (aspect kept, bicubic, centred on black) to the best canvas of the grid.
 * out [n][3][S][S]; returns n (<= 1 + max tiles) or < 0; grid_w x grid_h = tiles across / down (0 x 0 without a grid). */
MI355_API int32_t     mi355_clip_image_preprocess_grid(const mi355_clip *clip, const uint8_t *rgb, int32_t nx, int32_t ny, float *out, size_t out_floats,
                                                       int32_t *grid_w, int32_t *grid_h);
/* clip_image_encode: img [3][S][S] -> out [n_patches][n_mmproj_embd] (host memory) */
MI355_API int32_t     mi355_clip_image_encode(mi355_clip *clip, const float *img, float *out);
/* llava_image_embed_make_with_clip_img on encoded image bytes: decode + preprocess + encode (+ with an image grid, the tiles' rows re-ordered to the canvas'
 * row-major order behind the overview's: clip_llava_handle_patches).  Returns the number of rows written (<= mi355_clip_max_image_rows) or < 0. */
MI355_API int32_t     mi355_llava_image_embed_from_bytes(mi355_clip *clip, const uint8_t *bytes, size_t n_bytes, float *out, size_t out_floats);

#ifdef __cplusplus
}
#endif
#endif /* MI355_LLAMA_H */
