// model_plan.h — what a GGUF file's model looks like and where each of its tensors goes, worked out on the host alone.
//
// plan_model() reads the hyper-parameters, refuses what this backend does not run, and lays out the weight arena: it
// touches no device, so every refusal and every arena rule is the same with and without a GPU (tests/test_model_plan_cpu.py).
// runtime.cc's model_load uploads what the plan says.  No HIP header here: this compiles with a plain C++ compiler.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../csrc/ggml_types.h"
#include "gguf.h"

namespace mi355 {

struct DevTensor {
    std::string name;
    int type = 0;
    int64_t K = 0;          // ne[0]: contraction / row length
    int64_t N = 0;          // rows per expert (ne[1])
    int64_t n_expert = 1;   // ne[2] for *_exps tensors
    uint8_t *data = nullptr;
    size_t row_bytes = 0;   // device row stride
    size_t bytes = 0;       // device bytes
    size_t ggml_bytes = 0;  // on-disk bytes
    uint8_t *planes = nullptr;   // pre-expanded MFMA operand planes for prompt processing (mmq.hip), optional
    size_t planes_bytes = 0;
    bool valid() const { return data != nullptr; }
};

struct LayerWeights {
    DevTensor attn_norm, wq, wk, wv, wo, bq, bk, bv;
    DevTensor q_norm, k_norm;     // qwen3: [head_dim] f32 weights of the per-head RMSNorm of Q and K before the rope (empty otherwise)
    DevTensor ffn_norm, gate, up, down;
    // single-token steps of a feed-forward width the weight stream has no form for (K = 28672: a 16 KB row does not fit the ring pairwise) while half of
    // it has one: the column halves of ffn_down as two tensors of their own, contracted by two launches (x += W_lo a_lo; x += W_hi a_hi).  A second copy
    // of the tensor in HBM; prompt batches keep the whole tensor (and its planes).  Empty otherwise.
    DevTensor down_lo, down_hi;
    DevTensor gate_inp, gate_exps, up_exps, down_exps;
    // encoder files (nomic-bert): the fused Q | K | V projection (wq / wk / wv are row ranges of it), LayerNorms with biases after the attention and the feed-forward block
    DevTensor wqkv, bo, attn_out_norm, attn_out_norm_b, layer_out_norm, layer_out_norm_b;
};

struct HParams {
    std::string arch;
    int n_embd = 0, n_layer = 0, n_ff = 0, n_head = 0, n_head_kv = 0, n_rot = 0, n_vocab = 0;
    int n_expert = 0, n_expert_used = 0, head_dim = 0, n_ctx_train = 0;
    int pooling_type = 0;          // {arch}.pooling_type: 0 none, 1 mean, 2 cls, 3 last (what llama_get_embeddings_seq pools over a sequence's tokens)
    float eps = 1e-5f, rope_base = 10000.0f, rope_scale = 1.0f;
    int rope_neox = 0;
    bool encoder = false;          // bidirectional attention, embeddings only (general.architecture nomic-bert: llm_build_bert)
    bool qk_norm = false;          // qwen3: per-head RMSNorm of Q and K before the rope (LayerWeights::q_norm / k_norm); head_dim from attention.key_length
    float yarn_ext = 0.0f, yarn_attn = 1.0f, yarn_lo = 0.0f, yarn_hi = 0.0f;   // rope.scaling.type "yarn" (RopeArgs, kernels.h)
    // row split: n_head, n_head_kv and n_ff above are THIS RANK's share; the file's values are kept here.
    // A shard is the same graph with fewer heads and a narrower feed-forward, attn_output and ffn_down contracting over
    // the local slice only: their partial sums are the one thing exchanged (tp_comm.h).
    int tp_rank = 0, tp_size = 1;
    bool tp_exchange = false;    // the process has a matching group: partial sums and logits slices go through it
    int n_head_full = 0, n_head_kv_full = 0, n_ff_full = 0;
    int n_vocab_local = 0;       // rows of the output projection held here (n_vocab when it is not split)
};

// the model as the file describes it: filled in place by plan_model (the plan points at these tensors), given device addresses by the upload
struct ModelLayout {
    HParams hp;
    DevTensor tok_embd, out_norm, output, rope_freqs;
    DevTensor tok_types, tok_norm, tok_norm_b;       // encoder files: token-type table (row 0 is added to every token), LayerNorm of the embeddings
    std::vector<LayerWeights> layers;
};

// one tensor of the arena and where its bytes come from: the whole file tensor, this rank's rows (a contiguous range), or a
// column range (the same block range of every row: src_rows pieces of src_width bytes, src_pitch apart)
struct TensorPlan {
    const GGUFTensorInfo *ti;
    DevTensor *dst;
    size_t off;                                  // arena offset (256-aligned)
    size_t src_off, src_pitch, src_width;
    int64_t src_rows;
    size_t src_bytes;
    bool extra_copy;                             // a second copy of bytes another entry holds (the column halves of ffn_down): not counted
};

struct LoadPlan {
    std::vector<TensorPlan> tensors;             // in the order they were asked for = arena order
    size_t total = 0;                            // arena bytes
    size_t max_stage = 0;                        // largest source range of a tensor that is repacked on its way (the staging buffer)
    uint64_t file_tensor_bytes = 0;              // on-disk bytes of what is loaded, each once
    uint64_t bytes_per_token = 0;                // algorithmic bytes per decoded token
};

// tp_size > 1: rank tp_rank's slice of every projection (rows of attn_q/k/v, ffn_gate/up and output; the matching
// super-block columns of attn_output and ffn_down), cut on head and 256-element boundaries.  tp_group_matches: the process
// has a row-split group of that size in which it is that rank (tp_comm.h; the caller asks, the planner links nothing of it).
// False with err and status (-102) set when the file is refused; layout and plan are then meaningless.
bool plan_model(const GGUFFile &f, int tp_rank, int tp_size, bool tp_group_matches, ModelLayout &layout, LoadPlan &plan, std::string &err, int &status);

}  // namespace mi355
