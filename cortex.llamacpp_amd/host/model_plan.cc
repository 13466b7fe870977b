// model_plan.cc — GGUF metadata -> hyper-parameters, refusals and the weight arena's layout (model_plan.h).  Host arithmetic only.
#include "model_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <initializer_list>

namespace mi355 {
namespace {

// The graph built by the runtime is llm_build_llama's: "llama" files (Llama, Mistral, TinyLlama, Mixtral ... all carry that name), "qwen2"
// (the same op order with NEOX rope pairing and Q / K / V biases) and "qwen3" (llm_build_qwen3: qwen2's order without biases, a per-head RMSNorm of Q and K
// before the rope, the head size from attention.key_length - the attention width H * D need not be n_embd) and "qwen3moe" (llm_build_qwen3moe: qwen3's
// attention with build_moe_ffn's routed feed-forward - softmax gating, top-k, weights renormalised - and no shared expert).  Gemma, Phi-3, BERT-type
// encoders etc. are other graphs: refused, never run as llama.
// "nomic-bert" (the reference's embedding smoke model, Makefile:6) is the one encoder graph: llm_build_bert's NOMIC_BERT branches (run_layers_encoder)
struct ArchTraits {
    const char *name;          // general.architecture
    bool encoder;              // bidirectional attention, LayerNorms, fused Q | K | V
    bool qk_norm;              // per-head RMSNorm of Q and K; the head size comes from attention.key_length
    bool rope_neox;            // NEOX rope pairing
    bool routed_only;          // every layer's feed-forward is routed (no dense ffn_gate / ffn_up / ffn_down)
    const char *ff_key;        // the key that holds the feed-forward width the tensors are checked against
    const char *eps_key;       // the norm epsilon's key, and its value when the file has none
    double eps_default;
};
// qwen3moe: feed_forward_length is the width of a dense layer the file does not have; the experts' width is expert_feed_forward_length (optional: the
// tensors' own width stands when it is absent)
const ArchTraits ARCHS[] = {
    {"llama",      false, false, false, false, "feed_forward_length",        "attention.layer_norm_rms_epsilon", 1e-5},
    {"qwen2",      false, false, true,  false, "feed_forward_length",        "attention.layer_norm_rms_epsilon", 1e-5},
    {"qwen3",      false, true,  true,  false, "feed_forward_length",        "attention.layer_norm_rms_epsilon", 1e-5},
    {"qwen3moe",   false, true,  true,  true,  "expert_feed_forward_length", "attention.layer_norm_rms_epsilon", 1e-5},
    {"nomic-bert", true,  false, true,  false, "feed_forward_length",        "attention.layer_norm_epsilon",     1e-12},
};
const ArchTraits *arch_traits(const std::string &arch) {
    for (const ArchTraits &t : ARCHS)
        if (arch == t.name) return &t;
    return nullptr;
}

bool type_supported(int t) {
    return t == T_F32 || t == T_F16 || t == T_BF16 || type_is_quant(t);
}

// where a tensor's bytes come from: the whole tensor, or this rank's rows (a contiguous range), or this rank's
// columns (the same block range of every row: a strided copy)
enum { SPLIT_NONE = 0, SPLIT_ROWS = 1, SPLIT_COLS = 2 };

// One plan_model call.  A refusal sets err; the steps that look at many tensors go on after one (fail) exactly as far as
// they always have, so a file with several faults names the same one as ever.
struct Planner {
    const GGUFFile &f;
    ModelLayout &m;
    LoadPlan &lp;
    std::string &err;
    HParams &hp;
    const ArchTraits *tr = nullptr;
    int P = 1, R = 0;              // row split: ranks, this rank
    bool fail = false;

    Planner(const GGUFFile &file, ModelLayout &layout, LoadPlan &plan, std::string &e) : f(file), m(layout), lp(plan), err(e), hp(layout.hp) {}
    bool refuse(const std::string &why) { err = why; fail = true; return false; }

    bool read_hparams();
    bool read_rope(const std::string &a);
    bool plan_row_split(int tp_rank, int tp_size, bool tp_group_matches);
    bool type_refused(const std::string &name, const GGUFTensorInfo &ti);
    bool cut_source(const std::string &name, const GGUFTensorInfo &ti, DevTensor &dst, TensorPlan &pl, int split, int cpart, int cparts);
    void place(const GGUFTensorInfo &ti, DevTensor &dst, const TensorPlan &pl);
    void plan_tensor(const std::string &name, DevTensor &dst, bool required, int split = SPLIT_NONE, int cpart = 0, int cparts = 1);
    bool list_tensors();
    void list_encoder_layer(const std::string &p, LayerWeights &L);
    void list_decoder_layer(const std::string &p, LayerWeights &L);
    void shape(const DevTensor &t, int64_t K, int64_t N, int64_t NE, bool vec);
    void must_be_f32(std::initializer_list<const DevTensor *> ts);
    bool check_shapes();
    void check_shapes_encoder(int64_t E, int64_t D, int64_t QW, int64_t KVW);
    void check_shapes_decoder(int64_t E, int64_t D, int64_t QW, int64_t KVW);
    bool check_widths();
    void bytes_per_token();
};

// ---- the keys, the head-count and head-size rules
bool Planner::read_hparams() {
    hp.arch = f.get_s("general.architecture", "");
    if (hp.arch.empty()) return refuse("general.architecture missing");
    tr = arch_traits(hp.arch);
    if (!tr) return refuse("unsupported general.architecture '" + hp.arch + "' (this backend builds the llama graph - llama, qwen2, qwen3, qwen3moe - and the nomic-bert encoder)");
    hp.encoder = tr->encoder;
    hp.qk_norm = tr->qk_norm;
    const std::string a = hp.arch + ".";
    hp.n_embd = (int)f.get_u(a + "embedding_length", 0);
    hp.n_layer = (int)f.get_u(a + "block_count", 0);
    hp.n_ff = (int)f.get_u(a + tr->ff_key, 0);
    hp.n_head = (int)f.get_u(a + "attention.head_count", 0);
    hp.n_head_kv = (int)f.get_u(a + "attention.head_count_kv", (uint64_t)hp.n_head);
    hp.eps = (float)f.get_f(a + tr->eps_key, tr->eps_default);
    hp.rope_base = (float)f.get_f(a + "rope.freq_base", 10000.0);
    hp.n_expert = (int)f.get_u(a + "expert_count", 0);
    hp.n_expert_used = (int)f.get_u(a + "expert_used_count", 0);
    hp.n_ctx_train = (int)f.get_u(a + "context_length", 0);
    hp.pooling_type = (int)f.get_u(a + "pooling_type", 0);
    if (tr->routed_only && hp.n_expert <= 0) return refuse("qwen3moe file without experts (expert_count missing or 0): dense feed-forward layers under the qwen3moe name are not supported");
    if (tr->routed_only && (f.tensor("blk.0.ffn_gate.weight") || f.tensor("blk.0.ffn_up.weight") || f.tensor("blk.0.ffn_down.weight")))
        return refuse("qwen3moe file with dense ffn_gate / ffn_up / ffn_down tensors: not supported (a qwen3moe layer is routed: ffn_gate_inp and *_exps)");
    if (hp.n_embd <= 0 || hp.n_layer <= 0 || hp.n_head <= 0) return refuse("missing hyper-parameters for arch " + hp.arch);
    if (hp.n_layer > 1024 || hp.n_embd > (1 << 20) || hp.n_head > 4096) return refuse("implausible hyper-parameters for arch " + hp.arch);
    // the head counts size buffers and pick kernels: check them here, not at the first decode
    if (hp.n_head_kv <= 0 || hp.n_head % hp.n_head_kv) return refuse("attention.head_count_kv (" + std::to_string(hp.n_head_kv) + ") must be positive and divide attention.head_count (" + std::to_string(hp.n_head) + ")");
    const int ratio = hp.n_head / hp.n_head_kv;
    // (1, 2, 4, 8 have the tuned single-launch decode attention and the matrix-core prompt attention; 3, 5, 6, 7 take the general split kernel)
    if (ratio < 1 || ratio > 8) return refuse("unsupported query / kv head ratio " + std::to_string(ratio) + " (the attention kernels are built for 1 .. 8)");
    // (qwen3 sets its head size itself: n_embd / n_head need not be whole)
    if (!hp.qk_norm && hp.n_embd % hp.n_head) return refuse("embedding_length is not a multiple of attention.head_count");
    if (hp.n_expert < 0 || hp.n_expert > 256 || hp.n_expert_used < 0 || hp.n_expert_used > hp.n_expert || (hp.n_expert > 0 && hp.n_expert_used == 0)) return refuse("bad expert_count / expert_used_count");
    // llama / qwen2: n_embd / n_head, whatever attention.key_length says (a llama file whose key_length disagrees - Mistral-Nemo style - is read exactly as
    // before; the width handling below is the groundwork for it).  qwen3: attention.key_length, which value_length must equal.
    hp.head_dim = hp.n_embd / hp.n_head;
    if (hp.qk_norm) {
        const uint64_t kl = f.get_u(a + "attention.key_length", 0), vl = f.get_u(a + "attention.value_length", kl);
        if (kl == 0) return refuse("qwen3 file without attention.key_length");
        if (vl != kl) return refuse("attention.value_length (" + std::to_string(vl) + ") differs from attention.key_length (" + std::to_string(kl) + "): not supported");
        if (kl > 4096) return refuse("implausible attention.key_length");
        hp.head_dim = (int)kl;
    }
    if (!read_rope(a)) return false;
    if (hp.head_dim != 64 && hp.head_dim != 128) return refuse("unsupported head_dim " + std::to_string(hp.head_dim));
    // Row lengths - n_embd, the attention width H * D, n_ff - are whole numbers of 32-element blocks; what each TENSOR's type makes of its own row length is
    // checked tensor by tensor (plan_tensor), and the graphs that still want whole 256-blocks say so by name once the widths are known (check_widths).
    if (hp.n_embd % 32) return refuse("embedding_length (" + std::to_string(hp.n_embd) + ") must be a multiple of 32");
    return true;
}

// ---- the rotary parameters and rope.scaling
bool Planner::read_rope(const std::string &a) {
    hp.n_rot = (int)f.get_u(a + "rope.dimension_count", (uint64_t)hp.head_dim);
    hp.rope_neox = tr->rope_neox;
    const std::string scaling = f.get_s(a + "rope.scaling.type", "none");
    if (scaling == "linear") hp.rope_scale = 1.0f / (float)f.get_f(a + "rope.scaling.factor", 1.0);
    if (scaling == "yarn") {
        // YaRN (llama.cpp: rope_yarn / ggml_rope_yarn_corr_dims with the context defaults beta_fast 32, beta_slow 1, ext_factor 1): pairs that turn more than
        // beta_fast times over the ORIGINAL context keep their angle, pairs that turn less than beta_slow times are interpolated by 1/factor, a linear ramp between
        const float factor = (float)f.get_f(a + "rope.scaling.factor", 1.0);
        if (!(factor > 0.0f)) return refuse("rope.scaling.factor must be positive");
        const float n_orig = (float)f.get_u(a + "rope.scaling.original_context_length", f.get_u(a + "context_length", 4096));
        hp.rope_scale = 1.0f / factor;
        hp.yarn_ext = 1.0f;
        hp.yarn_attn = (float)f.get_f(a + "rope.scaling.attn_factor", 1.0);
        const float two_log_base = 2.0f * logf(hp.rope_base);
        const float lo = floorf((float)hp.n_rot * logf(n_orig / (32.0f * 2.0f * 3.14159265358979323846f)) / two_log_base);
        const float hi = ceilf((float)hp.n_rot * logf(n_orig / (1.0f * 2.0f * 3.14159265358979323846f)) / two_log_base);
        hp.yarn_lo = lo > 0.0f ? lo : 0.0f;
        hp.yarn_hi = hi < (float)(hp.n_rot - 1) ? hi : (float)(hp.n_rot - 1);
    } else if (scaling != "none" && scaling != "linear") return refuse("unsupported rope.scaling.type " + scaling);
    return true;
}

// ---- row split: this rank's share of the heads and of the feed-forward width
bool Planner::plan_row_split(int tp_rank, int tp_size, bool tp_group_matches) {
    P = tp_size > 1 ? tp_size : 1;
    R = tp_size > 1 ? tp_rank : 0;
    hp.n_head_full = hp.n_head; hp.n_head_kv_full = hp.n_head_kv; hp.n_ff_full = hp.n_ff;
    hp.tp_rank = R; hp.tp_size = P;
    // the exchange steps run whenever the process has a group of that size — also a group of ONE rank, which is how the
    // RCCL calls (and their capture into graphs) are exercised on a single GPU
    hp.tp_exchange = tp_group_matches;
    // (the q / k norm weights and the per-rank path of a qwen3 file are untested under a row split; Qwen3-32B Q4_K_M and Qwen3-30B-A3B fit one device)
    if (P > 1 && hp.qk_norm) return refuse("row split (split_mode \"row\" / tp_size > 1) of " + hp.arch + " files is not supported: load it on one device");
    if (P > 1 && !hp.tp_exchange) return refuse("tp_size > 1 needs the process's row-split group first (mi355_tp_init with the same rank / size)");
    if (P > 1) {
        if (R < 0 || R >= P) return refuse("tp_rank out of range");
        if (hp.n_expert > 0) return refuse("row split of mixture-of-experts files is not supported");
        if (hp.n_head % P || hp.n_head_kv % P) return refuse("tp_size must divide the head counts (" + std::to_string(hp.n_head) + " / " + std::to_string(hp.n_head_kv) + ")");
        if (((hp.n_head / P) * hp.head_dim) % 256) return refuse("a rank's attention width must be a multiple of 256");
        hp.n_head /= P; hp.n_head_kv /= P;
    }
    return true;
}

// ---- plan_tensor, part 1: what a tensor's type rules out (true: refused, err set)
bool Planner::type_refused(const std::string &name, const GGUFTensorInfo &ti) {
    if (!type_supported(ti.type)) return !refuse("tensor " + name + " has unsupported type " + ggml_type_name(ti.type));
    if (ti.type == T_MXFP4) {
        // mxfp4 is a type of the 2-D and expert weights of the decoder graphs: the kernels read norm and bias vectors as f32, the encoder graph's launches
        // and the row split's column cuts and exchange steps are untested with it
        const char *why = ti.n_dims == 1 ? "norm and bias vectors must be f32" : hp.encoder ? "the encoder graph is not supported with mxfp4 tensors" :
                          P > 1 ? "a row split (split_mode \"row\" / tp_size > 1) of mxfp4 tensors is not supported: load the file on one device" : nullptr;
        if (why) return !refuse("tensor " + name + " has type mxfp4: " + why);
    }
    if (type_is_ternary(ti.type)) {
        // tq1_0 / tq2_0 are types of the 2-D and expert weights of the decoder graphs, as mxfp4 is (a row split is refused below in the words of the other types)
        const char *why = ti.n_dims == 1 ? "norm and bias vectors must be f32" : hp.encoder ? "the encoder graph is not supported with ternary tensors" : nullptr;
        if (why) return !refuse("tensor " + name + " has type " + ggml_type_name(ti.type) + ": " + why);
    }
    if (P > 1 && type_row_split_unsupported(ti.type))    // (Q4_1, Q5_1, IQ4_XS, TQ1_0, TQ2_0; an mxfp4 tensor has been refused above in its own words)
        return !refuse(std::string("row split (split_mode \"row\" / tp_size > 1) of ") + ggml_type_name(ti.type) + " tensors is not supported (tensor " + name + "): load the file on one device");
    if (ti.type == T_BF16) {
        // bf16 is a type of the dense 2-D weights (and of token_embd / output): the norm and bias vectors are read as f32 by the kernels, the routed experts,
        // the encoder graph and the row split's column cuts have no bf16 kernels.  Rows are loaded as 16-byte pieces: 8 weights.
        const bool expert = name.size() > 12 && (name.compare(name.size() - 12, 12, "_exps.weight") == 0 || name.find("ffn_gate_inp") != std::string::npos);
        const char *why = ti.n_dims == 1 ? "norm and bias vectors must be f32" : expert ? "bf16 expert tensors are not supported" :
                          hp.encoder ? "the encoder graph has no bf16 kernels" : P > 1 ? "a row split (split_mode \"row\" / tp_size > 1) of bf16 tensors is not supported: load the file on one device" :
                          (ti.ne[0] % 8) ? "bf16 rows must hold a multiple of 8 weights" :
                          // (the bf16 weight stream has a tail form, the matrix-core prompt path is untested at such a width: refused rather than run unchecked)
                          (hp.n_embd % 256) ? "bf16 tensors in a file whose embedding_length is not a multiple of 256 are not supported" : nullptr;
        if (why) return !refuse("tensor " + name + " has type bf16: " + why);
    }
    return false;
}

// ---- plan_tensor, part 2: this rank's rows or columns of the tensor, then column part cpart of cparts of that (false: refused)
bool Planner::cut_source(const std::string &name, const GGUFTensorInfo &ti, DevTensor &dst, TensorPlan &pl, int split, int cpart, int cparts) {
    if (P > 1 && split != SPLIT_NONE) {
        const int64_t blk = std::max<int64_t>(ggml_block_elems(dst.type), 1);
        if (ti.n_dims == 1 || split == SPLIT_COLS) {          // a bias vector is cut like the rows it is added to
            const int64_t unit = split == SPLIT_COLS && blk > 1 ? std::max<int64_t>(blk, 256) : blk;
            if (dst.K % P || (dst.K / P) % unit) return refuse("tensor " + name + ": row length " + std::to_string(dst.K) + " cannot be cut " + std::to_string(P) + " ways on block boundaries");
            dst.K /= P;
            pl.src_width = ggml_row_bytes(dst.type, dst.K);
            pl.src_off = (size_t)R * pl.src_width;
        } else {
            if (dst.N % P) return refuse("tensor " + name + ": " + std::to_string(dst.N) + " rows cannot be cut " + std::to_string(P) + " ways");
            dst.N /= P;
            pl.src_rows = dst.N;
            pl.src_off = (size_t)R * (size_t)dst.N * pl.src_pitch;
        }
        pl.src_bytes = pl.src_width * (size_t)pl.src_rows;
    }
    if (cparts > 1) {                                          // (on 256-element boundaries, checked by the caller)
        dst.name = name + "[cols " + std::to_string(cpart) + "/" + std::to_string(cparts) + "]";
        dst.K /= cparts;
        pl.src_width = ggml_row_bytes(dst.type, dst.K);
        pl.src_off += (size_t)cpart * pl.src_width;
        pl.src_bytes = pl.src_width * (size_t)pl.src_rows;
    }
    return true;
}

// ---- plan_tensor, part 3: the device row, the tensor's place in the arena, the staging buffer it may need
void Planner::place(const GGUFTensorInfo &ti, DevTensor &dst, const TensorPlan &pl) {
    dst.row_bytes = ti.n_dims == 1 ? ggml_row_bytes(dst.type, dst.K) : dev_row_bytes(dst.type, dst.K);
    const int64_t rows = ti.n_dims == 1 ? 1 : dst.N * dst.n_expert;
    dst.bytes = dst.row_bytes * (size_t)rows;
    dst.ggml_bytes = pl.src_bytes;
    lp.tensors.push_back(pl);
    lp.total += (dst.bytes + 255) & ~(size_t)255;
    if (type_is_repacked(dst.type) || dst.row_bytes != ggml_row_bytes(dst.type, dst.K)) lp.max_stage = std::max(lp.max_stage, pl.src_bytes);
}

// cpart / cparts: column part cpart of cparts of THIS RANK's tensor as a tensor of its own (a second copy for the single-token steps, see LayerWeights::down_lo)
void Planner::plan_tensor(const std::string &name, DevTensor &dst, bool required, int split, int cpart, int cparts) {
    const GGUFTensorInfo *ti = f.tensor(name);
    if (!ti) {
        if (required) refuse("missing tensor " + name);
        return;
    }
    if (type_refused(name, *ti)) return;
    dst.name = name;
    dst.type = ti->type;
    dst.K = ti->ne[0];
    dst.N = ti->ne[1];
    dst.n_expert = ti->ne[2];
    // a row is a whole number of its type's blocks: 256 elements for the K-quants, IQ4_XS, TQ1_0 and TQ2_0, 32 for Q8_0 / Q4_0 / Q5_0 / Q4_1 / Q5_1 / IQ4_NL / MXFP4
    // (llama-quantize writes a tensor whose rows are no multiple of 256 in one of the latter)
    const int64_t row_unit = std::max<int64_t>(ggml_block_elems(dst.type), 1);
    if (dst.K % row_unit) {
        refuse("tensor " + name + " (" + ggml_type_name(dst.type) + "): its row length " + std::to_string(dst.K) + " is not a whole number of " + std::to_string(row_unit) + "-element blocks");
        return;
    }
    const size_t full_row = ggml_row_bytes(dst.type, dst.K);
    TensorPlan pl{ti, &dst, lp.total, 0, full_row, full_row, ti->n_dims == 1 ? 1 : dst.N * dst.n_expert, (size_t)ti->bytes, cparts > 1};
    if (!cut_source(name, *ti, dst, pl, split, cpart, cparts)) return;
    place(*ti, dst, pl);
}

// ---- which tensors the file's graph has, in arena order
void Planner::list_encoder_layer(const std::string &p, LayerWeights &L) {
    plan_tensor(p + "attn_qkv.weight", L.wqkv, true);
    plan_tensor(p + "attn_output.weight", L.wo, true);
    plan_tensor(p + "attn_output.bias", L.bo, false);
    plan_tensor(p + "attn_output_norm.weight", L.attn_out_norm, true);
    plan_tensor(p + "attn_output_norm.bias", L.attn_out_norm_b, true);
    plan_tensor(p + "ffn_gate.weight", L.gate, true);
    plan_tensor(p + "ffn_up.weight", L.up, true);
    plan_tensor(p + "ffn_down.weight", L.down, true);
    plan_tensor(p + "layer_output_norm.weight", L.layer_out_norm, true);
    plan_tensor(p + "layer_output_norm.bias", L.layer_out_norm_b, true);
}

void Planner::list_decoder_layer(const std::string &p, LayerWeights &L) {
    plan_tensor(p + "attn_norm.weight", L.attn_norm, true);
    plan_tensor(p + "attn_q.weight", L.wq, true, SPLIT_ROWS);
    plan_tensor(p + "attn_k.weight", L.wk, true, SPLIT_ROWS);
    plan_tensor(p + "attn_v.weight", L.wv, true, SPLIT_ROWS);
    plan_tensor(p + "attn_output.weight", L.wo, true, SPLIT_COLS);
    plan_tensor(p + "attn_q.bias", L.bq, false, SPLIT_ROWS);
    plan_tensor(p + "attn_k.bias", L.bk, false, SPLIT_ROWS);
    plan_tensor(p + "attn_v.bias", L.bv, false, SPLIT_ROWS);
    if (hp.qk_norm) {
        plan_tensor(p + "attn_q_norm.weight", L.q_norm, true);
        plan_tensor(p + "attn_k_norm.weight", L.k_norm, true);
    }
    plan_tensor(p + "ffn_norm.weight", L.ffn_norm, true);
    if (hp.n_expert > 0) {
        plan_tensor(p + "ffn_gate_inp.weight", L.gate_inp, true);
        plan_tensor(p + "ffn_gate_exps.weight", L.gate_exps, true);
        plan_tensor(p + "ffn_up_exps.weight", L.up_exps, true);
        plan_tensor(p + "ffn_down_exps.weight", L.down_exps, true);
        return;
    }
    plan_tensor(p + "ffn_gate.weight", L.gate, true, SPLIT_ROWS);
    plan_tensor(p + "ffn_up.weight", L.up, true, SPLIT_ROWS);
    plan_tensor(p + "ffn_down.weight", L.down, true, SPLIT_COLS);
    // a contraction length without a weight-stream form whose half has one (mmvq_stream_applicable: 1, 2, 3, 4, 6, 7 or 10 passes of 2048):
    // Llama-3-70B's 28672 -> 2 x 14336
    static const bool halves_on = !(getenv("MI355_DOWN_HALVES") && getenv("MI355_DOWN_HALVES")[0] == '0');
    auto kb_ok = [](int64_t K) { const int64_t kb = (K + 2047) >> 11; return kb == 1 || kb == 2 || kb == 3 || kb == 4 || kb == 6 || kb == 7 || kb == 10; };
    const int64_t Kd = L.down.K;
    if (halves_on && !fail && type_is_kq456(L.down.type) && !kb_ok(Kd) && Kd % 512 == 0 && kb_ok(Kd / 2)) {
        plan_tensor(p + "ffn_down.weight", L.down_lo, true, SPLIT_COLS, 0, 2);
        plan_tensor(p + "ffn_down.weight", L.down_hi, true, SPLIT_COLS, 1, 2);
    }
}

bool Planner::list_tensors() {
    plan_tensor("token_embd.weight", m.tok_embd, true);
    if (hp.encoder) {
        if (P > 1) return refuse("row split of encoder files is not supported");
        if (hp.n_expert > 0) return refuse("mixture-of-experts encoder files are not supported");
        plan_tensor("token_types.weight", m.tok_types, false);
        plan_tensor("token_embd_norm.weight", m.tok_norm, true);
        plan_tensor("token_embd_norm.bias", m.tok_norm_b, true);
    } else {
        plan_tensor("output_norm.weight", m.out_norm, true);
        // the output projection is cut by vocabulary rows when they divide evenly (logits are gathered), else every rank keeps it whole
        const GGUFTensorInfo *ot = f.tensor("output.weight");
        plan_tensor("output.weight", m.output, false, ot && ot->ne[1] % P == 0 ? SPLIT_ROWS : SPLIT_NONE);
        plan_tensor("rope_freqs.weight", m.rope_freqs, false);
    }
    m.layers.resize((size_t)hp.n_layer);
    for (int il = 0; il < hp.n_layer && !fail; il++) {
        const std::string p = "blk." + std::to_string(il) + ".";
        if (hp.encoder) list_encoder_layer(p, m.layers[(size_t)il]);
        else list_decoder_layer(p, m.layers[(size_t)il]);
    }
    return !fail;
}

// ---- every tensor against the shape the hyper-parameters imply (per rank under a row split).  The activation buffers
// are sized from the hyper-parameters and the kernels write one value per weight ROW: a file whose tensors disagree
// with its own metadata must fail here, not write out of bounds at the first decode (upstream create_tensor does the
// same).  Per-rank sizes: hp.n_head / n_head_kv are already this rank's.
void Planner::shape(const DevTensor &t, int64_t K, int64_t N, int64_t NE, bool vec) {
    if (fail || t.name.empty()) return;                    // (absent optional tensor)
    const bool ok = vec ? (t.K == K && t.N == 1 && t.n_expert == 1) : (t.K == K && t.N == N && t.n_expert == NE);
    if (!ok)
        refuse("tensor " + t.name + " has shape [" + std::to_string(t.K) + ", " + std::to_string(t.N) + ", " + std::to_string(t.n_expert) + "], expected [" +
               std::to_string(K) + (vec ? "]" : ", " + std::to_string(N) + ", " + std::to_string(NE) + "]"));
}

// norms and biases are read as f32 vectors by the kernels
void Planner::must_be_f32(std::initializer_list<const DevTensor *> ts) {
    for (const DevTensor *t : ts)
        if (!fail && !t->name.empty() && t->type != T_F32) refuse("tensor " + t->name + " must be f32");
}

void Planner::check_shapes_encoder(int64_t E, int64_t D, int64_t QW, int64_t KVW) {
    if (!m.tok_types.name.empty() && (m.tok_types.K != E || m.tok_types.N < 1 || m.tok_types.type != T_F32)) refuse("token_types.weight must hold f32 rows of embedding_length");
    shape(m.tok_norm, E, 0, 0, true); shape(m.tok_norm_b, E, 0, 0, true);
    if (hp.n_rot != D) refuse("encoder files rotate whole heads (rope.dimension_count must equal the head size)");
    int64_t FFe = 0;
    for (int il = 0; il < hp.n_layer && !fail; il++) {
        const LayerWeights &L = m.layers[(size_t)il];
        if (il == 0) FFe = L.gate.N;
        shape(L.wqkv, E, QW + 2 * KVW, 1, false); shape(L.wo, QW, E, 1, false); shape(L.bo, E, 0, 0, true);
        shape(L.attn_out_norm, E, 0, 0, true); shape(L.attn_out_norm_b, E, 0, 0, true);
        shape(L.layer_out_norm, E, 0, 0, true); shape(L.layer_out_norm_b, E, 0, 0, true);
        shape(L.gate, E, FFe, 1, false); shape(L.up, E, FFe, 1, false); shape(L.down, FFe, E, 1, false);
        if (!fail && (FFe <= 0 || (hp.n_ff_full > 0 && FFe != hp.n_ff_full))) refuse("feed-forward tensors do not match feed_forward_length");
        must_be_f32({&L.bo, &L.attn_out_norm, &L.attn_out_norm_b, &L.layer_out_norm, &L.layer_out_norm_b});
    }
    if (!fail && (m.tok_norm.type != T_F32 || m.tok_norm_b.type != T_F32)) refuse("token_embd_norm must be f32");
}

void Planner::check_shapes_decoder(int64_t E, int64_t D, int64_t QW, int64_t KVW) {
    const int64_t V = m.tok_embd.N;
    shape(m.out_norm, E, 0, 0, true);
    if (!m.output.name.empty()) shape(m.output, E, f.tensor("output.weight")->ne[1] % P == 0 ? V / P : V, 1, false);
    if (!m.rope_freqs.name.empty() && (m.rope_freqs.K != hp.n_rot / 2 || m.rope_freqs.type != T_F32)) refuse("rope_freqs.weight must hold rope.dimension_count / 2 f32 factors");
    if (hp.n_rot <= 0 || hp.n_rot > D || (hp.n_rot & 1)) refuse("bad rope.dimension_count");
    // (the q / k norm kernels rotate whole heads)
    if (!fail && hp.qk_norm && hp.n_rot != D) refuse("qwen3 files must rotate whole heads (rope.dimension_count must equal attention.key_length)");
    if (!fail && hp.qk_norm && !tr->routed_only && hp.n_expert > 0) refuse("qwen3 files with experts are not supported");
    int64_t FF = 0;
    for (int il = 0; il < hp.n_layer && !fail; il++) {
        const LayerWeights &L = m.layers[(size_t)il];
        shape(L.attn_norm, E, 0, 0, true); shape(L.ffn_norm, E, 0, 0, true);
        shape(L.wq, E, QW, 1, false); shape(L.wk, E, KVW, 1, false); shape(L.wv, E, KVW, 1, false);
        shape(L.wo, QW, E, 1, false);
        shape(L.bq, QW, 0, 0, true); shape(L.bk, KVW, 0, 0, true); shape(L.bv, KVW, 0, 0, true);
        shape(L.q_norm, D, 0, 0, true); shape(L.k_norm, D, 0, 0, true);
        if (hp.n_expert > 0) {
            if (il == 0) FF = L.gate_exps.N;
            shape(L.gate_inp, E, hp.n_expert, 1, false);
            shape(L.gate_exps, E, FF, hp.n_expert, false); shape(L.up_exps, E, FF, hp.n_expert, false);
            shape(L.down_exps, FF, E, hp.n_expert, false);
        } else {
            if (il == 0) FF = L.gate.N;
            shape(L.gate, E, FF, 1, false); shape(L.up, E, FF, 1, false);
            shape(L.down, FF, E, 1, false);
        }
        if (!fail && (FF <= 0 || (hp.n_ff_full > 0 && FF * P != hp.n_ff_full))) refuse(std::string("feed-forward tensors do not match ") + tr->ff_key);
        must_be_f32({&L.attn_norm, &L.ffn_norm, &L.bq, &L.bk, &L.bv, &L.q_norm, &L.k_norm});
    }
    if (!fail && m.out_norm.type != T_F32) refuse("output_norm.weight must be f32");
}

bool Planner::check_shapes() {
    const int64_t E = hp.n_embd, D = hp.head_dim, QW = (int64_t)hp.n_head * D, KVW = (int64_t)hp.n_head_kv * D;
    if (m.tok_embd.K != E || m.tok_embd.N <= 0 || m.tok_embd.n_expert != 1) refuse("token_embd.weight does not have embedding_length columns");
    if (hp.encoder) check_shapes_encoder(E, D, QW, KVW);
    else check_shapes_decoder(E, D, QW, KVW);
    if (fail) return false;
    // what the tensors settle: the vocabulary, this rank's feed-forward width, the output rows held here
    hp.n_vocab = (int)m.tok_embd.N;
    hp.n_ff = (int)(hp.n_expert ? m.layers[0].gate_exps.N : m.layers[0].gate.N);     // this rank's width under a row split
    if (!hp.n_ff_full) hp.n_ff_full = hp.n_ff * P;
    hp.n_vocab_local = !m.output.name.empty() ? (int)m.output.N : hp.n_vocab;
    return true;
}

// ---- Where whole 256-blocks are still wanted: graphs whose kernels have no general form to fall back to at such a width.  The dense llama / qwen2 / qwen3
// graph runs every width that is a multiple of 32 (the quantisers, the generic mat-vec and the Q8_0 prompt kernel take a row that ends inside a 256-group).
bool Planner::check_widths() {
    const int64_t aw = (int64_t)hp.n_head_full * hp.head_dim;
    const bool odd = (hp.n_embd % 256) || (aw % 256) || (hp.n_ff_full % 256);
    const std::string widths = "embedding_length " + std::to_string(hp.n_embd) + ", attention width " + std::to_string(aw) + ", feed-forward width " + std::to_string(hp.n_ff_full);
    const char *what = !odd ? nullptr : hp.n_expert > 0 ? "mixture-of-experts files (the expert gather and the expert mat-vecs work on whole 256-blocks)" :
                       hp.encoder ? "encoder files" : P > 1 ? "a row split (split_mode \"row\" / tp_size > 1)" : nullptr;
    if (what) return refuse(std::string(what) + " need widths that are multiples of 256 (" + widths + ")");
    return true;
}

// ---- algorithmic bytes per decoded token: each tensor once, one embedding row, used experts only; and the file bytes loaded
void Planner::bytes_per_token() {
    for (const TensorPlan &pl : lp.tensors) {
        if (pl.extra_copy) continue;                               // (the column halves of ffn_down: the same bytes a second time)
        lp.file_tensor_bytes += pl.src_bytes;
        const DevTensor &d = *pl.dst;
        uint64_t b = pl.src_bytes;
        if (&d == &m.tok_embd) b = ggml_row_bytes(d.type, d.K);
        else if (d.n_expert > 1 && hp.n_expert_used > 0) b = b / (uint64_t)d.n_expert * (uint64_t)hp.n_expert_used;
        lp.bytes_per_token += b;
    }
    // no output.weight: the output head is the embedding table, read whole (counted for an encoder file too, which has no head)
    if (m.output.name.empty()) lp.bytes_per_token += m.tok_embd.ggml_bytes;
}

}  // namespace

bool plan_model(const GGUFFile &f, int tp_rank, int tp_size, bool tp_group_matches, ModelLayout &layout, LoadPlan &plan, std::string &err, int &status) {
    Planner p(f, layout, plan, err);
    const bool ok = p.read_hparams() && p.plan_row_split(tp_rank, tp_size, tp_group_matches) && p.list_tensors() && p.check_shapes() && p.check_widths();
    if (!ok) { status = -102; return false; }
    p.bytes_per_token();
    return true;
}

}  // namespace mi355
