// lora.cc — the checks of a LoRA adapter file against its base model (lora.h).  Host arithmetic only: no HIP header, compiles with a plain C++ compiler.
#include "lora.h"

#include <cstdlib>

namespace mi355 {
namespace {

bool ends_with(const std::string &s, const char *suf) {
    const size_t n = std::char_traits<char>::length(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

std::string dims(const GGUFTensorInfo &t) {
    std::string s = "[";
    for (int i = 0; i < t.n_dims; i++) s += (i ? ", " : "") + std::to_string(t.ne[i]);
    return s + "]";
}

struct Target { const char *leaf; int target; };
const Target LAYER_TARGETS[] = {{"attn_q.weight", LORA_Q}, {"attn_k.weight", LORA_K}, {"attn_v.weight", LORA_V}, {"attn_output.weight", LORA_O},
                                {"ffn_gate.weight", LORA_GATE}, {"ffn_up.weight", LORA_UP}, {"ffn_down.weight", LORA_DOWN}};

const DevTensor *layer_tensor(const LayerWeights &L, int target) {
    switch (target) {
        case LORA_Q: return &L.wq;
        case LORA_K: return &L.wk;
        case LORA_V: return &L.wv;
        case LORA_O: return &L.wo;
        case LORA_GATE: return &L.gate;
        case LORA_UP: return &L.up;
        default: return &L.down;
    }
}

// a target this backend has no adapter form for: why (nullptr: not one of them)
const char *excluded_target(const std::string &base) {
    if (base == "token_embd.weight") return "the embedding lookup has no adapter form";
    if (base.find("ffn_gate_inp") != std::string::npos) return "the router of a mixture-of-experts layer is not adapted";
    if (base.find("_exps.") != std::string::npos) return "expert tensors have no adapter form";
    if (base.find("attn_qkv") != std::string::npos) return "the encoder's fused Q | K | V projection has no adapter form";
    return nullptr;
}

}  // namespace

bool plan_lora(const GGUFFile &f, const ModelLayout &m, LoraPlan &plan, std::string &err, int &status) {
    auto refuse = [&](const std::string &why) { err = why; status = -102; return false; };
    plan = LoraPlan();
    const HParams &hp = m.hp;
    const std::string gtype = f.get_s("general.type", ""), atype = f.get_s("adapter.type", ""), arch = f.get_s("general.architecture", "");
    if (gtype != "adapter") return refuse("not an adapter file: general.type is '" + gtype + "' (a LoRA adapter says 'adapter')");
    if (atype != "lora") return refuse("unsupported adapter.type '" + atype + "' (this backend applies 'lora' adapters)");
    if (hp.encoder) return refuse("LoRA adapters are not supported on encoder models (" + hp.arch + ")");
    if (hp.tp_size > 1 || hp.tp_exchange) return refuse("LoRA adapters are not supported on a model loaded as a rank of a row split (split_mode \"row\" / tp_size > 1): load it on one device");
    if (arch != hp.arch) return refuse("adapter architecture '" + arch + "' does not match the model's '" + hp.arch + "'");
    const GGUFValue *alpha = f.find("adapter.lora.alpha");
    if (!alpha || alpha->type != GV_F32) return refuse("adapter.lora.alpha is missing or not an f32");
    plan.alpha = (float)alpha->f;

    for (const GGUFTensorInfo &ti : f.tensors) {
        const bool is_a = ends_with(ti.name, ".lora_a"), is_b = ends_with(ti.name, ".lora_b");
        if (!is_a && !is_b) return refuse("adapter tensor " + ti.name + " ends in neither .lora_a nor .lora_b");
        const std::string base = ti.name.substr(0, ti.name.size() - 7);
        if (!f.tensor(base + (is_a ? ".lora_b" : ".lora_a"))) return refuse("adapter tensor " + ti.name + " has no " + base + (is_a ? ".lora_b" : ".lora_a") + " beside it");
        if (!is_a) continue;
        const GGUFTensorInfo &ta = ti, &tb = *f.tensor(base + ".lora_b");
        LoraPairPlan p;
        p.base = base; p.a = &ta; p.b = &tb;
        // which tensor of the model: blk.N.<leaf> or output.weight
        if (const char *why = excluded_target(base)) return refuse("adapter on " + base + " is not supported: " + why);
        const DevTensor *w = nullptr;
        if (base == "output.weight") {
            p.layer = -1; p.target = LORA_OUTPUT;
            w = m.output.name == "output.weight" ? &m.output : &m.tok_embd;      // (a tied head: the embedding table's rows)
        } else if (base.rfind("blk.", 0) == 0) {
            char *end = nullptr;
            const long il = strtol(base.c_str() + 4, &end, 10);
            const std::string leaf = end && *end == '.' ? std::string(end + 1) : std::string();
            int target = -1;
            for (const Target &t : LAYER_TARGETS) if (leaf == t.leaf) target = t.target;
            if (end == base.c_str() + 4 || target < 0)
                return refuse("adapter on " + base + " is not supported (adapters apply to blk.N.{attn_q,attn_k,attn_v,attn_output,ffn_gate,ffn_up,ffn_down}.weight and output.weight)");
            p.layer = (int)il; p.target = target;
            if (il >= 0 && il < (long)m.layers.size()) w = layer_tensor(m.layers[(size_t)il], target);
        } else {
            return refuse("adapter on " + base + " is not supported (adapters apply to blk.N.{attn_q,attn_k,attn_v,attn_output,ffn_gate,ffn_up,ffn_down}.weight and output.weight)");
        }
        if (!w || w->name.empty()) return refuse("adapter targets " + base + ", which the model does not have");
        p.K = w->K; p.N = w->N;
        for (const GGUFTensorInfo *t : {&ta, &tb})
            if (t->type != T_F32 && t->type != T_F16) return refuse("adapter tensor " + t->name + " has unsupported type " + ggml_type_name(t->type) + " (f32 and f16 are)");
        if (ta.type != tb.type)
            return refuse("adapter pair " + base + ": lora_a is " + ggml_type_name(ta.type) + " and lora_b is " + ggml_type_name(tb.type) + " (both halves must have one type)");
        p.type = ta.type;
        if (ta.n_dims > 2 || tb.n_dims > 2 || ta.ne[0] != p.K || tb.ne[1] != p.N || ta.ne[1] != tb.ne[0])
            return refuse("adapter pair " + base + ": lora_a is " + dims(ta) + " and lora_b is " + dims(tb) + " where the base tensor is [" + std::to_string(p.K) + ", " +
                          std::to_string(p.N) + "] (lora_a [K, r], lora_b [r, N])");
        if (ta.ne[1] < 1 || ta.ne[1] > LORA_RANK_MAX) return refuse("adapter pair " + base + ": rank " + std::to_string(ta.ne[1]) + " is outside 1 .. " + std::to_string(LORA_RANK_MAX));
        p.r = (int)ta.ne[1];
        plan.pairs.push_back(p);
    }
    if (plan.pairs.empty()) return refuse("adapter file without tensors");
    return true;
}

}  // namespace mi355
