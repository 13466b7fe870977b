// lora_plan_main BASE.gguf ADAPTER.gguf [user_scale [tp_rank tp_size]] — what host/lora.cc makes of an adapter file against a base model, without a GPU:
// {"status": -102, "err": "..."} for a refusal, else {"status": 0, "alpha": a, "pairs": [{"base", "layer", "target", "r", "type", "K", "N", "scale"}]}.
// Built by tests/test_lora_cpu.py from this file, host/gguf.cc, host/model_plan.cc and host/lora.cc.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../cortex.llamacpp_amd/host/lora.h"

using namespace mi355;

static std::string quoted(const std::string &s) {
    std::string o = "\"";
    for (char c : s) {
        if (c == '"' || c == '\\') { o += '\\'; o += c; }
        else if ((unsigned char)c < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", c); o += b; }
        else o += c;
    }
    return o + "\"";
}

static int refused(int status, const std::string &err) {
    printf("{\"status\": %d, \"err\": %s}\n", status, quoted(err).c_str());
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s BASE.gguf ADAPTER.gguf [user_scale [tp_rank tp_size]]\n", argv[0]); return 2; }
    const float user_scale = argc > 3 ? (float)atof(argv[3]) : 1.0f;
    const int tp_rank = argc > 5 ? atoi(argv[4]) : 0, tp_size = argc > 5 ? atoi(argv[5]) : 1;
    GGUFFile base, ad;
    std::string err = base.open(argv[1]);
    if (!err.empty()) return refused(-101, err);
    ModelLayout layout;
    LoadPlan lp;
    int status = 0;
    if (!plan_model(base, tp_rank, tp_size, tp_size > 1, layout, lp, err, status)) return refused(status, "base model: " + err);
    err = ad.open(argv[2]);
    if (!err.empty()) return refused(err.rfind("cannot", 0) == 0 ? -101 : -102, err);
    LoraPlan plan;
    if (!plan_lora(ad, layout, plan, err, status)) return refused(status, err);
    printf("{\"status\": 0, \"alpha\": %.9g, \"pairs\": [", plan.alpha);
    for (size_t i = 0; i < plan.pairs.size(); i++) {
        const LoraPairPlan &p = plan.pairs[i];
        printf("%s{\"base\": %s, \"layer\": %d, \"target\": %d, \"r\": %d, \"type\": %s, \"K\": %lld, \"N\": %lld, \"scale\": %.9g}", i ? ", " : "", quoted(p.base).c_str(), p.layer,
               p.target, p.r, quoted(ggml_type_name(p.type)).c_str(), (long long)p.K, (long long)p.N, lora_scale(user_scale, plan.alpha, p.r));
    }
    printf("]}\n");
    return 0;
}
