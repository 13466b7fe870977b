// cvec.cc — the control-vector file loader (cvec.h)
#include "cvec.h"

#include <cstdlib>
#include <cstring>

#include "gguf.h"

namespace mi355 {

static bool load_one(const ControlVectorFile &cf, std::vector<float> &data, int &n_embd, std::string &err) {
    GGUFFile f;
    const std::string oerr = f.open(cf.path);
    if (!oerr.empty()) { err = cf.path + ": " + oerr; return false; }
    static const char prefix[] = "direction.";
    bool any = false;
    for (const GGUFTensorInfo &t : f.tensors) {
        if (t.name.compare(0, sizeof(prefix) - 1, prefix) != 0) continue;
        const std::string num = t.name.substr(sizeof(prefix) - 1);
        if (num.empty() || num.size() > 6 || num.find_first_not_of("0123456789") != std::string::npos) {
            err = cf.path + ": " + t.name + ": the layer index is not a number"; return false;
        }
        const long il = std::strtol(num.c_str(), nullptr, 10);
        if (il == 0) { err = cf.path + ": direction.0: layer 0 never has a control vector"; return false; }
        if (t.type != T_F32) { err = cf.path + ": " + t.name + ": type " + ggml_type_name(t.type) + ", a direction tensor must be F32"; return false; }
        if (t.n_dims != 1) { err = cf.path + ": " + t.name + ": " + std::to_string(t.n_dims) + " dimensions, a direction tensor must have one"; return false; }
        if (t.ne[0] < 1 || t.ne[0] > (1 << 20) || !t.data || t.bytes < (size_t)t.ne[0] * 4) { err = cf.path + ": " + t.name + ": bad length"; return false; }
        if (n_embd == 0) n_embd = (int)t.ne[0];
        if (t.ne[0] != n_embd) {
            err = cf.path + ": " + t.name + ": length " + std::to_string(t.ne[0]) + " differs from the other direction tensors' " + std::to_string(n_embd); return false;
        }
        if (data.size() < (size_t)n_embd * (size_t)il) data.resize((size_t)n_embd * (size_t)il, 0.0f);
        float *dst = data.data() + (size_t)n_embd * (size_t)(il - 1);
        for (int j = 0; j < n_embd; j++) {
            float v;
            memcpy(&v, t.data + (size_t)j * 4, 4);
            dst[j] += cf.scale * v;
        }
        any = true;
    }
    if (!any) { err = cf.path + ": no direction tensor (direction.N) in the file"; return false; }
    return true;
}

bool control_vector_load(const std::vector<ControlVectorFile> &files, std::vector<float> &data, int &n_embd, std::string &err) {
    data.clear();
    n_embd = 0;
    if (files.empty()) { err = "control vector: no file given"; return false; }
    for (const ControlVectorFile &cf : files)
        if (!load_one(cf, data, n_embd, err)) { data.clear(); n_embd = 0; return false; }
    return true;
}

}  // namespace mi355
