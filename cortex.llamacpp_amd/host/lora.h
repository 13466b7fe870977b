// lora.h — a LoRA adapter GGUF file (convert_lora_to_gguf.py output) checked against the model it is loaded onto.  Host arithmetic only.
//
// llama.cpp reads such a file with llama_adapter_lora_init and applies it inside every mul_mat of the graph (build_lora_mm):
//   y = W x + sum over the active adapters of scale * B (A x),   scale = user_scale * alpha / r   (user_scale when alpha == 0)
// The file: general.type "adapter", adapter.type "lora", general.architecture = the base model's, adapter.lora.alpha (f32), and tensor pairs
// <base tensor name>.lora_a with ne = [K, r] and <base tensor name>.lora_b with ne = [r, N], both F32 or both F16.
// plan_lora() names every refusal (status -102) without touching a device: tests/host/lora_plan_main.cc prints what it makes of a file.
#pragma once

#include <string>
#include <vector>

#include "gguf.h"
#include "model_plan.h"

namespace mi355 {

constexpr int LORA_RANK_MAX = 512;

// which launch group of the layer forward pass a pair belongs to (host/runtime.cc)
enum LoraTarget : int { LORA_Q = 0, LORA_K, LORA_V, LORA_O, LORA_GATE, LORA_UP, LORA_DOWN, LORA_OUTPUT, LORA_N_TARGETS };

struct LoraPairPlan {
    std::string base;                        // the base tensor's name
    int layer = -1;                          // -1: output.weight
    int target = LORA_OUTPUT;
    int type = 0;                            // T_F32 or T_F16, both halves
    int r = 0;
    int64_t K = 0, N = 0;                    // the base tensor's input width and rows
    const GGUFTensorInfo *a = nullptr, *b = nullptr;
};

struct LoraPlan {
    float alpha = 0.0f;
    std::vector<LoraPairPlan> pairs;         // in the order of the file's lora_a tensors
};

inline float lora_scale(float user_scale, float alpha, int r) { return alpha != 0.0f ? user_scale * alpha / (float)r : user_scale; }

// False with err and status (-102) set when the file is refused.
bool plan_lora(const GGUFFile &f, const ModelLayout &m, LoraPlan &plan, std::string &err, int &status);

}  // namespace mi355
