// tests/host/sample_vocab_host_tests.cc — CPU checks of what the slot loop asks a Sampler before it sends a slot to the whole-row device sampler
// (host/sampling.h device_vocab_ok, plan_adjust) and of the mirostat-2 mu update from a returned probability.  Built and run by tests/test_sample_vocab_host.py.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../cortex.llamacpp_amd/host/sampling.h"

using namespace mi355;

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); g_fail++; } } while (0)

int main() {
    struct Case { int top_k, mirostat, n_probs; float temp, typ_p, dynatemp, top_p; bool want; };
    const Case cases[] = {
        {0, 0, 0, 0.8f, 1.0f, 0.0f, 0.95f, true},    {-1, 0, 0, 0.8f, 1.0f, 0.0f, 0.95f, true},  {129, 0, 0, 0.8f, 1.0f, 0.0f, 0.95f, true},
        {40, 2, 0, 0.8f, 1.0f, 0.0f, 0.95f, true},   {0, 2, 0, 0.8f, 1.0f, 0.0f, 7.0f, true},    // (mirostat 2 does not read top_p)
        {40, 0, 0, 0.8f, 1.0f, 0.0f, 0.95f, false},  {128, 0, 0, 0.8f, 1.0f, 0.0f, 0.95f, false}, // the front's
        {0, 1, 0, 0.8f, 1.0f, 0.0f, 0.95f, false},   {0, 0, 3, 0.8f, 1.0f, 0.0f, 0.95f, false},  {0, 0, 0, 0.0f, 1.0f, 0.0f, 0.95f, false},
        {0, 0, 0, 0.8f, 0.5f, 0.0f, 0.95f, false},   {0, 0, 0, 0.8f, 1.0f, 0.5f, 0.95f, false},  {0, 0, 0, 0.8f, 1.0f, 0.0f, 1.5f, false},
        {0, 2, 0, 0.8f, 0.5f, 0.0f, 0.95f, false},
    };
    for (const Case &c : cases) {
        SamplingParams p;
        p.top_k = c.top_k; p.mirostat = c.mirostat; p.n_probs = c.n_probs; p.temp = c.temp; p.typ_p = c.typ_p; p.dynatemp_range = c.dynatemp; p.top_p = c.top_p;
        CHECK(Sampler(p).device_vocab_ok(128) == c.want);
    }
    {   // the adjustments: one bias per token, at most max_adj tokens; mirostat does not stand in the way as it does for plan_front
        SamplingParams p;
        p.mirostat = 2; p.penalty_repeat = 1.2f; p.logit_bias = {{3, 1.0f}, {900, 2.0f}};
        Sampler s(p);
        s.accept(3); s.accept(5); s.accept(5);
        Sampler::FrontPlan a, f;
        CHECK(s.plan_adjust(100, 192, a) && !s.plan_front(100, 128, 192, f));
        CHECK(a.tok == std::vector<int32_t>({3, 5}) && a.bias == std::vector<float>({1.0f, 0.0f}) && a.cnt == std::vector<int32_t>({1, 2}));
        CHECK(!s.plan_adjust(100, 1, a));
        p.logit_bias.push_back({3, 0.5f});
        CHECK(!Sampler(p).plan_adjust(100, 192, a));
    }
    {   // mu after a probability the device returned = mu after the host branch drew the same token with that probability
        SamplingParams p;
        p.mirostat = 2; p.temp = 0.7f; p.seed = 9; p.mirostat_tau = 3.0f; p.mirostat_eta = 0.2f;
        std::vector<float> row(64);
        for (int i = 0; i < 64; i++) row[(size_t)i] = 0.1f * (float)((i * 37) % 64);
        Sampler host(p), dev(p);
        for (int step = 0; step < 4; step++) {
            const int32_t t = host.sample(row.data(), 64);
            float pt = -1.0f;
            for (const TokenProb &c : host.candidates()) if (c.tok == t) pt = c.p;
            CHECK(pt > 0.0f);
            dev.set_device_result_mirostat(t, pt);
            CHECK(dev.device_mu() == host.device_mu() && dev.device_draw() == (uint64_t)step + 1);
        }
        CHECK(host.device_mu() != 2.0f * p.mirostat_tau);
    }
    if (g_fail == 0) printf("all whole-row sampler host checks passed\n");
    return g_fail ? 1 : 0;
}
