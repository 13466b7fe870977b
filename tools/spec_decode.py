#!/usr/bin/env python3
"""What the pieces of a speculative-decoding round cost: target = the benchmark's synthetic Llama-3-8B Q4_K_M, draft = the synthetic
`tinyllama-1.1b` config in Q4_K_M, q8_0 caches, 512 tokens of context.

  us per draft step         one single-token decode of the draft + mi355_get_argmax_prob_ith (logits left on the device)
  us per verify batch, k    one target decode of k + 1 rows, all flagged, + mi355_spec_verify + the roll-back, k = 2, 4, 8, 16
  us per plain target step  one single-token decode + mi355_get_argmax_ith
  break-even acceptance     the per-token acceptance rate a at which a round of k drafts, (k t_draft + t_verify(k)) / ((1 - a^(k+1)) / (1 - a)), costs what plain
                            steps cost per token (drafts accepted independently with probability a; 1 where no rate is enough)

Synthetic weights give no meaningful acceptance, so nothing here is a speed-up: the costs and the rate a real pair would have to reach.
Every figure is the median of passes x reps host-clock timings that end in a synchronise, with its quartiles, extremes and each pass's own median beside it.
usage: spec_decode.py [reps] [out.json]   -> one JSON line on stdout, the same object in out.json (default profiles/spec_decode.json)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_pkg()
gs = pkg.gguf_synth
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 64
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "spec_decode.json")
model_dir = os.environ.get("MI355_BENCH_DIR", "/tmp")
N_PROMPT, KS = 512, (2, 4, 8, 16)


def model_file(cfg_name, ftype):
    path = os.path.join(model_dir, f"mi355-bench-{cfg_name}-{ftype}.gguf")
    if not os.path.exists(path):
        gs.write_synthetic_llama(path + ".tmp", gs.CONFIGS[cfg_name], ftype, seed=0xC0FFEE, with_vocab=False)
        os.replace(path + ".tmp", path)
    return path


pkg.Backend()
target, draft = pkg.Model(model_file("llama-3-8b", "q4_k_m")), pkg.Model(model_file("tinyllama-1.1b", "q4_k_m"))
ct = pkg.Context(target, n_ctx=4096, n_batch=2048, n_ubatch=2048, type_k=8, type_v=8, logits_to_host=False)
cd = pkg.Context(draft, n_ctx=4096, n_batch=2048, n_ubatch=2048, type_k=8, type_v=8, logits_to_host=False)
n_vocab = min(target.n_vocab, draft.n_vocab)
prompt = np.random.default_rng(1234).integers(0, n_vocab, N_PROMPT)
for c in (ct, cd):
    assert c.decode(prompt, np.arange(N_PROMPT)) == 0


def sample_us(fn, n):
    fn(); fn()                                           # warm-up: code objects, the captured step
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()                                             # (every fn ends in a call that synchronises the stream)
        ts.append((time.perf_counter() - t0) * 1e6)
    return ts


def spread(passes):
    """median over all samples, the quartiles and extremes, and each pass's own median (the passes alternate between the measured things)"""
    a = np.concatenate(passes)
    return {"median": round(float(np.median(a)), 1), "p25": round(float(np.percentile(a, 25)), 1), "p75": round(float(np.percentile(a, 75)), 1),
            "min": round(float(a.min()), 1), "max": round(float(a.max()), 1), "pass_medians": [round(float(np.median(p)), 1) for p in passes]}


pos_t, pos_d = [N_PROMPT], [N_PROMPT]                    # the single-token steps advance, as a generation does (no roll-back between them)


def plain_step():
    ct.decode([17], [pos_t[0]]); ct.argmax(); pos_t[0] += 1


def draft_step():
    cd.decode([17], [pos_d[0]]); cd.argmax_prob(); pos_d[0] += 1


def verify(k):
    p0 = pos_t[0]
    toks, pos, flags, gs_, dr = np.full(k + 1, 17, np.int32), np.arange(k + 1) + p0, [1] * (k + 1), [0, k + 1], np.zeros(k + 1, np.int32)

    def fn():                                            # (the roll-back is part of a round: the next batch re-uploads the cell table)
        ct.decode(toks, pos, logits=flags); ct.spec_verify(gs_, dr); ct.kv_seq_rm(0, p0, -1)
    return fn


def break_even(t_round, k, t_plain):
    def per_token(a):
        return t_round / (k + 1 if a >= 1.0 else (1.0 - a ** (k + 1)) / (1.0 - a))
    if per_token(1.0) >= t_plain:
        return 1.0
    lo, hi = 0.0, 1.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if per_token(mid) < t_plain else (mid, hi)
    return hi


N_PASSES = 3
things = [("plain", plain_step), ("draft", draft_step)] + [(k, None) for k in KS]
samples = {name: [] for name, _ in things}
for _ in range(N_PASSES):                                # every pass measures everything once: drift of the box shows as a difference between pass medians
    for name, fn in things:
        if name in KS:
            fn = verify(name)                            # the batch starts where the target's sequence now ends
        samples[name].append(sample_us(fn, reps))
plain, drafted = spread(samples["plain"]), spread(samples["draft"])
t_plain, t_draft = plain["median"], drafted["median"]
row = {"target": "llama-3-8b q4_k_m (synthetic)", "draft": "tinyllama-1.1b q4_k_m (synthetic)", "context_tokens": N_PROMPT, "reps": reps, "passes": N_PASSES,
       "cache": "q8_0", "plain_step_us": plain, "draft_step_us": drafted, "verify": [],
       "note": "costs only: synthetic weights give no meaningful acceptance, no real model pair has been measured; break-even figures carry two digits, "
               "break_even_range: the lowest and the highest figure that a single pass's own medians give"}
for k in KS:
    v = spread(samples[k])
    be_all = [break_even(k * d + t, k, p) for d, t, p in zip(drafted["pass_medians"], v["pass_medians"], plain["pass_medians"])]
    row["verify"].append({"k": k, "verify_batch_us": v, "round_us": round(k * t_draft + v["median"], 1),
                          "break_even_acceptance": round(break_even(k * t_draft + v["median"], k, t_plain), 2),
                          "break_even_range": [round(min(be_all), 2), round(max(be_all), 2)]})
print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(row, f, indent=1)
    f.write("\n")
ct.close(); cd.close(); target.close(); draft.close()
