#!/usr/bin/env python3
"""Prompt-lookup drafting against plain greedy steps in one run.

  lookup    mi355_lookup_steps over the prompt: tokens per round, acceptance (accepted / drafted), us per emitted token
  greedy    mi355_greedy_steps on the same prompt, same context, same number of tokens: us per token
  kernel_us ngram_draft_kernel's own time at history lengths 512, 8192 and 131072, from a kernel trace taken in a run of its own:
                rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/lookup_decode.py --kernels
                python tools/lookup_decode.py --parse DIR/.../*_kernel_trace.csv        (adds "kernel_us" to the JSON file)
            --kernels launches mi355_op_ngram_draft KERNEL_REPS times per length (random ids over a 32000-token vocabulary: the common miss, no 16-token repeat).

Default model: the benchmark's synthetic Llama-3-8B Q4_K_M; default prompt: a random 128-token block four times over (512 tokens).  A synthetic model's
acceptance says nothing about real text: its output does not follow the prompt.  The figures that carry over are the costs: a round's time against a plain
step's, and with them the tokens per round at which lookup pays.
Step figures are the median of three passes with the smallest and the largest beside it; the passes alternate between lookup and greedy.
usage: lookup_decode.py [model.gguf] [prompt file: text, or token ids separated by blanks] [n tokens] [out.json]"""
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
args = sys.argv[1:]
n_tokens = int(args[2]) if len(args) > 2 else 128
out_path = args[3] if len(args) > 3 else os.path.join(ROOT, "profiles", "lookup_decode.json")
model_dir = os.environ.get("MI355_BENCH_DIR", "/tmp")
N_PASSES, NGRAM, K = 3, (2, 4), 8
KERNEL_LENS, KERNEL_REPS = (512, 8192, 131072), 40       # (the first 8 launches of a length are warm-up)


def synthetic(cfg_name, ftype):
    path = os.path.join(model_dir, f"mi355-bench-{cfg_name}-{ftype}.gguf")
    if not os.path.exists(path):
        gs.write_synthetic_llama(path + ".tmp", gs.CONFIGS[cfg_name] if cfg_name in gs.CONFIGS else cfg_name, ftype, seed=0xC0FFEE, with_vocab=False)
        os.replace(path + ".tmp", path)
    return path


def spread(v):
    return {"median": round(float(np.median(v)), 1), "min": round(float(min(v)), 1), "max": round(float(max(v)), 1)}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()                                             # (both loops end in a call that synchronises the stream)
    return r, (time.perf_counter() - t0) * 1e6


def run(ctx, prompt, n, ngram, k):
    """N_PASSES alternating passes of lookup_steps and greedy_steps behind the same prompt; the context is rolled back to the prompt between them"""
    assert ctx.decode(prompt, np.arange(prompt.size)) == 0
    first = ctx.argmax()
    us_l, us_g, stats, same = [], [], None, 0
    for p in range(N_PASSES + 1):                        # pass 0 warms up: code objects, the captured step
        (toks, stats), t_l = timed(lambda: ctx.lookup_steps(prompt, first, prompt.size, n, ngram_min=ngram[0], ngram_max=ngram[1], n_max=k))
        ctx.kv_seq_rm(0, prompt.size, -1)
        greedy, t_g = timed(lambda: ctx.greedy_steps(first, prompt.size, n))
        ctx.kv_seq_rm(0, prompt.size, -1)
        same = int((toks == greedy).sum())
        if p:
            us_l.append(t_l); us_g.append(t_g)
    return us_l, us_g, stats, same


if args[:1] == ["--parse"]:
    import csv
    out_path = args[2] if len(args) > 2 else out_path
    rows = sorted((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                  for r in csv.DictReader(open(args[1])) if "ngram_draft_kernel" in r["Kernel_Name"])
    assert len(rows) == len(KERNEL_LENS) * KERNEL_REPS, len(rows)
    row = json.load(open(out_path))
    row["kernel_us"] = {str(n): spread([d for _, d in rows[i * KERNEL_REPS + 8:(i + 1) * KERNEL_REPS]]) for i, n in enumerate(KERNEL_LENS)}
    row["kernel_us"]["source"] = f"kernel trace, {KERNEL_REPS - 8} launches per length: median, smallest, largest"
    print(json.dumps(row["kernel_us"]))
    with open(out_path, "w") as f:
        json.dump(row, f, indent=1)
        f.write("\n")
    sys.exit(0)
be = pkg.Backend()
if args[:1] == ["--kernels"]:
    for n in KERNEL_LENS:
        hist = np.random.default_rng(n).integers(0, 32000, (1, n)).astype(np.int32)
        for _ in range(KERNEL_REPS):
            be.ngram_draft(hist, [n], 16, 16, 16)
    sys.exit(0)
model = pkg.Model(args[0] if args else synthetic("llama-3-8b", "q4_k_m"))
if len(args) > 1:
    text = open(args[1]).read()
    prompt = np.array([int(t) for t in text.split()] if text.replace(" ", "").replace("\n", "").isdigit() else model.tokenize(text), np.int32)
else:
    prompt = np.tile(np.random.default_rng(1234).integers(0, model.n_vocab, 128), 4).astype(np.int32)
ctx = pkg.Context(model, n_ctx=int(prompt.size + n_tokens + 64), n_batch=2048, n_ubatch=2048, type_k=8, type_v=8, logits_to_host=False)
us_l, us_g, stats, same = run(ctx, prompt, n_tokens, NGRAM, K)
rounds, drafted, accepted, plain = (int(x) for x in stats)
row = {"model": os.path.basename(args[0]) if args else "llama-3-8b q4_k_m (synthetic)", "prompt_tokens": int(prompt.size), "tokens": n_tokens, "passes": N_PASSES,
       "cache": "q8_0", "ngram": list(NGRAM), "draft_max": K, "rounds": rounds, "drafted": drafted, "accepted": accepted, "plain_steps": plain,
       "tokens_per_round": round(n_tokens / max(rounds, 1), 2), "acceptance": round(accepted / drafted, 3) if drafted else None,
       "tokens_equal_to_greedy": same,
       "lookup_us_per_token": spread([t / n_tokens for t in us_l]), "greedy_us_per_token": spread([t / n_tokens for t in us_g]),
       "lookup_us_per_round": spread([t / max(rounds, 1) for t in us_l]),
       "note": "synthetic weights: the acceptance says nothing about real text (the output does not follow the prompt); the costs carry over"}
ctx.close(); model.close()

print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(row, f, indent=1)
    f.write("\n")
