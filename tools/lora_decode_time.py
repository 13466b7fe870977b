#!/usr/bin/env python3
"""What a LoRA adapter costs at run time: single-stream decode tok/s and 512-token prompt tok/s of the benchmark's synthetic Llama-3-8B Q4_K_M model
without an adapter, with a rank-16 F16 adapter on all seven layer tensors, and with the same adapter on attn_q and attn_v only.

usage: lora_decode_time.py [steps] [out.json]    -> one JSON line per configuration on stdout, and the three of them as a list in out.json
(the numbers of profiles/lora_decode.json and DESIGN.md §4.4).  The model file is the one bench.py writes (MI355_BENCH_DIR, default /tmp)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_pkg()
gs = pkg.gguf_synth
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 128
out_path = sys.argv[2] if len(sys.argv) > 2 else None
model_dir = os.environ.get("MI355_BENCH_DIR", "/tmp")
cfg_name, ftype, n_prompt, rank = "llama-3-8b", "q4_k_m", 512, 16
ALL7 = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")

path = os.path.join(model_dir, f"mi355-bench-{cfg_name}-{ftype}.gguf")
if not os.path.exists(path):
    gs.write_synthetic_llama(path + ".tmp", gs.CONFIGS[cfg_name], ftype, seed=0xC0FFEE, with_vocab=False)
    os.replace(path + ".tmp", path)
model = pkg.Model(path)
ctx = pkg.Context(model, n_ctx=4096, n_batch=2048, n_ubatch=2048, type_k=8, type_v=8)


def decode_tok_s():
    ctx.kv_clear()
    prompt = np.random.default_rng(1234).integers(0, model.n_vocab, n_prompt)
    assert ctx.decode(prompt, np.arange(n_prompt)) == 0
    tok, pos = ctx.argmax(), n_prompt
    for _ in range(16):
        ctx.decode([tok], [pos]); ctx.logits_ready(); tok = ctx.argmax(); pos += 1
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ctx.decode([tok], [pos]); ctx.logits_ready(); tok = ctx.argmax(); pos += 1
    ctx.synchronize()
    return steps / (time.perf_counter() - t0)


def prefill_tok_s(reps=5):
    prompt = np.random.default_rng(99).integers(0, model.n_vocab, n_prompt)
    ts = []
    for _ in range(reps + 1):                        # (the first pass warms up)
        ctx.kv_clear(); ctx.synchronize()
        t0 = time.perf_counter()
        assert ctx.decode(prompt, np.arange(n_prompt)) == 0
        ctx.logits_ready()
        ts.append(time.perf_counter() - t0)
    return n_prompt / sorted(ts[1:])[reps // 2]


rows = []
for name, targets in (("no adapter", None), ("rank-16 f16, all seven layer tensors", ALL7), ("rank-16 f16, attn_q and attn_v", ("attn_q", "attn_v"))):
    adapter = None
    if targets:
        apath = os.path.join(model_dir, f"mi355-bench-lora-r{rank}-{len(targets)}.gguf")
        gs.write_synthetic_lora(apath, cfg_name, rank=rank, alpha=2.0 * rank, targets=targets, dtype="f16", std=0.02)
        adapter = pkg.LoraAdapter(model, apath)
        ctx.set_adapter_lora(adapter, 1.0)
    row = {"config": name, "model": f"{cfg_name} {ftype} (synthetic)", "decode_tok_s": round(decode_tok_s(), 1), "prefill_tok_s": round(prefill_tok_s(), 0),
           "steps": steps, "prompt_tokens": n_prompt, "adapter_bytes": os.path.getsize(apath) if targets else 0}
    rows.append(row)
    print(json.dumps(row), flush=True)
    if adapter:
        ctx.clear_adapter_lora()
        adapter.close()
        os.remove(apath)
for r in rows[1:]:
    r["decode_ratio_to_base"] = round(r["decode_tok_s"] / rows[0]["decode_tok_s"], 3)
    r["prefill_ratio_to_base"] = round(r["prefill_tok_s"] / rows[0]["prefill_tok_s"], 3)
if out_path:
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
ctx.close(); model.close()
