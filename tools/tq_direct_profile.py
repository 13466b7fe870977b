#!/usr/bin/env python3
"""Prompt rate and device memory of a dense ternary file on its two routes (profiles/tq_direct.json): the kernel on the packed trits
(csrc/mmq_ternary.hip, the default) and the plane sets (MI355_TQ_DIRECT=0), each in a fresh process, taking turns.  Synthetic TQ2_0 and TQ1_0 files of
--config (default tiny-8b-3l: three layers of Llama-3-8B's geometry, 512-token vocabulary), a 512-token prompt, q8_0 cache.  Medians of --passes passes
with the smallest and the largest.

  tq_direct_profile.py [--config tiny-8b-3l] [--passes 3] [--reps 8] [--json OUT]
  tq_direct_profile.py --one --ftype tq2_0       one pass on the route the environment names, one JSON line"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PROMPT = 512


def load_pkg():
    spec = importlib.util.spec_from_file_location("_graft_entry_tq", os.path.join(HERE, "__graft_entry__.py"))
    ge = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ge)
    return ge.load_pkg()


def one_pass(cfg, ftype, reps):
    """the prompt from an empty cache: one warm-up, then `reps` timed prompts between two synchronisations"""
    pkg = load_pkg()
    gs = pkg.gguf_synth
    path = os.path.join(os.environ.get("MI355_BENCH_DIR", "/tmp"), f"mi355-tq-{cfg}-{ftype}.gguf")
    if not os.path.exists(path):
        gs.write_synthetic_llama(path + f".tmp{os.getpid()}", gs.CONFIGS[cfg], ftype, seed=0xC0FFEE, with_vocab=False)
        os.replace(path + f".tmp{os.getpid()}", path)
    model = pkg.Model(path)
    ctx = pkg.Context(model, n_ctx=1024, n_batch=512, n_ubatch=512, type_k=8, type_v=8)
    prompt = np.random.default_rng(1234).integers(0, model.n_vocab, N_PROMPT)

    def run():
        ctx.kv_clear()
        assert ctx.decode(prompt, np.arange(N_PROMPT)) == 0

    run(); ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    ctx.synchronize()
    dt = (time.perf_counter() - t0) / reps
    out = {"ftype": ftype, "direct": os.environ.get("MI355_TQ_DIRECT", "1") != "0", "prompt_tok_s": round(N_PROMPT / dt, 1), "vram": model.vram, "size": model.size,
           "planes_bytes": model.planes_bytes}
    ctx.close(); model.close()
    return out


def summary(xs):
    return {"median": round(statistics.median(xs), 1), "min": round(min(xs), 1), "max": round(max(xs), 1), "passes": xs}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--ftype", default="tq2_0")
    ap.add_argument("--config", default="tiny-8b-3l")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one_pass(a.config, a.ftype, a.reps)), flush=True)
        return 0
    report = {"model": f"{a.config} (synthetic)", "cache": "q8_0", "prompt_tokens": N_PROMPT, "passes": a.passes, "prompts_per_pass": a.reps, "routes": {}}
    for ftype in ("tq2_0", "tq1_0"):
        rows = {"direct": [], "planes": []}
        for _ in range(a.passes):
            for route in ("direct", "planes"):
                env = dict(os.environ, MI355_TQ_DIRECT="1" if route == "direct" else "0")
                r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--one", "--ftype", ftype, "--config", a.config, "--reps", str(a.reps)],
                                   capture_output=True, text=True, env=env)
                if r.returncode != 0:
                    print(r.stdout + r.stderr, file=sys.stderr)
                    return 1
                rows[route].append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(ftype, route, rows[route][-1], flush=True)
        report["routes"][ftype] = {route: dict(prompt_tok_s=summary([x["prompt_tok_s"] for x in v]), vram=v[0]["vram"], planes_bytes=v[0]["planes_bytes"], file_tensor_bytes=v[0]["size"])
                                   for route, v in rows.items()}
    print(json.dumps(report, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
