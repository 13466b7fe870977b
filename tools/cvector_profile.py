#!/usr/bin/env python3
"""What a control vector costs (profiles/control_vector.json), on the benchmark's synthetic Llama-3-8B Q4_K_M model with a q8_0 cache behind a
512-token prompt: microseconds per single-token step without a vector, with a vector on all layers and on layers 10 - 20, and milliseconds per layer of the
generator's power method at R = 512, E = 4096, 1000 iterations.  Medians of --passes passes, with the smallest and the largest.

  cvector_profile.py [--steps 256] [--passes 3] [--parent-tree DIR] [--json OUT]
  cvector_profile.py --plain [--tree DIR]          one pass of the step without a vector, one JSON line - the mode that also runs on a checkout without vectors

--parent-tree: another checkout of the project, built (the parent commit).  Its --plain pass and this tree's then run in child processes of their own, taking
turns, --passes times each; the report holds both series and whether this tree's median lies within the spread the parent shows against itself.  The model
file is the one bench.py writes (MI355_BENCH_DIR, default /tmp)."""
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
CFG, FTYPE, N_PROMPT = "llama-3-8b", "q4_k_m", 512


def load_pkg(tree):
    spec = importlib.util.spec_from_file_location("_graft_entry_" + str(abs(hash(tree))), os.path.join(tree, "__graft_entry__.py"))
    ge = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ge)
    return ge.load_pkg()


def open_model(pkg):
    gs = pkg.gguf_synth
    path = os.path.join(os.environ.get("MI355_BENCH_DIR", "/tmp"), f"mi355-bench-{CFG}-{FTYPE}.gguf")
    if not os.path.exists(path):
        gs.write_synthetic_llama(path + f".tmp{os.getpid()}", gs.CONFIGS[CFG], FTYPE, seed=0xC0FFEE, with_vocab=False)
        os.replace(path + f".tmp{os.getpid()}", path)
    model = pkg.Model(path)
    return model, pkg.Context(model, n_ctx=4096, n_batch=2048, n_ubatch=2048, type_k=8, type_v=8)


def step_us(model, ctx, steps):
    """one pass: the prompt from an empty cache, 16 steps of warm-up, then `steps` timed single-token steps between two synchronisations"""
    ctx.kv_clear()
    prompt = np.random.default_rng(1234).integers(0, model.n_vocab, N_PROMPT)
    assert ctx.decode(prompt, np.arange(N_PROMPT)) == 0
    tok, pos = ctx.argmax(), N_PROMPT
    for _ in range(16):
        ctx.decode([tok], [pos]); ctx.logits_ready(); tok = ctx.argmax(); pos += 1
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ctx.decode([tok], [pos]); ctx.logits_ready(); tok = ctx.argmax(); pos += 1
    ctx.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def summary(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2), "passes": [round(x, 2) for x in xs]}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--parent-tree")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--json")
    a = ap.parse_args()
    if a.plain:
        pkg = load_pkg(os.path.abspath(a.tree))
        model, ctx = open_model(pkg)
        print(json.dumps({"tree": os.path.abspath(a.tree), "steps": a.steps, "us_per_step": round(step_us(model, ctx, a.steps), 2)}), flush=True)
        ctx.close(); model.close()
        return 0

    report = {"model": f"{CFG} {FTYPE} (synthetic)", "cache": "q8_0", "prompt_tokens": N_PROMPT, "steps": a.steps, "passes": a.passes}
    if a.parent_tree:
        series = {"parent": [], "this": []}
        for _ in range(a.passes):
            for name, tree in (("parent", os.path.abspath(a.parent_tree)), ("this", HERE)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain", "--tree", tree, "--steps", str(a.steps)], capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    print(r.stdout + r.stderr, file=sys.stderr)
                    return 1
                series[name].append(json.loads(r.stdout.strip().splitlines()[-1])["us_per_step"])
                print(name, series[name][-1], flush=True)
        spread = max(series["parent"]) - min(series["parent"])
        diff = statistics.median(series["this"]) - statistics.median(series["parent"])
        report["step_no_vector_us"] = {"parent_commit": summary(series["parent"]), "this_commit": summary(series["this"]), "parent_spread": round(spread, 2),
                                       "median_difference": round(diff, 2), "within_parent_spread": bool(abs(diff) <= spread)}

    pkg = load_pkg(HERE)
    be = pkg.Backend()
    model, ctx = open_model(pkg)
    L, E = model.n_layer, model.n_embd
    vec = (np.random.default_rng(7).standard_normal((L - 1, E)) * 0.1).astype(np.float32)
    rows = {}
    for name, rng in (("no vector", None), ("all layers", (1, L)), ("layers 10 - 20", (10, 20))):
        if rng:
            ctx.apply_cvec(vec, *rng)
        else:
            ctx.clear_cvec()
        rows[name] = [step_us(model, ctx, a.steps) for _ in range(a.passes)]
        print(name, rows[name], flush=True)
    ctx.clear_cvec()
    n_extra = {"no vector": 0, "all layers": L - 1, "layers 10 - 20": 11}
    report["step_us"] = {k: dict(summary(v), extra_launches_per_step=n_extra[k]) for k, v in rows.items()}
    for k in ("all layers", "layers 10 - 20"):
        extra = report["step_us"][k]["median"] - report["step_us"]["no vector"]["median"]
        report["step_us"][k]["extra_us_per_step"] = round(extra, 2)
        report["step_us"][k]["extra_us_per_launch"] = round(extra / n_extra[k], 3)
    ctx.close(); model.close()

    R, iters = 512, 1000
    g = np.random.default_rng(11)
    u = g.standard_normal(E); u /= np.linalg.norm(u)
    D = ((1.0 + np.abs(g.standard_normal(R)))[:, None] * u[None, :] + 0.05 * g.standard_normal((R, E))).astype(np.float32)
    b0 = g.standard_normal(E).astype(np.float32)
    be.cvec_direction(D, b0, "pca", 10, 10, 0.0)                        # (warm-up)
    ms = []
    for _ in range(a.passes):
        t0 = time.perf_counter()
        _, n_done, _ = be.cvec_direction(D, b0, "pca", iters, 100, 0.0)
        ms.append((time.perf_counter() - t0) * 1e3)
        assert n_done == iters
    report["pca_ms_per_layer"] = dict(summary(ms), rows=R, n_embd=E, iterations=iters, launches=3 * iters + 2, includes="upload of the rows, the iterations, download")
    print(json.dumps(report, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
