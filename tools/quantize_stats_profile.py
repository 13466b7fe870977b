#!/usr/bin/env python3
"""What the per-tensor error statistics cost on the device: tools/quantize_stats.py on the synthetic `tinyllama-1.1b` as F16 (the file of
tools/quantize_profile.py) for q4_k and q6_k, three passes, every pass a process of its own under its own time limit; the first failure ends the script.  The
wall time of the run (median of the passes [smallest, largest]); per type the error launches' own time between two events as source GB/s, next to the
quantiser's figures of profiles/quantize.json.  Then the decode launch alone on 2048 x 5632 rows of Q4_K, Q6_K and Q8_0 to F32 and to F16, as block bytes and
as written bytes per second.  No parent-commit counterpart, no threshold.  Synthetic weights: only the times mean anything.
usage: quantize_stats_profile.py [out.json]   (default profiles/quantize_stats.json; the file goes to $MI355_BENCH_DIR, default /tmp, as bench.py's)"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

CONFIG, TYPES, PASSES, LIMIT_S = "tinyllama-1.1b", ("q4_k", "q6_k"), 3, 300


def med(v):
    return [round(float(np.median(v)), 4), round(float(min(v)), 4), round(float(max(v)), 4)]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "quantize_stats.json")
    pkg = ge.load_pkg()
    gs = pkg.gguf_synth
    model_dir = os.environ.get("MI355_BENCH_DIR", "/tmp")
    src = os.path.join(model_dir, f"mi355-bench-{CONFIG}-f16.gguf")
    if not os.path.exists(src):
        print("writing the F16 file", flush=True)
        gs.write_synthetic_llama(src + ".tmp", gs.CONFIGS[CONFIG], "f16", seed=0xC0FFEE, with_vocab=False)
        os.replace(src + ".tmp", src)
    res = {"model": f"{CONFIG} f16: gguf_synth.write_synthetic_llama(CONFIGS['{CONFIG}'], 'f16', seed=0xC0FFEE, with_vocab=False), {os.path.getsize(src)} bytes",
           "note": f"{PASSES} passes, each a process of its own; values are [median, smallest, largest] of the passes; wall_s is stats_file alone (reading through "
                   "a memory map, the quantiser's and the error entry's device calls), without the interpreter's start and the library load; no threshold"}
    js, runs = os.path.join(model_dir, "mi355-quantize-stats-profile.json"), []
    for p in range(PASSES):
        cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.join(ROOT, "tools", "quantize_stats.py"), "-m", src, "--json", js]
        r = subprocess.run(cmd + [a for t in TYPES for a in ("--type", t)], capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-2000:], sep="\n")
            print(f"pass {p}: exit status {r.returncode}; stopping", flush=True)
            return 1
        runs.append(json.load(open(js)))
        print(f"pass {p}: {runs[-1]['wall_s']:.2f} s", flush=True)
    os.remove(js)
    res["stats"] = {"types": list(TYPES), "wall_s": med([r["wall_s"] for r in runs]), "rel_rms": {k: v["rel_rms"] for k, v in runs[0]["types"].items()}, "error": {}}
    for name, st in runs[0]["error_calls"].items():
        res["stats"]["error"][name] = {"source_bytes": st["source_bytes"], "calls": st["calls"], "kernel_ms": med([r["error_calls"][name]["kernel_ms"] for r in runs]),
                                       "source_GBps": med([st["source_bytes"] / 1e9 / (r["error_calls"][name]["kernel_ms"] / 1e3) for r in runs]),
                                       "upload_ms": med([r["error_calls"][name]["upload_ms"] for r in runs])}
    be = pkg.Backend()
    rows, n = 5632, 2048
    res["decode"] = {"shape": [rows, n]}
    for t in (gs.Q4_K, gs.Q6_K, gs.Q8_0):
        raw = gs.random_blocks(np.random.default_rng(t), t, rows * n, 0.02)
        for dst in ("f32", "f16"):
            ms = []
            for _ in range(PASSES + 1):                      # the first call carries the kernel's load
                be.dequantize_rows(raw, t, n, dst=dst)
                ms.append(be.quant_error_last_times()[1])
            res["decode"][f"{gs.TYPE_NAME[t]}->{dst}"] = {"kernel_ms": med(ms[1:]), "block_GBps": med([raw.nbytes / 1e6 / m for m in ms[1:]]),
                                                           "written_GBps": med([rows * n * (4 if dst == "f32" else 2) / 1e6 / m for m in ms[1:]])}
    with open(out_path, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
