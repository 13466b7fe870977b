#!/usr/bin/env python3
"""What quantising a file on the device costs: the synthetic `tinyllama-1.1b` as F16 (about 2.2 GB) to q4_k_m and to q2_k with
tools/quantize.py, three passes each, every pass a process of its own under its own time limit; the first failure ends the script.  Per file: the wall time of
quantize_file (median of the passes [smallest, largest]); per destination type the launches' own time between two events, as source GB/s; the share of the
wall time the uploads and the downloads take.  For scale, the numpy twin's seconds for one 2048 x 2048 tensor per type on this host.  There is no parent-commit
counterpart and no threshold.  Synthetic weights: only the times mean anything.
usage: quantize_profile.py [out.json]   (default profiles/quantize.json; the files go to $MI355_BENCH_DIR, default /tmp, as bench.py's)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

CONFIG, FTYPES, PASSES, LIMIT_S = "tinyllama-1.1b", ("q4_k_m", "q2_k"), 3, 300


def med(v):
    return [round(float(np.median(v)), 4), round(float(min(v)), 4), round(float(max(v)), 4)]


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "quantize.json")
    pkg = ge.load_pkg()
    gs = pkg.gguf_synth
    model_dir = os.environ.get("MI355_BENCH_DIR", "/tmp")
    src = os.path.join(model_dir, f"mi355-bench-{CONFIG}-f16.gguf")
    if not os.path.exists(src):
        print("writing the F16 file", flush=True)
        gs.write_synthetic_llama(src + ".tmp", gs.CONFIGS[CONFIG], "f16", seed=0xC0FFEE, with_vocab=False)
        os.replace(src + ".tmp", src)
    res = {"model": f"{CONFIG} f16: gguf_synth.write_synthetic_llama(CONFIGS['{CONFIG}'], 'f16', seed=0xC0FFEE, with_vocab=False), {os.path.getsize(src)} bytes",
           "note": f"{PASSES} passes per mix, each a process of its own; values are [median, smallest, largest] of the passes; wall_s is quantize_file alone "
                   "(reading through a memory map, the device calls, writing), without the interpreter's start and the library load; no threshold",
           "files": {}}
    dst = os.path.join(model_dir, "mi355-quantize-profile-out.gguf")
    for ftype in FTYPES:
        runs = []
        for p in range(PASSES):
            js = dst + ".json"
            cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.join(ROOT, "tools", "quantize.py"), "--json", js, src, dst, ftype]
            t0 = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-2000:], sep="\n")
                print(f"{ftype} pass {p}: exit status {r.returncode}; stopping", flush=True)
                return 1
            info = json.load(open(js))
            info["process_s"] = time.perf_counter() - t0
            runs.append(info)
            print(f"{ftype} pass {p}: {info['wall_s']:.2f} s ({info['process_s']:.2f} s with start-up)", flush=True)
        wall = [r["wall_s"] for r in runs]
        f = {"wall_s": med(wall), "process_s": med([r["process_s"] for r in runs]), "out_bytes": os.path.getsize(dst), "per_type": {}}
        shares = {"kernel": [], "upload": [], "download": []}
        for r in runs:
            for k in shares:
                shares[k].append(sum(t[k + "_ms"] for t in r["per_type"].values()) / 1e3 / r["wall_s"])
        for name in runs[0]["per_type"]:
            sb = runs[0]["per_type"][name]["source_bytes"]
            f["per_type"][name] = {"source_bytes": sb, "calls": runs[0]["per_type"][name]["calls"],
                                   "kernel_ms": med([r["per_type"][name]["kernel_ms"] for r in runs]),
                                   "source_GBps": med([sb / 1e9 / (r["per_type"][name]["kernel_ms"] / 1e3) for r in runs])}
        f["share_of_wall"] = {k: med(v) for k, v in shares.items()}
        rest = 1.0 - sum(f["share_of_wall"][k][0] for k in shares)
        f["share_of_wall"]["file_io_and_host"] = round(rest, 4)
        parts = {"kernel": f["share_of_wall"]["kernel"][0], "copy": f["share_of_wall"]["upload"][0] + f["share_of_wall"]["download"][0], "file_io_and_host": rest}
        f["bound_by"] = max(parts, key=parts.get)
        res["files"][ftype] = f
    import quantize_ref as qr
    x = (np.random.default_rng(1).standard_normal((2048, 2048)) * 0.02).astype(np.float32)
    res["twin_seconds_2048x2048"] = {}
    for t in (qr.Q8_0, qr.Q5_0, qr.Q5_1) + qr.K_TYPES:
        t0 = time.perf_counter()
        qr.quantize_rows(t, x)
        res["twin_seconds_2048x2048"][gs.TYPE_NAME[t]] = round(time.perf_counter() - t0, 3)
    for p in (dst, dst + ".json"):
        if os.path.exists(p):
            os.remove(p)
    with open(out_path, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
    print(json.dumps(res["files"], indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
