#!/usr/bin/env python3
"""What collecting an importance matrix costs: on the benchmark's synthetic Llama-3-8B Q4_K_M file, q8_0 cache, 8 chunks of 512 tokens,
n_ubatch 512, three passes each of
  perplexity        tools/perplexity.py of this tree (collection off: the path the collector does not touch)
  imatrix           tools/imatrix.py (collection on, the chunks through Context.perplexity)
  imatrix_no_ppl    tools/imatrix.py --no-ppl (plain decode calls without logits)
  parent_perplexity tools/perplexity.py of another checkout with its own built library (--parent-tree DIR), when one is given
every run in a process of its own under its own time limit; the first failure ends the script.  A pass gives the median of its per-chunk host-clock times
(the first chunk holds the warm-up); a case reports the median of its three passes and their smallest and largest.  Then, in this process, one 512-token
chunk with the per-launch-group event timing on (mi355_profile_last_decode), collection off and on: the "imatrix" and "imatrix_glu" roles are the collector launches' own time
(the runtime sets a "rows" mark in front of each, so the launches that produced the rows are not counted), the rest of the difference is what the forced unfused
routes add.  Synthetic weights and random tokens: only the times mean anything.
usage: imatrix_profile.py [--parent-tree DIR] [out.json]   (default profiles/imatrix.json; the model file goes to $MI355_BENCH_DIR, default /tmp, as bench.py's)"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

CONFIG, FTYPE, N_CHUNKS, N_CHUNK, TOKEN_SEED, LIMIT_S, PASSES = "llama-3-8b", "q4_k_m", 8, 512, 1234, 300, 3


def main():
    argv = sys.argv[1:]
    parent = None
    if "--parent-tree" in argv:
        i = argv.index("--parent-tree")
        parent = os.path.abspath(argv[i + 1])
        del argv[i:i + 2]
    out_path = argv[0] if argv else os.path.join(ROOT, "profiles", "imatrix.json")
    pkg = ge.load_pkg()
    gs = pkg.gguf_synth
    model_dir = os.environ.get("MI355_BENCH_DIR", "/tmp")
    name = f"mi355-bench-{CONFIG}-{FTYPE}.gguf"
    path = os.path.join(model_dir, name)
    if not os.path.exists(path):
        print("writing the model file", flush=True)
        gs.write_synthetic_llama(path + ".tmp", gs.CONFIGS[CONFIG], FTYPE, seed=0xC0FFEE, with_vocab=False)
        os.replace(path + ".tmp", path)

    res = {"model": f"{CONFIG} {FTYPE}: gguf_synth.write_synthetic_llama(CONFIGS['{CONFIG}'], '{FTYPE}', seed=0xC0FFEE, with_vocab=False), bench.py's file",
           "tokens": f"numpy.random.default_rng({TOKEN_SEED}).integers(0, {gs.CONFIGS[CONFIG].n_vocab}, {N_CHUNKS * N_CHUNK}).astype(int32)",
           "note": f"{PASSES} passes per case, each a process of its own; a pass = the median of its {N_CHUNKS} per-chunk host-clock times (the first chunk holds the "
                   "warm-up); ms_per_chunk = median of the passes, with their smallest and largest; no threshold", "commands": {}, "cases": {}}
    tokens = np.random.default_rng(TOKEN_SEED).integers(0, gs.CONFIGS[CONFIG].n_vocab, N_CHUNKS * N_CHUNK).astype(np.int32)
    with tempfile.TemporaryDirectory() as td:
        tok = os.path.join(td, "tokens.npy")
        np.save(tok, tokens)
        common = ["-m", path, "--tokens", tok, "--ctx", str(N_CHUNK), "--ubatch", str(N_CHUNK), "--cache-type", "q8_0", "--chunks", str(N_CHUNKS)]
        cases = [("perplexity", ROOT, "perplexity.py", []), ("imatrix", ROOT, "imatrix.py", ["-o", os.path.join(td, "im.gguf")]),
                 ("imatrix_no_ppl", ROOT, "imatrix.py", ["-o", os.path.join(td, "im2.gguf"), "--no-ppl"])]
        if parent:
            cases.insert(0, ("parent_perplexity", parent, "perplexity.py", []))
        times = {case: [] for case, _, _, _ in cases}
        for p in range(PASSES):                                    # the cases alternate within a pass, so a drift of the machine touches all alike
            for case, tree, tool, extra in cases:
                passes = times[case]
                js = os.path.join(td, f"{case}{p}.json")
                args = common + extra + ["--json", js]
                res["commands"][case] = f"python tools/{tool} " + " ".join(a.replace(path, name).replace(td + os.sep, "") for a in args[:-2])
                r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.join(tree, "tools", tool)] + args, capture_output=True, text=True, cwd=tree)
                if r.returncode != 0:
                    print(r.stdout[-600:], r.stderr[-600:], flush=True)
                    sys.exit(r.returncode)
                passes.append(json.load(open(js))["seconds_per_chunk_median"] * 1e3)
                print(f"{case} pass {p}: {passes[-1]:.2f} ms per chunk", flush=True)
        for case, passes in times.items():
            res["cases"][case] = {"ms_per_chunk": round(float(np.median(passes)), 3), "min": round(min(passes), 3), "max": round(max(passes), 3), "passes": [round(x, 3) for x in passes]}

    # the split: one chunk under the event timing, collection off and on (the second chunk of each: the first holds the warm-up)
    pkg.Backend()
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=N_CHUNK, n_batch=N_CHUNK, n_ubatch=N_CHUNK, type_k=8, type_v=8, logits_to_host=False)
    c.profile(True)
    flags = np.zeros(N_CHUNK, np.int8)
    flags[N_CHUNK // 2:N_CHUNK - 1] = 1

    def chunk_profile():
        prof = None
        for k in range(2):
            c.kv_seq_rm(0, 0, -1)
            assert c.decode(tokens[k * N_CHUNK:(k + 1) * N_CHUNK], np.arange(N_CHUNK), logits=flags) == 0
            c.synchronize()
            prof = c.last_profile()
        return {k: round(v, 1) for k, v in prof.items() if k[:2] not in ("k:", "n:")}      # the launch groups; the per-kernel "k:" / "n:" entries overlap them

    off = chunk_profile()
    c.imatrix_begin(False)
    on = chunk_profile()
    c.imatrix_end()
    c.close(); m.close()
    t_off, t_on, t_col = sum(off.values()), sum(on.values()), sum(v for k, v in on.items() if k.startswith("imatrix"))
    res["split_us_per_chunk"] = {"note": "event time per launch group of one 512-token chunk (mi355_profile_last_decode): serialised by the events, so the totals sit "
                                         "above the unprofiled chunk times; collector = the 'imatrix' roles, routes = total_on - collector - total_off",
                                 "off": off, "on": on, "total_off": round(t_off, 1), "total_on": round(t_on, 1), "collector": round(t_col, 1),
                                 "routes": round(t_on - t_col - t_off, 1)}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"cases": {k: v["ms_per_chunk"] for k, v in res["cases"].items()}, "split": {k: res["split_us_per_chunk"][k] for k in ("total_off", "total_on", "collector", "routes")}}))


if __name__ == "__main__":
    main()
