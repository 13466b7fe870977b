#!/usr/bin/env python3
"""What a perplexity run costs with the scoring on the device and on the host: tools/perplexity.py on the benchmark's synthetic Llama-3-8B
Q4_K_M file, q8_0 cache, 8 chunks of 512 tokens, n_ubatch 512, in four modes - device, --host-score, and both again with --base (the SAME file loaded a second
time as the base: every KL is 0, the cost is that of a real base of this size).  Each mode is one run in a process of its own under its own time limit; the
first failure ends the script.  The tokens are numpy.random.default_rng(1234).integers(0, n_vocab, 8 * 512); synthetic weights and random tokens, so the
perplexity means nothing and only the modes agreeing does.
usage: perplexity_profile.py [out.json]   (default profiles/perplexity.json; the model file is written to $MI355_BENCH_DIR, default /tmp, as bench.py does)"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

CONFIG, FTYPE, N_CHUNKS, N_CHUNK, TOKEN_SEED, LIMIT_S = "llama-3-8b", "q4_k_m", 8, 512, 1234, 300
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "perplexity.json")
gs = ge.load_pkg().gguf_synth
model_dir = os.environ.get("MI355_BENCH_DIR", "/tmp")
name = f"mi355-bench-{CONFIG}-{FTYPE}.gguf"
path = os.path.join(model_dir, name)
if not os.path.exists(path):
    print("writing the model file", flush=True)
    gs.write_synthetic_llama(path + ".tmp", gs.CONFIGS[CONFIG], FTYPE, seed=0xC0FFEE, with_vocab=False)
    os.replace(path + ".tmp", path)

res = {"model": f"{CONFIG} {FTYPE}: gguf_synth.write_synthetic_llama(CONFIGS['{CONFIG}'], '{FTYPE}', seed=0xC0FFEE, with_vocab=False), bench.py's file",
       "tokens": f"numpy.random.default_rng({TOKEN_SEED}).integers(0, {gs.CONFIGS[CONFIG].n_vocab}, {N_CHUNKS * N_CHUNK}).astype(int32)",
       "note": "one run per mode, each in a process of its own; host clock between the per-chunk callbacks, so seconds_per_chunk[0] holds the warm-up; "
               "the base of the *_base modes is the same file loaded a second time; no threshold", "commands": {}}
with tempfile.TemporaryDirectory() as td:
    tok = os.path.join(td, "tokens.npy")
    np.save(tok, np.random.default_rng(TOKEN_SEED).integers(0, gs.CONFIGS[CONFIG].n_vocab, N_CHUNKS * N_CHUNK).astype(np.int32))
    for mode, extra in (("device", []), ("host", ["--host-score"]), ("device_base", ["--base", path]), ("host_base", ["--base", path, "--host-score"])):
        js = os.path.join(td, mode + ".json")
        args = ["-m", path, "--tokens", tok, "--ctx", str(N_CHUNK), "--ubatch", str(N_CHUNK), "--cache-type", "q8_0", "--chunks", str(N_CHUNKS), "--json", js] + extra
        res["commands"][mode] = "python tools/perplexity.py " + " ".join(a.replace(path, name).replace(tok, "tokens.npy").replace(js, mode + ".json") for a in args)
        print("+", res["commands"][mode], flush=True)
        r = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.join(ROOT, "tools", "perplexity.py")] + args, capture_output=True, text=True)
        print(r.stdout[-600:], r.stderr[-600:], flush=True)
        if r.returncode != 0:
            sys.exit(r.returncode)
        res[mode] = json.load(open(js))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps({m: res[m]["seconds_per_chunk_median"] for m in ("device", "host", "device_base", "host_base")}))
