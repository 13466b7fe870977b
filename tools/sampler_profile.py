"""What the device sampler (csrc/sample.hip) costs and saves, in one build: the median of three passes with the smallest and largest.

    python tools/sampler_profile.py [--steps 256] [--slots 32] [--out profiles/device_sampler.json]

  sampled_steps:  n single-token steps of the default sampled request (temp 0.8, top_k 40, top_p 0.95, min_p 0.05) through mi355_sampled_steps, against a
                  Python loop over decode + mi355_get_topk_ith + the chain in numpy (what a C-ABI user without the device sampler writes).
  slot_step:      the sampling time of a 32-slot step, per step (the mean of calls_per_pass steps in a pass): one mi355_sample_rows call over 32 rows, against 32 mi355_get_topk_ith calls + 32 numpy chains
                  (the engine's own host path batches the front; its tail runs on a thread pool - tools/bench_engine.py measures that end to end).

    python tools/sampler_profile.py --vocab [--out profiles/device_sampler_vocab.json]

  --vocab:        the whole-row sampler (csrc/sample_vocab.hip) on the same model and on it with n_vocab 151936: one mi355_sample_rows_vocab
                  call (top_k 0, top_p 0.95) for a 1-slot and a 32-slot step, and engine tokens/s of that request with "device_sampler" on and off (off: the
                  host whole-row chain, the only path such a request had before).
"""
import argparse
import dataclasses
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge   # noqa: E402
import sample_ref as ref       # noqa: E402

PARAMS = dict(top_k=40, top_p=0.95, min_p=0.05, temp=0.8, seed=1)


def three(f, calls=1):
    """f three times; milliseconds per call where f makes `calls` of them"""
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3 / calls)
    return dict(median=round(float(np.median(t)), 4), min=round(min(t), 4), max=round(max(t), 4))


def host_tail(toks, lg, u):
    t, p, _ = ref.chain(toks, lg, **PARAMS)
    return int(t[ref.draw(p, u)])


VOCAB_PARAMS = dict(top_k=0, top_p=0.95, temp=0.8, seed=1)


def vocab_mode(pkg, a):
    doc = dict(passes=3, params=VOCAB_PARAMS, models={})
    base = pkg.gguf_synth.CONFIGS[a.config]
    for cfg in (base, dataclasses.replace(base, name=base.name + "-v151936", n_vocab=151936)):
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "m.gguf")
            pkg.gguf_synth.write_synthetic_llama(path, cfg, "q4_k_m", seed=7, with_vocab=True)
            m = pkg.Model(path)
            c = pkg.Context(m, n_ctx=256, n_batch=64, n_seq_max=a.slots)
            out, reps = {}, 20
            for n in (1, a.slots):
                c.kv_clear()
                assert c.decode(list(range(10, 10 + n)), [0] * n, seq=list(range(n)), logits=[1] * n) == 0
                rows = list(range(n))

                def call():
                    for _ in range(reps):
                        c.sample_rows_vocab(rows, [dict(VOCAB_PARAMS, stream=r) for r in rows], 0)
                call()
                out[f"sample_rows_vocab_ms_{n}_slots"] = three(call, reps)
            c.close(); m.close()
            for key in (True, False):
                e = pkg.Engine()
                st, body = e.load_model(llama_model_path=path, ctx_len=512, n_parallel=1, ngl=100, device_sampler=key)
                assert st["status_code"] == 200, (st, body)
                req = dict(model="m", messages=[{"role": "user", "content": "tell me"}], max_tokens=a.steps, temperature=0.8, top_k=0, top_p=0.95, seed=5)
                e.chat_completion(**req)
                t = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    n_tok = e.chat_completion(**req)[-1][1]["usage"]["completion_tokens"]
                    t.append(n_tok / (time.perf_counter() - t0))
                out["engine_tok_s_device" if key else "engine_tok_s_host_chain"] = dict(median=round(float(np.median(t)), 1), min=round(min(t), 1), max=round(max(t), 1))
                e.close()
        doc["models"][f"{cfg.name} q4_k_m (synthetic), n_vocab {cfg.n_vocab}"] = out
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", action="store_true")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--config", default="tiny-8b-2l")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_sampler.json"))
    a = ap.parse_args()
    pkg = ge.load_pkg()
    pkg.Backend()
    if a.vocab:
        doc = vocab_mode(pkg, a)
        out = a.out if a.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "device_sampler_vocab.json")
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(json.dumps(doc))
        return
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "m.gguf")
        pkg.gguf_synth.write_synthetic_llama(path, a.config, "q4_k_m", seed=7)
        m = pkg.Model(path)
        c = pkg.Context(m, n_ctx=a.steps + 64, n_batch=64, n_seq_max=a.slots)
        rng = np.random.default_rng(0)

        def prompt():
            c.kv_clear()
            assert c.decode([1, 2, 3, 4], [0, 1, 2, 3]) == 0

        def device_steps():
            prompt()
            c.sampled_steps(5, 4, a.steps, PARAMS)

        def host_steps():
            prompt()
            tok = 5
            for i in range(a.steps):
                assert c.decode([tok], [4 + i]) == 0
                tok = host_tail(*c.topk(40), rng.random())
        device_steps(); host_steps()                                   # (warm: graphs captured, workspaces allocated)
        steps = dict(device_ms=three(device_steps), host_loop_ms=three(host_steps))
        # a 32-slot step: 32 sequences, one token each, every row flagged; the decode is outside the timed part
        n = a.slots
        c.kv_clear()
        assert c.decode(list(range(10, 10 + n)), [0] * n, seq=list(range(n)), logits=[1] * n) == 0
        rows, reps = list(range(n)), 20

        def device_slots():
            for _ in range(reps):
                c.sample_rows(rows, [dict(PARAMS, stream=r) for r in rows], 0)

        def host_slots():
            for _ in range(reps):
                for r in rows:
                    host_tail(*c.topk(40, r), rng.random())
        device_slots(); host_slots()
        slots = dict(device_ms_per_call=three(device_slots, reps), host_loop_ms_per_call=three(host_slots, reps), calls_per_pass=reps)
        doc = dict(model=f"{a.config} q4_k_m (synthetic)", passes=3, sampled_steps=dict(steps=a.steps, **steps), slot_step=dict(slots=n, **slots),
                   note="host_loop: Python over mi355_get_topk_ith plus the float64 numpy chain; same build, same process")
        c.close(); m.close()
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
