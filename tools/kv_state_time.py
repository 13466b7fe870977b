#!/usr/bin/env python3
"""What saving and restoring a sequence's KV state costs, against prefilling it again: the benchmark's synthetic Llama-3-8B Q4_K_M model, q8_0 cache, 4096 cells.

  parts      for N = 512 and 3968 cells: the pack launch, the device-to-host copy and the unpack launch, each from events of its own, against the bytes moved
  end to end for N = 64, 256, 512, 3968: "a prompt of N tokens answered after a restore" (state_seq_set of the N cells, drop the last one, evaluate the last
             token: what the slot loop does with a stored conversation) against "the same prompt prefilled" (kv_clear, evaluate N tokens), and the save
             (state_seq_get) a slot pays when its conversation is pushed out

usage: kv_state_time.py [out.json]   -> one JSON line per row on stdout, all of them as a list in out.json (profiles/kv_state_time.json).
The model file is the one bench.py writes (MI355_BENCH_DIR, default /tmp)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_pkg()
gs = pkg.gguf_synth
out_path = sys.argv[1] if len(sys.argv) > 1 else None
model_dir = os.environ.get("MI355_BENCH_DIR", "/tmp")
cfg_name, ftype, REPS = "llama-3-8b", "q4_k_m", 5

path = os.path.join(model_dir, f"mi355-bench-{cfg_name}-{ftype}.gguf")
if not os.path.exists(path):
    gs.write_synthetic_llama(path + ".tmp", gs.CONFIGS[cfg_name], ftype, seed=0xC0FFEE, with_vocab=False)
    os.replace(path + ".tmp", path)
model = pkg.Model(path)
ctx = pkg.Context(model, n_ctx=4096, n_batch=2048, n_ubatch=2048, type_k=8, type_v=8)
rng = np.random.default_rng(4321)
rows = []


def median(xs):
    return sorted(xs)[len(xs) // 2]


def prefill(prompt):
    ctx.kv_clear()
    for i0 in range(0, prompt.size, 2048):
        assert ctx.decode(prompt[i0:i0 + 2048], np.arange(i0, min(prompt.size, i0 + 2048))) == 0
    ctx.logits_ready()


def get_into(buf):
    """mi355_state_seq_get_data into a buffer the caller keeps (its pages are touched once, not on every pass)"""
    n = int(ctx.lib.mi355_state_seq_get_data(ctx.h, buf.ctypes.data, buf.size, 0))
    assert n > 0
    return n


def set_from(buf, n):
    assert int(ctx.lib.mi355_state_seq_set_data(ctx.h, buf.ctypes.data, n, 0)) == n


def emit(row):
    rows.append(row)
    print(json.dumps(row), flush=True)


# ---- the parts, from events
ctx.state_seq_timing()                                     # (switches the events on)
for n in (512, 3968):
    prompt = rng.integers(0, model.n_vocab, n)
    prefill(prompt)
    pack, copy, unpack = [], [], []
    buf = np.zeros(ctx.state_seq_size(0), np.uint8)
    for _ in range(REPS + 1):                              # (the first pass allocates the staging block and warms up)
        size = get_into(buf)
        p, c, _u = ctx.state_seq_timing()
        set_from(buf, size)
        _p, _c, u = ctx.state_seq_timing()
        pack.append(p); copy.append(c); unpack.append(u)
    rows_bytes = size - 32 - 4 * n
    p, c, u = median(pack[1:]), median(copy[1:]), median(unpack[1:])
    emit({"what": "parts", "cells": n, "row_bytes": rows_bytes, "pack_ms": round(p, 3), "copy_d2h_ms": round(c, 3), "unpack_ms": round(u, 3),
          "pack_GBps_read_plus_written": round(2 * rows_bytes / p / 1e6, 1), "unpack_GBps_read_plus_written": round(2 * rows_bytes / u / 1e6, 1),
          "copy_GBps": round(rows_bytes / c / 1e6, 1)})

# ---- end to end, wall clock (events off: a fresh context)
ctx.close()
ctx = pkg.Context(model, n_ctx=4096, n_batch=2048, n_ubatch=2048, type_k=8, type_v=8)
for n in (64, 256, 512, 3968):
    prompt = rng.integers(0, model.n_vocab, n)
    t_prefill, t_restore, t_save = [], [], []
    buf = None
    for _ in range(REPS + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        prefill(prompt)
        t_prefill.append(time.perf_counter() - t0)
        if buf is None:
            buf = np.zeros(ctx.state_seq_size(0), np.uint8)
        t0 = time.perf_counter()
        size = get_into(buf)
        t_save.append(time.perf_counter() - t0)
        ctx.kv_clear()
        t0 = time.perf_counter()
        set_from(buf, size)
        ctx.kv_seq_rm(0, n - 1, -1)
        assert ctx.decode(prompt[n - 1:], [n - 1]) == 0
        ctx.logits_ready()
        t_restore.append(time.perf_counter() - t0)
    pf, rs, sv = median(t_prefill[1:]) * 1e3, median(t_restore[1:]) * 1e3, median(t_save[1:]) * 1e3
    emit({"what": "end_to_end", "tokens": n, "blob_bytes": size, "prefill_ms": round(pf, 3), "restore_and_last_token_ms": round(rs, 3), "save_ms": round(sv, 3),
          "restore_wins": bool(rs < pf), "save_plus_restore_wins": bool(rs + sv < pf)})
if out_path:
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
ctx.close(); model.close()
