#!/usr/bin/env python3
"""Merge LoRA adapters into a base GGUF file on the device: what upstream's llama-export-lora does (the kernel is csrc/lora_merge.hip behind
mi355_lora_merge_rows; the rules are upstream's as remembered, not pinned to its source).

  export_lora.py -m BASE.gguf --lora AD.gguf [--lora-scaled AD2.gguf 0.5 ...] -o MERGED.gguf [--outtype f16|f32] [--json OUT]

A base tensor X is merged when an adapter holds X.lora_a and X.lora_b: X' = round(deq(X) + sum_i s_i B_i A_i), s_i = user scale_i * adapter.lora.alpha_i / r_i
(the user scale alone where alpha is 0), written as F16 (or F32) whatever X's type was; a 3-D *_exps tensor is merged expert by expert from lora_a [K, r, E]
and lora_b [r, N, E].  Every other tensor and every key leaves byte for byte; general.file_type is rewritten to F16 only when every tensor of two and more
dimensions ended up F16.  Rows go to the device in chunks, so the largest tensor needs no second copy in host memory.  The merged file goes through
tools/quantize.py as any F16 file does.  Refused by name, before any device work: a pair whose shapes do not fit the base tensor, half a pair, a missing
alpha, a rank above 512, a base tensor of a type the kernel does not read, an adapter of another architecture."""
import argparse
import importlib.util
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

_spec = importlib.util.spec_from_file_location("mi355_quantize_tool", os.path.join(ROOT, "tools", "quantize.py"))
qt = importlib.util.module_from_spec(_spec)           # the GGUF reader (tools/quantize.py)
_spec.loader.exec_module(qt)

F32, F16, BF16, Q8_0, Q4_K, Q5_K, Q6_K = 0, 1, 30, 8, 12, 13, 14
BASE_TYPES = (F32, F16, BF16, Q8_0, Q4_K, Q5_K, Q6_K)      # what csrc/lora_merge.hip decodes (mi355_lora_merge_supported)
PAIR_DTYPE = {F32: np.dtype("<f4"), F16: np.dtype("<f2")}
MAX_RANK, MAX_ADAPTERS = 512, 8
CHUNK_BYTES = 256 << 20                  # merged bytes of one device call


class ExportError(ValueError):
    pass


def read_adapter(path: str, arch: str):
    """-> (alpha, {base tensor name: (A [E][r][K], B [E][N][r], pair type)}) of an adapter for a base of architecture `arch`; E = 1 for a 2-D pair"""
    kv_list, tensors = qt.read_gguf(path)
    kv = {k: v for k, v, _ in kv_list}
    if kv.get("general.type") != "adapter" or kv.get("adapter.type") != "lora":
        raise ExportError(f"{path}: not a LoRA adapter file (general.type {kv.get('general.type')!r}, adapter.type {kv.get('adapter.type')!r})")
    if kv.get("general.architecture") != arch:
        raise ExportError(f"{path}: adapter architecture {kv.get('general.architecture')!r} does not match the base file's {arch!r}")
    if not isinstance(kv.get("adapter.lora.alpha"), float):
        raise ExportError(f"{path}: adapter.lora.alpha is missing or not an f32")
    halves = {}
    for name, ne, t, data in tensors:
        if not name.endswith((".lora_a", ".lora_b")):
            raise ExportError(f"{path}: adapter tensor {name} ends in neither .lora_a nor .lora_b")
        halves.setdefault(name[:-7], {})[name[-1]] = (ne, t, data)
    pairs = {}
    for base, h in halves.items():
        for have, lack in (("a", "b"), ("b", "a")):
            if lack not in h:
                raise ExportError(f"{path}: adapter tensor {base}.lora_{have} has no {base}.lora_{lack} beside it")
        (ne_a, ta, da), (ne_b, tb, db) = h["a"], h["b"]
        if ta != tb or ta not in PAIR_DTYPE:
            raise ExportError(f"{path}: adapter pair {base}: lora_a has type {ta} and lora_b type {tb} (both halves must be f16, or both f32)")
        if len(ne_a) != len(ne_b) or len(ne_a) not in (2, 3) or ne_a[1] != ne_b[0] or ne_a[2:] != ne_b[2:]:
            raise ExportError(f"{path}: adapter pair {base}: lora_a is {list(ne_a)} and lora_b is {list(ne_b)} (lora_a [K, r], lora_b [r, N])")
        K, r, N, E = int(ne_a[0]), int(ne_a[1]), int(ne_b[1]), int(ne_a[2]) if len(ne_a) == 3 else 1
        if not 1 <= r <= MAX_RANK:
            raise ExportError(f"{path}: adapter pair {base}: rank {r} is outside 1 .. {MAX_RANK}")
        dt = PAIR_DTYPE[ta]
        pairs[base] = (da[:E * r * K * dt.itemsize].view(dt).reshape(E, r, K), db[:E * N * r * dt.itemsize].view(dt).reshape(E, N, r), ta)
    if not pairs:
        raise ExportError(f"{path}: adapter file without tensors")
    return float(kv["adapter.lora.alpha"]), pairs


def merge_file(base: str, adapters, dst: str, outtype: str = "f16", merge_rows=None, chunk_bytes: int = CHUNK_BYTES, out=print):
    """base + adapters = [(path, user scale), ...] -> dst.  merge_rows(base_type, base_rows uint8 [n][row bytes], [(A [r][K], B [n][r], scale)], out_type) ->
    [n][K] of the out type does the arithmetic: Backend.lora_merge_rows, or the numpy twin.  Returns [(name, ne, source type, type)] in file order."""
    pkg = ge.load_pkg()
    gs = pkg.gguf_synth
    if outtype not in ("f16", "f32"):
        raise ExportError(f"--outtype {outtype!r} is neither f16 nor f32")
    out_type = F16 if outtype == "f16" else F32
    if not 1 <= len(adapters) <= MAX_ADAPTERS:
        raise ExportError(f"{len(adapters)} adapters: one call merges 1 .. {MAX_ADAPTERS}")
    kv_list, tensors = qt.read_gguf(base)
    kv = {k: v for k, v, _ in kv_list}
    shapes = {name: (ne, t) for name, ne, t, _ in tensors}
    loaded = []
    for path, user in adapters:
        alpha, pairs = read_adapter(path, kv.get("general.architecture", "llama"))
        for name, (A, B, _) in pairs.items():
            if name not in shapes:
                raise ExportError(f"{path}: adapter targets {name}, which the base file does not have" +
                                  (" (its head is tied to token_embd.weight: a merge would need a tensor of its own)" if name == "output.weight" else ""))
            ne, t = shapes[name]
            E = int(ne[2]) if len(ne) == 3 else 1
            if len(ne) not in (2, 3) or (A.shape[2], B.shape[1], A.shape[0]) != (int(ne[0]), int(ne[1]), E):
                raise ExportError(f"{path}: adapter pair {name}: lora_a is [{A.shape[2]}, {A.shape[1]}] and lora_b is [{B.shape[2]}, {B.shape[1]}]" +
                                  (f" x {A.shape[0]}" if A.shape[0] > 1 else "") + f" where the base tensor is {list(ne)} (lora_a [K, r], lora_b [r, N])")
            if t not in BASE_TYPES:
                raise ExportError(f"{name}: the base tensor is {gs.TYPE_NAME.get(t, t)}, which the merge does not read (f32, f16, bf16, q8_0, q4_K, q5_K and q6_K are)")
            if ne[0] % 8:
                raise ExportError(f"{name}: rows of {ne[0]} are no multiple of 8")
        loaded.append((pairs, [float(user) * alpha / A.shape[1] if alpha != 0.0 else float(user) for A, _, _ in pairs.values()]))
    scale_of = [dict(zip(pairs, scales)) for pairs, scales in loaded]

    lock = threading.Lock()                                  # (the writer draws tensors from a few threads: one device call at a time)

    def merged(name, ne, t, data):
        def make():
            K, N, E = int(ne[0]), int(ne[1]), int(ne[2]) if len(ne) == 3 else 1
            rb = gs.row_bytes(t, K)
            rows = data[:rb * N * E].reshape(E, N, rb)
            mine = [(pairs[name], sc[name]) for (pairs, _), sc in zip(loaded, scale_of) if name in pairs]
            step = max(1, chunk_bytes // (K * 4))
            parts = []
            for e in range(E):                               # expert by expert, rows in chunks
                for r0 in range(0, N, step):
                    ads = [(np.ascontiguousarray(A[e]), np.ascontiguousarray(B[e, r0:r0 + step]), s) for (A, B, _), s in mine]
                    with lock:
                        parts.append(merge_rows(t, np.ascontiguousarray(rows[e, r0:r0 + step]), ads, out_type))
            return np.concatenate([p.reshape(-1).view(np.uint8) for p in parts])
        return make

    w = gs.GGUFWriter(alignment=int(kv.get("general.alignment", 32)))
    plan = []
    for name, ne, t, data in tensors:
        nt = out_type if any(name in pairs for pairs, _ in loaded) else t
        plan.append((name, ne, t, nt))
        if nt == t and not any(name in pairs for pairs, _ in loaded):
            w.add_tensor(name, ne, t, data[:gs.row_bytes(t, ne[0]) * (int(np.prod(ne)) // ne[0])])
            out(f"{name:40s} [{' x '.join(str(x) for x in ne):>20s}] {gs.TYPE_NAME.get(t, t):>6s}   copied")
        else:
            w.add_tensor(name, ne, nt, merged(name, ne, t, data))
            out(f"{name:40s} [{' x '.join(str(x) for x in ne):>20s}] {gs.TYPE_NAME.get(t, t):>6s} -> {gs.TYPE_NAME[nt]:<6s} merged")
    all_f16 = all(nt == F16 for _, ne, _, nt in plan if len(ne) >= 2)
    for k, _, raw in kv_list:                                # key for key, in order, as the bytes they were
        if k == "general.file_type" and all_f16:
            w.add(k, "u32", gs.FTYPE_ID["f16"])
        else:
            w.kv.append(raw)
    size = w.write(dst)
    n_merged = sum(1 for name, _, _, _ in plan if any(name in pairs for pairs, _ in loaded))
    out(f"merged {n_merged} of {len(plan)} tensors from {len(loaded)} adapter(s): file {size / 2**20:.2f} MiB")
    return plan


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-m", "--model", required=True, help="the base GGUF file")
    ap.add_argument("--lora", action="append", default=[], metavar="FILE", help="an adapter, user scale 1")
    ap.add_argument("--lora-scaled", action="append", default=[], nargs=2, metavar=("FILE", "SCALE"), help="an adapter with a user scale")
    ap.add_argument("-o", "--output", required=True)
    ap.add_argument("--outtype", default="f16", help="f16 (default) or f32: the type of the merged tensors")
    ap.add_argument("--json", help="write the run's times here: wall seconds and the upload / launch / download ms of the device calls")
    args = ap.parse_args(argv)
    pkg = ge.load_pkg()
    try:
        adapters = [(p, 1.0) for p in args.lora] + [(p, float(s)) for p, s in args.lora_scaled]
        be = []                                              # (the device is opened by the first merge: every refusal comes before it)
        times = {"upload_ms": 0.0, "kernel_ms": 0.0, "download_ms": 0.0, "calls": 0, "merged_bytes": 0}

        def rows(base_type, base_rows, ads, out_type):
            if not be:
                be.append(pkg.Backend())
            y = be[0].lora_merge_rows(base_type, base_rows, ads, out_type)
            for k, v in zip(("upload_ms", "kernel_ms", "download_ms"), be[0].lora_merge_last_times()):
                times[k] += v
            times["calls"] += 1
            times["merged_bytes"] += int(y.nbytes)
            return y

        t0 = time.perf_counter()
        merge_file(args.model, adapters, args.output, outtype=args.outtype.lower(), merge_rows=rows)
        if args.json:
            with open(args.json, "w") as f:
                json.dump({"outtype": args.outtype.lower(), "wall_s": round(time.perf_counter() - t0, 4), **times}, f, indent=1)
                f.write("\n")
    except (ValueError, pkg.MI355Error) as e:
        print(f"export_lora: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
