#!/usr/bin/env python3
"""Quantise an F32 / F16 / BF16 GGUF file on the device: what upstream's llama-quantize does for the ten mixes the reference publishes (the
kernels are csrc/quantize.hip behind mi355_quantize_chunk, the arithmetic is restated from memory of ggml and not pinned to its source).

  quantize.py [--imatrix FILE] [--pure] [--leave-output-tensor] [--json OUT] IN.gguf OUT.gguf TYPE

TYPE: q2_k, q3_k_s, q3_k_m, q3_k_l, q4_k_s, q4_k_m, q5_k_s, q5_k_m, q6_k or q8_0.  Every 2-D *.weight tensor and every 3-D expert tensor takes the type
gguf_synth.tensor_type gives it (the mix, then the 32-element fallback for rows that are no multiple of 256); 1-D tensors, the router (ffn_gate_inp), rope_freqs
and an encoder's position / type tables are copied.  --pure gives every tensor the mix's base type; --leave-output-tensor copies output.weight.  --imatrix
takes a file written by tools/imatrix.py (GGUF or legacy form): every layer tensor needs an entry of its row length; token_embd and output are quantised
without one when the file has none, as upstream does.  A tensor that would need IQ4_NL (a Q2_K / Q3_K tensor with such rows) and a source tensor that is
already quantised are refused by name."""
import argparse
import importlib.util
import json
import os
import re
import struct
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

_spec = importlib.util.spec_from_file_location("mi355_imatrix_tool", os.path.join(ROOT, "tools", "imatrix.py"))
imx = importlib.util.module_from_spec(_spec)          # the importance-matrix file readers (tools/imatrix.py)
_spec.loader.exec_module(imx)

F32, F16, BF16 = 0, 1, 30
SRC_DTYPE = {F32: np.dtype("<f4"), F16: np.dtype("<f2"), BF16: np.dtype("<u2")}
MIXES = ("q2_k", "q3_k_s", "q3_k_m", "q3_k_l", "q4_k_s", "q4_k_m", "q5_k_s", "q5_k_m", "q6_k", "q8_0")
CHUNK_BYTES = 256 << 20                  # source bytes of one device call
COPIED = ("ffn_gate_inp.weight", "rope_freqs.weight", "token_types.weight", "position_embd.weight")
_SC = {0: "<B", 1: "<b", 2: "<H", 3: "<h", 4: "<I", 5: "<i", 6: "<f", 7: "<?", 10: "<Q", 11: "<q", 12: "<d"}


class QuantizeError(ValueError):
    pass


def read_gguf(path: str):
    """-> (kv: [(key, value, raw bytes of the whole entry)] in file order, tensors: [(name, ne, type, uint8 view of the payload)] in file order); the payloads
    are views of a memory map, read when used"""
    buf = np.memmap(path, np.uint8, "r")
    off = 0

    def take(fmt):
        nonlocal off
        v = struct.unpack_from(fmt, buf, off)[0]
        off += struct.calcsize(fmt)
        return v

    def string():
        nonlocal off
        n = take("<Q")
        s = bytes(buf[off:off + n]).decode("utf-8", "replace")
        off += n
        return s

    def value(t):
        nonlocal off
        if t == 8:
            return string()
        if t == 9:
            et, n = take("<I"), take("<Q")
            if et in _SC:                                    # (a vocabulary's scores and token types: not element by element)
                sz = struct.calcsize(_SC[et])
                v = np.frombuffer(buf, np.dtype(_SC[et][1:]).newbyteorder("<"), n, off)
                off += sz * n
                return v
            return [value(et) for _ in range(n)]
        return take(_SC[t])

    if buf.size < 24 or take("<I") != 0x46554747:
        raise QuantizeError(f"{path}: not a GGUF file")
    if take("<I") != 3:
        raise QuantizeError(f"{path}: not GGUF version 3")
    n_tensors, n_kv = take("<Q"), take("<Q")
    kv = []
    for _ in range(n_kv):
        at = off
        k = string()
        v = value(take("<I"))
        kv.append((k, v, bytes(buf[at:off])))
    infos = []
    for _ in range(n_tensors):
        name = string()
        ne = tuple(take("<Q") for _ in range(take("<I")))
        t, o = take("<I"), take("<Q")
        infos.append((name, ne, t, o))
    al = dict((k, v) for k, v, _ in kv).get("general.alignment", 32)
    base = (off + al - 1) // al * al
    return kv, [(name, ne, t, buf[base + o:]) for name, ne, t, o in infos]


def config_of(pkg, kv: dict, tensors):
    """the LlamaConfig gguf_synth.tensor_type asks for, from the file's metadata"""
    gs = pkg.gguf_synth
    arch = kv.get("general.architecture", "llama")
    shapes = {name: ne for name, ne, _, _ in tensors}

    def k(name, default=0):
        return int(kv.get(f"{arch}.{name}", default))

    n_embd, n_head = k("embedding_length"), k("attention.head_count")
    n_layer = k("block_count")
    n_head_kv = k("attention.head_count_kv", n_head)
    if not (n_embd and n_head and n_layer and n_head_kv):
        raise QuantizeError(f"the file's metadata lacks {arch}.embedding_length / block_count / attention.head_count")
    hd = k("attention.key_length")
    return gs.LlamaConfig(kv.get("general.name", "model"), n_embd, n_layer, n_head, n_head_kv, k("feed_forward_length"),
                          int(shapes.get("token_embd.weight", (n_embd, 0))[1]), n_expert=k("expert_count"), n_expert_used=k("expert_used_count"),
                          big_model=n_layer == 80 and n_head // n_head_kv == 8, arch=arch, n_head_dim=0 if hd * n_head == n_embd else hd,
                          tied_output="output.weight" not in shapes, n_ff_exp=k("expert_feed_forward_length"))


def base_type(gs, ftype: str) -> int:
    return {"q2": gs.Q2_K, "q3": gs.Q3_K, "q4": gs.Q4_K, "q5": gs.Q5_K, "q6": gs.Q6_K, "q8": gs.Q8_0}[ftype[:2]]


def kind_of(name: str):
    """(kind, layer) of a weight as gguf_synth names them, or None"""
    if name in ("token_embd.weight", "output.weight"):
        return name[:-7], 0
    m = re.fullmatch(r"blk\.(\d+)\.(\w+?)(_exps)?\.weight", name)
    return (m.group(2), int(m.group(1))) if m else None


def column_weights(im, name: str, ne0: int, n_mat: int):
    """f32 [n_mat][ne0] of a tensor: in_sum2 / counts per column (legacy form: values / ncall); an expert that was never routed to gets the neutral weight 1.
    None for token_embd / output without an entry."""
    if name not in im.entries:
        if name in ("token_embd.weight", "output.weight"):
            return None
        raise QuantizeError(f"{name}: the importance matrix has no entry for this tensor")
    s, c = im.entries[name]
    if s.size != ne0 * n_mat or (not im.flat and s.shape != (n_mat, ne0)):
        raise QuantizeError(f"{name}: the importance matrix entry has {s.shape[0]} x {s.shape[1]} values, the tensor needs {n_mat} x {ne0}")
    s = s.reshape(n_mat, ne0).astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), (n_mat,)).reshape(n_mat, 1)
    w = np.where(c > 0, s / np.where(c > 0, c, 1.0), 1.0).astype(np.float32)
    if not np.isfinite(w).all() or (w < 0).any():
        raise QuantizeError(f"{name}: the importance matrix entry holds a negative or non-finite value")
    return w


def quantize_file(src: str, dst: str, ftype: str, imatrix=None, quantize_rows=None, pure: bool = False, leave_output: bool = False,
                  chunk_bytes: int = CHUNK_BYTES, out=print):
    """src (F32 / F16 / BF16 weights) -> dst in the mix `ftype`.  imatrix: a path, or None.  quantize_rows(dst_type, rows, imatrix=None, src_type=...) ->
    uint8 [n_rows][row bytes] does the arithmetic: Backend.quantize_rows, or the numpy twin.  Returns [(name, ne, source type, type)] in file order."""
    pkg = ge.load_pkg()
    gs = pkg.gguf_synth
    if ftype not in MIXES:
        raise QuantizeError(f"{ftype!r} is not one of {', '.join(MIXES)}")
    kv_list, tensors = read_gguf(src)
    kv = {k: v for k, v, _ in kv_list}
    cfg = config_of(pkg, kv, tensors)
    im = imx.read_imatrix(imatrix) if imatrix else None

    plan = []
    for name, ne, t, data in tensors:
        kind = kind_of(name)
        copy = len(ne) < 2 or not name.endswith(".weight") or name.endswith(COPIED) or kind is None or (leave_output and name == "output.weight")
        if copy:
            plan.append((name, ne, t, t, data, None))
            continue
        if t not in SRC_DTYPE:
            raise QuantizeError(f"{name}: the source tensor is {gs.TYPE_NAME.get(t, t)}, not F32, F16 or BF16 (requantising is not built)")
        if pure:
            nt = base_type(gs, ftype)
            nt = gs.FALLBACK_32[nt] if gs.BLOCK_ELEMS[nt] == 256 and ne[0] % 256 else nt
        else:
            nt = gs.tensor_type(cfg, ftype, kind[0], kind[1])
            if gs.BLOCK_ELEMS[nt] == 256 and ne[0] % 256:          # (a row length the metadata did not foretell)
                nt = gs.FALLBACK_32[nt]
        if nt == gs.IQ4_NL:
            raise QuantizeError(f"{name}: rows of {ne[0]} are no multiple of 256 and the mix's type here falls back to IQ4_NL, which is not built")
        if ne[0] % gs.BLOCK_ELEMS[nt]:
            raise QuantizeError(f"{name}: rows of {ne[0]} are no whole number of {gs.TYPE_NAME[nt]} blocks")
        n_mat = int(ne[2]) if len(ne) == 3 else 1
        plan.append((name, ne, t, nt, data, column_weights(im, name, int(ne[0]), n_mat) if im is not None else None))

    w = gs.GGUFWriter(alignment=int(kv.get("general.alignment", 32)))
    replaced = {"general.file_type": ("u32", gs.FTYPE_ID[ftype]), "general.quantization_version": ("u32", 2)}
    for k, _, raw in kv_list:                                # key for key, in order, as the bytes they were
        if k in replaced:
            w.add(k, *replaced.pop(k))
        elif not k.startswith("quantize.imatrix."):
            w.kv.append(raw)
    for k, (kind, v) in replaced.items():
        w.add(k, kind, v)
    if im is not None:
        w.add("quantize.imatrix.file", "str", str(imatrix))
        w.add("quantize.imatrix.dataset", "str", im.datasets[0] if im.datasets else "")
        w.add("quantize.imatrix.entries_count", "i32", len(im.entries))
        w.add("quantize.imatrix.chunks_count", "i32", im.chunk_count)

    lock = threading.Lock()                                  # (the writer draws tensors from a few threads: one device call at a time)

    def quantised(ne, t, nt, data, cw):
        def make():
            ne0 = int(ne[0])
            n_mat = int(ne[2]) if len(ne) == 3 else 1
            rows = int(np.prod(ne[1:])) // n_mat
            x = data[:ne0 * rows * n_mat * SRC_DTYPE[t].itemsize].view(SRC_DTYPE[t]).reshape(n_mat, rows, ne0)
            step = max(1, chunk_bytes // (ne0 * SRC_DTYPE[t].itemsize))
            parts = []
            for m in range(n_mat):                           # expert by expert, each with its own column weights
                for r0 in range(0, rows, step):
                    with lock:
                        parts.append(quantize_rows(nt, np.ascontiguousarray(x[m, r0:r0 + step]), imatrix=None if cw is None else cw[m], src_type=t))
            return np.concatenate([p.reshape(-1) for p in parts])
        return make

    total_in = total_out = 0
    for name, ne, t, nt, data, cw in plan:
        n = int(np.prod(ne))
        b_in, b_out = gs.row_bytes(t, ne[0]) * (n // ne[0]), gs.row_bytes(nt, ne[0]) * (n // ne[0])
        total_in += b_in
        total_out += b_out
        if nt == t:
            w.add_tensor(name, ne, t, data[:b_in])
            out(f"{name:40s} [{' x '.join(str(x) for x in ne):>20s}] {gs.TYPE_NAME.get(t, t):>6s}   copied, {b_in / 2**20:9.3f} MiB")
        else:
            w.add_tensor(name, ne, nt, quantised(ne, t, nt, data, cw))
            out(f"{name:40s} [{' x '.join(str(x) for x in ne):>20s}] {gs.TYPE_NAME[t]:>6s} -> {gs.TYPE_NAME[nt]:<6s} {b_in / 2**20:9.3f} MiB -> {b_out / 2**20:9.3f} MiB")
    size = w.write(dst)
    out(f"model size = {total_in / 2**20:.2f} MiB, quantised size = {total_out / 2**20:.2f} MiB, file {size / 2**20:.2f} MiB ({ftype})")
    return [(name, ne, t, nt) for name, ne, t, nt, _, _ in plan]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--imatrix", help="an importance matrix written by tools/imatrix.py (GGUF or legacy form)")
    ap.add_argument("--pure", action="store_true", help="every tensor takes the mix's base type")
    ap.add_argument("--leave-output-tensor", action="store_true", help="copy output.weight as it is")
    ap.add_argument("--json", help="write the run's times here: wall seconds, and per destination type the source bytes and the upload / launch / download ms")
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("type")
    args = ap.parse_args(argv)
    ftype = args.type.lower()
    pkg = ge.load_pkg()
    lib = pkg.load_library()
    try:
        if ftype not in MIXES:
            raise QuantizeError(f"{args.type!r} is not one of {', '.join(MIXES)}")
        if not lib.mi355_quantize_supported(base_type(pkg.gguf_synth, ftype)):
            raise QuantizeError(f"the library does not quantise to {ftype}")
        be = pkg.Backend()
        per_type = {}

        def rows(dst_type, x, imatrix=None, src_type=None):
            out = be.quantize_rows(dst_type, x, imatrix, src_type)
            st = per_type.setdefault(pkg.gguf_synth.TYPE_NAME[dst_type], {"source_bytes": 0, "upload_ms": 0.0, "kernel_ms": 0.0, "download_ms": 0.0, "calls": 0})
            for k, v in zip(("upload_ms", "kernel_ms", "download_ms"), be.quantize_last_times()):
                st[k] += v
            st["source_bytes"] += int(x.nbytes)
            st["calls"] += 1
            return out

        t0 = time.perf_counter()
        quantize_file(args.src, args.dst, ftype, imatrix=args.imatrix, quantize_rows=rows, pure=args.pure, leave_output=args.leave_output_tensor)
        if args.json:
            with open(args.json, "w") as f:
                json.dump({"type": ftype, "wall_s": round(time.perf_counter() - t0, 4), "per_type": per_type}, f, indent=1)
                f.write("\n")
    except (QuantizeError, ValueError, pkg.MI355Error) as e:
        print(f"quantize: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
