#!/usr/bin/env python3
"""The importance matrix of a GGUF file over a calibration text: what upstream's llama-imatrix writes and llama-quantize --imatrix reads (DESIGN.md §4.11;
the collection is Context.imatrix_begin / mi355_imatrix_*, the arithmetic and both file formats are restated from memory of llama.cpp and not pinned to
its source).

  imatrix.py -m MODEL (-f TEXT | --tokens FILE.npy) [-o imatrix.gguf] [--ctx 512] [--ubatch 512] [--cache-type f16|q8_0|q4_0] [--chunks N]
             [--process-output] [--no-ppl] [--in-file PATH ...] [--json OUT]

For every weight matrix the model multiplies, the file holds the per-input-column sum of squared activations over the text and the number of rows summed
(per expert for the expert tensors).  The chunks run through Context.perplexity with collection on, so the running perplexity line of llama-imatrix is
printed on the way (its last digits may differ from tools/perplexity.py: collection takes the launches that keep the f32 rows); --no-ppl runs plain decode
calls without logits instead.  An output name ending in .gguf gives the GGUF form, any other name the legacy .dat form.  --in-file adds the sums and
counts of earlier files, entry by entry; a file with another entry set or other shapes is refused."""
import argparse
import json
import math
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

KV = {"f16": 1, "q8_0": 8, "q4_0": 2}
GGML_F32 = 0
SUM2, COUNTS = ".in_sum2", ".counts"


class IMatrix:
    """entries: {tensor name: (sum2 f32 [n_mat][ne0], counts f32 [n_mat])} in file order, with the datasets, the chunk count and the chunk size."""

    def __init__(self, entries=None, datasets=(), chunk_count=0, chunk_size=0):
        self.entries = {k: (np.ascontiguousarray(s, np.float32).reshape(np.shape(s)[0] if np.ndim(s) == 2 else 1, -1), np.asarray(c, np.float32).reshape(-1))
                        for k, (s, c) in (entries or {}).items()}
        for k, (s, c) in self.entries.items():
            if s.shape[0] != c.size:
                raise ValueError(f"{k}: {s.shape[0]} matrices but {c.size} counts")
        self.datasets = list(datasets)
        self.chunk_count = int(chunk_count)
        self.chunk_size = int(chunk_size)
        self.flat = False                  # read_dat: one matrix per entry whatever the tensor, counts in calls

    def shapes(self):
        return {k: s.shape for k, (s, _) in self.entries.items()}

    def add(self, other: "IMatrix", what: str = "the other file") -> None:
        """self += other, entry by entry (sums through float64); refuses another entry set or other shapes.  A legacy file (flat) records no split into
        experts: its entry must have as many values as this one's matrices together, and its one count goes to every matrix, as upstream loads it."""
        mine, theirs = self.shapes(), other.shapes()
        if other.flat:
            theirs = {k: (mine[k] if k in mine and int(np.prod(mine[k])) == int(np.prod(v)) else v) for k, v in theirs.items()}
        if mine != theirs:
            diff = sorted(set(mine) ^ set(theirs)) or sorted(k for k in mine if mine[k] != theirs[k])
            raise ValueError(f"{what} does not hold the same entries: {len(theirs)} against {len(mine)}; first difference {diff[0]}")
        for k, (s, c) in self.entries.items():
            os_, oc = other.entries[k]
            os_ = os_.reshape(s.shape)
            oc = np.broadcast_to(oc, c.shape) if oc.size == 1 else oc
            self.entries[k] = ((s.astype(np.float64) + os_).astype(np.float32), (c.astype(np.float64) + oc).astype(np.float32))
        self.chunk_count += other.chunk_count
        self.datasets += [d for d in other.datasets if d not in self.datasets]
        if self.chunk_size == 0:
            self.chunk_size = other.chunk_size


# ---------------------------------------------------------------- GGUF form
def write_gguf(path: str, im: IMatrix) -> None:
    """general.type "imatrix", imatrix.datasets / chunk_count / chunk_size, and per entry NAME.in_sum2 [ne0, n_mat] and NAME.counts [1, n_mat], both F32."""
    pkg = ge.load_pkg()
    w = pkg.gguf_synth.GGUFWriter()
    w.add("general.type", "str", "imatrix")
    w.add_array("imatrix.datasets", "str", list(im.datasets))
    w.add("imatrix.chunk_count", "u32", im.chunk_count)
    w.add("imatrix.chunk_size", "u32", im.chunk_size)
    for name, (s, c) in im.entries.items():
        n_mat, ne0 = s.shape
        w.add_tensor(name + SUM2, (ne0, n_mat), GGML_F32, s.astype("<f4").tobytes())
        w.add_tensor(name + COUNTS, (1, n_mat), GGML_F32, c.astype("<f4").tobytes())
    w.write(path)


def read_gguf(path: str) -> IMatrix:
    buf = open(path, "rb").read()
    off = 0
    sc = {0: "<B", 1: "<b", 2: "<H", 3: "<h", 4: "<I", 5: "<i", 6: "<f", 7: "<?", 10: "<Q", 11: "<q", 12: "<d"}

    def take(fmt):
        nonlocal off
        v = struct.unpack_from(fmt, buf, off)[0]
        off += struct.calcsize(fmt)
        return v

    def string():
        nonlocal off
        n = take("<Q")
        s = buf[off:off + n].decode("utf-8", "replace")
        off += n
        return s

    def value(t):
        if t == 8:
            return string()
        if t == 9:
            et, n = take("<I"), take("<Q")
            return [value(et) for _ in range(n)]
        return take(sc[t])

    if len(buf) < 24 or take("<I") != 0x46554747:
        raise ValueError(f"{path}: not a GGUF file")
    if take("<I") != 3:
        raise ValueError(f"{path}: not GGUF version 3")
    n_tensors, n_kv = take("<Q"), take("<Q")
    kv = {}
    for _ in range(n_kv):
        k = string()
        kv[k] = value(take("<I"))
    if kv.get("general.type") != "imatrix":
        raise ValueError(f"{path}: general.type is {kv.get('general.type')!r}, not 'imatrix'")
    infos = []
    for _ in range(n_tensors):
        name = string()
        ne = tuple(take("<Q") for _ in range(take("<I")))
        t, o = take("<I"), take("<Q")
        if t != GGML_F32:
            raise ValueError(f"{path}: tensor {name} is not F32")
        infos.append((name, ne, o))
    al = kv.get("general.alignment", 32)
    base = (off + al - 1) // al * al
    raw = {}
    for name, ne, o in infos:
        n = int(np.prod(ne))
        raw[name] = (ne, np.frombuffer(buf, "<f4", n, base + o).astype(np.float32))
    entries = {}
    for name, (ne, data) in raw.items():
        if not name.endswith(SUM2):
            continue
        stem = name[:-len(SUM2)]
        if stem + COUNTS not in raw or len(ne) != 2:
            raise ValueError(f"{path}: {name} has no counts tensor or is not 2-D")
        ne0, n_mat = ne
        cne, cdata = raw[stem + COUNTS]
        if tuple(cne) != (1, n_mat):
            raise ValueError(f"{path}: {stem}{COUNTS} has shape {cne}, expected (1, {n_mat})")
        entries[stem] = (data.reshape(n_mat, ne0), cdata)
    return IMatrix(entries, kv.get("imatrix.datasets", []), kv.get("imatrix.chunk_count", 0), kv.get("imatrix.chunk_size", 0))


# ---------------------------------------------------------------- legacy .dat form
def dat_values(sum2: np.ndarray, counts: np.ndarray, ncall: int) -> np.ndarray:
    """What the legacy file stores for an entry: sum2 / count * ncall, flattened expert-major.  An expert that was never routed to (count 0) is written as a
    flat 1.0 * ncall, so that the reader's values / ncall give every one of its columns the neutral weight 1."""
    s = np.asarray(sum2, np.float64).reshape(np.asarray(counts).size, -1)
    c = np.asarray(counts, np.float64).reshape(-1, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(c > 0, s / np.where(c > 0, c, 1.0), 1.0) * float(ncall)
    return v.astype(np.float32).reshape(-1)


def write_dat(path: str, im: IMatrix) -> None:
    """int32 n_entries; per entry int32 len, name, int32 ncall, int32 nval, float32[nval]; int32 last_chunk; int32 len + dataset name.  Little endian."""
    ncall = max(im.chunk_count, 1)
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(im.entries)))
        for name, (s, c) in im.entries.items():
            nb = name.encode("utf-8")
            v = dat_values(s, c, ncall)
            f.write(struct.pack("<i", len(nb)) + nb + struct.pack("<ii", ncall, v.size) + v.astype("<f4").tobytes())
        ds = (im.datasets[0] if im.datasets else "").encode("utf-8")
        f.write(struct.pack("<i", im.chunk_count) + struct.pack("<i", len(ds)) + ds)


def read_dat(path: str) -> IMatrix:
    """The legacy file as upstream loads it: an entry's values become its sums and ncall its (single) count, so sums / counts is again the mean square.  The
    split into experts is not recorded: every entry comes back as one matrix of nval columns."""
    buf = open(path, "rb").read()
    off = 0

    def i32():
        nonlocal off
        if off + 4 > len(buf):
            raise ValueError(f"{path}: truncated")
        v = struct.unpack_from("<i", buf, off)[0]
        off += 4
        return v

    n = i32()
    if n < 0:
        raise ValueError(f"{path}: negative entry count")
    entries = {}
    for _ in range(n):
        ln = i32()
        if ln < 1 or off + ln > len(buf):
            raise ValueError(f"{path}: bad name length")
        name = buf[off:off + ln].decode("utf-8", "replace")
        off += ln
        ncall, nval = i32(), i32()
        if nval < 1 or off + 4 * nval > len(buf):
            raise ValueError(f"{path}: bad value count for {name}")
        entries[name] = (np.frombuffer(buf, "<f4", nval, off).astype(np.float32).reshape(1, nval), np.asarray([ncall], np.float32))
        off += 4 * nval
    last_chunk, datasets = 0, []
    if off + 4 <= len(buf):
        last_chunk = i32()
        if off + 4 <= len(buf):
            ln = i32()
            datasets = [buf[off:off + ln].decode("utf-8", "replace")]
    im = IMatrix(entries, datasets, last_chunk, 0)
    im.flat = True
    return im


def write_imatrix(path: str, im: IMatrix) -> None:
    (write_gguf if path.endswith(".gguf") else write_dat)(path, im)


def read_imatrix(path: str) -> IMatrix:
    return (read_gguf if path.endswith(".gguf") else read_dat)(path)


def from_context(ctx, dataset: str, chunk_count: int, chunk_size: int) -> IMatrix:
    return IMatrix({k: (s, c.astype(np.float32)) for k, (s, c) in ctx.imatrix_entries().items()}, [dataset], chunk_count, chunk_size)


def vocab_bos(model) -> int:
    """the BOS id if the vocabulary puts one in front of a text, else -1 (also for a file without a vocabulary)"""
    try:
        bos = int(model.lib.mi355_token_bos(model.h))
        with_, without = model.tokenize("a", add_special=True), model.tokenize("a", add_special=False)
    except Exception:
        return -1
    return bos if bos >= 0 and len(with_) == len(without) + 1 and with_[0] == bos else -1


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-m", "--model", required=True)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("-f", "--file", help="the calibration text, tokenised with the model's tokenizer")
    src.add_argument("--tokens", help="a .npy file of token ids")
    ap.add_argument("-o", "--output", default="imatrix.gguf", help="*.gguf: the GGUF form; any other name: the legacy .dat form")
    ap.add_argument("--ctx", type=int, default=512, help="chunk length")
    ap.add_argument("--ubatch", type=int, default=512)
    ap.add_argument("--cache-type", default="f16", choices=sorted(KV))
    ap.add_argument("--chunks", type=int, default=0, help="only the first N chunks")
    ap.add_argument("--process-output", action="store_true", help="also collect output.weight (token_embd.weight for a tied head)")
    ap.add_argument("--no-ppl", action="store_true", help="plain decode calls without logits: no perplexity line")
    ap.add_argument("--in-file", action="append", default=[], help="an earlier imatrix file to add (repeatable)")
    ap.add_argument("--json", help="write the run's figures here")
    args = ap.parse_args(argv)

    pkg = ge.load_pkg()
    pkg.Backend()
    model = pkg.Model(args.model)
    if args.tokens:
        tokens = np.load(args.tokens).astype(np.int32).reshape(-1)
    else:
        with open(args.file, encoding="utf-8", errors="replace") as f:
            tokens = np.asarray(model.tokenize(f.read(), add_special=False), np.int32)
    bos = vocab_bos(model)
    if args.chunks > 0:
        tokens = tokens[:args.chunks * args.ctx]
    n_chunks = tokens.size // args.ctx
    if n_chunks < 1:
        print(f"{tokens.size} tokens are less than one chunk of {args.ctx}", file=sys.stderr)
        return 2
    earlier = [(p, read_imatrix(p)) for p in args.in_file]          # (before the run: a file that cannot be read should not cost one)
    kv = KV[args.cache_type]
    ctx = pkg.Context(model, n_ctx=args.ctx, n_batch=max(args.ubatch, 1), n_ubatch=args.ubatch, type_k=kv, type_v=kv, logits_to_host=False)
    ctx.imatrix_begin(args.process_output)
    t_chunk = [time.perf_counter()]
    out = {"n_chunk": args.ctx, "n_ubatch": args.ubatch, "cache": args.cache_type, "bos": bos, "process_output": bool(args.process_output),
           "mode": "decode" if args.no_ppl else "perplexity"}
    if args.no_ppl:
        for c in range(n_chunks):
            tk = tokens[c * args.ctx:(c + 1) * args.ctx].copy()
            if bos >= 0:
                tk[0] = bos
            ctx.kv_seq_rm(0, 0, -1)
            for i0 in range(0, args.ctx, args.ubatch):
                pos = np.arange(i0, min(i0 + args.ubatch, args.ctx))
                flags = np.zeros(pos.size, np.int8)
                flags[-1] = 1 if args.process_output else 0       # (the head's entry needs a flagged row)
                if ctx.decode(tk[pos], pos, logits=flags) != 0:
                    raise RuntimeError("decode failed")
            ctx.synchronize()
            t_chunk.append(time.perf_counter())
        ctx.kv_seq_rm(0, 0, -1)
        done = n_chunks
    else:
        def on_chunk(st):
            t_chunk.append(time.perf_counter())
            if st["count"] > 0:
                print(f"[{st['n_chunks']}]{math.exp(st['nll'] / st['count']):.4f},", end="", flush=True)
            return 0

        st = ctx.perplexity(tokens, args.ctx, bos=bos, callback=on_chunk)
        print()
        done = int(st["n_chunks"])
        if st["count"] > 0:
            out["ppl"] = math.exp(st["nll"] / st["count"])
            print(f"PPL = {out['ppl']:.4f}   ({st['count']} tokens, {done} chunks of {args.ctx})")
    dataset = os.path.basename(args.file or args.tokens)
    im = from_context(ctx, dataset, done, args.ctx)
    ctx.imatrix_end()
    for p, e in earlier:
        im.add(e, p)
    write_imatrix(args.output, im)
    secs = np.diff(t_chunk)
    out.update(n_chunks=done, entries=len(im.entries), output=args.output, seconds_per_chunk=[round(float(s), 4) for s in secs],
               seconds_per_chunk_median=round(float(np.median(secs)), 4) if secs.size else None)
    print(f"{len(im.entries)} entries over {done} chunks of {args.ctx} -> {args.output}" +
          (f"; {float(np.median(secs)):.4f} s per chunk (median of {secs.size}; first {float(secs[0]):.4f})" if secs.size else ""))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    ctx.close()
    model.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
