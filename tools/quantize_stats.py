#!/usr/bin/env python3
"""Where the quantisation error of a GGUF file sits, per tensor, on the device: what upstream's llama-quantize-stats measures (the kernels are
csrc/quant_error.hip behind mi355_quant_error_rows).

  quantize_stats.py -m model.F16.gguf [--type q4_k --type q6_k ...] [--imatrix imatrix.gguf] [--include-layers RE] [--json out.json]
  quantize_stats.py -m model.F16.gguf --quantized model.Q4_K_M.gguf [--imatrix ...] [--include-layers RE] [--json out.json]

First form: every 2-D weight tensor (and every 3-D expert tensor) of the F32 / F16 / BF16 file is quantised on the device to each requested type (default:
the eight block types of the ten mixes) and compared with itself.  Second form: the tensors of the two files are matched by name and the quantised file's
blocks, whatever loadable type each tensor has, are compared with the source's.  1-D tensors, the router, rope_freqs and an encoder's tables are left out;
--include-layers RE takes exactly the tensors whose name matches instead.  Expert tensors go expert by expert with their own column weights (an expert the
matrix never saw gets the weight 1); rows go in chunks of at most 256 MiB of source.

Per tensor and type: the relative RMS error sqrt(sum e^2 / sum w^2); the importance-weighted one, sqrt(sum c e^2 / (mean(c) sum w^2)) with the matrix's column
weights c (the same figure without a matrix); the largest |e|.  Then, per type, the figures over the whole file and the ten worst tensors.  Refused by name
before a device is asked for: a tensor missing from one of the files, differing shapes, a 1-D tensor, a type the library does not decode or quantise."""
import argparse
import importlib.util
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

_spec = importlib.util.spec_from_file_location("mi355_quantize_tool", os.path.join(ROOT, "tools", "quantize.py"))
qt = importlib.util.module_from_spec(_spec)            # the GGUF reader, the column weights and the chunk size (tools/quantize.py)
_spec.loader.exec_module(qt)

DEFAULT_TYPES = ("q8_0", "q5_0", "q5_1", "q2_k", "q3_k", "q4_k", "q5_k", "q6_k")


class StatsError(ValueError):
    pass


def selected(tensors, include):
    """the tensors to compare, in file order; a 1-D tensor that --include-layers names is refused"""
    out = []
    for name, ne, t, data in tensors:
        if include is not None:
            if not re.search(include, name):
                continue
            if len(ne) < 2:
                raise StatsError(f"{name}: a 1-D tensor has no rows to compare")
        elif len(ne) < 2 or not name.endswith(".weight") or name.endswith(qt.COPIED):
            continue
        out.append((name, ne, t, data))
    if not out:
        raise StatsError("no tensor to compare" + (f" matches {include!r}" if include is not None else ""))
    return out


def plan_file(pkg, lib, src, types=None, quantized=None, imatrix=None, include=None):
    """Every refusal, without a device.  -> [(name, ne, source type, source payload, column weights or None, [(label, type, quantised payload or None)])]"""
    gs = pkg.gguf_synth
    by_name = {v.lower(): k for k, v in gs.TYPE_NAME.items()}
    cands = selected(qt.read_gguf(src)[1], include)
    im = qt.imx.read_imatrix(imatrix) if imatrix else None
    if quantized is None:
        wanted = []
        for label in types or DEFAULT_TYPES:
            t = by_name.get(label.lower())
            if t is None or not lib.mi355_quant_error_supported(t):
                raise StatsError(f"--type {label}: not a weight type the library decodes")
            if not lib.mi355_quantize_supported(t):
                raise StatsError(f"--type {label}: the device quantiser does not write {gs.TYPE_NAME[t]}")
            wanted.append((gs.TYPE_NAME[t], t))
    else:
        other = {name: (ne, t, data) for name, ne, t, data in qt.read_gguf(quantized)[1]}
        for name, _, _, _ in selected([(n, ne, t, d) for n, (ne, t, d) in other.items()], include):
            if name not in {c[0] for c in cands}:
                raise StatsError(f"{name}: in {quantized}, not in {src}")
    plan = []
    for name, ne, t, data in cands:
        if t not in qt.SRC_DTYPE:
            raise StatsError(f"{name}: the source tensor is {gs.TYPE_NAME.get(t, t)}, not F32, F16 or BF16")
        n_mat = int(ne[2]) if len(ne) == 3 else 1
        cw = qt.column_weights(im, name, int(ne[0]), n_mat) if im is not None else None
        if quantized is None:
            for label, qtype in wanted:
                if ne[0] % gs.BLOCK_ELEMS[qtype]:
                    raise StatsError(f"{name}: rows of {ne[0]} are no whole number of {label} blocks")
            plan.append((name, ne, t, data, cw, [(label, qtype, None) for label, qtype in wanted]))
            continue
        if name not in other:
            raise StatsError(f"{name}: in {src}, not in {quantized}")
        qne, qtype, qdata = other[name]
        if tuple(qne) != tuple(ne):
            raise StatsError(f"{name}: {' x '.join(map(str, ne))} in {src}, {' x '.join(map(str, qne))} in {quantized}")
        if not lib.mi355_quant_error_supported(qtype):
            raise StatsError(f"{name}: type {gs.TYPE_NAME.get(qtype, qtype)} in {quantized} is not a weight type the library decodes")
        plan.append((name, ne, t, data, cw, [(gs.TYPE_NAME[qtype], qtype, qdata)]))
    return plan


def figures(s, mean_c=1.0):
    """{rel_rms, weighted_rel, max_abs} of the sums s = (sum e^2, sum w^2, sum c e^2 / mean(c), max |e|)"""
    return {"rel_rms": float(np.sqrt(s[0] / s[1])) if s[1] > 0 else 0.0, "weighted_rel": float(np.sqrt(s[2] / (mean_c * s[1]))) if s[1] > 0 else 0.0,
            "max_abs": float(s[3]), "sum_e2": float(s[0]), "sum_w2": float(s[1])}


def stats_file(pkg, be, plan, chunk_bytes=qt.CHUNK_BYTES, out=print, on_call=None):
    """Runs the plan on Backend `be` (quantize_rows, quant_error_rows).  -> {"tensors": [...], "types": {label: summary}}"""
    gs = pkg.gguf_synth
    per_tensor, totals = [], {}
    for name, ne, t, data, cw, cases in plan:
        ne0 = int(ne[0])
        n_mat = int(ne[2]) if len(ne) == 3 else 1
        rows = int(np.prod(ne[1:])) // n_mat
        x = data[:ne0 * rows * n_mat * qt.SRC_DTYPE[t].itemsize].view(qt.SRC_DTYPE[t]).reshape(n_mat, rows, ne0)
        step = max(1, chunk_bytes // (ne0 * qt.SRC_DTYPE[t].itemsize))
        for label, qtype, qdata in cases:
            rb = gs.row_bytes(qtype, ne0)
            q = None if qdata is None else qdata[:rb * rows * n_mat].reshape(n_mat, rows, rb)
            s = np.zeros(4)
            for m in range(n_mat):                           # expert by expert, each with its own column weights
                c = None if cw is None else cw[m]
                for r0 in range(0, rows, step):
                    xs = np.ascontiguousarray(x[m, r0:r0 + step])
                    blocks = be.quantize_rows(qtype, xs, imatrix=c, src_type=t) if q is None else np.ascontiguousarray(q[m, r0:r0 + step])
                    e = be.quant_error_rows(xs, t, blocks, qtype, ne0, c)
                    if on_call:
                        on_call(label, xs.nbytes)
                    s[:2] += e[:, :2].sum(axis=0)
                    s[2] += e[:, 2].sum() / (float(np.mean(c, dtype=np.float64)) if c is not None and np.any(c) else 1.0)
                    s[3] = max(s[3], e[:, 3].max())
            f = dict(figures(s), name=name, type=label, shape=[int(v) for v in ne])
            per_tensor.append(f)
            tot = totals.setdefault(label, np.zeros(4))
            tot[:3] += s[:3]
            tot[3] = max(tot[3], s[3])
            out(f"{name:40s} [{' x '.join(str(v) for v in ne):>20s}] {label:>6s}  rel rms {f['rel_rms']:.6f}  weighted {f['weighted_rel']:.6f}  max |e| {f['max_abs']:.6g}")
    summary = {}
    for label, tot in totals.items():
        mine = sorted((f for f in per_tensor if f["type"] == label), key=lambda f: -f["rel_rms"])
        summary[label] = dict(figures(tot), tensors=len(mine), worst=[{"name": f["name"], "rel_rms": f["rel_rms"]} for f in mine[:10]])
        sm = summary[label]
        out(f"{label:>6s}: {len(mine)} tensors, rel rms {sm['rel_rms']:.6f}, weighted {sm['weighted_rel']:.6f}, max |e| {sm['max_abs']:.6g}; worst: " +
            ", ".join("%s %.4f" % (w["name"], w["rel_rms"]) for w in sm["worst"]))
    return {"tensors": per_tensor, "types": summary}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-m", "--model", required=True, help="the F32 / F16 / BF16 source file")
    ap.add_argument("--type", action="append", help="a block type to quantise to and measure (repeatable; default: " + ", ".join(DEFAULT_TYPES) + ")")
    ap.add_argument("--quantized", help="a quantised file of the same model to measure instead")
    ap.add_argument("--imatrix", help="an importance matrix written by tools/imatrix.py: column weights of the quantiser and of the weighted error")
    ap.add_argument("--include-layers", metavar="RE", help="only the tensors whose name matches")
    ap.add_argument("--json", help="write every figure here")
    args = ap.parse_args(argv)
    pkg = ge.load_pkg()
    try:
        if args.quantized and args.type:
            raise StatsError("--type and --quantized exclude each other")
        plan = plan_file(pkg, pkg.load_library(), args.model, args.type, args.quantized, args.imatrix, args.include_layers)
        be = pkg.Backend()
        times = {}                                           # per type: the source bytes compared and the error launches' upload / launch / download ms

        def on_call(label, nbytes):
            st = times.setdefault(label, {"source_bytes": 0, "upload_ms": 0.0, "kernel_ms": 0.0, "download_ms": 0.0, "calls": 0})
            for k, v in zip(("upload_ms", "kernel_ms", "download_ms"), be.quant_error_last_times()):
                st[k] += v
            st["source_bytes"] += int(nbytes)
            st["calls"] += 1

        t0 = time.perf_counter()
        res = stats_file(pkg, be, plan, on_call=on_call)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(dict(res, model=args.model, quantized=args.quantized, imatrix=args.imatrix, wall_s=round(time.perf_counter() - t0, 4), error_calls=times), f, indent=1)
                f.write("\n")
    except (StatsError, qt.QuantizeError, pkg.MI355Error, OSError) as e:
        print(f"quantize_stats: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
