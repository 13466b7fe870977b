#!/usr/bin/env python3
"""A control vector from pairs of prompts: what upstream's llama-cvector-generator writes and --control-vector reads (the procedure and the
file format are restated from memory of llama.cpp and not pinned to its source).

  cvector_generator.py -m MODEL --positive-file P --negative-file N -o OUT.gguf [--method pca|mean] [--pca-iter 1000] [--pca-batch 100] [--seed S]
                       [--ctx N] [--cache-type f16|q8_0|q4_0]

P and N hold one prompt per line and are paired line by line.  Each prompt is tokenised with BOS and the shorter of a pair is padded with the token of " "
to the longer one's length.  Both run with the layer taps on; for every layer the rows positive - negative are formed, rows that are all zero are dropped
and the pairs are concatenated.  direction.il, il = 1 .. n_layer - 1, is the direction of the rows taken AFTER layer il - the rows Context.apply_cvec adds
it to - by the power method on the device (Backend.cvec_direction: deterministic in its arguments; the start vectors come from numpy's seeded generator) or
as the normalised mean, with the sign that points from the negative prompts to the positive ones.  The file: general.architecture "controlvector",
controlvector.model_hint, controlvector.layer_count and the F32 tensors direction.il."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

KV = {"f16": 1, "q8_0": 8, "q4_0": 2}
GGML_F32 = 0


def read_prompts(path: str) -> list:
    with open(path, encoding="utf-8") as f:
        return [ln.rstrip("\r\n") for ln in f if ln.strip()]


def pad_pair(pos, neg, pad: int):
    """The two token lists at the longer one's length, the shorter padded with `pad` at its end."""
    pos, neg = list(pos), list(neg)
    n = max(len(pos), len(neg))
    return pos + [pad] * (n - len(pos)), neg + [pad] * (n - len(neg))


def diff_rows(taps_pos: np.ndarray, taps_neg: np.ndarray) -> list:
    """taps [n_layer][T][E] of the two prompts of a pair -> per layer the rows pos - neg (f32) without the rows that are all zero."""
    d = (np.asarray(taps_pos, np.float32) - np.asarray(taps_neg, np.float32)).astype(np.float32)
    return [layer[np.any(layer != 0, axis=1)] for layer in d]


def generate(token_pairs, run_taps, direction, n_layer: int, n_embd: int, method: str = "pca", seed: int = 0) -> dict:
    """{il: unit direction f32 [n_embd]} for il = 1 .. n_layer - 1.  token_pairs: [(pos tokens, neg tokens)] of equal lengths; run_taps(tokens) -> the layers'
    output rows [n_layer][T][n_embd]; direction(rows, init, method) -> the direction of rows [R][n_embd] (init: the start vector of pca, None for mean).  A layer
    all of whose rows were dropped gets no vector."""
    per_layer = [[] for _ in range(n_layer)]
    for pos, neg in token_pairs:
        assert len(pos) == len(neg)
        for il, rows in enumerate(diff_rows(run_taps(pos), run_taps(neg))):
            per_layer[il].append(rows)
    rng = np.random.default_rng(seed)
    out = {}
    for il in range(1, n_layer):
        init = rng.standard_normal(n_embd).astype(np.float32)       # (drawn for every layer, whatever the method: a layer's start does not depend on the others)
        init /= np.float32(np.linalg.norm(init))
        rows = np.concatenate(per_layer[il]) if per_layer[il] else np.zeros((0, n_embd), np.float32)
        if rows.shape[0] == 0:
            continue
        out[il] = np.asarray(direction(rows, init if method == "pca" else None, method), np.float32)
    return out


def write_cvec(path: str, dirs: dict, model_hint: str, gguf_writer=None) -> None:
    w = (gguf_writer or ge.load_pkg().gguf_synth.GGUFWriter)()
    w.add("general.architecture", "str", "controlvector")
    w.add("controlvector.model_hint", "str", model_hint)
    w.add("controlvector.layer_count", "i32", max(dirs) if dirs else 0)
    for il in sorted(dirs):
        v = np.ascontiguousarray(dirs[il], "<f4")
        w.add_tensor(f"direction.{il}", (v.size,), GGML_F32, v.tobytes())
    w.write(path)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("-m", "--model", required=True)
    ap.add_argument("--positive-file", required=True)
    ap.add_argument("--negative-file", required=True)
    ap.add_argument("-o", "--output", default="control_vector.gguf")
    ap.add_argument("--method", choices=("pca", "mean"), default="pca")
    ap.add_argument("--pca-iter", type=int, default=1000)
    ap.add_argument("--pca-batch", type=int, default=100)
    ap.add_argument("--pca-tol", type=float, default=1e-7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ctx", type=int, default=512)
    ap.add_argument("--cache-type", choices=sorted(KV), default="f16")
    a = ap.parse_args(argv)
    pos_p, neg_p = read_prompts(a.positive_file), read_prompts(a.negative_file)
    if not pos_p or len(pos_p) != len(neg_p):
        print(f"error: {len(pos_p)} positive and {len(neg_p)} negative prompts: the files must pair line by line", file=sys.stderr)
        return 1
    pkg = ge.load_pkg()
    be = pkg.Backend()
    m = pkg.Model(a.model)
    arch = m.meta("general.architecture")
    pad = m.tokenize(" ", add_special=False)
    if not pad:
        print("error: the tokenizer gives no token for \" \"", file=sys.stderr)
        return 1
    pairs = [pad_pair(m.tokenize(p, add_special=True, parse_special=True), m.tokenize(n, add_special=True, parse_special=True), pad[0]) for p, n in zip(pos_p, neg_p)]
    longest = max(len(p) for p, _ in pairs)
    if longest > a.ctx:
        print(f"error: a prompt of {longest} tokens does not fit --ctx {a.ctx}", file=sys.stderr)
        return 1
    c = pkg.Context(m, n_ctx=a.ctx, n_batch=a.ctx, n_ubatch=a.ctx, type_k=KV[a.cache_type], type_v=KV[a.cache_type])   # (a prompt is one micro-batch: the taps hold one)
    c.enable_taps(True)

    def run_taps(tokens):
        c.kv_clear()
        if c.decode(tokens, np.arange(len(tokens))) != 0:
            raise RuntimeError("decode failed")
        return np.stack([c.layer_out(il, len(tokens)).reshape(len(tokens), -1) for il in range(m.n_layer)])

    stats = []

    def direction(rows, init, method):
        d, iters, dist = be.cvec_direction(rows, init, method, a.pca_iter, a.pca_batch, a.pca_tol)
        stats.append((rows.shape[0], iters, dist))
        return d

    dirs = generate(pairs, run_taps, direction, m.n_layer, m.n_embd, a.method, a.seed)
    for il, (rows, iters, dist) in zip(sorted(dirs), stats):
        print(f"layer {il}: {rows} rows, {iters} iterations, last distance {dist:.3g}")
    write_cvec(a.output, dirs, arch or os.path.basename(a.model))
    print(f"wrote {a.output}: {len(dirs)} directions of {m.n_embd} from {len(pairs)} prompt pairs ({a.method})")
    c.close(); m.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
