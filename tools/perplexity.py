#!/usr/bin/env python3
"""Perplexity of a GGUF file over a text, and with --base the KL divergence from the file it was quantised from: what upstream's llama-perplexity prints
(the procedure is Context.perplexity / mi355_perplexity, restated from memory of llama.cpp's perplexity() and not pinned to its source).

  perplexity.py -m MODEL (-f TEXT | --tokens FILE.npy) [--base MODEL] [--ctx 512] [--ubatch 512] [--cache-type f16|q8_0|q4_0] [--chunks N] [--json OUT]
                [--host-score]

The text is tokenised with the model's tokenizer; every chunk starts with BOS only if the vocabulary adds one.  The contexts are opened with
logits_to_host = 0: the scoring reads the device logits and a few words per row come back.  --host-score does the same scoring through logits(i) and numpy
(float64 log-softmax of every scored row on the host), the path there was before the kernels, for comparison.  Prints the running line [1]x,[2]y,... of
per-chunk perplexities so far, then PPL = exp(mean nll) +/- PPL * sqrt((mean nll^2 - mean^2) / (count - 1)); with --base both perplexities, the mean KLD with
its standard error and the share of rows on which both models have the same top token; and the seconds per chunk."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

KV = {"f16": 1, "q8_0": 8, "q4_0": 2}
STAT_KEYS = ("n_chunks", "count", "top1", "dead", "same_top", "has_base", "stopped", "nll", "nll2", "nll_base", "nll2_base", "kl", "kl2")


def vocab_bos(model) -> int:
    """the BOS id if the vocabulary puts one in front of a text, else -1 (also for a file without a vocabulary)"""
    try:
        bos = int(model.lib.mi355_token_bos(model.h))
        with_, without = model.tokenize("a", add_special=True), model.tokenize("a", add_special=False)
    except Exception:
        return -1
    return bos if bos >= 0 and len(with_) == len(without) + 1 and with_[0] == bos else -1


def host_score(ctx, base, tokens, n_chunk, bos, n_ubatch, on_chunk):
    """Context.perplexity's procedure with the scoring on the host: every scored row crosses as a whole (logits(i)) and is reduced in float64."""
    first = n_chunk // 2
    st = dict.fromkeys(STAT_KEYS, 0)
    st.update(nll=0.0, nll2=0.0, nll_base=0.0, nll2_base=0.0, kl=0.0, kl2=0.0, has_base=int(base is not None))

    def log_softmax(row):
        v = row.astype(np.float64)
        v -= v.max()
        return v - math.log(np.exp(v).sum())

    for c in range(tokens.size // n_chunk):
        tk = tokens[c * n_chunk:(c + 1) * n_chunk].copy()
        if bos >= 0:
            tk[0] = bos
        for x in (ctx, base):
            if x is not None:
                x.kv_seq_rm(0, 0, -1)
        for i0 in range(0, n_chunk, n_ubatch):
            pos = np.arange(i0, min(i0 + n_ubatch, n_chunk))
            flags = ((pos >= first) & (pos <= n_chunk - 2)).astype(np.int8)
            for x in (ctx, base):
                if x is not None and x.decode(tk[pos], pos, logits=flags) != 0:
                    raise RuntimeError("decode failed")
            for i in np.flatnonzero(flags):
                t = int(tk[pos[i] + 1])
                lq = log_softmax(ctx.logits(int(i)))
                st["count"] += 1; st["nll"] -= lq[t]; st["nll2"] += lq[t] * lq[t]; st["top1"] += int(lq.argmax() == t)
                if base is not None:
                    lp = log_softmax(base.logits(int(i)))
                    kl = float((np.exp(lp) * (lp - lq)).sum())
                    st["nll_base"] -= lp[t]; st["nll2_base"] += lp[t] * lp[t]; st["kl"] += kl; st["kl2"] += kl * kl; st["same_top"] += int(lp.argmax() == lq.argmax())
        st["n_chunks"] = c + 1
        on_chunk(st)
    for x in (ctx, base):
        if x is not None:
            x.kv_seq_rm(0, 0, -1)
    return st


def mean_err(s, s2, n):
    m = s / n
    return m, math.sqrt(max(0.0, s2 / n - m * m) / (n - 1)) if n > 1 else float("nan")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-m", "--model", required=True)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("-f", "--file", help="a text file, tokenised with the model's tokenizer")
    src.add_argument("--tokens", help="a .npy file of token ids")
    ap.add_argument("--base", help="the f16 / Q8_0 file the model was made from: also prints its perplexity, the KL divergence and the same-top share")
    ap.add_argument("--ctx", type=int, default=512, help="chunk length")
    ap.add_argument("--ubatch", type=int, default=512)
    ap.add_argument("--cache-type", default="f16", choices=sorted(KV))
    ap.add_argument("--chunks", type=int, default=0, help="score only the first N chunks")
    ap.add_argument("--json", help="write the stats here")
    ap.add_argument("--host-score", action="store_true", help="score on the host through logits(i) and numpy instead of the device kernels")
    args = ap.parse_args()

    pkg = ge.load_pkg()
    pkg.Backend()
    model = pkg.Model(args.model)
    base_model = pkg.Model(args.base) if args.base else None
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
    kv = KV[args.cache_type]
    # (with the device kernels no row is ever read on the host; --host-score copies the rows when it asks for them)
    mk = lambda m: pkg.Context(m, n_ctx=args.ctx, n_batch=max(args.ubatch, 1), n_ubatch=args.ubatch, type_k=kv, type_v=kv, logits_to_host=False)
    ctx = mk(model)
    base = mk(base_model) if base_model is not None else None

    t_chunk = [time.perf_counter()]

    def on_chunk(st):
        t_chunk.append(time.perf_counter())
        if st["count"] > 0:
            print(f"[{st['n_chunks']}]{math.exp(st['nll'] / st['count']):.4f},", end="", flush=True)
        return 0

    if args.host_score:
        st = host_score(ctx, base, tokens, args.ctx, bos, args.ubatch, on_chunk)
    else:
        st = ctx.perplexity(tokens, args.ctx, bos=bos, base=base, callback=on_chunk)
    print()
    out = {k: st[k] for k in STAT_KEYS}
    secs = np.diff(t_chunk)
    out.update(mode="host" if args.host_score else "device", n_chunk=args.ctx, n_ubatch=args.ubatch, cache=args.cache_type, bos=bos,
               seconds_per_chunk=[round(float(s), 4) for s in secs], seconds_per_chunk_median=round(float(np.median(secs)), 4) if secs.size else None)
    n = out["count"]
    if n > 0:
        m, e = mean_err(out["nll"], out["nll2"], n)
        out.update(ppl=math.exp(m), ppl_err=math.exp(m) * e)
        print(f"PPL = {out['ppl']:.4f} +/- {out['ppl_err']:.5f}   ({n} tokens, {out['n_chunks']} chunks of {args.ctx}, top-1 {out['top1'] / n:.4f}, skipped {out['dead']})")
        if base is not None:
            mb, eb = mean_err(out["nll_base"], out["nll2_base"], n)
            mk_, ek = mean_err(out["kl"], out["kl2"], n)
            out.update(ppl_base=math.exp(mb), ppl_base_err=math.exp(mb) * eb, mean_kl=mk_, mean_kl_err=ek, same_top_share=out["same_top"] / n)
            print(f"base PPL = {out['ppl_base']:.4f} +/- {out['ppl_base_err']:.5f}")
            print(f"mean KLD = {mk_:.6f} +/- {ek:.6f}   same top = {100.0 * out['same_top_share']:.3f} %")
    if secs.size:
        print(f"{float(np.median(secs)):.4f} s per chunk (median of {secs.size}; first {float(secs[0]):.4f}), scoring on the {out['mode']}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    for c in (ctx, base):
        if c is not None:
            c.close()
    model.close()
    if base_model is not None:
        base_model.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
