"""float64 restatement of the whole-row device sampler (csrc/sample_vocab.hip): the adjustments in f32 as include/mi355_llama.h documents them at
mi355_op_topk_rows, the order (logit descending, token ascending, -0.0 == +0.0) by numpy.lexsort, the plain chain through sample_ref.chain, and the
mirostat-2 branch of Sampler::sample_chain (host/sampling.cc) restated."""
import numpy as np

import sample_ref as ref

def adjusted(row, adj=None, penalty_repeat=1.0, penalty_freq=0.0, penalty_present=0.0, **_):
    l = np.array(row, np.float32)
    for tok, bias, cnt in zip(*(adj or ([], [], []))):
        v = np.float32(l[tok] + np.float32(bias))
        if cnt > 0:
            v = np.float32(v * np.float32(penalty_repeat)) if v <= 0 else np.float32(v / np.float32(penalty_repeat))
            v = np.float32(v - np.float32(np.float32(np.float32(cnt) * np.float32(penalty_freq)) + np.float32(penalty_present)))
        l[tok] = v
    return l

def ordered(l):
    """(tokens, logits) best first"""
    o = np.lexsort((np.arange(len(l)), -(l + np.float32(0.0))))
    return o.astype(np.int32), l[o]

def plain(row, params, adj=None):
    """(kept tokens, their probabilities float64, margin) of the plain chain over the whole row"""
    tok, l = ordered(adjusted(row, adj, **params))
    return ref.chain(tok, l, **params)

def mirostat2(row, params, mu, adj=None):
    """(kept tokens, their probabilities float64, margin): temperature, softmax over the row, the prefix whose surprise does not exceed mu, renormalised"""
    tok, l = ordered(adjusted(row, adj, **params))
    l = l.astype(np.float64)
    if not np.isfinite(l[0]):
        return np.array([-1]), np.array([0.0]), np.inf
    p = np.exp((l - l[0]) / float(np.float32(params.get("temp", 1.0))))
    p /= p.sum()
    s = -np.log2(np.maximum(p, float(np.float32(1e-37))))
    over = np.nonzero(s > mu)[0]
    keep = max(int(over[0]) if len(over) else len(p), 1)
    return tok[:keep], p[:keep] / p[:keep].sum(), float(np.abs(s - mu).min() / max(abs(mu), 1.0))
