"""float64 restatement of the device sampler's tail (csrc/sample.hip) as host/sampling.cc's Sampler::finish states the chain, and Philox4x32-10 from its
published round function.  No f32 emulation: the candidates' f32 logits are taken as they are and everything after them is float64 (the one f32 value the
chain itself defines is the typical-p sort key, which the host casts to float)."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(seed: int, counter: int, stream: int):
    """key = seed (lo, hi); counter words = (counter lo, counter hi, stream, 0)"""
    c = [counter & MASK, (counter >> 32) & MASK, stream & MASK, 0]
    k = [seed & MASK, (seed >> 32) & MASK]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return c


def philox_u(seed: int, counter: int, stream: int) -> np.float32:
    return np.float32((philox4x32_10(seed, counter, stream)[0] >> 8) * 2.0 ** -24)


def chain(tok, logit, top_k=0, top_p=1.0, min_p=0.0, typ_p=1.0, temp=1.0, min_keep=0, **_):
    """(kept tokens, their final probabilities float64, margin): margin = the smallest relative distance between a threshold and a value compared with it."""
    tok, l = np.asarray(tok), np.asarray(logit, np.float32).astype(np.float64)
    mk = max(int(min_keep), 1)
    n = len(l) if top_k <= 0 else min(len(l), max(int(top_k), mk))
    tok, l = tok[:n], l[:n]
    if not np.isfinite(l[0]):
        return np.array([-1]), np.array([0.0]), np.inf
    if temp <= 0:
        return tok[:1], np.array([1.0]), np.inf
    top_p, min_p, typ_p, temp = (float(np.float32(v)) for v in (top_p, min_p, typ_p, temp))
    p = np.exp(l - l[0])
    p /= p.sum()
    margin = np.inf
    if typ_p < 1.0 and n > 1:
        ent = -(p[p > 0] * np.log(p[p > 0])).sum()
        dev = np.abs(-np.log(np.maximum(p, float(np.float32(1e-30)))) - ent).astype(np.float32)
        order = np.lexsort((np.arange(n), dev))
        cum = np.cumsum(p[order])
        hit = [i for i in range(n) if cum[i] > typ_p and i + 1 >= mk]
        margin = min(margin, np.abs(cum - typ_p).min() / typ_p)
        keep = np.sort(order[:hit[0] + 1 if hit else n])
        tok, p = tok[keep], p[keep] / p[keep].sum()
    if top_p < 1.0:
        cum = np.cumsum(p)
        hit = [i for i in range(len(p)) if cum[i] >= top_p and i + 1 >= mk]
        margin = min(margin, np.abs(cum - top_p).min() / top_p)
        last = hit[0] + 1 if hit else len(p)
        tok, p = tok[:last], p[:last] / p[:last].sum()
    if min_p > 0.0:
        thr = p[0] * min_p
        hit = [i for i in range(len(p)) if p[i] < thr and i >= mk]
        margin = min(margin, np.abs(p - thr).min() / thr)
        last = max(hit[0] if hit else len(p), 1)
        tok, p = tok[:last], p[:last] / p[:last].sum()
    p = p ** (1.0 / temp)
    return tok, p / p.sum(), margin


def draw(p, u: float) -> int:
    """index of the first candidate whose inclusive prefix sum exceeds u * total; the last one if none does"""
    c = np.cumsum(p)
    hit = np.nonzero(c > u * c[-1])[0]
    return int(hit[0]) if len(hit) else len(p) - 1
