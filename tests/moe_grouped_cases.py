"""The grouped-expert prompt launches as op-level cases: the table, the inputs and the reference (tests/test_moe_grouped_cpu.py, tests/test_gpu_moe_grouped.py).

A case is one launch as the model issues it on a prompt batch of a mixture-of-experts layer (Backend.moe_mul_mat_grouped): n_expert expert tensors of N rows of K,
the grouped activation rows (expert e owns rows [off_e, off_e + n_e)), the per-expert row counts.  form 0: the plane sets, one projection
(launch_mmq_planes_moe); 1: the plane sets, gate | up with SwiGLU (launch_mmq_planes_swiglu_moe); 2 / 3: the Q8_0-layout copies of MXFP4 experts, one / two
segments (launch_mmq_q80_moe; every case runs at each token tile of TILES_Q80).

The grouping is the model's: a case's selections ids [T][k] go through select_ref.moe_group, its counts are the launch's counts and grouped row slot_of[p] is
the activation row of pair p.  The reference is never a device intermediate: expert e's rows of oq.mul_mat (Q4_K / Q5_K / Q6_K), iq4xs_ref, tq_ref or
mxfp4_ref.mul_mat over that expert's tensor; form 1 is silu(g) * u with the sigmoid in f64 (test_ffn_gate_up_swiglu_launch of tests/test_gpu_iq4xs.py).

Tolerances, per expert batch against that batch's own scale: the re-association bound of the same kernel bodies, 2e-5 * max|ref_e| + 1e-6 for the plane
forms (tests/test_gpu_ops.py; the same figure tests/test_gpu_iq4xs.py and tests/test_gpu_tq.py use for their prompt batches), 4e-5 with SwiGLU; MXFP4: the
restatement's bits (tests/test_gpu_mxfp4.py)."""
from __future__ import annotations

import functools
import zlib

import numpy as np

import iq4xs_ref
import mxfp4_ref
import np_twin as tw
import oracle_py as oq
import select_ref
import tq_ref
from oracle_py import Q4_K, Q5_K, Q6_K

IQ4_XS, MXFP4, TQ1_0, TQ2_0 = iq4xs_ref.IQ4_XS, mxfp4_ref.MXFP4, tq_ref.TQ1_0, tq_ref.TQ2_0
TYPE_NAME = {Q4_K: "q4k", Q5_K: "q5k", Q6_K: "q6k", IQ4_XS: "iq4xs", TQ1_0: "tq1", TQ2_0: "tq2", MXFP4: "mxfp4"}
MINS_TYPES = (Q4_K, Q5_K)                        # the plane body with the block-sum term; every other plane type takes the body without it
BLOCK_BYTES = {Q4_K: 144, Q5_K: 176, Q6_K: 210}
P2_TOK = 256                                     # tokens of a workgroup tile of the plane kernels (csrc/mmq.hip)
TILES_Q80 = (1, 2, 4, 0)                         # "mmq_q80_tiles": 32, 64, 128 tokens per tile, and the launcher's choice
GUARD_ROWS = 2
MOE_MAX_EXPERT = 256


def _qwen(n_expert: int, seed: int):
    """(n_expert, ids [64][8]): 64 tokens x 8 distinct experts each, as a router of n_expert experts selects them."""
    rng = np.random.default_rng(seed)
    return n_expert, np.stack([rng.permutation(n_expert)[:8] for _ in range(64)]).astype(np.int32)


def _ids_of(counts, seed: int):
    """(n_expert, ids [R][1]): one selection per token with the given counts, in a seeded order - the grouping sorts them."""
    flat = np.repeat(np.arange(len(counts)), counts)
    return len(counts), np.random.default_rng(seed).permutation(flat).astype(np.int32).reshape(-1, 1)


# name -> (n_expert, selections ids [T][k]); the counts per expert are the selections' histogram
DISTS = {
    # empty experts first and in the middle; T = 1; both sides of the 256-token tile (257: a second tile of one row); both sides of the idle token half; the
    # last batch ends the array
    "edges8": _ids_of([0, 1, 255, 256, 257, 0, 129, 128], 1),
    "last_only": _ids_of([0, 0, 0, 600], 2),                       # tiles 0..2 of one expert, after walking every empty one
    "ones16": _ids_of([1] * 16, 3),                                # 16 tiles of ceil(16 / tile) + 16 = 17 slots: the slot bound at its tightest
    "qwen128": _qwen(128, 4),                                      # the meta words span more than one cache line; many empty experts
    "qwen160": _qwen(160, 5),                                      # ... and an expert count that is no multiple of 64
    "max256": _ids_of([2, 0] * 128, 6),                            # the walk at MOE_MAX_EXPERT
    # the copy form's tiles are 32 / 64 / 128 rows
    "edges9": _ids_of([0, 1, 31, 32, 33, 0, 65, 128, 129], 7),
    "edges_mt": _ids_of([63, 64, 127, 0, 385], 8),                 # the other side of the 64 and 128 boundaries; four tiles of 128
}


def counts_of(c: dict) -> np.ndarray:
    return np.bincount(DISTS[c["dist"]][1].reshape(-1), minlength=c["n_expert"]).astype(np.int32)


def tiles_used(counts, tile: int) -> int:
    return int(sum((int(n) + tile - 1) // tile for n in counts))


def slot_bound(counts, tile: int) -> int:
    """The token-tile slots the launchers size their grids with: every expert may end in a partial tile."""
    return (int(np.sum(counts)) + tile - 1) // tile + len(counts)


def q80_tile(counts, forced: int) -> int:
    """Rows per token tile of the copy form: 32 * mt, mt forced or from the mean batch (launch_mmq_q80_moe)."""
    mean = int(np.sum(counts)) // len(counts)
    mt = forced if forced else 4 if mean > 64 else 2 if mean > 32 else 1
    return 32 * mt


def tiles_of(c: dict):
    """Every tile size the case runs at."""
    return (P2_TOK,) if c["form"] < 2 else tuple(sorted({q80_tile(counts_of(c), f) for f in TILES_Q80}))


def case(form, t, dist, N, K, ld_pad):
    n_expert = DISTS[dist][0]
    name = f"f{form}_{TYPE_NAME[t]}_{dist}_n{N}_k{K}_ld{ld_pad}"
    return dict(name=name, form=form, type=t, dist=dist, n_expert=n_expert, N=N, K=K, ld_out=N + ld_pad, seed=zlib.crc32(name.encode()) % 100000)


def build_cases():
    c = []
    small = ("last_only", "ones16", "qwen128", "qwen160", "max256")
    # ---- planes, one projection.  Every distribution on Q4_K, Q5_K (the body with the block-sum term) and Q6_K (without); N 128 = one row tile, 1152 = nine
    # (the second group of eight in the workgroup-to-XCD mapping, with idle workgroups where row_tile >= n_row_tiles); K 256 = one super-block, 768, 1536
    for i, t in enumerate((Q4_K, Q5_K, Q6_K)):
        c.append(case(0, t, "edges8", 128, 256, 3))
        for j, d in enumerate(small):
            c.append(case(0, t, d, 128, 256 if (i + j) % 2 else 768, 3 * ((i + j) % 2)))
    for N, K, pad in ((128, 768, 0), (128, 1536, 3), (1152, 256, 0), (1152, 768, 3), (1152, 1536, 0)):
        c.append(case(0, Q4_K, "edges8", N, K, pad))               # (every N / K on a distribution with multi-tile experts)
    c.append(case(0, Q6_K, "last_only", 1152, 768, 3))
    c.append(case(0, Q6_K, "edges8", 1152, 1536, 3))
    c.append(case(0, Q5_K, "edges8", 1152, 768, 0))
    for t in (IQ4_XS, TQ1_0, TQ2_0):
        c.append(case(0, t, "edges8", 256, 512, 3))
        c.append(case(0, t, "qwen128", 128, 256, 0))
    # ---- planes, gate | up with SwiGLU.  N 128 = two 64-row tiles, 640 = ten (a second group of eight, six of its workgroups idle); K 256, 512
    for i, t in enumerate((Q4_K, Q5_K, Q6_K)):
        c.append(case(1, t, "edges8", 128, 256, 3))
        for j, d in enumerate(small):
            c.append(case(1, t, d, 128, 512 if (i + j) % 2 else 256, 3 * ((i + j + 1) % 2)))
    for N, K, pad in ((128, 512, 0), (640, 256, 3), (640, 512, 0)):
        c.append(case(1, Q5_K, "edges8", N, K, pad))
    c.append(case(1, Q6_K, "edges8", 640, 512, 3))
    c.append(case(1, Q6_K, "last_only", 640, 256, 0))
    c.append(case(1, Q4_K, "last_only", 640, 512, 3))
    for t in (IQ4_XS, TQ1_0, TQ2_0):
        c.append(case(1, t, "edges8", 128, 512, 0))
        c.append(case(1, t, "qwen128", 128, 256, 3))
    # ---- the Q8_0-layout copies of MXFP4 experts, one and two segments.  K 96: an odd block count; 2080: one chunk of 64 blocks and one more block; 4096
    for form in (2, 3):
        for j, d in enumerate(("edges8", "edges9", "edges_mt") + small):
            c.append(case(form, MXFP4, d, 128, 96, 3 * ((form + j) % 2)))
    c.append(case(3, MXFP4, "edges9", 384, 2080, 3))
    c.append(case(2, MXFP4, "edges9", 384, 4096, 0))
    c.append(case(2, MXFP4, "edges_mt", 128, 2080, 3))
    c.append(case(3, MXFP4, "edges8", 128, 4096, 0))
    c.append(case(2, MXFP4, "edges8", 384, 96, 3))
    names = [x["name"] for x in c]
    assert len(set(names)) == len(names)
    return c


def rand_weights(rng, t: int, n_elems: int) -> np.ndarray:
    """Random blocks with scaled d / dmin: rand_weights of tests/test_gpu_ops.py for the K-quants, gguf_synth.random_blocks for the other formats."""
    if t in BLOCK_BYTES:
        raw = rng.integers(0, 256, n_elems // 256 * BLOCK_BYTES[t], dtype=np.uint8)
        blk = raw.view(tw.DT[t])
        blk["d"] = (rng.uniform(0.5, 1.5, blk.size) * 1e-2).astype("<f2")
        if t in MINS_TYPES:
            blk["dmin"] = (rng.uniform(0.5, 1.5, blk.size) * 1e-2).astype("<f2")
        return raw
    import __graft_entry__ as ge
    return ge.load_pkg().gguf_synth.random_blocks(rng, t, n_elems, 0.05 if t == MXFP4 else 0.02)


def n_weights(c: dict) -> int:
    return 2 if c["form"] in (1, 3) else 1


def inputs(c: dict) -> dict:
    """The case's tensors, from its seed: W[s] (raw ggml rows, n_expert tensors back to back), ids / slot_of / counts / offs (the grouping), xp (the rows in
    pair order, t * k + j: normal with a per-row scale in 0.1 .. 4, so neighbouring experts' rows differ in magnitude) and x (the grouped rows)."""
    rng = np.random.default_rng(c["seed"])
    ne, N, K = c["n_expert"], c["N"], c["K"]
    Ws = [rand_weights(rng, c["type"], ne * N * K) for _ in range(n_weights(c))]
    ids = DISTS[c["dist"]][1]
    meta, slot_of, _ = select_ref.moe_group(ids, ne)
    R = ids.size
    xp = (rng.standard_normal((R, K)) * rng.uniform(0.1, 4.0, (R, 1))).astype(np.float32)
    x = np.empty_like(xp)
    x[slot_of] = xp
    return dict(W=Ws, ids=ids, slot_of=slot_of, counts=meta[:ne].copy(), offs=meta[ne:2 * ne].copy(), xp=xp, x=x, R=R)


def mul(t: int, W: np.ndarray, N: int, K: int, x: np.ndarray) -> np.ndarray:
    if t == IQ4_XS:
        return iq4xs_ref.mul_mat(W, N, K, x)
    if t in tq_ref.TYPES:
        return tq_ref.mul_mat(t, W, N, K, x)
    if t == MXFP4:
        return mxfp4_ref.mul_mat(W, N, K, x)
    return oq.mul_mat(t, W, N, K, x, oq.threads(16) if x.shape[0] * N * K >= 1 << 22 else 1)   # (a team of threads costs more than a few rows take)


def expert_weights(c: dict, W: np.ndarray, e: int) -> np.ndarray:
    rb = len(W) // c["n_expert"]
    return W[e * rb:(e + 1) * rb]


def swiglu(g: np.ndarray, u: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return (g / (1.0 + np.exp(-g.astype(np.float64)))).astype(np.float32) * u


def expert_rows(c: dict, inp: dict, e: int, x: np.ndarray):
    """The reference of rows x [n][K] through expert e: one array per out buffer."""
    prods = [mul(c["type"], expert_weights(c, W, e), c["N"], c["K"], x) for W in inp["W"]]
    return [swiglu(prods[0], prods[1])] if c["form"] == 1 else prods


def reference(c: dict, inp: dict):
    """-> list of f32 [R][N] per out buffer (two for form 3), in grouped row order."""
    out = [np.zeros((inp["R"], c["N"]), np.float32) for _ in range(2 if c["form"] == 3 else 1)]
    for e in range(c["n_expert"]):
        n, o = int(inp["counts"][e]), int(inp["offs"][e])
        if n:
            for dst, r in zip(out, expert_rows(c, inp, e, inp["x"][o:o + n])):
                dst[o:o + n] = r
    return out


def tol_rel(c: dict) -> float:
    """The relative part of the bound (the MXFP4 forms are compared for equality: their entry is the figure the neighbour-expert check scales by)."""
    return 4e-5 if c["form"] == 1 else 2e-5


def bound(c: dict, ref_e: np.ndarray) -> float:
    return 0.0 if c["form"] >= 2 else tol_rel(c) * float(np.abs(ref_e).max()) + 1e-6


@functools.lru_cache(maxsize=None)
def prepared(name: str):
    """(inputs, reference) of a case, computed once per process and shared: treat both as read-only."""
    c = BY_NAME[name]
    inp = inputs(c)
    ref = reference(c, inp)
    for a in list(inp.values()) + ref:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return inp, ref


CASES = build_cases()
BY_NAME = {c["name"]: c for c in CASES}
