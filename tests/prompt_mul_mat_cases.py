"""The dense prompt batch's mat-mul launches as op-level cases: the table, the inputs and the oracle reference (tests/test_prompt_mul_mat_cpu.py,
tests/test_gpu_prompt_mul_mat.py).

A case is one launch as the model issues it (Backend.prompt_mul_mat): 1..3 K-quant tensors over one activation of T rows, an epilogue (store / residual add /
SwiGLU), the producer of the activation (prologue 0: the quantiser, then launch_mmq_prep; 1: the norm; 2: SwiGLU; 3: the quantiser - each of 1..3 writing the
bh / bl block-sum planes itself), the launcher (form 0: the model's choice; 1: K-split; 2: plane sets; 3: expansion on the fly) and the debug options that pick
the tile form and the K split ("mmq_tiles", "mmq_split").  `path` is what the launch must take (Backend.prompt_mul_mat's dict).

The reference is the oracle alone, never a device intermediate: oq.rms_norm(x, eps) * w rounded to f32, or oq.silu(g) * u, or x; oq.quantize(Q8_K, .); one
vec_dot per row (oq.mul_mat is that loop; test_prompt_mul_mat_cpu checks it against oq.vec_dot); then resid + y as one f32 add, or oq.silu(y0) * y1.  IQ4_XS is
not in the oracle: its rows come from tests/iq4xs_ref.py over the oracle's Q8_K blocks.

Tolerances are the project's: 2e-5 * max|ref| + 1e-6 per segment for store and add, 4e-5 * max|ref| + 1e-6 for a SwiGLU epilogue (tests/test_gpu_ops.py).
One flipped activation code moves a result by about 1e-3 of its scale, and the device's sum of squares or its expf may differ from the oracle's in the last
place, so a case whose activation is computed (prologues 1 and 2) must not sit on a rounding boundary: codes_stable() asserts that the oracle's codes are the
same for y, y * (1 - 2^-23) and y * (1 + 2^-23); the seeds below are those for which it holds."""
from __future__ import annotations

import zlib

import numpy as np

import iq4xs_ref
import np_twin as tw
import oracle_py as oq
from oracle_py import Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, Q8_K

IQ4_XS = iq4xs_ref.IQ4_XS
STORE, ADD, SWIGLU = 0, 1, 2
FORM_MODEL, FORM_KSPLIT, FORM_PLANES, FORM_FLY = 0, 1, 2, 3
KERNEL_KSPLIT, KERNEL_PLANES_256X32, KERNEL_PLANES_128X128, KERNEL_LDS, KERNEL_FLY = 1, 2, 3, 4, 5
EPS = 1e-5
ERR_ARG = -103                                                   # MI355_ERR_ARG
BLOCK_BYTES = {Q4_K: 144, Q5_K: 176, Q6_K: 210, Q2_K: 84, Q3_K: 110, IQ4_XS: 136}
TYPE_NAME = {Q4_K: "q4k", Q5_K: "q5k", Q6_K: "q6k", Q2_K: "q2k", Q3_K: "q3k", IQ4_XS: "iq4xs"}
KQ = (Q4_K, Q5_K, Q6_K)
PLANES_ONLY = (Q2_K, Q3_K, IQ4_XS)
HAS_MINS = (Q4_K, Q5_K, Q2_K)            # the unsigned plane format (a block-sum term); Q6_K, Q3_K and IQ4_XS expand to signed codes


def path(kernel, T=0, n_split=1, mixed=0, swiglu=0, prep=1):
    return dict(kernel=kernel, token_tiles=(1 if T <= 32 else 2) if kernel == KERNEL_KSPLIT else 0, n_split=n_split, mixed=mixed, swiglu=swiglu, prep=prep)


def case(name, types, Ns, K, T, form, pth, epi=STORE, prologue=0, tiles=0, split=0, ld_pad=3, refused=False):
    return dict(name=name, types=tuple(types), Ns=tuple(Ns), K=K, T=T, form=form, epi=epi, prologue=prologue, tiles=tiles, split=split, ld_pad=ld_pad,
                path=pth, refused=refused, seed=0)


def names(ts):
    return "_".join(TYPE_NAME[t] for t in ts)


def build_cases():
    c = []
    # ---- the residual epilogue, one tensor (each also runs in place and as a store: test_gpu_prompt_mul_mat)
    for t in (Q4_K, Q6_K, Q5_K):                                 # K-split: one token tile with ragged rows; two token tiles, the second ragged; fewer rows than a tile
        c.append(case(f"add_ksplit_{TYPE_NAME[t]}_k512_n37_t5", (t,), (37,), 512, 5, FORM_KSPLIT, path(KERNEL_KSPLIT, 5), epi=ADD))
    for t in (Q4_K, Q6_K):
        c.append(case(f"add_ksplit_{TYPE_NAME[t]}_k512_n37_t33", (t,), (37,), 512, 33, FORM_KSPLIT, path(KERNEL_KSPLIT, 33), epi=ADD))
        c.append(case(f"add_ksplit_{TYPE_NAME[t]}_k256_n5_t9", (t,), (5,), 256, 9, FORM_KSPLIT, path(KERNEL_KSPLIT, 9), epi=ADD))
    for t in (Q4_K, Q6_K, Q5_K, Q2_K, Q3_K, IQ4_XS):             # planes 256 x 32: two row tiles, two token tiles, both ragged
        c.append(case(f"add_planes1_{TYPE_NAME[t]}_k512_n300_t40", (t,), (300,), 512, 40, FORM_PLANES, path(KERNEL_PLANES_256X32), epi=ADD, tiles=1))
    for t in (Q4_K, Q6_K):
        # planes 128 x 128: the second tile of rows holds 2, of tokens 1
        c.append(case(f"add_planes2_{TYPE_NAME[t]}_k512_n130_t129", (t,), (130,), 512, 129, FORM_PLANES, path(KERNEL_PLANES_128X128), epi=ADD, tiles=2))
        # the 128 x 256 LDS kernel, unsplit: the second token tile holds one token, so the residual's token clamp is live
        c.append(case(f"add_lds_{TYPE_NAME[t]}_k512_n130_t257", (t,), (130,), 512, 257, FORM_PLANES, path(KERNEL_LDS), epi=ADD, tiles=4, split=1))
        # ... split over K three ways (super-blocks 1 | 1 | 2): mmq_splitk_reduce_kernel adds the residual; and a forced split of 4 over one super-block, clamped to 1
        c.append(case(f"add_lds_split3_{TYPE_NAME[t]}_k1024_n132_t140", (t,), (132,), 1024, 140, FORM_PLANES, path(KERNEL_LDS, n_split=3), epi=ADD, tiles=4, split=3, ld_pad=4))
        c.append(case(f"add_lds_split4_clamped_{TYPE_NAME[t]}_k256_n132_t140", (t,), (132,), 256, 140, FORM_PLANES, path(KERNEL_LDS), epi=ADD, tiles=4, split=4))
        for tiles in (1, 2):                                     # expansion on the fly, both tile forms
            c.append(case(f"add_fly{tiles}_{TYPE_NAME[t]}_k512_n70_t40", (t,), (70,), 512, 40, FORM_FLY, path(KERNEL_FLY), epi=ADD, tiles=tiles))
    # ---- several segments over concatenated plane sets: one 256-row tile spans all three, every 32-row wave tile picks its own
    qkv, qkv_n = (Q4_K, Q5_K, Q4_K), (96, 32, 40)
    c.append(case("multi_planes1_q4k_q5k_q4k_t40", qkv, qkv_n, 512, 40, FORM_PLANES, path(KERNEL_PLANES_256X32), tiles=1))
    c.append(case("multi_planes2_q4k_q5k_q4k_t129", qkv, qkv_n, 512, 129, FORM_PLANES, path(KERNEL_PLANES_128X128), tiles=2))
    c.append(case("multi_lds_q4k_q5k_q4k_t257", qkv, qkv_n, 512, 257, FORM_PLANES, path(KERNEL_LDS), tiles=4, split=1))
    c.append(case("multi_planes1_q6k_q6k_t40", (Q6_K, Q6_K), (64, 37), 512, 40, FORM_PLANES, path(KERNEL_PLANES_256X32), tiles=1))
    c.append(case("multi_lds_q6k_q6k_t257", (Q6_K, Q6_K), (64, 37), 512, 257, FORM_PLANES, path(KERNEL_LDS), tiles=4, split=1))
    # the two plane formats in one launch (mmq_planes2_kernel<2>, mins_mask): segments end on 128-row tiles
    c.append(case("mixed_lds_q4k_q4k_q6k_t257", (Q4_K, Q4_K, Q6_K), (128, 128, 72), 512, 257, FORM_PLANES, path(KERNEL_LDS, mixed=1), tiles=4, split=1))
    c.append(case("mixed_lds_q6k_q5k_t140", (Q6_K, Q5_K), (256, 40), 512, 140, FORM_PLANES, path(KERNEL_LDS, mixed=1), tiles=4, split=1))
    c.append(case("mixed_lds_split2_q4k_q4k_q6k_k1024_t140", (Q4_K, Q4_K, Q6_K), (128, 128, 64), 1024, 140, FORM_PLANES, path(KERNEL_LDS, n_split=2, mixed=1), tiles=4,
                  split=2, ld_pad=4))
    for t in (Q4_K, Q6_K):                                       # gate | up with SwiGLU in the LDS kernel's epilogue: 64 rows of each per workgroup, the second ragged
        c.append(case(f"swiglu_lds_{TYPE_NAME[t]}_k512_n96_t257", (t, t), (96, 96), 512, 257, FORM_PLANES, path(KERNEL_LDS, swiglu=1), epi=SWIGLU, tiles=4))
    # ---- several segments on the K-split kernel: tile0 = 0, 3, 5 with ragged last tiles
    for T in (9, 48):
        c.append(case(f"multi_ksplit_q4k_q4k_q6k_t{T}", (Q4_K, Q4_K, Q6_K), (70, 37, 8), 512, T, FORM_KSPLIT, path(KERNEL_KSPLIT, T)))
    c.append(case("multi_ksplit_q5k_q6k_t3", (Q5_K, Q6_K), (33, 33), 512, 3, FORM_KSPLIT, path(KERNEL_KSPLIT, 3)))
    for t in (Q4_K, Q6_K):
        for T in (5, 32, 40):                                    # the SwiGLU pair: mmq_ksplit_kernel<1, true> up to 32 tokens, <2, true> beyond
            c.append(case(f"swiglu_ksplit_{TYPE_NAME[t]}_n37_t{T}", (t, t), (37, 37), 512, T, FORM_KSPLIT, path(KERNEL_KSPLIT, T, swiglu=1), epi=SWIGLU))
    # ---- the producers that write bh / bl themselves, one case per consuming kernel family (the LDS kernel reads the int16 block sums)
    for pro, tag in ((1, "norm"), (2, "swiglu"), (3, "quant")):
        c.append(case(f"pro_{tag}_ksplit_q4k_k1024_n37_t9", (Q4_K,), (37,), 1024, 9, FORM_KSPLIT, path(KERNEL_KSPLIT, 9, prep=0), prologue=pro))
        c.append(case(f"pro_{tag}_planes1_q4k_k1024_n70_t40", (Q4_K,), (70,), 1024, 40, FORM_PLANES, path(KERNEL_PLANES_256X32, prep=0), prologue=pro, tiles=1))
        c.append(case(f"pro_{tag}_fly_q5k_k1024_n70_t40", (Q5_K,), (70,), 1024, 40, FORM_FLY, path(KERNEL_FLY, prep=0), prologue=pro, tiles=1))
        c.append(case(f"pro_{tag}_lds_q5k_k1024_n130_t40", (Q5_K,), (130,), 1024, 40, FORM_PLANES, path(KERNEL_LDS, prep=0), prologue=pro, tiles=4, split=1))
    # ---- form 0, the model's choice (host/runtime.cc prompt_mul_mat_choice); the tile options pin what would otherwise follow the device's CU count
    c.append(case("model_one_q4k_t5", (Q4_K,), (37,), 512, 5, FORM_MODEL, path(KERNEL_KSPLIT, 5), epi=ADD))
    c.append(case("model_one_q4k_t260", (Q4_K,), (70,), 512, 260, FORM_MODEL, path(KERNEL_PLANES_256X32), epi=ADD, tiles=1))      # past the K-split kernel's 256 tokens
    c.append(case("model_one_q3k_t40", (Q3_K,), (70,), 512, 40, FORM_MODEL, path(KERNEL_PLANES_256X32), tiles=1))                   # a planes-only type
    c.append(case("model_qkv_t9", (Q4_K, Q4_K, Q6_K), (128, 128, 72), 512, 9, FORM_MODEL, path(KERNEL_KSPLIT, 9)))
    c.append(case("model_qkv_mixed_t260", (Q4_K, Q4_K, Q6_K), (128, 128, 72), 512, 260, FORM_MODEL, path(KERNEL_LDS, mixed=1), tiles=4, split=1))
    c.append(case("model_qkv_q6k_alone_t260", (Q4_K, Q4_K, Q6_K), (128, 128, 72), 512, 260, FORM_MODEL, path(KERNEL_PLANES_256X32), tiles=1))   # Q | K fuse, V follows alone
    c.append(case("model_gate_up_t5", (Q4_K, Q4_K), (37, 37), 512, 5, FORM_MODEL, path(KERNEL_KSPLIT, 5, swiglu=1), epi=SWIGLU))
    c.append(case("model_gate_up_t260", (Q4_K, Q4_K), (96, 96), 512, 260, FORM_MODEL, path(KERNEL_LDS, swiglu=1), epi=SWIGLU, tiles=4))
    # ---- what a launcher refuses: MI355_ERR_ARG, nothing launched, the buffers 0xFF
    c.append(case("refuse_two_segments_with_residual", (Q4_K, Q4_K), (32, 32), 512, 40, FORM_PLANES, None, epi=ADD, tiles=1, refused=True))
    c.append(case("refuse_planes_segment_not_32_rows", (Q4_K, Q4_K), (37, 32), 512, 40, FORM_PLANES, None, tiles=1, refused=True))
    c.append(case("refuse_mixed_segment_not_128_rows", (Q4_K, Q6_K), (96, 64), 512, 257, FORM_PLANES, None, tiles=4, refused=True))
    c.append(case("refuse_mixed_without_lds_kernel_t40", (Q4_K, Q4_K, Q6_K), (128, 128, 72), 512, 40, FORM_PLANES, None, tiles=0, refused=True))
    c.append(case("refuse_swiglu_pair_unequal_types", (Q4_K, Q6_K), (37, 37), 512, 5, FORM_KSPLIT, None, epi=SWIGLU, refused=True))
    # (the model runs the pair of a batch of 33..128 tokens WITHOUT SwiGLU in the epilogue and a pass of its own behind it: not one launch)
    c.append(case("refuse_model_gate_up_t40_swiglu_behind", (Q4_K, Q4_K), (37, 37), 512, 40, FORM_MODEL, None, epi=SWIGLU, refused=True))
    nm = [x["name"] for x in c]
    assert len(set(nm)) == len(nm)
    for x in c:
        x["seed"] = SEEDS.get(x["name"], zlib.crc32(x["name"].encode()) % 100000)
    return c


# seeds changed from the default (a checksum of the name) because codes_stable() failed with it: name -> seed
SEEDS: dict = {"pro_swiglu_fly_q5k_k1024_n70_t40": 1}


def rand_weights(rng, t: int, n_elems: int, dscale: float = 1e-2) -> np.ndarray:
    """Random blocks with sane scales (tests/test_gpu_ops.py rand_weights; every byte value is a valid IQ4_XS code as well)."""
    raw = rng.integers(0, 256, n_elems // 256 * BLOCK_BYTES[t], dtype=np.uint8)
    blk = raw.view(iq4xs_ref.DT if t == IQ4_XS else tw.DT[t])
    blk["d"] = (rng.uniform(0.5, 1.5, blk.size) * dscale).astype("<f2")
    if t in (Q4_K, Q5_K, Q2_K):
        blk["dmin"] = (rng.uniform(0.5, 1.5, blk.size) * dscale).astype("<f2")
    return raw


def inputs(c: dict) -> dict:
    """The case's tensors, from its seed: W[s] (raw ggml rows), x ([T][K]; prologue 2: [2][T][K], gate then up), norm_w, resid (whole padded rows).  Rows are
    scaled per token by a factor in [0.1, 4], so that the activation's f32 block scales differ from token to token."""
    rng = np.random.default_rng(c["seed"])
    K, T = c["K"], c["T"]
    Ws = [rand_weights(rng, t, N * K) for t, N in zip(c["types"], c["Ns"])]
    x = (rng.standard_normal((T, K)) * rng.uniform(0.1, 4.0, (T, 1))).astype(np.float32)
    if c["prologue"] == 2:
        x = np.stack([(rng.standard_normal((T, K)) * 1.5).astype(np.float32), x])
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32) if c["prologue"] == 1 else None
    resid = rng.standard_normal((T, c["Ns"][0] + c["ld_pad"])).astype(np.float32) if c["epi"] == ADD else None
    return dict(W=Ws, x=x, nw=nw, resid=resid)


def activation(c: dict, inp: dict) -> np.ndarray:
    """The f32 rows the launch quantises: prologue 1 - oq.rms_norm(x, eps) * w rounded to f32; 2 - oq.silu(g) * u; else x."""
    if c["prologue"] == 1:
        return np.stack([(oq.rms_norm(r, EPS) * inp["nw"]).astype(np.float32) for r in inp["x"]])
    if c["prologue"] == 2:
        return (oq.silu(inp["x"][0]) * inp["x"][1]).astype(np.float32)
    return inp["x"]


def codes_of(blocks: np.ndarray):
    """What must not move: the int8 codes (the block sums are sums of them).  A block's f32 scale follows the row's scale in its last place: inside the bound."""
    b = blocks.view(tw.DT[Q8_K])
    return b["qs"].copy(), b["bsums"].copy()


def codes_stable(c: dict, inp: dict) -> bool:
    """The oracle's activation codes do not move when every value moves by one part in 2^23 either way."""
    for r in activation(c, inp):
        q = codes_of(oq.quantize(Q8_K, r))
        for f in (np.float32(1.0) - np.float32(2.0 ** -23), np.float32(1.0) + np.float32(2.0 ** -23)):
            q2 = codes_of(oq.quantize(Q8_K, (r * f).astype(np.float32)))
            if not all((a == b).all() for a, b in zip(q, q2)):
                return False
    return True


def mul(t: int, W: np.ndarray, N: int, K: int, y: np.ndarray) -> np.ndarray:
    if t == IQ4_XS:
        return iq4xs_ref.mul_mat(W, N, K, y)
    return oq.mul_mat(t, W, N, K, y, oq.threads(16))


def reference(c: dict, inp: dict):
    """-> list of f32 [T][N] per out buffer (one for SwiGLU)."""
    y = activation(c, inp)
    prods = [mul(t, inp["W"][s], N, c["K"], y) for s, (t, N) in enumerate(zip(c["types"], c["Ns"]))]
    if c["epi"] == SWIGLU:
        return [(oq.silu(prods[0]) * prods[1]).astype(np.float32)]
    if c["epi"] == ADD:
        return [(inp["resid"][:, :c["Ns"][0]] + prods[0]).astype(np.float32)]
    return prods


def bound(c: dict, ref: np.ndarray) -> float:
    return (4e-5 if c["epi"] == SWIGLU else 2e-5) * float(np.abs(ref).max()) + 1e-6


SPLIT_BOUND = 2e-6          # a K split against the unsplit launch, of max|ref| (+ 1e-6): tests/test_gpu_ops.py test_mul_mat_prefill_split_k

CASES = build_cases()
RUN_CASES = [c for c in CASES if not c["refused"]]
REFUSED_CASES = [c for c in CASES if c["refused"]]
BY_NAME = {c["name"]: c for c in CASES}


# ---------------------------------------------------------------- the producers of the activation and of its bh / bl planes (Backend.act_q8k_planes)
PRODUCER_T = (1, 7, 9, 31, 32, 40)
PRODUCER_N = (256, 1024, 4352, 5120, 5632, 8192, 8448)
CONST = 0.75
N_EDGE = 4
EDGE_SUMS = ((2032, 31, 48), (-2032, -32, 16), (0, 0, 0), (-2032, -32, 16))     # (block sum, bh, bl) of a block's sub-blocks 1..15, per edge row


def producer_inputs(producer: int, T: int, n: int):
    """(x, x2, norm_w, n_edge): T rows in all - random rows scaled per token, the last n_edge = min(4, T - 1) of them edge rows, in EDGE_SUMS' order.
    quantize_row_q8_K maps a block's largest magnitude to -127.  A block whose FIRST value is a little above +c and whose others are -c has codes -127, 127, 127 ..: block sums
    2032 from the second on, the highest there is (bh 31, bl 48).  A constant block has codes -127 whatever its sign: block sums -2032, the lowest (bh -32,
    bl 16).  And a row of zeros.  The norm (producer 1) multiplies by its weight, so its edge rows are these divided by the weight: equal again up to a
    rounding, which the codes do not see."""
    rng = np.random.default_rng(1000 * producer + 17 * T + n)
    x = (rng.standard_normal((T, n)) * rng.uniform(0.1, 4.0, (T, 1))).astype(np.float32)
    lead = np.full(n, -CONST, np.float32)
    lead[::256] = CONST * 1.002                                  # (the largest by a margin no rounding of the norm closes; the others still round to 127)
    n_edge = min(N_EDGE, T - 1)
    edges = np.stack([lead, np.full(n, CONST, np.float32), np.zeros(n, np.float32), np.full(n, -CONST, np.float32)])[:n_edge]
    if producer == 1:
        nw = rng.uniform(0.5, 1.5, n).astype(np.float32)
        x[T - n_edge:] = (edges / nw).astype(np.float32)
        return x, None, nw, n_edge
    x[T - n_edge:] = edges
    if producer == 2:
        # silu(g) * u against the oracle byte for byte wants the device's expf and the host's to agree to the last bit, which two libraries do not: from
        # g = 17.4 on exp(-g) < 2^-25, so 1 + exp(-g) = 1 and silu(g) = g in f32 whatever the expf - gate values in [18, 40), the rows are then g * u.
        # (General gate values: tests/test_gpu_prompt_mul_mat.py test_swiglu_quant_is_swiglu_then_quantise.)  Edge rows: g = 32, a constant times u.
        g = rng.uniform(18.0, 40.0, (T, n)).astype(np.float32)
        g[T - n_edge:] = 32.0
        return g, x, None, n_edge
    return x, None, None, n_edge


def producer_reference(producer: int, x, x2, nw) -> np.ndarray:
    """The f32 rows the producer quantises, from the oracle alone."""
    if producer == 1:
        return np.stack([(oq.rms_norm(r, EPS) * nw).astype(np.float32) for r in x])
    if producer == 2:
        return (oq.silu(x) * x2).astype(np.float32)
    return x
