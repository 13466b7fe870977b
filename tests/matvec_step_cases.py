"""The decode step's mat-vec launches as op-level cases: the table, the inputs and the oracle reference (tests/test_matvec_step_cpu.py, tests/test_gpu_matvec_step.py).

A case is one launch as the model issues it (Backend.mat_vec_step): 1..3 weight tensors over one activation, an epilogue (store / add / SwiGLU), a prologue
(fuse 0: the quantiser's launch; 1: RMSNorm * w then quantise inside the launch; 2: quantise inside the launch), optionally the pinned host copy or the
selected-experts form.  `path` is what the launch must take, one entry per launch issued (T tokens go out as launches of 16 / 8 / 4 / 2 / 1): the kernel, and for
the weight stream its role, pass count kb = ceil(K / 2048) and the preloaded-argument forms (fast_ok, down_early).

The reference is the oracle alone, never a device intermediate: fuse 1 - oq.rms_norm(x, eps) * w rounded to f32; the activation quantised to the weight type's
vec_dot type; one vec_dot per row (oq.mul_mat is that loop; test_matvec_step_cpu checks it against oq.vec_dot); then resid + y or oq.silu(g) * u.  TQ1_0 / TQ2_0
are not in the oracle: their rows come from tests/tq_ref.py over the oracle's Q8_K blocks.

The tolerance is the project's re-association bound, 2e-5 * max|ref| + 1e-6 per segment (tests/test_gpu_ops.py).  One flipped activation code would move a
result by about 1e-3 of its scale, and the device's sum of squares may differ from the oracle's in the last place, so a fuse 1 case must not sit on a rounding
boundary: codes_stable() asserts that the oracle's codes are the same for y, y * (1 - 2^-23) and y * (1 + 2^-23); the seeds below are those for which it holds."""
from __future__ import annotations

import zlib

import numpy as np

import np_twin as tw
import oracle_py as oq
import tq_ref
from oracle_py import IQ4_NL, Q2_K, Q3_K, Q4_0, Q4_K, Q5_0, Q5_K, Q6_K, Q8_0, Q8_K

TQ1_0, TQ2_0 = tq_ref.TQ1_0, tq_ref.TQ2_0
STORE, ADD, SWIGLU = 0, 1, 2
EPS = 1e-5
BLOCK_BYTES = {Q4_0: 18, Q8_0: 34, Q4_K: 144, Q5_K: 176, Q6_K: 210, Q2_K: 84, Q3_K: 110, Q5_0: 22, IQ4_NL: 18, TQ1_0: 54, TQ2_0: 66}
Q80_TYPES = (Q8_0, Q4_0, Q5_0, IQ4_NL)
TYPE_NAME = {Q4_0: "q40", Q8_0: "q80", Q4_K: "q4k", Q5_K: "q5k", Q6_K: "q6k", Q2_K: "q2k", Q3_K: "q3k", Q5_0: "q50", IQ4_NL: "iq4nl", TQ1_0: "tq1", TQ2_0: "tq2"}


def kb_of(K: int) -> int:
    return (K + 2047) // 2048


def tokens_split(T: int):
    out = []
    while T:
        nt = 16 if T >= 16 else 8 if T >= 8 else 4 if T >= 4 else 2 if T >= 2 else 1
        out.append(nt)
        T -= nt
    return out


def stream(role, K, fast_ok=False, down_early=False):
    return {"T": 1, "kernel": "stream", "role": role, "kb": kb_of(K), "fast_ok": fast_ok, "down_early": down_early}


def other(kernel, T=1):
    return {"T": T, "kernel": kernel}


def case(name, types, Ns, K, path, T=1, epi=STORE, fuse=0, host=False, sel=None, n_expert=1, ld_pad=3, seed=0):
    return dict(name=name, types=tuple(types), Ns=tuple(Ns), K=K, T=T, epi=epi, fuse=fuse, host=host, sel=sel, n_expert=n_expert, ld_pad=ld_pad, seed=seed, path=path)


def build_cases():
    c = []
    # ---- Q | K | V: fuse 1, store, two and three tensors.  Rows: an odd last pair, fewer rows than the segment's workgroups, an uneven deal (773 = 193 * 4 + 1)
    c.append(case("qkv_k1024_q4k_q4k_q6k", (Q4_K, Q4_K, Q6_K), (96, 32, 32), 1024, [stream("qkv", 1024)], fuse=1))
    c.append(case("qkv_k2048_q5k_q80_q80", (Q5_K, Q8_0, Q8_0), (773, 37, 8), 2048, [stream("qkv", 2048)], fuse=1))
    c.append(case("qkv_k4096_q3k_q5k", (Q3_K, Q5_K), (300, 300), 4096, [stream("qkv", 4096)], fuse=1))
    c.append(case("qkv_k4096_q4k_q4k_q6k", (Q4_K, Q4_K, Q6_K), (773, 37, 8), 4096, [stream("qkv", 4096)], fuse=1))
    c.append(case("qkv_k5632_iq4nl", (IQ4_NL, IQ4_NL, IQ4_NL), (96, 32, 32), 5632, [stream("qkv", 5632)], fuse=1))
    c.append(case("qkv_k5632_q3k_q3k_q5k", (Q3_K, Q3_K, Q5_K), (773, 37, 8), 5632, [stream("qkv", 5632)], fuse=1))
    c.append(case("qkv_k8192_q4k_q4k_q6k", (Q4_K, Q4_K, Q6_K), (96, 32, 32), 8192, [stream("qkv", 8192)], fuse=1))
    c.append(case("qkv_k8192_q5k_q80", (Q5_K, Q8_0), (300, 300), 8192, [stream("qkv", 8192)], fuse=1))
    c.append(case("qkv_k2048_iq4nl", (IQ4_NL, IQ4_NL, IQ4_NL), (773, 37, 8), 2048, [stream("qkv", 2048)], fuse=1))
    # ---- gate | up: fuse 1, SwiGLU
    c.append(case("gate_up_k2048_q4k", (Q4_K, Q4_K), (261, 261), 2048, [stream("gate_up", 2048, fast_ok=True)], epi=SWIGLU, fuse=1))
    c.append(case("gate_up_k4096_q6k", (Q6_K, Q6_K), (1000, 1000), 4096, [stream("gate_up", 4096, fast_ok=True)], epi=SWIGLU, fuse=1))
    c.append(case("gate_up_k8192_q2k", (Q2_K, Q2_K), (261, 261), 8192, [stream("gate_up", 8192, fast_ok=True)], epi=SWIGLU, fuse=1))
    c.append(case("gate_up_k2048_q40", (Q4_0, Q4_0), (1000, 1000), 2048, [stream("gate_up", 2048, fast_ok=True)], epi=SWIGLU, fuse=1))
    c.append(case("gate_up_k5632_q4k", (Q4_K, Q4_K), (261, 261), 5632, [stream("gate_up", 5632, fast_ok=True)], epi=SWIGLU, fuse=1))
    c.append(case("gate_up_k4096_q2k", (Q2_K, Q2_K), (1000, 1000), 4096, [stream("gate_up", 4096, fast_ok=True)], epi=SWIGLU, fuse=1))
    # ---- ffn_down: fuse 2, add, one tensor.  kb 1, 2, 3, 4, 6, 7, 7, 10; Q4_K at K = 14336 has 8064-byte rows (single rows), Q2_K 4704-byte rows (row pairs)
    for K, N, t in ((2048, 300, Q4_K), (4096, 37, Q6_K), (5632, 300, Q5_K), (8192, 37, Q4_K), (11008, 300, Q4_K), (13824, 37, Q4_K), (14336, 300, Q4_K), (14336, 37, Q2_K),
                    (18944, 300, Q4_K), (18944, 37, Q3_K)):
        c.append(case(f"ffn_down_k{K}_n{N}_{TYPE_NAME[t]}", (t,), (N,), K, [stream("ffn_down", K, down_early=kb_of(K) in (6, 7))], epi=ADD, fuse=2))
    # the residual of a workgroup that owns more than 64 rows: 64 * 256 + 300 rows over 256 workgroups
    c.append(case("ffn_down_k1024_n16684_q4k", (Q4_K,), (64 * 256 + 300,), 1024, [stream("ffn_down", 1024)], epi=ADD, fuse=2))
    # ---- the head: fuse 1, store, one long tensor, with and without the pinned host copy (which takes the plain kernel: the packed geometry has no second copy)
    c.append(case("head_k2048_q6k", (Q6_K,), (16411,), 2048, [stream("head", 2048, fast_ok=True)], fuse=1))
    c.append(case("head_k2048_q6k_host", (Q6_K,), (16411,), 2048, [stream("head", 2048)], fuse=1, host=True, ld_pad=0))
    c.append(case("head_k4096_q4k", (Q4_K,), (16411,), 4096, [stream("head", 4096, fast_ok=True)], fuse=1))
    c.append(case("head_k4096_q4k_host", (Q4_K,), (16411,), 4096, [stream("head", 4096)], fuse=1, host=True, ld_pad=0))
    c.append(case("head_k5632_q2k", (Q2_K,), (16411,), 5632, [stream("head", 5632, fast_ok=True)], fuse=1))
    c.append(case("head_k8192_q2k_host", (Q2_K,), (16411,), 8192, [stream("head", 8192)], fuse=1, host=True, ld_pad=0))
    c.append(case("head_k8192_q2k", (Q2_K,), (16411,), 8192, [stream("head", 8192, fast_ok=True)], fuse=1))
    c.append(case("head_k5632_q2k_host", (Q2_K,), (16411,), 5632, [stream("head", 5632)], fuse=1, host=True, ld_pad=0))
    # ---- launches with no role: one short tensor behind the norm; a stored ffn_down; ready-made planes (fuse 0) with every epilogue
    for K in (2048, 4096, 5632, 8192):
        c.append(case(f"any_fuse1_k{K}", (Q4_K,), (37,), K, [stream("stream", K)], fuse=1))
    for K in (2048, 4096, 5632, 8192, 11008, 14336, 18944):
        c.append(case(f"any_fuse2_store_k{K}", (Q5_K,), (37,), K, [stream("stream", K)], fuse=2))
        c.append(case(f"any_fuse0_k{K}", (Q4_K,), (300,), K, [stream("stream", K)], epi=ADD if kb_of(K) % 2 else STORE, fuse=0))
    c.append(case("any_fuse0_qkv_k4096", (Q4_K, Q4_K, Q6_K), (96, 32, 32), 4096, [stream("stream", 4096)], fuse=0))
    # ---- no stream form: rows under 512 bytes, a pass count the stream is not built for (K = 10240: 5), Q8_0 tensors only, 32-element rows of K = 2080 and
    # K = 16384 (8 passes: neither the stream nor the ring), which take the generic kernel
    c.append(case("ring_k1024_q2k_row336", (Q2_K,), (300,), 1024, [other("ring")], epi=ADD, fuse=2))
    c.append(case("ring_k1024_q3k_qkv", (Q3_K, Q3_K, Q5_K), (96, 32, 32), 1024, [other("ring")], fuse=1))
    c.append(case("ring_k10240_q4k", (Q4_K,), (37,), 10240, [other("ring")], epi=ADD, fuse=2))
    c.append(case("ring_k10240_gate_up_fuse0", (Q4_K, Q4_K), (261, 261), 10240, [other("ring")], epi=SWIGLU, fuse=0))
    c.append(case("ring_gate_up_fuse0_k2048", (Q6_K, Q6_K), (261, 261), 2048, [other("ring")], epi=SWIGLU, fuse=0))
    c.append(case("ring_q80_small_k2048", (Q8_0, Q8_0), (300, 37), 2048, [other("ring")], fuse=1))
    c.append(case("ring_q80_fuse0_k4096", (Q8_0,), (300,), 4096, [other("ring")], epi=ADD, fuse=0))
    c.append(case("base_k2080_q40_fuse1", (Q4_0,), (300,), 2080, [other("base")], fuse=1))
    c.append(case("base_k2080_q80_fuse2_add", (Q8_0,), (37,), 2080, [other("base")], epi=ADD, fuse=2))
    c.append(case("base_k2080_iq4nl_gate_up", (IQ4_NL, IQ4_NL), (261, 261), 2080, [other("base")], epi=SWIGLU, fuse=1))
    c.append(case("base_k16384_q4k", (Q4_K,), (37,), 16384, [other("base")], fuse=0))
    # 3584 and 6656 (Qwen2-7B's and Llama-30B's hidden sizes): 14 and 26 whole super-blocks, so the last pass is partial; mmvq_stream_applicable asks for
    # K % 256 == 0 only and the stream takes them ("ffn_down K = 3584 = 14 super-blocks")
    c.append(case("k3584_qkv", (Q4_K, Q4_K, Q6_K), (96, 32, 32), 3584, [stream("qkv", 3584)], fuse=1))
    c.append(case("k6656_ffn_down", (Q4_K,), (300,), 6656, [stream("ffn_down", 6656)], epi=ADD, fuse=2))
    c.append(case("k3584_gate_up", (Q5_K, Q5_K), (261, 261), 3584, [stream("gate_up", 3584, fast_ok=True)], epi=SWIGLU, fuse=1))
    # ---- several tokens (fuse 0): launches of 16 / 8 / 4 / 2 / 1.  16 and 8 take the tiled kernel, 4 and 2 the generic one, the last token a single-token kernel
    for T in (2, 3, 5, 9, 17):
        def chunks(single, T=T):
            return [other("tiled" if nt >= 8 else "base", nt) if nt > 1 else single for nt in tokens_split(T)]
        # (a Q8_0 tensor in the launch, or SwiGLU over ready-made planes: the last token's launch has no stream form and takes the register ring)
        c.append(case(f"tok{T}_qkv_mixed", (Q4_K, Q8_0, Q6_K), (96, 37, 8), 2048, chunks(other("ring")), T=T, fuse=0))
        c.append(case(f"tok{T}_gate_up", (Q4_K, Q4_K), (261, 261), 2048, chunks(other("ring")), T=T, epi=SWIGLU, fuse=0))
        c.append(case(f"tok{T}_add_k2048", (Q5_K,), (300,), 2048, chunks(stream("stream", 2048)), T=T, epi=ADD, fuse=0))
        c.append(case(f"tok{T}_add_k5632", (Q6_K,), (37,), 5632, chunks(stream("stream", 5632)), T=T, epi=ADD, fuse=0))
    # ---- the selected experts of one token (Context::moe_selected_desc): gate | up behind the norm, down quantising one row per expert; repeated and out-of-order ids
    ids2, ids8 = (11, 3), (5, 0, 15, 5, 9, 2, 15, 1)
    for K, t, ids in ((2048, Q4_K, ids2), (4096, Q5_K, ids8), (2048, Q5_K, ids8)):
        c.append(case(f"moe_gate_up_k{K}_{TYPE_NAME[t]}_sel{len(ids)}", (t, t), (261, 261), K, [stream("moe", K)], epi=SWIGLU, fuse=1, sel=ids, n_expert=16))
    for K, t, ids in ((4096, Q4_K, ids8), (8192, Q5_K, ids2), (14336, Q4_K, ids8), (8192, Q4_K, ids8)):
        c.append(case(f"moe_down_k{K}_{TYPE_NAME[t]}_sel{len(ids)}", (t,), (37 if K > 8192 else 300,), K, [stream("moe", K)], fuse=2, sel=ids, n_expert=16))
    # ---- ternary
    c.append(case("tq_qkv_k4096", (TQ1_0, TQ2_0, TQ2_0), (773, 37, 8), 4096, [stream("ternary", 4096)], fuse=1))
    c.append(case("tq_gate_up_k4096", (TQ2_0, TQ2_0), (261, 261), 4096, [stream("ternary", 4096)], epi=SWIGLU, fuse=1))
    c.append(case("tq_ffn_down_k14336", (TQ1_0,), (300,), 14336, [stream("ternary", 14336)], epi=ADD, fuse=2))
    names = [x["name"] for x in c]
    assert len(set(names)) == len(names)
    for i, x in enumerate(c):
        x["seed"] = SEEDS.get(x["name"], zlib.crc32(x["name"].encode()) % 100000)
    return c


# seeds changed from the default (a checksum of the name) because codes_stable() failed with it: name -> seed
SEEDS: dict = {}

# the subset a fresh child process computes under each start-up switch (tests/test_gpu_matvec_step.py), and the path a case takes there where it differs
SWITCH_CASES = {
    "MI355_STREAM_FAST_START": ("gate_up_k2048_q4k", "gate_up_k4096_q6k", "gate_up_k5632_q4k", "gate_up_k8192_q2k", "head_k2048_q6k", "head_k4096_q4k", "head_k5632_q2k", "head_k8192_q2k"),
    "MI355_STREAM_DOWN_EARLY": ("ffn_down_k13824_n37_q4k", "ffn_down_k14336_n300_q4k", "ffn_down_k14336_n37_q2k", "ffn_down_k11008_n300_q4k"),
    "MI355_MMVQ_FAST": ("qkv_k4096_q4k_q4k_q6k", "qkv_k2048_q5k_q80_q80", "gate_up_k2048_q4k", "ffn_down_k5632_n300_q5k", "any_fuse0_k4096", "base_k2080_q40_fuse1"),
}


def switch_path(var: str, c: dict):
    if var == "MI355_MMVQ_FAST":
        return [other("base", p["T"]) for p in c["path"]]
    return [dict(p, fast_ok=False, down_early=False) if p["kernel"] == "stream" else p for p in c["path"]]


def rand_weights(rng, t: int, n_elems: int, dscale: float = 1e-2) -> np.ndarray:
    """Random blocks with sane scales (tests/test_gpu_ops.py rand_weights, and the ternary formats: every byte value is a valid code)."""
    be_ = 32 if t in Q80_TYPES else 256
    raw = rng.integers(0, 256, n_elems // be_ * BLOCK_BYTES[t], dtype=np.uint8)
    blk = raw.view(tq_ref.DT[t] if t in tq_ref.TYPES else tw.DT[t])
    blk["d"] = (rng.uniform(0.5, 1.5, blk.size) * dscale).astype("<f2")
    if t in (Q4_K, Q5_K, Q2_K):
        blk["dmin"] = (rng.uniform(0.5, 1.5, blk.size) * dscale).astype("<f2")
    return raw


def inputs(c: dict) -> dict:
    """The case's tensors, from its seed: W[s] (raw ggml rows; n_expert tensors back to back), x, norm_w, resid (whole padded rows)."""
    rng = np.random.default_rng(c["seed"])
    K, ne = c["K"], c["n_expert"]
    Ws = [rand_weights(rng, t, ne * N * K) for t, N in zip(c["types"], c["Ns"])]
    n_sel = len(c["sel"]) if c["sel"] else 0
    xr = n_sel if (n_sel and c["fuse"] == 2) else c["T"]
    x = (rng.standard_normal((xr, K)) * rng.uniform(0.3, 3.0, (xr, 1))).astype(np.float32)
    nw = rng.uniform(0.5, 1.5, K).astype(np.float32) if c["fuse"] == 1 else None
    R = n_sel if n_sel else c["T"]
    resid = rng.standard_normal((R, c["Ns"][0] + c["ld_pad"])).astype(np.float32) if c["epi"] == ADD else None
    return dict(W=Ws, x=x, nw=nw, resid=resid)


def normed(c: dict, inp: dict) -> np.ndarray:
    """The f32 rows the launch quantises: fuse 1 - oq.rms_norm(x, eps) * w rounded to f32, else x."""
    if c["fuse"] != 1:
        return inp["x"]
    return np.stack([(oq.rms_norm(r, EPS) * inp["nw"]).astype(np.float32) for r in inp["x"]])


def act_type(t: int) -> int:
    return Q8_K if t in tq_ref.TYPES else oq.vec_dot_type(t)


def codes_of(at: int, blocks: np.ndarray):
    """What must not move: the int8 codes (the Q8_K block sums are sums of them), and for Q8_0 the f16 block scales as well - one step of an f16 scale is
    5e-4 of its block.  A Q8_K block's f32 scale follows the row's scale in its last place, which is inside the bound."""
    b = blocks.view(tw.DT[at])
    return (b["qs"].copy(), b["bsums"].copy()) if at == Q8_K else (b["qs"].copy(), b["d"].copy())


def codes_stable(c: dict, inp: dict) -> bool:
    """The oracle's activation codes do not move when every value moves by one part in 2^23 either way (every activation format the case's tensors take)."""
    y = normed(c, inp)
    for at in sorted({act_type(t) for t in c["types"]}):
        for r in y:
            q = codes_of(at, oq.quantize(at, r))
            for f in (np.float32(1.0) - np.float32(2.0 ** -23), np.float32(1.0) + np.float32(2.0 ** -23)):
                q2 = codes_of(at, oq.quantize(at, (r * f).astype(np.float32)))
                if not all((a == b).all() for a, b in zip(q, q2)):
                    return False
    return True


def _mul(t: int, W: np.ndarray, N: int, K: int, y: np.ndarray) -> np.ndarray:
    if t in tq_ref.TYPES:
        return tq_ref.mul_mat(t, W, N, K, y)
    return oq.mul_mat(t, W, N, K, y, oq.threads(16))


def reference(c: dict, inp: dict):
    """-> list of f32 [rows][N] per out buffer (one for SwiGLU); rows = tokens, or the selected experts in launch order."""
    y = normed(c, inp)
    K = c["K"]
    prods = []
    for s, (t, N) in enumerate(zip(c["types"], c["Ns"])):
        W = inp["W"][s]
        if c["sel"]:
            rb = len(W) // (c["n_expert"] * N)
            rows = []
            for j, e in enumerate(c["sel"]):
                We = W[e * N * rb:(e + 1) * N * rb]
                rows.append(_mul(t, We, N, K, y[j if c["fuse"] == 2 else 0][None, :])[0])
            prods.append(np.stack(rows))
        else:
            prods.append(_mul(t, W, N, K, y))
    if c["epi"] == SWIGLU:
        return [(oq.silu(prods[0]) * prods[1]).astype(np.float32)]
    if c["epi"] == ADD:
        return [(inp["resid"][:, :c["Ns"][0]] + prods[0]).astype(np.float32)]
    return prods


def bound(ref: np.ndarray) -> float:
    return 2e-5 * float(np.abs(ref).max()) + 1e-6


CASES = build_cases()
BY_NAME = {c["name"]: c for c in CASES}
