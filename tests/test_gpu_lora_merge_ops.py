"""csrc/lora_merge.hip through mi355_lora_merge_rows against the float64 merge of tests/lora_merge_ref.py, at the shapes where the kernel can go wrong:
one row, ragged last tiles in N and K, a rank below one matrix-core step, one ragged against every step, and the largest.

The bound, per element: |got - ref64| <= u_out |ref64| + 2 r_total 2^-24 sum_i |s_i| (|B_i| @ |A_i|).  The first term is the final rounding (half an ulp of
the out type: 2^-11 relative for f16 and never below half its smallest subnormal step, 2^-24 relative for f32), the second the textbook bound of an f32 sum
of r_total terms, doubled for the base addition and the scale.  Nothing in it is measured; a kernel that rounds an F32 pair to f16 (2^-11 of the terms)
cannot meet it."""
import numpy as np
import pytest

import lora_merge_ref as mr

pytestmark = pytest.mark.gpu
NAMES = {mr.F32: "f32", mr.F16: "f16", mr.BF16: "bf16", mr.Q8_0: "q8_0", mr.Q4_K: "q4_K", mr.Q5_K: "q5_K", mr.Q6_K: "q6_K"}
FLOAT_BASES = (mr.F32, mr.F16, mr.BF16)
U_OUT = {mr.F16: (2.0 ** -11, 2.0 ** -25), mr.F32: (2.0 ** -24, 2.0 ** -150)}      # (relative half ulp, half the smallest subnormal step)


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def base_rows(gs, rng, t, N, K):
    raw = gs.random_blocks(rng, t, N * K, 0.05)
    return raw.view({mr.F32: "<f4", mr.F16: "<f2", mr.BF16: "<u2"}.get(t, np.uint8)).reshape(N, -1)


def adapter(rng, N, K, r, pair, scale):
    dt = np.float16 if pair == mr.F16 else np.float32
    return ((rng.standard_normal((r, K)) / np.sqrt(K)).astype(dt), (rng.standard_normal((N, r)) * 0.1).astype(dt), scale)


def check(got, ref64, bound, out_type, r_total, what):
    rel, floor = U_OUT[out_type]
    allowed = np.maximum(rel * np.abs(ref64), floor) + 2.0 * r_total * 2.0 ** -24 * bound
    err = np.abs(got.astype(np.float64) - ref64)
    worst = float((err / allowed).max())
    print(f"{what}: worst error / allowed = {worst:.3f}, max error {err.max():.3e}")
    assert worst <= 1.0, what


@pytest.mark.parametrize("pair", [mr.F16, mr.F32], ids=["pair-f16", "pair-f32"])
@pytest.mark.parametrize("base", mr.BASE_TYPES, ids=[NAMES[t] for t in mr.BASE_TYPES])
def test_merge_within_the_derived_bound(pkg, be, base, pair):
    gs = pkg.gguf_synth
    rng = np.random.default_rng([base, pair])
    for K in (256, 768) + ((96,) if base in FLOAT_BASES else ()):
        for N in (1, 33, 130):
            w = base_rows(gs, rng, base, N, K)
            for r in (1, 24, 512):
                ad = adapter(rng, N, K, r, pair, 0.37 * 16.0 / r)
                out_type = mr.F32 if (N + r) % 2 else mr.F16                  # both out types over the shapes of every (base, pair)
                _, ref64, bound = mr.merge_rows(base, w, [ad], out_type)
                got = be.lora_merge_rows(base, w, [ad], out_type)
                assert got.dtype == mr.OUT_DTYPE[out_type] and got.shape == (N, K)
                check(got, ref64, bound, out_type, r, f"{NAMES[base]} N={N} K={K} r={r} out={NAMES[out_type]}")


@pytest.mark.parametrize("base", [mr.F16, mr.Q4_K], ids=["f16", "q4_K"])
def test_two_adapters_in_one_call(pkg, be, base):
    rng = np.random.default_rng(7)
    N, K = 130, 768
    w = base_rows(pkg.gguf_synth, rng, base, N, K)
    ads = [adapter(rng, N, K, 24, mr.F16, 1.25), adapter(rng, N, K, 7, mr.F32, -0.6)]
    _, ref64, bound = mr.merge_rows(base, w, ads, mr.F16)
    got = be.lora_merge_rows(base, w, ads, mr.F16)
    check(got, ref64, bound, mr.F16, 31, f"{NAMES[base]} two adapters")
    assert be.lora_merge_rows(base, w, ads, mr.F16).tobytes() == got.tobytes()


@pytest.mark.parametrize("out_type", [mr.F16, mr.F32], ids=["out-f16", "out-f32"])
@pytest.mark.parametrize("base", mr.BASE_TYPES, ids=[NAMES[t] for t in mr.BASE_TYPES])
def test_scale_zero_is_the_rounded_base(pkg, be, base, out_type):
    rng = np.random.default_rng(11)
    N, K = 33, 256
    w = base_rows(pkg.gguf_synth, rng, base, N, K)
    got = be.lora_merge_rows(base, w, [adapter(rng, N, K, 24, mr.F16, 0.0)], out_type)
    assert got.tobytes() == mr.dequantize64(base, w).astype(mr.OUT_DTYPE[out_type]).tobytes()
    if base == mr.F16 and out_type == mr.F16:
        assert got.tobytes() == w.tobytes()


@pytest.mark.parametrize("base,K,r,pair,word", [(2, 256, 8, 1, "base type"), (1, 256, 0, 1, "rank"), (1, 256, 513, 1, "rank"), (12, 128, 8, 1, "n_per_row"),
                                                (1, 256, 8, 8, "pair type")], ids=["q4_0", "r0", "r513", "q4_K-128", "pair-8"])
def test_refusals(pkg, be, base, K, r, pair, word):
    w = np.zeros(4 * K, np.uint8)
    a, b, out = np.zeros((max(r, 1), K), np.float32), np.zeros((4, max(r, 1)), np.float32), np.full((4, K), 3.0, np.float32)
    rec = np.zeros(1, pkg.binding.LORA_MERGE_DTYPE)
    rec[0] = (a.ctypes.data, b.ctypes.data, r, pair, 1.0)
    rc = be.lib.mi355_lora_merge_rows(base, w.ctypes.data, 4, K, rec.ctypes.data, 1, 0, out.ctypes.data)
    assert rc == -103 and word in be.lib.mi355_last_error().decode()
    assert (out == 3.0).all()
