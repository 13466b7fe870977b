"""TQ1_0 / TQ2_0 prompt batches on the kernel that reads the packed trits (csrc/mmq_ternary.hip): the op entries under set_option("mmq_ternary_direct", 1),
a dense ternary file end to end, and what the file costs in device memory - against the numpy restatement of tests/tq_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_tq as base
import tq_ref as tq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = base.TYPES
MODEL = ("tiny-d128", "q8_0", 40)        # E 1024, FF 2048, 2 layers: the smallest dense config of tests/test_gpu_tq.py with a 40-token case (its seed)
SLACK = 1 << 20


@pytest.fixture(scope="module")
def be(pkg):
    b = pkg.Backend()
    b.set_option("mmq_ternary_direct", 1)
    yield b
    b.set_option("mmq_ternary_direct", 0)
    b.set_option("mmq_ternary_tiles", 0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def close(y, ref, scale=None, k=2e-5):
    """The bar of tests/test_gpu_tq.py::_check_mul_mat."""
    return np.abs(y - ref).max() <= k * np.abs(ref if scale is None else scale).max() + 1e-6


def check_mul_mat(be, t, W, N, K, x, tiles=0):
    be.set_option("mmq_ternary_tiles", tiles)
    y, isum, msum = be.mul_mat(t, W, N, K, x, want_ints=True)
    rb = tq.row_bytes(t, K)
    for tt in range(0, x.shape[0], max(1, x.shape[0] // 5)):
        act = tq.quantize_act(x[tt])
        for r in range(0, N, max(1, N // 7)):
            assert (isum[tt, r] == tq.vec_dot_int_partials(t, W[r * rb:(r + 1) * rb], act, K)).all(), (tt, r)
    assert not msum.any()
    assert np.isfinite(y).all() and close(y, tq.mul_mat(t, W, N, K, x))
    assert np.array_equal(bits(y), bits(be.mul_mat(t, W, N, K, x)))               # the second call: the same bits
    return y


@pytest.mark.parametrize("N", [16, 96, 136])
@pytest.mark.parametrize("T", [32, 45, 200])
@pytest.mark.parametrize("K", [256, 768, 4096])
@pytest.mark.parametrize("t", TYPES)
def test_mul_mat_int_partials_value_and_fixed_order(be, pkg, t, K, T, N):
    """The kernel's own integer per (token, row, super-block) exact, the f32 result within the bar, bit-identical call to call.  The row tile is 128 with 32
    rows a wave: N = 16 is under one wave, 96 under one tile, 136 a tile and a ragged one.  T = 200 runs four token tiles a wave (128 + 72 tokens) and its
    first 45 rows must be the bits of a 45-token call, which runs one."""
    rng = np.random.default_rng(K + 7 * T + N + t)
    W, x = base.weights(pkg, rng, t, N * K), rng.standard_normal((T, K)).astype(np.float32)
    y = check_mul_mat(be, t, W, N, K, x, tiles=4 if T == 200 else 0)
    if T == 200:
        be.set_option("mmq_ternary_tiles", 0)
        assert np.array_equal(bits(y[:45]), bits(be.mul_mat(t, W, N, K, x[:45])))


@pytest.mark.parametrize("t", TYPES)
def test_mul_mat_arbitrary_bytes(be, t):
    """qs / qh from all 256 byte values (TQ2_0: code 3 is p = 2), finite d."""
    rng = np.random.default_rng(61 + t)
    N, K, T = 96, 768, 32
    blk = np.zeros(N * K // 256, tq.DT[t])
    blk["qs"] = rng.integers(0, 256, blk["qs"].shape, dtype=np.uint8)
    if t == tq.TQ1_0:
        blk["qh"] = rng.integers(0, 256, blk["qh"].shape, dtype=np.uint8)
    blk["d"] = rng.uniform(0.01, 0.03, blk.shape[0]).astype(np.float16)
    check_mul_mat(be, t, blk.view(np.uint8).reshape(-1), N, K, rng.standard_normal((T, K)).astype(np.float32))


@pytest.mark.parametrize("K", [256, 768])
@pytest.mark.parametrize("t", TYPES)
def test_residual_segments_and_swiglu_forms(be, pkg, t, K):
    """attn_output's residual, Q | K | V as one launch (the bits of three) and gate | up with SwiGLU (two products of the bar and the sigmoid's slope: the
    4e-5 of tests/test_gpu_tq.py), composed from tq_ref in float64."""
    rng = np.random.default_rng(5 * K + t)
    T, Ns = 45, [136, 40, 40]
    Ws = [base.weights(pkg, rng, t, n * K) for n in Ns]
    x = (rng.standard_normal((T, K)) * rng.uniform(0.1, 2.0, (T, 1))).astype(np.float32)
    be.set_option("mmq_ternary_tiles", 0)
    refs = [tq.mul_mat(t, w, n, K, x).astype(np.float64) for w, n in zip(Ws, Ns)]
    resid = rng.standard_normal((T, Ns[0])).astype(np.float32)
    assert close(be.mul_mat_add(t, Ws[0], Ns[0], K, x, resid), resid + refs[0], scale=refs[0])
    ys, path, _ = be.prompt_mul_mat([t] * 3, Ws, Ns, K, x)
    assert path["kernel"] == 6
    for y, w, n, ref in zip(ys, Ws, Ns, refs):
        assert close(y, ref) and np.array_equal(bits(y), bits(be.mul_mat(t, w, n, K, x)))
    g, u = refs[1], refs[2]
    assert close(be.ffn_gate_up(t, Ws[1], Ws[2], Ns[1], K, x), g / (1.0 + np.exp(-g)) * u, k=4e-5)


def vram_bound(m, ref):
    """Model.size + 2.25 B per weight of every 2-D tensor that is not ternary (the cap on a plane set or Q8_0-layout copy) + 1 MiB."""
    other = sum(ne[0] * ne[1] for ne, ty, _ in ref.t.values() if len(ne) > 1 and ne[1] > 1 and ty not in tq.TYPES)
    return m.size + int(2.25 * other) + SLACK


@pytest.mark.parametrize("t", TYPES)
def test_dense_ternary_file_prompt_steps_and_footprint(be, pkg, tmp_models, t):
    """A 40-token prompt and 3 greedy steps against the restatement with the tolerances of tests/test_gpu_tq.py, on a file that holds no plane set.
    tiny-d128 has 2 x 8,912,896 ternary weights: their planes alone (2 B a weight and more) were 35.7 MB on the parent against 3.25 MiB between Model.size and the bound
    (2.25 B x 1 M weights of token_embd and output, + 1 MiB), so the bound fails there."""
    path = base.make(pkg, tmp_models, MODEL[0], base.FTYPE[t], base.SEEDS[MODEL])
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=512, n_batch=512, n_ubatch=512, type_k=8, type_v=8)
    ref = tq.TqRef(path, 512, 8, 8)
    base._check_run(pkg, c, m, ref, MODEL[2], MODEL[1], tight=True, steps=3)
    ternary = sum(ne[0] * ne[1] for ne, ty, _ in ref.t.values() if ty in tq.TYPES)
    assert ternary == 2 * 8912896 and 2 * ternary > 10 * (vram_bound(m, ref) - m.size)
    assert m.planes_bytes == 0 and m.vram <= vram_bound(m, ref), (m.vram, m.size, vram_bound(m, ref))
    c.close(); m.close()


def test_plane_route_switch_in_a_fresh_process(pkg, tmp_models):
    """MI355_TQ_DIRECT=0: the same file loads with its plane sets, above the bound."""
    path = base.make(pkg, tmp_models, MODEL[0], "tq2_0", base.SEEDS[MODEL])
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import __graft_entry__ as ge; m = ge.load_pkg().Model(sys.argv[2]); print('vram', m.vram, m.size, m.planes_bytes)")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", code, ROOT, path], capture_output=True, text=True, env=dict(os.environ, MI355_TQ_DIRECT="0"))
    assert r.returncode == 0, r.stderr[-2000:]
    vram, size, planes = (int(v) for v in r.stdout.split("vram")[1].split()[:3])
    assert planes >= 2 * 2 * 8912896 and vram > size + int(2.25 * 2 * 512 * 1024) + SLACK, r.stdout
