"""BF16 (ggml type 30) without a GPU: the numpy restatement (tests/bf16_ref.py) on known answers and against the CPU oracle where the oracle can speak,
the synthetic writer's bf16 ftype, the reference model on a bf16 file, and the library's op hooks on a machine without a device."""
import hashlib

import numpy as np
import pytest

import bf16_ref as bf
import oracle_py as oq
from gguf_read import read_gguf
from qwen3_ref import Qwen3Ref


def _f(bits):
    return np.array(bits, np.uint32).view(np.float32)


def test_rounding_known_answers():
    r = lambda u: int(bf.round_bf16(_f([u]))[0])
    assert r(0x3F808000) == 0x3F80          # a tie: down to the even mantissa
    assert r(0x3F818000) == 0x3F82          # a tie: up to the even mantissa
    assert r(0x3F808001) == 0x3F81 and r(0x3F807FFF) == 0x3F80
    assert r(0x7F7FFFFF) == 0x7F80          # the largest finite f32 rounds to infinity
    assert r(0x7F800000) == 0x7F80 and r(0xFF800000) == 0xFF80
    for nan in (0x7F800001, 0x7FC00000, 0xFFFFFFFF, 0x7F80FFFF):
        b = r(nan)
        assert (b & 0x7F80) == 0x7F80 and (b & 0x0040) and (b & 0x007F), hex(b)      # still a NaN, quiet bit set
        assert (b & 0x8000) == ((nan >> 16) & 0x8000)
    assert r(0x00000000) == 0x0000 and r(0x80000000) == 0x8000                         # +-0
    assert r(0x00400000) == 0x0040 and r(0x80012345) == 0x8001                         # f32 subnormals keep their upper bits (not flushed)
    assert r(0x00008000) == 0x0000 and r(0x00018000) == 0x0002                         # ... and round like everything else


def test_rounding_is_nearest_even_on_random_values():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(200000) * np.exp(rng.uniform(-30, 30, 200000))).astype(np.float32)
    b = bf.round_bf16(x)
    y = bf.widen(b).astype(np.float64)
    lo = bf.widen((x.view(np.uint32) >> 16).astype(np.uint16)).astype(np.float64)      # truncation: the neighbour towards zero
    hi = bf.widen(((x.view(np.uint32) >> 16) + 1).astype(np.uint16)).astype(np.float64)
    xd = x.astype(np.float64)
    assert (np.abs(y - xd) <= np.minimum(np.abs(lo - xd), np.abs(hi - xd))).all()
    tie = np.abs(lo - xd) == np.abs(hi - xd)
    assert ((b[tie] & 1) == 0).all()


def test_widening_is_exact_for_all_patterns():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    w = bf.widen(bits)
    assert (w.view(np.uint32) == (bits.astype(np.uint32) << 16)).all()
    finite = np.isfinite(w)
    assert (bf.round_bf16(w[finite]) == bits[finite]).all()                            # a bf16 value rounds to itself
    nan = np.isnan(w)
    assert (bf.round_bf16(w[nan]) == (bits[nan] | 64)).all()


@pytest.mark.parametrize("N,K,T", [(64, 256, 1), (48, 4096, 5), (33, 3584, 3), (16, 14336, 2)])
def test_restatement_against_the_oracle_f32_mul_mat(N, K, T):
    """The oracle has no BF16 but it has F32 tensors: on widen(W) and widen(round_bf16(x)) its F32 mul_mat sums the same exact products (in f32, in its own
    order), so the two agree within the project's bar for float re-association, 2e-5 of the output scale."""
    rng = np.random.default_rng(N + K + T)
    W = bf.round_bf16((rng.standard_normal((N, K)) * 0.05).astype(np.float32))
    x = (rng.standard_normal((T, K)) * rng.uniform(0.1, 3.0, (T, 1))).astype(np.float32)
    got = bf.mul_mat(W, N, K, x)
    xb = bf.widen(bf.round_bf16(x))
    ref = oq.mul_mat(oq.F32, bf.widen(W).view(np.uint8).reshape(-1), N, K, xb, oq.threads())
    assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max()
    # ... and the f64 sum is what the docstring says: one output summed in element order
    w0 = bf.widen(W[0]).astype(np.float64)
    acc = 0.0
    for wk, xk in zip(w0, xb[0].astype(np.float64)):
        acc += wk * xk
    assert abs(float(got[0, 0]) - acc) <= 2.0 ** -23 * max(abs(acc), 1e-30) + 1e-12 * float(np.abs(w0).sum())


def test_get_rows_is_the_exact_widening():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16).reshape(-1, 256)
    got = bf.get_rows(bits, 256, [0, 255, 127, 128])
    assert (got.view(np.uint32) == (bits[[0, 255, 127, 128]].astype(np.uint32) << 16)).all()


# ------------------------------------------------------------------------------------------------ the writer
def test_writer_ids_and_sizes(pkg):
    gs = pkg.gguf_synth
    assert gs.BF16 == 30 and gs.FTYPE_ID["bf16"] == 32 and gs.TYPE_NAME[gs.BF16] == "bf16"
    assert gs.row_bytes(gs.BF16, 4096) == 8192 and gs.row_bytes(gs.BF16, 8) == 16
    assert pkg.binding.BF16 == 30


@pytest.mark.parametrize("cfg", ["tiny", "tiny-qwen2", "tiny-qwen3", "tiny-8b-2l", "llama-3-8b"])
def test_writer_every_2d_weight_is_bf16(pkg, cfg):
    gs = pkg.gguf_synth
    for name, ne, t, _ in gs.model_tensors(gs.CONFIGS[cfg], "bf16"):
        if len(ne) == 1:
            assert t == gs.F32, name
        else:
            assert t == gs.BF16, name


@pytest.mark.parametrize("cfg", ["tiny", "tiny-qwen2", "tiny-qwen3"])
def test_writer_file_is_the_f16_files_draws_rounded_to_bf16(pkg, tmp_path, cfg):
    """A bf16 file parses, and every BF16 tensor is round_bf16 of the f32 draws that the f16 file of the same seed rounds to half: wherever the half is a
    normal number, widen(bf16) and the half are two roundings of one value (8 and 11 significant bits)."""
    gs = pkg.gguf_synth
    pb, ph = str(tmp_path / "b.gguf"), str(tmp_path / "h.gguf")
    gs.write_synthetic_llama(pb, cfg, "bf16", seed=7)
    gs.write_synthetic_llama(ph, cfg, "f16", seed=7)
    kv, tb = read_gguf(pb)
    _, th = read_gguf(ph)
    assert kv["general.file_type"] == 32
    want = {n: (ne, ty) for n, ne, ty, _ in gs.model_tensors(gs.CONFIGS[cfg], "bf16")}
    assert set(tb) == set(want) == set(th)
    n_bf = 0
    for n, (ne, ty, raw) in tb.items():
        assert (ne, ty) == want[n], n
        cnt = int(np.prod(ne))
        if ty != gs.BF16:
            assert raw[:4 * cnt].tobytes() == th[n][2][:4 * cnt].tobytes(), n          # the f32 vectors are the same draws
            continue
        n_bf += 1
        assert raw.size >= 2 * cnt
        b = bf.widen(bf.bits_of(raw, cnt)).astype(np.float64)
        h = th[n][2][:2 * cnt].view("<f2").astype(np.float64)
        ok = np.abs(h) >= 6.2e-5                                                        # normal halves
        assert np.abs(b[ok] - h[ok]).max() <= (2.0 ** -8 + 2.0 ** -11) * np.abs(h[ok]).max()
        assert (np.abs(b[ok] - h[ok]) <= (2.0 ** -8 + 2.0 ** -11) * np.abs(h[ok])).all(), n
    assert n_bf >= 8
    # the draws themselves: the writer's generator replayed for the first tensor
    rng_raw = gs.random_blocks(np.random.default_rng(0), gs.BF16, 4096, 0.02)
    draws = np.random.default_rng(0).standard_normal(4096, dtype=np.float32) * np.float32(0.02)
    assert (rng_raw.view("<u2") == bf.round_bf16(draws)).all() and (gs.round_bf16(draws) == bf.round_bf16(draws)).all()
    assert (gs.random_blocks(np.random.default_rng(0), gs.F16, 4096, 0.02).view("<f2") == draws.astype("<f2")).all()


def test_existing_ftypes_write_what_they_wrote(pkg, tmp_path):
    """(every pinned digest is checked by tests/test_qwen3_cpu.py; this is the same pin for one f16 and one q4_k_m file, read from that table)"""
    import test_qwen3_cpu as tq
    for (cfg, ftype), want in sorted(tq.DIGESTS.items())[:2]:
        path = str(tmp_path / f"{cfg}-{ftype}.gguf")
        pkg.gguf_synth.write_synthetic_llama(path, cfg, ftype, seed=3)
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == want


# ------------------------------------------------------------------------------------------------ the reference model
def test_reference_model_is_its_parent_without_bf16(pkg, tmp_path):
    path = str(tmp_path / "m.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny-qwen3", "q4_k_m", seed=11)
    a, b = Qwen3Ref(path, 64, oq.Q8_0, oq.Q8_0), bf.Bf16Ref(path, 64, oq.Q8_0, oq.Q8_0)
    la, lb = a.decode([1, 17, 42, 5], np.arange(4)), b.decode([1, 17, 42, 5], np.arange(4))
    assert la.tobytes() == lb.tobytes()


@pytest.mark.parametrize("cfg", ["tiny", "tiny-qwen2", "tiny-qwen3"])
def test_reference_model_runs_on_bf16_file(pkg, tmp_path, cfg):
    gs = pkg.gguf_synth
    path = str(tmp_path / "m.gguf")
    gs.write_synthetic_llama(path, cfg, "bf16", seed=2)
    r = bf.Bf16Ref(path, 32, oq.Q8_0, oq.Q8_0)
    ne, ty, raw = r._embd_bf16
    E = ne[0]
    assert (r.t["token_embd.weight"][2].view("<f4")[7 * E:8 * E].view(np.uint32) == (bf.bits_of(raw, ne[0] * ne[1])[7 * E:8 * E].astype(np.uint32) << 16)).all()
    lg = r.decode([1, 7, 3], np.arange(3))
    assert lg.shape == (1, ne[1]) and np.isfinite(lg).all() and float(np.abs(lg).max()) > 0


# ------------------------------------------------------------------------------------------------ the library without a device
def test_op_hooks_accept_type_30_and_need_a_device(pkg):
    """Without a GPU every entry point that computes returns MI355_ERR_NO_DEVICE (-100) - the new bf16 hooks and the widened ones with type 30 - and
    never an argument error for the type."""
    import ctypes as C
    lib = pkg.load_library()
    if lib.mi355_device_count() > 0:
        pytest.skip("GPU present")
    N, K, T = 32, 256, 2
    W = np.zeros((N, K), np.uint16)
    x = np.zeros((T, K), np.float32)
    y = np.zeros((T, N), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.mi355_op_mul_mat(30, p(W), N, K, p(x), T, p(y), None, None) == -100
    ids = np.zeros(2, np.int32)
    out = np.zeros((2, K), np.float32)
    assert lib.mi355_op_get_rows(30, p(W), K, N, p(ids), 2, p(out)) == -100
    b = np.zeros(T * K, np.uint16)
    assert lib.mi355_op_f32_to_bf16(p(x), T * K, p(b)) == -100
    wp, yp = (C.c_void_p * 1)(W.ctypes.data), (C.c_void_p * 1)(y.ctypes.data)
    Ns = np.array([N], np.int64)
    assert lib.mi355_op_mul_mat_bf16(1, wp, p(Ns), K, p(x), T, None, None, 0, 0, 0, 0, yp) == -100
    with pytest.raises(pkg.MI355Error):
        pkg.Backend()
