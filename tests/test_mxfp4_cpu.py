"""MXFP4 on the CPU side: the numpy restatement of tests/mxfp4_ref.py on hand-written blocks, the writer's reference quantiser, the block-order dot against a
float64 dot, what the synthetic writer's mxfp4 / mxfp4_moe files hold, and the written file through the host's own GGUF reader."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import mxfp4_ref as xr
import oracle_py as oq
from gguf_read import read_gguf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MXFP4 = xr.MXFP4
LEVELS = [0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12]


def _block(e, idx):
    """One block from its level indices idx[32] (element order), built byte by byte from the layout in the format's definition: e | qs[16]."""
    raw = np.zeros(17, np.uint8)
    raw[0] = e
    for j in range(16):
        raw[1 + j] = (int(idx[j]) & 15) | ((int(idx[j + 16]) & 15) << 4)
    return raw


def test_ids_and_block_size(pkg):
    gs = pkg.gguf_synth
    assert gs.MXFP4 == MXFP4 == pkg.binding.MXFP4 == 39
    assert gs.BLOCK_BYTES[MXFP4] == xr.BLOCK_BYTES == gs.BLOCK_DTYPE[MXFP4].itemsize == 17 and gs.BLOCK_ELEMS[MXFP4] == 32
    assert gs.TYPE_NAME[MXFP4] == "mxfp4" and gs.FTYPE_ID["mxfp4_moe"] == gs.FTYPE_ID["mxfp4"] == xr.FTYPE_MXFP4_MOE == 38
    assert gs.KVALUES_MXFP4.tolist() == LEVELS == xr.KVALUES.tolist()
    assert gs.row_bytes(MXFP4, 4096) == xr.row_bytes(4096) == 128 * 17


@pytest.mark.parametrize("e,d", [(0, 2.0 ** -128), (1, 2.0 ** -127), (2, 2.0 ** -126), (127, 0.5), (254, 2.0 ** 126), (255, 2.0 ** 127)])
def test_dequantize_hand_written_blocks(pkg, e, d):
    """Every level index in both nibble positions, at the ends and the middle of the scale range: y = level * (half of 2^(e - 127)), e = 255 included (no NaN).
    A product that f32 holds is exact (a level has two significant bits; the smallest scale, 2^-128, is a subnormal f32); from 4 * 2^126 on it is the
    infinity of its sign, as one f32 multiply gives - never a NaN."""
    idx = np.r_[np.arange(16), np.arange(16)[::-1]]
    raw = _block(e, idx)
    assert (xr.make_blocks([e], idx) == raw).all()
    dd, lv = xr.decode(raw, 32)
    assert dd.dtype == np.float32 and float(dd[0]) == d and lv[0].tolist() == [LEVELS[i] for i in idx]
    assert float(pkg.gguf_synth.mxfp4_scale(np.array([e]))[0]) == d
    y = xr.dequantize(raw, 32)
    assert y.dtype == np.float32 and not np.isnan(y).any() and (np.isfinite(y).all() or e >= 254)
    with np.errstate(over="ignore"):
        want = np.array([LEVELS[i] * d for i in idx], np.float64).astype(np.float32)
    assert y.view(np.uint32).tolist() == want.view(np.uint32).tolist() or (y == want).all()           # (+0 and -0 levels both give a zero)


def test_scale_is_exact_for_every_e(pkg):
    e = np.arange(256)
    want = np.ldexp(1.0, e - 128)
    assert (xr.scale(e).astype(np.float64) == want).all() and (pkg.gguf_synth.mxfp4_scale(e).astype(np.float64) == want).all()


def test_quantiser_nearest_level_ties_to_the_lower_index(pkg):
    gs = pkg.gguf_synth
    # amax 12 -> floor(log2 12) = 3 -> e = 128, d = 1: the levels are the integers themselves
    x = np.zeros(32, np.float32)
    x[:20] = [12, -12, 0.4, 0.5, 0.6, 1.5, 2.5, 3.5, 5, 7, 10, -0.5, -1.5, -5, -7, -10, 11.9, -0.4, 6.9, 7.1]
    b = gs.quantize_mxfp4(x).view(gs.DT_MXFP4)
    assert b["e"][0] == 128
    lv = xr.decode(b.view(np.uint8), 32)[1][0]
    # ties (0.5, 1.5, 2.5, 3.5, 5, 7, 10 and their negatives) go to the level with the lower index: the one nearer zero
    assert lv[:20].tolist() == [12, -12, 0, 0, 1, 1, 2, 3, 4, 6, 8, 0, -1, -4, -6, -8, 12, 0, 6, 8]
    idx = np.r_[b["qs"][0] & 15, b["qs"][0] >> 4]
    assert idx[3] == 0 and idx[11] == 0 and idx[2] == 0 and idx[17] == 0          # +-0.5, +-0.4: index 0 (the +0), never index 8 (the -0)
    # a random row: every weight takes a level no other level is strictly nearer to, and the first such index
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(32 * 64) * rng.uniform(1e-3, 50.0, 32 * 64)).astype(np.float32)
    raw = gs.quantize_mxfp4(x)
    d, lv = xr.decode(raw, x.size)
    b = raw.view(gs.DT_MXFP4)
    idx = np.concatenate([b["qs"] & 15, b["qs"] >> 4], axis=1)
    amax = np.abs(x.reshape(-1, 32)).max(axis=1)
    assert (b["e"] == (np.floor(np.log2(amax)) - 2 + 127).astype(np.int64)).all()
    cand = (np.array(LEVELS, np.float32)[None, None, :] * d[:, None, None]).astype(np.float32)
    err = np.abs(cand - x.reshape(-1, 32)[:, :, None])
    assert (idx == err.argmin(axis=2)).all()
    assert (np.take_along_axis(err, idx[:, :, None].astype(np.int64), axis=2)[:, :, 0] == err.min(axis=2)).all()
    # round trip: within half the widest level gap (4 d, between 8 and 12) of x inside the level range, and |x| - 12 d beyond it (amax < 16 d)
    y = xr.dequantize(raw, x.size).reshape(-1, 32)
    assert (amax < 16 * d).all()
    assert (np.abs(y - x.reshape(-1, 32)) <= np.maximum(2 * d[:, None], np.abs(x.reshape(-1, 32)) - 12 * d[:, None]) + 1e-30).all()


def test_quantiser_zero_block(pkg):
    gs = pkg.gguf_synth
    x = np.zeros(64, np.float32)
    x[40] = 3.0
    b = gs.quantize_mxfp4(x).view(gs.DT_MXFP4)
    assert b["e"][0] == 0 and (b["qs"][0] == 0).all()              # amax = 0: e = 0, every index 0
    assert b["e"][1] == 126 and (xr.dequantize(b.view(np.uint8), 64)[32:] == x[32:]).all()        # 3 = level 6 * 0.5


@pytest.mark.parametrize("K,N", [(32, 33), (96, 33), (2080, 33), (4096, 128)])
def test_block_order_dot_against_float64(pkg, K, N):
    """The restatement (per block: an exact integer sum, the product of the two scales, one product, one add - all f32) against the float64 dot of the same
    operands: each of the K / 32 terms carries two roundings and the running sum one, so the chain stays within 3 (K / 32) 2^-24 of sum |term|, which is at most
    the float64 sum of |w a|.  And the integer partials are the dots of the levels."""
    rng = np.random.default_rng(K + N)
    T = 3
    W = pkg.gguf_synth.random_blocks(rng, MXFP4, N * K, 0.05)
    x = (rng.standard_normal((T, K)) * rng.uniform(0.1, 3.0, (T, 1))).astype(np.float32)
    y, ref = xr.mul_mat(W, N, K, x), xr.mul_mat_f64(W, N, K, x)
    Wf = xr.dequantize(W, N * K).reshape(N, K)
    af = np.stack([oq.dequantize(oq.Q8_0, oq.quantize(oq.Q8_0, r), K) for r in x])
    scale = np.abs(af.astype(np.float64)) @ np.abs(Wf.astype(np.float64)).T
    assert np.abs(ref - af.astype(np.float64) @ Wf.astype(np.float64).T).max() <= 1e-12 * scale.max()      # (the float64 dot is the dot of the dequantised operands)
    assert (np.abs(y.astype(np.float64) - ref) <= 3 * (K // 32) * 2.0 ** -24 * scale + 1e-30).all(), float((np.abs(y - ref) / scale).max())
    codes = xr.quantize_act(x[1])[0]
    lv = xr.decode(W, N * K)[1].reshape(N, -1, 32)
    rb = xr.row_bytes(K)
    for r in (0, N - 1):
        isum = xr.vec_dot_int_partials(W[r * rb:(r + 1) * rb], codes, K)
        assert (isum == (lv[r].astype(np.int64) * codes).sum(axis=1)).all() and np.abs(isum).max() <= 32 * 127 * 12


def test_random_blocks_spread(pkg):
    """The writer's blocks: e in a band of three around the exponent of the requested std, levels uniform: a dequantised std within the band's factor of two,
    centred on zero."""
    gs = pkg.gguf_synth
    raw = gs.random_blocks(np.random.default_rng(5), MXFP4, 32 * 8192, 0.03)
    e = raw.view(gs.DT_MXFP4)["e"]
    assert int(e.max()) - int(e.min()) == 2 and 127 - 12 <= int(e.min()) and int(e.max()) <= 127 - 6
    y = xr.dequantize(raw, 32 * 8192)
    assert 0.5 < y.std() / 0.03 < 2.0 and abs(y.mean()) < 0.003


@pytest.mark.parametrize("cfg", ["tiny-qwen3moe", "qwen3-30b-a3b", "mixtral-8x7b", "tiny-gqa4", "llama-3-8b"])
def test_writer_mix(pkg, cfg):
    """mxfp4_moe: the tensors with a third dimension MXFP4, every other 2-D weight Q8_0 (token_embd and output included), norms and ffn_gate_inp F32 - all Q8_0
    on a dense config.  mxfp4: every 2-D weight MXFP4, the head F16."""
    gs = pkg.gguf_synth
    c = gs.CONFIGS[cfg]
    n_mx = 0
    for name, ne, ty, _ in gs.model_tensors(c, "mxfp4_moe"):
        if len(ne) == 1 or name.endswith("ffn_gate_inp.weight"):
            assert ty == gs.F32, name
        elif len(ne) == 3:
            assert ty == MXFP4 and "_exps." in name, name
            n_mx += 1
        else:
            assert ty == gs.Q8_0, name
    assert n_mx == (3 * c.n_layer if c.n_expert else 0)
    for name, ne, ty, _ in gs.model_tensors(c, "mxfp4"):
        if len(ne) == 1 or name.endswith("ffn_gate_inp.weight"):
            assert ty == gs.F32, name
        else:
            assert ty == (gs.F16 if name == "output.weight" else MXFP4), name
    assert gs.tensor_type(c, "q5_0", "attn_q", 0) == gs.Q5_0 and gs.tensor_type(c, "q8_0", "ffn_down", 0) == gs.Q8_0          # the other ftypes are what they were
    # bytes a decoded token reads: the expert share at 17 / 34 of the q8_0 file's, everything else equal
    a, b = gs.weight_bytes_per_token(c, "mxfp4_moe"), gs.weight_bytes_per_token(c, "q8_0")
    exp8 = sum(gs.row_bytes(gs.Q8_0, ne[0]) * ne[1] * c.n_expert_used for n, ne, _, _ in gs.model_tensors(c, "q8_0") if "_exps." in n)
    assert b - a == exp8 // 2


HOST_MAIN = r"""
#include "gguf.h"
#include <cstdio>
int main(int argc, char **argv) {
    mi355::GGUFFile f;
    const std::string err = f.open(argv[1]);
    if (!err.empty()) { std::printf("error: %s\n", err.c_str()); return 1; }
    std::printf("file_type %llu\n", (unsigned long long)f.get_u("general.file_type", 0));
    for (const auto &t : f.tensors)
        std::printf("%s %d %s %zu %zu\n", t.name.c_str(), t.type, mi355::ggml_type_name(t.type), t.bytes, mi355::ggml_type_row_bytes(t.type, t.ne[0]));
    return 0;
}
"""


def test_written_files_parse_and_reload_through_the_host_reader(pkg, tmp_path):
    gs = pkg.gguf_synth
    host = os.path.join(ROOT, "cortex.llamacpp_amd", "host")
    (tmp_path / "main.cc").write_text(HOST_MAIN)
    exe = str(tmp_path / "gguf_list")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", host, str(tmp_path / "main.cc"), os.path.join(host, "gguf.cc"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    for cfg, ftype in (("tiny-qwen3moe", "mxfp4_moe"), ("tiny-gqa4", "mxfp4"), ("tiny-gqa4", "mxfp4_moe")):
        path = str(tmp_path / f"{cfg}-{ftype}.gguf")
        gs.write_synthetic_llama(path, cfg, ftype, seed=7)
        kv, tens = read_gguf(path)
        assert kv["general.file_type"] == 38
        want = {n: (ne, ty) for n, ne, ty, _ in gs.model_tensors(gs.CONFIGS[cfg], ftype)}
        assert set(tens) == set(want)
        n_mx = 0
        for n, (ne, ty, raw) in tens.items():
            assert (ne, ty) == want[n], n
            if ty == MXFP4:
                cnt = int(np.prod(ne))
                nbytes = xr.row_bytes(ne[0]) * cnt // ne[0]
                assert raw.size >= nbytes and np.isfinite(xr.dequantize(raw[:nbytes], cnt)).all()
                n_mx += 1
        assert (n_mx > 0) == (ftype == "mxfp4" or cfg == "tiny-qwen3moe")
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.strip().split("\n")
        assert lines[0] == "file_type 38" and len(lines) == 1 + len(want)
        for ln in lines[1:]:
            name, ty, tname, nbytes, rowb = ln.split()
            ne, wty = want[name]
            assert int(ty) == wty and int(rowb) > 0
            if wty == MXFP4:
                assert tname == "mxfp4" and int(rowb) == ne[0] // 32 * 17 and int(nbytes) == int(rowb) * int(np.prod(ne)) // ne[0]


def test_existing_ftype_file_is_unchanged(pkg, tmp_path):
    """The writer's q4_0 and q8_0 files of tiny-qwen3moe, byte for byte what the parent commit's writer gave (sha256 recorded from it)."""
    gs = pkg.gguf_synth
    want = {"q4_0": "2f37cb112bcaca80fb940bef829b325aded30466f76af58a069404e05384221a", "q8_0": "0623d87eb21f4a65e3bcf221912ffa32142898bcc0861f5da5db6feeee727a02"}
    for ftype, sha in want.items():
        path = str(tmp_path / f"{ftype}.gguf")
        gs.write_synthetic_llama(path, "tiny-qwen3moe", ftype, seed=7)
        assert hashlib.sha256(open(path, "rb").read()).hexdigest() == sha, ftype


def test_reference_model_runs_on_an_mxfp4_moe_file(pkg, tmp_path):
    """The reference decodes an mxfp4_moe file: finite logits, one selection per layer; and on an mxfp4 file its embedding rows are the dequantised table."""
    gs = pkg.gguf_synth
    path = str(tmp_path / "m.gguf")
    gs.write_synthetic_llama(path, "tiny-qwen3moe", "mxfp4_moe", seed=2)
    r = xr.Mxfp4MoeRef(path, 32, oq.Q8_0, oq.Q8_0)
    assert r._embd_mx is None and r.t["blk.0.ffn_gate_exps.weight"][1] == MXFP4
    lg = r.decode([1, 7, 3], np.arange(3))
    assert np.isfinite(lg).all() and r.routes[-1].shape == (r.n_layer, 3, r.k)
    gs.write_synthetic_llama(path, "tiny-gqa4", "mxfp4", seed=2)
    r = xr.Mxfp4Ref(path, 32, oq.Q8_0, oq.Q8_0)
    ne, ty, raw = r._embd_mx
    E, rb = ne[0], xr.row_bytes(ne[0])
    assert ty == MXFP4 and (r.t["token_embd.weight"][2].view("<f4")[7 * E:8 * E] == xr.dequantize(raw[7 * rb:8 * rb], E)).all()
    lg = r.decode([1, 7, 3], np.arange(3))
    assert lg.shape == (1, ne[1]) and np.isfinite(lg).all()
