"""The quantiser without a GPU: the numpy twin of tests/quantize_ref.py (the specification csrc/quantize.hip follows) against the CPU oracle's decoders, the
three conditions the GPU tests rely on, the rounding spread that sets their margins, and every piece of file logic of tools/quantize.py with the twin in the
kernel's place."""
import importlib.util
import os

import numpy as np
import pytest

import quantize_cases as qc
import quantize_ref as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_TYPES = (qr.Q8_0, qr.Q5_0, qr.Q5_1) + qr.K_TYPES
FILES = ("tiny", "tiny-w576-2l", "tiny-moe")


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("quantize_tool", os.path.join(ROOT, "tools", "quantize.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def f16_files(pkg, tmp_models):
    out = {}
    for cfg in FILES:
        out[cfg] = os.path.join(str(tmp_models), f"{cfg}.f16.gguf")
        if not os.path.exists(out[cfg]):
            pkg.gguf_synth.write_synthetic_llama(out[cfg], cfg, "f16")
    return out


def rel_rms(t, x, raw):
    y = qc.dequantize(t, raw, x.shape[1]).astype(np.float64)
    return ((y - x) ** 2).sum(), (x.astype(np.float64) ** 2).sum()


def test_q8_0_equals_the_oracle_bit_for_bit():
    import oracle_py as op
    for K in qc.K32_SHAPES:
        for x in (qc.normal(K, 67), qc.special(K)):
            got = qr.quantize_rows(qr.Q8_0, x)
            want = np.stack([op.quantize(op.Q8_0, r) for r in x])
            assert np.array_equal(got, want), K


@pytest.mark.parametrize("t", ALL_TYPES, ids=lambda t: qc.NAME[t])
def test_every_block_dequantises_finite(t):
    for K in qc.shapes(t):
        for w in (None, qc.heavy_imatrix(K)):
            for x in (qc.normal(K, 3), qc.special(K)):
                raw = qr.quantize_rows(t, x, w)
                assert raw.shape == (x.shape[0], K // qr.BLOCK_ELEMS[t] * qr.BLOCK_BYTES[t])
                y = qc.dequantize(t, raw, K)
                assert np.isfinite(y).all(), (K, w is not None)
            zero = qc.dequantize(t, qr.quantize_rows(t, qc.special(K)[:1], w), K)
            assert (zero == 0).all()
            # the row that F32, F16 and BF16 all hold exactly: the same bytes from each source format
            common = qc.special(K)[5:6]
            ref = qr.quantize_rows(t, common, w)
            for st in (qr.F16, qr.BF16):
                assert np.array_equal(qr.quantize_rows(t, qc.as_source(common, st), w, src_type=st), ref), st


def test_conditions_the_gpu_tests_rely_on():
    """On the normal inputs: the tensor-mean relative RMS error is strictly ordered by bit width; the search is no worse than the same type's plain
    round-to-nearest; the 1/4-heavy importance matrix lowers the squared error on the heavy columns."""
    rms = {}
    for t in (qr.Q8_0,) + qr.K_TYPES:
        num = den = num_rtn = heavy = heavy_im = 0.0
        for K in qc.shapes(t):
            for R in qc.ROWS:
                x = qc.normal(K, R)
                a, b = rel_rms(t, x, qr.quantize_rows(t, x))
                num, den = num + a, den + b
                if t in qr.K_TYPES:
                    num_rtn += rel_rms(t, x, qr.quantize_rtn(t, x))[0]
                    y = qc.dequantize(t, qr.quantize_rows(t, x), K)
                    yi = qc.dequantize(t, qr.quantize_rows(t, x, qc.heavy_imatrix(K)), K)
                    heavy += float((((y - x)[:, ::4]).astype(np.float64) ** 2).sum())
                    heavy_im += float((((yi - x)[:, ::4]).astype(np.float64) ** 2).sum())
        rms[t] = np.sqrt(num / den)
        print(f"{qc.NAME[t]}: rel rms {rms[t]:.5f}" + (f", round-to-nearest {np.sqrt(num_rtn / den):.5f}, heavy columns {heavy:.4e} -> {heavy_im:.4e}"
                                                     if t in qr.K_TYPES else ""))
        if t in qr.K_TYPES:
            assert num <= num_rtn, qc.NAME[t]
            assert heavy_im < heavy, qc.NAME[t]
    order = (qr.Q8_0, qr.Q6_K, qr.Q5_K, qr.Q4_K, qr.Q3_K, qr.Q2_K)
    assert all(rms[a] < rms[b] for a, b in zip(order, order[1:])), rms


def spread_inputs(t):
    for K in qc.shapes(t):
        for x in [qc.normal(K, R) for R in qc.ROWS] + [qc.special(K)]:
            for w in (None, qc.heavy_imatrix(K)):
                yield K, x, w


@pytest.mark.parametrize("t", qr.K_TYPES, ids=lambda t: qc.NAME[t])
def test_rounding_spread(t):
    """The f32 twin against the f64 twin over the case inputs: the share of byte-identical blocks and the largest per-row relative difference in weighted
    error.  M_TYPE (the GPU test's margin) is twice that spread, written as a constant: it must cover what is measured here and not be a round-up of more
    than a tenth on top."""
    spread, same, blocks = 0.0, 0, 0
    for K, x, w in spread_inputs(t):
        b32, b64 = qr.quantize_rows(t, x, w), qr.quantize_rows(t, x, w, dtype=np.float64)
        e32, e64 = qc.weighted_error(t, x, b32, w), qc.weighted_error(t, x, b64, w)
        nz = e64 > 0
        assert (e32[~nz] == 0).all()
        if nz.any():
            spread = max(spread, float((np.abs(e32[nz] - e64[nz]) / e64[nz]).max()))
        nb = b32.size // qr.BLOCK_BYTES[t]
        same += int((b32.reshape(nb, -1) == b64.reshape(nb, -1)).all(axis=1).sum())
        blocks += nb
    print(f"{qc.NAME[t]}: {same / blocks:.4f} of {blocks} blocks byte-identical between the f32 and the f64 twin; largest per-row relative difference in "
          f"weighted error {spread:.4e}; M_TYPE {qc.M_TYPE[t]:.4e}")
    want = 2.0 * spread if spread > 0 else 1e-4
    assert want <= qc.M_TYPE[t] <= 1.1 * want, (want, qc.M_TYPE[t])


def check_file(pkg, tool, src, dst, cfg_name, ftype, with_imatrix=False):
    """per-tensor types as gguf_synth.tensor_type gives them, copied tensors and metadata byte-equal, the file-type keys"""
    from gguf_read import read_gguf
    gs = pkg.gguf_synth
    kv0, t0 = read_gguf(src)
    kv1, t1 = read_gguf(dst)
    assert list(t0) == list(t1)
    want = {name: ty for name, _, ty, _ in gs.model_tensors(gs.CONFIGS[cfg_name], ftype)}
    for name, (ne, ty, raw) in t1.items():
        assert ne == t0[name][0], name
        if name in want and len(ne) >= 2 and "ffn_gate_inp" not in name:
            assert ty == want[name], (name, ty, want[name])
        else:
            assert ty == t0[name][1] and raw.tobytes() == t0[name][2].tobytes(), name
    extra = [k for k in kv1 if k.startswith("quantize.imatrix.")]
    added = [k for k in kv1 if k not in kv0 and k not in extra]              # (a file-type key the source lacks goes behind the copied ones)
    assert set(added) <= {"general.file_type", "general.quantization_version"}
    assert list(kv1) == list(kv0) + added + extra
    for k, v in kv0.items():
        if k not in ("general.file_type", "general.quantization_version"):
            assert kv1[k] == v, k
    assert kv1["general.file_type"] == gs.FTYPE_ID[ftype] and kv1["general.quantization_version"] == 2
    assert bool(extra) == with_imatrix
    return kv1, t1


@pytest.mark.parametrize("cfg,ftype,chunk_rows", [("tiny", "q4_k_m", 1), ("tiny", "q2_k", 37), ("tiny-w576-2l", "q4_k_m", 37), ("tiny-w576-2l", "q8_0", 1),
                                                  ("tiny-moe", "q4_k_m", 301)])
def test_quantize_file_with_the_twin(pkg, tool, f16_files, tmp_path, cfg, ftype, chunk_rows):
    import oracle_py as op
    dst = str(tmp_path / "out.gguf")
    lines = []
    tool.quantize_file(f16_files[cfg], dst, ftype, quantize_rows=qr.quantize_rows, out=lines.append)
    check_file(pkg, tool, f16_files[cfg], dst, cfg, ftype)
    assert len(lines) == len(pkg.gguf_synth.model_tensors(pkg.gguf_synth.CONFIGS[cfg], ftype)) + 1 and "quantised size" in lines[-1]
    m = op.OracleModel(dst)
    assert m.n_vocab == pkg.gguf_synth.CONFIGS[cfg].n_vocab
    # the bytes do not depend on the chunk size: one row a call (a few odd rows where a row a call would take the twin minutes) against everything in one
    dst1 = str(tmp_path / "out1.gguf")
    tool.quantize_file(f16_files[cfg], dst1, ftype, quantize_rows=qr.quantize_rows, chunk_bytes=chunk_rows * 256 * 2 if chunk_rows > 1 else 1, out=lines.append)
    assert open(dst, "rb").read() == open(dst1, "rb").read()


def random_imatrix(pkg, tool, path, seed=5, zero_expert=True):
    """an importance matrix of random positive sums for every layer tensor of the file (one expert never routed to)"""
    from gguf_read import read_gguf
    rng = np.random.default_rng(seed)
    entries = {}
    for name, (ne, ty, _) in read_gguf(path)[1].items():
        if len(ne) < 2 or not name.startswith("blk.") or "ffn_gate_inp" in name:
            continue
        n_mat = ne[2] if len(ne) == 3 else 1
        counts = rng.integers(5, 90, n_mat).astype(np.float32)
        if zero_expert and n_mat > 1:
            counts[1] = 0
        entries[name] = ((rng.random((n_mat, ne[0])).astype(np.float32) + 0.05) * counts[:, None], counts)
    return tool.imx.IMatrix(entries, ["calib.txt"], 7, 64)


@pytest.mark.parametrize("form", ["gguf", "dat"])
def test_quantize_file_with_an_imatrix(pkg, tool, f16_files, tmp_path, form):
    from gguf_read import read_gguf
    src = f16_files["tiny-moe"]
    im = random_imatrix(pkg, tool, src)
    imp = str(tmp_path / f"im.{form}")
    tool.imx.write_imatrix(imp, im)
    dst, plain = str(tmp_path / "im.out.gguf"), str(tmp_path / "plain.gguf")
    tool.quantize_file(src, dst, "q4_k_m", imatrix=imp, quantize_rows=qr.quantize_rows, out=lambda s: None)
    tool.quantize_file(src, plain, "q4_k_m", quantize_rows=qr.quantize_rows, out=lambda s: None)
    kv, t = check_file(pkg, tool, src, dst, "tiny-moe", "q4_k_m", with_imatrix=True)
    assert kv["quantize.imatrix.file"] == imp and kv["quantize.imatrix.dataset"] == "calib.txt"
    assert kv["quantize.imatrix.entries_count"] == len(im.entries) and kv["quantize.imatrix.chunks_count"] == 7
    # expert by expert with its own columns: expert 2 of blk.0.ffn_up_exps equals the twin on that expert's rows and weights; the expert that was never routed to
    # (count 0) took the neutral weight 1
    name = "blk.0.ffn_up_exps.weight"
    ne, ty, raw = t[name]
    src_raw = read_gguf(src)[1][name][2]
    rb = qr.BLOCK_BYTES[ty] * ne[0] // qr.BLOCK_ELEMS[ty]
    s, c = im.entries[name]
    w2 = s[2].astype(np.float64) / c[2]
    if form == "dat":                                # (the legacy file stores the mean square times the call count in f32; the reader divides again)
        w2 = (w2 * 7).astype(np.float32).astype(np.float64) / 7
    for e, w in ((2, w2.astype(np.float32)), (1, np.ones(ne[0], np.float32))):
        x = src_raw[e * ne[1] * ne[0] * 2:(e + 1) * ne[1] * ne[0] * 2].view(np.float16).reshape(ne[1], ne[0])
        got = raw[e * ne[1] * rb:(e + 1) * ne[1] * rb].reshape(ne[1], rb)
        assert np.array_equal(got, qr.quantize_rows(ty, x, w)), e
    assert raw.tobytes() != read_gguf(plain)[1][name][2].tobytes()


def test_refusals(pkg, tool, f16_files, tmp_models, tmp_path):
    dst = str(tmp_path / "no.gguf")
    with pytest.raises(ValueError, match="q4_0"):                                    # a mix outside the ten
        tool.quantize_file(f16_files["tiny"], dst, "q4_0", quantize_rows=qr.quantize_rows)
    q = os.path.join(str(tmp_models), "tiny.q4_k_m.forquant.gguf")
    pkg.gguf_synth.write_synthetic_llama(q, "tiny", "q4_k_m")
    with pytest.raises(ValueError, match="token_embd.weight.*requantising"):          # a quantised source
        tool.quantize_file(q, dst, "q8_0", quantize_rows=qr.quantize_rows)
    im = random_imatrix(pkg, tool, f16_files["tiny"])
    del im.entries["blk.1.ffn_down.weight"]
    imp = str(tmp_path / "missing.gguf")
    tool.imx.write_imatrix(imp, im)
    with pytest.raises(ValueError, match="blk.1.ffn_down.weight"):                    # an imatrix with a missing entry
        tool.quantize_file(f16_files["tiny"], dst, "q4_k_m", imatrix=imp, quantize_rows=qr.quantize_rows)
    im = random_imatrix(pkg, tool, f16_files["tiny"])
    im.entries["blk.0.attn_q.weight"] = (np.ones((1, 128), np.float32), np.ones(1, np.float32))
    tool.imx.write_imatrix(imp, im)
    with pytest.raises(ValueError, match="blk.0.attn_q.weight"):                      # ... or one of another length
        tool.quantize_file(f16_files["tiny"], dst, "q4_k_m", imatrix=imp, quantize_rows=qr.quantize_rows)
    with pytest.raises(ValueError, match="IQ4_NL"):                                   # rows of 576 in a Q2_K mix
        tool.quantize_file(f16_files["tiny-w576-2l"], dst, "q2_k", quantize_rows=qr.quantize_rows)
    assert not os.path.exists(dst)
    assert tool.main([f16_files["tiny"], dst, "iq4_xs"]) == 2                         # refused before a device is asked for


def softmax_kl(p_logits, q_logits):
    p = p_logits.astype(np.float64) - p_logits.max()
    q = q_logits.astype(np.float64) - q_logits.max()
    lp, lq = p - np.log(np.exp(p).sum()), q - np.log(np.exp(q).sum())
    return float((np.exp(lp) * (lp - lq)).sum())


def test_kl_against_f16_is_ordered_through_the_oracle(pkg, tool, f16_files, tmp_path):
    """over 40 tokens against the F16 file, the mean KL divergence of the twin's files: q8_0 < q4_k_m < q2_k (the ordering the GPU test asserts for the
    device's files, here for the reference alone)"""
    import oracle_py as op
    toks = np.random.default_rng(3).integers(0, 512, 40).astype(np.int32)

    def logits(path):
        m = op.OracleModel(path)
        c = op.OracleContext(m, 64)
        return np.asarray(c.decode(toks, np.arange(40), want_logits=np.ones(40, np.int8))).reshape(40, -1)

    base = logits(f16_files["tiny"])
    kl = {}
    for ftype in ("q8_0", "q4_k_m", "q2_k"):
        dst = str(tmp_path / f"{ftype}.gguf")
        tool.quantize_file(f16_files["tiny"], dst, ftype, quantize_rows=qr.quantize_rows, out=lambda s: None)
        got = logits(dst)
        kl[ftype] = float(np.mean([softmax_kl(base[i], got[i]) for i in range(40)]))
    print(kl)
    assert 0 <= kl["q8_0"] < kl["q4_k_m"] < kl["q2_k"], kl


def test_exports_and_no_device(pkg):
    lib = pkg.load_library()
    assert "mi355_quantize_chunk" in pkg.binding.SYMBOLS and "mi355_quantize_supported" in pkg.binding.SYMBOLS
    for t in ALL_TYPES:
        assert lib.mi355_quantize_supported(t) == 1
    for t in (0, 1, 2, 3, 20, 23, 30, 39, -1, 1000):
        assert lib.mi355_quantize_supported(t) == 0
    if lib.mi355_device_count() > 0:
        return
    x = np.zeros(256, np.float32)
    out = np.zeros(144, np.uint8)
    assert lib.mi355_quantize_chunk(qr.Q4_K, 0, x.ctypes.data, 256, 1, None, out.ctypes.data) == -100
