"""The ternary quantiser without a GPU: the numpy twin (tests/ternary_quantize_ref.py, the specification of csrc/quantize.hip's TQ1_0 / TQ2_0 branches) through
the decoders of tests/quant_error_ref.py, and tools/quantize.py's two ternary mixes with the twin in the kernel's place.  The rows built here are the GPU
test's too."""
import itertools

import numpy as np
import pytest

import quantize_ref as qr
import ternary_quantize_ref as tqr
from test_quantize_cpu import check_file, f16_files, tool  # noqa: F401  (the last two are fixtures)

TYPES = [pytest.param(tqr.TQ1_0, id="tq1_0"), pytest.param(tqr.TQ2_0, id="tq2_0")]
ZERO_BLOCK = 4


def ternary_rows(n_rows, n_per_row, seed=11):
    """f32 rows of t * s, t in {-1, 0, 1} and s an f16-exact scale per block, no block all zero: what both formats hold exactly"""
    rng = np.random.default_rng(seed)
    nb = n_rows * n_per_row // 256
    t = rng.integers(-1, 2, (nb, 256))
    t[np.arange(nb), rng.integers(0, 256, nb)] = rng.choice([-1, 1], nb)
    s = rng.uniform(0.004, 3.0, nb).astype(np.float16).astype(np.float32)
    return (t * s[:, None]).astype(np.float32).reshape(n_rows, n_per_row)


def edge_rows():
    """f32 [3][768], nine blocks.  Block 4 is all zero.  Over the other eight, the five elements j + 32 n of byte j of the first 160-element region run through
    all 243 five-trit patterns.  Every block's tail holds + and - half its extreme (the tie, exact where the scale is a power of two: the even blocks), the f32
    next below a half (code 0, not 1), and the extreme itself, which is negative in the odd blocks; nothing else reaches it."""
    rng = np.random.default_rng(5)
    pats = np.array(list(itertools.product((-1, 0, 1), repeat=5)))                              # [243][5]
    x = np.zeros((9, 256), np.float32)
    for i, b in enumerate(k for k in range(9) if k != ZERO_BLOCK):
        s = np.float32(2.0 ** -(b % 4)) * np.float32(1.0 if b % 2 == 0 else 0.8125)
        t = rng.integers(-1, 2, 256)
        t[:160] = pats[(32 * i + np.arange(32)) % 243].T.reshape(-1)                            # element j + 32 n = trit n of pattern 32 i + j
        u = np.where(t == 0, rng.uniform(-0.45, 0.45, 256), t * rng.uniform(0.55, 0.95, 256))
        u[240:245] = [0.5, -0.5, np.nextafter(np.float32(0.5), np.float32(0)), -np.nextafter(np.float32(0.5), np.float32(0)), -1.0 if b % 2 else 1.0]
        x[b] = (u * s).astype(np.float32)
    return x.reshape(3, 768)


def as_source(x, st):
    if st == tqr.BF16:
        import __graft_entry__ as ge
        return ge.load_pkg().gguf_synth.round_bf16(x).reshape(x.shape)
    return x.astype(np.float16 if st == tqr.F16 else np.float32)


@pytest.mark.parametrize("t", TYPES)
def test_the_twin_round_trips_ternary_rows_exactly(t):
    import quant_error_ref as qe
    x = ternary_rows(3, 768)
    raw = tqr.quantize_rows(t, x)
    assert raw.shape == (3, 3 * tqr.BLOCK_BYTES[t])
    assert np.array_equal(qe.decode(t, raw, 768), x)
    assert np.array_equal(tqr.quantize_rows(t, x, imatrix=np.arange(768, dtype=np.float32)), raw)
    # the edge rows hold what their docstring says: the decoded codes of the f32 rows
    e = edge_rows().reshape(9, 256)
    code = np.rint(qe.decode(t, tqr.quantize_rows(t, e.reshape(3, 768)), 768).reshape(9, 256) / np.abs(e).max(axis=1).clip(1e-30)[:, None]).astype(int)
    assert (code[ZERO_BLOCK] == 0).all() and (code[[0, 2, 6, 8], 240:244] == [1, -1, 0, 0]).all() and (code[1::2, 244] == -1).all()
    first = np.delete(code, ZERO_BLOCK, axis=0)[:, :160].reshape(8, 5, 32).transpose(0, 2, 1).reshape(-1, 5)
    assert len({tuple(p) for p in first}) == 243


def twin_rows(t, x, imatrix=None, src_type=None):
    if t in tqr.BLOCK_BYTES:
        return tqr.quantize_rows(t, x, imatrix, src_type)
    return qr.quantize_rows(t, x, imatrix, src_type=src_type)


def test_quantize_file_with_the_twin(pkg, tool, f16_files, tmp_path):  # noqa: F811
    from gguf_read import read_gguf
    gs = pkg.gguf_synth
    dst = str(tmp_path / "out.gguf")
    tool.quantize_file(f16_files["tiny"], dst, "tq2_0", quantize_rows=twin_rows, out=lambda s: None)
    _, t = check_file(pkg, tool, f16_files["tiny"], dst, "tiny", "tq2_0")
    assert t["token_embd.weight"][1] == gs.Q4_K and t["output.weight"][1] == gs.Q6_K and t["blk.1.ffn_down.weight"][1] == gs.TQ2_0
    tool.quantize_file(f16_files["tiny"], dst, "tq1_0", quantize_rows=twin_rows, pure=True, out=lambda s: None)
    kv, t = read_gguf(dst)
    assert kv["general.file_type"] == gs.FTYPE_ID["tq1_0"]
    assert all(ty == gs.TQ1_0 for ne, ty, _ in t.values() if len(ne) >= 2)
    with pytest.raises(ValueError, match=r"blk\.0\.\w+\.weight: rows of 576 .* Q4_0"):          # the ternary types' 32-element fallback is not written
        tool.quantize_file(f16_files["tiny-w576-2l"], dst, "tq2_0", quantize_rows=twin_rows)
