"""The upload's regrouping of ggml rows into device rows (csrc/misc.hip launch_repack_rows), alone, through mi355_op_repack_rows: byte for byte against a numpy
restatement that knows each type's plane order as a list of block field names and nothing of the C++ table.  The inputs are random BYTES (this compares bytes, not
values); the entry fills the destination with 0xA5 first, so a padding byte that is anything else was written by a store past a row's end."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 0xA5
ERR_ARG = -103                                              # MI355_ERR_ARG (include/mi355_llama.h)
# device order of each repacked type's planes, as field names of gguf_synth.BLOCK_DTYPE (a tuple: fields that sit side by side in the block and stay together)
PLANES = {
    "Q6_K": ["ql", "qh", "scales", "d"], "Q2_K": ["qs", "scales", ("d", "dmin")], "Q3_K": ["hmask", "qs", "scales", "d"],
    "IQ4_XS": ["qs", "scales_l", "scales_h", "d"], "TQ1_0": ["qs", "qh", "d"], "TQ2_0": ["qs", "d"], "Q8_0": ["qs", "d"],
    "Q4_0": ["qs", "d"], "IQ4_NL": ["qs", "d"], "Q5_0": ["qs", "qh", "d"], "Q4_1": ["qs", "d", "m"], "Q5_1": ["qs", "qh", "d", "m"], "MXFP4": ["qs", "e"],
}
TYPES_256 = ["Q6_K", "Q2_K", "Q3_K", "IQ4_XS", "TQ1_0", "TQ2_0"]
TYPES_32 = ["Q8_0", "Q4_0", "IQ4_NL", "Q5_0", "Q4_1", "Q5_1", "MXFP4"]


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def plane(blk, f):
    """blk: (rows, blocks).  One plane of every row: the bytes of field f (or of the fields f, side by side) of the row's blocks, one block after the other"""
    fs = f if isinstance(f, tuple) else (f,)
    per_block = np.concatenate([np.ascontiguousarray(blk[x]).view(np.uint8).reshape(blk.shape + (-1,)) for x in fs], axis=2)
    return per_block.reshape(blk.shape[0], -1)


def reference(gs, name, raw, K, n_rows):
    """(n_rows, row bytes): the device rows without their padding, plane after plane"""
    t = getattr(gs, name)
    blk = raw.view(gs.BLOCK_DTYPE[t]).reshape(n_rows, K // gs.BLOCK_ELEMS[t])
    want = np.concatenate([plane(blk, f) for f in PLANES[name]], axis=1)
    assert want.shape == (n_rows, raw.size // n_rows)           # the planes are the whole block
    return want


def run(pkg, be, name, K, n_rows, seed=0):
    gs = pkg.gguf_synth
    t = getattr(gs, name)
    grow = K // gs.BLOCK_ELEMS[t] * gs.BLOCK_BYTES[t]
    drow = (grow + 15) & ~15
    raw = np.random.default_rng(seed).integers(0, 256, n_rows * grow, dtype=np.uint8)
    got = be.repack_rows(t, raw, K, n_rows, drow)
    assert got.shape == (n_rows, drow)
    return raw, got, grow


def check_rows(got, want, grow, rows):
    for r in rows:
        assert (got[r, :grow] == want[r]).all(), (r, np.flatnonzero(got[r, :grow] != want[r])[:8])
    assert (got[:, grow:] == GUARD).all()


@pytest.mark.parametrize("name", TYPES_256 + TYPES_32)
def test_repacked_rows_byte_exact(pkg, be, name):
    # three 256-element blocks: every `blocks *` offset differs from its one-block value; eleven 32-element blocks: not a multiple of the eight a workgroup
    # takes, and a row size that needs padding
    K = 768 if name in TYPES_256 else 352
    raw, got, grow = run(pkg, be, name, K, 3, seed=len(name) + K)
    check_rows(got, reference(pkg.gguf_synth, name, raw, K, 3), grow, range(3))


def test_the_cases_cover_every_repacked_type():
    assert len(TYPES_256) + len(TYPES_32) == 13 and set(TYPES_256 + TYPES_32) == set(PLANES)


@pytest.mark.parametrize("name,K", [("Q4_0", 32), ("Q6_K", 256)])
def test_more_rows_than_one_grid_holds(pkg, be, name, K):
    n = 65538                                                   # 65535 rows to a launch: the second one takes three
    raw, got, grow = run(pkg, be, name, K, n, seed=5)
    want = reference(pkg.gguf_synth, name, raw, K, n)
    check_rows(got, want, grow, (0, 65534, 65535, n - 1))
    assert zlib.crc32(np.ascontiguousarray(got[:, :grow])) == zlib.crc32(np.ascontiguousarray(want))


@pytest.mark.parametrize("name,K", [("Q4_K", 256), ("Q5_K", 256), ("F16", 36)])
def test_unchanged_rows(pkg, be, name, K):
    raw, got, grow = run(pkg, be, name, K, 3, seed=K)
    assert name != "F16" or (grow, got.shape[1]) == (72, 80)    # the strided copy
    check_rows(got, raw.reshape(3, grow), grow, range(3))


@pytest.mark.parametrize("t,K", [(14, 300), (2, 40), (99, 256)])
def test_refusals(be, t, K):
    src, dst = np.zeros(4096, np.uint8), np.full(4096, 7, np.uint8)
    assert be.lib.mi355_op_repack_rows(t, src.ctypes.data, K, 1, dst.ctypes.data) == ERR_ARG
    assert be.lib.mi355_op_repack_rows(14, src.ctypes.data, 256, 0, dst.ctypes.data) == ERR_ARG
    assert (dst == 7).all()
