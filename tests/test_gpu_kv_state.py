"""A sequence's KV state on the GPU: the gather / scatter kernels against the numpy restatement (tests/kv_state_ref.py), byte for byte, and
mi355_state_seq_get_data / set_data / save_file / load_file on small models - a restored sequence continues as the original does."""
import numpy as np
import pytest

import kv_state_ref as ref
from test_gpu_model import FLIP_TOL, KV, make, rel_err      # FLIP_TOL: the bar tests/test_gpu_model.py holds a shifted context to against the CPU restatement

pytestmark = pytest.mark.gpu

N_CELLS, N_LAYER = 192, 2                                   # three 64-cell attention chunks
CELL_LISTS = {
    "first_chunk": list(range(64)),
    "last_cell": [191],
    "all": list(range(192)),
    "scattered": [130, 5, 64, 63, 191],                     # not ascending; both sides of a chunk boundary; the last cell of a plane
}
TYPE_PAIRS = [(ref.F16, ref.F16), (ref.Q8_0, ref.Q8_0), (ref.Q4_0, ref.Q4_0), (ref.Q8_0, ref.F16), (ref.F16, ref.Q4_0)]


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def random_caches(rng, type_k, type_v, G, D):
    ks = [rng.integers(0, 256, (N_CELLS, ref.row_bytes(type_k, G, D)), dtype=np.uint8) for _ in range(N_LAYER)]
    vs = [rng.integers(0, 256, (N_CELLS, ref.row_bytes(type_v, G, D)), dtype=np.uint8) for _ in range(N_LAYER)]
    return ks, vs


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("type_k,type_v", TYPE_PAIRS)
def test_pack_and_unpack_kernels_are_exact(be, type_k, type_v, D, G):
    """Byte equality against the restatement for every cell list: pack gives the listed rows in list order; unpack into a cache pre-filled with a byte pattern
    sets the listed cells to the rows and leaves every other cell of every layer - codes and scales, both travel inside the ggml rows - as it was; pack(unpack(x)) == x."""
    rng = np.random.default_rng(1000 * type_k + 100 * type_v + D + G)
    ks, vs = random_caches(rng, type_k, type_v, G, D)
    for name, cells in CELL_LISTS.items():
        want = ref.pack_rows(ks, vs, cells)
        got = be.kv_state_pack(type_k, type_v, G, D, ks, vs, cells)
        assert got.shape == want.shape and np.array_equal(got, want), name
        # unpack: fresh random rows into caches that hold a byte pattern
        x = rng.integers(0, 256, want.size, dtype=np.uint8)
        k0 = [np.full_like(k, 0xA5) for k in ks]
        v0 = [np.full_like(v, 0x5A) for v in vs]
        k1, v1 = be.kv_state_unpack(type_k, type_v, G, D, k0, v0, cells, x)
        kw, vw = ref.unpack_rows(k0, v0, cells, x)
        rest = np.setdiff1d(np.arange(N_CELLS), cells)
        for l in range(N_LAYER):
            assert np.array_equal(k1[l], kw[l]) and np.array_equal(v1[l], vw[l]), (name, l)
            assert np.all(k1[l][rest] == 0xA5) and np.all(v1[l][rest] == 0x5A), (name, l)
        assert np.array_equal(be.kv_state_pack(type_k, type_v, G, D, k1, v1, cells), x), name


def test_op_hooks_refuse_cells_outside_the_cache_and_listed_twice(be, pkg):
    rng = np.random.default_rng(5)
    ks, vs = random_caches(rng, ref.Q8_0, ref.Q8_0, 1, 64)
    with pytest.raises(pkg.MI355Error, match="outside the cache"):
        be.kv_state_pack(ref.Q8_0, ref.Q8_0, 1, 64, ks, vs, [0, N_CELLS])
    x = np.zeros(ref.pack_rows(ks, vs, [3, 3]).size, np.uint8)
    with pytest.raises(pkg.MI355Error, match="listed twice"):
        be.kv_state_unpack(ref.Q8_0, ref.Q8_0, 1, 64, ks, vs, [3, 3], x)


# ---------------------------------------------------------------------------------------------------------------- model level
def steps(ctx, toks, pos0, seq=0):
    out = []
    for i, t in enumerate(toks):
        ctx.decode([int(t)], [pos0 + i], [seq])
        out.append(ctx.logits().copy())
    return np.stack(out)


@pytest.mark.parametrize("kv", ["f16", "q8_0"])
@pytest.mark.parametrize("cfg", ["tiny", "tiny-d128"])
def test_restored_sequence_continues_bit_identically(be, pkg, tmp_models, cfg, kv):
    """Context 1 decodes a 40-token prompt, hands out its state and takes 4 single-token steps; a fresh context 2 takes the state and the same 4 steps.  Both hold
    the sequence in cells 0..39, so the launches see the same memory: the logits are compared with np.array_equal.  Context 1's four steps are first run twice
    from the same state: were they not bit-reproducible run to run at this shape, that spread would be the bar instead (observed spread on an MI355X: 0 for all
    four cases, so the bar is equality)."""
    path = make(pkg, tmp_models, cfg, "q4_k_m")
    m = pkg.Model(path)
    rng = np.random.default_rng(17)
    prompt, nxt = rng.integers(0, m.n_vocab, 40), rng.integers(0, m.n_vocab, 4)
    c1 = pkg.Context(m, n_ctx=128, type_k=KV[kv], type_v=KV[kv])
    c1.decode(prompt, np.arange(40))
    blob = c1.state_seq_get(0)
    hdr = ref.parse(blob)
    assert hdr["n"] == 40 and list(hdr["positions"]) == list(range(40)) and hdr["type_k"] == KV[kv] and len(blob) == c1.state_seq_size(0)
    a = steps(c1, nxt, 40)
    assert c1.kv_seq_rm(0, 40, -1)
    b = steps(c1, nxt, 40)
    spread = float(np.abs(a - b).max())
    print(f"run-to-run spread of the four steps ({cfg}, {kv}): {spread:g}")
    c2 = pkg.Context(m, n_ctx=128, type_k=KV[kv], type_v=KV[kv])
    assert c2.state_seq_set(0, blob) == len(blob) and c2.kv_used() == 40
    r = steps(c2, nxt, 40)
    print(f"restored against original: max abs difference {float(np.abs(r - a).max()):g}")
    if spread == 0.0:
        assert np.array_equal(r, a)
    else:
        assert float(np.abs(r - a).max()) <= spread
    assert c2.state_seq_get(0)[:len(blob)][32:32 + 160] == blob[32:32 + 160]      # (positions 0..39 again; 4 more cells behind them)
    c1.close(); c2.close(); m.close()


def test_state_through_a_small_staging_block_in_chunks(be, pkg, tmp_models):
    """The device staging of the rows is bounded (64 MiB): a longer sequence crosses it in chunks of cells, every chunk's rows copied to / from their places in
    the blob.  Here the bound is 16 KiB, a 45-cell sequence of this model goes in several chunks with a ragged last one, K in q8_0 and V in f16 (rows of
    different sizes), and the blob, the restored cells and the continuation are those of the one-chunk path."""
    path = make(pkg, tmp_models, "tiny-d128", "q4_k_m")
    m = pkg.Model(path)
    rng = np.random.default_rng(19)
    prompt, nxt = rng.integers(0, m.n_vocab, 45), rng.integers(0, m.n_vocab, 4)
    c1 = pkg.Context(m, n_ctx=128, type_k=KV["q8_0"], type_v=KV["f16"])
    c1.decode(prompt, np.arange(45))
    blob = c1.state_seq_get(0)
    per_cell = (len(blob) - ref.HEADER_BYTES - 4 * 45) // 45
    assert 16 * 1024 // per_cell >= 1 and 45 / (16 * 1024 // per_cell) > 2 and 45 % (16 * 1024 // per_cell), per_cell     # at least three chunks, the last one ragged
    a = steps(c1, nxt, 45)
    be.set_option("state_stage_kib", 16)
    try:
        c2 = pkg.Context(m, n_ctx=128, type_k=KV["q8_0"], type_v=KV["f16"])
        c3 = pkg.Context(m, n_ctx=128, type_k=KV["q8_0"], type_v=KV["f16"])
        assert c2.state_seq_set(0, blob) == len(blob)
        assert c2.state_seq_get(0) == blob                                  # chunked scatter, then chunked gather
    finally:
        be.set_option("state_stage_kib", 0)
    assert c3.state_seq_set(0, c2.state_seq_get(0)) == len(blob)            # (c3 first moves a state now: one chunk)
    assert c3.state_seq_get(0) == blob
    assert np.array_equal(steps(c2, nxt, 45), a)
    for c in (c1, c2, c3):
        c.close()
    m.close()


@pytest.mark.parametrize("kv", ["f16", "q8_0"])
def test_restore_into_another_sequence_of_the_same_context(be, pkg, tmp_models, kv):
    """n_seq_max 4 over 512 cells: regions of 128 cells, whole chunks.  Sequence 0's state restored into sequence 2 while sequence 0 stays resident lands on the
    first cells of region 2 (alloc_cells: results do not depend on the slot), and the same 4 steps give the same bits."""
    path = make(pkg, tmp_models, "tiny-d128", "q4_k_m")
    m = pkg.Model(path)
    rng = np.random.default_rng(23)
    prompt, nxt = rng.integers(0, m.n_vocab, 40), rng.integers(0, m.n_vocab, 4)
    c = pkg.Context(m, n_ctx=512, n_seq_max=4, type_k=KV[kv], type_v=KV[kv])
    c.decode(prompt, np.arange(40), [0] * 40)
    blob = c.state_seq_get(0)
    a = steps(c, nxt, 40, seq=0)
    assert c.state_seq_set(2, blob) == len(blob)
    assert c.kv_used() == 44 + 40 and c.state_seq_size(2) == len(blob) and c.state_seq_get(2) == blob
    r = steps(c, nxt, 40, seq=2)
    print(f"sequence 2 against sequence 0: max abs difference {float(np.abs(r - a).max()):g}")
    assert np.array_equal(r, a)
    c.close(); m.close()


@pytest.mark.parametrize("kv", ["f16", "q8_0"])
def test_state_of_a_shifted_sequence(be, pkg, tmp_models, kv):
    """A context shift is pending when the state is taken: get applies it first, so the blob's positions are 0..31 and its K rows are rotated for them.  The
    restored context holds the sequence in cells 0..31, the original in cells 0..7 and 24..47 - another chunk partition, so the next step is compared at
    FLIP_TOL, the bar tests/test_gpu_model.py (test_kv_seq_ops_match_oracle) holds a shifted context to."""
    path = make(pkg, tmp_models, "tiny-d128", "q4_k_m")
    m = pkg.Model(path)
    rng = np.random.default_rng(29)
    prompt = rng.integers(0, m.n_vocab, 48)
    c1 = pkg.Context(m, n_ctx=128, type_k=KV[kv], type_v=KV[kv])
    c1.decode(prompt, np.arange(48))
    assert c1.kv_seq_rm(0, 8, 24)
    c1.kv_seq_add(0, 24, -1, -16)
    blob = c1.state_seq_get(0)
    assert list(ref.parse(blob)["positions"]) == list(range(32))
    c2 = pkg.Context(m, n_ctx=128, type_k=KV[kv], type_v=KV[kv])
    assert c2.state_seq_set(0, blob) == len(blob)
    c1.decode([11], [32]); a = c1.logits().copy()
    c2.decode([11], [32]); r = c2.logits().copy()
    print(f"shifted, restored against original: rel_err {rel_err(r, a):g}")
    assert rel_err(r, a) <= FLIP_TOL
    c1.close(); c2.close(); m.close()


def test_refusals_name_the_field_and_leave_the_sequence_empty(be, pkg, tmp_models):
    path = make(pkg, tmp_models, "tiny-d128", "q4_k_m")
    m = pkg.Model(path)
    rng = np.random.default_rng(31)
    src = pkg.Context(m, n_ctx=256, type_k=KV["q8_0"], type_v=KV["q8_0"])
    src.decode(rng.integers(0, m.n_vocab, 130), np.arange(130))
    blob = src.state_seq_get(0)

    def empty(ctx, seq):
        return ctx.kv_used() == 0 and ctx.state_seq_size(seq) == ref.HEADER_BYTES

    f16 = pkg.Context(m, n_ctx=256, type_k=KV["f16"], type_v=KV["f16"])
    with pytest.raises(pkg.MI355Error, match=r"type_k mismatch: the blob has 8, the context has 1"):
        f16.state_seq_set(0, blob)
    assert empty(f16, 0)
    q8 = pkg.Context(m, n_ctx=256, type_k=KV["q8_0"], type_v=KV["q8_0"])
    with pytest.raises(pkg.MI355Error, match=rf"truncated blob: {len(blob) - 10} bytes, its header asks for {len(blob)}"):
        q8.state_seq_set(0, blob[:-10])
    assert empty(q8, 0)
    with pytest.raises(pkg.MI355Error, match=r"truncated blob: 12 bytes"):
        q8.state_seq_set(0, blob[:12])
    bad = bytearray(blob); bad[32 + 4:32 + 8] = (0).to_bytes(4, "little")          # position 1 -> 0: not ascending
    with pytest.raises(pkg.MI355Error, match=r"positions not ascending at index 1: 0 then 0"):
        q8.state_seq_set(0, bytes(bad))
    assert empty(q8, 0)
    par = pkg.Context(m, n_ctx=512, n_seq_max=4, type_k=KV["q8_0"], type_v=KV["q8_0"])     # regions of 128 cells
    with pytest.raises(pkg.MI355Error, match=r"n mismatch: the blob has 130 cells, the region of sequence 1 has 128"):
        par.state_seq_set(1, blob)
    assert empty(par, 1)
    assert q8.state_seq_set(0, blob) == len(blob) and q8.kv_used() == 130               # (the blob itself is good)
    for c in (src, f16, q8, par):
        c.close()
    m.close()


def test_file_round_trip(be, pkg, tmp_models, tmp_path):
    path = make(pkg, tmp_models, "tiny-d128", "q4_k_m")
    m = pkg.Model(path)
    rng = np.random.default_rng(37)
    prompt = rng.integers(0, m.n_vocab, 40).astype(np.int32)
    c1 = pkg.Context(m, n_ctx=128, type_k=KV["q8_0"], type_v=KV["q8_0"])
    c1.decode(prompt, np.arange(40))
    f = str(tmp_path / "seq0.state")
    n = c1.state_seq_save_file(f, 0, prompt)
    assert n == 24 + 4 * 40 + c1.state_seq_size(0)
    import os
    assert os.path.getsize(f) == n and not os.path.exists(f + ".tmp")
    c2 = pkg.Context(m, n_ctx=128, type_k=KV["q8_0"], type_v=KV["q8_0"])
    toks = c2.state_seq_load_file(f, 0)
    assert np.array_equal(toks, prompt) and c2.kv_used() == 40
    c1.decode([3], [40]); c2.decode([3], [40])
    assert np.array_equal(c1.logits(), c2.logits())
    with open(f, "rb") as fh:
        data = fh.read()
    with open(f, "wb") as fh:
        fh.write(data[:-100])                                                          # the length no longer matches the header: refused before a row is read
    c3 = pkg.Context(m, n_ctx=128, type_k=KV["q8_0"], type_v=KV["q8_0"])
    with pytest.raises(pkg.MI355Error, match="file length mismatch"):
        c3.state_seq_load_file(f, 0)
    assert c3.kv_used() == 0
    for c in (c1, c2, c3):
        c.close()
    m.close()
