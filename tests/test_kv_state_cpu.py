"""CPU-side checks of the sequence-state surface: the exports exist and refuse without a GPU / on a null context, and the numpy restatement of the blob
(tests/kv_state_ref.py, the reference of tests/test_gpu_kv_state.py) gives hand-written bytes for one f16 cell and one q8_0 cell."""
import ctypes as C
import struct

import numpy as np

import kv_state_ref as ref


def test_state_exports_exist_and_refuse_a_null_context(pkg):
    lib = pkg.load_library()
    buf = np.zeros(64, np.uint8)
    n_tok = C.c_size_t(7)
    assert lib.mi355_state_seq_get_size(None, 0) == 0
    assert lib.mi355_state_seq_get_data(None, buf.ctypes.data, buf.size, 0) == 0
    assert lib.mi355_state_seq_set_data(None, buf.ctypes.data, buf.size, 0) == 0
    assert b"null context" in lib.mi355_last_error()
    assert lib.mi355_state_seq_save_file(None, b"/nonexistent/x.bin", 0, None, 0) == 0
    assert lib.mi355_state_seq_load_file(None, b"/nonexistent/x.bin", 0, None, 0, C.byref(n_tok)) == 0
    lib.mi355_debug_state_seq_timing(None, None)                       # (a null context: nothing to switch on)
    out = (C.c_int64 * 6)(*([9] * 6))
    assert lib.mi355_engine_prompt_cache_stats(None, b"m", out) < 0    # (an engine needs a device: tests/test_gpu_prompt_cache_engine.py)
    assert list(out) == [9] * 6


def test_state_op_hooks_refuse_without_a_gpu(pkg):
    lib = pkg.load_library()
    if lib.mi355_device_count() > 0:
        return                                   # (with a GPU the hooks compute: tests/test_gpu_kv_state.py)
    k = np.zeros((1, 64), np.uint8)
    ptrs = (C.c_void_p * 1)(k.ctypes.data)
    cells = np.zeros(1, np.int32)
    out = np.zeros(128, np.uint8)
    assert lib.mi355_op_kv_state_pack(1, 1, 1, 1, 32, 1, ptrs, ptrs, cells.ctypes.data, 1, out.ctypes.data) == -100
    assert lib.mi355_op_kv_state_unpack(1, 1, 1, 1, 32, 1, out.ctypes.data, cells.ctypes.data, 1, ptrs, ptrs) == -100


def test_reference_blob_of_one_f16_cell_by_hand():
    # one layer, one kv head of 32 halves, a cache of two cells; the sequence is cell 1 at position 5
    k = np.arange(2 * 64, dtype=np.uint8).reshape(2, 64)
    v = (200 - np.arange(2 * 64)).astype(np.uint8).reshape(2, 64)
    want = struct.pack("<8I", 0x564B354D, 1, 1, 1, 1, 1, 32, 1) + struct.pack("<i", 5) + bytes(range(64, 128)) + bytes((200 - i) & 255 for i in range(64, 128))
    got = ref.blob(ref.F16, ref.F16, 1, 32, [5], [k], [v], [1])
    assert got == want and len(got) == ref.blob_size(ref.F16, ref.F16, 1, 1, 32, 1) == 32 + 4 + 128
    assert want[:4] == b"M5KV"
    p = ref.parse(got)
    assert (p["n"], p["n_layer"], p["head_dim"], list(p["positions"])) == (1, 1, 32, [5])


def test_reference_blob_of_one_q8_0_cell_by_hand():
    # two layers, K q8_0 (34-byte blocks {f16 d, 32 codes}) and V f16, two kv heads of 32; cells 2 then 0 of a three-cell cache at positions 3, 9
    rbk, rbv = 2 * 34, 2 * 64
    assert (ref.row_bytes(ref.Q8_0, 2, 32), ref.row_bytes(ref.F16, 2, 32), ref.row_bytes(ref.Q4_0, 2, 32)) == (rbk, rbv, 36)
    ks = [np.full((3, rbk), 10 * l, np.uint8) + np.arange(3, dtype=np.uint8)[:, None] for l in range(2)]
    vs = [np.full((3, rbv), 100 + 10 * l, np.uint8) + np.arange(3, dtype=np.uint8)[:, None] for l in range(2)]
    want = struct.pack("<8I", 0x564B354D, 1, 8, 1, 2, 2, 32, 2) + struct.pack("<2i", 3, 9)
    for l in range(2):
        want += bytes([10 * l + 2]) * rbk + bytes([10 * l]) * rbk            # K rows of cells 2, 0
        want += bytes([100 + 10 * l + 2]) * rbv + bytes([100 + 10 * l]) * rbv    # then the V rows
    got = ref.blob(ref.Q8_0, ref.F16, 2, 32, [3, 9], ks, vs, [2, 0])
    assert got == want and len(got) == ref.blob_size(ref.Q8_0, ref.F16, 2, 2, 32, 2)
    # ... and unpack is its inverse on the listed cells, every other cell untouched
    k0 = [np.full((3, rbk), 0xEE, np.uint8) for _ in range(2)]
    v0 = [np.full((3, rbv), 0xDD, np.uint8) for _ in range(2)]
    k1, v1 = ref.unpack_rows(k0, v0, [2, 0], ref.parse(got)["rows"])
    for l in range(2):
        assert np.array_equal(k1[l][[2, 0]], ks[l][[2, 0]]) and np.array_equal(v1[l][[2, 0]], vs[l][[2, 0]])
        assert np.all(k1[l][1] == 0xEE) and np.all(v1[l][1] == 0xDD)
    assert np.array_equal(ref.pack_rows(k1, v1, [2, 0]), ref.parse(got)["rows"])
