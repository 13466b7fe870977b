"""The state blob of a sequence (mi355_state_seq_get_data) restated in numpy, from caches given as ggml-layout rows - the form the op-level test entries take
and return.  In that form the blob's row section is a plain row gather: what the device has to do on top (head-major planes, codes and scales apart) is the
kernels' business and exactly what the comparison against this file checks.

    header  8 little-endian uint32: magic "M5KV", version 1, type_k, type_v, n_layer, n_head_kv, head_dim, n
    n int32 positions, ascending
    per layer: K rows [n][row_bytes(type_k)] of the listed cells in list order, then V rows [n][row_bytes(type_v)]
"""
import struct

import numpy as np

MAGIC = 0x564B354D          # "M5KV"
VERSION = 1
HEADER_BYTES = 32
F16, Q4_0, Q8_0 = 1, 2, 8
BLOCK_BYTES = {F16: 64, Q8_0: 34, Q4_0: 18}      # bytes of 32 elements


def row_bytes(type_: int, n_head_kv: int, head_dim: int) -> int:
    assert head_dim % 32 == 0
    return n_head_kv * (head_dim // 32) * BLOCK_BYTES[type_]


def pack_rows(k_layers, v_layers, cells) -> np.ndarray:
    """The row section: k_layers / v_layers hold one uint8 [n_cells][row bytes] cache per layer."""
    cells = np.asarray(cells, np.int64).reshape(-1)
    parts = []
    for k, v in zip(k_layers, v_layers):
        parts.append(np.ascontiguousarray(k[cells]).reshape(-1))
        parts.append(np.ascontiguousarray(v[cells]).reshape(-1))
    return np.concatenate(parts).astype(np.uint8) if parts else np.zeros(0, np.uint8)


def unpack_rows(k_layers, v_layers, cells, rows):
    """The caches after `rows` (the layout pack_rows gives) were written into the listed cells: copies, every other cell untouched."""
    cells = np.asarray(cells, np.int64).reshape(-1)
    rows = np.asarray(rows, np.uint8).reshape(-1)
    ko, vo, off = [], [], 0
    for k, v in zip(k_layers, v_layers):
        k, v = k.copy(), v.copy()
        nk, nv = cells.size * k.shape[1], cells.size * v.shape[1]
        k[cells] = rows[off:off + nk].reshape(cells.size, k.shape[1]); off += nk
        v[cells] = rows[off:off + nv].reshape(cells.size, v.shape[1]); off += nv
        ko.append(k); vo.append(v)
    assert off == rows.size
    return ko, vo


def blob(type_k: int, type_v: int, n_head_kv: int, head_dim: int, positions, k_layers, v_layers, cells) -> bytes:
    positions = np.asarray(positions, np.int32).reshape(-1)
    cells = np.asarray(cells, np.int64).reshape(-1)
    assert positions.size == cells.size and np.all(np.diff(positions) > 0)
    for k, v in zip(k_layers, v_layers):
        assert k.shape[1] == row_bytes(type_k, n_head_kv, head_dim) and v.shape[1] == row_bytes(type_v, n_head_kv, head_dim)
    head = struct.pack("<8I", MAGIC, VERSION, type_k, type_v, len(k_layers), n_head_kv, head_dim, cells.size)
    return head + positions.astype("<i4").tobytes() + pack_rows(k_layers, v_layers, cells).tobytes()


def blob_size(type_k: int, type_v: int, n_layer: int, n_head_kv: int, head_dim: int, n: int) -> int:
    return HEADER_BYTES + 4 * n + n_layer * n * (row_bytes(type_k, n_head_kv, head_dim) + row_bytes(type_v, n_head_kv, head_dim))


def parse(data: bytes) -> dict:
    """Header fields, positions and the row section of a blob (checks the length against the header)."""
    magic, version, tk, tv, nl, g, d, n = struct.unpack_from("<8I", data, 0)
    assert magic == MAGIC and version == VERSION, (hex(magic), version)
    assert len(data) == blob_size(tk, tv, nl, g, d, n), (len(data), blob_size(tk, tv, nl, g, d, n))
    pos = np.frombuffer(data, "<i4", n, HEADER_BYTES)
    return {"type_k": tk, "type_v": tv, "n_layer": nl, "n_head_kv": g, "head_dim": d, "n": n, "positions": pos,
            "rows": np.frombuffer(data, np.uint8, offset=HEADER_BYTES + 4 * n)}
