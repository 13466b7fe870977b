"""Synthetic GGUF v3 writer (tests / bench tooling, not product code).

There is no network and no real checkpoint on either box, so models are
synthesised: exact hparams / tensor names / shapes / `*_K_M` type mix of the named config
(SURVEY.md §A.4, §A.5), weights = seeded random *valid* quant blocks.  The files are ordinary
GGUF v3 and are loaded through the same loader as any unmodified GGUF.

Reference behaviour this feeds: `/loadmodel` -> LoadModelImpl (src/llama_engine.cc:547-732) ->
common_init_from_params (src/llama_server_context.cc:207).
"""
from __future__ import annotations

import os
import struct
from dataclasses import dataclass, field

import numpy as np

# ggml type ids: the package's one list of them (binding.py takes them from here; tests pin them to csrc/ggml_types.h)
F32, F16, Q4_0, Q8_0, Q4_K, Q5_K, Q6_K = 0, 1, 2, 8, 12, 13, 14
Q8_K = 15   # an activation format, never a file type
Q2_K, Q3_K = 10, 11
Q5_0, IQ4_NL = 6, 20
Q4_1, Q5_1 = 3, 7
IQ4_XS = 23
BF16 = 30
MXFP4 = 39
TQ1_0, TQ2_0 = 34, 35
TYPE_NAME = {F32: "f32", F16: "f16", Q4_0: "q4_0", Q8_0: "q8_0", Q4_K: "q4_K", Q5_K: "q5_K", Q6_K: "q6_K", Q2_K: "q2_K", Q3_K: "q3_K", Q5_0: "q5_0", IQ4_NL: "iq4_nl", IQ4_XS: "iq4_xs", BF16: "bf16", Q4_1: "q4_1", Q5_1: "q5_1", MXFP4: "mxfp4", TQ1_0: "tq1_0", TQ2_0: "tq2_0"}
BLOCK_ELEMS = {F32: 1, F16: 1, Q4_0: 32, Q8_0: 32, Q4_K: 256, Q5_K: 256, Q6_K: 256, Q2_K: 256, Q3_K: 256, Q5_0: 32, IQ4_NL: 32, IQ4_XS: 256, BF16: 1, Q4_1: 32, Q5_1: 32, MXFP4: 32, TQ1_0: 256, TQ2_0: 256}
BLOCK_BYTES = {F32: 4, F16: 2, Q4_0: 18, Q8_0: 34, Q4_K: 144, Q5_K: 176, Q6_K: 210, Q2_K: 84, Q3_K: 110, Q5_0: 22, IQ4_NL: 18, IQ4_XS: 136, BF16: 2, Q4_1: 20, Q5_1: 24, MXFP4: 17, TQ1_0: 54, TQ2_0: 66}

DT_Q4_0 = np.dtype([("d", "<f2"), ("qs", "u1", 16)])
DT_Q8_0 = np.dtype([("d", "<f2"), ("qs", "i1", 32)])
DT_Q4_K = np.dtype([("d", "<f2"), ("dmin", "<f2"), ("scales", "u1", 12), ("qs", "u1", 128)])
DT_Q5_K = np.dtype([("d", "<f2"), ("dmin", "<f2"), ("scales", "u1", 12), ("qh", "u1", 32), ("qs", "u1", 128)])
DT_Q6_K = np.dtype([("ql", "u1", 128), ("qh", "u1", 64), ("scales", "i1", 16), ("d", "<f2")])
DT_Q2_K = np.dtype([("scales", "u1", 16), ("qs", "u1", 64), ("d", "<f2"), ("dmin", "<f2")])
DT_Q3_K = np.dtype([("hmask", "u1", 32), ("qs", "u1", 64), ("scales", "u1", 12), ("d", "<f2")])
DT_Q5_0 = np.dtype([("d", "<f2"), ("qh", "u1", 4), ("qs", "u1", 16)])
# Q4_1 / Q5_1: unsigned codes q (0..15; 0..31 with the fifth bit of element j in bit j of qh) and a per-block minimum, weight = q * d + m
DT_Q4_1 = np.dtype([("d", "<f2"), ("m", "<f2"), ("qs", "u1", 16)])
DT_Q5_1 = np.dtype([("d", "<f2"), ("m", "<f2"), ("qh", "u1", 4), ("qs", "u1", 16)])
# MXFP4: one E8M0 scale byte e and sixteen level indices per half block, weight = KVALUES_MXFP4[nibble] * d with d = half of 2^(e - 127) (mxfp4_scale)
DT_MXFP4 = np.dtype([("e", "u1"), ("qs", "u1", 16)])
KVALUES_MXFP4 = np.array([0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12], np.int8)      # the e2m1 values doubled
# IQ4_XS: 6-bit sub-block scales ls (low nibbles in scales_l, high bit pairs in scales_h), weight = d * (ls - 32) * kvalues_iq4nl[nibble]
DT_IQ4_XS = np.dtype([("d", "<f2"), ("scales_h", "<u2"), ("scales_l", "u1", 4), ("qs", "u1", 128)])
# the ternary types: 256 codes 0..2 per block and one f16 scale, weight = (code - 1) * d.  TQ2_0: element 128 h + 32 l + m is bits 2 l .. 2 l + 1 of qs[32 h + m].
# TQ1_0: five trits to a byte (four in a qh byte), trit n of byte b = ((b * 3^n mod 256) * 3) >> 8; qs[0..31] hold elements 32 n + m, qs[32..47] elements
# 160 + 16 n + m, qh[0..3] elements 240 + 4 n + j (tq1_element_map).  Restated from upstream's generic-scalar code as remembered; its source is not available
# where this was written, so the layout cannot be pinned against it here.
DT_TQ1_0 = np.dtype([("qs", "u1", 48), ("qh", "u1", 4), ("d", "<f2")])
DT_TQ2_0 = np.dtype([("qs", "u1", 64), ("d", "<f2")])
POW3 = np.array([1, 3, 9, 27, 81], np.uint32)
BLOCK_DTYPE = {Q4_0: DT_Q4_0, Q8_0: DT_Q8_0, Q4_K: DT_Q4_K, Q5_K: DT_Q5_K, Q6_K: DT_Q6_K, Q2_K: DT_Q2_K, Q3_K: DT_Q3_K, Q5_0: DT_Q5_0, IQ4_NL: DT_Q4_0, IQ4_XS: DT_IQ4_XS, Q4_1: DT_Q4_1, Q5_1: DT_Q5_1, MXFP4: DT_MXFP4, TQ1_0: DT_TQ1_0, TQ2_0: DT_TQ2_0}
for _t, _dt in BLOCK_DTYPE.items():
    assert _dt.itemsize == BLOCK_BYTES[_t], (_t, _dt.itemsize)

# std of (dequantised weight / d) for uniformly random block payloads (derived in DESIGN.md)
# (Q2_K: w / d = sc * q - r * m with sc, m uniform 0..15, q uniform 0..3, r = 1.5: variance 144.7 + 2.25 * 21.25; Q3_K: (sc - 32) * q, sc 0..63, q -4..3)
_UNIT_STD = {Q4_0: 4.6, Q8_0: 73.9, Q4_K: 258.0, Q5_K: 527.0, Q6_K: 1367.0, Q2_K: 13.9, Q3_K: 43.3, Q5_0: 9.23, IQ4_NL: 67.2,
             IQ4_XS: 1246.3,   # (Q5_0: codes 0..31 minus 16; IQ4_NL: the sixteen code-book levels; IQ4_XS: (ls - 32) * level, ls 0..63: sqrt(341.5 * 4548))
             Q4_1: 4.61, Q5_1: 9.23,   # (codes uniform 0..15 / 0..31 around the minimum below: sqrt((16^2 - 1) / 12), sqrt((32^2 - 1) / 12))
             MXFP4: 5.85,              # (the sixteen levels, uniform: sqrt(2 * 274 / 16))
             TQ1_0: float(np.sqrt(2.0 / 3.0)), TQ2_0: float(np.sqrt(2.0 / 3.0))}    # (trits - 1, 0, 1 uniform)
# dmin/d ratio that centres the weights of a random block on zero
_DMIN_RATIO = {Q4_K: 7.5, Q5_K: 15.5, Q2_K: 1.5}
# m/d ratio doing the same for the per-block minimum of Q4_1 / Q5_1 (weight = q d + m: minus the mean code)
_MIN_RATIO = {Q4_1: -7.5, Q5_1: -15.5}


def row_bytes(t: int, n: int) -> int:
    assert n % BLOCK_ELEMS[t] == 0, (t, n)
    return n // BLOCK_ELEMS[t] * BLOCK_BYTES[t]


def round_bf16(x: np.ndarray) -> np.ndarray:
    """f32 -> bf16 bits (uint16) as ggml_compute_fp32_to_bf16 does: nearest, ties to even; a NaN keeps its upper bits and gets the quiet bit; subnormals are kept."""
    u = np.ascontiguousarray(x, "<f4").view(np.uint32)
    r = ((u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)).astype(np.uint16)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, ((u >> np.uint32(16)) | np.uint32(64)).astype(np.uint16), r).astype("<u2")


def random_blocks(rng: np.random.Generator, t: int, n_elems: int, std: float) -> np.ndarray:
    """n_elems weights of ggml type t as raw bytes; dequantised std ~= `std`, mean ~= 0."""
    if t == F32:
        return (rng.standard_normal(n_elems, dtype=np.float32) * np.float32(std)).astype("<f4").view(np.uint8)
    if t == F16:
        return (rng.standard_normal(n_elems, dtype=np.float32) * np.float32(std)).astype("<f2").view(np.uint8)
    if t == BF16:                                            # the f32 draws that F16 rounds to half, rounded to bf16 instead
        return round_bf16(rng.standard_normal(n_elems, dtype=np.float32) * np.float32(std)).view(np.uint8)
    nb = n_elems // BLOCK_ELEMS[t]
    if t in (TQ1_0, TQ2_0):                                  # well-formed codes: uniform trits (never TQ2_0's code 3 nor a TQ1_0 byte that no five trits encode)
        blk = pack_ternary(t, rng.integers(0, 3, size=(nb, 256), dtype=np.uint8))
        d = (rng.uniform(0.5, 1.5, size=nb) * (std / _UNIT_STD[t])).astype(np.float32)
        blk["d"] = d.astype("<f2")
        return blk.view(np.uint8).reshape(-1)
    raw = rng.integers(0, 256, size=nb * BLOCK_BYTES[t], dtype=np.uint8)
    blk = raw.view(BLOCK_DTYPE[t])
    if t == MXFP4:
        # power-of-two scales: e in a band of three around the exponent whose scale gives the requested std (d = 2^(e - 128) = std / 5.85: e = 127 - 10 .. 127 - 6
        # for the model tensors' std of 0.01 .. 0.1)
        c = int(np.clip(np.rint(np.log2(std / _UNIT_STD[t])) + 128, 2, 253))
        blk["e"] = rng.integers(c - 1, c + 2, size=nb).astype(np.uint8)
        return raw
    d = (rng.uniform(0.5, 1.5, size=nb) * (std / _UNIT_STD[t])).astype(np.float32)
    blk["d"] = d.astype("<f2")
    if t in _DMIN_RATIO:
        blk["dmin"] = (d * _DMIN_RATIO[t]).astype("<f2")
    if t in _MIN_RATIO:
        blk["m"] = (d * _MIN_RATIO[t]).astype("<f2")
    return raw


def tq1_element_map():
    """(byte, n) of each of the 256 elements of a TQ1_0 block: byte indexes qs (0..47) then qh (48..51), n is the trit position in that byte."""
    e = np.arange(256)
    byte = np.where(e < 160, e % 32, np.where(e < 240, 32 + (e - 160) % 16, 48 + (e - 240) % 4))
    n = np.where(e < 160, e // 32, np.where(e < 240, (e - 160) // 16, (e - 240) // 4))
    return byte, n


def pack_ternary(t: int, codes: np.ndarray) -> np.ndarray:
    """codes [nb][256] (0..2; TQ2_0 also takes 3) as blocks of type t with d = 0.  TQ1_0 as quantize_row_tq1_0_ref packs: a byte's trits are accumulated
    most significant first (q = q * 3 + trit, the trit of position 0 first), a qh byte takes four and is multiplied by 3 once more, and the byte stored is
    (q * 256 + 242) / 243."""
    codes = np.ascontiguousarray(codes).astype(np.uint32).reshape(-1, 256)
    blk = np.zeros(codes.shape[0], BLOCK_DTYPE[t])
    if t == TQ2_0:
        c = codes.reshape(-1, 2, 4, 32)                     # [block][h][l][m]
        blk["qs"] = (c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).reshape(-1, 64).astype(np.uint8)
        return blk
    assert t == TQ1_0 and codes.max(initial=0) <= 2
    byte, n = tq1_element_map()
    q = np.zeros((codes.shape[0], 52), np.uint32)
    for pos in range(5):                                     # position 0 is the most significant digit
        sel = n == pos
        q[:, byte[sel]] = q[:, byte[sel]] * 3 + codes[:, sel]
    q[:, 48:] *= 3                                           # four trits only: the fifth digit is zero
    packed = ((q * 256 + 242) // 243).astype(np.uint8)
    blk["qs"], blk["qh"] = packed[:, :48], packed[:, 48:]
    return blk


def unpack_ternary(t: int, raw: np.ndarray) -> np.ndarray:
    """The codes [nb][256] of blocks of type t by the formats' formulas - defined for every byte value (TQ2_0: 0..3, TQ1_0: 0..2)."""
    blk = np.ascontiguousarray(raw).view(np.uint8).reshape(-1).view(BLOCK_DTYPE[t])
    if t == TQ2_0:
        qs = blk["qs"].reshape(-1, 2, 1, 32)
        return ((qs >> (2 * np.arange(4, dtype=np.uint8)).reshape(1, 1, 4, 1)) & 3).reshape(-1, 256).astype(np.uint8)
    assert t == TQ1_0
    byte, n = tq1_element_map()
    b = np.concatenate([blk["qs"], blk["qh"]], axis=1).astype(np.uint32)[:, byte]
    return ((((b * POW3[n][None, :]) & 0xff) * 3) >> 8).astype(np.uint8)


def _quantize_ternary(t: int, x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 256)
    d = np.abs(x).max(axis=1).astype(np.float32)
    with np.errstate(divide="ignore"):
        inv = np.where(d != 0, np.float32(1.0) / d, np.float32(0.0)).astype(np.float32)
    v = (x * inv[:, None]).astype(np.float32)
    xi = (np.sign(v) * np.floor(np.abs(v) + np.float32(0.5))).astype(np.int32) + 1          # lroundf: halves away from zero
    blk = pack_ternary(t, xi.astype(np.uint32) & 3)
    blk["d"] = d.astype("<f2")
    return blk.view(np.uint8).reshape(-1)


def quantize_tq1_0(x: np.ndarray) -> np.ndarray:
    """x (f32, a multiple of 256 values) as TQ1_0 blocks (raw bytes) by quantize_row_tq1_0_ref: d = max |x|, id = d ? 1 / d : 0, trit = lroundf(x * id) + 1."""
    return _quantize_ternary(TQ1_0, x)


def quantize_tq2_0(x: np.ndarray) -> np.ndarray:
    """As quantize_tq1_0 with TQ2_0's two-bit fields (quantize_row_tq2_0_ref: q |= (xi & 3) << 2 n)."""
    return _quantize_ternary(TQ2_0, x)


def quantize_min32(t: int, x: np.ndarray) -> np.ndarray:
    """x (f32, a multiple of 32 values) as Q4_1 / Q5_1 blocks (raw bytes), by ggml's reference quantisers quantize_row_q4_1_ref / quantize_row_q5_1_ref:
    per block d = (max - min) / 15 (Q5_1: / 31), m = min, q = min(15 | 31, (int)((x - min) * (1 / d) + 0.5)) in f32 (1 / d = 0 for a constant block); d and m are
    stored as f16.  Element j < 16 goes to the low nibble of qs[j], element j + 16 to the high one; Q5_1's fifth bit of element j is bit j of qh."""
    assert t in (Q4_1, Q5_1), t
    top = 15 if t == Q4_1 else 31
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 32)
    mn, mx = x.min(axis=1), x.max(axis=1)
    d = ((mx - mn) / np.float32(top)).astype(np.float32)
    with np.errstate(divide="ignore"):
        inv = np.where(d != 0, np.float32(1.0) / d, np.float32(0.0)).astype(np.float32)
    q = np.minimum(top, (((x - mn[:, None]) * inv[:, None]).astype(np.float32) + np.float32(0.5)).astype(np.int32)).astype(np.uint32)
    blk = np.zeros(x.shape[0], BLOCK_DTYPE[t])
    blk["d"], blk["m"] = d.astype("<f2"), mn.astype("<f2")
    blk["qs"] = ((q[:, :16] & 15) | ((q[:, 16:] & 15) << 4)).astype(np.uint8)
    if t == Q5_1:
        qh = (((q >> 4) & 1) << np.arange(32, dtype=np.uint32)).sum(axis=1, dtype=np.uint32)
        blk["qh"] = qh.astype("<u4").view(np.uint8).reshape(-1, 4)
    return blk.view(np.uint8).reshape(-1)


def mxfp4_scale(e: np.ndarray) -> np.ndarray:
    """The f32 block scale of E8M0 byte e: half of 2^(e - 127), as a bit pattern (0x00200000 << e below 2, else (e - 1) << 23; e = 255 gives 2^127)."""
    e = np.asarray(e).astype(np.uint32)
    return np.where(e < 2, np.uint32(0x00200000) << e, (np.maximum(e, 1) - np.uint32(1)) << np.uint32(23)).astype("<u4").view(np.float32)


def quantize_mxfp4(x: np.ndarray) -> np.ndarray:
    """x (f32, a multiple of 32 values) as MXFP4 blocks (raw bytes) by ggml's reference quantiser quantize_row_mxfp4_ref: per block amax = max |x|,
    e = amax > 0 ? (u8)(floor(log2f(amax)) - 2 + 127) : 0, d = mxfp4_scale(e); each weight takes the level index with the smallest |level * d - x|, the lowest
    index on a tie (strict < scanning 0..15).  Element j < 16 goes to the low nibble of qs[j], element j + 16 to the high one."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 32)
    amax = np.abs(x).max(axis=1)
    with np.errstate(divide="ignore"):
        lg = np.floor(np.log2(np.where(amax > 0, amax, np.float32(1.0)).astype(np.float32))).astype(np.float32)
    e = np.where(amax > 0, (lg - np.float32(2) + np.float32(127)).astype(np.int32) & 0xff, 0).astype(np.uint8)
    d = mxfp4_scale(e)
    err = np.abs((KVALUES_MXFP4.astype(np.float32)[None, None, :] * d[:, None, None]).astype(np.float32) - x[:, :, None])      # [block][element][level]
    q = np.argmin(err, axis=2).astype(np.uint8)               # (argmin returns the first minimum: the lowest index on a tie)
    blk = np.zeros(x.shape[0], DT_MXFP4)
    blk["e"] = e
    blk["qs"] = (q[:, :16] & 15) | ((q[:, 16:] & 15) << 4)
    return blk.view(np.uint8).reshape(-1)


# ---------------------------------------------------------------- container
_GT = {"u8": 0, "i8": 1, "u16": 2, "i16": 3, "u32": 4, "i32": 5, "f32": 6, "bool": 7, "str": 8, "arr": 9,
       "u64": 10, "i64": 11, "f64": 12}
_FMT = {0: "<B", 1: "<b", 2: "<H", 3: "<h", 4: "<I", 5: "<i", 6: "<f", 7: "<?", 10: "<Q", 11: "<q", 12: "<d"}


def _s(b: str | bytes) -> bytes:
    if isinstance(b, str):
        b = b.encode("utf-8")
    return struct.pack("<Q", len(b)) + b


class GGUFWriter:
    """Streaming GGUF v3 writer: metadata first, tensor payloads generated one at a time."""

    def __init__(self, alignment: int = 32):
        self.alignment = alignment
        self.kv: list[bytes] = []
        self.tensors: list[tuple[str, tuple[int, ...], int, object]] = []

    def add(self, key: str, kind: str, value) -> None:
        t = _GT[kind]
        if kind == "str":
            payload = _s(value)
        else:
            payload = struct.pack(_FMT[t], value)
        self.kv.append(_s(key) + struct.pack("<I", t) + payload)

    def add_array(self, key: str, kind: str, values) -> None:
        et = _GT[kind]
        if kind == "str":
            body = b"".join(_s(v) for v in values)
        else:
            body = np.asarray(values).astype(np.dtype(_FMT[et][1:]).newbyteorder("<")).tobytes()
        self.kv.append(_s(key) + struct.pack("<I", 9) + struct.pack("<IQ", et, len(values)) + body)

    def add_tensor(self, name: str, ne: tuple[int, ...], t: int, data) -> None:
        """data: bytes-like / uint8 ndarray, or a zero-arg callable returning one (lazy)."""
        self.tensors.append((name, tuple(int(x) for x in ne), t, data))

    def write(self, path: str) -> int:
        al = self.alignment
        sizes, offs, off = [], [], 0
        for _, ne, t, _ in self.tensors:
            n = int(np.prod(ne))
            sz = row_bytes(t, ne[0]) * (n // ne[0])
            sizes.append(sz)
            offs.append(off)
            off += (sz + al - 1) // al * al
        with open(path, "wb") as f:
            f.write(struct.pack("<IIQQ", 0x46554747, 3, len(self.tensors), len(self.kv)))
            for kv in self.kv:
                f.write(kv)
            for (name, ne, t, _), o in zip(self.tensors, offs):
                f.write(_s(name) + struct.pack("<I", len(ne)) + b"".join(struct.pack("<Q", x) for x in ne))
                f.write(struct.pack("<IQ", t, o))
            pos = f.tell()
            f.write(b"\0" * ((-pos) % al))
            # lazy tensors are generated by a few threads running ahead of the writer (numpy's generators release the GIL on bulk draws; every tensor has its
            # own seeded generator, so the bytes do not depend on who draws them or when), a bounded window of them in memory at a time
            from concurrent.futures import ThreadPoolExecutor
            n_workers = max(1, min(8, (os.cpu_count() or 2) - 1))
            window = 2 * n_workers
            with ThreadPoolExecutor(max_workers=n_workers) as ex:
                pending = {}

                def submit(i):
                    d = self.tensors[i][3]
                    pending[i] = ex.submit(d) if callable(d) else None

                nt = len(self.tensors)
                for i in range(min(window, nt)):
                    submit(i)
                for i, ((name, ne, t, data), sz) in enumerate(zip(self.tensors, sizes)):
                    fut = pending.pop(i)
                    buf = fut.result() if fut is not None else data
                    if i + window < nt:
                        submit(i + window)
                    buf = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf.view(np.uint8).reshape(-1)
                    assert buf.size == sz, (name, buf.size, sz)
                    f.write(memoryview(buf))
                    f.write(b"\0" * ((-sz) % al))
                    del buf
            return f.tell()


# ---------------------------------------------------------------- model configs
@dataclass
class LlamaConfig:
    name: str
    n_embd: int
    n_layer: int
    n_head: int
    n_head_kv: int
    n_ff: int
    n_vocab: int
    rope_base: float = 10000.0
    eps: float = 1e-5
    n_ctx_train: int = 4096
    n_expert: int = 0
    n_expert_used: int = 0
    big_model: bool = False          # 70B-class rule: attn_v Q4_K -> Q5_K on the non-Q6_K layers
    arch: str = "llama"              # general.architecture: "qwen2" is the same graph with NEOX rope pairing and (qkv_bias) attention biases;
                                     # "qwen3" is qwen2's without biases, with a per-head RMSNorm of Q and K before the rope and its own head size;
                                     # "qwen3moe" is qwen3's attention with routed experts (n_expert > 0) of width n_ff_exp
    qkv_bias: bool = False
    extra: dict = field(default_factory=dict)
    n_head_dim: int = 0              # attention head size (attention.key_length / value_length); 0: n_embd / n_head
    tied_output: bool = False        # no output.weight: the head reuses token_embd.weight
    n_ff_exp: int = 0                # width of one expert ({arch}.expert_feed_forward_length, written when set); 0: n_ff

    @property
    def head_dim(self) -> int:
        return self.n_head_dim or self.n_embd // self.n_head


CONFIGS = {
    # BASELINE.json configs (SURVEY.md §8a sizes)
    "tinyllama-1.1b": LlamaConfig("TinyLlama-1.1B-Chat", 2048, 22, 32, 4, 5632, 32000, 10000.0, 1e-5, 2048),
    "llama-2-7b": LlamaConfig("Llama-2-7B-Chat", 4096, 32, 32, 32, 11008, 32000, 10000.0, 1e-5, 4096),
    "llama-3-8b": LlamaConfig("Llama-3-8B-Instruct", 4096, 32, 32, 8, 14336, 128256, 500000.0, 1e-5, 8192),
    "mixtral-8x7b": LlamaConfig("Mixtral-8x7B-Instruct", 4096, 32, 32, 8, 14336, 32000, 1e6, 1e-5, 32768, 8, 2),
    "llama-3-70b": LlamaConfig("Llama-3-70B-Instruct", 8192, 80, 64, 8, 28672, 128256, 500000.0, 1e-5, 8192,
                               big_model=True),
    # qwen2 architecture (NEOX rope, Q / K / V biases), 7 query heads per kv head, hidden size and feed-forward width that are no multiples of 1024
    "qwen2-7b": LlamaConfig("Qwen2-7B-Instruct", 3584, 28, 28, 4, 18944, 152064, 1e6, 1e-6, 32768, arch="qwen2", qkv_bias=True),
    # qwen3 architecture (qwen2's graph without biases, per-head q / k RMSNorm, head size 128): Qwen3-8B's geometry, and Qwen3-4B's (attention width 4096 > n_embd
    # 2560, tied output)
    "qwen3-8b": LlamaConfig("Qwen3-8B", 4096, 36, 32, 8, 12288, 151936, 1e6, 1e-6, 40960, arch="qwen3", n_head_dim=128),
    "qwen3-4b": LlamaConfig("Qwen3-4B", 2560, 36, 32, 8, 9728, 151936, 1e6, 1e-6, 40960, arch="qwen3", n_head_dim=128, tied_output=True),
    # the reference's embedding smoke model (Makefile:6): nomic-embed-text-v1.5's geometry, a bidirectional encoder (general.architecture nomic-bert)
    "nomic-embed": LlamaConfig("nomic-embed-text-v1.5", 768, 12, 12, 12, 3072, 30522, 1000.0, 1e-12, 2048, arch="nomic-bert"),
    # test-sized
    "tiny": LlamaConfig("tiny-test", 256, 2, 4, 2, 512, 512, 10000.0, 1e-5, 512),
    "tiny-gqa4": LlamaConfig("tiny-gqa4", 512, 3, 8, 2, 1024, 768, 500000.0, 1e-5, 1024),
    "tiny-d128": LlamaConfig("tiny-d128", 1024, 2, 8, 2, 2048, 512, 500000.0, 1e-5, 1024),      # head_dim 128, GQA 4:1
    "tiny-d128-mha": LlamaConfig("tiny-d128-mha", 512, 2, 4, 4, 1024, 512, 10000.0, 1e-5, 1024),  # head_dim 128, MHA
    "tiny-moe": LlamaConfig("tiny-moe", 256, 2, 4, 2, 512, 512, 1e6, 1e-5, 512, 8, 2),
    # hidden sizes that are multiples of 2048: the shapes the persistent single-token mat-vec (fused RMSNorm / quantise
    # prologues) and the MFMA prefill planes are built for
    "tiny-e2048": LlamaConfig("tiny-e2048", 2048, 2, 16, 4, 4096, 512, 500000.0, 1e-5, 1024),
    # TinyLlama-1.1B's layer geometry (the reference's smoke model, Makefile:5): head_dim 64, 8 query heads per kv head, FF = 5632 = 5.5 x 1024
    "tiny-tl-2l": LlamaConfig("tiny-tl-2l", 2048, 2, 32, 4, 5632, 512, 10000.0, 1e-5, 1024),
    # 8 KV heads of 128 (one 1024-wide K / V row, GQA 2:1): the shape the single-launch decode attention (rope + cache
    # store + split attention + merge) and the chunk-list batched steps are built for — Llama-3-8B's own KV geometry
    # Llama-3-8B's layer geometry (4096 / 14336, 32 heads over 8 KV heads), two layers: the whole-step kernel's shape
    "tiny-8b-2l": LlamaConfig("tiny-8b-2l", 4096, 2, 32, 8, 14336, 512, 500000.0, 1e-5, 1024),
    # Llama-3-8B's ATTENTION geometry (4096, 32 heads over 8 kv heads) with a narrow feed-forward: the ctx-4096 parity case needs a 3968-token prompt on the
    # CPU side, and four fifths of a layer's CPU time are its feed-forward, which does not depend on the context length (tests/test_gpu_model.py)
    "tiny-8b-attn-2l": LlamaConfig("tiny-8b-attn-2l", 4096, 2, 32, 8, 2048, 512, 500000.0, 1e-5, 4096),
    # two layers of Llama-3-70B's geometry (BASELINE config 5): split over 8 ranks a rank holds 8 query heads on ONE kv head, attn_output columns of 1024 = 4
    # super-blocks, ffn_down columns of 3584 = 14 super-blocks (and the 28672-wide ffn_down's column halves meet the column slicing)
    "tiny-70b-2l": LlamaConfig("tiny-70b-2l", 8192, 2, 64, 8, 28672, 512, 500000.0, 1e-5, 1024),
    "tiny-g8": LlamaConfig("tiny-g8", 2048, 2, 16, 8, 4096, 512, 500000.0, 1e-5, 1024),
    # Llama-2-7B's ATTENTION geometry (4096, 32 heads, 32 kv heads: BASELINE config 2) with a narrow feed-forward, two layers: a workgroup's share of the 12288 Q | K | V
    # rows is 140 KB - more than the fused attention-block launch (csrc/attn_out.hip) can hold: the two launches (tools/r6_qf_ring.patch streamed it through a ring: slower)
    "tiny-7b-attn-2l": LlamaConfig("tiny-7b-attn-2l", 4096, 2, 32, 32, 2048, 512, 10000.0, 1e-5, 1024),
    # Llama-3-70B's feed-forward width on a narrow model: 28672 has no weight-stream form, its single-token ffn_down runs as two column halves of 14336
    "tiny-ff28k": LlamaConfig("tiny-ff28k", 1024, 2, 8, 2, 28672, 512, 500000.0, 1e-5, 1024),
    # three layers of Llama-3-8B's geometry: two launches of the layer engine (decode_engine.hip) that hand Q | K | V on + the last one
    # general.architecture "qwen2": NEOX rope pairing + Q / K / V biases (one of the reference's weekend test families, e2e-test-server-weekend.py:22-76).
    # tiny-qwen2: head_dim 64; tiny-qwen2-1.5b-2l / -7b-2l: two layers of Qwen2-1.5B's (1536, 12 / 2 heads of 128, 8960) and Qwen2-7B's (3584, 28 / 4, 18944) geometry
    "tiny-qwen2": LlamaConfig("tiny-qwen2", 512, 3, 8, 2, 1024, 768, 1e6, 1e-6, 1024, arch="qwen2", qkv_bias=True),
    "tiny-qwen2-1.5b-2l": LlamaConfig("tiny-qwen2-1.5b-2l", 1536, 2, 12, 2, 8960, 512, 1e6, 1e-6, 1024, arch="qwen2", qkv_bias=True),
    "tiny-qwen2-7b-2l": LlamaConfig("tiny-qwen2-7b-2l", 3584, 2, 28, 4, 18944, 512, 1e6, 1e-6, 1024, arch="qwen2", qkv_bias=True),
    # three and five query heads of 128 per kv head (Llama-3.2-3B's 24 / 8; 40 / 8): the attention kernels' odd head ratios on prompts and steps
    "tiny-r3": LlamaConfig("tiny-r3", 1536, 2, 12, 4, 4096, 512, 500000.0, 1e-5, 1024),
    "tiny-r5": LlamaConfig("tiny-r5", 1280, 2, 10, 2, 3584, 512, 500000.0, 1e-5, 1024),
    # YaRN rope scaling read from the file (factor 4 over an original context of 32 positions, attn_factor 0.9): golden fixture + parity case
    "tiny-yarn": LlamaConfig("tiny-yarn", 512, 3, 8, 2, 1024, 768, 500000.0, 1e-5, 1024,
                             extra={"rope.scaling.type": "yarn", "rope.scaling.factor": 4.0, "rope.scaling.original_context_length": 32, "rope.scaling.attn_factor": 0.9}),
    # general.architecture nomic-bert (the reference's embedding smoke model is nomic-embed-text-v1.5, Makefile:6): a bidirectional encoder, embeddings only.
    # tiny-nomic: head_dim 64 as the real one; nomic-embed-2l: two layers of its geometry (768, 12 heads of 64, 3072, 30522 WordPiece tokens, rope base 1000)
    "tiny-nomic": LlamaConfig("tiny-nomic", 256, 2, 4, 4, 512, 512, 1000.0, 1e-12, 2048, arch="nomic-bert"),
    "nomic-embed-2l": LlamaConfig("nomic-embed-2l", 768, 2, 12, 12, 3072, 30522, 1000.0, 1e-12, 2048, arch="nomic-bert"),
    # a mixture-of-experts file whose expert tensors are wide enough for the weight-stream mat-vec (hidden 2048, rows of >= 1 KiB): 8 experts, 2 used
    "tiny-moe-e2048": LlamaConfig("tiny-moe-e2048", 2048, 2, 16, 4, 4096, 512, 1e6, 1e-5, 1024, 8, 2),
    "tiny-8b-3l": LlamaConfig("tiny-8b-3l", 4096, 3, 32, 8, 14336, 512, 500000.0, 1e-5, 1024),
    # general.architecture "qwen3": head size 128 whatever n_embd / n_head is (attention width H * D above, equal to or below n_embd), q / k norms, no biases.
    # tiny-qwen3: H * D = 1024 > E = 512; the -2l configs: two layers of Qwen3-0.6B's, -4B's and -8B's geometry (the first two with tied output)
    "tiny-qwen3": LlamaConfig("tiny-qwen3", 512, 3, 8, 2, 1536, 768, 1e6, 1e-6, 1024, arch="qwen3", n_head_dim=128, tied_output=True),
    "tiny-qwen3-0.6b-2l": LlamaConfig("tiny-qwen3-0.6b-2l", 1024, 2, 16, 8, 3072, 512, 1e6, 1e-6, 1024, arch="qwen3", n_head_dim=128, tied_output=True),
    "tiny-qwen3-4b-2l": LlamaConfig("tiny-qwen3-4b-2l", 2560, 2, 32, 8, 9728, 512, 1e6, 1e-6, 1024, arch="qwen3", n_head_dim=128, tied_output=True),
    "tiny-qwen3-8b-2l": LlamaConfig("tiny-qwen3-8b-2l", 4096, 2, 32, 8, 12288, 512, 1e6, 1e-6, 1024, arch="qwen3", n_head_dim=128),
    # general.architecture "qwen3moe": qwen3's attention, 128 routed experts of which 8 are used, no shared expert; feed_forward_length is the dense width the
    # file does not use, expert_feed_forward_length the experts'.  Qwen3-30B-A3B's geometry (attention width 32 x 128 = 4096 > n_embd 2048, 8 query heads per
    # kv head); tiny-qwen3moe: H * D = 1024 > E = 512; tiny-qwen3moe-160e: more experts than 128 and not a multiple of 64; the -2l configs: two layers of
    # Qwen3-30B-A3B's and Qwen3-235B-A22B's (4096, 64 / 4 heads of 128, experts of 1536) geometry
    "qwen3-30b-a3b": LlamaConfig("Qwen3-30B-A3B", 2048, 48, 32, 4, 6144, 151936, 1e6, 1e-6, 40960, 128, 8, arch="qwen3moe", n_head_dim=128, n_ff_exp=768),
    "tiny-qwen3moe": LlamaConfig("tiny-qwen3moe", 512, 3, 8, 2, 1536, 768, 1e6, 1e-6, 1024, 128, 8, arch="qwen3moe", n_head_dim=128, n_ff_exp=256),
    "tiny-qwen3moe-160e": LlamaConfig("tiny-qwen3moe-160e", 512, 2, 8, 2, 1536, 512, 1e6, 1e-6, 1024, 160, 8, arch="qwen3moe", n_head_dim=128, n_ff_exp=256),
    "tiny-qwen3moe-30b-2l": LlamaConfig("tiny-qwen3moe-30b-2l", 2048, 2, 32, 4, 6144, 512, 1e6, 1e-6, 1024, 128, 8, arch="qwen3moe", n_head_dim=128,
                                        n_ff_exp=768),
    "tiny-qwen3moe-235b-2l": LlamaConfig("tiny-qwen3moe-235b-2l", 4096, 2, 64, 4, 12288, 512, 1e6, 1e-6, 1024, 128, 8, arch="qwen3moe", n_head_dim=128,
                                         n_ff_exp=1536),
    # hidden sizes that are whole 32-element blocks but no multiple of 256: a K-quant mix falls back to 32-element types there (FALLBACK_32), tensor by tensor.
    # Qwen2.5-0.5B (896 = 3.5 x 256, 14 / 2 heads of 64, ffn_down rows of 4864 = 19 x 256 keep their K-quants) and SmolLM2-135M (576, 9 / 3 heads of 64)
    "qwen2.5-0.5b": LlamaConfig("Qwen2.5-0.5B-Instruct", 896, 24, 14, 2, 4864, 151936, 1e6, 1e-6, 32768, arch="qwen2", qkv_bias=True, tied_output=True),
    "smollm2-135m": LlamaConfig("SmolLM2-135M-Instruct", 576, 30, 9, 3, 1536, 49152, 100000.0, 1e-5, 8192, tied_output=True),
    "tiny-w896-2l": LlamaConfig("tiny-w896-2l", 896, 2, 14, 2, 4864, 512, 1e6, 1e-6, 1024, arch="qwen2", qkv_bias=True, tied_output=True),
    "tiny-w896-2l-untied": LlamaConfig("tiny-w896-2l-untied", 896, 2, 14, 2, 4864, 512, 1e6, 1e-6, 1024, arch="qwen2", qkv_bias=True),
    "tiny-w576-2l": LlamaConfig("tiny-w576-2l", 576, 2, 9, 3, 1536, 512, 100000.0, 1e-5, 1024, tied_output=True),
    # both n_embd (320) and n_ff (608) end inside a 256-group; five query heads on one kv head
    "tiny-w320": LlamaConfig("tiny-w320", 320, 2, 5, 1, 608, 512, 1e6, 1e-6, 1024, arch="qwen2", qkv_bias=True),
}

FTYPE_ID = {"f32": 0, "f16": 1, "bf16": 32, "q4_0": 2, "q4_1": 3, "q5_0": 8, "q5_1": 9, "iq4_nl": 25, "iq4_xs": 30, "q8_0": 7, "q4_k_m": 15, "q5_k_m": 17, "q2_k": 10, "q3_k_s": 11, "q3_k_m": 12, "q3_k_l": 13, "q4_k_s": 14, "q5_k_s": 16, "q6_k": 18, "mxfp4": 38, "mxfp4_moe": 38, "tq1_0": 36, "tq2_0": 37}


def use_more_bits(i: int, n: int) -> bool:
    return i < n // 8 or i >= 7 * n // 8 or (i - n // 8) % 3 == 2


def _row_len(cfg: LlamaConfig, kind: str) -> int:
    """Row length (ne[0]) of a 2-D weight of this kind."""
    if kind == "attn_output":
        return cfg.n_head * cfg.head_dim
    if kind == "ffn_down":
        return (cfg.n_ff_exp or cfg.n_ff) if cfg.n_expert else cfg.n_ff
    return cfg.n_embd


# llama-quantize's fallback for a tensor whose rows are not a whole number of 256-element super-blocks: the 32-element type nearest in bits per weight.
# (Upstream's source is not available where this was written: the table is restated from its documented behaviour - the message "tensor cols not divisible
# by 256, required for q4_K - using fallback quantization q5_0" - and cannot be pinned against it here.)
FALLBACK_32 = {Q4_K: Q5_0, Q5_K: Q5_1, Q6_K: Q8_0, Q2_K: IQ4_NL, Q3_K: IQ4_NL, IQ4_XS: IQ4_NL, TQ1_0: Q4_0, TQ2_0: Q4_0}


def tensor_type(cfg: LlamaConfig, ftype: str, kind: str, il: int) -> int:
    """ggml type of a 2-D weight: the mix's choice (mix_tensor_type), or its 32-element fallback where the tensor's rows are not a multiple of 256 - output and a
    tied token_embd included.  No config with such a row existed before the fallback did, so every older file is written byte for byte as it was."""
    t = mix_tensor_type(cfg, ftype, kind, il)
    if BLOCK_ELEMS[t] == 256 and _row_len(cfg, kind) % 256:
        return FALLBACK_32[t]
    return t


def mix_tensor_type(cfg: LlamaConfig, ftype: str, kind: str, il: int) -> int:
    """ggml type of a 2-D weight per llama-quantize's `*_K_M` mix, before the row-length fallback."""
    if ftype == "f32":                                       # LLAMA_FTYPE_ALL_F32
        return F32
    if ftype == "f16":
        return F16
    if ftype == "bf16":                                      # LLAMA_FTYPE_MOSTLY_BF16: every 2-D weight
        return BF16
    if ftype == "q8_0":
        return Q8_0
    if ftype == "mxfp4_moe":
        # LLAMA_FTYPE_MOSTLY_MXFP4_MOE: the tensors with a third dimension (ffn_gate_exps, ffn_up_exps, ffn_down_exps) MXFP4, every other 2-D weight Q8_0,
        # token_embd and output included (a dense config has no expert tensors: all Q8_0)
        return MXFP4 if cfg.n_expert and kind in ("ffn_gate", "ffn_up", "ffn_down") else Q8_0
    if ftype == "mxfp4":
        # every 2-D weight MXFP4 with an F16 head (what `--tensor-type` overrides give; the dense decoders' test file): the id is MXFP4_MOE's, the one ftype
        # upstream has for the type
        return F16 if kind == "output" else MXFP4
    if ftype in ("q2_k", "q3_k_m"):
        # llama-quantize's rules for LLAMA_FTYPE_MOSTLY_Q2_K / Q3_K_M on the llama architecture (the reference's e2e smoke model is a TinyLlama Q2_K
        # file, /root/reference/Makefile:5): output Q6_K; Q2_K: attn_v Q4_K with a query / kv head ratio >= 4 (else Q3_K), ffn_down and attn_output
        # Q3_K; Q3_K_M: attn_v Q5_K in the first two layers then Q4_K, ffn_down Q5_K in the first n_layer / 16 layers then Q4_K, attn_output Q4_K
        q2 = ftype == "q2_k"
        if kind == "output":
            return Q6_K
        if kind == "attn_v":
            if q2:
                return Q4_K if cfg.n_head // cfg.n_head_kv >= 4 else Q3_K
            return Q5_K if il < 2 else Q4_K
        if kind == "ffn_down":
            return Q3_K if q2 else (Q5_K if il < cfg.n_layer // 16 else Q4_K)
        if kind == "attn_output":
            return Q3_K if q2 else Q4_K
        return Q2_K if q2 else Q3_K
    if ftype in ("q4_0", "q5_0", "iq4_nl", "q4_1", "q5_1"):
        # the 32-element formats (llama-quantize's legacy types and the fallbacks it takes for rows that are not a multiple of 256): output Q6_K;
        # IQ4_NL promotes attn_v (grouped-query models) and the first eighth of ffn_down to Q5_K, as upstream does for IQ4_NL / IQ4_XS
        if kind == "output":
            return Q6_K
        if ftype == "iq4_nl" and ((kind == "attn_v" and cfg.n_head // cfg.n_head_kv >= 4) or (kind == "ffn_down" and il < max(1, cfg.n_layer // 8))):
            return Q5_K
        return {"q4_0": Q4_0, "q5_0": Q5_0, "iq4_nl": IQ4_NL, "q4_1": Q4_1, "q5_1": Q5_1}[ftype]
    if ftype == "iq4_xs":
        # upstream's mix for IQ4_XS (the IQ4_NL one above): output Q6_K; attn_v Q5_K with a query / kv head ratio >= 4 and the first eighth of ffn_down
        # Q5_K; a tensor whose rows are not a multiple of 256 falls back to IQ4_NL; everything else IQ4_XS, expert tensors included.  token_embd stays
        # IQ4_XS, tied output too, as for this writer's other ftypes (upstream writes Q6_K there): tiny-qwen3's head then runs on an IQ4_XS tensor
        if kind == "output":
            return Q6_K
        if (kind == "attn_v" and cfg.n_head // cfg.n_head_kv >= 4) or (kind == "ffn_down" and il < max(1, cfg.n_layer // 8)):
            return Q5_K
        return IQ4_NL if _row_len(cfg, kind) % 256 else IQ4_XS
    if ftype in ("tq1_0", "tq2_0"):
        # LLAMA_FTYPE_MOSTLY_TQ1_0 / TQ2_0 as remembered from llama-quantize (unpinned like the fallback table): token_embd Q4_K, output Q6_K, every other 2-D
        # weight the ternary type, expert tensors included; a tensor whose rows are not a multiple of 256 falls back to Q4_0 (by this rule itself, as the
        # IQ4_XS mix does, so tensor_type and the mix agree on the older configs)
        if kind == "token_embd":
            return Q4_K
        if kind == "output":
            return Q6_K
        t = TQ1_0 if ftype == "tq1_0" else TQ2_0
        return FALLBACK_32[t] if _row_len(cfg, kind) % 256 else t
    if ftype in ("q3_k_s", "q3_k_l", "q4_k_s", "q5_k_s", "q6_k"):
        # the other mixes the reference publishes (.github/workflows/convert-model-all-quant.yml:106-152), by llama-quantize's rules for the llama
        # architecture: output Q6_K everywhere; Q3_K_S: everything else Q3_K; Q3_K_L: attn_v, ffn_down, attn_output Q5_K, the rest Q3_K; Q4_K_S: Q4_K
        # with attn_v Q5_K in the first four layers and ffn_down Q5_K in the first n_layer / 8; Q5_K_S: Q5_K; Q6_K: Q6_K
        if kind == "output" or ftype == "q6_k":
            return Q6_K
        if ftype == "q3_k_s":
            return Q3_K
        if ftype == "q3_k_l":
            return Q5_K if kind in ("attn_v", "ffn_down", "attn_output") else Q3_K
        if ftype == "q4_k_s":
            if (kind == "attn_v" and il < 4) or (kind == "ffn_down" and il < max(1, cfg.n_layer // 8)):
                return Q5_K
            return Q4_K
        return Q5_K
    base = {"q4_k_m": Q4_K, "q5_k_m": Q5_K}[ftype]
    if kind == "output":
        return Q6_K
    if kind in ("attn_v", "ffn_down") and use_more_bits(il, cfg.n_layer):
        return Q6_K
    if cfg.n_expert == 8 and kind in ("attn_k", "attn_v"):
        return Q8_0
    if cfg.big_model and kind == "attn_v" and base == Q4_K:
        return Q5_K
    return base


def model_tensors(cfg: LlamaConfig, ftype: str):
    """[(name, ne, type, fan_in)] in file order."""
    E, F, V = cfg.n_embd, cfg.n_ff, cfg.n_vocab
    kv = cfg.n_head_kv * cfg.head_dim
    out = [("token_embd.weight", (E, V), tensor_type(cfg, ftype, "token_embd", 0), None)]
    if cfg.arch == "nomic-bert":
        # encoder: token-type table, LayerNorms with biases, fused Q | K | V; no output head (the reference's embedding smoke model, Makefile:6)
        out.append(("token_types.weight", (E, 2), F32, E))
        out.append(("token_embd_norm.weight", (E,), F32, None))
        out.append(("token_embd_norm.bias", (E,), F32, None))
        for il in range(cfg.n_layer):
            p = f"blk.{il}."
            out.append((p + "attn_qkv.weight", (E, E + 2 * kv), tensor_type(cfg, ftype, "attn_qkv", il), E))
            out.append((p + "attn_output.weight", (E, E), tensor_type(cfg, ftype, "attn_output", il), E))
            out.append((p + "attn_output_norm.weight", (E,), F32, None))
            out.append((p + "attn_output_norm.bias", (E,), F32, None))
            out.append((p + "ffn_up.weight", (E, F), tensor_type(cfg, ftype, "ffn_up", il), E))
            out.append((p + "ffn_gate.weight", (E, F), tensor_type(cfg, ftype, "ffn_gate", il), E))
            out.append((p + "ffn_down.weight", (F, E), tensor_type(cfg, ftype, "ffn_down", il), F))
            out.append((p + "layer_output_norm.weight", (E,), F32, None))
            out.append((p + "layer_output_norm.bias", (E,), F32, None))
        return out
    QW = cfg.n_head * cfg.head_dim                 # attention width: n_embd unless the file sets its own head size
    for il in range(cfg.n_layer):
        p = f"blk.{il}."
        out.append((p + "attn_norm.weight", (E,), F32, None))
        out.append((p + "attn_q.weight", (E, QW), tensor_type(cfg, ftype, "attn_q", il), E))
        out.append((p + "attn_k.weight", (E, kv), tensor_type(cfg, ftype, "attn_k", il), E))
        out.append((p + "attn_v.weight", (E, kv), tensor_type(cfg, ftype, "attn_v", il), E))
        if cfg.qkv_bias:
            out.append((p + "attn_q.bias", (QW,), F32, None))
            out.append((p + "attn_k.bias", (kv,), F32, None))
            out.append((p + "attn_v.bias", (kv,), F32, None))
        if cfg.arch in ("qwen3", "qwen3moe"):
            out.append((p + "attn_q_norm.weight", (cfg.head_dim,), F32, None))
            out.append((p + "attn_k_norm.weight", (cfg.head_dim,), F32, None))
        out.append((p + "attn_output.weight", (QW, E), tensor_type(cfg, ftype, "attn_output", il), QW))
        out.append((p + "ffn_norm.weight", (E,), F32, None))
        if cfg.n_expert:
            X, F = cfg.n_expert, cfg.n_ff_exp or cfg.n_ff
            out.append((p + "ffn_gate_inp.weight", (E, X), F32, E))
            out.append((p + "ffn_gate_exps.weight", (E, F, X), tensor_type(cfg, ftype, "ffn_gate", il), E))
            out.append((p + "ffn_down_exps.weight", (F, E, X), tensor_type(cfg, ftype, "ffn_down", il), F))
            out.append((p + "ffn_up_exps.weight", (E, F, X), tensor_type(cfg, ftype, "ffn_up", il), E))
        else:
            out.append((p + "ffn_gate.weight", (E, F), tensor_type(cfg, ftype, "ffn_gate", il), E))
            out.append((p + "ffn_down.weight", (F, E), tensor_type(cfg, ftype, "ffn_down", il), F))
            out.append((p + "ffn_up.weight", (E, F), tensor_type(cfg, ftype, "ffn_up", il), E))
    out.append(("output_norm.weight", (E,), F32, None))
    if not cfg.tied_output:
        out.append(("output.weight", (E, V), tensor_type(cfg, ftype, "output", 0), E))
    return out


def weight_bytes_per_token(cfg: LlamaConfig, ftype: str) -> int:
    """Algorithmic weight bytes one decoded token reads: every tensor once, one
    token_embd row, and n_expert_used of n_expert experts."""
    total = 0
    for name, ne, t, _ in model_tensors(cfg, ftype):
        n = int(np.prod(ne))
        b = row_bytes(t, ne[0]) * (n // ne[0])
        if name == "token_embd.weight":
            b = row_bytes(t, ne[0]) if not cfg.tied_output else b       # (a tied head reads the whole table)
        elif "_exps." in name:
            b = b // cfg.n_expert * cfg.n_expert_used
        total += b
    return total


def write_synthetic_llama(path: str, cfg: LlamaConfig | str, ftype: str = "q4_k_m", seed: int = 0xC0FFEE,
                          with_vocab: bool = True, gain: float = 1.0, blocks=None) -> int:
    """Write a synthetic llama-arch GGUF; returns the file size in bytes.  blocks (optional): a callable (rng, type, n_elems, std) -> raw bytes that takes
    random_blocks' place for the 2-D weights, e.g. to write a second file whose weights are a coarser rounding of this one's (a draft model for a target)."""
    if isinstance(cfg, str):
        cfg = CONFIGS[cfg]
    w = GGUFWriter()
    a = cfg.arch
    w.add("general.architecture", "str", a)
    w.add("general.name", "str", cfg.name + " (synthetic)")
    w.add("general.file_type", "u32", FTYPE_ID[ftype])
    w.add(f"{a}.context_length", "u32", cfg.n_ctx_train)
    w.add(f"{a}.embedding_length", "u32", cfg.n_embd)
    w.add(f"{a}.block_count", "u32", cfg.n_layer)
    w.add(f"{a}.feed_forward_length", "u32", cfg.n_ff)
    w.add(f"{a}.attention.head_count", "u32", cfg.n_head)
    w.add(f"{a}.attention.head_count_kv", "u32", cfg.n_head_kv)
    if cfg.arch == "nomic-bert":
        w.add(f"{a}.attention.layer_norm_epsilon", "f32", cfg.eps)
        w.add(f"{a}.attention.causal", "bool", False)
        w.add(f"{a}.pooling_type", "u32", 1)
    else:
        w.add(f"{a}.attention.layer_norm_rms_epsilon", "f32", cfg.eps)
    w.add(f"{a}.rope.dimension_count", "u32", cfg.head_dim)
    if cfg.n_head_dim:
        w.add(f"{a}.attention.key_length", "u32", cfg.head_dim)
        w.add(f"{a}.attention.value_length", "u32", cfg.head_dim)
    w.add(f"{a}.rope.freq_base", "f32", cfg.rope_base)
    w.add(f"{a}.vocab_size", "u32", cfg.n_vocab)
    if cfg.n_expert:
        w.add(f"{a}.expert_count", "u32", cfg.n_expert)
        w.add(f"{a}.expert_used_count", "u32", cfg.n_expert_used)
    if cfg.n_ff_exp:
        w.add(f"{a}.expert_feed_forward_length", "u32", cfg.n_ff_exp)
    for k, v in cfg.extra.items():                 # e.g. {"pooling_type": 1, "rope.scaling.type": "yarn", "rope.scaling.factor": 4.0}: extra keys under the architecture prefix
        w.add(f"{a}.{k}", "str" if isinstance(v, str) else "f32" if isinstance(v, float) else "u32", v)
    if with_vocab and cfg.arch == "nomic-bert":
        # synthetic WordPiece vocabulary in the GGUF convention (word-initial pieces carry the U+2581 prefix, continuations are bare): the five BERT specials,
        # letters / digits / punctuation in both roles, then generated multi-letter pieces
        toks, types = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"], [3, 3, 3, 3, 3]
        alphabet = "abcdefghijklmnopqrstuvwxyz0123456789"
        for ch in alphabet + ".,!?'-":
            toks += ["\u2581" + ch, ch]
            types += [1, 1]
        i = 0
        while len(toks) < cfg.n_vocab:
            s, k = "", i + 36
            while True:
                s = alphabet[k % 26] + s
                k //= 26
                if k == 0:
                    break
            piece = ("\u2581" + s) if i % 2 == 0 else s
            if piece not in toks[:100] and len(s) > 1:
                toks.append(piece)
                types.append(1)
            i += 1
        w.add("tokenizer.ggml.model", "str", "bert")
        w.add_array("tokenizer.ggml.tokens", "str", toks[: cfg.n_vocab])
        w.add_array("tokenizer.ggml.token_type", "i32", types[: cfg.n_vocab])
        w.add("tokenizer.ggml.token_type_count", "u32", 2)
        w.add("tokenizer.ggml.unknown_token_id", "u32", 1)
        w.add("tokenizer.ggml.seperator_token_id", "u32", 3)
        w.add("tokenizer.ggml.padding_token_id", "u32", 0)
        w.add("tokenizer.ggml.cls_token_id", "u32", 2)
        w.add("tokenizer.ggml.mask_token_id", "u32", 4)
        w.add("tokenizer.ggml.bos_token_id", "u32", 2)
        w.add("tokenizer.ggml.eos_token_id", "u32", 3)
    elif with_vocab:
        # synthetic SentencePiece-style vocab: <unk>,<s>,</s>, 256 byte tokens, then printable pieces
        toks, scores, types = ["<unk>", "<s>", "</s>"], [0.0, 0.0, 0.0], [2, 3, 3]
        for b in range(256):
            toks.append(f"<0x{b:02X}>")
            scores.append(0.0)
            types.append(6)
        alphabet = "abcdefghijklmnopqrstuvwxyz"
        for piece in ["▁"] + list(alphabet):
            toks.append(piece)
            scores.append(-1000.0)
            types.append(1)
        i = 26
        while len(toks) < cfg.n_vocab:
            s, k = "", i
            while True:
                s = alphabet[k % 26] + s
                k //= 26
                if k == 0:
                    break
            toks.append(("▁" + s) if i % 2 == 0 else s)
            scores.append(-float(len(toks)))
            types.append(1)
            i += 1
        w.add("tokenizer.ggml.model", "str", "llama")
        w.add_array("tokenizer.ggml.tokens", "str", toks[: cfg.n_vocab])
        w.add_array("tokenizer.ggml.scores", "f32", scores[: cfg.n_vocab])
        w.add_array("tokenizer.ggml.token_type", "i32", types[: cfg.n_vocab])
        w.add("tokenizer.ggml.bos_token_id", "u32", 1)
        w.add("tokenizer.ggml.eos_token_id", "u32", 2)
        w.add("tokenizer.ggml.unknown_token_id", "u32", 0)
        w.add("tokenizer.ggml.add_bos_token", "bool", True)
        w.add("tokenizer.ggml.add_eos_token", "bool", False)

    for idx, (name, ne, t, fan_in) in enumerate(model_tensors(cfg, ftype)):
        n = int(np.prod(ne))

        def gen(idx=idx, name=name, ne=ne, t=t, fan_in=fan_in, n=n):
            rng = np.random.default_rng([seed, idx])
            if name.endswith(".bias"):
                return (rng.standard_normal(n) * 0.25).astype("<f4").view(np.uint8)
            if name.endswith("_q_norm.weight") or name.endswith("_k_norm.weight"):
                # a wide band: a skipped weight multiply, a norm over the wrong span or after the rope lands far outside every tolerance
                return rng.uniform(0.25, 2.0, size=n).astype("<f4").view(np.uint8)
            if len(ne) == 1:  # norm weights
                return rng.uniform(0.9, 1.1, size=n).astype("<f4").view(np.uint8)
            draw = blocks or random_blocks
            if name == "token_embd.weight":
                return draw(rng, t, n, 1.0)
            return draw(rng, t, n, gain / np.sqrt(fan_in))

        w.add_tensor(name, ne, t, gen)
    return w.write(path)


# ---------------------------------------------------------------- LoRA adapter files (convert_lora_to_gguf.py output)
LORA_KINDS = ("attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down")


def lora_pairs(cfg: LlamaConfig, rank: int, targets):
    """[(base tensor name, K, N)] of an adapter on `targets`: kinds ("attn_q" ... "ffn_down": that tensor of every layer; "output": output.weight, the
    embedding table's shape when the config ties them) or whole tensor names ("blk.1.attn_v.weight"), in the order given, layers innermost."""
    shapes = {name: ne for name, ne, _, _ in model_tensors(cfg, "f16") if len(ne) >= 2}
    shapes.setdefault("output.weight", shapes["token_embd.weight"])
    out = []
    for tgt in targets:
        names = [f"blk.{il}.{tgt}.weight" for il in range(cfg.n_layer)] if tgt in LORA_KINDS else ["output.weight"] if tgt == "output" else [tgt]
        for name in names:
            out.append((name, shapes[name][0], shapes[name][1]))
    return out


def write_synthetic_lora(path: str, cfg: LlamaConfig | str, rank: int = 8, alpha: float = 16.0, targets=("attn_q", "attn_v"), dtype: str = "f16",
                         seed: int = 0x10A, std: float = 0.05) -> int:
    """Write a llama.cpp-shaped LoRA adapter for a synthetic base: general.type "adapter", adapter.type "lora", adapter.lora.alpha and, per target, the pair
    <name>.lora_a (ne [K, rank], std 1 / sqrt(K)) and <name>.lora_b (ne [rank, N], std `std`), both `dtype` ("f16" / "f32").  With an activation of unit
    scale the delta is about alpha / rank * std * sqrt(rank) of the base tensor's own product.  Returns the file size in bytes."""
    if isinstance(cfg, str):
        cfg = CONFIGS[cfg]
    t = {"f16": F16, "f32": F32}[dtype]
    w = GGUFWriter()
    w.add("general.architecture", "str", cfg.arch)
    w.add("general.type", "str", "adapter")
    w.add("general.name", "str", cfg.name + " adapter (synthetic)")
    w.add("adapter.type", "str", "lora")
    w.add("adapter.lora.alpha", "f32", float(alpha))
    for idx, (name, K, N) in enumerate(lora_pairs(cfg, rank, targets)):
        for half, ne, sd in ((".lora_a", (K, rank), 1.0 / np.sqrt(K)), (".lora_b", (rank, N), std)):
            def gen(idx=idx, half=half, ne=ne, sd=sd):
                rng = np.random.default_rng([seed, idx, half == ".lora_b"])
                return random_blocks(rng, t, int(np.prod(ne)), sd)

            w.add_tensor(name + half, ne, t, gen)
    return w.write(path)


# ---------------------------------------------------------------- LLaVA projector files ("mmproj": general.architecture clip)
@dataclass
class ClipConfig:
    """The vision tower + projector of a LLaVA-1.5 style mmproj file as llama.cpp's convert_image_encoder_to_gguf.py writes it: CLIP ViT (pre-LN, learned position
    embeddings, class token, quick-GELU MLP) cut after its second-to-last layer (block_count = layers - 1), and the two-layer MLP projector mm.0 / mm.2.
    clip.cpp then runs block_count - 1 of the file's blocks for a LLaVA projector (get_deepest_feature_layer): the file's last block is dead weight."""
    name: str
    image_size: int
    patch_size: int
    n_embd: int          # vision hidden size
    n_head: int
    n_ff: int
    n_layer: int         # blocks in the file
    proj_dim: int        # the language model's n_embd
    eps: float = 1e-5
    use_gelu: bool = False
    mean: tuple = (0.48145466, 0.4578275, 0.40821073)
    std: tuple = (0.26862954, 0.26130258, 0.27577711)
    # LLaVA-1.6: the (width, height) canvases of the image grid, flattened, and the merge type that turns the grid on
    pinpoints: tuple = ()
    merge_type: str = ""

    @property
    def n_patches(self) -> int:
        return (self.image_size // self.patch_size) ** 2


CLIP_CONFIGS = {
    # ViT-L/14-336 as LLaVA-1.5-7B uses it (576 patches -> 576 rows of 4096)
    "clip-vit-l-336": ClipConfig("clip-vit-large-patch14-336", 336, 14, 1024, 16, 4096, 23, 4096),
    # the same graph at test size: 56 x 56 pixels = 16 patches of 14 x 14, head_dim 64 like the real tower (d128: 36 patches, 4 heads, 3 blocks)
    "tiny-clip": ClipConfig("tiny-clip", 56, 14, 128, 2, 256, 3, 256),
    "tiny-clip-d128": ClipConfig("tiny-clip-d128", 84, 14, 256, 4, 512, 4, 512),
    # head size 128 at the real tower's 577 rows (the tiled attention's largest LDS footprint: 157 KB)
    "clip-d128-336": ClipConfig("clip-d128-336", 336, 14, 256, 2, 512, 2, 256),
    "tiny-clip-gelu": ClipConfig("tiny-clip-gelu", 56, 14, 128, 2, 256, 3, 4096, use_gelu=True),
    # a projector as wide as the tiny language models of the engine tests (n_embd 1024): 16 rows per image
    "tiny-clip-1024": ClipConfig("tiny-clip-1024", 56, 14, 128, 2, 256, 3, 1024),
    # LLaVA-1.6: ViT-L/14-336 with the image grid of llava-v1.6 (an overview + up to four tiles: 2880 rows a picture), and the same at test size
    "clip-vit-l-336-grid": ClipConfig("llava-v1.6-clip", 336, 14, 1024, 16, 4096, 23, 4096, pinpoints=(336, 672, 672, 336, 672, 672, 1008, 336, 336, 1008),
                                      merge_type="spatial_unpad"),
    "tiny-clip-grid": ClipConfig("tiny-clip-grid", 56, 14, 128, 2, 256, 3, 256, pinpoints=(56, 112, 112, 56, 112, 112, 168, 56, 56, 168), merge_type="spatial_unpad"),
    "tiny-clip-grid-1024": ClipConfig("tiny-clip-grid-1024", 56, 14, 128, 2, 256, 3, 1024, pinpoints=(56, 112, 112, 56, 112, 112, 168, 56, 56, 168),
                                      merge_type="spatial_unpad"),
    # a grid in the file but the merge type "flat": only the overview is encoded
    "tiny-clip-grid-flat": ClipConfig("tiny-clip-grid-flat", 56, 14, 128, 2, 256, 3, 256, pinpoints=(56, 112, 112, 56, 112, 112), merge_type="flat"),
}


def clip_tensors(cfg: ClipConfig):
    """(name, ne, type, fan_in); ne in ggml order (fastest dimension first).  The feed-forward names are the converter's: `ffn_down` is the FIRST projection
    (n_embd -> n_ff) and `ffn_up` the second - clip.cpp reads them that way round."""
    E, FF, P = cfg.n_embd, cfg.n_ff, cfg.patch_size
    out = [("v.class_embd", (E,), F32, 1),
           ("v.patch_embd.weight", (P, P, 3, E), F16, 3 * P * P),
           ("v.position_embd.weight", (E, cfg.n_patches + 1), F16, 1),
           ("v.pre_ln.weight", (E,), F32, 1), ("v.pre_ln.bias", (E,), F32, 1)]
    for il in range(cfg.n_layer):
        p = f"v.blk.{il}."
        for nm in ("attn_q", "attn_k", "attn_v", "attn_out"):
            out += [(p + nm + ".weight", (E, E), F16, E), (p + nm + ".bias", (E,), F32, 1)]
        out += [(p + "ln1.weight", (E,), F32, 1), (p + "ln1.bias", (E,), F32, 1)]
        out += [(p + "ffn_down.weight", (E, FF), F16, E), (p + "ffn_down.bias", (FF,), F32, 1)]
        out += [(p + "ffn_up.weight", (FF, E), F16, FF), (p + "ffn_up.bias", (E,), F32, 1)]
        out += [(p + "ln2.weight", (E,), F32, 1), (p + "ln2.bias", (E,), F32, 1)]
    out += [("mm.0.weight", (E, cfg.proj_dim), F16, E), ("mm.0.bias", (cfg.proj_dim,), F32, 1),
            ("mm.2.weight", (cfg.proj_dim, cfg.proj_dim), F16, cfg.proj_dim), ("mm.2.bias", (cfg.proj_dim,), F32, 1)]
    if cfg.pinpoints:      # LLaVA-1.6 files carry the row separator of the original model; llama.cpp's layout ("without newline tokens") never reads it
        out += [("model.image_newline", (cfg.proj_dim,), F32, 1)]
    return out


def write_synthetic_clip(path: str, cfg: ClipConfig | str, seed: int = 0xC11F) -> int:
    """A random-weight mmproj file of the given geometry (same container, keys and tensor names as a converted LLaVA-1.5 projector)."""
    if isinstance(cfg, str):
        cfg = CLIP_CONFIGS[cfg]
    w = GGUFWriter()
    w.add("general.architecture", "str", "clip")
    w.add("general.name", "str", cfg.name)
    w.add("general.file_type", "u32", 1)
    w.add("clip.has_text_encoder", "bool", False)
    w.add("clip.has_vision_encoder", "bool", True)
    w.add("clip.has_llava_projector", "bool", True)
    w.add("clip.projector_type", "str", "mlp")
    w.add("clip.use_gelu", "bool", cfg.use_gelu)
    w.add("clip.vision.image_size", "u32", cfg.image_size)
    w.add("clip.vision.patch_size", "u32", cfg.patch_size)
    w.add("clip.vision.embedding_length", "u32", cfg.n_embd)
    w.add("clip.vision.feed_forward_length", "u32", cfg.n_ff)
    w.add("clip.vision.projection_dim", "u32", cfg.proj_dim)
    w.add("clip.vision.attention.head_count", "u32", cfg.n_head)
    w.add("clip.vision.attention.layer_norm_epsilon", "f32", cfg.eps)
    w.add("clip.vision.block_count", "u32", cfg.n_layer)
    w.add_array("clip.vision.image_mean", "f32", list(cfg.mean))
    w.add_array("clip.vision.image_std", "f32", list(cfg.std))
    if cfg.pinpoints:
        w.add_array("clip.vision.image_grid_pinpoints", "i32", list(cfg.pinpoints))
    if cfg.merge_type:
        w.add("clip.vision.mm_patch_merge_type", "str", cfg.merge_type)
    for idx, (name, ne, t, fan_in) in enumerate(clip_tensors(cfg)):
        n = int(np.prod(ne))

        def gen(idx=idx, name=name, ne=ne, t=t, fan_in=fan_in, n=n):
            rng = np.random.default_rng([seed, idx])
            if name.endswith(".bias"):
                return (rng.standard_normal(n) * 0.1).astype("<f4").view(np.uint8)
            if name in ("v.class_embd",):
                return (rng.standard_normal(n) * 0.5).astype("<f4").view(np.uint8)
            if len(ne) == 1:      # LayerNorm weights
                return rng.uniform(0.9, 1.1, size=n).astype("<f4").view(np.uint8)
            if name == "v.position_embd.weight":
                return (rng.standard_normal(n) * 0.3).astype("<f2").view(np.uint8)
            return (rng.standard_normal(n) * (1.4 / np.sqrt(fan_in))).astype("<f2").view(np.uint8)

        w.add_tensor(name, ne, t, gen)
    return w.write(path)
