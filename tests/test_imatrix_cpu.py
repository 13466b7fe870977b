"""The importance matrix without a GPU: the reference collector of tests/imatrix_ref.py against plain numpy for one projection, and the two file formats of
tools/imatrix.py - round trips, the GGUF form through tests/gguf_read.py, the legacy values, the --in-file merge and its refusals."""
import importlib.util
import os
import struct

import numpy as np
import pytest

import imatrix_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("imatrix_tool", os.path.join(ROOT, "tools", "imatrix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_reference_collector_against_plain_numpy(pkg, tmp_models):
    """blk.0.attn_q.weight of `tiny` by hand: its input rows are RMSNorm(embedding row) * attn_norm, so the entry is the column sum of their squares; the
    entries that share an input are equal; every count is the number of tokens, the head's the number of flagged rows."""
    import oracle_py as oq
    from gguf_read import read_gguf
    from imatrix_ref import ImatrixRef
    path = ic.model_file(pkg, tmp_models, "tiny", "q4_k_m")
    toks, flags = ic.prompt_tokens(512, 12), ic.head_flags(12)
    ref = ImatrixRef(path, 64, ic.KV["q8_0"], ic.KV["q8_0"])
    ref.decode(toks, np.arange(12), want=flags)
    kv, t = read_gguf(path)
    ne, ty, raw = t["token_embd.weight"]
    rb = oq.row_bytes(ty, ne[0])
    x = np.stack([oq.dequantize(ty, raw[int(k) * rb:(int(k) + 1) * rb], ne[0]) for k in toks]).astype(np.float64)
    h = x / np.sqrt((x * x).mean(axis=1, keepdims=True) + kv["llama.attention.layer_norm_rms_epsilon"]) * t["blk.0.attn_norm.weight"][2].view("<f4")
    by_hand = (h * h).sum(axis=0)
    got, cnt = ref.im["blk.0.attn_q.weight"]
    assert got.shape == (1, 256) and cnt.tolist() == [12]
    assert np.abs(got[0] - by_hand).max() <= 1e-5 * by_hand.max()
    for a, b in (("attn_q", "attn_k"), ("attn_q", "attn_v"), ("ffn_gate", "ffn_up")):
        assert np.array_equal(ref.im[f"blk.1.{a}.weight"][0], ref.im[f"blk.1.{b}.weight"][0])
    want = ic.expected_names(path, True)
    assert set(ref.im) == set(want)
    for name, (s, c) in ref.im.items():
        assert s.shape == (want[name][1], want[name][0]), name
        assert c.tolist() == [int(flags.sum()) if name == "output.weight" else 12], name


def sample(tool, seed=0, n_chunks=3):
    rng = np.random.default_rng(seed)
    counts = np.array([5, 0, 192 - 5 - 7, 7], np.float32)
    sum2 = rng.random((4, 64)).astype(np.float32) * counts[:, None]
    return tool.IMatrix({"blk.0.attn_q.weight": (rng.random((1, 96)).astype(np.float32) * 192, np.array([192], np.float32)),
                         "blk.0.ffn_down_exps.weight": (sum2, counts)}, ["calib.txt"], n_chunks, 64)


def test_gguf_form_round_trips_and_reads_with_the_test_reader(tool, tmp_path):
    from gguf_read import read_gguf
    im = sample(tool)
    p = str(tmp_path / "a.gguf")
    tool.write_imatrix(p, im)
    back = tool.read_imatrix(p)
    assert list(back.entries) == list(im.entries) and back.datasets == ["calib.txt"] and (back.chunk_count, back.chunk_size) == (3, 64)
    for k, (s, c) in im.entries.items():
        assert back.entries[k][0].tobytes() == s.tobytes() and back.entries[k][1].tobytes() == c.tobytes()
    kv, t = read_gguf(p)
    assert kv["general.type"] == "imatrix" and kv["imatrix.datasets"] == ["calib.txt"] and kv["imatrix.chunk_count"] == 3 and kv["imatrix.chunk_size"] == 64
    assert sorted(t) == sorted(k + sfx for k in im.entries for sfx in (".in_sum2", ".counts"))
    ne, ty, raw = t["blk.0.ffn_down_exps.weight.in_sum2"]
    assert ne == (64, 4) and ty == 0
    assert raw[:4 * 64 * 4].view("<f4").reshape(4, 64).tobytes() == im.entries["blk.0.ffn_down_exps.weight"][0].tobytes()
    ne, ty, raw = t["blk.0.ffn_down_exps.weight.counts"]
    assert ne == (1, 4) and ty == 0 and raw[:16].view("<f4").tolist() == [5, 0, 180, 7]


def test_dat_form_values_and_round_trip(tool, tmp_path):
    """The legacy file holds sum2 / count * ncall, expert-major; a never-routed expert's columns are the flat ncall; the reader hands the values back as sums
    with ncall as the count."""
    im = sample(tool)
    p = str(tmp_path / "a.dat")
    tool.write_imatrix(p, im)
    buf = open(p, "rb").read()
    assert struct.unpack_from("<i", buf, 0)[0] == 2
    back = tool.read_imatrix(p)
    assert back.flat and list(back.entries) == list(im.entries) and back.chunk_count == 3 and back.datasets == ["calib.txt"]
    s, c = im.entries["blk.0.ffn_down_exps.weight"]
    want = np.where(c[:, None] > 0, s.astype(np.float64) / np.maximum(c[:, None], 1) * 3, 3.0).astype(np.float32).reshape(-1)
    v, n = back.entries["blk.0.ffn_down_exps.weight"]
    assert v.shape == (1, 256) and n.tolist() == [3] and v.reshape(-1).tobytes() == want.tobytes()
    assert (v.reshape(4, 64)[1] == 3.0).all()
    v, n = back.entries["blk.0.attn_q.weight"]
    assert np.array_equal(v[0], (im.entries["blk.0.attn_q.weight"][0][0].astype(np.float64) / 192 * 3).astype(np.float32))
    assert buf.endswith(struct.pack("<i", 3) + struct.pack("<i", 9) + b"calib.txt")


def test_in_file_merge_and_refusals(tool, tmp_path):
    a, b = sample(tool, 1, 3), sample(tool, 2, 5)
    pa, pb = str(tmp_path / "a.gguf"), str(tmp_path / "b.gguf")
    tool.write_imatrix(pa, a)
    tool.write_imatrix(pb, b)
    m = tool.read_imatrix(pa)
    m.add(tool.read_imatrix(pb), pb)
    assert m.chunk_count == 8
    for k in a.entries:
        assert np.array_equal(m.entries[k][0], (a.entries[k][0].astype(np.float64) + b.entries[k][0]).astype(np.float32))
        assert np.array_equal(m.entries[k][1], a.entries[k][1] + b.entries[k][1])
    other = tool.IMatrix({"blk.0.attn_q.weight": a.entries["blk.0.attn_q.weight"]}, ["x"], 1, 64)
    with pytest.raises(ValueError, match="same entries"):
        tool.read_imatrix(pa).add(other, "other")
    wide = sample(tool)
    wide.entries["blk.0.attn_q.weight"] = (np.zeros((1, 128), np.float32), np.array([1], np.float32))
    with pytest.raises(ValueError, match="blk.0.attn_q.weight"):
        tool.read_imatrix(pa).add(wide, "wide")
    # a legacy file merges by value count: its one count goes to every expert
    pd = str(tmp_path / "a.dat")
    tool.write_imatrix(pd, a)
    m = tool.read_imatrix(pa)
    m.add(tool.read_imatrix(pd), pd)
    assert np.array_equal(m.entries["blk.0.ffn_down_exps.weight"][1], a.entries["blk.0.ffn_down_exps.weight"][1] + 3)
