"""csrc/quantize.hip's TQ1_0 / TQ2_0 branches through Backend.quantize_rows: the bytes of tests/ternary_quantize_ref.py from F32, F16 and BF16 rows that hold
every edge (test_ternary_quantize_cpu.edge_rows), ternary rows back exactly through Backend.dequantize_rows, the refusals, and tools/quantize.py's two ternary
mixes on the device: planned types, a file that loads, the reference's greedy tokens.  Every comparison is of bytes or tokens: there is no tolerance."""
import os
import re

import numpy as np
import pytest

import ternary_quantize_ref as tqr
from test_gpu_quantize_tool import run_tool
from test_gpu_tq import GREEDY, _greedy_ref
from test_ternary_quantize_cpu import TYPES, as_source, edge_rows, ternary_rows

pytestmark = pytest.mark.gpu

ERR_ARG = -103            # MI355_ERR_ARG
SRC = {"f32": tqr.F32, "f16": tqr.F16, "bf16": tqr.BF16}


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


@pytest.mark.parametrize("shape", [(1, 256), (3, 768)], ids=["1x256", "3x768"])
@pytest.mark.parametrize("st", list(SRC))
@pytest.mark.parametrize("t", TYPES)
def test_bytes_equal_the_twin(be, t, st, shape):
    """3 x 768: nine chunks over four waves, the last workgroup ragged; 1 x 256: block 1 of those rows (patterns, ties, a negative extreme) alone"""
    x = edge_rows() if shape == (3, 768) else edge_rows().reshape(9, 256)[1:2]
    s = as_source(x, SRC[st])
    got = be.quantize_rows(t, s, src_type=SRC[st])
    want = tqr.quantize_rows(t, s, src_type=SRC[st])
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:8]


@pytest.mark.parametrize("t", TYPES)
def test_round_trip_is_exact(be, t):
    x = ternary_rows(5, 1024)
    assert np.array_equal(be.dequantize_rows(be.quantize_rows(t, x), t, 1024), x)


def test_other_behaviour(be, pkg):
    lib = be.lib
    assert lib.mi355_quantize_supported(tqr.TQ1_0) == lib.mi355_quantize_supported(tqr.TQ2_0) == 1
    x = edge_rows()
    for t in (tqr.TQ1_0, tqr.TQ2_0):
        assert np.array_equal(be.quantize_rows(t, x, np.linspace(0.0, 9.0, 768, dtype=np.float32)), be.quantize_rows(t, x))
        bad = x.copy()
        bad[2, 300] = np.nan
        with pytest.raises(pkg.MI355Error, match="row 2"):
            be.quantize_rows(t, bad)
        out = np.zeros(66, np.uint8)
        assert lib.mi355_quantize_chunk(t, 0, x.ctypes.data, 288, 1, None, out.ctypes.data) == ERR_ARG
        assert "n_per_row" in (lib.mi355_last_error() or b"").decode() and not out.any()


def test_the_tool_writes_ternary_files_that_run(pkg, tmp_models, tmp_path):
    """tiny as F16 -> tq2_0, and -> tq1_0 under --pure (a ternary token_embd and head too): the planned types, and /v1/chat/completions returns the greedy
    tokens of tests/tq_ref.py's model of the written file - the comparison of test_gpu_tq.py's engine test"""
    from gguf_read import read_gguf
    gs = pkg.gguf_synth
    pkg.Backend()
    # The seed, chosen on the CPU with the twin's files as test_gpu_tq.py chooses its own: no seed from 3 to 59 keeps the reference's top-two logit gap above
    # 2 * FLIP_TOL * max(1, max |logit|) at all nine steps of both files; 39 has the widest smallest gap (0.50 x that bar for tq2_0, 0.39 x for tq1_0), no
    # end-of-sequence token and no "u:" in either text, so the comparison below is made for both.
    src = os.path.join(str(tmp_models), "tiny.f16.vocab.gguf")
    gs.write_synthetic_llama(src, "tiny", "f16", seed=39, with_vocab=True)
    for args, ftype in (((), "tq2_0"), (("--pure",), "tq1_0")):
        dst = str(tmp_path / f"tiny-{ftype}.gguf")
        r = run_tool(*args, src, dst, ftype)
        assert r.returncode == 0, r.stdout + r.stderr
        kv, tensors = read_gguf(dst)
        assert kv["general.file_type"] == gs.FTYPE_ID[ftype]
        base = gs.TQ1_0 if ftype == "tq1_0" else gs.TQ2_0
        want = {name: base if args else ty for name, _, ty, _ in gs.model_tensors(gs.CONFIGS["tiny"], ftype)}
        for name, (ne, ty, _) in tensors.items():
            assert len(ne) < 2 or ty == want[name], (name, ty)
        assert tensors["blk.0.attn_q.weight"][1] == base and tensors["token_embd.weight"][1] == (base if args else gs.Q4_K)
        e = pkg.Engine()
        try:
            st, body = e.load_model(llama_model_path=dst, ctx_len=256, n_parallel=1, ngl=100, user_prompt="u:", ai_prompt="a:", system_prompt="s:")
            assert st["status_code"] == 200 and not st["has_error"], (st, body)
            msgs = [{"role": "system", "content": "be brief"}, {"role": "user", "content": "hello world"}]
            st, body = e.chat_completion(model=os.path.splitext(os.path.basename(dst))[0], messages=msgs, max_tokens=8, **GREEDY)[-1]
            assert st["status_code"] == 200 and not st["has_error"], (st, body)
            content = body["choices"][0]["message"]["content"]
        finally:
            e.close()
        want_text = _greedy_ref(dst, pkg, "s:be briefu:hello worlda:", 8)
        # (byte tokens that are no UTF-8: the engine replaces each byte, Python's decoder a truncated sequence as one - runs of U+FFFD count once)
        content, want_text = re.sub("\ufffd+", "\ufffd", content), re.sub("\ufffd+", "\ufffd", want_text)
        assert "u:" not in want_text and content in (want_text.lstrip(" "), want_text), (ftype, content, want_text)
