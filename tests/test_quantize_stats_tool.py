"""tools/quantize_stats.py: on the tiny model as F16 the JSON of `--type q4_k --type q8_0` equals, within quant_error_ref.margin, what the numpy quantiser twin
and the float64 reference give; `--quantized` reads a file tools/quantize.py wrote; what cannot be compared is refused by name before a device is asked for."""
import importlib.util
import json
import os

import numpy as np
import pytest

import quant_error_ref as qe
import quantize_ref as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("quantize_stats_tool", os.path.join(ROOT, "tools", "quantize_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def f16(pkg, tmp_models):
    path = os.path.join(str(tmp_models), "tiny.f16.stats.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny", "f16")
    return path


@pytest.mark.gpu
def test_json_equals_the_twin_and_the_reference(tool, f16, tmp_path):
    out = str(tmp_path / "stats.json")
    assert tool.main(["-m", f16, "--type", "q4_k", "--type", "q8_0", "--json", out]) == 0
    got = {(f["name"], f["type"]): f for f in json.load(open(out))["tensors"]}
    tensors = [(name, ne, data) for name, ne, _, data in tool.qt.read_gguf(f16)[1] if len(ne) == 2 and name.endswith(".weight") and not name.endswith(tool.qt.COPIED)]
    assert len(got) == 2 * len(tensors) > 0
    for name, ne, data in tensors:
        x = data[:2 * ne[0] * ne[1]].view(np.float16).reshape(ne[1], ne[0])
        w = x.astype(np.float32)
        for label, t in (("q4_K", qr.Q4_K), ("q8_0", qr.Q8_0)):
            y = qe.decode(t, qr.quantize_rows(t, x, src_type=qr.F16), ne[0])
            want, (spread, margin) = qe.errors(w, y).sum(axis=0), qe.margin(w, y)
            f = got[name, label]
            print(f"{name} {label}: rel rms {f['rel_rms']:.6f}, reference {np.sqrt(want[0] / want[1]):.6f}, margin {margin:.2e}")
            assert abs(f["sum_e2"] - want[0]) <= margin * want[0] and abs(f["sum_w2"] - want[1]) <= margin * want[1], (name, label)
            assert f["rel_rms"] == pytest.approx(np.sqrt(want[0] / want[1]), rel=margin) and f["weighted_rel"] == f["rel_rms"]
            assert f["max_abs"] == qe.errors(w, y)[:, 3].max()


@pytest.mark.gpu
def test_quantized_file_of_the_quantiser(pkg, tool, f16, tmp_path):
    q, out = str(tmp_path / "tiny.q4_k_m.gguf"), str(tmp_path / "stats.json")
    assert tool.qt.main([f16, q, "q4_k_m"]) == 0
    assert tool.main(["-m", f16, "--quantized", q, "--json", out]) == 0
    res = json.load(open(out))
    types = {f["name"]: f["type"] for f in res["tensors"]}
    assert types["token_embd.weight"] == "q4_K" and "q6_K" in types.values() and all(0 < f["rel_rms"] < 0.2 for f in res["tensors"])
    assert set(res["types"]) == set(types.values()) and all(len(s["worst"]) <= 10 for s in res["types"].values())


def test_refusals_come_before_the_device(pkg, tool, f16, tmp_models, capsys):
    """(without a GPU a Backend cannot be made: a return of 2 with these messages says the plan refused first)"""
    other = os.path.join(str(tmp_models), "tiny-w576.q8_0.stats.gguf")
    pkg.gguf_synth.write_synthetic_llama(other, "tiny-w576-2l", "q8_0")
    for argv, word in ((["-m", f16, "--quantized", other], f" in {f16}, "), (["-m", f16, "--include-layers", "attn_norm"], "1-D tensor"),
                       (["-m", f16, "--include-layers", "attn_q", "--quantized", other, "--type", "q8_0"], "exclude each other"),
                       (["-m", f16, "--type", "q8_k"], "--type q8_k"), (["-m", f16, "--type", "q4_0"], "does not write q4_0"),
                       (["-m", other, "--include-layers", r"blk\.1\.attn_q", "--quantized", f16], "not F32, F16 or BF16")):
        assert tool.main(argv) == 2
        assert word in capsys.readouterr().err, argv
