"""tools/quantize.py in child processes on the device: `tiny` as F16 to q8_0, q4_k_m and q2_k, and `tiny-moe` as F16 to q4_k_m with an importance matrix
written by tools/imatrix.py's writer.  Per-tensor types and metadata as test_quantize_cpu.py checks them for the twin; every output loads with pkg.Model;
the KL divergence of the outputs' logits against the F16 file's over 40 tokens is ordered q8_0 < q4_k_m < q2_k; the importance-matrix keys are written."""
import os
import subprocess
import sys

import numpy as np
import pytest

import quantize_cases as qc  # noqa: F401  (puts tests/ helpers on the path the same way the CPU file does)
from test_quantize_cpu import check_file, random_imatrix

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q8 = 8


@pytest.fixture(scope="module")
def tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("quantize_tool", os.path.join(ROOT, "tools", "quantize.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def f16_file(pkg, tmp_models, cfg):
    p = os.path.join(str(tmp_models), f"{cfg}.f16.gguf")
    if not os.path.exists(p):
        pkg.gguf_synth.write_synthetic_llama(p, cfg, "f16")
    return p


def run_tool(*args):
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tools", "quantize.py"), *args]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_tiny_to_three_mixes_and_their_kl_order(pkg, tool, tmp_models, tmp_path):
    pkg.Backend()
    src = f16_file(pkg, tmp_models, "tiny")
    toks = np.random.default_rng(3).integers(0, 512, 40).astype(np.int32)
    mb = pkg.Model(src)
    cb = pkg.Context(mb, n_ctx=64, n_ubatch=64, type_k=Q8, type_v=Q8, logits_to_host=False)
    assert cb.decode(toks, np.arange(40), logits=[1] * 40) == 0
    kl = {}
    for ftype in ("q8_0", "q4_k_m", "q2_k"):
        dst = str(tmp_path / f"tiny.{ftype}.gguf")
        r = run_tool(src, dst, ftype)
        assert r.returncode == 0, r.stdout + r.stderr
        n_tensors = len(pkg.gguf_synth.model_tensors(pkg.gguf_synth.CONFIGS["tiny"], ftype))
        assert len(r.stdout.strip().splitlines()) == n_tensors + 1 and "quantised size" in r.stdout
        check_file(pkg, tool, src, dst, "tiny", ftype)
        m = pkg.Model(dst)
        c = pkg.Context(m, n_ctx=64, n_ubatch=64, type_k=Q8, type_v=Q8, logits_to_host=False)
        assert c.decode(toks, np.arange(40), logits=[1] * 40) == 0
        k, _ = c.logits_kl(cb, np.arange(40), np.arange(40))
        assert np.isfinite(k).all()
        kl[ftype] = float(k.astype(np.float64).mean())
        c.close(); m.close()
    cb.close(); mb.close()
    print(kl)
    assert 0 <= kl["q8_0"] < kl["q4_k_m"] < kl["q2_k"], kl


def test_moe_with_an_imatrix_file(pkg, tool, tmp_models, tmp_path):
    from gguf_read import read_gguf
    pkg.Backend()
    src = f16_file(pkg, tmp_models, "tiny-moe")
    imp = str(tmp_path / "im.gguf")
    tool.imx.write_imatrix(imp, random_imatrix(pkg, tool, src))
    dst, plain = str(tmp_path / "moe.q4_k_m.gguf"), str(tmp_path / "moe.plain.gguf")
    r = run_tool("--imatrix", imp, src, dst, "q4_k_m")
    assert r.returncode == 0, r.stdout + r.stderr
    kv, t = check_file(pkg, tool, src, dst, "tiny-moe", "q4_k_m", with_imatrix=True)
    assert kv["quantize.imatrix.file"] == imp and kv["quantize.imatrix.dataset"] == "calib.txt"
    assert kv["quantize.imatrix.entries_count"] == len(tool.imx.read_imatrix(imp).entries) and kv["quantize.imatrix.chunks_count"] == 7
    r = run_tool(src, plain, "q4_k_m")
    assert r.returncode == 0, r.stdout + r.stderr
    name = "blk.0.ffn_up_exps.weight"
    assert t[name][2].tobytes() != read_gguf(plain)[1][name][2].tobytes()            # the matrix reached the expert tensors
    m = pkg.Model(dst)
    c = pkg.Context(m, n_ctx=64, n_ubatch=64, type_k=Q8, type_v=Q8)
    assert c.decode(np.arange(8, dtype=np.int32), np.arange(8)) == 0
    assert np.isfinite(c.logits()).all()
    c.close(); m.close()


def test_the_tool_refuses_before_it_reads(tmp_path):
    r = run_tool(str(tmp_path / "missing.gguf"), str(tmp_path / "out.gguf"), "iq4_xs")
    assert r.returncode == 2 and "iq4_xs" in r.stderr and not os.path.exists(str(tmp_path / "out.gguf"))
