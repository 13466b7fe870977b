"""CPU tests of the Sampler's side of the whole-row device sampler: tests/host/sample_vocab_host_tests.cc (what qualifies, what is sent, mirostat-2's mu after
a returned probability) is built with g++ the way tests/test_spec_host.py builds its program and must exit 0."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cortex.llamacpp_amd", "host")

def test_sample_vocab_host_program(tmp_path):
    exe = str(tmp_path / "sample_vocab_host_tests")
    srcs = [os.path.join(ROOT, "tests", "host", "sample_vocab_host_tests.cc"), os.path.join(HOST, "sampling.cc"), os.path.join(HOST, "grammar.cc")]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", *srcs, "-o", exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "all whole-row sampler host checks passed" in r.stdout, (r.stdout + r.stderr)[-6000:]
