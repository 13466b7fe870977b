"""CPU tests of speculative decoding in the slot loop: tests/host/spec_host_tests.cc (a fake arithmetic backend with a scripted draft model: what a request
emits must not depend on the draft; n_predict, stop strings and </s> cut inside an accepted run; grammar and n_probs requests never ask the draft; two slots
in one tick; the context shift) is built with g++ the way tests/test_host_logic.py builds its program and must exit 0 - plain, and as a stand-alone binary with
the address and undefined-behaviour sanitizers compiled in."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cortex.llamacpp_amd", "host")
SRCS = [os.path.join(ROOT, "tests", "host", "spec_host_tests.cc")] + [
    os.path.join(HOST, f) for f in ("vocab.cc", "sampling.cc", "grammar.cc", "json_schema.cc", "server_context.cc", "gguf.cc", "log.cc")]


@pytest.mark.parametrize("name,flags", [("plain", []), ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])])
def test_spec_host_program(tmp_path, name, flags):
    exe = str(tmp_path / f"spec_host_tests_{name}")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-pthread", *flags, *SRCS, "-o", exe],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    assert "all speculative-decoding host checks passed" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-6000:]
