"""CPU tests of the host-RAM prompt cache: tests/host/prompt_cache_tests.cc (the store's LRU / replacement rules and the slot loop's save / restore decisions
against a fake backend whose sequence states round-trip) is built with g++ the way tests/test_host_logic.py builds its program - here as a stand-alone binary
with the address and undefined-behaviour sanitizers compiled in - and must exit 0."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cortex.llamacpp_amd", "host")
SRCS = [os.path.join(ROOT, "tests", "host", "prompt_cache_tests.cc")] + [
    os.path.join(HOST, f) for f in ("vocab.cc", "sampling.cc", "grammar.cc", "json_schema.cc", "server_context.cc", "gguf.cc", "log.cc")]


def test_prompt_cache_program_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "prompt_cache_tests")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-pthread", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", *SRCS, "-o", exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    assert "all prompt-cache checks passed" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-6000:]
