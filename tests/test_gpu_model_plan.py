"""The plan the CPU tests look at is the plan the loader carries out: a loaded model's sizes, through the C ABI, against `host_tests --plan` on the same file."""
import pytest

from test_model_plan_cpu import model_file, plan, plan_exe  # noqa: F401  (plan_exe: the fixture)

pytestmark = pytest.mark.gpu


def test_loaded_model_matches_the_cpu_plan(pkg, plan_exe, tmp_models):  # noqa: F811
    pkg.Backend()
    for cfg, ftype in (("tiny", "q4_k_m"), ("tiny-qwen3", "q4_k_m"), ("tiny-moe", "q4_k_m"), ("tiny-nomic", "f16")):
        path = model_file(pkg.gguf_synth, tmp_models, cfg, ftype)
        p = plan(plan_exe, path)
        assert "err" not in p, p
        m = pkg.Model(path)
        got = (m.size, m.bytes_per_token, m.vram - m.planes_bytes)
        m.close()
        assert got == (p["file_tensor_bytes"], p["bytes_per_token"], p["total"]), (cfg, ftype)
