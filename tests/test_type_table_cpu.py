"""The weight-type table of csrc/ggml_types.h against the two Python statements of the same facts: a few-line program prints `id name block_elems block_bytes`
per table row, and every type the synthetic writer knows (gguf_synth.TYPE_NAME / BLOCK_ELEMS / BLOCK_BYTES) must say the same; the ids are the binding's."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = r"""
#include "ggml_types.h"
#include <cstdio>
int main() {
    for (int i = 0; i < mi355::N_TYPE_LAYOUTS; i++) {
        const mi355::TypeLayout &r = mi355::kTypeLayouts[i];
        std::printf("%d %s %d %d\n", r.id, r.name, r.block_elems, r.block_bytes);
    }
    return 0;
}
"""


def test_table_rows_match_the_writer_and_the_binding(pkg, tmp_path):
    gs, binding = pkg.gguf_synth, pkg.binding
    (tmp_path / "main.cc").write_text(MAIN)
    exe = str(tmp_path / "type_table")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "cortex.llamacpp_amd", "csrc"), str(tmp_path / "main.cc"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    rows = {}
    for line in out.stdout.split("\n"):
        if line:
            i, name, be, bb = line.split()
            assert int(i) not in rows, line
            rows[int(i)] = (name, int(be), int(bb))
    # every type the writer knows is a table row with the same name and block
    assert len(gs.TYPE_NAME) == 18 and set(gs.TYPE_NAME) == set(gs.BLOCK_ELEMS) == set(gs.BLOCK_BYTES)
    for t in gs.TYPE_NAME:
        assert rows[t] == (gs.TYPE_NAME[t], gs.BLOCK_ELEMS[t], gs.BLOCK_BYTES[t]), t
    # the table knows one thing more: the Q8_K activation block
    assert set(rows) - set(gs.TYPE_NAME) == {gs.Q8_K} and rows[gs.Q8_K] == ("q8_K", 256, 292)
    # the ids: one Python list (the binding's names are the writer's objects), each under the table's name
    ids = {n: getattr(binding, n) for n in ("F32", "F16", "BF16", "Q4_0", "Q4_1", "Q5_0", "Q5_1", "Q8_0", "Q2_K", "Q3_K", "Q4_K", "Q5_K", "Q6_K", "Q8_K", "IQ4_NL", "IQ4_XS",
                                            "TQ1_0", "TQ2_0", "MXFP4")}
    assert sorted(ids.values()) == sorted(rows)
    for n, t in ids.items():
        assert getattr(gs, n) == t and rows[t][0] == n.lower().replace("_k", "_K"), n
