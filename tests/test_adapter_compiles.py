"""The outer drop-in boundary: integration/mi355_engine_adapter.cc must implement EVERY pure virtual of the reference's EngineI
(base/cortex-common/enginei.h:31-73) and export get_engine (src/llama_engine.cc:1300-1304).  Compile-only: EngineI is declared from its members in vtable order
(tests/golden/enginei_v1.json) + stub json / trantor headers under tests/stubs/.  Pins the SHAPE of the boundary, no numbers."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(ROOT, "cortex.llamacpp_amd", "lib")


def write_enginei(base_dir) -> None:
    """<base_dir>/cortex-common/enginei.h: class EngineI as the fixture lists it (a member that is not pure keeps a body that returns the default)."""
    with open(os.path.join(ROOT, "tests", "golden", "enginei_v1.json")) as f:
        shape = json.load(f)
    lines = ["#pragma once"] + [f"#include {h}" for h in shape["includes"]] + ["class EngineI {", " public:", "  struct EngineLoadOption {"]
    lines += [f"    {t} {n};" for t, n in shape["load_option"]]
    lines += ["  };", "  struct EngineUnloadOption {};", "  virtual ~EngineI() {}"]
    for m in shape["methods"]:
        body = " = 0;" if m.get("pure", True) else " { return {}; }"
        lines.append(f"  virtual {m['ret']} {m['name']}({', '.join(m['params'])}){body}")
    lines.append("};")
    os.makedirs(os.path.join(base_dir, "cortex-common"))
    with open(os.path.join(base_dir, "cortex-common", "enginei.h"), "w") as f:
        f.write("\n".join(lines) + "\n")


def test_adapter_is_concrete_and_get_engine_links(tmp_path):
    base = str(tmp_path / "base")
    write_enginei(base)
    so = tmp_path / "libengine.so"
    cmd = ["g++", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", base, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "integration", "mi355_engine_adapter.cc"), "-L", LIB_DIR, "-lmi355_llama", "-Wl,-rpath," + LIB_DIR, "-Wl,--no-undefined", "-o", str(so)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    # (`new Mi355Engine()` inside get_engine is ill-formed if one pure virtual is left unimplemented; -Wl,--no-undefined: every mi355_engine_* it calls exists)
    assert r.returncode == 0, r.stderr
    syms = subprocess.run(["nm", "-D", "--defined-only", str(so)], capture_output=True, text=True).stdout
    assert " T get_engine" in syms
    und = subprocess.run(["nm", "-D", "--undefined-only", str(so)], capture_output=True, text=True).stdout
    for fn in ("mi355_engine_load", "mi355_engine_unload", "mi355_engine_set_file_logger", "mi355_engine_set_log_level", "mi355_engine_create"):
        assert fn in und
