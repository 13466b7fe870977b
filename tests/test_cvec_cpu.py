"""Control vectors without a GPU: the exported symbols and their answers without a device, the file loader (host/cvec.cc) through
mi355_control_vector_load, the composed reference tests/cvec_ref.py against Qwen3Ref, the delta condition of the end-to-end cases, the power method's numpy
twins against float64 (the margin M_PCA the GPU test allows), and tools/cvector_generator.py end to end on a stand-in model with the twin for the device."""
import importlib.util
import os
import re

import numpy as np
import pytest

import cvec_cases as cc
import cvec_ref as cr
import lora_cases as lc
import oracle_py as oq
from gguf_read import read_gguf
from lora_cases import FLIP_TOL, KV, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi355_apply_adapter_cvec", "mi355_control_vector_load", "mi355_cvec_direction", "mi355_op_add_row_vec")
F32, F16 = 0, 1


@pytest.fixture(scope="module")
def gs(pkg):
    return pkg.gguf_synth


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("cvector_generator", os.path.join(ROOT, "tools", "cvector_generator.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ exports
def test_exports_and_no_device(pkg, lib):
    hdr = open(os.path.join(ROOT, "include", "mi355_llama.h")).read()
    for name in NEW:
        assert re.search(r"MI355_API[^;(]*\b" + name + r"\s*\(", hdr), name
        assert name in pkg.binding.SYMBOLS and hasattr(lib, name), name
    err = lambda: (lib.mi355_last_error() or b"").decode()
    no_dev = lib.mi355_device_count() == 0
    x = np.ones((2, 32), np.float32)
    out = np.full(32, 7.0, np.float32)
    # a null context: the device first (as every entry here), then the argument
    rc = lib.mi355_apply_adapter_cvec(None, x.ctypes.data, x.size, 32, 1, 1)
    assert rc == (-100 if no_dev else -103) and ("no HIP device" in err() if no_dev else "null context" in err())
    if no_dev:
        assert lib.mi355_cvec_direction(0, x.ctypes.data, 2, 32, x.ctypes.data, 4, 2, 0.0, out.ctypes.data, None, None) == -100 and "no HIP device" in err()
        assert (out == 7.0).all()
        y = np.zeros((3, 32), np.float32)
        assert lib.mi355_op_add_row_vec(x.ctypes.data, x.ctypes.data, 32, 2, y.ctypes.data) == -100 and "no HIP device" in err()
    # the loader is host arithmetic: it answers for itself with or without a device
    assert lib.mi355_control_vector_load(None, None, 0, None, 0, None) == -103 and "no file given" in err()


# ------------------------------------------------------------------------------------------------ loader
def write_dirs(gs, path, dirs, extra=()):
    """dirs: {layer: array | (ne, type, bytes)}"""
    w = gs.GGUFWriter()
    w.add("general.architecture", "str", "controlvector")
    for il, v in dirs.items():
        if isinstance(v, tuple):
            w.add_tensor(f"direction.{il}", *v)
        else:
            w.add_tensor(f"direction.{il}", (v.size,), F32, np.ascontiguousarray(v, "<f4").tobytes())
    for name, v in extra:
        w.add_tensor(name, (v.size,), F32, np.ascontiguousarray(v, "<f4").tobytes())
    w.write(str(path))
    return str(path)


def test_loader_sums_scaled_files(pkg, lib, gs, tmp_path):
    rng = np.random.default_rng(1)
    E = 64
    a = {il: rng.standard_normal(E).astype(np.float32) for il in (1, 2, 4)}          # layer 3 absent: zero
    b = {il: rng.standard_normal(E).astype(np.float32) for il in (2, 3, 4, 5, 6)}    # ends at another layer
    pa = write_dirs(gs, tmp_path / "a.gguf", a, extra=[("something.else", np.ones(3, np.float32))])     # other tensors are ignored
    pb = write_dirs(gs, tmp_path / "b.gguf", b)
    load = lambda items: pkg.binding.control_vector_load(lib, items)
    data, ne = load([(pa, 0.5), (pb, -2.0)])
    assert ne == E and data.size == 6 * E
    want = np.zeros((6, E), np.float32)
    for il, v in a.items():
        want[il - 1] += np.float32(0.5) * v
    for il, v in b.items():
        want[il - 1] += np.float32(-2.0) * v
    assert data.reshape(6, E).tobytes() == want.tobytes()
    data1, _ = load([pa])                                                             # a path alone: scale 1; as long as the highest layer named
    assert data1.size == 4 * E and (data1.reshape(4, E)[2] == 0).all() and data1.reshape(4, E)[3].tobytes() == a[4].tobytes()
    data2, _ = load([(pb, 1.0), (pa, 1.0)])                                           # the shorter file second: the length is still the longest
    assert data2.size == 6 * E
    # a cap that is too small writes nothing and still reports the size
    out = np.full(10, 3.0, np.float32)
    import ctypes as C
    paths = (C.c_char_p * 1)(pa.encode())
    assert lib.mi355_control_vector_load(C.cast(paths, C.c_void_p), None, 1, out.ctypes.data, 10, None) == 4 * E and (out == 3.0).all()


@pytest.mark.parametrize("name,text", [
    ("zero", "direction.0: layer 0 never has a control vector"), ("f16", "a direction tensor must be F32"), ("2d", "a direction tensor must have one"),
    ("ragged", "differs from the other direction tensors'"), ("two-lengths", "differs from the other direction tensors'"), ("none", "no direction tensor"),
    ("missing", "missing.gguf"), ("nan-index", "the layer index is not a number")])
def test_loader_refusals(pkg, lib, gs, tmp_path, name, text):
    v = np.ones(64, np.float32)
    good = write_dirs(gs, tmp_path / "good.gguf", {1: v})
    files = {
        "zero": lambda: [write_dirs(gs, tmp_path / "x.gguf", {0: v, 1: v})],
        "f16": lambda: [write_dirs(gs, tmp_path / "x.gguf", {1: ((64,), F16, np.ones(64, np.float16).tobytes())})],
        "2d": lambda: [write_dirs(gs, tmp_path / "x.gguf", {1: ((32, 2), F32, v.tobytes())})],
        "ragged": lambda: [write_dirs(gs, tmp_path / "x.gguf", {1: v, 2: np.ones(96, np.float32)})],
        "two-lengths": lambda: [good, write_dirs(gs, tmp_path / "x.gguf", {1: np.ones(96, np.float32)})],
        "none": lambda: [write_dirs(gs, tmp_path / "x.gguf", {}, extra=[("other", v)])],
        "missing": lambda: [good, str(tmp_path / "missing.gguf")],
        "nan-index": lambda: [write_dirs(gs, tmp_path / "x.gguf", {"x1": v})],
    }[name]()
    with pytest.raises(pkg.MI355Error, match=re.escape(text)) as ei:
        pkg.binding.control_vector_load(lib, files)
    assert "(-102)" in str(ei.value)


def test_tool_writer_round_trips(pkg, lib, tool, tmp_path):
    rng = np.random.default_rng(2)
    dirs = {il: rng.standard_normal(96).astype(np.float32) for il in (1, 2, 3)}
    path = str(tmp_path / "cv.gguf")
    tool.write_cvec(path, dirs, "llama")
    kv, t = read_gguf(path)
    assert kv["general.architecture"] == "controlvector" and kv["controlvector.model_hint"] == "llama" and kv["controlvector.layer_count"] == 3
    assert sorted(t) == ["direction.1", "direction.2", "direction.3"] and all(ty == F32 and tuple(ne) == (96,) for ne, ty, _ in t.values())
    data, ne = pkg.binding.control_vector_load(lib, [(path, 1.0)])
    assert ne == 96 and data.tobytes() == np.stack([dirs[1], dirs[2], dirs[3]]).tobytes()


# ------------------------------------------------------------------------------------------------ the composed reference
@pytest.fixture(scope="module")
def plain_runs(gs, tmp_models):
    """per case: (base path, prompt, Qwen3Ref's logits and taps of the prompt without a vector) - computed once, shared, left unchanged"""
    out = {}
    for case in cc.MODEL_CASES:
        oq.set_fa_v_acc_f32(1 if case.kv == "f16" else 0)
        try:
            base = lc.base_file(gs, tmp_models, case)
            ref = lc.reference(case, base, [], 32, False)                 # LoraRef / LoraMoeRef without adapters: Qwen3Ref's own decode
            prompt = np.random.default_rng(cc.PROMPT_SEED).integers(0, ref.n_vocab, cc.N_PROMPT)
            r = ref.decode(prompt, np.arange(cc.N_PROMPT))[0].copy()
            out[case.name] = (base, prompt, r, [t.copy() for t in ref.taps])
        finally:
            oq.set_fa_v_acc_f32(0)
    return out


def run_ref(case, base, prompt, vec, a, b):
    oq.set_fa_v_acc_f32(1 if case.kv == "f16" else 0)
    try:
        ref = cc.reference(case, base, 32)
        ref.apply_cvec(vec, a, b)
        r = ref.decode(prompt, np.arange(prompt.size))[0]
        return r, ref.taps
    finally:
        oq.set_fa_v_acc_f32(0)


@pytest.mark.parametrize("case", cc.MODEL_CASES, ids=cc.MODEL_IDS)
def test_reference_forward(plain_runs, case):
    base, prompt, r0, taps0 = plain_runs[case.name]
    n_layer, E = len(taps0), taps0[0].shape[1]
    # no vector, and an all-zero vector: Qwen3Ref's taps and logits, bit for bit
    for vec in (None, np.zeros((n_layer - 1, E), np.float32)):
        r, taps = run_ref(case, base, prompt, vec, 1, n_layer)
        assert r.tobytes() == r0.tobytes() and all(t.tobytes() == t0.tobytes() for t, t0 in zip(taps, taps0))
    # a vector on layer l only: the taps below l are untouched, the tap of l is the plain one plus the vector, above it they move
    vec = cc.case_vector(case, n_layer, E)
    for l in sorted({1, n_layer - 1}):
        r, taps = run_ref(case, base, prompt, vec, l, l)
        assert all(taps[il].tobytes() == taps0[il].tobytes() for il in range(l))
        assert taps[l].tobytes() == (taps0[l] + vec[l - 1]).astype(np.float32).tobytes()
        assert r.tobytes() != r0.tobytes()
    # a buffer that ends before layer l leaves l alone; layer 0 never takes one
    r, taps = run_ref(case, base, prompt, vec[:0], 0, n_layer)
    assert r.tobytes() == r0.tobytes()


@pytest.mark.parametrize("case", cc.MODEL_CASES, ids=cc.MODEL_IDS)
def test_delta_condition(plain_runs, case):
    """The reference alone moves the logits by at least 10 * FLIP_TOL on every end-to-end case and range: a device that ignored the vector fails FLIP_TOL."""
    base, prompt, r0, taps0 = plain_runs[case.name]
    n_layer, E = len(taps0), taps0[0].shape[1]
    vec = cc.case_vector(case, n_layer, E)
    for name, a, b in cc.ranges(n_layer):
        r, _ = run_ref(case, base, prompt, vec, a, b)
        d = rel_err(r, r0)
        print(case.name, name, "delta", d)
        assert d >= 10 * FLIP_TOL, (name, d)


# ------------------------------------------------------------------------------------------------ the power method
def test_pca_twin_margin():
    """Both f32 twins against the float64 eigenvector on every case; lambda_2 / lambda_1 <= GAP_MAX from the float64 spectrum; M_PCA is twice the largest
    1 - |cos| seen, written as a constant that must cover what is measured here and not be a round-up of more than a tenth."""
    worst = 0.0
    for R, E in cc.PCA_CASES:
        D, u, b0 = cc.pca_rows(R, E)
        u64, lam = cr.top_eigvec64(D)
        gap = float(lam[1] / lam[0]) if lam.size > 1 else 0.0
        assert gap <= cc.GAP_MAX, (R, E, gap)
        assert cr.one_minus_abs_cos(u64, u) < 0.05                      # (the planted direction is the one found)
        for order in ("serial", "pairwise"):
            b, _ = cr.pca_twin(D, b0, cc.PCA_ITERS, order)
            assert float(D.astype(np.float64).dot(b.astype(np.float64)).sum()) >= 0
            worst = max(worst, cr.one_minus_abs_cos(b, u64))
            if R == 1:
                assert cr.one_minus_abs_cos(b, D[0]) <= cc.M_PCA
        assert cr.one_minus_abs_cos(cr.mean_twin(D), cr.mean_dir64(D)) <= cc.M_PCA
    want = 2.0 * worst
    print(f"largest 1 - |cos| of an f32 twin: {worst:.4e}; M_PCA {cc.M_PCA:.4e}")
    assert want <= cc.M_PCA <= 1.1 * want, (want, cc.M_PCA)


# ------------------------------------------------------------------------------------------------ the tool on the twin
def test_tool_on_the_twin(pkg, lib, tool, tmp_path):
    """Pairing, padding, the zero-row filter, the layer numbering and the file, with seeded taps for the model and the numpy twin for the device."""
    n_layer, E, PAD = 4, 64, 99
    rng = np.random.default_rng(3)
    u = {il: rng.standard_normal(E) for il in range(n_layer)}
    u = {il: v / np.linalg.norm(v) for il, v in u.items()}
    assert tool.pad_pair([1, 2, 3], [1, 4], PAD) == ([1, 2, 3], [1, 4, PAD]) and tool.pad_pair([1], [1, 5, 6], PAD) == ([1, PAD, PAD], [1, 5, 6])
    pairs = [tool.pad_pair(p, n, PAD) for p, n in (([1, 10, 11, 12], [1, 20, 21]), ([1, 13], [1, 22, 23]), ([1, 14, 15], [1, 24, 25]))]
    calls = []

    def run_taps(tokens):
        """row t of layer il: a function of the token alone - so the BOS rows of a pair are equal (their difference is dropped) - that leans along
        +u[il] for the positive prompts' tokens (10 ..) and along -u[il] for the negative ones' (20 .. and the pad)"""
        calls.append(list(tokens))
        out = np.zeros((n_layer, len(tokens), E), np.float32)
        for il in range(n_layer):
            for t, tok in enumerate(tokens):
                g = np.random.default_rng(1000 * il + tok)
                lean = 0.0 if tok == 1 else (1.0 + 0.1 * (tok % 7)) * (1 if 10 <= tok < 20 else -1)
                out[il, t] = (lean * u[il] + (0.02 * g.standard_normal(E) if tok != 1 else g.standard_normal(E))).astype(np.float32)
        return out

    seen = {}

    def direction(rows, init, method):
        seen[len(seen) + 1] = rows
        if method == "mean":
            assert init is None
            return cr.mean_twin(rows)
        assert abs(float(np.linalg.norm(init)) - 1) < 1e-6
        return cr.pca_twin(rows, init, 32)[0]

    dirs = tool.generate(pairs, run_taps, direction, n_layer, E, "pca", seed=4)
    assert calls == [p for pair in pairs for p in pair]
    assert sorted(dirs) == [1, 2, 3]                                     # never layer 0; the last layer's rows too (after layer n_layer - 1)
    n_rows = sum(len(p) - 1 for p, _ in pairs)                           # every position but BOS, whose rows are equal and are dropped
    assert all(seen[il].shape == (n_rows, E) for il in (1, 2, 3))
    for il in (1, 2, 3):
        assert cr.one_minus_abs_cos(dirs[il], u[il]) < 1e-3 and float(dirs[il].astype(np.float64) @ u[il]) > 0      # from negative to positive
    again = tool.generate(pairs, run_taps, direction, n_layer, E, "pca", seed=4)
    assert all(again[il].tobytes() == dirs[il].tobytes() for il in dirs)
    seen.clear()
    mean = tool.generate(pairs, run_taps, direction, n_layer, E, "mean", seed=4)
    assert all(float(mean[il].astype(np.float64) @ u[il]) > 0.99 for il in (1, 2, 3))
    path = str(tmp_path / "twin.gguf")
    tool.write_cvec(path, dirs, "stand-in")
    data, ne = pkg.binding.control_vector_load(lib, [(path, 2.0)])
    assert ne == E and data.tobytes() == (np.float32(2.0) * np.stack([dirs[1], dirs[2], dirs[3]])).astype(np.float32).tobytes()
