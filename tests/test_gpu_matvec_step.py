"""The decode step's mat-vec launches, op by op: every launch of tests/matvec_step_cases.py through Backend.mat_vec_step - the code the model issues it with -
against the oracle within the re-association bound, on the path the case names, with the whole padded out buffers checked: no NaN inside N (the buffers are
0xFF bytes before the launch), the pad columns still 0xFF, the pinned host copy equal to the device row.  Then the relations the code states between its
forms, bit for bit: EPI_ADD = resid + EPI_STORE; weight stream = register ring; the in-launch quantiser = the quantiser's launch; and the forms behind the
start-up switches, each in a fresh child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if __name__ == "__main__":                                       # the child of test_start_up_switch: argv = out.npz, case names
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)

import matvec_step_cases as mc
from matvec_step_cases import ADD, CASES, STORE

pytestmark = pytest.mark.gpu

SEEN = set()           # (kernel, role, kb, fuse, fast_ok, down_early) of every launch a test of this module made
_REF, _INP = {}, {}


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def inputs(c):
    if c["name"] not in _INP:
        _INP[c["name"]] = mc.inputs(c)
    return _INP[c["name"]]


def reference(c):
    if c["name"] not in _REF:
        _REF[c["name"]] = mc.reference(c, inputs(c))
        for r in _REF[c["name"]]:
            r.setflags(write=False)
    return _REF[c["name"]]


def run(be, c, epi=None, fuse=None, x=None, host=None):
    inp = inputs(c)
    epi = c["epi"] if epi is None else epi
    fuse = c["fuse"] if fuse is None else fuse
    ys, yh, path = be.mat_vec_step(c["types"], inp["W"], c["Ns"], c["K"], inp["x"] if x is None else x, epi=epi, resid=inp["resid"] if epi == ADD else None, fuse=fuse,
                                   norm_w=inp["nw"] if fuse == 1 else None, eps=mc.EPS, want_host_copy=c["host"] if host is None else host, expert_ids=c["sel"],
                                   n_expert=c["n_expert"], ld_pad=c["ld_pad"])
    for p in path:
        SEEN.add((p["kernel"], p.get("role"), p.get("kb"), fuse, p.get("fast_ok"), p.get("down_early")))
    return ys, yh, path


def check_buffers(c, ys, yh, refs, what=""):
    """Every out buffer whole: values inside N within the bound of the oracle and none NaN, the pad columns untouched; the host copy the device row's bits."""
    assert len(ys) == len(refs)
    for s, (y, ref) in enumerate(zip(ys, refs)):
        N = ref.shape[1]
        assert y.shape == (ref.shape[0], N + c["ld_pad"]), (c["name"], what, s)
        inside = y[:, :N]
        nan_rows = np.argwhere(np.isnan(inside))
        assert nan_rows.size == 0, f"{c['name']} {what} segment {s}: unwritten / NaN results at (row of the buffer, output) {nan_rows[:8].tolist()} of {len(nan_rows)}"
        assert (y[:, N:].view(np.uint32) == 0xFFFFFFFF).all(), f"{c['name']} {what} segment {s}: a pad column was written"
        err = np.abs(inside - ref)
        i = np.unravel_index(int(err.argmax()), err.shape)
        print(f"{c['name']} {what} segment {s}: max |err| {err.max():.3e} at {i}, bound {mc.bound(ref):.3e}")
        assert err.max() <= mc.bound(ref), f"{c['name']} {what} segment {s}: |err| {err.max():.3e} at {i} (got {inside[i]!r}, want {ref[i]!r}) > {mc.bound(ref):.3e}"
    if c["host"]:
        assert yh is not None and (yh.view(np.uint32) == ys[0][0, :len(yh)].view(np.uint32)).all(), f"{c['name']} {what}: the host copy is not the device row"


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_launch_matches_oracle_on_its_path(be, c):
    ys, yh, path = run(be, c)
    assert path == c["path"], f"{c['name']}: took {path}"
    check_buffers(c, ys, yh, reference(c))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("c", [c for c in CASES if c["epi"] == ADD], ids=lambda c: c["name"])
def test_add_is_resid_plus_store(be, c):
    """Every kernel's epilogue is out = resid + v with v the value EPI_STORE stores (mmvq_stream_dev.h flush, mmvq_fast_dev.h, mmvq.hip): one IEEE f32 add."""
    ya, _, pa = run(be, c)
    ystore, _, ps = run(be, c, epi=STORE)
    assert [p["kernel"] for p in pa] == [p["kernel"] for p in ps], (pa, ps)
    N = c["Ns"][0]
    want = (inputs(c)["resid"][:, :N] + ystore[0][:, :N]).astype(np.float32)
    assert (_bits(ya[0][:, :N]) == _bits(want)).all(), c["name"]


STREAM_CASES = [c for c in CASES if any(p["kernel"] == "stream" for p in c["path"])]


@pytest.mark.parametrize("c", STREAM_CASES, ids=lambda c: c["name"])
def test_stream_is_ring_bitwise(be, c):
    """kernels.h: the weight stream is bit-identical to the register ring.  Both are held to the oracle above; here to each other, every buffer whole."""
    ys, yh, _ = run(be, c)
    be.set_option("mmvq_stream", 0)
    try:
        yr, yhr, pr = run(be, c)
    finally:
        be.set_option("mmvq_stream", 1)
    assert [p["kernel"] for p in pr] == ["ring" if p["kernel"] == "stream" else p["kernel"] for p in c["path"]], pr
    check_buffers(c, yr, yhr, reference(c), "ring")
    for a, b in zip(ys, yr):
        assert (_bits(a) == _bits(b)).all(), c["name"]
    if c["host"]:
        assert (_bits(yh) == _bits(yhr)).all(), c["name"]


@pytest.mark.parametrize("c", [c for c in CASES if c["fuse"] == 2 and not c["sel"]], ids=lambda c: c["name"])
def test_in_launch_quantiser_is_the_quantiser_launch(be, c):
    """mmvq.hip launch_mmvq / runtime.cc: the prologue that quantises the activation inside the launch gives the codes of the quantiser's own launch, so the
    two forms store the same bits."""
    y2, _, _ = run(be, c)
    y0, _, _ = run(be, c, fuse=0)
    for a, b in zip(y2, y0):
        assert (_bits(a) == _bits(b)).all(), c["name"]


@pytest.mark.parametrize("name", ["qkv_k4096_q4k_q4k_q6k", "qkv_k2048_q5k_q80_q80", "gate_up_k2048_q4k", "qkv_k2048_iq4nl", "base_k2080_q40_fuse1"])
def test_in_launch_norm_is_the_norm_launch(be, name):
    """runtime.cc moe_selected_desc: RMSNorm + quantise in the prologue is the arithmetic of the norm launch.  The norm's f32 rows from its own launch, quantised
    by the quantiser's launch (fuse 0), against the prologue (fuse 1): the same bits.  (The oracle is not involved: both sides are the device's.)"""
    c = mc.BY_NAME[name]
    inp = inputs(c)
    y1, _, p1 = run(be, c)
    xn = be.rms_norm_mul(inp["x"], inp["nw"], mc.EPS)
    y0, _, p0 = run(be, c, fuse=0, x=xn)
    # (the claim is per kernel: stream and ring share their arithmetic, the generic kernel sums in another order - a pair across the two is not one)
    family = lambda p: "generic" if p["kernel"] in ("base", "tiled") else "ring"
    assert [family(p) for p in p1] == [family(p) for p in p0], (p1, p0)
    for a, b in zip(y1, y0):
        assert (_bits(a) == _bits(b)).all(), name


def _child(out, names):
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    be = pkg.Backend()
    res = {}
    for nm in names:
        c = mc.BY_NAME[nm]
        ys, yh, path = run(be, c)
        for s, y in enumerate(ys):
            res[f"{nm}/y{s}"] = y
        if yh is not None:
            res[f"{nm}/host"] = yh
        res[f"{nm}/path"] = np.array([[mc_kernel_id(p), p.get("kb", 0), int(p.get("fast_ok", False)), int(p.get("down_early", False)), p["T"]] for p in path], np.int32)
        res[f"{nm}/role"] = np.array([p.get("role", "") for p in path])
    np.savez(out, **res)


def mc_kernel_id(p):
    return ("base", "ring", "stream", "tiled").index(p["kernel"])


@pytest.mark.parametrize("var", sorted(mc.SWITCH_CASES))
def test_start_up_switch(be, var, tmp_path):
    """MI355_STREAM_FAST_START=0 / MI355_STREAM_DOWN_EARLY=0: the plain kernels of gate | up, the head and ffn_down - the same consumers' arithmetic, so the
    bits of the default forms.  MI355_MMVQ_FAST=0: the generic kernel on every shape, a third implementation - the oracle bound.  Read once per process: a
    fresh child computes the subset and hands the raw buffers back."""
    names = mc.SWITCH_CASES[var]
    out = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out] + list(names), cwd=ROOT, capture_output=True, text=True, timeout=300, env=dict(os.environ, **{var: "0"}))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    got = np.load(out)
    for nm in names:
        c = mc.BY_NAME[nm]
        want_path = mc.switch_path(var, c)
        pth, roles = got[f"{nm}/path"], got[f"{nm}/role"]
        took = []
        for row, role in zip(pth, roles):
            d = {"T": int(row[4]), "kernel": ("base", "ring", "stream", "tiled")[row[0]]}
            if row[0] == 2:
                d.update(role=str(role), kb=int(row[1]), fast_ok=bool(row[2]), down_early=bool(row[3]))
            took.append(d)
            SEEN.add((d["kernel"], d.get("role"), d.get("kb"), c["fuse"], d.get("fast_ok"), d.get("down_early")))
        assert took == want_path, (var, nm, took)
        ys = [got[f"{nm}/y{s}"] for s in range(len(reference(c)))]
        yh = got[f"{nm}/host"] if c["host"] else None
        check_buffers(c, ys, yh, reference(c), var + "=0")
        if var != "MI355_MMVQ_FAST":
            mine, _, _ = run(be, c)
            for a, b in zip(mine, ys):
                assert (_bits(a) == _bits(b)).all(), (var, nm)


def test_raised_error_word_fails_the_entry(be, pkg):
    """The entry installs the process's stream error word as a context does: a launch whose kernel raises it (here: raised by hand, as a bounded wait that gives
    up does) is an error, never a result; the word is consumed, so the next launch is clean."""
    c = mc.BY_NAME["qkv_k1024_q4k_q4k_q6k"]
    run(be, c)                                                   # (installs the word)
    be.set_option("raise_stream_error", 1)
    with pytest.raises(pkg.MI355Error, match="stream error word"):
        run(be, c)
    ys, yh, _ = run(be, c)
    check_buffers(c, ys, yh, reference(c))


def test_every_form_was_run():
    """Last in the module: the launches above cover every kernel launch_mmvq_stream's switches instantiate in a product build - per prologue and pass count the
    plain kernel and every role, with and without the preloaded-argument forms, the expert forms, the ternary kernel's three cases - and launch_mmvq's
    other kernels (register ring, generic, tiled)."""
    need = set()
    for kb in (1, 2, 3, 4, 6, 7, 10):
        need.add(("stream", "stream", kb, 0, False, False))                               # STREAM0
        need.add(("stream", "stream", kb, 2, False, False))                               # STREAM2, no role
        need.add(("stream", "ffn_down", kb, 2, False, kb in (6, 7)))                      # STREAM2 / STREAM_EARLY
    for kb in (6, 7):
        need.add(("stream", "ffn_down", kb, 2, False, False))                             # MI355_STREAM_DOWN_EARLY=0
    for kb in (1, 2, 3, 4):
        need.add(("stream", "stream", kb, 1, False, False))                               # STREAM1
        need.add(("stream", "qkv", kb, 1, False, False))
        for role in ("gate_up", "head"):
            need.add(("stream", role, kb, 1, True, False))                                # STREAM_FAST
            need.add(("stream", role, kb, 1, False, False))                               # MI355_STREAM_FAST_START=0 (and the head with a host copy)
    for kb, fz in ((1, 1), (2, 1), (2, 2), (4, 2), (7, 2)):
        need.add(("stream", "moe", kb, fz, False, False))                                 # STREAM_MOE
    for kb, fz in ((2, 1), (7, 2)):
        need.add(("stream", "ternary", kb, fz, False, False))
    for k in ("ring", "base", "tiled"):
        assert any(s[0] == k for s in SEEN), k
    missing = sorted(need - SEEN, key=str)
    assert not missing, f"forms no test of this module launched: {missing}"


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2:])
