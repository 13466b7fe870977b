"""Row split across ranks, on the one GPU the test box has.

* two / four ranks = separate processes that share the device; each loads its slice of every projection through
  mi355_model_load_from_file(tp_rank, tp_size) and runs the same mi355_decode calls; the partial sums of attn_output /
  ffn_down and the logits slices are exchanged through the host transport (gloo) because RCCL refuses two ranks on one
  device.  The gathered logits are compared with the CPU oracle run on the WHOLE file (same tolerance rule as
  test_gpu_model.py) and with the unsplit HIP run.
* the RCCL transport itself is exercised with a group of one rank: same code path, the all-reduce and all-gather are
  issued through librccl on the context's stream and captured into the decode graphs; results must equal the unsplit run
  bit for bit.
"""
import dataclasses
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as oq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KV = {"f16": 1, "q8_0": 8}
FLIP_TOL = 3e-2     # see test_gpu_model.py: one flipped int8 rounding moves these tiny models' logits by up to ~1e-2
TIGHT_TOL = 2e-5
# The shared device admits at most 6 processes with it open: this test's own, its ranks and (test_reduce_scatter_case_in_a_fresh_process) a child pytest.
# So at most 4 ranks.  A rank's geometry in a split of Llama-3-8B / Llama-3-70B over 8 GPUs is carried by 4 ranks of a model half as wide: the same query and
# kv heads, attn_output and ffn_down columns per rank.  name: (full-width config, n_embd, n_head, n_head_kv, n_ff)
HALF_WIDTH = {
    "tiny-8b-half-2l": ("tiny-8b-2l", 2048, 16, 4, 7168),
    "tiny-70b-half-2l": ("tiny-70b-2l", 4096, 32, 4, 14336),
}


def config(pkg, cfg):
    if cfg in pkg.gguf_synth.CONFIGS:
        return pkg.gguf_synth.CONFIGS[cfg]
    base, n_embd, n_head, n_head_kv, n_ff = HALF_WIDTH[cfg]
    return dataclasses.replace(pkg.gguf_synth.CONFIGS[base], name=cfg, n_embd=n_embd, n_head=n_head, n_head_kv=n_head_kv, n_ff=n_ff)


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


# what the test's OWN plumbing leaves behind when it fails: the port taken between _free_port() and the bind, the gloo store / rendezvous timing out.  Nothing
# broader ("socket", "NCCL", "ProcessGroup", "Broken pipe", "Connection reset": the strings a rank's PEERS print when it segfaults or aborts in product code)
INFRA_SIGNATURES = ("Address already in use", "EADDRINUSE", "connect() timed out", "store is not available", "Timed out waiting for clients", "DistStoreError")
PRODUCT_SIGNATURES = ("bounded wait gave up", "MI355Error", "AssertionError", "assert ", "mismatch", "Segmentation fault", "core dumped", "Aborted", "hipError", "HSA_STATUS")


class RanksFailed(AssertionError):
    def __init__(self, msg, returncodes):
        super().__init__(msg)
        self.returncodes = list(returncodes)


def run_ranks(world, plan_path, out_path, timeout=600):
    """One process per rank.  A launch is repeated ONCE, and only when (1) its output carries the signature of the test's own plumbing (a port taken between
    _free_port() and the bind, the gloo store timing out), (2) none of the product's (a bounded in-kernel wait that gave up, an MI355Error, an assertion of
    tp_worker, a device error, any wrong number) and (3) NO rank was ended by a signal: a rank that segfaults or aborts makes its peers print connection
    errors, and must not buy a second run with them.  A retry is reported as a warning, so flakiness stays visible."""
    try:
        return _run_ranks_once(world, plan_path, out_path, timeout)
    except RanksFailed as e:
        msg = str(e)
        by_signal = any(rc is None or rc < 0 for rc in e.returncodes)
        if by_signal or any(k in msg for k in PRODUCT_SIGNATURES) or not any(k in msg for k in INFRA_SIGNATURES):
            raise
        import warnings
        warnings.warn(f"run_ranks: infrastructure failure, launch repeated once: {msg[-600:]}")
        return _run_ranks_once(world, plan_path, out_path, timeout)


def _run_ranks_once(world, plan_path, out_path, timeout):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(world),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = []
    for r in range(world):
        e = dict(env, RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "tp_worker.py"), plan_path, out_path],
                                      env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=timeout)
            outs.append(o)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    if os.environ.get("MI355_TP_TRACE") == "1":               # diagnosis (tools/r6_tp_coldstart.sh): every rank's [tp trace] lines, passed or not
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(ROOT, "gpurun_out", "tp_trace_" + os.path.basename(out_path) + ".log"), "a") as f:
            for r, o in enumerate(outs):
                f.write(f"==== rank {r} exit {procs[r].returncode}\n" + "\n".join(l for l in o.splitlines() if "[tp" in l or "gave up" in l or "Error" in l) + "\n")
    if any(p.returncode != 0 for p in procs):                 # (a rank that fails takes its peers' exchanges down with it: show every rank's last lines)
        tails = "\n".join(f"---- rank {r} (exit {p.returncode})\n{outs[r][-1500:]}" for r, p in enumerate(procs))
        raise RanksFailed(f"{sum(p.returncode != 0 for p in procs)} of {world} ranks failed:\n{tails}", [p.returncode for p in procs])
    return np.load(out_path)


def make_plan(pkg, tmp_models, cfg, ftype, kv, n_prompt, transport, n_steps=6, n_tail=3, seed=21, p2p_floats=0, p2p_prompt_floats=0):
    path = str(tmp_models / f"tp-{cfg}-{ftype}.gguf")
    if not os.path.exists(path):
        pkg.gguf_synth.write_synthetic_llama(path, config(pkg, cfg), ftype, seed=seed)
    om = oq.OracleModel(path)
    oc = oq.OracleContext(om, 256, KV[kv], KV[kv], True, oq.threads())
    if kv == "f16":
        oq.set_fa_v_acc_f32(1)
    rng = np.random.default_rng(5)
    prompt = rng.integers(0, om.n_vocab, n_prompt).astype(np.int32)
    ref = [oc.decode(prompt, np.arange(n_prompt))[0]]
    steps = []
    pos = n_prompt
    for _ in range(n_steps):                       # teacher-forced with the oracle's own greedy choice
        tok = int(ref[-1].argmax())
        steps.append(tok)
        ref.append(oc.decode([tok], [pos])[0])
        pos += 1
    tail = rng.integers(0, om.n_vocab, n_tail).astype(np.int32)
    ref.extend(oc.decode(tail, np.arange(pos, pos + n_tail), want_logits=np.ones(n_tail, np.int8)))
    oq.set_fa_v_acc_f32(0)
    oc.close(); om.close()
    plan_path = str(tmp_models / f"tp-plan-{cfg}-{ftype}-{kv}-{n_prompt}-{transport}-{p2p_floats}-{p2p_prompt_floats}.npz")
    np.savez(plan_path, path=path, kv=KV[kv], transport=transport, n_ctx=256, n_ubatch=64, prompt=prompt,
             steps=np.asarray(steps, np.int32), tail=tail, p2p_floats=p2p_floats, p2p_prompt_floats=p2p_prompt_floats)
    return path, plan_path, np.stack(ref)


def unsplit_logits(pkg, plan_path):
    plan = np.load(plan_path)
    m = pkg.Model(str(plan["path"]))
    c = pkg.Context(m, n_ctx=int(plan["n_ctx"]), type_k=int(plan["kv"]), type_v=int(plan["kv"]), n_ubatch=int(plan["n_ubatch"]))
    rows = []
    prompt = plan["prompt"]
    c.enable_taps(True)
    c.decode(prompt, np.arange(prompt.size))
    rows.append(c.logits())
    taps = np.stack([c.layer_out(il, prompt.size).reshape(prompt.size, -1) for il in range(m.n_layer)])
    c.enable_taps(False)
    pos = prompt.size
    for tok in plan["steps"]:
        c.decode([int(tok)], [pos]); rows.append(c.logits()); pos += 1
    tail = plan["tail"]
    c.decode(tail, np.arange(pos, pos + tail.size), logits=np.ones(tail.size))
    rows.extend(c.logits(i) for i in range(tail.size))
    heads = (m.n_head, m.n_head_kv, m.bytes_per_token)
    c.close(); m.close()
    return np.stack(rows), taps, heads


@pytest.mark.parametrize("cfg,ftype,kv,n_prompt,world", [
    ("tiny-d128", "q4_k_m", "q8_0", 8, 2),        # rows of Q4_K / Q6_K tensors, columns of Q4_K and (repacked) Q6_K
    ("tiny-d128", "q8_0", "f16", 8, 2),           # Q8_0: column slices go through the row regrouping
    ("tiny-e2048", "q5_k_m", "q8_0", 40, 2),      # 40-token prompt: the MFMA prompt path on a slice; fused prologues on the steps
    ("tiny-e2048", "q4_k_m", "q8_0", 8, 4),       # four ranks: one KV head each
    ("tiny-8b-2l", "q4_k_m", "q8_0", 8, 2),       # Llama-3-8B's layer geometry
    ("tiny-8b-half-2l", "q4_k_m", "q8_0", 8, 4),  # north_star's rank geometry: 4 query heads + 1 KV head and 1792 = 7 x 256 feed-forward columns per rank
    # BASELINE config 5's per-rank geometry (Llama-3-70B over 8 GPUs): 8 query heads on ONE kv head, attn_output columns of 1024 = 4 super-blocks, ffn_down
    # columns of 3584 = 14 super-blocks; and Llama-3-70B's own layers over 4 ranks: slices of the 28672-wide ffn_down (whose single-GPU form is two column halves)
    ("tiny-70b-half-2l", "q4_k_m", "q8_0", 8, 4),
    ("tiny-70b-2l", "q4_k_m", "q8_0", 8, 4),
])
def test_ranks_sharing_one_gpu_match_oracle_and_unsplit(pkg, tmp_models, cfg, ftype, kv, n_prompt, world):
    pkg.Backend()
    path, plan_path, ref = make_plan(pkg, tmp_models, cfg, ftype, kv, n_prompt, "host")
    out_path = str(tmp_models / f"tp-out-{cfg}-{ftype}-{world}.npz")
    got = run_ranks(world, plan_path, out_path)
    one, taps_one, (H, G, bpt) = unsplit_logits(pkg, plan_path)
    assert int(got["n_head"]) * world == H and int(got["n_head_kv"]) * world == G
    # a rank streams its share of the projections (+ the norms and one embedding row, which every rank reads)
    assert bpt / world <= int(got["bytes_per_token"]) <= bpt / world * 1.02 + (1 << 16)
    lg = got["logits"]
    assert lg.shape == ref.shape == one.shape
    errs_ref = [rel_err(a, b) for a, b in zip(lg, ref)]
    errs_one = [rel_err(a, b) for a, b in zip(lg, one)]
    assert max(errs_ref) <= FLIP_TOL, errs_ref
    assert max(errs_one) <= FLIP_TOL, errs_one
    # Against the unsplit HIP run only the order of the f32 sums differs (partial sums per rank, attention splits per
    # head count).  Where no int8 / f16 rounding flips, the two agree to round-off: some logits row does, or — when a flip in
    # the prompt's first layers lands in the KV cache and stays — most prompt tokens after the first layer do.
    tok_err0 = np.abs(got["taps"][0] - taps_one[0]).max(axis=1) / max(1.0, float(np.abs(taps_one[0]).max()))
    assert min(errs_one) <= TIGHT_TOL or float(np.median(tok_err0)) <= TIGHT_TOL, (errs_one, tok_err0)
    if kv != "f16":      # (f16 K / V rows round every element once more: never flip-free against the CPU restatement)
        assert min(errs_ref) <= TIGHT_TOL or float(np.median(tok_err0)) <= TIGHT_TOL, (errs_ref, tok_err0)
    # greedy ids agree with the oracle wherever the oracle's own top-2 margin exceeds the tolerance
    for a, b in zip(lg, ref):
        top = np.sort(b)[-2:]
        if top[1] - top[0] > 2 * FLIP_TOL * max(1.0, np.abs(b).max()):
            assert int(a.argmax()) == int(b.argmax())


@pytest.mark.parametrize("cfg,ftype,kv,world", [("tiny-e2048", "q4_k_m", "q8_0", 2), ("tiny-8b-2l", "q4_k_m", "q8_0", 2), ("tiny-e2048", "q4_k_m", "q8_0", 4), ("tiny-70b-half-2l", "q4_k_m", "q8_0", 4)])
def test_peer_to_peer_all_reduce_matches_the_host_exchange(pkg, tmp_models, cfg, ftype, kv, world):
    """The one-shot peer-to-peer all-reduce (host/tp_comm.cc: every rank writes its partial into slot `rank` of every rank's IPC-mapped buffer, flags,
    rank-order sum) takes the decode-sized exchanges; the prompt batch and the logits gather keep the host transport.  IPC mapping works between
    processes that share the one GPU of this box (the xGMI path itself needs a multi-GPU node).  Two ranks: p0 + p1 is the same sum in either
    transport, so every logits row is bit-identical to the pure host-exchange run; four ranks: the rank-order sum differs from gloo's by re-association
    only - oracle bound, and the same bits on a second run."""
    pkg.Backend()
    E = config(pkg, cfg).n_embd
    path, plan_host, ref = make_plan(pkg, tmp_models, cfg, ftype, kv, 8, "host")
    _, plan_p2p, _ = make_plan(pkg, tmp_models, cfg, ftype, kv, 8, "host", p2p_floats=4 * E)
    host = run_ranks(world, plan_host, str(tmp_models / f"tp-out-host-{cfg}-{world}.npz"))
    p2p = run_ranks(world, plan_p2p, str(tmp_models / f"tp-out-p2p-{cfg}-{world}.npz"))
    n_layer = config(pkg, cfg).n_layer
    assert int(host["p2p_exchanges"]) == 0
    assert int(p2p["p2p_exchanges"]) >= 2 * n_layer * 6            # the six single-token steps (and the three-token tail: 3 E <= 4 E)
    errs = [rel_err(a, b) for a, b in zip(p2p["logits"], ref)]
    assert max(errs) <= FLIP_TOL, errs
    if world == 2:
        assert np.array_equal(p2p["logits"], host["logits"])
    else:
        again = run_ranks(world, plan_p2p, str(tmp_models / f"tp-out-p2p2-{cfg}-{world}.npz"))
        assert np.array_equal(p2p["logits"], again["logits"])
        assert max(rel_err(a, b) for a, b in zip(p2p["logits"], host["logits"])) <= FLIP_TOL


@pytest.mark.parametrize("cfg,ftype,kv,world,wgs", [("tiny-e2048", "q4_k_m", "q8_0", 2, 0), ("tiny-8b-2l", "q4_k_m", "q8_0", 2, 7), ("tiny-e2048", "q4_k_m", "q8_0", 4, 0),
                                                    ("tiny-e2048", "q5_k_m", "f16", 4, 5), ("tiny-8b-half-2l", "q4_k_m", "q8_0", 4, 0), ("tiny-70b-half-2l", "q4_k_m", "q8_0", 4, 0)])
def test_prompt_sized_exchange_as_reduce_scatter_all_gather(pkg, tmp_models, cfg, ftype, kv, world, wgs, monkeypatch):
    """Prompt batches: the n_embd x n_ubatch partial sums go through ONE reduce-scatter + all-gather kernel (host/tp_comm.cc p2p_rsag_kernel:
    a segment per rank, every rank stores its part of segment q into rank q's IPC-mapped buffer, the owner adds in rank order and stores the sum
    into everybody's buffer) instead of the base transport.  A 100-token prompt in micro-batches of 64 = messages of 64 E and 36 E floats, twice
    per layer; the single-token steps keep the one-shot kernel.  Two ranks: bit-identical to the pure host-exchange run (p0 + p1 either way);
    four ranks: the rank-order sum is the one-shot kernel's association - oracle bound, the host run within the flip tolerance, the same bits
    again on a second run.  `wgs` cuts the segments into an odd number of slices (ragged last slice)."""
    pkg.Backend()
    if wgs:
        monkeypatch.setenv("MI355_TP_RSAG_WGS", str(wgs))
    C_ = config(pkg, cfg)
    E, n_layer = C_.n_embd, C_.n_layer
    path, plan_host, ref = make_plan(pkg, tmp_models, cfg, ftype, kv, 100, "host")
    _, plan_rs, _ = make_plan(pkg, tmp_models, cfg, ftype, kv, 100, "host", p2p_floats=4 * E, p2p_prompt_floats=64 * E)
    host = run_ranks(world, plan_host, str(tmp_models / f"tp-out-host100-{cfg}-{ftype}-{world}.npz"))
    rs = run_ranks(world, plan_rs, str(tmp_models / f"tp-out-rsag-{cfg}-{ftype}-{world}.npz"))
    assert int(host["p2p_prompt_exchanges"]) == 0
    assert int(rs["p2p_prompt_exchanges"]) == 2 * n_layer * 2         # two micro-batches
    assert int(rs["p2p_exchanges"]) >= 2 * n_layer * 6
    errs = [rel_err(a, b) for a, b in zip(rs["logits"], ref)]
    assert max(errs) <= FLIP_TOL, errs
    if world == 2:
        assert np.array_equal(rs["logits"], host["logits"])
        assert np.array_equal(rs["taps"], host["taps"])
    else:
        again = run_ranks(world, plan_rs, str(tmp_models / f"tp-out-rsag2-{cfg}-{ftype}-{world}.npz"))
        assert np.array_equal(rs["logits"], again["logits"])
        assert np.array_equal(rs["taps"], again["taps"])
        assert max(rel_err(a, b) for a, b in zip(rs["logits"], host["logits"])) <= FLIP_TOL


def test_reduce_scatter_case_in_a_fresh_process():
    """The reduce-scatter + all-gather case of BASELINE config 5's per-rank geometry (it ran over 8 ranks until the shared device's process limit; see
    HALF_WIDTH) as the FIRST and ONLY multi-rank test of its own pytest process (it runs in file order as well): its colour must not depend on what ran
    before it (it was red whenever it ran alone - cold box or warm - and green in file order).  Round 6 found two causes, neither in the exchange kernel:
    the ranks of this rig reached their first exchange seconds apart (nothing stepped them in lock-step: tests/tp_worker.py now meets at a barrier, as a row
    split's driver does), and the one-launch attention + attn_output kernel - workgroups that wait for each other - ran in eight processes on ONE device
    (host/runtime.cc keeps it off now where the ranks exchange through the host callback, i.e. share a device).  profiles/r6_tp_shared_device_trace.txt."""
    case = "tests/test_gpu_tp.py::test_prompt_sized_exchange_as_reduce_scatter_all_gather[tiny-70b-half-2l-q4_k_m-q8_0-4-0]"
    r = subprocess.run([sys.executable, "-m", "pytest", case, "-x", "-q", "-p", "no:cacheprovider"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    assert "1 passed" in r.stdout


def test_rccl_group_of_one_captured_in_graphs_is_bit_identical(pkg, tmp_models):
    pkg.Backend()
    path, plan_path, ref = make_plan(pkg, tmp_models, "tiny-e2048", "q4_k_m", "q8_0", 8, "rccl", n_steps=12)
    out_path = str(tmp_models / "tp-out-rccl1.npz")
    got = run_ranks(1, plan_path, out_path)
    one, taps_one, _ = unsplit_logits(pkg, plan_path)
    assert np.array_equal(got["logits"], one)
    assert np.array_equal(got["taps"], taps_one)
