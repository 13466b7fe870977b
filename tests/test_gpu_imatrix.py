"""Importance-matrix collection on the device (Context.imatrix_* behind mi355_imatrix_*, csrc/imatrix.hip) on tiny synthetic files: the entry set, the
counts, the sums against the device's own layer taps and against the reference collector of tests/imatrix_ref.py; small batches, where the fused
single-token launches, the engine and the captured graphs must stand aside; mixture-of-experts files per expert with the reference's routes forced, as one
batch and with single-token steps; a micro-batch size whose full batch needs fewer slabs than a smaller one; the
lifecycle (begin / clear / end, the steps before and after); and tools/imatrix.py in a child process.

Largest rel_err(device, reference) over every entry of every case below on the first GPU run: 4.5e-2 (tiny-qwen3moe, 5 tokens, q8_0 cache; 3.9e-2 and 3.1e-2
at 40 tokens), which is within a factor of four of the bound 2 * FLIP_TOL = 6e-2; the dense files stay at or below 8.9e-3 (tiny-qwen3), tiny-moe at 1.3e-3
(DESIGN.md §4.11)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import imatrix_cases as ic
import oracle_py as oq
from gguf_read import read_gguf
from imatrix_ref import ImatrixMoeRef, ImatrixRef

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = ic.N_PROMPT
N_CTX = 128


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


@pytest.fixture(scope="module")
def refs(pkg, tmp_models):
    """(cfg, ftype, kv, T) -> (path, tokens, flags, reference entries, routes or None): each reference pass runs once and is shared, unchanged"""
    cache = {}

    def get(cfg, ftype, kv, T=N, moe=False):
        key = (cfg, ftype, kv, T)
        if key not in cache:
            path = ic.model_file(pkg, tmp_models, cfg, ftype)
            n_vocab = read_gguf(path)[1]["token_embd.weight"][0][1]
            toks, flags = ic.prompt_tokens(n_vocab)[:T], ic.head_flags()[:T].copy()
            flags[-1] = 1
            oq.set_fa_v_acc_f32(1 if kv == "f16" else 0)
            try:
                ref = (ImatrixMoeRef if moe else ImatrixRef)(path, N_CTX, ic.KV[kv], ic.KV[kv])
                ref.decode(toks, np.arange(T), want=flags)
            finally:
                oq.set_fa_v_acc_f32(0)
            cache[key] = (path, toks, flags, ref.im, ref.routes[-1] if moe else None)
        return cache[key]
    return get


def collect(c, toks, flags, splits, process_output=True, routes=None):
    """the tokens in consecutive decode calls of the given sizes from an empty cache, collection on: the entries"""
    c.kv_clear()
    c.imatrix_begin(process_output)
    i = 0
    for n in splits:
        if routes is not None:
            c.force_moe_ids(routes[:, i:i + n])                   # (the hook takes the next call's tokens)
        assert c.decode(toks[i:i + n], np.arange(i, i + n), logits=flags[i:i + n]) == 0
        i += n
    assert i == toks.size
    return c.imatrix_entries()


def check_counts_and_reference(entries, ref_im, path, n_tokens, n_flagged, tag):
    want = ic.expected_names(path, True)
    assert set(entries) == set(want) == set(ref_im), (sorted(set(entries) ^ set(want)), tag)
    worst = 0.0
    for name, (s, c) in entries.items():
        ne0, n_mat = want[name]
        assert s.shape == (n_mat, ne0) and c.shape == (n_mat,), name
        head = not name.startswith("blk.")
        rs, rc = ref_im[name]
        if n_mat == 1:
            assert c.tolist() == [n_flagged if head else n_tokens], (name, c)
        assert c.tolist() == rc.tolist(), name
        for m in range(n_mat):
            if c[m] == 0:
                assert not s[m].any(), (name, m)
                continue
            e = ic.rel_err(s[m].astype(np.float64), rs[m])
            worst = max(worst, e)
            assert e <= 2 * ic.FLIP_TOL, (tag, name, m, e)
    return worst


# ------------------------------------------------------------------------------------------------ dense files
@pytest.mark.parametrize("kv", ["q8_0", "f16"])
@pytest.mark.parametrize("cfg,ftype", ic.DENSE_FILES)
def test_dense_entries_counts_taps_and_reference(be, pkg, refs, cfg, ftype, kv):
    path, toks, flags, ref_im, _ = refs(cfg, ftype, kv)
    gkv, gt = read_gguf(path)
    arch = gkv["general.architecture"]
    eps = gkv[f"{arch}.attention.layer_norm_rms_epsilon"]
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=N_CTX, type_k=ic.KV[kv], type_v=ic.KV[kv])
    # (a) without process_output the head has no entry
    plain = collect(c, toks, flags, [N], process_output=False)
    assert set(plain) == set(ic.expected_names(path, False))
    c.imatrix_end()
    c.enable_taps(True)
    entries = collect(c, toks, flags, [N])
    taps = [c.layer_out(il, N).astype(np.float64) for il in range(m.n_layer)]
    c.imatrix_end()
    c.enable_taps(False)
    # (a), (b), (d)
    worst = check_counts_and_reference(entries, ref_im, path, N, int(flags.sum()), (cfg, kv))
    assert np.array_equal(plain["blk.0.attn_q.weight"][0], entries["blk.0.attn_q.weight"][0])          # (the same bits run to run, taps or not)
    # (c) against the device's own taps
    def normed(x, w):
        return x / np.sqrt((x * x).mean(axis=1, keepdims=True) + eps) * gt[w][2].view("<f4").astype(np.float64)
    worst_tap = 0.0
    for il in range(1, m.n_layer):
        want = (normed(taps[il - 1], f"blk.{il}.attn_norm.weight") ** 2).sum(axis=0)
        got = entries[f"blk.{il}.attn_q.weight"][0][0]
        worst_tap = max(worst_tap, float((np.abs(got - want) / want).max()))
        assert (np.abs(got - want) <= ic.tap_bound(want, N)).all(), (il, float((np.abs(got - want) / want).max()))
        for other in ("attn_k", "attn_v"):
            assert entries[f"blk.{il}.{other}.weight"][0].tobytes() == entries[f"blk.{il}.attn_q.weight"][0].tobytes()
        assert entries[f"blk.{il}.ffn_up.weight"][0].tobytes() == entries[f"blk.{il}.ffn_gate.weight"][0].tobytes()
    head = "output.weight" if "output.weight" in gt else "token_embd.weight"
    rows = np.flatnonzero(flags)
    want = (normed(taps[-1][rows], "output_norm.weight") ** 2).sum(axis=0)
    got = entries[head][0][0]
    assert (np.abs(got - want) <= ic.tap_bound(want, rows.size)).all(), float((np.abs(got - want) / want).max())
    print(f"{cfg} {ftype} kv {kv}: largest rel_err against the reference {worst:.3g} (bound {2 * ic.FLIP_TOL:.3g}); against the taps {worst_tap:.3g} "
          f"(bound {2 * ic.NORM_REL + (N + 4) * ic.U:.3g})")
    c.close(); m.close()


SPLITS = {"steps": [32] + [1] * 8, "3+37": [3, 37], "ubatch16": [N]}


@pytest.mark.parametrize("mode", list(SPLITS))
@pytest.mark.parametrize("kv", ["q8_0", "f16"])
@pytest.mark.parametrize("cfg,ftype", ic.DENSE_FILES)
def test_dense_small_batches(be, pkg, refs, cfg, ftype, kv, mode):
    """The same 40 tokens as a 32-token prompt and eight single-token steps, as 3 + 37, and in micro-batches of 16: the counts are the tokens run and the
    sums meet the reference as the one batch does - a step that had taken a fused single-token launch, the engine or a graph would have collected nothing.
    Both caches: on the f16 cache a single-token step takes other attention launches and another attn_output form."""
    path, toks, flags, ref_im, _ = refs(cfg, ftype, kv)
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=N_CTX, n_ubatch=16 if mode == "ubatch16" else 512, type_k=ic.KV[kv], type_v=ic.KV[kv])
    # (steps before collection starts: a captured single-token step exists and must not be replayed while collecting)
    assert c.decode(toks[:4], np.arange(4)) == 0
    for i in range(3):
        assert c.decode([int(toks[4 + i])], [4 + i]) == 0
    k0 = (c.mega_steps(), c.engine_steps(), c.qkv_attn_launches())
    entries = collect(c, toks, flags, SPLITS[mode])
    assert (c.mega_steps(), c.engine_steps(), c.qkv_attn_launches()) == k0
    c.imatrix_end()
    worst = check_counts_and_reference(entries, ref_im, path, N, int(flags.sum()), (cfg, kv, mode))
    print(f"{cfg} kv {kv} {mode}: largest rel_err against the reference {worst:.3g}")
    c.close(); m.close()


# ------------------------------------------------------------------------------------------------ mixture-of-experts files
@pytest.mark.parametrize("T", ic.MOE_TS)
@pytest.mark.parametrize("kv", ["q8_0", "f16"])
@pytest.mark.parametrize("cfg,ftype", ic.MOE_FILES)
def test_moe_per_expert(be, pkg, refs, cfg, ftype, kv, T):
    path, toks, flags, ref_im, routes = refs(cfg, ftype, kv, T, moe=True)
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=N_CTX, type_k=ic.KV[kv], type_v=ic.KV[kv])
    c.profile(True)
    entries = collect(c, toks, flags, [T], routes=routes)
    roles = c.last_profile()
    c.imatrix_end()
    # which grouped form fed ffn_down_exps: the one-launch form leaves silu(gate) * up itself and is collected plainly ("imatrix"); the others leave gate and
    # up and are collected through the SwiGLU producer ("imatrix_glu").  Both files qualify for the one-launch form (Q4_K / Q6_K expert tensors, row counts
    # multiples of 128, row lengths of 256), which takes batches from 32 tokens on.
    assert "imatrix" in roles and ("imatrix_glu" in roles) == (T < 32), (T, sorted(roles))
    worst = check_counts_and_reference(entries, ref_im, path, T, int(flags.sum()), (cfg, kv, T))
    n_layer, _, k = routes.shape
    for il in range(n_layer):
        n_expert = entries[f"blk.{il}.ffn_down_exps.weight"][1].size
        hist = np.bincount(routes[il].reshape(-1), minlength=n_expert)
        for stem in ("ffn_gate_exps", "ffn_up_exps", "ffn_down_exps"):
            cnt = entries[f"blk.{il}.{stem}.weight"][1]
            assert cnt.tolist() == hist.tolist() and int(cnt.sum()) == T * k, (il, stem)
        assert entries[f"blk.{il}.ffn_gate_exps.weight"][0].tobytes() == entries[f"blk.{il}.ffn_up_exps.weight"][0].tobytes()
        assert entries[f"blk.{il}.ffn_gate_inp.weight"][1].tolist() == [T]
    print(f"{cfg} kv {kv} T {T}: largest rel_err against the reference {worst:.3g}")
    c.close(); m.close()


@pytest.mark.parametrize("kv", ["q8_0", "f16"])
@pytest.mark.parametrize("cfg,ftype", ic.MOE_FILES)
def test_moe_single_token_steps(be, pkg, refs, cfg, ftype, kv):
    """The 40 tokens as a 37-token prompt and three single-token steps: a step groups T = 1, GR = k rows (without collection it would take the selected-experts
    launches, which leave no per-expert rows), and the per-expert counts and sums are those of the one batch."""
    path, toks, flags, ref_im, routes = refs(cfg, ftype, kv, N, moe=True)
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=N_CTX, type_k=ic.KV[kv], type_v=ic.KV[kv])
    assert c.decode(toks[:4], np.arange(4)) == 0                      # (a captured single-token step exists before collection starts)
    assert c.decode([int(toks[4])], [4]) == 0
    k0 = (c.mega_steps(), c.engine_steps(), c.qkv_attn_launches())
    c.profile(True)
    entries = collect(c, toks, flags, [N - 3, 1, 1, 1], routes=routes)
    roles = c.last_profile()                                          # of the last step
    c.profile(False)
    assert (c.mega_steps(), c.engine_steps(), c.qkv_attn_launches()) == k0
    c.imatrix_end()
    assert "imatrix" in roles and "imatrix_glu" in roles, sorted(roles)
    worst = check_counts_and_reference(entries, ref_im, path, N, int(flags.sum()), (cfg, kv, "steps"))
    for il in range(routes.shape[0]):
        hist = np.bincount(routes[il].reshape(-1), minlength=entries[f"blk.{il}.ffn_down_exps.weight"][1].size)
        for stem in ("ffn_gate_exps", "ffn_up_exps", "ffn_down_exps"):
            assert entries[f"blk.{il}.{stem}.weight"][1].tolist() == hist.tolist(), (il, stem)
    print(f"{cfg} kv {kv} 37 + 3 x 1: largest rel_err against the reference {worst:.3g}")
    c.close(); m.close()


def test_scratch_holds_a_smaller_batch_with_more_slices(be, pkg, tmp_models):
    """n_ubatch 600 (slices of 10 rows: 60 slabs) and a 512-token batch (slices of 8: 64 slabs), and on a mixture-of-experts file n_ubatch 65 with a 64-token
    batch (520 against 512 grouped rows): the slab count is not monotone in the rows, and the scratch sized at begin must hold the smaller batch's slabs.  The
    same batch on a context of n_ubatch 512 (64), where the batch is the largest launch, gives the same bits."""
    for cfg, T, ub in (("tiny", 512, 600), ("tiny-moe", 64, 65)):
        path = ic.model_file(pkg, tmp_models, cfg, "q4_k_m")
        m = pkg.Model(path)
        toks = ic.prompt_tokens(m.n_vocab, T, seed=77)
        flags = np.zeros(T, np.int8)
        flags[-1] = 1
        got = []
        for n_ubatch in (ub, T):
            c = pkg.Context(m, n_ctx=T, n_batch=ub, n_ubatch=n_ubatch, type_k=ic.KV["q8_0"], type_v=ic.KV["q8_0"])
            got.append(collect(c, toks, flags, [T]))
            c.imatrix_end()
            c.close()
        assert list(got[0]) == list(got[1])
        for name in got[0]:
            assert got[0][name][1].tolist() == got[1][name][1].tolist() and int(got[0][name][1].sum()) in (1, T, T * 2), name
            assert got[0][name][0].tobytes() == got[1][name][0].tobytes(), name
        m.close()


@pytest.mark.parametrize("T", ic.MOE_TS)
def test_moe_160_experts_shapes_and_counts(be, pkg, tmp_models, T):
    cfg, ftype = ic.MOE_SHAPES_ONLY
    path = ic.model_file(pkg, tmp_models, cfg, ftype)
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=N_CTX, type_k=ic.KV["q8_0"], type_v=ic.KV["q8_0"])
    rng = np.random.default_rng(160 + T)
    NE, k = 160, 8
    routes = np.stack([np.stack([rng.permutation(NE)[:k] for _ in range(T)]) for _ in range(m.n_layer)]).astype(np.int32)
    toks, flags = ic.prompt_tokens(m.n_vocab)[:T], np.zeros(T, np.int8)
    flags[-1] = 1
    entries = collect(c, toks, flags, [T], routes=routes)
    c.imatrix_end()
    want = ic.expected_names(path, True)
    assert set(entries) == set(want)
    for name, (s, cnt) in entries.items():
        assert s.shape == (want[name][1], want[name][0]) and np.isfinite(s).all(), name
    for il in range(m.n_layer):
        hist = np.bincount(routes[il].reshape(-1), minlength=NE)
        for stem in ("ffn_gate_exps", "ffn_up_exps", "ffn_down_exps"):
            s, cnt = entries[f"blk.{il}.{stem}.weight"]
            assert cnt.tolist() == hist.tolist() and int(cnt.sum()) == T * k
            assert not s[hist == 0].any() and (s[hist > 0].sum(axis=1) > 0).all()
    c.close(); m.close()


# ------------------------------------------------------------------------------------------------ lifecycle
def test_lifecycle_and_neutrality(be, pkg, tmp_models):
    """tiny-d128 with a q8_0 cache takes the one-launch attention block and captured steps.  Before begin and after end the logits of a prompt and of single
    steps are the same bits and the step counters advance alike; between them no counter moves, the logits stay within FLIP_TOL, clear zeroes, a second begin
    is an error, and the accumulators are device memory of the context only while collection is on.  An encoder is refused."""
    path = ic.model_file(pkg, tmp_models, "tiny-d128", "q4_k_m")
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=64, type_k=ic.KV["q8_0"], type_v=ic.KV["q8_0"])
    n = 9
    prompt = ic.prompt_tokens(m.n_vocab, n, seed=3)
    counters = lambda: np.array([c.mega_steps(), c.engine_steps(), c.qkv_attn_launches()])
    dev_bytes = lambda: int(c.lib.mi355_context_device_bytes(c.h))

    def run():
        c.kv_clear()
        k0 = counters()
        assert c.decode(prompt, np.arange(n)) == 0
        rows = [c.logits()]
        for i in range(3):
            assert c.decode([5 + i], [n + i]) == 0
            rows.append(c.logits())
        return np.stack(rows), counters() - k0

    before, k_before = run()
    assert k_before[2] > 0                                            # (the one-launch attention block does run here)
    with pytest.raises(pkg.binding.MI355Error, match="not on"):
        c.imatrix_end()
    b0 = dev_bytes()
    c.imatrix_begin(True)
    assert dev_bytes() > b0
    with pytest.raises(pkg.binding.MI355Error, match="already on"):
        c.imatrix_begin(False)
    assert dev_bytes() > b0
    during, k_during = run()
    assert not k_during.any()
    assert ic.rel_err(during, before) <= ic.FLIP_TOL
    e = c.imatrix_entries()
    assert all(cnt.tolist() == [4 if not name.startswith("blk.") else n + 3] for name, (_, cnt) in e.items())
    assert all(s.any() for s, _ in e.values())
    c.imatrix_clear()
    assert all(not s.any() and not cnt.any() for s, cnt in c.imatrix_entries().values())
    assert c.decode([9], [n + 3]) == 0                                # still collecting after clear
    assert all(cnt.tolist() == [1] for _, cnt in c.imatrix_entries().values())
    c.imatrix_end()
    assert dev_bytes() == b0
    assert c.imatrix_entries() == {}
    after, k_after = run()
    assert after.tobytes() == before.tobytes()
    assert k_after.tolist() == k_before.tolist()
    c.close(); m.close()
    enc = ic.model_file(pkg, tmp_models, "tiny-nomic", "f16")
    me = pkg.Model(enc)
    ce = pkg.Context(me, n_ctx=64)
    with pytest.raises(pkg.binding.MI355Error, match="encoder"):
        ce.imatrix_begin(False)
    ce.close(); me.close()


# ------------------------------------------------------------------------------------------------ the tool
def test_the_tool_in_child_processes(be, pkg, tmp_models, tmp_path):
    """tools/imatrix.py --tokens on `tiny`, 3 chunks of 64, as .gguf and as .dat: read back through the tool's readers the files hold what
    Context.imatrix_entries() gives after the same calls; with --in-file of its own output the sums and counts are doubled."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("imatrix_tool", os.path.join(ROOT, "tools", "imatrix.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    path = ic.model_file(pkg, tmp_models, "tiny", "q4_k_m")
    tokens = ic.prompt_tokens(512, 3 * 64 + 10, seed=9)
    tok_path = str(tmp_path / "tokens.npy")
    np.save(tok_path, tokens)

    def run_tool(out, *more):
        cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tools", "imatrix.py"), "-m", path, "--tokens", tok_path, "--ctx", "64", "--ubatch", "32",
               "--cache-type", "q8_0", "-o", out, "--json", out + ".json", *more]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout, json.load(open(out + ".json"))

    g, d, g2 = str(tmp_path / "a.gguf"), str(tmp_path / "a.dat"), str(tmp_path / "b.gguf")
    stdout, info = run_tool(g)
    assert "[1]" in stdout and "[3]" in stdout and "[4]" not in stdout and "PPL = " in stdout and info["n_chunks"] == 3
    run_tool(d)
    run_tool(g2, "--in-file", g)
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=64, n_batch=32, n_ubatch=32, type_k=ic.KV["q8_0"], type_v=ic.KV["q8_0"], logits_to_host=False)      # the tool's context
    c.imatrix_begin(False)
    c.perplexity(tokens, 64, bos=info["bos"])
    want = c.imatrix_entries()
    c.imatrix_end()
    c.close(); m.close()
    assert set(want) == set(ic.expected_names(path, False))
    fg, fd, fg2 = tool.read_imatrix(g), tool.read_imatrix(d), tool.read_imatrix(g2)
    assert fg.chunk_count == 3 and fg.chunk_size == 64 and fg.datasets == ["tokens.npy"] and fd.chunk_count == 3 and fg2.chunk_count == 6
    assert list(fg.entries) == list(want) == list(fd.entries)
    for name, (s, cnt) in want.items():
        assert cnt.tolist() == [3 * 64]
        assert fg.entries[name][0].tobytes() == s.tobytes() and fg.entries[name][1].tolist() == [3 * 64], name
        assert fd.entries[name][0].reshape(-1).tobytes() == tool.dat_values(s, cnt, 3).tobytes() and fd.entries[name][1].tolist() == [3], name
        assert np.array_equal(fg2.entries[name][0], (2.0 * s.astype(np.float64)).astype(np.float32)) and fg2.entries[name][1].tolist() == [2 * 3 * 64], name
