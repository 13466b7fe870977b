"""general.architecture "qwen3moe" on the GPU: the wave-parallel router for up to 256 experts (mi355_op_moe_router, op by op against a numpy restatement of
its arithmetic), and qwen3moe files end to end against the composed reference of tests/qwen3moe_ref.py - per-layer taps, logits and greedy ids with the
reference's expert selections handed to the device (force_moe_ids), prompt batches in each of the three expert forms, the 8-expert single-token step,
batched steps, the engine, and the refusals."""
import dataclasses
import os

import numpy as np
import pytest

import oracle_py as oq
from qwen3moe_ref import Qwen3MoeRef, selection_numpy
from test_gpu_qwen3 import _need_experiments

pytestmark = pytest.mark.gpu

KV = {"f16": 1, "q8_0": 8, "q4_0": 2}
# the end-to-end tolerances of tests/test_gpu_model.py and tests/test_gpu_qwen3.py: every layer and step within FLIP_TOL
FLIP_TOL = 3e-2
TIGHT_TOL = 2e-5         # two forms of one launch sequence: f32 round-off on most tokens (tests/test_gpu_model.py)
F32, F16 = 0, 1


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def make(pkg, tmp_models, cfg, ftype, seed=13):          # (seed 13: tests/test_gpu_qwen3.py writes a dense "tiny-qwen3moe" with seed 11 into the same directory)
    name = cfg if isinstance(cfg, str) else cfg.name
    path = str(tmp_models / f"{name}-{ftype}-{seed}.gguf")
    if not os.path.exists(path):
        pkg.gguf_synth.write_synthetic_llama(path, cfg, ftype, seed=seed)
    return path


# ------------------------------------------------------------------------------------------------ op level
def kernel_selection(lg: np.ndarray, k: int, forced=None):
    """The router kernel's arithmetic in numpy on one token's logits: mx, p = exp(lg - mx) in f32, the double sum in expert order, inv = f32(1 / sum),
    p *= inv, first-max picks, f32 renormalisation in rank order."""
    lg = lg.astype(np.float32)
    p = np.exp(lg - lg.max()).astype(np.float32)
    s = 0.0
    for v in p:
        s += float(v)
    p = (p * np.float32(1.0 / s)).astype(np.float32)
    return selection_numpy(p, k, forced)


@pytest.mark.parametrize("n_expert", [8, 60, 64, 65, 128, 160, 256])
@pytest.mark.parametrize("t", [F32, F16])
def test_moe_router_op(be, n_expert, t):
    """The fused router (gate_inp . x, then the wave-parallel selection) at 1 .. 256 experts and k = 1, 2, 4, 8: logits bit-equal to the two-launch form
    (mmv_float, then the selection on its logits), ids and weights bit-equal between the two; ids equal to the numpy restatement of the kernel's arithmetic
    and weights within a few ulp of it (the device expf is not libm's), with constructed ties going to the lower expert index."""
    K, T = 2048, 7
    rng = np.random.default_rng(n_expert * 2 + t)
    W = (rng.standard_normal((n_expert, K)) * 0.05).astype(np.float32 if t == F32 else np.float16)
    x = rng.standard_normal((T, K)).astype(np.float32)
    # ties: token 1's logits are those of token 0 (same x); expert rows duplicated (experts 1 and n - 1 copy expert 0; expert 3 copies expert 2) give equal
    # logits inside a token, so equal probabilities
    x[1] = x[0]
    W[n_expert - 1] = W[0]
    W[1] = W[0]
    if n_expert > 3:
        W[3] = W[2]
    x[2] = 0.0                                                     # every logit 0: all experts tie, the k lowest indices win
    for k in (1, 2, 4, 8):
        lg1, ids1, w1 = be.moe_router(t, W, n_expert, K, x, k, fused=True)
        lg2, ids2, w2 = be.moe_router(t, W, n_expert, K, x, k, fused=False)
        assert lg1.view(np.uint32).tolist() == lg2.view(np.uint32).tolist()
        assert (ids1 == ids2).all() and w1.view(np.uint32).tolist() == w2.view(np.uint32).tolist(), k
        # the logits themselves: a double-accumulated dot product, against float64
        Wf = W.astype(np.float64)
        xf = x.astype(np.float16).astype(np.float64) if t == F16 else x.astype(np.float64)
        assert np.abs(lg1 - xf @ Wf.T).max() <= 1e-5 * max(1.0, float(np.abs(lg1).max()))
        for tk in range(T):
            ids_r, w_r = kernel_selection(lg1[tk], k)
            assert (ids1[tk] == ids_r).all(), (k, tk, ids1[tk], ids_r)
            assert np.abs(w1[tk] - w_r).max() <= 4e-7 * max(1.0, float(w_r.max())), (k, tk)
            assert len(set(ids1[tk].tolist())) == k
            assert abs(float(w1[tk].astype(np.float64).sum()) - 1.0) <= 1e-6
        assert (ids1[1] == ids1[0]).all() and (w1[1] == w1[0]).all()
        assert ids1[2].tolist() == list(range(k)) and (w1[2] == w1[2][0]).all()
        # a duplicated expert that is picked is picked at the lower index first
        for tk in range(T):
            row = ids1[tk].tolist()
            for a, b in ((0, 1), (0, n_expert - 1), (2, 3)):
                if b < n_expert and b in row and a != b:
                    assert a in row and row.index(a) < row.index(b), (tk, row)


@pytest.mark.parametrize("n_expert,k", [(64, 2), (128, 8), (256, 8), (160, 4)])
def test_moe_router_forced(be, n_expert, k):
    """The forced-routing hook at up to 256 experts: the ids handed over (out-of-range ones clamped), the weights this side's probabilities of them,
    renormalised - in the fused and the two-launch form alike."""
    K, T = 1024, 5
    rng = np.random.default_rng(n_expert + k)
    W = (rng.standard_normal((n_expert, K)) * 0.05).astype(np.float32)
    x = rng.standard_normal((T, K)).astype(np.float32)
    forced = np.stack([rng.permutation(n_expert)[:k] for _ in range(T)]).astype(np.int32)
    forced[0, 0] = n_expert + 40                                   # clamped to n_expert - 1
    forced[1, -1] = -3                                             # clamped to 0
    for fused in (True, False):
        lg, ids, w = be.moe_router(F32, W, n_expert, K, x, k, fused=fused, forced=forced)
        for tk in range(T):
            ids_r, w_r = kernel_selection(lg[tk], k, forced[tk])
            assert (ids[tk] == ids_r).all(), (fused, tk)
            assert np.abs(w[tk] - w_r).max() <= 4e-7, (fused, tk)
        assert ids[0, 0] == n_expert - 1 and ids[1, -1] == 0


@pytest.mark.parametrize("n_expert,k", [(8, 2), (60, 4), (64, 8)])
def test_moe_route_matches_oracle_route(be, n_expert, k):
    """mi355_op_moe_route where oq_moe_route applies (at most 64 experts): the same ids, weights within the expf difference; and the route op equals the
    fused router's selection on the same logits bit for bit."""
    rng = np.random.default_rng(n_expert * 3 + k)
    lg = (rng.standard_normal((40, n_expert)) * 2).astype(np.float32)
    lg[5] = np.round(lg[5])
    ids, w = be.moe_route(lg, k)
    for t in range(lg.shape[0]):
        a_ids, a_w = oq.moe_route(lg[t], k)
        assert (ids[t] == a_ids).all(), t
        assert np.abs(w[t] - a_w).max() <= 4e-7
    # the logits of an f32 identity router are the rows themselves: the two entry points select on the same numbers
    K = 256
    W = np.zeros((n_expert, K), np.float32)
    W[np.arange(n_expert), np.arange(n_expert)] = 1.0
    x = np.zeros((lg.shape[0], K), np.float32)
    x[:, :n_expert] = lg
    lg2, ids2, w2 = be.moe_router(F32, W, n_expert, K, x, k)
    assert (lg2 == lg).all() and (ids2 == ids).all() and w2.view(np.uint32).tolist() == w.view(np.uint32).tolist()


def test_moe_router_refuses_bad_shapes(be, pkg):
    W = np.zeros((257, 256), np.float32)
    x = np.zeros((1, 256), np.float32)
    with pytest.raises(pkg.binding.MI355Error):
        be.moe_router(F32, W, 257, 256, x, 8)
    with pytest.raises(pkg.binding.MI355Error):
        be.moe_router(F32, W[:8], 8, 256, x, 9)


# ------------------------------------------------------------------------------------------------ model level
def run_forced(c, ref, toks, pos, seq=None, want=None):
    """The reference decodes first; its selections go to the device for the same call (no token can take another expert on a near tie of the router)."""
    r = ref.decode(toks, pos, seq, want)
    c.force_moe_ids(ref.routes[-1])
    rc = c.decode(toks, pos) if seq is None else c.decode(toks, pos, seq, want)
    assert rc == 0
    return r


CASES = [("tiny-qwen3moe", "q4_k_m", "q8_0", 21), ("tiny-qwen3moe", "q8_0", "f16", 40), ("tiny-qwen3moe", "q5_k_m", "q4_0", 70),
         ("tiny-qwen3moe-160e", "q4_k_m", "q8_0", 40), ("tiny-qwen3moe-30b-2l", "q4_k_m", "q8_0", 40), ("tiny-qwen3moe-30b-2l", "q5_k_m", "f16", 21)]


@pytest.mark.parametrize("cfg,ftype,kv,n_prompt", CASES)
def test_qwen3moe_layers_logits_and_greedy_ids(be, pkg, tmp_models, cfg, ftype, kv, n_prompt):
    """A prompt (21 tokens: the per-expert grouped form; 40 / 70: every expert's batch in one launch per projection), then single-token steps (the 8 selected
    experts share one launch per projection), teacher-forced with the reference's tokens and its expert selections: per layer, logits and greedy ids."""
    path = make(pkg, tmp_models, cfg, ftype)
    oq.set_fa_v_acc_f32(1 if kv == "f16" else 0)
    try:
        m = pkg.Model(path)
        c = pkg.Context(m, n_ctx=128, type_k=KV[kv], type_v=KV[kv])
        ref = Qwen3MoeRef(path, 128, KV[kv], KV[kv])
        rng = np.random.default_rng(5)
        prompt = rng.integers(0, m.n_vocab, n_prompt)
        c.enable_taps(True)
        r = run_forced(c, ref, prompt, np.arange(n_prompt))[0]
        errs = [rel_err(c.layer_out(il, n_prompt).reshape(n_prompt, -1), ref.layer_out(il, n_prompt)) for il in range(m.n_layer)]
        errs.append(rel_err(c.logits(), r))
        assert max(errs) <= FLIP_TOL, errs
        c.enable_taps(False)
        tok, mism, step_err = int(r.argmax()), 0, []
        for step in range(8):
            r = run_forced(c, ref, [tok], [n_prompt + step])[0]
            step_err.append(rel_err(c.logits(), r))
            tok = int(r.argmax())
            if c.argmax() != tok:                # only at a near tie of the reference's logits
                top2 = np.sort(r)[-2:]
                assert top2[1] - top2[0] <= 2 * FLIP_TOL * max(1.0, np.abs(r).max()), (step, top2)
                mism += 1
        assert max(step_err) <= FLIP_TOL, step_err
        assert mism <= 1, (mism, step_err)
        c.close(); m.close()
    finally:
        oq.set_fa_v_acc_f32(0)


def test_qwen3moe_prompt_forms_agree(be, pkg, tmp_models):
    """One 40-token prompt through the three expert forms: every expert's batch in one launch (T >= 32), one launch per expert (moe_group_min 8 with the
    one-launch form unavailable below 32 tokens: a 21-token slice), and the per-(token, rank) mat-vec loop (moe_group_min above the batch) - each against
    the reference with its selections handed over."""
    path = make(pkg, tmp_models, "tiny-qwen3moe", "q4_k_m")
    m = pkg.Model(path)
    rng = np.random.default_rng(23)
    try:
        for n, gmin in ((40, 8), (21, 8), (40, 1 << 20), (21, 1 << 20)):
            be.set_option("moe_group_min", gmin)
            prompt = rng.integers(0, m.n_vocab, n)
            c = pkg.Context(m, n_ctx=128, type_k=KV["q8_0"], type_v=KV["q8_0"])
            ref = Qwen3MoeRef(path, 128, KV["q8_0"], KV["q8_0"])
            c.enable_taps(True)
            r = run_forced(c, ref, prompt, np.arange(n))[0]
            errs = [rel_err(c.layer_out(il, n).reshape(n, -1), ref.layer_out(il, n)) for il in range(m.n_layer)] + [rel_err(c.logits(), r)]
            assert max(errs) <= FLIP_TOL, (n, gmin, errs)
            c.close()
    finally:
        be.set_option("moe_group_min", 8)
        m.close()


def test_grouped_plane_launch_against_the_mat_vec_loop(be, pkg, tmp_models):
    """96 tokens with the expert ids forced so that layer 1's batches are of 288 rows (expert 5, three ranks of every token: two 256-token tiles, the second of
    32 rows), 33 (expert 9), 32 (expert 7), 1 (expert 11), a spread of small ones, and none at all for most of the low experts: every expert's batch in one
    launch per projection against the per-(token, rank) mat-vec loop (moe_group_min above the batch), compared as the two forms of
    test_moe_prompt_batches_grouped_by_expert (tests/test_gpu_model.py) are - per layer the median over the tokens of the per-token error within TIGHT_TOL,
    the logits within FLIP_TOL."""
    path = make(pkg, tmp_models, "tiny-qwen3moe", "q4_k_m")
    m = pkg.Model(path)
    T, KU, NE = 96, 8, 128
    rng = np.random.default_rng(96)
    ids = np.stack([np.stack([rng.permutation(NE)[:KU] for _ in range(T)]) for _ in range(m.n_layer)]).astype(np.int32)
    L1 = ids[1]
    L1[:, 0:3] = 5
    L1[:32, 3], L1[32:65, 3], L1[65:, 3] = 7, 9, 12 + np.arange(T - 65) % 8
    L1[:, 4] = 20 + np.arange(T) % 50
    L1[0, 4] = 11
    L1[:, 5:] = 70 + (np.arange(T)[:, None] * 3 + np.arange(3)[None, :]) % 58
    counts = np.bincount(L1.reshape(-1), minlength=NE)
    assert counts[5] == 288 and counts[9] == 33 and counts[7] == 32 and counts[11] == 1 and (counts == 0).sum() >= 4 and counts.sum() == T * KU
    toks = rng.integers(0, m.n_vocab, T)
    outs = {}
    try:
        for mode, gmin in (("grouped", 8), ("loop", 1 << 20)):
            be.set_option("moe_group_min", gmin)
            c = pkg.Context(m, n_ctx=256, type_k=KV["q8_0"], type_v=KV["q8_0"])
            c.enable_taps(True)
            c.force_moe_ids(ids)
            assert c.decode(toks, np.arange(T)) == 0
            outs[mode] = (c.logits().copy(), [c.layer_out(il, T).copy() for il in range(m.n_layer)])
            c.close()
    finally:
        be.set_option("moe_group_min", 8)
    n_layer = m.n_layer
    m.close()
    for il in range(n_layer):
        g, l = outs["grouped"][1][il].reshape(T, -1), outs["loop"][1][il].reshape(T, -1)
        assert np.isfinite(g).all() and np.abs(g).max() > 0
        tok = np.abs(g - l).max(axis=1) / max(1.0, float(np.abs(l).max()))
        print(f"layer {il}: per-token error median {float(np.median(tok)):.3g} max {float(tok.max()):.3g}")
        assert float(np.median(tok)) <= TIGHT_TOL, (il, tok)
    assert rel_err(outs["grouped"][0], outs["loop"][0]) <= FLIP_TOL


@pytest.mark.parametrize("cfg,kv", [("tiny-qwen3moe", "q8_0"), ("tiny-qwen3moe-30b-2l", "f16")])
def test_qwen3moe_batched_steps(be, pkg, tmp_models, cfg, kv):
    """Three sequences of different lengths advance together (one token each per step), then one sequence takes two tokens in one step; against the
    reference, sequence by sequence, with its selections handed over."""
    path = make(pkg, tmp_models, cfg, "q4_k_m")
    oq.set_fa_v_acc_f32(1 if kv == "f16" else 0)
    try:
        m = pkg.Model(path)
        c = pkg.Context(m, n_ctx=512, n_seq_max=4, type_k=KV[kv], type_v=KV[kv])
        ref = Qwen3MoeRef(path, 512, KV[kv], KV[kv])
        rng = np.random.default_rng(17)
        lens = [70, 9, 33]
        for sq, n in enumerate(lens):
            p = rng.integers(0, m.n_vocab, n)
            fl = np.zeros(n, np.int8); fl[-1] = 1
            r = run_forced(c, ref, p, np.arange(n), [sq] * n, fl)
            assert rel_err(c.logits(n - 1), r[0]) <= FLIP_TOL
        toks = [3, 5, 7]
        for step in range(6):
            pos = [n + step for n in lens]
            r = run_forced(c, ref, toks, pos, [0, 1, 2], [1, 1, 1])
            for j in range(3):
                assert rel_err(c.logits(j), r[j]) <= FLIP_TOL, (step, j)
            toks = [int(x.argmax()) for x in r]
        p1 = lens[1] + 6
        r = run_forced(c, ref, [toks[1], 11], [p1, p1 + 1], [1, 1], [1, 1])
        for j in range(2):
            assert rel_err(c.logits(j), r[j]) <= FLIP_TOL
        c.close(); m.close()
    finally:
        oq.set_fa_v_acc_f32(0)


@pytest.mark.parametrize("option", ["decode_mega", "decode_engine"])
def test_qwen3moe_refused_by_mega_and_engine(be, pkg, tmp_models, option, request):
    """The whole-step kernel and the layer engine have neither the router nor the q / k norm: switched on, a qwen3moe context must take neither, nor the
    one-launch attention block, and give the default options' logits bit for bit."""
    if not _need_experiments(be, option, request):
        return
    path = make(pkg, tmp_models, "tiny-qwen3moe-30b-2l", "q4_k_m")
    m = pkg.Model(path)
    prompt = np.random.default_rng(9).integers(0, m.n_vocab, 21)

    def run(on):
        be.set_option(option, 1 if on else (0 if option == "decode_mega" else -1))
        try:
            c = pkg.Context(m, n_ctx=256, type_k=KV["q8_0"], type_v=KV["q8_0"])
            assert c.decode(prompt, np.arange(21)) == 0
            rows = [c.logits().copy()]
            for s in range(8):
                assert c.decode([int(rows[-1].argmax())], [21 + s]) == 0
                rows.append(c.logits().copy())
            assert c.mega_steps() == 0 and c.engine_steps() == 0 and c.qkv_attn_launches() == 0
            c.close()
        finally:
            be.set_option(option, 0 if option == "decode_mega" else -1)
        return np.stack(rows)

    a, b = run(True), run(False)
    assert np.isfinite(a).all() and np.array_equal(a, b)
    m.close()


# ------------------------------------------------------------------------------------------------ engine
GREEDY = dict(temperature=0.0, repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)


@pytest.fixture(scope="module")
def qwen3moe_vocab_model(pkg, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("q3meng") / "tiny-qwen3moe.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny-qwen3moe", "q4_k_m", with_vocab=True)
    return path


def _greedy(pkg, path, prompt: str, n_predict: int) -> str:
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=512, n_seq_max=1)
    toks = m.tokenize(prompt, add_special=True, parse_special=True)
    assert c.decode(toks, list(range(len(toks)))) == 0
    out, pos = b"", len(toks)
    eos = m.lib.mi355_token_eos(m.h)
    for _ in range(n_predict + 1):
        t = int(np.argmax(c.logits(-1)))
        if t == eos:
            break
        out += m.token_to_piece(t)
        assert c.decode([t], [pos]) == 0
        pos += 1
    c.close(); m.close()
    return out.decode("utf-8", errors="replace")


def test_qwen3moe_engine_chat_and_context_shift(pkg, qwen3moe_vocab_model):
    """/loadmodel of a qwen3moe file, a greedy chat completion equal to the direct greedy decode, then a generation that shifts a 96-cell context."""
    e = pkg.Engine()
    try:
        st, body = e.load_model(llama_model_path=qwen3moe_vocab_model, ctx_len=512, n_parallel=1, ngl=100, user_prompt="u:", ai_prompt="a:", system_prompt="s:")
        assert st["status_code"] == 200 and not st["has_error"], (st, body)
        msgs = [{"role": "system", "content": "be brief"}, {"role": "user", "content": "hello world"}]
        st, body = e.chat_completion(model="tiny-qwen3moe", messages=msgs, max_tokens=12, **GREEDY)[-1]
        assert st["status_code"] == 200 and not st["has_error"], (st, body)
        content = body["choices"][0]["message"]["content"]
        want = _greedy(pkg, qwen3moe_vocab_model, "s:be briefu:hello worlda:", 12)
        if "u:" not in want:
            assert content in (want.lstrip(" "), want), (content, want)
        st, body = e.unload_model(model="tiny-qwen3moe")
        assert st["status_code"] == 200
        # (the user prompt is a stop word: a long one, so that a random model does not write it before the context has shifted)
        st, body = e.load_model(llama_model_path=qwen3moe_vocab_model, ctx_len=96, n_parallel=1, ngl=100, user_prompt="user-turn-marker:", ai_prompt="a:")
        assert st["status_code"] == 200, (st, body)
        st, body = e.chat_completion(model="tiny-qwen3moe", messages=[{"role": "user", "content": "abc def ghi"}], max_tokens=200, ignore_eos=True, **GREEDY)[-1]
        assert st["status_code"] == 200 and body["usage"]["completion_tokens"] == 200       # went well past the 96-cell context
    finally:
        e.close()


def test_qwen3moe_refusals(pkg, tmp_models, qwen3moe_vocab_model):
    """A row split of a qwen3moe file (at model_load and in the engine before any worker starts), a qwen3moe file whose layers are dense, a qwen3 file with
    experts, and an expert_feed_forward_length the tensors disagree with are refused, with errors that name the case."""
    e = pkg.Engine()
    try:
        st, body = e.load_model(llama_model_path=qwen3moe_vocab_model, ctx_len=128, split_mode="row", split_ranks=2)
        assert st["status_code"] != 200 and "qwen3moe" in str(body) and "row split" in str(body), (st, body)
    finally:
        e.close()
    with pytest.raises(pkg.binding.MI355Error, match="qwen3moe"):
        pkg.Model(qwen3moe_vocab_model, tp_rank=0, tp_size=2)
    base = pkg.gguf_synth.CONFIGS["tiny-qwen3moe"]
    dense = dataclasses.replace(base, name="tiny-qwen3moe-dense", n_expert=0, n_expert_used=0, n_ff_exp=0)
    with pytest.raises(pkg.binding.MI355Error, match="qwen3moe"):
        pkg.Model(make(pkg, tmp_models, dense, "q8_0"))
    q3e = dataclasses.replace(base, name="tiny-qwen3-experts", arch="qwen3", n_ff=256, n_ff_exp=0)
    with pytest.raises(pkg.binding.MI355Error, match="qwen3 files with experts"):
        pkg.Model(make(pkg, tmp_models, q3e, "q8_0"))
    bad = dataclasses.replace(base, name="tiny-qwen3moe-badff", n_ff=256, n_ff_exp=0, extra={"expert_feed_forward_length": 512})
    with pytest.raises(pkg.binding.MI355Error, match="expert_feed_forward_length"):
        pkg.Model(make(pkg, tmp_models, bad, "q8_0"))
