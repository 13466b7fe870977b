"""general.architecture "qwen3" on the GPU: the per-head q / k RMSNorm inside the kernels that rotate (the single-launch and store-fused decode attention,
rope_kv_store of prompt batches), attention widths H * D other than n_embd, tied output heads - op by op against the oracle's primitives, and end to end
against the composed reference of tests/qwen3_ref.py (the CPU oracle's graph cannot load a qwen3 file)."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as oq
from oracle_py import F16, Q4_0, Q8_0
from qwen3_ref import Qwen3Ref

pytestmark = pytest.mark.gpu

KV = {"f16": 1, "q8_0": 8, "q4_0": 2}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPERIMENTS_LIB = os.path.join(ROOT, "cortex.llamacpp_amd", "lib", "libmi355_llama_experiments.so")
# the end-to-end tolerances of tests/test_gpu_model.py (see the calibration note there): every layer and step within FLIP_TOL, agreement to f32 round-off
# before the first rounding flip within TIGHT_TOL
FLIP_TOL = 3e-2
TIGHT_TOL = 2e-5


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def make(pkg, tmp_models, cfg, ftype, seed=11):
    name = cfg if isinstance(cfg, str) else cfg.name
    path = str(tmp_models / f"{name}-{ftype}-{seed}.gguf")
    if not os.path.exists(path):
        pkg.gguf_synth.write_synthetic_llama(path, cfg, ftype, seed=seed)
    return path


def head_norm(x, n_head, D, w, eps):
    return np.concatenate([oq.rms_norm(x[h * D:(h + 1) * D], eps) * w for h in range(n_head)]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ op level
@pytest.mark.parametrize("mode", [1, 0, 2])
@pytest.mark.parametrize("tkv,H,G,n_cells", [(Q8_0, 32, 8, 4000), (F16, 32, 8, 1500), (Q4_0, 32, 8, 2048),     # Qwen3-8B / -4B's heads: 4 per kv head
                                              (Q8_0, 16, 8, 561), (F16, 16, 8, 130),                          # Qwen3-0.6B / -1.7B's: 2
                                              (Q8_0, 8, 8, 300), (Q4_0, 16, 2, 2100), (F16, 64, 8, 900)])     # 1 and 8 (Qwen3-32B's)
def test_attn_decode_qk_norm(be, mode, tkv, H, G, n_cells):
    """The decode attention of one token with NEOX rope and the per-head q / k RMSNorm (mi355_op_attn_decode_neox) against the oracle's ops chained the same
    way: rms_norm per head * weight, rope(neox), quantize into the cache, flash_attn.  mode 1: single-launch step; 0: store-fused batched form; 2: the generic
    rope_kv_store path.  Null weights: the plain NEOX path, against the chain without the norm."""
    D, base, eps = 128, 1e6, 1e-6
    rng = np.random.default_rng(H * 1000 + G * 10 + n_cells + tkv)
    kf = rng.standard_normal((n_cells, G * D)).astype(np.float32)
    vf = (rng.standard_normal((n_cells, G * D)) * rng.uniform(0.2, 3.0, (n_cells, 1))).astype(np.float32)
    kc = np.stack([oq.quantize(tkv, r) for r in kf])
    vc = np.stack([oq.quantize(tkv, r) for r in vf])
    tok_pos = n_cells + 7
    cell_pos = rng.permutation(n_cells).astype(np.int32)
    cell_pos[rng.random(n_cells) < 0.1] = -1                        # holes
    cell_pos[rng.random(n_cells) < 0.03] = tok_pos + 5              # cells of later positions: not visible
    tok_cell = int(n_cells * 0.61)
    cell_pos[tok_cell] = tok_pos
    # un-normalised projections at a scale of their own per head (the norm must take each head's own sum of squares)
    q = (rng.standard_normal((H, D)) * rng.uniform(0.3, 6.0, (H, 1))).astype(np.float32).reshape(-1)
    k_new = (rng.standard_normal((G, D)) * rng.uniform(0.3, 6.0, (G, 1))).astype(np.float32).reshape(-1)
    v_new = (rng.standard_normal(G * D) * 1.7).astype(np.float32)
    qn = rng.uniform(0.25, 2.0, D).astype(np.float32)
    kn = rng.uniform(0.25, 2.0, D).astype(np.float32)
    scale = 1 / np.sqrt(D)
    rb = oq.row_bytes(tkv, G * D)
    cells = np.nonzero((cell_pos >= 0) & (cell_pos <= tok_pos))[0].astype(np.int32)
    for normed in (True, False):
        att, kr, vr = be.attn_decode_neox(q, k_new, v_new, H, G, D, tkv, kc, tkv, vc, cell_pos, tok_pos, tok_cell, base, scale,
                                          qn if normed else None, kn if normed else None, eps, mode, rb, rb)
        qq = head_norm(q, H, D, qn, eps) if normed else q
        kk = head_norm(k_new, G, D, kn, eps) if normed else k_new
        qr = oq.rope(qq, H, D, tok_pos, base, neox=True)
        kr_ref = oq.rope(kk, G, D, tok_pos, base, neox=True).reshape(-1)
        k_row = oq.quantize(tkv, kr_ref)
        assert (vr == oq.quantize(tkv, v_new)).all()                 # no arithmetic before the V row's quantisation: bit-exact
        # the K row goes through the norm and the rope first: its codes may sit one step off on a rounding tie
        dk_ref, dk_got = oq.dequantize(tkv, k_row, G * D), oq.dequantize(tkv, kr, G * D)
        if tkv == Q8_0:
            step = np.abs(kr_ref).reshape(-1, 32).max(axis=1).repeat(32) / 127
        elif tkv == Q4_0:
            step = np.abs(kr_ref).reshape(-1, 32).max(axis=1).repeat(32) / 8
        else:
            step = np.abs(kr_ref) * 2.0 ** -10
        assert (np.abs(dk_ref - dk_got) <= 1.01 * step + 1e-6).all(), float(np.abs(dk_ref - dk_got).max())
        assert (dk_ref == dk_got).mean() >= 0.99
        kc2, vc2 = kc.copy(), vc.copy()
        kc2[tok_cell] = kr                                           # (the row the device wrote: what its attention saw)
        vc2[tok_cell] = vr
        oq.set_fa_v_acc_f32(1 if tkv == F16 else 0)
        try:
            ref = oq.flash_attn(qr, H, G, D, tkv, kc2, tkv, vc2, cells, scale).reshape(-1)
        finally:
            oq.set_fa_v_acc_f32(0)
        assert np.abs(att - ref).max() <= 2e-5 * max(1.0, float(np.abs(ref).max())), (normed, float(np.abs(att - ref).max()))
        if normed:
            normed_att = att
    # the norm changes the result by far more than the tolerance (the weights are not ignored)
    assert np.abs(normed_att - att).max() > 1e-2 * max(1.0, float(np.abs(att).max()))


# ------------------------------------------------------------------------------------------------ model level
CASES = [("tiny-qwen3", "q4_k_m", "q8_0", 21), ("tiny-qwen3", "q8_0", "f16", 40), ("tiny-qwen3", "q5_k_m", "q4_0", 70),
         ("tiny-qwen3-0.6b-2l", "q5_k_m", "q8_0", 70), ("tiny-qwen3-0.6b-2l", "q4_k_m", "q4_0", 21),
         ("tiny-qwen3-4b-2l", "q4_k_m", "q8_0", 40), ("tiny-qwen3-4b-2l", "q6_k", "f16", 21),
         ("tiny-qwen3-8b-2l", "q4_k_m", "q8_0", 70), ("tiny-qwen3-8b-2l", "q8_0", "q8_0", 21)]


@pytest.mark.parametrize("cfg,ftype,kv,n_prompt", CASES)
def test_qwen3_layers_logits_and_greedy_ids(be, pkg, tmp_models, cfg, ftype, kv, n_prompt):
    """A prompt (21 tokens: the generic rope_kv_store path; 40 / 70: the matrix-core prompt attention behind it), then single-token steps (the
    single-launch decode attention with the norm inside) teacher-forced with the reference's tokens: per layer, logits and greedy ids."""
    path = make(pkg, tmp_models, cfg, ftype)
    oq.set_fa_v_acc_f32(1 if kv == "f16" else 0)
    try:
        m = pkg.Model(path)
        c = pkg.Context(m, n_ctx=128, type_k=KV[kv], type_v=KV[kv])
        ref = Qwen3Ref(path, 128, KV[kv], KV[kv])
        rng = np.random.default_rng(5)
        prompt = rng.integers(0, m.n_vocab, n_prompt)
        c.enable_taps(True)
        assert c.decode(prompt, np.arange(n_prompt)) == 0
        r = ref.decode(prompt, np.arange(n_prompt))[0]
        errs = [rel_err(c.layer_out(il, n_prompt).reshape(n_prompt, -1), ref.layer_out(il, n_prompt)) for il in range(m.n_layer)]
        a0 = c.layer_out(0, n_prompt).reshape(n_prompt, -1)
        b0 = ref.layer_out(0, n_prompt)
        tok_err0 = np.abs(a0 - b0).max(axis=1) / max(1.0, float(np.abs(b0).max()))
        errs.append(rel_err(c.logits(), r))
        assert max(errs) <= FLIP_TOL, errs
        c.enable_taps(False)
        tok, mism, step_err = int(r.argmax()), 0, []
        for step in range(10):
            assert c.decode([tok], [n_prompt + step]) == 0
            r = ref.decode([tok], [n_prompt + step])[0]
            g = c.logits()
            step_err.append(rel_err(g, r))
            tok = int(r.argmax())
            if c.argmax() != tok:                # only at a near tie of the reference's logits
                top2 = np.sort(r)[-2:]
                assert top2[1] - top2[0] <= 2 * FLIP_TOL * max(1.0, np.abs(r).max()), (step, top2)
                mism += 1
        assert max(step_err) <= FLIP_TOL, step_err
        assert mism <= 1, (mism, step_err)
        if kv != "f16" and ftype not in ("q8_0",):
            # before the first rounding flip the two agree to f32 round-off: the typical token of the first layer, and most tokens individually
            assert float(np.median(tok_err0)) <= TIGHT_TOL, (errs, tok_err0)
            assert int((tok_err0 <= TIGHT_TOL).sum()) * 3 >= 2 * n_prompt, (errs, tok_err0)
        c.close(); m.close()
    finally:
        oq.set_fa_v_acc_f32(0)


@pytest.mark.parametrize("cfg,kv", [("tiny-qwen3", "q8_0"), ("tiny-qwen3-4b-2l", "f16"), ("tiny-qwen3-8b-2l", "q4_0")])
def test_qwen3_batched_steps(be, pkg, tmp_models, cfg, kv):
    """Three sequences of different lengths advance together (each token of another sequence: the store-fused batched step, K normalised, rotated and
    stored inside the attention launch), then one sequence takes two tokens in one step (the generic path); against the reference, sequence by sequence."""
    path = make(pkg, tmp_models, cfg, "q4_k_m")
    oq.set_fa_v_acc_f32(1 if kv == "f16" else 0)
    try:
        m = pkg.Model(path)
        c = pkg.Context(m, n_ctx=512, n_seq_max=4, type_k=KV[kv], type_v=KV[kv])
        ref = Qwen3Ref(path, 512, KV[kv], KV[kv])
        rng = np.random.default_rng(17)
        lens = [70, 9, 33]
        for sq, n in enumerate(lens):
            p = rng.integers(0, m.n_vocab, n)
            fl = np.zeros(n, np.int8); fl[-1] = 1
            assert c.decode(p, np.arange(n), [sq] * n, fl) == 0
            r = ref.decode(p, np.arange(n), [sq] * n, fl)
            assert rel_err(c.logits(n - 1), r[0]) <= FLIP_TOL
        toks = [3, 5, 7]
        for step in range(8):
            pos = [n + step for n in lens]
            assert c.decode(toks, pos, [0, 1, 2], [1, 1, 1]) == 0
            r = ref.decode(toks, pos, [0, 1, 2], [1, 1, 1])
            for j in range(3):
                assert rel_err(c.logits(j), r[j]) <= FLIP_TOL, (step, j)
            toks = [int(x.argmax()) for x in r]
        p1 = lens[1] + 8
        assert c.decode([toks[1], 11], [p1, p1 + 1], [1, 1], [1, 1]) == 0
        r = ref.decode([toks[1], 11], [p1, p1 + 1], [1, 1], [1, 1])
        for j in range(2):
            assert rel_err(c.logits(j), r[j]) <= FLIP_TOL
        c.close(); m.close()
    finally:
        oq.set_fa_v_acc_f32(0)


# ------------------------------------------------------------------------------------------------ guards
def _need_experiments(be, option, request) -> bool:
    """As tests/test_gpu_model.py: the whole-step kernel and the layer engine live in the experiments library only; where this process lacks them the test
    runs again in a child pytest on that library (returns False: the caller has nothing left to do)."""
    try:
        be.set_option(option, 1)
    except Exception as e:
        assert "MI355_BUILD_EXPERIMENTS" in str(e), e
        assert os.environ.get("MI355_LLAMA_LIB") != EXPERIMENTS_LIB, f"{EXPERIMENTS_LIB} does not hold the experiment kernels: {e}"
        assert os.path.exists(EXPERIMENTS_LIB), f"{EXPERIMENTS_LIB} is missing: run build()"
        r = subprocess.run([sys.executable, "-m", "pytest", request.node.nodeid, "-q", "-p", "no:cacheprovider"], cwd=ROOT, capture_output=True, text=True,
                           timeout=600, env=dict(os.environ, MI355_LLAMA_LIB=EXPERIMENTS_LIB))
        assert r.returncode == 0 and "1 passed" in r.stdout, (r.stdout + r.stderr)[-6000:]
        return False
    be.set_option(option, 0 if option == "decode_mega" else -1)
    return True


@pytest.mark.parametrize("option", ["decode_mega", "decode_engine"])
def test_qwen3_refused_by_mega_and_engine(be, pkg, tmp_models, option, request):
    """The whole-step kernel and the layer engine have no q / k norm: switched on, a qwen3 context of the one geometry they have forms for (Llama-3-8B's
    4096 / 14336 with 4 query heads per kv head, K-quant tensors, no biases) must take neither, nor the one-launch attention block, and give the default
    options' logits bit for bit."""
    if not _need_experiments(be, option, request):
        return
    cfg = dataclasses.replace(pkg.gguf_synth.CONFIGS["tiny-qwen3-8b-2l"], name="tiny-qwen3-8b-ff14k-2l", n_ff=14336)
    path = make(pkg, tmp_models, cfg, "q4_k_m")
    m = pkg.Model(path)
    prompt = np.random.default_rng(9).integers(0, m.n_vocab, 21)

    def run(on):
        be.set_option(option, 1 if on else (0 if option == "decode_mega" else -1))
        try:
            c = pkg.Context(m, n_ctx=256, type_k=KV["q8_0"], type_v=KV["q8_0"])
            assert c.decode(prompt, np.arange(21)) == 0
            rows = [c.logits().copy()]
            for s in range(12):
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
def qwen3_vocab_model(pkg, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("q3eng") / "tiny-qwen3.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny-qwen3", "q4_k_m", with_vocab=True)
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


def test_qwen3_engine_chat_and_context_shift(pkg, qwen3_vocab_model):
    """/loadmodel of a qwen3 file, a greedy chat completion equal to the direct greedy decode, then a generation that shifts a 96-cell context."""
    e = pkg.Engine()
    try:
        st, body = e.load_model(llama_model_path=qwen3_vocab_model, ctx_len=512, n_parallel=1, ngl=100, user_prompt="u:", ai_prompt="a:", system_prompt="s:")
        assert st["status_code"] == 200 and not st["has_error"], (st, body)
        msgs = [{"role": "system", "content": "be brief"}, {"role": "user", "content": "hello world"}]
        st, body = e.chat_completion(model="tiny-qwen3", messages=msgs, max_tokens=12, **GREEDY)[-1]
        assert st["status_code"] == 200 and not st["has_error"], (st, body)
        content = body["choices"][0]["message"]["content"]
        want = _greedy(pkg, qwen3_vocab_model, "s:be briefu:hello worlda:", 12)
        if "u:" not in want:
            assert content in (want.lstrip(" "), want), (content, want)
        st, body = e.unload_model(model="tiny-qwen3")
        assert st["status_code"] == 200
        st, body = e.load_model(llama_model_path=qwen3_vocab_model, ctx_len=96, n_parallel=1, ngl=100, user_prompt="u:", ai_prompt="a:")
        assert st["status_code"] == 200, (st, body)
        st, body = e.chat_completion(model="tiny-qwen3", messages=[{"role": "user", "content": "abc def ghi"}], max_tokens=200, ignore_eos=True, **GREEDY)[-1]
        assert st["status_code"] == 200 and body["usage"]["completion_tokens"] == 200       # went well past the 96-cell context
    finally:
        e.close()


def test_qwen3_refusals(pkg, tmp_models, qwen3_vocab_model):
    """qwen3moe files and a row split of a qwen3 file are refused, with an error that names the case."""
    cfg = dataclasses.replace(pkg.gguf_synth.CONFIGS["tiny-qwen3"], name="tiny-qwen3moe", arch="qwen3moe")
    moe = make(pkg, tmp_models, cfg, "q4_k_m")
    with pytest.raises(pkg.binding.MI355Error, match="qwen3moe"):
        pkg.Model(moe)
    e = pkg.Engine()
    try:
        st, body = e.load_model(llama_model_path=moe, ctx_len=128)
        assert st["status_code"] != 200 and "qwen3moe" in str(body), (st, body)
        st, body = e.load_model(llama_model_path=qwen3_vocab_model, ctx_len=128, split_mode="row", split_ranks=2)
        assert st["status_code"] != 200 and "qwen3" in str(body) and "row split" in str(body), (st, body)
    finally:
        e.close()
    with pytest.raises(pkg.binding.MI355Error, match="qwen3"):
        pkg.Model(qwen3_vocab_model, tp_rank=0, tp_size=2)
