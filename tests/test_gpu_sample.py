"""The device sampler (csrc/sample.hip): the chain's tail and the draw against the float64 restatement (tests/sample_ref.py), the device's Philox sequence,
the path through a context (mi355_sample_rows, mi355_sampled_steps), the refusals and the engine key "device_sampler"."""
import numpy as np
import pytest

import sample_ref as ref

pytestmark = pytest.mark.gpu

CUTS = {
    "none": {}, "top_k": dict(top_k=10), "typ_p": dict(typ_p=0.5), "top_p": dict(top_p=0.7), "top_p_to_one": dict(top_p=0.01), "min_p": dict(min_p=0.1),
    "all": dict(top_k=100, typ_p=0.5, top_p=0.7, min_p=0.1),
}
ROW_KINDS = [dict(min_keep=mk, temp=t) for mk in (0, 1, 5) for t in (0.0, 0.25, 1.0, 4.0)]
RATIOS = (0.95, 0.94, 0.96)          # flat enough that the last of 128 candidates keeps p > 1e-14 at temp 0.25: every CDF interval is one float64 resolves
TOL = 64 * 2.0 ** -23                # 64 ulp of f32, relative


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


def ladder(R, k):
    """candidates of R rows, best first: a geometric ladder of probabilities (ratio by row) with exact ties at ranks 4|5 and 21|22, distinct tokens"""
    j = np.arange(k)
    lg = np.stack([(2.0 - 0.03 * r + np.log(RATIOS[r % 3]) * j).astype(np.float32) for r in range(R)])
    for a in (5, 22):
        if k > a:
            lg[:, a] = lg[:, a - 1]
    return (j[None, :] * 7 + np.arange(R)[:, None]).astype(np.int32), lg


@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("R", [1, 3, 67])
@pytest.mark.parametrize("k", [1, 2, 64, 65, 128])
def test_chain_against_float64(be, k, R, cut):
    tok, lg = ladder(R, k)
    params = [{**CUTS[cut], **ROW_KINDS[(r + k) % len(ROW_KINDS)]} for r in range(R)]
    want = [ref.chain(tok[r], lg[r], **params[r]) for r in range(R)]
    assert min(w[2] for w in want) >= 1e-3                       # every threshold sits in the middle of a gap of the reference
    # one launch with u = 0: the kept sets, their order and probabilities, and the first kept candidate
    got_t, got_n, got_p, kept_t, kept_p = be.sample_rows_op(tok, lg, params, u=np.zeros(R))
    worst = 0.0
    for r, (wt, wp, _) in enumerate(want):
        assert got_n[r] == len(wt) and list(kept_t[r, :len(wt)]) == list(wt), (r, params[r])
        worst = max(worst, float(np.abs(kept_p[r, :len(wt)].astype(np.float64) / wp - 1.0).max()))
        assert got_t[r] == wt[0]
    print(f"k={k} R={R} {cut}: worst relative probability error {worst:.3g}")
    assert worst <= TOL
    # one more launch, a row per (row, kept candidate j) with u at the float64 midpoint of j's CDF interval, and per row u = 1 - 2^-24: the last kept
    rows, us, exp = [], [], []
    for r, (wt, wp, _) in enumerate(want):
        c = np.concatenate([[0.0], np.cumsum(wp)]) / wp.sum()
        for j in range(len(wt)):
            rows.append(r); us.append(0.5 * (c[j] + c[j + 1])); exp.append(wt[j])
        rows.append(r); us.append(1.0 - 2.0 ** -24); exp.append(wt[ref.draw(wp, 1.0 - 2.0 ** -24)])
    got_t = be.sample_rows_op(tok[rows], lg[rows], [params[r] for r in rows], u=np.array(us), kept=False)[0]
    assert list(got_t) == exp


def test_row_without_a_finite_logit_gives_minus_one(be):
    tok, lg = ladder(3, 8)
    lg[1, :] = -np.inf
    got_t, got_n, got_p, _, _ = be.sample_rows_op(tok, lg, dict(top_p=0.7), u=np.zeros(3))
    assert list(got_t) == [tok[0, 0], -1, tok[2, 0]] and got_n[1] == 0 and got_p[1] == 0.0


@pytest.mark.parametrize("stream", [0, 5])
@pytest.mark.parametrize("counter", [0, 2 ** 32 - 1, 2 ** 32])
@pytest.mark.parametrize("seed", [0, 1, 2 ** 64 - 1])
def test_philox_is_the_published_generator(be, seed, counter, stream):
    assert ref.philox4x32_10(0, 0, 0) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]      # the known answer of Random123's kat_vectors
    got = be.philox_u(seed, counter, stream, 4)                  # (counter 2^32 - 1: the second draw carries into the high word)
    want = np.array([ref.philox_u(seed, counter + i, stream) for i in range(4)], np.float32)
    assert got.tobytes() == want.tobytes()
    other = be.philox_u(seed, counter, stream + 1, 4)
    assert len(set(got.tolist())) == 4 and not set(got.tolist()) & set(other.tolist())


SAMPLED = dict(top_k=40, top_p=0.95, min_p=0.05, typ_p=1.0, temp=0.8, penalty_repeat=1.3, penalty_freq=0.1, penalty_present=0.2)


@pytest.fixture(scope="module")
def ctx(pkg, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("smp") / "tiny.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny", "q4_k_m", seed=7)
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=64)
    yield c
    c.close(); m.close()


def test_context_rows_equal_the_op_on_the_front_candidates(be, ctx):
    ctx.kv_clear()
    assert ctx.decode([5, 9, 300], [0, 1, 2], logits=[1, 1, 1]) == 0
    adjs = [([9, 300], [2.0, 0.0], [0, 2]), None, ([17], [-1.0], [1])]
    params = [dict(SAMPLED, seed=11, stream=r) for r in range(3)]
    calls = ctx.sample_rows_calls()
    got_t, got_p = ctx.sample_rows([0, 1, 2], params, [4, 5, 6], adjs)
    assert ctx.sample_rows_calls() == calls + 1
    for r in range(3):
        a = adjs[r] or ([], [], [])
        toks, lg = ctx.topk(40, r, *a, repeat=1.3, freq=0.1, present=0.2)
        t, _, p, _, _ = be.sample_rows_op(toks, lg, params[r], u=[float(ref.philox_u(11, 4 + r, r))], kept=False)
        assert (got_t[r], got_p[r]) == (t[0], p[0])


def manual_steps(ctx, first, pos0, n, params):
    out, tok = [], first
    for i in range(n):
        assert ctx.decode([tok], [pos0 + i]) == 0
        win = sorted(set(out[-64:]))
        adj = (win, [0.0] * len(win), [out[-64:].count(t) for t in win]) if win else None
        tok = int(ctx.sample_rows([0], params, [i], [adj])[0][0])
        out.append(tok)
    return out


def test_sampled_steps(ctx):
    def run(params):
        ctx.kv_clear()
        assert ctx.decode([5, 9, 300], [0, 1, 2]) == 0
        return list(ctx.sampled_steps(7, 3, 8, params)[0])
    a = run(dict(SAMPLED, seed=21))
    ctx.kv_clear()
    assert ctx.decode([5, 9, 300], [0, 1, 2]) == 0
    assert a == manual_steps(ctx, 7, 3, 8, dict(SAMPLED, seed=21))               # the C loop = 8 rounds of decode + sample_rows, draw counters 0 .. 7
    assert a == run(dict(SAMPLED, seed=21)) and a != run(dict(SAMPLED, seed=22))  # (the two seeds' u sequences differ in every one of the 8 draws)
    ctx.kv_clear()
    assert ctx.decode([5, 9, 300], [0, 1, 2]) == 0
    greedy = list(ctx.greedy_steps(7, 3, 8))
    assert run(dict(top_k=40, temp=0.0, seed=21)) == greedy


BAD = [(dict(top_p=1.5), "top_p"), (dict(top_p=float("nan")), "top_p"), (dict(min_p=-0.1), "min_p"), (dict(typ_p=2.0), "typ_p"), (dict(min_keep=-1), "min_keep")]


@pytest.mark.parametrize("params,word", BAD + [(dict(top_k=0), "top_k"), (dict(top_k=129), "top_k")])
def test_refusals(pkg, be, ctx, params, word):
    tok, lg = ladder(1, 4)
    ctx.kv_clear()
    assert ctx.decode([5, 9], [0, 1], logits=[0, 1]) == 0
    calls = [lambda: ctx.sample_rows([1], {"top_k": 40, **params}, [0])]
    if word != "top_k":                                           # (the launcher takes any top_k: it is the front that needs 1 .. 128)
        calls.append(lambda: be.sample_rows_op(tok, lg, params, u=[0.0]))
    for call in calls:
        with pytest.raises(pkg.binding.MI355Error, match=word):
            call()


def test_refusals_of_shape_and_rows(pkg, be, ctx):
    tok, lg = ladder(1, 4)
    with pytest.raises(pkg.binding.MI355Error, match="k outside"):
        be.sample_rows_op(np.zeros((1, 129), np.int32), np.zeros((1, 129), np.float32), {}, u=[0.0])
    with pytest.raises(pkg.binding.MI355Error, match="R outside"):
        be.sample_rows_op(np.zeros((0, 4), np.int32), np.zeros((0, 4), np.float32), [], u=[])
    ctx.kv_clear()
    assert ctx.decode([5, 9], [0, 1], logits=[0, 1]) == 0
    with pytest.raises(pkg.binding.MI355Error, match="not flagged"):
        ctx.sample_rows([0], dict(top_k=40), [0])
    with pytest.raises(pkg.binding.MI355Error, match="adj_n"):
        ctx.sample_rows([1], dict(top_k=40), [0], [(list(range(193)), [0.0] * 193, [1] * 193)])
    for call in (lambda: ctx.lib.mi355_sample_rows(ctx.h, 1, *[None] * 9), lambda: be.lib.mi355_op_sample_rows(*[None] * 2, 1, 4, *[None] * 7)):
        assert call() == -103 and "null pointer" in pkg.binding._err(be.lib)          # MI355_ERR_ARG (include/mi355_llama.h)
    ctx.set_embeddings(True)                                      # (the rank of a row split, the last refusal, needs a second rank: not here)
    assert ctx.decode([5, 9], [2, 3], logits=[0, 1]) == 0
    with pytest.raises(pkg.binding.MI355Error, match="embeddings"):
        ctx.sample_rows([1], dict(top_k=40), [0])
    ctx.set_embeddings(False)


def test_engine_key_routes_qualifying_requests(pkg, tmp_path):
    path = str(tmp_path / "tiny-vocab.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny", "q4_k_m", with_vocab=True)
    req = dict(model="tiny-vocab", messages=[{"role": "user", "content": "tell me"}], max_tokens=8, temperature=0.9, top_k=20, top_p=0.9, seed=5)
    texts = {}
    for key, n_par in ((None, 1), (False, 1), (True, 1), (True, 2)):   # two slots: the second request of a pair lands in the other slot
        e = pkg.Engine()
        st, body = e.load_model(llama_model_path=path, ctx_len=128 * n_par, n_parallel=n_par, ngl=100, **({} if key is None else {"device_sampler": key}))
        assert st["status_code"] == 200, (st, body)
        texts[key, n_par] = [e.chat_completion(**req)[-1][1]["choices"][0]["message"]["content"] for _ in range(2)]
        plain = e.sampler_stats("tiny-vocab")
        assert (plain["device"] > 0) == (key is True) and (plain["other"] == 0) == (key is True), (key, plain)
        if key:                                                   # a grammar keeps its request on the host chain
            e.chat_completion(**req, grammar='root ::= [a-z]+\n')
            after = e.sampler_stats("tiny-vocab")
            assert after["device"] == plain["device"] and after["other"] > 0
        e.close()
    assert texts[None, 1] == texts[False, 1]                      # off = today's text; on = a text that depends on the seed, not on the slot
    assert all(t[0] == t[1] for (key, _), t in texts.items() if key)
