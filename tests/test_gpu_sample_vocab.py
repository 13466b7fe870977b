"""The whole-row device sampler (csrc/sample_vocab.hip): cuts and draws over a whole vocabulary row against the float64 restatement
(tests/sample_vocab_ref.py), mirostat 2, equal bytes on equal input, the path through a context (mi355_sample_rows_vocab), its refusals, and the engine key."""
import functools

import numpy as np
import pytest

import sample_ref as ref
import sample_vocab_ref as vref

pytestmark = pytest.mark.gpu

# one below / at / one above what the kernel's loops are cut by: 64 lanes x 4 logits, 1024 histogram bins (= threads), 4096 logits a round of the workgroup
NS = [1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 151936]
TEMPS = (0.25, 1.0, 1.7, 0.0)
PEN = dict(penalty_repeat=1.1, penalty_freq=0.05, penalty_present=0.05)
TOL = 64 * 2.0 ** -23                # 64 ulp of f32, relative: the bound tests/test_gpu_sample.py holds this quantity to
N_CUTS = 12

@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()

def cuts(n):
    return [{}] + [dict(top_k=k) for k in (1, 2, 129, n - 1, n, n + 5)] + [dict(top_p=0.7), "tie", dict(min_p=0.1), dict(top_p=0.01, min_keep=5),
                                                                          dict(top_k=129, top_p=0.7, min_p=0.1, min_keep=3)]

@functools.lru_cache(maxsize=None)
def rows_for(n, R):
    """R rows as test_gpu_sample.ladder builds candidates, over random token ids: a geometric ladder spanning at most 3 nats (the last candidate keeps a weight above
    e^-15 at temp 0.25, far above the fixed point's 2^-44), exact ties at ranks 1|2, 4|5, 21|22, 128|129; row 1 all equal (zeros of both signs), row 2 with -inf entries,
    row 3 all -inf; rows 0 and 4 adjusted: a bias carries rank 200 to the top, a penalty takes the best down across the cuts, a penalty on the (negative) last."""
    rng, j, rows, adjs = np.random.default_rng(n), np.arange(n), [], []
    for r in range(R):
        lg = (1.0 - min(0.05, 3.0 / n) * (1 - 0.1 * r) * j).astype(np.float32)
        for a in (2, 5, 22, 129):
            if n > a:
                lg[a] = lg[a - 1]
        if r == 1:
            lg = np.where(j % 2, np.float32(-0.0), np.float32(0.0))
        if r == 2:
            lg[1:][rng.random(n - 1) < 0.1] = -np.inf
        if r == 3:
            lg[:] = -np.inf
        perm = rng.permutation(n)
        row = np.empty(n, np.float32)
        row[perm] = lg
        rows.append(row)
        adj = {int(perm[min(200, n - 1)]): (float(lg[0] - lg[min(200, n - 1)]) + 0.25, 0), int(perm[0]): (0.0, 2), int(perm[n - 1]): (0.0, 1)} if r % 4 == 0 else {}
        adjs.append((list(adj), [b for b, _ in adj.values()], [c for _, c in adj.values()]) if adj else None)
    rows = np.stack(rows)
    rows.setflags(write=False)
    return rows, adjs

def check(be, rows, params, adjs, want, mu=None):
    """n_kept, token and probability for draws at the middle of a candidate's interval: the first, one in a tie group, the last kept with a probability; and u = 1 - 2^-24"""
    assert min(w[2] for w in want) >= 1e-9                         # every comparison of the reference is clear of its threshold
    at, us, exp_t, exp_p = [], [], [], []
    for r, (wt, wp, _) in enumerate(want):
        c = np.concatenate([[0.0], np.cumsum(wp)]) / wp.sum() if wt[0] >= 0 else np.zeros(2)
        for jj in sorted({0, min(5, len(wt) - 1), int(np.nonzero(wp > 0)[0][-1]) if wt[0] >= 0 else 0}):
            at.append(r); us.append(0.5 * (c[jj] + c[jj + 1])); exp_t.append(wt[jj]); exp_p.append(wp[jj])
        jj = ref.draw(wp, 1.0 - 2.0 ** -24)
        at.append(r); us.append(1.0 - 2.0 ** -24); exp_t.append(wt[jj]); exp_p.append(wp[jj])
    got_t, got_n, got_p = be.sample_vocab_op(rows[at], [params[r] for r in at], u=np.array(us), adjs=[adjs[r] for r in at], mu=None if mu is None else mu[at])
    assert list(got_n) == [len(want[r][0]) if want[r][0][0] >= 0 else 0 for r in at]
    assert list(got_t) == exp_t
    exp_p = np.array(exp_p)
    worst = float(np.abs(got_p[exp_p > 0] / exp_p[exp_p > 0] - 1.0).max()) if (exp_p > 0).any() else 0.0
    print(f"worst relative probability error {worst:.3g}")
    assert worst <= TOL and not got_p[exp_p == 0].any()

@pytest.mark.parametrize("ci", range(N_CUTS))
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("n", NS)
def test_plain_chain_against_float64(be, n, R, ci):
    rows, adjs = rows_for(n, R)
    cut, params = cuts(n)[ci], []
    for r in range(R):
        c = cut
        if cut == "tie":                                             # top_p between ranks 3 and 4: the tie 4|5 (the all-equal row's one group) is cut by token id
            _, p, _ = vref.plain(rows[r], dict(PEN), adjs[r])
            c = dict(top_p=float(np.float32(0.5 * (p[:4].sum() + p[:5].sum())))) if len(p) > 5 else dict(top_p=0.45)
        params.append({**c, **PEN, "temp": TEMPS[(r + ci) % 4]})
    check(be, rows, params, adjs, [vref.plain(rows[r], params[r], adjs[r]) for r in range(R)])

@pytest.mark.parametrize("which", ["one", "mid", "all"])
@pytest.mark.parametrize("n", [2, 1025, 4097, 151936])
def test_mirostat2_against_float64(be, n, which):
    rows, adjs = rows_for(n, 5)
    params = [{**PEN, "temp": TEMPS[r % 3], "top_k": 3, "top_p": 0.1} for r in range(5)]     # (the cuts are not read in this chain)
    mu = np.zeros(5, np.float32)
    for r in range(5):
        _, p, _ = vref.mirostat2(rows[r], params[r], 1000.0, adjs[r])
        s, h = -np.log2(np.maximum(p, float(np.float32(1e-37)))), n // 2
        mu[r] = dict(one=0.5 * s[0], all=200.0, mid=0.5 * (s[h - 1] + s[h]) if s[h - 1] != s[h] else s[h] + 0.5)[which] if len(p) == n else 5.0
    check(be, rows, params, adjs, [vref.mirostat2(rows[r], params[r], float(mu[r]), adjs[r]) for r in range(5)], mu=mu)

def test_equal_input_gives_equal_bytes(be):
    rows, adjs = rows_for(4097, 5)
    params = [{**PEN, "top_p": 0.9, "temp": 0.8, "seed": 3, "stream": r} for r in range(5)]
    mu = np.array([np.nan, 4.0, np.nan, 4.0, 6.0], np.float32)
    a, b = (be.sample_vocab_op(rows, params, adjs=adjs, mu=mu) for _ in range(2))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(set(a[0].tolist())) > 1

@pytest.fixture(scope="module")
def ctx(pkg, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("smpv") / "tiny.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny", "q4_k_m", seed=7)
    m = pkg.Model(path)
    c = pkg.Context(m, n_ctx=64)
    yield c
    c.close(); m.close()

def test_context_rows_equal_the_op_on_the_fetched_rows(be, ctx):
    ctx.kv_clear()
    assert ctx.decode([5, 9, 300], [0, 1, 2], logits=[1, 1, 1]) == 0
    adjs = [([9, 300], [2.0, 0.0], [0, 2]), None, ([17], [-1.0], [1])]
    params = [{**PEN, "top_k": k, "top_p": 0.95, "min_p": 0.02, "temp": 0.8, "seed": 11, "stream": r} for r, k in enumerate((0, 200, 40))]
    mu = np.array([np.nan, np.nan, 6.0], np.float32)
    calls = ctx.sample_rows_calls()
    got_t, got_p = ctx.sample_rows_vocab([0, 1, 2], params, [4, 5, 6], adjs, mu)
    assert ctx.sample_rows_calls() == calls + 1
    rows = np.stack([ctx.logits(r) for r in range(3)])
    t, _, p = be.sample_vocab_op(rows, params, u=[float(ref.philox_u(11, 4 + r, r)) for r in range(3)], adjs=adjs, mu=mu)
    assert got_t.tobytes() == t.tobytes() and got_p.tobytes() == p.tobytes()

def test_refusals(pkg, be, ctx):
    ctx.kv_clear()
    assert ctx.decode([5, 9], [0, 1], logits=[0, 1]) == 0
    bad = [(lambda: ctx.sample_rows_vocab([1], dict(typ_p=0.5), [0]), "typ_p"), (lambda: be.sample_vocab_op(np.zeros((1, 8)), dict(typ_p=0.5), u=[0.0]), "typ_p"),
           (lambda: ctx.sample_rows_vocab([1], dict(top_p=1.5), [0]), "top_p"), (lambda: ctx.sample_rows_vocab([0], {}, [0]), "not flagged"),
           (lambda: ctx.sample_rows_vocab([1], {}, [0], [(list(range(193)), [0.0] * 193, [1] * 193)]), "adj_n")]
    for call, word in bad:
        with pytest.raises(pkg.binding.MI355Error, match=word):
            call()
    ctx.set_embeddings(True)
    assert ctx.decode([5, 9], [2, 3], logits=[0, 1]) == 0
    with pytest.raises(pkg.binding.MI355Error, match="embeddings"):
        ctx.sample_rows_vocab([1], {}, [0])
    ctx.set_embeddings(False)

def test_engine_key_routes_whole_row_requests(pkg, tmp_path):
    path = str(tmp_path / "tiny-vocab.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny", "q4_k_m", with_vocab=True)
    base = dict(model="tiny-vocab", messages=[{"role": "user", "content": "tell me"}], max_tokens=8, temperature=0.9, seed=5)
    texts = {}
    for key in (False, True):
        e = pkg.Engine()
        st, body = e.load_model(llama_model_path=path, ctx_len=128, n_parallel=1, ngl=100, device_sampler=key)
        assert st["status_code"] == 200, (st, body)
        for req in (dict(base, top_k=0, top_p=0.9), dict(base, mirostat=2)):
            before = e.sampler_stats("tiny-vocab")
            texts[key, "mirostat" in req] = [e.chat_completion(**req)[-1][1]["choices"][0]["message"]["content"] for _ in range(2)]
            after = e.sampler_stats("tiny-vocab")
            assert (after["device"] > before["device"]) == key and (after["other"] == before["other"]) == key, (key, req, before, after)
            if key:                                                  # a grammar keeps its request on the host chain
                e.chat_completion(**req, grammar='root ::= [a-z]+\n')
                last = e.sampler_stats("tiny-vocab")
                assert last["device"] == after["device"] and last["other"] > after["other"]
        e.close()
    assert all(t[0] == t[1] for t in texts.values())                 # a text depends on the seed alone, on either path
