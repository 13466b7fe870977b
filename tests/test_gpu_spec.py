"""Context.speculative_steps (mi355_speculative_steps: the draft / verify / roll-back round on the C side, its decisions made by the kernels of csrc/spec.hip)
against (a) the same round restated in Python and driven through decode / logits / kv_seq_rm with numpy's arg-max and softmax, and (b) greedy_steps on the
target alone.  The cases (spec_cases.py) are those whose target logits have no near tie along the emitted path and whose draft probabilities keep clear of
p_min - test_spec_cpu.py asserts both on the oracle - so tokens and counters are compared for equality."""
import numpy as np
import pytest

import oracle_py as oq
import spec_cases as sc

pytestmark = pytest.mark.gpu

KV = {"f16": 1, "q8_0": 8}
N_CTX = 64


@pytest.fixture(scope="module")
def be(pkg):
    return pkg.Backend()


@pytest.fixture(scope="module")
def pairs(pkg, tmp_models):
    """case -> (target Model, draft Model), loaded once"""
    cache = {}

    def get(case):
        key = case[:2]
        if key not in cache:
            tgt, dft = sc.write_pair(pkg.gguf_synth, oq, tmp_models, case[0], case[1])
            cache[key] = (pkg.Model(tgt), pkg.Model(dft))
        return cache[key]
    yield get
    for mt, md in cache.values():
        mt.close(); md.close()


def primed(pkg, model, kv, prompt, **kw):
    c = pkg.Context(model, n_ctx=N_CTX, type_k=KV[kv], type_v=KV[kv], **kw)
    assert c.decode(prompt, np.arange(prompt.size)) == 0
    return c


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def run_case(pkg, mt, md, case, kv, n_min=0, n=sc.N_TOKENS):
    """speculative_steps on one pair of contexts, the Python round on a second, greedy_steps on a third; returns what the tests look at"""
    _, _, prompt_seed, n_max, p_min = case
    prompt = sc.prompt_of(mt.n_vocab, prompt_seed)
    ct, cd = primed(pkg, mt, kv, prompt), primed(pkg, md, kv, prompt, logits_to_host=False)
    first = ct.argmax()
    toks, stats = ct.speculative_steps(cd, first, sc.N_PROMPT, n, n_max=n_max, n_min=n_min, p_min=p_min)
    rt, rd = primed(pkg, mt, kv, prompt), primed(pkg, md, kv, prompt)
    assert rt.argmax() == first
    ref_toks, ref_stats, trace = sc.speculative_round_loop(sc.GpuSide(rt), sc.GpuSide(rd), first, sc.N_PROMPT, n, n_max, n_min, p_min)
    g = primed(pkg, mt, kv, prompt)
    greedy = g.greedy_steps(first, sc.N_PROMPT, n)
    # roll-back: one more plain step on the speculated target against a fresh context fed the same tokens
    fresh = pkg.Context(mt, n_ctx=N_CTX, type_k=KV[kv], type_v=KV[kv])
    seq = np.concatenate([prompt, [first], toks[:-1]]).astype(np.int32)
    assert fresh.decode(seq, np.arange(seq.size)) == 0
    assert fresh.decode([toks[-1]], [seq.size]) == 0 and ct.decode([toks[-1]], [seq.size]) == 0
    tail_err = rel_err(ct.logits(), fresh.logits())
    used = (ct.kv_used(), fresh.kv_used())
    for c in (ct, cd, rt, rd, g, fresh):
        c.close()
    return toks, stats, ref_toks, ref_stats, greedy, tail_err, used, trace


@pytest.mark.parametrize("kv", ["q8_0", "f16"])
@pytest.mark.parametrize("case", sc.CASES + [sc.MOE_CASE], ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_speculative_steps_equal_the_round_in_python_and_plain_greedy(be, pkg, pairs, case, kv):
    mt, md = pairs(case)
    toks, stats, ref_toks, ref_stats, greedy, tail_err, used, trace = run_case(pkg, mt, md, case, kv)
    print(f"{case} {kv}: stats {stats.tolist()} rounds {trace['accept']} tail err {tail_err:.3g}")
    assert toks.tolist() == ref_toks.tolist() and stats.tolist() == ref_stats.tolist()           # (a)
    assert toks.tolist() == greedy.tolist()                                                      # (b)
    assert stats[1] > stats[2] > 0 and stats[0] + stats[2] == sc.N_TOKENS                        # every round emits one token of the target's + its accepted drafts
    assert stats[0] == len(trace["accept"]) and stats[3] == sum(k == 0 for k, _ in trace["accept"])
    assert tail_err <= sc.FLIP_TOL and used[0] == used[1]                                        # no stale cell behind the roll-back


def test_n_min_above_what_the_draft_reaches_makes_every_step_plain(be, pkg, pairs):
    case = sc.CASES[0]
    mt, md = pairs(case)
    toks, stats, ref_toks, ref_stats, greedy, tail_err, used, _ = run_case(pkg, mt, md, case, "q8_0", n_min=case[3] + 1)
    assert toks.tolist() == greedy.tolist() == ref_toks.tolist() and stats.tolist() == ref_stats.tolist()
    assert stats[0] == stats[3] == sc.N_TOKENS and stats[1] == stats[2] == 0
    assert tail_err <= sc.FLIP_TOL and used[0] == used[1]


def test_the_target_as_its_own_draft_is_mostly_accepted(be, pkg, pairs):
    """draft == target file: the draft's single-token steps and the target's batched rows differ by rounding only.  The issue's bar, accepted >= drafted / 2,
    is not derived; the measured share is printed."""
    case = sc.CASES[1]
    mt, _ = pairs(case)
    toks, stats, ref_toks, ref_stats, greedy, tail_err, used, _ = run_case(pkg, mt, mt, case, "q8_0")
    print(f"self-draft: drafted {stats[1]} accepted {stats[2]}")
    assert toks.tolist() == greedy.tolist() == ref_toks.tolist() and stats.tolist() == ref_stats.tolist()
    assert stats[1] > 0 and 2 * stats[2] >= stats[1]
    assert tail_err <= sc.FLIP_TOL and used[0] == used[1]


def test_device_decisions_with_logits_left_on_the_device(be, pkg, pairs):
    """argmax_prob and spec_verify read the device logits: the same answers with logits_to_host = 0 as numpy gives on the host rows; a row that was not flagged
    and embeddings mode are refused"""
    case = sc.CASES[0]
    mt, _ = pairs(case)
    prompt = sc.prompt_of(mt.n_vocab, 5)
    on, off = primed(pkg, mt, "q8_0", prompt), primed(pkg, mt, "q8_0", prompt, logits_to_host=False)
    t, p = off.argmax_prob()
    want_t, want_p = sc.softmax_top(on.logits())
    assert t == want_t == off.argmax() and p == pytest.approx(want_p, rel=2e-5)
    batch = np.array([t, 3, 4, 5, 6, 7], np.int32)
    pos = np.arange(6) + prompt.size
    for c in (on, off):
        assert c.decode(batch, pos, logits=[1] * 6) == 0
    rows = np.stack([on.logits(i) for i in range(6)])
    ids = [sc.argmax_rule(r) for r in rows]
    draft = np.array([ids[0], ids[1], 0 if ids[2] else 1, ids[3], ids[4], ids[5]], np.int32)          # group 0 (rows 0 .. 3): two right, then wrong; group 1: one right
    got_ids, got_acc = off.spec_verify([0, 4, 6], draft)
    assert got_ids.tolist() == ids and got_acc.tolist() == [2, 1]
    got_ids, got_acc = off.spec_verify([1, 4], draft[1:4])                                            # a group that starts inside the batch
    assert got_ids.tolist() == ids[1:4] and got_acc.tolist() == [1]
    assert off.decode(batch, pos + 6, logits=[1, 1, 0, 1, 1, 1]) == 0
    with pytest.raises(pkg.binding.MI355Error, match="not flagged"):
        off.spec_verify([0, 4], draft[:4])
    off.set_embeddings(True)
    assert off.decode(batch[:2], pos[:2] + 12, logits=[1, 1]) == 0
    with pytest.raises(pkg.binding.MI355Error, match="embeddings"):
        off.spec_verify([0, 2], draft[:2])
    with pytest.raises(pkg.binding.MI355Error, match="embeddings"):
        off.argmax_prob()
    on.close(); off.close()
