"""Context.lookup_steps (mi355_lookup_steps: draft by prompt lookup on the device, verify, append, roll back) against greedy_steps on the same target, and
the engine's "spec_type": "ngram".  Models, seeds and the length of 7 tokens are those of spec_cases.py, whose cases have no near tie along the emitted path.

Perfect history: prompt + first + the target's own greedy continuation.  lookup_steps appends `first` again, so with ngram_min = 1 the tail's last token occurs
in the history and the rule gives a draft: the condition a case is kept on, asserted below on the CPU side of every case.  With n_max = 2 the rounds after the
first draft from tokens the history took from the verify launch's output on the device, and the counters are those the rule predicts for that history."""
import numpy as np
import pytest

import oracle_py as oq
import spec_cases as sc
from test_gpu_lookup_ops import ngram_rule

pytestmark = pytest.mark.gpu

N_CTX, Q8_0, MODEL_ID = 64, 8, "lookup-target"
GREEDY = dict(temperature=0.0, repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)
LOAD = dict(ctx_len=512, ngl=100, user_prompt="u:", ai_prompt="a:", system_prompt="s:", model=MODEL_ID)
PROMPT = "the quick brown fox jumps over the lazy dog. " * 3


def primed(pkg, model, prompt):
    c = pkg.Context(model, n_ctx=N_CTX, type_k=Q8_0, type_v=Q8_0)
    assert c.decode(prompt, np.arange(prompt.size)) == 0
    return c


def predicted_stats(hist, first, greedy, n_max):
    """the round of mi355_lookup_steps on a target that answers with `greedy`: [rounds, drafted, accepted, plain steps]"""
    h, done, st = hist.tolist() + [first], 0, [0, 0, 0, 0]
    while done < len(greedy):
        draft = ngram_rule(h, 1, 4, n_max)[0]
        a = next((j for j, t in enumerate(draft) if done + j >= len(greedy) or t != greedy[done + j]), len(draft))
        m = min(a + 1, len(greedy) - done)
        st = [st[0] + 1, st[1] + len(draft), st[2] + m - 1, st[3] + (not draft)]
        h += greedy[done:done + m].tolist()
        done += m
    return st


@pytest.mark.parametrize("n_max", [16, 2])
@pytest.mark.parametrize("case", sc.CASES + [sc.MOE_CASE], ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_perfect_and_repeat_free_histories_give_the_greedy_tokens(pkg, tmp_models, case, n_max):
    be, model = pkg.Backend(), pkg.Model(sc.write_pair(pkg.gguf_synth, oq, tmp_models, *case[:2])[0])
    prompt = sc.prompt_of(model.n_vocab, case[2])
    g = primed(pkg, model, prompt)
    first = g.argmax()
    greedy, used = g.greedy_steps(first, sc.N_PROMPT, sc.N_TOKENS), g.kv_used()
    hist = np.concatenate([prompt, [first], greedy]).astype(np.int32)
    assert ngram_rule(hist.tolist() + [first], 1, 4, 16)[0]                            # the condition of the module docstring
    c = primed(pkg, model, prompt)
    toks, stats = c.lookup_steps(hist, first, sc.N_PROMPT, sc.N_TOKENS, ngram_min=1, ngram_max=4, n_max=n_max)
    print(case, n_max, "perfect history:", stats.tolist())
    assert toks.tolist() == greedy.tolist() and stats.tolist() == predicted_stats(hist, first, greedy, n_max)
    assert stats[0] + stats[2] == sc.N_TOKENS and stats[2] > 0 and stats[3] == 0 and (n_max == 16 or stats[0] >= 3)
    assert c.kv_used() == used
    c.close()
    # distinct ids that are not the prompt's (the history is not tied to the cache), a 16-token repeat asked for: 20 tokens cannot hold one
    c = primed(pkg, model, prompt)
    toks, stats = c.lookup_steps(model.n_vocab - 1 - np.arange(sc.N_PROMPT), first, sc.N_PROMPT, sc.N_TOKENS, ngram_min=16, ngram_max=16)
    assert toks.tolist() == greedy.tolist() and stats.tolist() == [sc.N_TOKENS, 0, 0, sc.N_TOKENS]
    assert c.kv_used() == used
    with pytest.raises(pkg.MI355Error, match="exceed n_ctx"):
        c.lookup_steps(np.zeros(N_CTX, np.int32), first, sc.N_PROMPT + sc.N_TOKENS, 1)
    c.close(); g.close(); model.close()


def test_engine_spec_type_ngram(pkg, tmp_models, tmp_path):
    """the same greedy request gives the same text with and without the key and drafts from a prompt that repeats itself; what the key cannot serve is refused"""
    path = sc.write_pair(pkg.gguf_synth, oq, tmp_models, *sc.CASES[0][:2])[0]
    enc = str(tmp_path / "nomic.gguf")
    pkg.gguf_synth.write_synthetic_llama(enc, "tiny-nomic", "q8_0")
    texts, stats = [], []
    for keys in ({}, dict(spec_type="ngram", spec_ngram_min=1, draft_max=4), dict(spec_type="ngram", model_draft=path), dict(llama_model_path=enc, spec_type="ngram"),
                 dict(spec_type="ngram", split_mode="row"), dict(spec_type="ngram", mmproj=str(tmp_path / "p.gguf")), dict(spec_type="draft"),
                 dict(spec_type="ngram", spec_ngram_max=17)):
        e = pkg.Engine()
        try:
            st, body = e.load_model(**{**LOAD, "llama_model_path": path, **keys})
            if len(texts) == 2:
                assert st["has_error"] and st["status_code"] == 500 and "spec_type:" in body.get("error", ""), (keys, st, body)
                continue
            assert st["status_code"] == 200 and not st["has_error"], (st, body)
            st, body = e.chat_completion(model=MODEL_ID, messages=[{"role": "user", "content": PROMPT}], max_tokens=16, **GREEDY)[-1]
            assert st["status_code"] == 200 and not st["has_error"], (st, body)
            texts.append(body["choices"][0]["message"]["content"]); stats.append(e.spec_stats(MODEL_ID))
        finally:
            e.close()
    print("engine:", stats)
    assert texts[0] == texts[1] and stats[0]["drafted"] == 0
    assert stats[1]["rounds"] > 0 and stats[1]["drafted"] > 0 and stats[1]["drafted"] >= stats[1]["accepted"]
