"""Speculative decoding through the engine surface (mi355_engine_*, load key "model_draft"): the same greedy request gives the same text with and without a
draft model, the counters of mi355_engine_spec_stats move, a sampled request and two concurrent ones complete, and every load the key cannot serve is refused
with a message that names it.  The model pairs are those of spec_cases.py."""
import threading

import pytest

import oracle_py as oq
import spec_cases as sc

pytestmark = pytest.mark.gpu

GREEDY = dict(temperature=0.0, repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)
MODEL_ID = "spec-target"
PROMPTS = ["the quick brown fox jumps over the lazy dog", "zebra yaks walk under warm violet umbrellas"]
SAMPLED = dict(temperature=0.9, top_k=20, seed=7)
ZERO = dict(rounds=0, drafted=0, accepted=0, plain_steps=0)
LOAD = dict(ctx_len=512, ngl=100, user_prompt="u:", ai_prompt="a:", system_prompt="s:", model=MODEL_ID)


@pytest.fixture(scope="module")
def pair(pkg, tmp_path_factory):
    cfg, seed = sc.CASES[0][:2]
    return sc.write_pair(pkg.gguf_synth, oq, tmp_path_factory.mktemp("spec_engine"), cfg, seed)


def text_of(engine, prompt, **kw):
    st, body = engine.chat_completion(model=MODEL_ID, messages=[{"role": "user", "content": prompt}], max_tokens=16, **kw)[-1]
    assert st["status_code"] == 200 and not st["has_error"], (st, body)
    return body["choices"][0]["message"]["content"]


def loaded(pkg, path, **keys):
    e = pkg.Engine()
    st, body = e.load_model(llama_model_path=path, **LOAD, **keys)
    assert st["status_code"] == 200 and not st["has_error"], (st, body)
    return e


@pytest.fixture(scope="module")
def plain_texts(pkg, pair):
    e = loaded(pkg, pair[0], n_parallel=2)
    try:
        texts = [text_of(e, p, **GREEDY) for p in PROMPTS] + [text_of(e, PROMPTS[0], **SAMPLED)]
        assert e.spec_stats(MODEL_ID) == ZERO
        with pytest.raises(pkg.MI355Error, match="no model nope"):
            e.spec_stats("nope")
        return texts
    finally:
        e.close()


@pytest.mark.parametrize("draft", ["coarse", "self"])
def test_greedy_text_is_the_same_with_a_draft_model(pkg, pair, plain_texts, draft):
    # draft_p_min 0.2: these random models are rarely surer than that of their top token (spec_cases.py)
    e = loaded(pkg, pair[0], n_parallel=2, model_draft=pair[1] if draft == "coarse" else pair[0], draft_max=4, draft_p_min=0.2)
    try:
        texts = [text_of(e, p, **GREEDY) for p in PROMPTS]
        stats = e.spec_stats(MODEL_ID)
        print(draft, stats)
        assert texts == plain_texts[:2]
        assert stats["rounds"] > 0 and stats["drafted"] >= stats["accepted"] > 0, stats
        # a sampled request walks its rows through the device top-k front, as it does without a draft: the same seed gives the text of the engine without a
        # draft model, and it drafted
        before = stats["drafted"]
        assert text_of(e, PROMPTS[0], **SAMPLED) == plain_texts[2]
        assert e.spec_stats(MODEL_ID)["drafted"] > before
        # two concurrent requests: both speculate in shared ticks and each equals its serial text
        out = [None, None]

        def run(i):
            out[i] = text_of(e, PROMPTS[i], **GREEDY)
        th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        [t.start() for t in th]
        [t.join(120) for t in th]
        assert out == plain_texts[:2]
    finally:
        e.close()


def test_loads_the_key_cannot_serve_are_refused_by_name(pkg, pair, tmp_path):
    other = str(tmp_path / "gqa4.gguf")
    pkg.gguf_synth.write_synthetic_llama(other, "tiny-gqa4", "q8_0")                     # 768 tokens against 512
    enc = str(tmp_path / "nomic.gguf")
    pkg.gguf_synth.write_synthetic_llama(enc, "tiny-nomic", "q8_0")
    cases = [
        (dict(llama_model_path=pair[0], model_draft=str(tmp_path / "missing.gguf")), "model_draft"),
        (dict(llama_model_path=pair[0], model_draft=enc), "model_draft"),
        (dict(llama_model_path=enc, model_draft=pair[1]), "model_draft"),
        (dict(llama_model_path=pair[0], model_draft=pair[1], split_mode="row"), "model_draft"),
        (dict(llama_model_path=pair[0], model_draft=pair[1], mmproj=str(tmp_path / "proj.gguf")), "model_draft"),
        (dict(llama_model_path=pair[0], model_draft=other), "model_draft"),
    ]
    for keys, word in cases:
        e = pkg.Engine()
        try:
            st, body = e.load_model(**LOAD, **keys)
            assert st["has_error"] and st["status_code"] == 500, (keys, st, body)
            assert word in body.get("error", ""), (keys, body)
        finally:
            e.close()
