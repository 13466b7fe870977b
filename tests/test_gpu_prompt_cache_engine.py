"""The host-RAM prompt cache through the engine surface (mi355_engine_*, load key "cache_ram"): one slot, conversation A, then an unrelated conversation B,
then A again.  With the cache on, A's KV state comes back from host memory instead of being prefilled again, and the reply is the one the slot's own cache
gives (the control: the same engine sent A, A - the same arithmetic on the same cells).  Without the key nothing changes and every counter stays zero."""
import pytest

pytestmark = pytest.mark.gpu

GREEDY = dict(temperature=0.0, repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0)
MODEL_ID = "tiny-d128"
PROMPT_A = " ".join(["the quick brown fox jumps over the lazy dog and runs far away from the old stone bridge at dawn"] * 3)
PROMPT_B = " ".join(["zebra yaks walk under warm violet umbrellas toward some river while seven geese fly south again"] * 3)
ZERO = dict(entries=0, bytes=0, saves=0, restores=0, tokens_restored=0, evictions=0)


@pytest.fixture(scope="module")
def model_path(pkg, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("pc") / f"{MODEL_ID}.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny-d128", "q4_k_m", with_vocab=True)
    return path


def ask(engine, text):
    st, body = engine.chat_completion(model=MODEL_ID, messages=[{"role": "user", "content": text}], max_tokens=8, **GREEDY)[-1]
    assert st["status_code"] == 200 and not st["has_error"], (st, body)
    return body["choices"][0]["message"]["content"], body["usage"]["prompt_tokens"]


def run(pkg, model_path, order, **load_keys):
    e = pkg.Engine()
    try:
        st, body = e.load_model(llama_model_path=model_path, ctx_len=512, n_parallel=1, ngl=100, user_prompt="u:", ai_prompt="a:", system_prompt="s:", **load_keys)
        assert st["status_code"] == 200 and not st["has_error"], (st, body)
        replies = [ask(e, text) for text in order]
        stats = e.prompt_cache_stats(MODEL_ID)
        with pytest.raises(pkg.MI355Error, match="no model nope"):
            e.prompt_cache_stats("nope")
        return replies, stats
    finally:
        e.close()


@pytest.fixture(scope="module")
def control(pkg, model_path):
    """A, A on an engine without the key: the second reply comes off the slot's own cache."""
    replies, stats = run(pkg, model_path, [PROMPT_A, PROMPT_A])
    assert stats == ZERO
    return replies


def test_a_b_a_restores_a_from_host_memory(pkg, model_path, control):
    replies, stats = run(pkg, model_path, [PROMPT_A, PROMPT_B, PROMPT_A], cache_ram=64)
    n_prompt = replies[0][1]
    print(f"prompt tokens: {n_prompt}")
    assert 100 <= n_prompt <= 480 and replies[2][1] == n_prompt, replies             # (a prompt long enough for the restore rule to apply, and it fits the slot)
    assert replies[0] == control[0]
    assert replies[2][0] == control[1][0], (replies, control)
    assert stats["restores"] == 1 and stats["tokens_restored"] >= n_prompt - 1, stats
    assert stats["saves"] == 2 and stats["entries"] == 2 and stats["evictions"] == 0 and stats["bytes"] > 0, stats


def test_without_the_key_nothing_changes(pkg, model_path, control):
    replies, stats = run(pkg, model_path, [PROMPT_A, PROMPT_B, PROMPT_A])
    assert stats == ZERO
    assert replies[0] == control[0]
    off, stats_off = run(pkg, model_path, [PROMPT_A, PROMPT_B, PROMPT_A], cache_ram=0)
    assert stats_off == ZERO and off == replies
