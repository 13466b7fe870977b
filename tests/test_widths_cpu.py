"""Hidden sizes that are whole 32-element blocks but no multiple of 256 (Qwen2.5-0.5B's 896, SmolLM2-135M's 576), CPU side: the synthetic writer's
fallback types for such rows, the CPU references on the new configs, and the files of the older configs, which must not change by a byte."""
import hashlib

import numpy as np
import pytest

import oracle_py as oq
import q41_q51_ref as mr

NEW_TINY = ["tiny-w896-2l", "tiny-w896-2l-untied", "tiny-w576-2l", "tiny-w320"]


@pytest.fixture(scope="module")
def gs(pkg):
    return pkg.gguf_synth


def types_of(gs, cfg, ftype):
    return {name: (ne[0], gs.TYPE_NAME[t]) for name, ne, t, _ in gs.model_tensors(gs.CONFIGS[cfg], ftype) if len(ne) > 1}


def test_k_quant_mixes_fall_back_to_32_element_types_row_by_row(gs):
    """tiny-w896-2l (n_embd 896 = 3.5 x 256, n_ff 4864 = 19 x 256): every tensor over n_embd or the attention width takes its mix's type's fallback -
    Q4_K -> Q5_0, Q5_K -> Q5_1, Q6_K -> Q8_0, Q2_K / Q3_K / IQ4_XS -> IQ4_NL - the tied token_embd included; ffn_down (rows of 4864) keeps its K-quant."""
    t = types_of(gs, "tiny-w896-2l", "q4_k_m")
    assert t["token_embd.weight"] == (896, "q5_0")
    for il in (0, 1):
        for k in ("attn_q", "attn_k", "attn_output", "ffn_gate", "ffn_up"):
            assert t[f"blk.{il}.{k}.weight"] == (896, "q5_0"), (il, k)
    assert t["blk.0.attn_v.weight"] == (896, "q5_0") and t["blk.1.attn_v.weight"] == (896, "q8_0")      # (layer 1: the mix's "more bits" Q6_K)
    assert t["blk.0.ffn_down.weight"] == (4864, "q4_K") and t["blk.1.ffn_down.weight"] == (4864, "q6_K")

    t = types_of(gs, "tiny-w896-2l", "q5_k_m")
    assert t["token_embd.weight"] == (896, "q5_1") and t["blk.0.attn_q.weight"] == (896, "q5_1") and t["blk.1.attn_v.weight"] == (896, "q8_0")
    assert t["blk.0.ffn_down.weight"] == (4864, "q5_K") and t["blk.1.ffn_down.weight"] == (4864, "q6_K")

    t = types_of(gs, "tiny-w896-2l", "q2_k")
    assert t["token_embd.weight"] == (896, "iq4_nl") and t["blk.0.attn_q.weight"] == (896, "iq4_nl") and t["blk.0.attn_output.weight"] == (896, "iq4_nl")
    assert t["blk.0.attn_v.weight"] == (896, "q5_0")                   # (7 query heads per kv head: the mix's Q4_K)
    assert t["blk.0.ffn_down.weight"] == (4864, "q3_K")

    t = types_of(gs, "tiny-w896-2l", "iq4_xs")
    assert t["token_embd.weight"] == (896, "iq4_nl") and t["blk.0.ffn_gate.weight"] == (896, "iq4_nl")
    assert t["blk.0.attn_v.weight"] == (896, "q5_1")                   # (the mix's Q5_K)
    assert t["blk.0.ffn_down.weight"] == (4864, "q5_K") and t["blk.1.ffn_down.weight"] == (4864, "iq4_xs")

    # an untied head (the mixes' Q6_K) falls back too; a width where n_ff ends inside a 256-group as well
    assert types_of(gs, "tiny-w896-2l-untied", "q4_k_m")["output.weight"] == (896, "q8_0")
    t = types_of(gs, "tiny-w320", "q4_k_m")
    assert t["blk.0.ffn_down.weight"] == (608, "q5_0") and t["blk.1.ffn_down.weight"] == (608, "q8_0") and t["output.weight"] == (320, "q8_0")
    # every tensor of every new config holds whole blocks of its type
    for cfg in NEW_TINY + ["qwen2.5-0.5b", "smollm2-135m"]:
        for ftype in ("q4_k_m", "q5_k_m", "q2_k", "q3_k_m", "iq4_xs", "q6_k", "q8_0", "q5_0", "q4_1", "mxfp4", "f16"):
            for name, ne, ty, _ in gs.model_tensors(gs.CONFIGS[cfg], ftype):
                assert ne[0] % gs.BLOCK_ELEMS[ty] == 0, (cfg, ftype, name)


def test_full_size_configs_have_the_published_geometry(gs):
    q, s = gs.CONFIGS["qwen2.5-0.5b"], gs.CONFIGS["smollm2-135m"]
    assert (q.n_embd, q.n_layer, q.n_head, q.n_head_kv, q.n_ff, q.n_vocab, q.arch, q.qkv_bias, q.tied_output, q.head_dim) == (896, 24, 14, 2, 4864, 151936, "qwen2", True, True, 64)
    assert (s.n_embd, s.n_layer, s.n_head, s.n_head_kv, s.n_ff, s.n_vocab, s.arch, s.qkv_bias, s.tied_output, s.head_dim) == (576, 30, 9, 3, 1536, 49152, "llama", False, True, 64)
    w = gs.CONFIGS["tiny-w320"]
    assert (w.n_embd, w.n_layer, w.n_head, w.n_head_kv, w.n_ff, w.n_vocab, w.arch, w.qkv_bias, w.tied_output) == (320, 2, 5, 1, 608, 512, "qwen2", True, False)


@pytest.mark.parametrize("ftype", ["q8_0", "q4_k_m", "q5_0", "q4_1"])
@pytest.mark.parametrize("cfg", NEW_TINY)
def test_cpu_reference_runs_the_new_configs(gs, tmp_models, cfg, ftype):
    """A 21-token prompt and one step on the CPU reference (the oracle; the restatement of tests/q41_q51_ref.py over it for a file with Q4_1 tensors, which
    the oracle does not have): finite logits of the vocabulary's size."""
    path = str(tmp_models / f"{cfg}-{ftype}-11.gguf")
    gs.write_synthetic_llama(path, cfg, ftype, seed=11)
    prompt = np.random.default_rng(5).integers(0, 512, 21)
    if ftype == "q4_1":
        ref = mr.MinRef(path, 64, oq.Q8_0, oq.Q8_0)
        om = None
    else:
        om = oq.OracleModel(path)
        ref = oq.OracleContext(om, 64, oq.Q8_0, oq.Q8_0, True, oq.threads())
    a = np.asarray(ref.decode(prompt, np.arange(21))[0])
    b = np.asarray(ref.decode([int(a.argmax())], [21])[0])
    assert a.shape == b.shape == (512,) and np.isfinite(a).all() and np.isfinite(b).all()
    assert np.abs(a).max() > 0 and not np.array_equal(a, b)
    if om is not None:
        ref.close(); om.close()


# sha256 of the files the writer produced before the fallback and the new configs existed (config, ftype, seed)
OLD_FILES = {
    ("tiny", "q4_k_m", 7): "9eb766c845d46d8e3519fc20dd8e3d56564bb35d4081299da8cd9635034292e9",
    ("tiny-qwen3", "iq4_xs", 11): "9c184363c5855ccf2cf32d6ee7d52a2d50433d21fade80286eec82cf2d4d6ddf",
    ("tiny-moe", "q5_k_m", 3): "d59e2bcc07ee9f8eafcb6c10d488ccc1806d7082f73a3f47d0f28ab9a5827b2a",
    ("tiny-qwen2", "q2_k", 5): "ec0858342cb703d8965100096cd98ddf9ac53738c94bda389b91008ef155c5a2",
}


@pytest.mark.parametrize("key", list(OLD_FILES))
def test_older_configs_write_the_same_bytes(gs, tmp_path, key):
    cfg, ftype, seed = key
    path = str(tmp_path / "m.gguf")
    gs.write_synthetic_llama(path, cfg, ftype, seed=seed)
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == OLD_FILES[key]


def test_no_older_config_has_a_row_that_falls_back(gs):
    """The fallback changes a type only where a row is no multiple of 256: no config from before has such a row under a 256-block mix (tiny-qwen3's IQ4_XS mix
    already took IQ4_NL there by its own rule), so tensor_type and the mix agree on all of them."""
    for name, cfg in gs.CONFIGS.items():
        if name in NEW_TINY or name in ("qwen2.5-0.5b", "smollm2-135m"):
            continue
        for ftype in gs.FTYPE_ID:
            for kind in ("token_embd", "attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down", "output", "attn_qkv"):
                for il in range(min(cfg.n_layer, 4)):
                    assert gs.tensor_type(cfg, ftype, kind, il) == gs.mix_tensor_type(cfg, ftype, kind, il), (name, ftype, kind, il)
