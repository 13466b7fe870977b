"""qwen3 files on the CPU side: what the synthetic writer puts into them, that it writes every existing configuration byte for byte as before, and that the
composed reference of tests/qwen3_ref.py is the CPU oracle's own graph where the two overlap (a qwen2 file without biases, q / k norm off)."""
import dataclasses
import hashlib

import numpy as np
import pytest

import oracle_py as oq
from gguf_read import read_gguf
from qwen3_ref import Qwen3Ref

QWEN3_CONFIGS = ["tiny-qwen3", "tiny-qwen3-0.6b-2l", "tiny-qwen3-4b-2l", "tiny-qwen3-8b-2l", "qwen3-8b", "qwen3-4b"]


@pytest.mark.parametrize("cfg", QWEN3_CONFIGS)
def test_qwen3_configs_geometry(pkg, cfg):
    gs = pkg.gguf_synth
    c = gs.CONFIGS[cfg]
    assert c.arch == "qwen3" and c.head_dim == 128 and not c.qkv_bias
    E, QW, KV = c.n_embd, c.n_head * 128, c.n_head_kv * 128
    names = {n: (ne, t) for n, ne, t, _ in gs.model_tensors(c, "q4_k_m")}
    assert names["blk.0.attn_q.weight"][0] == (E, QW)
    assert names["blk.0.attn_k.weight"][0] == (E, KV)
    assert names["blk.0.attn_output.weight"][0] == (QW, E)
    assert names["blk.0.attn_q_norm.weight"] == ((128,), gs.F32)
    assert names["blk.0.attn_k_norm.weight"] == ((128,), gs.F32)
    assert not any(n.endswith(".bias") for n in names)
    assert ("output.weight" in names) == (not c.tied_output)
    # the per-token weight bytes count H * D-wide Q / O (and the whole embedding table when it is the output head)
    rb = gs.row_bytes
    want = 0
    for n, (ne, t) in names.items():
        b = rb(t, ne[0]) * int(np.prod(ne)) // ne[0]
        want += rb(t, ne[0]) if n == "token_embd.weight" and not c.tied_output else b
    assert gs.weight_bytes_per_token(c, "q4_k_m") == want
    q_o = sum(rb(names[f"blk.{il}.{k}.weight"][1], names[f"blk.{il}.{k}.weight"][0][0]) * names[f"blk.{il}.{k}.weight"][0][1]
              for il in range(c.n_layer) for k in ("attn_q", "attn_output"))
    assert q_o == c.n_layer * (rb(names["blk.0.attn_q.weight"][1], E) * QW + rb(names["blk.0.attn_output.weight"][1], QW) * E)


@pytest.mark.parametrize("cfg,tied", [("tiny-qwen3", True), ("tiny-qwen3-8b-2l", False)])
def test_qwen3_file_keys_and_tensors(pkg, tmp_path, cfg, tied):
    path = str(tmp_path / f"{cfg}.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, cfg, "q4_k_m", seed=3)
    kv, t = read_gguf(path)
    c = pkg.gguf_synth.CONFIGS[cfg]
    assert kv["general.architecture"] == "qwen3"
    assert kv["qwen3.attention.key_length"] == kv["qwen3.attention.value_length"] == 128
    assert kv["qwen3.rope.dimension_count"] == 128
    assert ("output.weight" in t) == (not tied)
    assert t["blk.0.attn_q.weight"][0] == (c.n_embd, c.n_head * 128)
    for il in range(c.n_layer):
        for k in ("attn_q_norm", "attn_k_norm"):
            ne, ty, raw = t[f"blk.{il}.{k}.weight"]
            w = raw.view("<f4")
            assert ne == (128,) and ty == 0
            # a wide band (a skipped multiply or a norm over the wrong span lands far outside every tolerance)
            assert w.min() >= 0.25 and w.max() <= 2.0 and w.max() - w.min() > 1.0


# SHA-256 of files written by the writer before qwen3 existed (seed 3): the new fields default to the old behaviour, and every tensor's random stream is keyed
# by its own index, so the existing configurations must come out byte for byte the same
DIGESTS = {
    ("tiny", "q4_k_m"): "fd01b687c52097929489f6f796317d160e998cd55ef051bbd7561850760a94fe",
    ("tiny-qwen2", "q5_k_m"): "d39961cc9efcaa219a65707d59ee5341a10d28f4b4748c470cae90fe9c2076c5",
    ("tiny-moe", "q8_0"): "ff489729d10ab50975473017f6e882306711d5d752cec5fbd81ccd51a85e297a",
    ("tiny-gqa4", "q6_k"): "d8b4f8dc706f92f0fd861ae25ef4588ad6a9e0888205c40b8e11ee9f1d37cb3e",
    ("tiny-nomic", "f16"): "2c05b5a7ae827c70cd578b6a97045b8d48dc36adede89a2cdc13b34eb6c80f87",
}


@pytest.mark.parametrize("cfg,ftype", sorted(DIGESTS))
def test_existing_configs_write_identical_files(pkg, tmp_path, cfg, ftype):
    path = str(tmp_path / "x.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, cfg, ftype, seed=3)
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == DIGESTS[(cfg, ftype)]


@pytest.mark.parametrize("ftype,kv", [("q4_k_m", oq.Q8_0), ("q8_0", oq.F16)])
def test_composed_reference_is_the_oracle_graph(pkg, tmp_path, ftype, kv):
    """The composed reference with the q / k norm off, on a qwen2 file without biases, against OracleContext.decode: logits and every layer's residual rows,
    prompt and single-token steps, to f32 round-off - the reference is checked against the oracle's full graph before a GPU test relies on it."""
    c = dataclasses.replace(pkg.gguf_synth.CONFIGS["tiny-qwen2"], name="tiny-qwen2-nobias", qkv_bias=False)
    path = str(tmp_path / "qwen2-nobias.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, c, ftype, seed=5)
    oq.set_fa_v_acc_f32(1 if kv == oq.F16 else 0)
    try:
        om = oq.OracleModel(path)
        oc = oq.OracleContext(om, 64, kv, kv, True, oq.threads())
        ref = Qwen3Ref(path, 64, kv, kv, qk_norm=False)
        rng = np.random.default_rng(2)
        prompt = rng.integers(0, om.n_vocab, 9)
        steps = [(prompt, np.arange(9))] + [([int(t)], [9 + i]) for i, t in enumerate(rng.integers(0, om.n_vocab, 3))]
        for toks, pos in steps:
            a = oc.decode(toks, pos)
            b = ref.decode(toks, pos)
            scale = max(1.0, float(np.abs(a).max()))
            assert np.abs(a - b).max() <= 1e-5 * scale, float(np.abs(a - b).max())
            for il in range(om.n_layer):
                la, lb = oc.layer_out(il, len(toks)), ref.layer_out(il, len(toks))
                assert np.abs(la - lb).max() <= 1e-5 * max(1.0, float(np.abs(la).max())), (il, float(np.abs(la - lb).max()))
        oc.close(); om.close()
    finally:
        oq.set_fa_v_acc_f32(0)


def test_qk_norm_changes_the_result(pkg, tmp_path):
    """On a qwen3 file the q / k norm is not a no-op: with it switched off the reference's logits move by more than the GPU tests' flip tolerance (3e-2)."""
    path = str(tmp_path / "q3.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny-qwen3", "q8_0", seed=5)
    prompt = np.arange(5) * 37 % 768
    on = Qwen3Ref(path, 32, oq.Q8_0, oq.Q8_0).decode(prompt, np.arange(5))
    off = Qwen3Ref(path, 32, oq.Q8_0, oq.Q8_0, qk_norm=False).decode(prompt, np.arange(5))
    assert np.abs(on - off).max() > 0.05 * max(1.0, float(np.abs(on).max()))
