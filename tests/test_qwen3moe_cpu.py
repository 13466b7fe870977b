"""qwen3moe files on the CPU side: what the synthetic writer puts into them, the numpy restatement of the router's selection against the oracle's
oq_moe_route, and the composed reference of tests/qwen3moe_ref.py against the CPU oracle's own graph where the two overlap (a Mixtral-style llama file with
at most 64 experts)."""
import numpy as np
import pytest

import oracle_py as oq
from gguf_read import read_gguf
from qwen3moe_ref import Qwen3MoeRef, route_numpy

QWEN3MOE_CONFIGS = ["qwen3-30b-a3b", "tiny-qwen3moe", "tiny-qwen3moe-160e", "tiny-qwen3moe-30b-2l", "tiny-qwen3moe-235b-2l"]


@pytest.mark.parametrize("cfg", QWEN3MOE_CONFIGS)
def test_qwen3moe_configs_geometry(pkg, cfg):
    gs = pkg.gguf_synth
    c = gs.CONFIGS[cfg]
    assert c.arch == "qwen3moe" and c.head_dim == 128 and not c.qkv_bias and c.n_expert >= 128 and c.n_expert_used == 8
    E, QW, KV, X, F = c.n_embd, c.n_head * 128, c.n_head_kv * 128, c.n_expert, c.n_ff_exp
    assert QW > E
    names = {n: (ne, t) for n, ne, t, _ in gs.model_tensors(c, "q4_k_m")}
    assert names["blk.0.attn_q.weight"][0] == (E, QW) and names["blk.0.attn_k.weight"][0] == (E, KV)
    assert names["blk.0.attn_q_norm.weight"] == ((128,), gs.F32) and names["blk.0.attn_k_norm.weight"] == ((128,), gs.F32)
    assert names["blk.0.ffn_gate_inp.weight"] == ((E, X), gs.F32)
    assert names["blk.0.ffn_gate_exps.weight"][0] == (E, F, X) and names["blk.0.ffn_up_exps.weight"][0] == (E, F, X)
    assert names["blk.0.ffn_down_exps.weight"][0] == (F, E, X)
    assert not any(n.endswith(".bias") or ".ffn_gate.weight" in n or "shexp" in n for n in names)
    # the grouped prompt kernels' shapes (N % 128, K % 256) and the 8-expert single-token launches
    assert F % 128 == 0 and E % 256 == 0 and F % 256 == 0


def test_qwen3_30b_a3b_size(pkg):
    """Qwen3-30B-A3B Q4_K_M: an ~18.6 GB file of which ~1.9 GB is read per decoded token (8 of 128 experts)."""
    gs = pkg.gguf_synth
    c = gs.CONFIGS["qwen3-30b-a3b"]
    total = sum(gs.row_bytes(t, ne[0]) * int(np.prod(ne)) // ne[0] for _, ne, t, _ in gs.model_tensors(c, "q4_k_m"))
    assert 18.0e9 < total < 19.0e9, total
    assert 1.8e9 < gs.weight_bytes_per_token(c, "q4_k_m") < 2.0e9


def test_qwen3moe_file_keys(pkg, tmp_path):
    path = str(tmp_path / "m.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny-qwen3moe", "q4_k_m", seed=3)
    kv, t = read_gguf(path)
    assert kv["general.architecture"] == "qwen3moe"
    assert kv["qwen3moe.expert_count"] == 128 and kv["qwen3moe.expert_used_count"] == 8
    assert kv["qwen3moe.expert_feed_forward_length"] == 256 and kv["qwen3moe.feed_forward_length"] == 1536
    assert kv["qwen3moe.attention.key_length"] == kv["qwen3moe.attention.value_length"] == 128
    assert t["blk.2.ffn_down_exps.weight"][0] == (256, 512, 128)
    assert "blk.0.attn_q_norm.weight" in t and "blk.0.ffn_gate.weight" not in t


@pytest.mark.parametrize("n_expert,k", [(8, 2), (60, 4), (64, 8), (64, 1), (17, 3)])
def test_selection_restatement_is_oq_moe_route(n_expert, k):
    """route_numpy (soft_max, first-max top-k, f32 renormalisation) gives oq_moe_route's ids and weights bit for bit, ties included."""
    rng = np.random.default_rng(n_expert * 10 + k)
    for trial in range(200):
        x = (rng.standard_normal(n_expert) * 3).astype(np.float32)
        if trial % 3 == 0:
            x = np.round(x)                                       # many exact ties
        if trial % 7 == 0:
            x[:] = 0.5                                            # all equal
        a_ids, a_w = oq.moe_route(x, k)
        b_ids, b_w = route_numpy(x, k)
        assert (a_ids == b_ids).all(), (trial, a_ids, b_ids)
        assert a_w.view(np.uint32).tolist() == b_w.view(np.uint32).tolist(), trial


@pytest.mark.parametrize("ftype,kv", [("q4_k_m", oq.Q8_0), ("q8_0", oq.F16)])
def test_composed_moe_reference_is_the_oracle_graph(pkg, tmp_path, ftype, kv):
    """The composed reference on a Mixtral-style file (llama graph, 8 experts, 2 used) against OracleContext.decode: logits, every layer's residual rows and
    the recorded expert ids, prompt and single-token steps - the routed feed-forward is checked against the oracle's before a GPU test relies on it."""
    path = str(tmp_path / "moe.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny-moe", ftype, seed=5)
    oq.set_fa_v_acc_f32(1 if kv == oq.F16 else 0)
    try:
        om = oq.OracleModel(path)
        oc = oq.OracleContext(om, 64, kv, kv, True, oq.threads())
        ref = Qwen3MoeRef(path, 64, kv, kv)
        rng = np.random.default_rng(2)
        prompt = rng.integers(0, om.n_vocab, 9)
        steps = [(prompt, np.arange(9))] + [([int(t)], [9 + i]) for i, t in enumerate(rng.integers(0, om.n_vocab, 3))]
        for toks, pos in steps:
            oq.moe_record_start()
            a = oc.decode(toks, pos)
            rec = oq.moe_record_get()
            oq.moe_record_start(0)
            b = ref.decode(toks, pos)
            assert (ref.routes[-1].reshape(-1) == rec).all()
            assert ref.routes[-1].shape == (om.n_layer, len(toks), 2)
            scale = max(1.0, float(np.abs(a).max()))
            assert np.abs(a - b).max() <= 1e-5 * scale, float(np.abs(a - b).max())
            for il in range(om.n_layer):
                la, lb = oc.layer_out(il, len(toks)), ref.layer_out(il, len(toks))
                assert np.abs(la - lb).max() <= 1e-5 * max(1.0, float(np.abs(la).max())), (il, float(np.abs(la - lb).max()))
        oc.close(); om.close()
    finally:
        oq.set_fa_v_acc_f32(0)


def test_qwen3moe_reference_routes_and_qk_norm(pkg, tmp_path):
    """On a qwen3moe file the reference records 8 distinct experts per token and layer, spread over many of the 128 (what the GPU tests hand over through
    force_moe_ids), and its q / k norm is not a no-op."""
    path = str(tmp_path / "q3m.gguf")
    pkg.gguf_synth.write_synthetic_llama(path, "tiny-qwen3moe", "q8_0", seed=5)
    prompt = np.arange(5) * 37 % 768
    ref = Qwen3MoeRef(path, 32, oq.Q8_0, oq.Q8_0)
    a = ref.decode(prompt, np.arange(5))
    r = ref.routes[-1]
    assert r.shape == (3, 5, 8) and len(np.unique(r)) > 16             # many experts in use
    for t in r.reshape(-1, 8):
        assert len(set(t.tolist())) == 8                               # 8 distinct experts per token
    off = Qwen3MoeRef(path, 32, oq.Q8_0, oq.Q8_0, qk_norm=False).decode(prompt, np.arange(5))
    assert np.abs(a - off).max() > 0.05 * max(1.0, float(np.abs(a).max()))
