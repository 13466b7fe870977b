"""tools/export_lora.py: the file plumbing with the numpy twin (tests/lora_merge_ref.py) on `tiny` and `tiny-moe`, every refusal by its text, and - on the
device - the merged file against Backend.lora_merge_rows and against the base file with the same adapter applied at run time."""
import importlib.util
import os

import numpy as np
import pytest

import lora_cases as lc
import lora_merge_ref as mr
from gguf_read import read_gguf
from test_lora_cpu import write_adapter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, F16, F32 = "blk.0.attn_q.weight", 1, 0
AD = dict(rank=6, alpha=9.0, targets=lc.ALL7 + ("output",), dtype="f32", seed=8, std=0.1)     # the adapter of test_reference_equals_a_base_with_merged_weights
USER = 0.8


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("export_lora_tool", os.path.join(ROOT, "tools", "export_lora.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def model_file(gs, tmp_models, cfg, ftype="f16"):
    p = str(tmp_models / f"merge-{cfg}-{ftype}.gguf")
    if not os.path.exists(p):
        gs.write_synthetic_llama(p, cfg, ftype, seed=21, with_vocab=False)
    return p


def twin(base_type, rows, ads, out_type):
    return mr.merge_rows(base_type, rows, ads, out_type)[0]


def expert_adapter(gs, path, cfg, name, r=5):
    """an adapter with one 3-D pair on an expert tensor: lora_a [K, r, E], lora_b [r, N, E]"""
    K, N, E = next(ne for n, ne, _, _ in gs.model_tensors(gs.CONFIGS[cfg], "f16") if n == name)
    rng = np.random.default_rng(9)
    w = gs.GGUFWriter()
    for k, v in (("general.architecture", gs.CONFIGS[cfg].arch), ("general.type", "adapter"), ("adapter.type", "lora")):
        w.add(k, "str", v)
    w.add("adapter.lora.alpha", "f32", 10.0)
    w.add_tensor(name + ".lora_a", (K, r, E), F16, (rng.standard_normal(E * r * K) / np.sqrt(K)).astype("<f2").view(np.uint8))
    w.add_tensor(name + ".lora_b", (r, N, E), F16, (rng.standard_normal(E * N * r) * 0.1).astype("<f2").view(np.uint8))
    w.write(path)
    return path


@pytest.mark.parametrize("cfg,chunk_bytes", [("tiny", 1 << 30), ("tiny-moe", 37 * 256 * 4)])
def test_merge_file_with_the_twin(pkg, tool, tmp_models, tmp_path, cfg, chunk_bytes):
    gs = pkg.gguf_synth
    base, dst, ad1 = model_file(gs, tmp_models, cfg), str(tmp_path / "merged.gguf"), str(tmp_path / "ad.gguf")
    gs.write_synthetic_lora(ad1, cfg, **(AD if cfg == "tiny" else dict(rank=4, alpha=10.0, targets=("attn_q", "blk.1.attn_v.weight"), std=0.1)))
    ads = [(ad1, USER)] + ([(expert_adapter(gs, str(tmp_path / "ex.gguf"), cfg, "blk.0.ffn_up_exps.weight"), -0.5)] if cfg == "tiny-moe" else [])
    tool.merge_file(base, ads, dst, merge_rows=twin, chunk_bytes=chunk_bytes, out=lambda s: None)
    (kv0, t0), (kv1, t1) = read_gguf(base), read_gguf(dst)
    assert list(kv1) == list(kv0) and kv1 == kv0 and list(t1) == list(t0)
    files = [(read_gguf(p), u) for p, u in ads]
    n_merged = 0
    for name, (ne, ty, raw) in t1.items():
        pairs = [(t, u * kv["adapter.lora.alpha"] / t[name + ".lora_a"][0][1]) for (kv, t), u in files if name + ".lora_a" in t]
        if not pairs:
            assert (ne, ty) == t0[name][:2] and raw.tobytes() == t0[name][2].tobytes(), name
            continue
        n_merged += 1
        K, N, E = ne[0], ne[1], ne[2] if len(ne) == 3 else 1
        assert ty == F16 and ne == t0[name][0]
        got = raw[:E * N * K * 2].view("<f2").reshape(E, N, K)
        for e in range(E):
            w = t0[name][2][:E * N * K * 2].reshape(E, N, K * 2)[e]
            one = []
            for t, s in pairs:
                (_, r, *_), ta, a = t[name + ".lora_a"]
                dt = "<f2" if ta == F16 else "<f4"
                b = t[name + ".lora_b"][2]
                one.append((a[:E * r * K * int(dt[2])].view(dt).reshape(E, r, K)[e], b[:E * N * r * int(dt[2])].view(dt).reshape(E, N, r)[e], s))
            assert got[e].tobytes() == twin(F16, w, one, F16).tobytes(), (name, e)
    assert n_merged == (len(lc.ALL7) * gs.CONFIGS[cfg].n_layer + 1 if cfg == "tiny" else gs.CONFIGS[cfg].n_layer + 2)


PAIR = [(Q + ".lora_a", (256, 4), F16), (Q + ".lora_b", (4, 256), F16)]
REFUSALS = [
    ("shape", "f16", dict(tensors=[(Q + ".lora_a", (128, 4), F16), (Q + ".lora_b", (4, 256), F16)]),
     f"adapter pair {Q}: lora_a is [128, 4] and lora_b is [4, 256] where the base tensor is [256, 256] (lora_a [K, r], lora_b [r, N])"),
    ("halves", "f16", dict(tensors=[(Q + ".lora_a", (256, 4), F16), (Q + ".lora_b", (8, 256), F16)]), f"adapter pair {Q}: lora_a is [256, 4] and lora_b is [8, 256] (lora_a [K, r], lora_b [r, N])"),
    ("no-b", "f16", dict(tensors=PAIR[:1]), f"adapter tensor {Q}.lora_a has no {Q}.lora_b beside it"),
    ("no-a", "f16", dict(tensors=PAIR[1:]), f"adapter tensor {Q}.lora_b has no {Q}.lora_a beside it"),
    ("alpha-missing", "f16", dict(tensors=PAIR, alpha=None), "adapter.lora.alpha is missing or not an f32"),
    ("rank", "f16", dict(tensors=[(Q + ".lora_a", (256, 513), F16), (Q + ".lora_b", (513, 256), F16)]), f"adapter pair {Q}: rank 513 is outside 1 .. 512"),
    ("base-type", "q2_k", dict(tensors=PAIR), f"{Q}: the base tensor is q2_K, which the merge does not read (f32, f16, bf16, q8_0, q4_K, q5_K and q6_K are)"),
    ("arch", "f16", dict(tensors=PAIR, arch="qwen2"), "adapter architecture 'qwen2' does not match the base file's 'llama'"),
]


@pytest.mark.parametrize("name,ftype,spec,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(pkg, tool, tmp_models, tmp_path, name, ftype, spec, text):
    gs = pkg.gguf_synth
    ad = write_adapter(gs, str(tmp_path / "bad.gguf"), **spec)

    def no_device(*a):
        raise AssertionError("a refusal comes before any merge")

    with pytest.raises(ValueError) as e:
        tool.merge_file(model_file(gs, tmp_models, "tiny", ftype), [(ad, 1.0)], str(tmp_path / "out.gguf"), merge_rows=no_device, out=lambda s: None)
    assert str(e.value) == f"{ad}: {text}" or str(e.value) == text
    assert not os.path.exists(str(tmp_path / "out.gguf"))


@pytest.mark.gpu
def test_the_tool_on_the_device_against_the_run_time_adapter(pkg, tool, tmp_models, tmp_path):
    """The merged file's logits for 12 prompt tokens against the base file's with the adapter set at run time.  Yardstick: the same comparison on the CPU
    reference (the merged file under Qwen3Ref against the base under LoraRef), of which the device may take twice: both sides carry the merged weights' one
    f16 rounding, the device its own f32 summation orders on top.  The figure must also stay below the distance to the base without the adapter."""
    import oracle_py as oq
    from lora_ref import Adapter, LoraRef
    from qwen3_ref import Qwen3Ref
    gs = pkg.gguf_synth
    base, dst, adp = model_file(gs, tmp_models, "tiny"), str(tmp_path / "merged.gguf"), str(tmp_path / "ad.gguf")
    gs.write_synthetic_lora(adp, "tiny", **AD)
    assert tool.main(["-m", base, "--lora-scaled", adp, str(USER), "-o", dst]) == 0
    be = pkg.Backend()
    (_, t0), (_, t1), ad = read_gguf(base), read_gguf(dst), Adapter(adp)
    for name in (Q, "output.weight"):
        (K, N), _, raw = t0[name]
        a, b = ad.t[name + ".lora_a"][2].view("<f4").reshape(6, K), ad.t[name + ".lora_b"][2].view("<f4").reshape(N, 6)
        assert t1[name][1] == F16 and t1[name][2][:N * K * 2].tobytes() == be.lora_merge_rows(F16, raw[:N * K * 2].reshape(N, K * 2), [(a, b, USER * 9.0 / 6)]).tobytes()
    prompt = np.random.default_rng(4).integers(0, gs.CONFIGS["tiny"].n_vocab, 12).astype(np.int32)
    pos = np.arange(12)

    def device_logits(path, adapter=None):
        m = pkg.Model(path)
        c = pkg.Context(m, n_ctx=32, n_ubatch=32)
        la = pkg.binding.LoraAdapter(m, adapter) if adapter else None
        if la:
            c.set_adapter_lora(la, USER)
        assert c.decode(prompt, pos) == 0
        y = np.array(c.logits(), np.float32, copy=True)
        c.close()
        if la:
            la.close()
        m.close()
        return y

    d_merged, d_lora, d_base = device_logits(dst), device_logits(base, adp), device_logits(base)
    oq.set_fa_v_acc_f32(1)
    try:
        r_lora = LoraRef(base, 32, 1, 1)
        r_lora.set_adapters([(ad, USER)])
        o_lora, o_merged = r_lora.decode(prompt, pos)[0], Qwen3Ref(dst, 32, 1, 1).decode(prompt, pos)[0]
    finally:
        oq.set_fa_v_acc_f32(0)
    dev, ref, moved = lc.rel_err(d_merged, d_lora), lc.rel_err(o_merged, o_lora), lc.rel_err(d_merged, d_base)
    print(f"merged against run-time adapter: device {dev:.3e}, CPU reference {ref:.3e}; merged against the base alone: {moved:.3e}")
    assert dev <= 2 * ref and dev < moved
