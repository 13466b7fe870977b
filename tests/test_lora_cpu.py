"""LoRA adapter files without a GPU: what the synthetic writer puts into a file, the reference with adapters (tests/lora_ref.py) against a base whose
weights were merged in float64, every refusal of host/lora.cc by its full text (tests/host/lora_plan_main.cc), and the delta condition of the
end-to-end cases (tests/lora_cases.py): the reference alone moves the logits by 10 * FLIP_TOL and more on each of them."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import lora_cases as lc
import oracle_py as oq
from gguf_read import read_gguf
from lora_ref import Adapter, LoraRef
from qwen3_ref import Qwen3Ref
from test_gpu_model import TIGHT_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cortex.llamacpp_amd", "host")
F32, F16, Q8_0 = 0, 1, 8
TARGETS_MSG = "(adapters apply to blk.N.{attn_q,attn_k,attn_v,attn_output,ffn_gate,ffn_up,ffn_down}.weight and output.weight)"


@pytest.fixture(scope="module")
def gs(pkg):
    return pkg.gguf_synth


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lora_plan") / "lora_plan_main")
    srcs = [os.path.join(ROOT, "tests", "host", "lora_plan_main.cc")] + [os.path.join(HOST, f) for f in ("gguf.cc", "model_plan.cc", "lora.cc")]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread", *srcs, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def plan(exe, base, adapter, *more):
    r = subprocess.run([exe, base, adapter, *[str(x) for x in more]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def base_model(gs, tmp_models, cfg, ftype="q4_k_m"):
    path = str(tmp_models / f"lorabase-{cfg}-{ftype}.gguf")
    if not os.path.exists(path):
        gs.write_synthetic_llama(path, cfg, ftype, seed=3, with_vocab=False)
    return path


def write_adapter(gs, path, tensors, arch="llama", gtype="adapter", atype="lora", alpha=("f32", 8.0)):
    """An adapter-shaped file with zero payloads: tensors = [(name, ne, ggml type)]; a None key value leaves the key out."""
    w = gs.GGUFWriter()
    w.add("general.architecture", "str", arch)
    if gtype is not None:
        w.add("general.type", "str", gtype)
    if atype is not None:
        w.add("adapter.type", "str", atype)
    if alpha is not None:
        w.add("adapter.lora.alpha", alpha[0], alpha[1])
    for name, ne, t in tensors:
        w.add_tensor(name, ne, t, np.zeros(gs.row_bytes(t, ne[0]) * int(np.prod(ne[1:])), np.uint8))
    w.write(path)
    return path


# ------------------------------------------------------------------------------------------------ the writer
@pytest.mark.parametrize("cfg,dtype,rank,targets", [("tiny-d128", "f16", 8, lc.ALL7 + ("output",)), ("tiny-qwen3", "f32", 3, ("attn_q", "ffn_down", "output")),
                                                    ("tiny-moe", "f16", 4, ("attn_q", "blk.1.attn_v.weight"))])
def test_writer_file_reads_back(gs, tmp_path, plan_exe, tmp_models, cfg, dtype, rank, targets):
    c = gs.CONFIGS[cfg]
    path = str(tmp_path / "a.gguf")
    gs.write_synthetic_lora(path, cfg, rank=rank, alpha=2.5 * rank, targets=targets, dtype=dtype, seed=5, std=0.1)
    kv, t = read_gguf(path)
    assert kv["general.type"] == "adapter" and kv["adapter.type"] == "lora" and kv["general.architecture"] == c.arch
    assert kv["adapter.lora.alpha"] == pytest.approx(2.5 * rank)
    shapes = {name: ne for name, ne, _, _ in gs.model_tensors(c, "f16")}
    shapes.setdefault("output.weight", shapes["token_embd.weight"])
    want = []
    for tg in targets:
        want += [f"blk.{il}.{tg}.weight" for il in range(c.n_layer)] if tg in lc.ALL7 else ["output.weight"] if tg == "output" else [tg]
    assert sorted(t) == sorted([n + h for n in want for h in (".lora_a", ".lora_b")])
    ty = {"f16": F16, "f32": F32}[dtype]
    for n in want:
        K, N = shapes[n]
        assert t[n + ".lora_a"][:2] == ((K, rank), ty) and t[n + ".lora_b"][:2] == ((rank, N), ty)
        b = t[n + ".lora_b"][2].view("<f2" if ty == F16 else "<f4").astype(np.float64)
        assert 0.5 * 0.1 < b.std() < 1.5 * 0.1                       # (lora_b is not the all-zero tensor of an untrained adapter)
    # ... and the loader's host half accepts it: every pair, with the scale user_scale * alpha / r
    p = plan(plan_exe, base_model(gs, tmp_models, cfg), path, 0.5)
    assert p["status"] == 0 and p["alpha"] == pytest.approx(2.5 * rank)
    assert [q["base"] for q in p["pairs"]] == want
    for q in p["pairs"]:
        assert (q["r"], q["type"], q["K"], q["N"]) == (rank, dtype, *shapes[q["base"]]) and q["scale"] == pytest.approx(0.5 * 2.5)


def test_alpha_zero_scale_is_the_user_scale(gs, tmp_path, plan_exe, tmp_models):
    path = str(tmp_path / "a.gguf")
    gs.write_synthetic_lora(path, "tiny", rank=4, alpha=0.0, targets=("attn_q",))
    p = plan(plan_exe, base_model(gs, tmp_models, "tiny"), path, -0.75)
    assert p["status"] == 0 and all(q["scale"] == -0.75 for q in p["pairs"])


# ------------------------------------------------------------------------------------------------ the reference
def test_scale_zero_is_the_base_model_bit_for_bit(gs, tmp_models):
    case = lc.CASES[lc.CASE_IDS.index("qwen3-all")]
    base = lc.base_file(gs, tmp_models, case)
    ad = lc.adapter_file(gs, tmp_models, case.cfg, case.adapters[0])
    prompt = np.random.default_rng(2).integers(0, gs.CONFIGS[case.cfg].n_vocab, 9)
    r0 = Qwen3Ref(base, 32, 8, 8)
    r1 = LoraRef(base, 32, 8, 8)
    r1.set_adapters([(Adapter(ad), 0.0)])
    a, b = r0.decode(prompt, np.arange(9)), r1.decode(prompt, np.arange(9))
    assert a.tobytes() == b.tobytes()
    for il in range(r0.n_layer):
        assert r0.layer_out(il, 9).tobytes() == r1.layer_out(il, 9).tobytes()


def test_reference_equals_a_base_with_merged_weights(gs, tmp_path):
    """An F32 adapter on an F32 `tiny` base against the same base with W + scale * B A (formed in float64, stored as f32) in place of W: the two forward
    passes differ by f32 round-off only (the delta is summed in another order and W' is rounded once), within TIGHT_TOL at every layer and at the logits."""
    base, merged, ad_path = str(tmp_path / "base.gguf"), str(tmp_path / "merged.gguf"), str(tmp_path / "ad.gguf")
    gs.write_synthetic_llama(base, "tiny", "f32", seed=21, with_vocab=False)
    gs.write_synthetic_lora(ad_path, "tiny", rank=6, alpha=9.0, targets=lc.ALL7 + ("output",), dtype="f32", seed=8, std=0.1)
    ad = Adapter(ad_path)
    user = 0.8
    shutil.copyfile(base, merged)
    _, t = read_gguf(base)
    blob = open(base, "rb").read()
    with open(merged, "r+b") as f:
        for name in ad.bases:
            ne, ty, raw = t[name]
            assert ty == F32
            (K, r), _, A = ad.t[name + ".lora_a"]
            (_, N), _, B = ad.t[name + ".lora_b"]
            W = raw.view("<f4").astype(np.float64).reshape(N, K)
            Wm = W + float(ad.scale(name, user)) * (B.view("<f4").astype(np.float64).reshape(N, r) @ A.view("<f4").astype(np.float64).reshape(r, K))
            off = blob.find(raw.tobytes()[:4096])                           # (the tensor's place in the file: random payloads do not repeat)
            assert off > 0 and blob[off:off + raw.size] == raw.tobytes()
            f.seek(off)
            f.write(Wm.astype("<f4").tobytes())
    prompt = np.random.default_rng(4).integers(0, gs.CONFIGS["tiny"].n_vocab, 12)
    oq.set_fa_v_acc_f32(1)
    try:
        r_lora = LoraRef(base, 32, 1, 1)
        r_lora.set_adapters([(ad, user)])
        r_merged = Qwen3Ref(merged, 32, 1, 1)
        r_base = Qwen3Ref(base, 32, 1, 1)
        a, b, c = r_lora.decode(prompt, np.arange(12))[0], r_merged.decode(prompt, np.arange(12))[0], r_base.decode(prompt, np.arange(12))[0]
    finally:
        oq.set_fa_v_acc_f32(0)
    errs = [lc.rel_err(r_lora.layer_out(il, 12), r_merged.layer_out(il, 12)) for il in range(r_lora.n_layer)] + [lc.rel_err(a, b)]
    print("merged-weights errors:", errs, "delta:", lc.rel_err(a, c))
    assert max(errs) <= TIGHT_TOL, errs
    assert lc.rel_err(a, c) >= 10 * lc.FLIP_TOL                                # (the adapter is not a no-op here)


@pytest.mark.parametrize("case", lc.CASES, ids=lc.CASE_IDS)
def test_delta_condition(gs, tmp_models, case):
    """What tests/test_gpu_lora.py compares the device with moves: base logits against adapted logits of the reference, at least 10 * FLIP_TOL apart."""
    base = lc.base_file(gs, tmp_models, case)
    ads = [lc.adapter_file(gs, tmp_models, case.cfg, ad) for ad in case.adapters]
    n = 21
    prompt = np.random.default_rng(5).integers(0, gs.CONFIGS[case.cfg].n_vocab, n)
    oq.set_fa_v_acc_f32(1 if case.kv == "f16" else 0)
    try:
        l0 = lc.reference(case, base, ads, 32, False).decode(prompt, np.arange(n))[0]
        l1 = lc.reference(case, base, ads, 32, True).decode(prompt, np.arange(n))[0]
    finally:
        oq.set_fa_v_acc_f32(0)
    assert lc.rel_err(l1, l0) >= 10 * lc.FLIP_TOL, lc.rel_err(l1, l0)


# ------------------------------------------------------------------------------------------------ refusals
Q, QN = "blk.0.attn_q.weight", "blk.0.attn_norm.weight"
PAIR = [(Q + ".lora_a", (256, 4), F16), (Q + ".lora_b", (4, 256), F16)]               # a good pair for `tiny` (n_embd 256, 4 heads of 64)
REFUSALS = [
    ("not-adapter", "tiny", dict(tensors=PAIR, gtype="model"), "not an adapter file: general.type is 'model' (a LoRA adapter says 'adapter')"),
    ("no-general-type", "tiny", dict(tensors=PAIR, gtype=None), "not an adapter file: general.type is '' (a LoRA adapter says 'adapter')"),
    ("adapter-type", "tiny", dict(tensors=PAIR, atype="ia3"), "unsupported adapter.type 'ia3' (this backend applies 'lora' adapters)"),
    ("encoder", "tiny-nomic", dict(tensors=PAIR, arch="nomic-bert"), "LoRA adapters are not supported on encoder models (nomic-bert)"),
    ("arch", "tiny", dict(tensors=PAIR, arch="qwen2"), "adapter architecture 'qwen2' does not match the model's 'llama'"),
    ("alpha-missing", "tiny", dict(tensors=PAIR, alpha=None), "adapter.lora.alpha is missing or not an f32"),
    ("alpha-int", "tiny", dict(tensors=PAIR, alpha=("u32", 8)), "adapter.lora.alpha is missing or not an f32"),
    ("suffix", "tiny", dict(tensors=PAIR + [(Q + ".lora_c", (256, 4), F16)]), f"adapter tensor {Q}.lora_c ends in neither .lora_a nor .lora_b"),
    ("no-b", "tiny", dict(tensors=PAIR[:1]), f"adapter tensor {Q}.lora_a has no {Q}.lora_b beside it"),
    ("no-a", "tiny", dict(tensors=PAIR[1:]), f"adapter tensor {Q}.lora_b has no {Q}.lora_a beside it"),
    ("token-embd", "tiny", dict(tensors=[("token_embd.weight.lora_a", (256, 4), F16), ("token_embd.weight.lora_b", (4, 512), F16)]),
     "adapter on token_embd.weight is not supported: the embedding lookup has no adapter form"),
    ("gate-inp", "tiny-moe", dict(tensors=[("blk.0.ffn_gate_inp.weight.lora_a", (256, 4), F16), ("blk.0.ffn_gate_inp.weight.lora_b", (4, 8), F16)]),
     "adapter on blk.0.ffn_gate_inp.weight is not supported: the router of a mixture-of-experts layer is not adapted"),
    ("exps", "tiny-moe", dict(tensors=[("blk.0.ffn_up_exps.weight.lora_a", (256, 4, 8), F16), ("blk.0.ffn_up_exps.weight.lora_b", (4, 512, 8), F16)]),
     "adapter on blk.0.ffn_up_exps.weight is not supported: expert tensors have no adapter form"),
    ("attn-qkv", "tiny", dict(tensors=[("blk.0.attn_qkv.weight.lora_a", (256, 4), F16), ("blk.0.attn_qkv.weight.lora_b", (4, 768), F16)]),
     "adapter on blk.0.attn_qkv.weight is not supported: the encoder's fused Q | K | V projection has no adapter form"),
    ("norm", "tiny", dict(tensors=[(QN + ".lora_a", (256, 4), F16), (QN + ".lora_b", (4, 1), F16)]), f"adapter on {QN} is not supported {TARGETS_MSG}"),
    ("other-name", "tiny", dict(tensors=[("rope_freqs.weight.lora_a", (32, 4), F16), ("rope_freqs.weight.lora_b", (4, 1), F16)]),
     f"adapter on rope_freqs.weight is not supported {TARGETS_MSG}"),
    ("no-such-layer", "tiny", dict(tensors=[("blk.7.attn_q.weight.lora_a", (256, 4), F16), ("blk.7.attn_q.weight.lora_b", (4, 256), F16)]),
     "adapter targets blk.7.attn_q.weight, which the model does not have"),
    ("dense-ffn-on-moe", "tiny-moe", dict(tensors=[("blk.0.ffn_gate.weight.lora_a", (256, 4), F16), ("blk.0.ffn_gate.weight.lora_b", (4, 512), F16)]),
     "adapter targets blk.0.ffn_gate.weight, which the model does not have"),
    ("type", "tiny", dict(tensors=[(Q + ".lora_a", (256, 32), Q8_0), (Q + ".lora_b", (32, 256), Q8_0)]), f"adapter tensor {Q}.lora_a has unsupported type q8_0 (f32 and f16 are)"),
    ("mixed", "tiny", dict(tensors=[(Q + ".lora_a", (256, 4), F16), (Q + ".lora_b", (4, 256), F32)]), f"adapter pair {Q}: lora_a is f16 and lora_b is f32 (both halves must have one type)"),
    ("shape-base", "tiny", dict(tensors=[(Q + ".lora_a", (128, 4), F16), (Q + ".lora_b", (4, 256), F16)]),
     f"adapter pair {Q}: lora_a is [128, 4] and lora_b is [4, 256] where the base tensor is [256, 256] (lora_a [K, r], lora_b [r, N])"),
    ("shape-rows", "tiny", dict(tensors=[("blk.1.attn_k.weight.lora_a", (256, 4), F16), ("blk.1.attn_k.weight.lora_b", (4, 256), F16)]),
     "adapter pair blk.1.attn_k.weight: lora_a is [256, 4] and lora_b is [4, 256] where the base tensor is [256, 128] (lora_a [K, r], lora_b [r, N])"),
    ("shape-halves", "tiny", dict(tensors=[(Q + ".lora_a", (256, 4), F16), (Q + ".lora_b", (8, 256), F16)]),
     f"adapter pair {Q}: lora_a is [256, 4] and lora_b is [8, 256] where the base tensor is [256, 256] (lora_a [K, r], lora_b [r, N])"),
    ("rank", "tiny", dict(tensors=[(Q + ".lora_a", (256, 513), F16), (Q + ".lora_b", (513, 256), F16)]), f"adapter pair {Q}: rank 513 is outside 1 .. 512"),
    ("empty", "tiny", dict(tensors=[]), "adapter file without tensors"),
]


@pytest.mark.parametrize("name,cfg,spec,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(gs, tmp_path, tmp_models, plan_exe, name, cfg, spec, text):
    ad = write_adapter(gs, str(tmp_path / "bad.gguf"), **spec)
    p = plan(plan_exe, base_model(gs, tmp_models, cfg, "f16" if cfg == "tiny-nomic" else "q4_k_m"), ad)
    assert p == {"status": -102, "err": text}


def test_refusal_on_a_rank_of_a_row_split(gs, tmp_path, tmp_models, plan_exe):
    ad = write_adapter(gs, str(tmp_path / "ok.gguf"), tensors=[(Q + ".lora_a", (1024, 4), F16), (Q + ".lora_b", (4, 1024), F16)])
    base = base_model(gs, tmp_models, "tiny-d128")
    assert plan(plan_exe, base, ad)["status"] == 0
    p = plan(plan_exe, base, ad, 1.0, 0, 2)
    assert p == {"status": -102, "err": "LoRA adapters are not supported on a model loaded as a rank of a row split (split_mode \"row\" / tp_size > 1): load it on one device"}


def test_tied_head_takes_an_output_pair(gs, tmp_path, tmp_models, plan_exe):
    """tiny-qwen3 has no output.weight: an output.weight pair is checked against the embedding table's shape; a token_embd pair stays refused (above)."""
    c = gs.CONFIGS["tiny-qwen3"]
    assert c.tied_output
    ad = write_adapter(gs, str(tmp_path / "o.gguf"), arch="qwen3", tensors=[("output.weight.lora_a", (c.n_embd, 4), F32), ("output.weight.lora_b", (4, c.n_vocab), F32)])
    p = plan(plan_exe, base_model(gs, tmp_models, "tiny-qwen3"), ad)
    assert p["status"] == 0 and [(q["base"], q["layer"], q["K"], q["N"]) for q in p["pairs"]] == [("output.weight", -1, c.n_embd, c.n_vocab)]
