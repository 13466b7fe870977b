"""The loader's host half on the CPU: `host_tests --plan FILE [tp_rank tp_size]` (tests/host/host_tests.cc) prints what host/model_plan.cc makes of a GGUF
file - hyper-parameters, every tensor's place in the weight arena and the source range its bytes come from, the totals - or the refusal.  Checked here
against the synthetic writer's own description of the file and a Python restatement of the layout rules: the arena, the row split's cuts, the column
halves of ffn_down, and every refusal's full text and status."""
import dataclasses
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_model import _patch_u32
from test_host_logic import SRCS

F32, F16, Q4_K, Q8_0, BF16, MXFP4 = 0, 1, 12, 8, 30, 39
_BUILT = []


@pytest.fixture(scope="session")
def plan_exe(tmp_path_factory):
    """The host test program, built with g++ as test_host_logic.py builds it (once per session, whichever module asks first)."""
    if not _BUILT:
        exe = str(tmp_path_factory.mktemp("plan") / "host_tests")
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread", *SRCS, "-o", exe], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        _BUILT.append(exe)
    return _BUILT[0]


def plan(exe, path, *tp, env=None):
    r = subprocess.run([exe, "--plan", path, *[str(x) for x in tp]], capture_output=True, text=True, timeout=60, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def cfg_of(gs, cfg):
    return gs.CONFIGS[cfg] if isinstance(cfg, str) else cfg


def model_file(gs, tmp_models, cfg, ftype):
    """A synthetic file, written once per session and never changed (the refusal cases patch copies)."""
    c = cfg_of(gs, cfg)
    path = str(tmp_models / f"plan-{c.name}-{ftype}.gguf")
    if not os.path.exists(path):
        gs.write_synthetic_llama(path, c, ftype, seed=3, with_vocab=False)
    return path


def align256(n):
    return (n + 255) & ~255


def dev_row_bytes(gs, t, K):
    """csrc/ggml_types.h dev_row_bytes: the on-disk row, padded to 16 bytes."""
    return (gs.row_bytes(t, K) + 15) & ~15


def asked_order(cfg):
    """The order in which the loader asks for a file's tensors (= arena order), restated."""
    if cfg.arch == "nomic-bert":
        names = ["token_embd.weight", "token_types.weight", "token_embd_norm.weight", "token_embd_norm.bias"]
        for il in range(cfg.n_layer):
            names += [f"blk.{il}.{n}" for n in ("attn_qkv.weight", "attn_output.weight", "attn_output_norm.weight", "attn_output_norm.bias", "ffn_gate.weight", "ffn_up.weight",
                                               "ffn_down.weight", "layer_output_norm.weight", "layer_output_norm.bias")]
        return names
    names = ["token_embd.weight", "output_norm.weight"] + ([] if cfg.tied_output else ["output.weight"])
    for il in range(cfg.n_layer):
        layer = ["attn_norm.weight", "attn_q.weight", "attn_k.weight", "attn_v.weight", "attn_output.weight"]
        layer += ["attn_q.bias", "attn_k.bias", "attn_v.bias"] if cfg.qkv_bias else []
        layer += ["attn_q_norm.weight", "attn_k_norm.weight"] if cfg.arch in ("qwen3", "qwen3moe") else []
        layer += ["ffn_norm.weight"]
        layer += ["ffn_gate_inp.weight", "ffn_gate_exps.weight", "ffn_up_exps.weight", "ffn_down_exps.weight"] if cfg.n_expert else ["ffn_gate.weight", "ffn_up.weight", "ffn_down.weight"]
        names += [f"blk.{il}.{n}" for n in layer]
    return names


def loader_bytes_per_token(gs, c, ftype):
    """What the loader reports for a file: gguf_synth.weight_bytes_per_token, stated with the two places where the loader counts more than the helper.
    The loader counts the embedding row looked up and, when the file has no output.weight, the whole table as the output head - for an encoder file too,
    which has no head.  The helper counts the table alone for a tied file and the row alone otherwise."""
    tensors = {name: (ne, t) for name, ne, t, _ in gs.model_tensors(c, ftype)}
    ne, t = tensors["token_embd.weight"]
    row, table = gs.row_bytes(t, ne[0]), gs.row_bytes(t, ne[0]) * ne[1]
    more = 0 if "output.weight" in tensors else row if c.tied_output else table
    return gs.weight_bytes_per_token(c, ftype) + more


LAYOUT_CASES = [(c, f) for c in ("tiny", "tiny-gqa4", "tiny-qwen2", "tiny-qwen3", "tiny-w320", "tiny-w896-2l", "tiny-w896-2l-untied") for f in ("q4_k_m", "q8_0", "q4_1", "iq4_xs")]
LAYOUT_CASES += [("tiny", "bf16"), ("tiny-moe", "q4_k_m"), ("tiny-moe", "mxfp4_moe"), ("tiny-qwen3moe", "q4_k_m"), ("tiny-qwen3moe", "mxfp4_moe"), ("tiny-nomic", "f16")]


@pytest.mark.parametrize("cfg,ftype", LAYOUT_CASES)
def test_layout(pkg, plan_exe, tmp_models, cfg, ftype):
    gs = pkg.gguf_synth
    c = gs.CONFIGS[cfg]
    p = plan(plan_exe, model_file(gs, tmp_models, cfg, ftype))
    assert "err" not in p, p
    hp = p["hp"]
    n_ff = (c.n_ff_exp or c.n_ff) if c.n_expert else c.n_ff
    want_hp = dict(arch=c.arch, n_embd=c.n_embd, n_layer=c.n_layer, n_ff=n_ff, n_head=c.n_head, n_head_kv=c.n_head_kv, n_rot=c.head_dim, n_vocab=c.n_vocab, n_expert=c.n_expert,
                   n_expert_used=c.n_expert_used, head_dim=c.head_dim, n_ctx_train=c.n_ctx_train, pooling_type=1 if c.arch == "nomic-bert" else 0, rope_neox=int(c.arch != "llama"),
                   encoder=int(c.arch == "nomic-bert"), qk_norm=int(c.arch in ("qwen3", "qwen3moe")), tp_rank=0, tp_size=1, n_head_full=c.n_head, n_head_kv_full=c.n_head_kv,
                   n_ff_full=n_ff, n_vocab_local=c.n_vocab, eps=float(np.float32(c.eps)), rope_base=float(np.float32(c.rope_base)), rope_scale=1.0, yarn_ext=0.0, yarn_attn=1.0)
    assert {k: hp[k] for k in want_hp} == want_hp

    file_tensors = {name: (ne, t) for name, ne, t, _ in gs.model_tensors(c, ftype)}
    names = [t["name"] for t in p["tensors"]]
    assert names == asked_order(c)
    assert ("output.weight" in names) == (not c.tied_output and c.arch != "nomic-bert")
    off = on_disk = stage = 0
    for t in p["tensors"]:
        ne, ty = file_tensors[t["name"]]
        K, N, X = ne[0], (ne[1] if len(ne) > 1 else 1), (ne[2] if len(ne) > 2 else 1)
        assert (t["type"], t["K"], t["N"], t["n_expert"], t["n_dims"]) == (ty, K, N, X, len(ne))
        ggml_row = gs.row_bytes(ty, K)
        row = ggml_row if len(ne) == 1 else dev_row_bytes(gs, ty, K)
        assert t["row_bytes"] == row and t["bytes"] == row * (1 if len(ne) == 1 else N * X)
        # arena: 256-aligned, ascending in the order asked for, nothing between or over one another
        assert t["offset"] == off and off % 256 == 0
        off += align256(t["bytes"])
        # the whole file tensor, one contiguous range
        disk = ggml_row * N * X
        assert (t["src_off"], t["src_pitch"], t["src_width"], t["src_rows"], t["src_bytes"], t["file_bytes"]) == (0, ggml_row, ggml_row, 1 if len(ne) == 1 else N * X, disk, disk)
        assert t["extra_copy"] is False
        on_disk += disk
        if ty not in (F32, F16, BF16, Q4_K, 13) or row != ggml_row:      # repacked on the way (every quantised type but Q4_K / Q5_K) or padded: staged
            stage = max(stage, disk)
    assert p["total"] == off
    assert p["max_stage"] == stage
    assert p["file_tensor_bytes"] == on_disk
    assert p["bytes_per_token"] == loader_bytes_per_token(gs, c, ftype)


# ---------------------------------------------------------------------------------------------------------------- row split
@pytest.mark.parametrize("cfg,P", [("tiny-d128", 2), ("tiny-8b-attn-2l", 8)])
def test_row_split_covers_every_tensor_once(pkg, plan_exe, tmp_models, cfg, P):
    gs = pkg.gguf_synth
    c = gs.CONFIGS[cfg]
    path = model_file(gs, tmp_models, cfg, "q4_k_m")
    ranks = [plan(plan_exe, path, r, P) for r in range(P)]
    for r, p in enumerate(ranks):
        assert "err" not in p, p
        hp = p["hp"]
        assert (hp["tp_rank"], hp["tp_size"]) == (r, P)
        assert (hp["n_head"], hp["n_head_kv"], hp["n_ff"]) == (c.n_head // P, c.n_head_kv // P, c.n_ff // P)
        assert (hp["n_head_full"], hp["n_head_kv_full"], hp["n_ff_full"], hp["n_vocab_local"]) == (c.n_head, c.n_head_kv, c.n_ff, c.n_vocab // P)
        assert [t["name"] for t in p["tensors"]] == asked_order(c)
    split = set()
    for i, t0 in enumerate(ranks[0]["tensors"]):
        per_rank = [p["tensors"][i] for p in ranks]
        if t0["src_bytes"] == t0["file_bytes"]:
            assert all(t == t0 for t in per_rank), t0["name"]        # unsplit: the same entry on every rank
            continue
        split.add(t0["name"].split(".")[-2] if t0["name"].startswith("blk.") else t0["name"])
        # every rank's source bytes: src_rows pieces of src_width bytes, src_pitch apart, from src_off
        starts = np.concatenate([t["src_off"] + np.arange(t["src_rows"], dtype=np.int64) * t["src_pitch"] for t in per_rank])
        widths = np.concatenate([np.full(t["src_rows"], t["src_width"], np.int64) for t in per_rank])
        order = np.argsort(starts, kind="stable")
        starts, ends = starts[order], (starts + widths)[order]
        assert starts[0] == 0 and ends[-1] == t0["file_bytes"], t0["name"]
        assert np.array_equal(starts[1:], ends[:-1]), t0["name"]     # pairwise disjoint, and their union is the whole tensor
        for t in per_rank:
            assert t["src_bytes"] == t["src_width"] * t["src_rows"] == t0["file_bytes"] // P
            assert t["bytes"] == t["row_bytes"] * t["N"] and t["K"] * t["N"] * P == t0["file_bytes"] // gs.BLOCK_BYTES[t["type"]] * gs.BLOCK_ELEMS[t["type"]]
    assert split == {"output.weight", "attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down"}


# ---------------------------------------------------------------------------------------------------------------- column halves of ffn_down
def test_ffn_down_column_halves(pkg, plan_exe, tmp_models):
    gs = pkg.gguf_synth
    c = gs.CONFIGS["tiny-ff28k"]
    path = model_file(gs, tmp_models, "tiny-ff28k", "q4_k_m")
    p = plan(plan_exe, path)
    by_name = {t["name"]: t for t in p["tensors"]}
    for il in range(c.n_layer):
        down = by_name[f"blk.{il}.ffn_down.weight"]
        lo, hi = by_name[f"blk.{il}.ffn_down.weight[cols 0/2]"], by_name[f"blk.{il}.ffn_down.weight[cols 1/2]"]
        half = gs.row_bytes(down["type"], c.n_ff // 2)
        for part, t in enumerate((lo, hi)):
            assert t["extra_copy"] is True and t["file_name"] == down["name"] and t["type"] == down["type"]
            assert (t["K"], t["N"]) == (c.n_ff // 2, c.n_embd)
            assert (t["src_off"], t["src_width"], t["src_pitch"], t["src_rows"], t["src_bytes"]) == (part * half, half, 2 * half, c.n_embd, half * c.n_embd)
        assert down["extra_copy"] is False and down["src_bytes"] == 2 * half * c.n_embd
    # a second copy: not file bytes, not bytes a token reads
    assert p["bytes_per_token"] == loader_bytes_per_token(gs, c, "q4_k_m")
    assert p["file_tensor_bytes"] == sum(t["src_bytes"] for t in p["tensors"] if "[cols" not in t["name"])
    assert p["total"] == sum(align256(t["bytes"]) for t in p["tensors"])
    off = plan(plan_exe, path, env={"MI355_DOWN_HALVES": "0"})
    assert [t["name"] for t in off["tensors"]] == asked_order(c)
    assert (off["bytes_per_token"], off["file_tensor_bytes"]) == (p["bytes_per_token"], p["file_tensor_bytes"])
    q8 = plan(plan_exe, model_file(gs, tmp_models, "tiny-ff28k", "q8_0"))
    assert [t["name"] for t in q8["tensors"]] == asked_order(c)


# ---------------------------------------------------------------------------------------------------------------- refusals
def _patch_bytes(path, old, new):
    """Replace the one occurrence of a byte string by another of the same length (a key or a tensor renamed in place)."""
    old, new = old.encode(), new.encode()
    blob = open(path, "rb").read()
    assert len(old) == len(new) and blob.count(old) == 1, old
    open(path, "wb").write(blob.replace(old, new))


def _patch_tensor_type(path, name, t):
    """Overwrite the type of a tensor's info record (name, n_dims u32, ne u64 each, type u32, offset u64); the data stays where and what it is."""
    blob = bytearray(open(path, "rb").read())
    k = name.encode()
    at = blob.find(struct.pack("<Q", len(k)) + k)
    assert at >= 0, name
    at += 8 + len(k)
    n_dims = struct.unpack_from("<I", blob, at)[0]
    struct.pack_into("<I", blob, at + 4 + 8 * n_dims, t)
    open(path, "wb").write(bytes(blob))


class Maker:
    """What a refusal case builds its file with."""

    def __init__(self, gs, tmp_models, tmp_path, monkeypatch):
        self.gs, self.tmp_models, self.tmp_path, self.monkeypatch = gs, tmp_models, tmp_path, monkeypatch

    def copy(self, cfg, ftype="q4_k_m"):
        path = str(self.tmp_path / "case.gguf")
        shutil.copy(model_file(self.gs, self.tmp_models, cfg, ftype), path)
        return path

    def u32(self, cfg, ftype="q4_k_m", **kv):
        path = self.copy(cfg, ftype)
        for key, value in kv.items():
            _patch_u32(path, cfg_of(self.gs, cfg).arch + "." + key.replace("__", "."), value)
        return path

    def rename_in(self, path, old, new):
        _patch_bytes(path, old, new)
        return path

    def renamed(self, cfg, old, new, ftype="q4_k_m"):
        return self.rename_in(self.copy(cfg, ftype), old, new)

    def retyped(self, cfg, name, t, ftype="q4_k_m"):
        path = self.copy(cfg, ftype)
        _patch_tensor_type(path, name, t)
        return path

    def variant(self, cfg, ftype="q4_k_m", tensors=None, **changes):
        """A config of its own (dataclasses.replace) and / or an edited tensor list (tensors: list -> list)."""
        c = dataclasses.replace(self.gs.CONFIGS[cfg], name="variant", **changes)
        if tensors:
            orig = self.gs.model_tensors
            self.monkeypatch.setattr(self.gs, "model_tensors", lambda cfg_, ftype_: tensors(orig(cfg_, ftype_)))
        path = str(self.tmp_path / "variant.gguf")
        self.gs.write_synthetic_llama(path, c, ftype, seed=3, with_vocab=False)
        return path


ROW = 'row split (split_mode "row" / tp_size > 1)'
W256 = " need widths that are multiples of 256 (embedding_length "
# (id, file, tp arguments, the refusal's full text) - one case per err text of host/model_plan.cc; every one of them is status -102.  Where a file has
# several faults the case pins which one is reported (see the cases marked "order").
REFUSALS = [
    ("arch-missing", lambda m: m.renamed("tiny", "general.architecture", "general.architecturX"), (), "general.architecture missing"),
    ("arch-unsupported", lambda m: m.variant("tiny", arch="gemma"), (),
     "unsupported general.architecture 'gemma' (this backend builds the llama graph - llama, qwen2, qwen3, qwen3moe - and the nomic-bert encoder)"),
    ("qwen3moe-no-experts", lambda m: m.u32("tiny-qwen3moe", expert_count=0), (),
     "qwen3moe file without experts (expert_count missing or 0): dense feed-forward layers under the qwen3moe name are not supported"),
    ("qwen3moe-dense-tensors", lambda m: m.variant("tiny-qwen3moe", tensors=lambda ts: ts + [("blk.0.ffn_gate.weight", (512, 256), F16, 512)]), (),
     "qwen3moe file with dense ffn_gate / ffn_up / ffn_down tensors: not supported (a qwen3moe layer is routed: ffn_gate_inp and *_exps)"),
    ("hparams-missing", lambda m: m.u32("tiny", embedding_length=0), (), "missing hyper-parameters for arch llama"),
    ("hparams-implausible", lambda m: m.u32("tiny", block_count=2000), (), "implausible hyper-parameters for arch llama"),
    ("head-count-kv", lambda m: m.u32("tiny", attention__head_count_kv=3), (), "attention.head_count_kv (3) must be positive and divide attention.head_count (4)"),
    ("head-ratio", lambda m: m.u32("tiny", attention__head_count=16, attention__head_count_kv=1), (), "unsupported query / kv head ratio 16 (the attention kernels are built for 1 .. 8)"),
    ("embd-head-count", lambda m: m.u32("tiny", attention__head_count=3, attention__head_count_kv=3), (), "embedding_length is not a multiple of attention.head_count"),
    ("expert-counts", lambda m: m.u32("tiny-moe", expert_used_count=9), (), "bad expert_count / expert_used_count"),
    ("qwen3-no-key-length", lambda m: m.renamed("tiny-qwen3", "qwen3.attention.key_length", "qwen3.attention.key_lengtX"), (), "qwen3 file without attention.key_length"),
    ("qwen3-value-length", lambda m: m.u32("tiny-qwen3", attention__value_length=64), (), "attention.value_length (64) differs from attention.key_length (128): not supported"),
    ("qwen3-key-length-implausible", lambda m: m.u32("tiny-qwen3", attention__key_length=8192, attention__value_length=8192), (), "implausible attention.key_length"),
    ("yarn-factor", lambda m: m.variant("tiny", extra={"rope.scaling.type": "yarn", "rope.scaling.factor": 0.0}), (), "rope.scaling.factor must be positive"),
    ("rope-scaling-type", lambda m: m.variant("tiny", extra={"rope.scaling.type": "longrope"}), (), "unsupported rope.scaling.type longrope"),
    ("head-dim", lambda m: m.u32("tiny", attention__head_count=8), (), "unsupported head_dim 32"),
    ("embd-32", lambda m: m.u32("tiny-qwen3", embedding_length=500), (), "embedding_length (500) must be a multiple of 32"),
    ("split-qwen3", lambda m: m.copy("tiny-qwen3"), (0, 2), ROW + " of qwen3 files is not supported: load it on one device"),
    ("split-no-group", lambda m: m.copy("tiny-d128"), (0, 2, "no-group"), "tp_size > 1 needs the process's row-split group first (mi355_tp_init with the same rank / size)"),
    ("split-rank-range", lambda m: m.copy("tiny-d128"), (5, 2), "tp_rank out of range"),
    ("split-moe", lambda m: m.copy("tiny-moe"), (0, 2), "row split of mixture-of-experts files is not supported"),
    ("split-head-counts", lambda m: m.copy("tiny"), (0, 4), "tp_size must divide the head counts (4 / 2)"),
    ("split-rank-width", lambda m: m.copy("tiny"), (0, 2), "a rank's attention width must be a multiple of 256"),
    ("type-unsupported", lambda m: m.retyped("tiny", "blk.0.attn_q.weight", 16), (), "tensor blk.0.attn_q.weight has unsupported type unknown"),
    ("mxfp4-vector", lambda m: m.retyped("tiny", "blk.0.attn_norm.weight", MXFP4), (), "tensor blk.0.attn_norm.weight has type mxfp4: norm and bias vectors must be f32"),
    ("mxfp4-encoder", lambda m: m.retyped("tiny-nomic", "blk.0.attn_qkv.weight", MXFP4, "f16"), (), "tensor blk.0.attn_qkv.weight has type mxfp4: the encoder graph is not supported with mxfp4 tensors"),
    ("mxfp4-split", lambda m: m.copy("tiny-d128", "mxfp4"), (0, 2),
     "tensor token_embd.weight has type mxfp4: a " + ROW + " of mxfp4 tensors is not supported: load the file on one device"),
    ("q4_1-split", lambda m: m.copy("tiny-d128", "q4_1"), (0, 2), ROW + " of q4_1 tensors is not supported (tensor token_embd.weight): load the file on one device"),
    ("bf16-vector", lambda m: m.retyped("tiny", "blk.0.attn_norm.weight", BF16), (), "tensor blk.0.attn_norm.weight has type bf16: norm and bias vectors must be f32"),
    # order: all three expert tensors of layer 0 are refused, and the layer's last refusal is the one reported
    ("bf16-experts", lambda m: m.copy("tiny-moe", "bf16"), (), "tensor blk.0.ffn_down_exps.weight has type bf16: bf16 expert tensors are not supported"),
    ("bf16-encoder", lambda m: m.copy("tiny-nomic", "bf16"), (), "tensor token_embd.weight has type bf16: the encoder graph has no bf16 kernels"),
    ("bf16-split", lambda m: m.copy("tiny-d128", "bf16"), (0, 2), "tensor output.weight has type bf16: a " + ROW + " of bf16 tensors is not supported: load the file on one device"),
    ("bf16-row-8", lambda m: m.variant("tiny", "bf16", n_ff=500), (), "tensor blk.0.ffn_down.weight has type bf16: bf16 rows must hold a multiple of 8 weights"),
    # order: token_embd and output are both refused before the layers are looked at; the later one is reported
    ("bf16-embd-256", lambda m: m.copy("tiny-w320", "bf16"), (), "tensor output.weight has type bf16: bf16 tensors in a file whose embedding_length is not a multiple of 256 are not supported"),
    ("row-not-blocks", lambda m: m.retyped("tiny-w320", "token_embd.weight", Q4_K, "q8_0"), (), "tensor token_embd.weight (q4_K): its row length 320 is not a whole number of 256-element blocks"),
    ("tensor-missing", lambda m: m.renamed("tiny", "blk.1.attn_q.weight", "blk.1.attn_X.weight"), (), "missing tensor blk.1.attn_q.weight"),
    # order: two faults - a missing tensor in layer 0 and hyper-parameters that contradict the tensors; the tensors are looked for first
    ("order-missing-before-shapes", lambda m: m.rename_in(m.u32("tiny", feed_forward_length=768), "blk.0.ffn_up.weight", "blk.0.ffn_Xp.weight"), (), "missing tensor blk.0.ffn_up.weight"),
    ("cut-columns", lambda m: m.variant("tiny-d128", n_ff=768), (0, 2), "tensor blk.0.ffn_down.weight: row length 768 cannot be cut 2 ways on block boundaries"),
    ("cut-rows", lambda m: m.variant("tiny-d128", tensors=lambda ts: [(n, (ne[0], 2047) if n == "blk.0.ffn_up.weight" else ne, t, f) for n, ne, t, f in ts]), (0, 2),
     "tensor blk.0.ffn_up.weight: 2047 rows cannot be cut 2 ways"),
    ("split-encoder", lambda m: m.variant("tiny-nomic", "f16", n_embd=512, n_head=8, n_head_kv=8), (0, 2), "row split of encoder files is not supported"),
    ("moe-encoder", lambda m: m.variant("tiny-nomic", "f16", extra={"expert_count": 4, "expert_used_count": 2}), (), "mixture-of-experts encoder files are not supported"),
    ("shape", lambda m: m.u32("tiny", attention__head_count=2), (), "tensor blk.0.attn_k.weight has shape [256, 128, 1], expected [256, 256, 1]"),
    ("shape-vector", lambda m: m.variant("tiny-qwen2", tensors=lambda ts: [(n, (256,) if n == "blk.0.attn_k.bias" else ne, t, f) for n, ne, t, f in ts]), (),
     "tensor blk.0.attn_k.bias has shape [256, 1, 1], expected [128]"),
    ("token-embd-width", lambda m: m.u32("tiny", embedding_length=512), (), "token_embd.weight does not have embedding_length columns"),
    ("token-types", lambda m: m.retyped("tiny-nomic", "token_types.weight", F16, "f16"), (), "token_types.weight must hold f32 rows of embedding_length"),
    ("encoder-rot", lambda m: m.u32("tiny-nomic", "f16", rope__dimension_count=32), (), "encoder files rotate whole heads (rope.dimension_count must equal the head size)"),
    ("encoder-ff", lambda m: m.u32("tiny-nomic", "f16", feed_forward_length=768), (), "feed-forward tensors do not match feed_forward_length"),
    ("encoder-norm-f32", lambda m: m.retyped("tiny-nomic", "blk.1.layer_output_norm.bias", F16, "f16"), (), "tensor blk.1.layer_output_norm.bias must be f32"),
    ("encoder-embd-norm-f32", lambda m: m.retyped("tiny-nomic", "token_embd_norm.weight", F16, "f16"), (), "token_embd_norm must be f32"),
    ("rope-freqs", lambda m: m.variant("tiny", tensors=lambda ts: ts + [("rope_freqs.weight", (16,), F32, None)]), (), "rope_freqs.weight must hold rope.dimension_count / 2 f32 factors"),
    ("rot-odd", lambda m: m.u32("tiny", rope__dimension_count=63), (), "bad rope.dimension_count"),
    ("qwen3-rot", lambda m: m.u32("tiny-qwen3", rope__dimension_count=64), (), "qwen3 files must rotate whole heads (rope.dimension_count must equal attention.key_length)"),
    ("qwen3-experts", lambda m: m.variant("tiny-qwen3", n_expert=4, n_expert_used=2), (), "qwen3 files with experts are not supported"),
    ("ff-length", lambda m: m.u32("tiny", feed_forward_length=768), (), "feed-forward tensors do not match feed_forward_length"),
    ("ff-length-qwen3moe", lambda m: m.u32("tiny-qwen3moe", expert_feed_forward_length=512), (), "feed-forward tensors do not match expert_feed_forward_length"),
    ("norm-f32", lambda m: m.retyped("tiny", "blk.1.ffn_norm.weight", F16), (), "tensor blk.1.ffn_norm.weight must be f32"),
    ("output-norm-f32", lambda m: m.retyped("tiny", "output_norm.weight", F16), (), "output_norm.weight must be f32"),
    ("widths-moe", lambda m: m.variant("tiny-moe", "q8_0", n_ff=288), (),
     "mixture-of-experts files (the expert gather and the expert mat-vecs work on whole 256-blocks)" + W256 + "256, attention width 256, feed-forward width 288)"),
    ("widths-encoder", lambda m: m.variant("tiny-nomic", "f16", n_ff=288), (), "encoder files" + W256 + "256, attention width 256, feed-forward width 288)"),
    ("widths-split", lambda m: m.variant("tiny-d128", "f16", n_ff=2080), (0, 2), "a " + ROW + W256 + "1024, attention width 1024, feed-forward width 2080)"),
]
# Every err text of host/model_plan.cc has a case above (the encoder's and the decoder's "feed-forward tensors do not match feed_forward_length" are one text: both have one).


@pytest.mark.parametrize("make,tp,err", [pytest.param(*c[1:], id=c[0]) for c in REFUSALS])
def test_refusal(pkg, plan_exe, tmp_models, tmp_path, monkeypatch, make, tp, err):
    m = Maker(pkg.gguf_synth, tmp_models, tmp_path, monkeypatch)
    p = plan(plan_exe, make(m), *tp)
    assert p == {"status": -102, "err": err}
