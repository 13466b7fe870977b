"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, exports every
symbol include/mi355_llama.h declares, and refuses to compute without a GPU (no CPU fallback)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "mi355_llama.h")).read()
    return sorted(set(re.findall(r"MI355_API[^;(]*?\b(mi355_\w+)\s*\(", src)))


def test_header_declares_what_binding_binds(pkg):
    decl = declared_symbols()
    assert len(decl) > 40
    assert sorted(pkg.binding.SYMBOLS) == decl


def test_library_builds_loads_and_exports_every_symbol(pkg):
    import __graft_entry__ as ge
    ge.build()
    lib = pkg.load_library()
    for name in declared_symbols():
        assert hasattr(lib, name), name


def test_no_cpu_fallback(pkg):
    lib = pkg.load_library()
    if lib.mi355_device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(pkg.MI355Error):
        pkg.Backend()
    assert lib.mi355_backend_init() == -100
    with pytest.raises(pkg.MI355Error):
        pkg.Model("/nonexistent.gguf")
    import numpy as np
    x = np.zeros(256, np.float32)
    out = np.zeros(292, np.uint8)
    rc = lib.mi355_op_quantize_act(15, x.ctypes.data, 256, 1, out.ctypes.data)
    assert rc == -100
    # the K / V cache write and the K-shift test entries: one cell of one 32-element f16 head
    q = np.zeros(32, np.float32)
    cache = np.zeros(64, np.uint8)
    zero = np.zeros(1, np.int32)
    for form in range(4):
        rc = lib.mi355_op_kv_store(form, q.ctypes.data, q.ctypes.data, q.ctypes.data, 1, 1, 1, 32, 32, 0, 1, 1, 1, zero.ctypes.data, zero.ctypes.data,
                                   1e4, 1.0, None, None, None, 0.0, cache.ctypes.data, cache.ctypes.data)
        assert rc == -100, form
    rc = lib.mi355_op_k_shift(1, 1, 32, 32, 0, 1, zero.ctypes.data, 1e4, 1.0, None, 0.0, 1.0, 0.0, 0.0, cache.ctypes.data)
    assert rc == -100
    # the test entries of the index kernels: one row of 256, one selection, one expert
    one = np.ones(1, np.int32)
    f = np.zeros(192, np.float32)
    adj = np.zeros(192, np.int32)
    key = np.zeros(1, np.uint64)
    b = np.zeros(2 * 256, np.uint8)
    assert lib.mi355_op_argmax_rows(x.ctypes.data, 256, one.ctypes.data, 1, 1, zero.ctypes.data) == -100
    assert lib.mi355_op_topk_rows(x.ctypes.data, 256, 1, zero.ctypes.data, 1, 1, zero.ctypes.data, adj.ctypes.data, f.ctypes.data, adj.ctypes.data,
                                  f.ctypes.data, f.ctypes.data, f.ctypes.data, key.ctypes.data) == -100
    assert lib.mi355_op_moe_group(zero.ctypes.data, 1, 1, 1, adj.ctypes.data, adj.ctypes.data, adj.ctypes.data) == -100
    assert lib.mi355_op_moe_gather_act(None, None, None, b.ctypes.data, b.ctypes.data, 1, 256, zero.ctypes.data, 1, None, None, None, b.ctypes.data,
                                       b.ctypes.data) == -100
    y = np.zeros(256, np.float32)
    for grouped in (0, 1):
        assert lib.mi355_op_moe_combine(x.ctypes.data, x.ctypes.data, x.ctypes.data, 1, 256, 1, grouped, zero.ctypes.data, y.ctypes.data) == -100
    assert lib.mi355_op_gather_rows_f32(x.ctypes.data, 1, 256, zero.ctypes.data, 1, y.ctypes.data) == -100
    # the grouped-expert launch, every form: one expert of 128 Q4_K / MXFP4 rows of 256, one grouped row
    wq = np.zeros(128 * 144, np.uint8)
    yg = np.zeros(3 * 128, np.float32)
    for form, t in ((0, 12), (1, 12), (2, 39), (3, 39)):
        assert lib.mi355_op_moe_mul_mat_grouped(t, form, wq.ctypes.data, wq.ctypes.data, 1, 128, 256, x.ctypes.data, one.ctypes.data, 1, 128, 2, yg.ctypes.data,
                                                yg.ctypes.data) == -100, form
        assert lib.mi355_op_moe_mul_mat_grouped(t, form, None, None, 1, 128, 256, None, None, 1, 128, 2, None, None) == -100, form
    # the decode step's mat-vec launch: one Q8_0 row of 256 (8 blocks of 34 bytes)
    import ctypes as C
    w = np.zeros(8 * 34, np.uint8)
    t8 = np.full(1, 8, np.int32)
    n1 = np.ones(1, np.int64)
    path = np.zeros(40, np.int32)
    wp, yp = (C.c_void_p * 1)(w.ctypes.data), (C.c_void_p * 1)(y.ctypes.data)
    assert lib.mi355_op_mat_vec_step(1, t8.ctypes.data, wp, n1.ctypes.data, 256, x.ctypes.data, 1, 0, None, 0, None, 0.0, 0, 0, 1, None, 0, yp, None,
                                     path.ctypes.data) == -100
    # the prompt batch's mat-mul launch: one Q4_K row of 256 (a block of 144 bytes) over three tokens; the producers of its activation; the batched
    # attention step with the merge's block-sum planes
    t12 = np.full(1, 12, np.int32)
    x3 = np.zeros(3 * 256, np.float32)
    y3 = np.zeros(3, np.float32)
    wp, yp = (C.c_void_p * 1)(wq.ctypes.data), (C.c_void_p * 1)(y3.ctypes.data)
    for form in range(4):
        assert lib.mi355_op_prompt_mul_mat(1, t12.ctypes.data, wp, n1.ctypes.data, 256, x3.ctypes.data, 3, 0, None, 0, 0, None, 0.0, form, 0, yp, path.ctypes.data) == -100
    planes = np.zeros(16, np.int8)
    for producer in range(3):
        assert lib.mi355_op_act_q8k_planes(producer, x.ctypes.data, x.ctypes.data, x.ctypes.data, 1e-5, 256, 1, out.ctypes.data, planes.ctypes.data,
                                           planes.ctypes.data, planes.ctypes.data, planes.ctypes.data, None) == -100
    assert lib.mi355_op_attn_batch_step_planes(None, None, None, 1, 8, 1, 32, 1, None, 1, None, 1, 1, None, None, None, None, None, 1e4, 32, 0, 1.0, 0, None, None,
                                               None, None) == -100
    # the image encoder's launches: one 32-wide head over four rows; 32 f16 rows of 16 over eight tokens; a 2 x 2 patch grid
    h16 = np.zeros(256, np.uint16)
    assert lib.mi355_op_clip_attn(x.ctypes.data, x.ctypes.data, x.ctypes.data, 4, 1, 32, 1, y.ctypes.data, h16.ctypes.data, path.ctypes.data) == -100
    w16 = np.zeros(32 * 16, np.uint16)
    for form in (0, 1):
        assert lib.mi355_op_mul_mat_f16_xh(w16.ctypes.data, 32, 16, x.ctypes.data, 8, 32, None, 1.0, 0, None, 0, form, y.ctypes.data) == -100, form
    assert lib.mi355_op_mul_mat_f16_xh(w16.ctypes.data, 16, 24, x.ctypes.data, 8, 16, None, 1.0, 0, None, 0, 0, y.ctypes.data) == -100
    assert lib.mi355_op_layer_norm(x.ctypes.data, x.ctypes.data, x.ctypes.data, 16, 4, 1e-5, 0, y.ctypes.data, h16.ctypes.data) == -100
    assert lib.mi355_op_clip_gelu(x.ctypes.data, 256, 0, y.ctypes.data, h16.ctypes.data) == -100
    assert lib.mi355_op_clip_im2col(x.ctypes.data, 4, 2, 16, y.ctypes.data) == -100
    assert lib.mi355_op_clip_embed(x.ctypes.data, x.ctypes.data, x.ctypes.data, 16, 4, y.ctypes.data) == -100
    assert lib.mi355_op_clip_bias(y.ctypes.data, x.ctypes.data, 16, 4, 1.0, 0) == -100
    assert lib.mi355_op_f32_to_f16(x.ctypes.data, 256, h16.ctypes.data) == -100
    assert lib.mi355_op_add_qkv_bias(y.ctypes.data, None, None, x.ctypes.data, None, None, 16, 0, 4) == -100


def test_every_op_entry_checks_the_device_first(pkg):
    """Every per-op test entry answers MI355_ERR_NO_DEVICE before it looks at an argument: each mi355_op_* symbol is called with zeros and null pointers made
    from its declared argtypes, which is safe only because the device check comes first - and this test keeps it first."""
    lib = pkg.load_library()
    if lib.mi355_device_count() > 0:
        pytest.skip("GPU present")
    names = sorted(n for n in pkg.binding.SYMBOLS if n.startswith("mi355_op_"))
    assert len(names) > 50
    for name in names:
        restype, argtypes = pkg.binding.SYMBOLS[name]
        assert restype is not None, name
        rc = getattr(lib, name)(*[t() for t in argtypes])
        assert rc == -100, name
        assert lib.mi355_last_error(), name


def test_product_does_not_touch_oracle():
    """The product path (package + C-ABI sources) must never import / link / call the oracle."""
    pkg_dir = os.path.join(ROOT, "cortex.llamacpp_amd")
    for base, _, files in os.walk(pkg_dir):
        if os.sep + "build" in base or os.sep + "lib" in base:
            continue
        for f in files:
            if f.endswith((".py", ".cc", ".h", ".hip")):
                txt = open(os.path.join(base, f), errors="replace").read()
                assert "oracle" not in txt.lower() or f == "build.py", os.path.join(base, f)


def test_fused_attention_block_plan_by_geometry(pkg):
    """Round 6 host logic (no GPU): which layers run their Q | K | V inside the attention + attn_output launch (csrc/attn_out.hip QF).  The plan is a
    question of LDS: the workgroup's rows of attn_q | attn_k | attn_v and of attn_output, the activation planes and the attention's scratch in <= 160 KB.
    Llama-3-8B's geometry fits for Q4_K_M, Q5_K_M and an all-Q6_K file; an 8-expert file's Q8_0 attn_k / attn_v fit too; Llama-2-7B's 12288 Q | K | V rows (140 KB per
    workgroup), the 70B's 8192-wide rows, head size 64, a Q8_0 attn_q / attn_output and n_embd != n_head * head_dim do not and keep the two launches."""
    import ctypes as C
    lib = pkg.load_library()
    Q40, Q80, Q4K, Q5K, Q6K = 2, 8, 12, 13, 14

    def plan(tq, tk, tv, to, E, H, G, D=128, kv=8, n_kv=576):
        slots = C.c_int32(0)
        lds = int(lib.mi355_debug_qkv_attn_plan(tq, tk, tv, to, E, H, G, D, kv, n_kv, C.byref(slots)))
        return lds, int(slots.value)

    lds, slots = plan(Q4K, Q4K, Q6K, Q4K, 4096, 32, 8)                 # Llama-3-8B Q4_K_M ("more bits" layer: attn_v in Q6_K)
    assert 100 * 1024 < lds <= 160 * 1024 and 20 <= slots <= 30, (lds, slots)
    lds4k, _ = plan(Q4K, Q4K, Q4K, Q4K, 4096, 32, 8, n_kv=4096)        # the context filled: 128-cell items, one per workgroup
    assert 0 < lds4k <= 160 * 1024
    assert plan(Q5K, Q5K, Q6K, Q5K, 4096, 32, 8)[0] > lds              # Q5_K_M: more bytes per row, still one launch
    assert 0 < plan(Q6K, Q6K, Q6K, Q6K, 4096, 32, 8)[0] <= 160 * 1024
    assert plan(Q5K, Q80, Q80, Q5K, 4096, 32, 8)[1] > 30               # Mixtral's attention tensors: more slots than a loader wave may have in flight - capped, not refused
    assert plan(Q5K, Q5K, Q6K, Q5K, 4096, 32, 32, kv=1)[0] == 0        # Llama-2-7B: 140 KB of Q | K | V rows per workgroup
    assert plan(Q4K, Q4K, Q6K, Q4K, 8192, 64, 8)[0] == 0               # Llama-3-70B on one GPU
    assert plan(Q4K, Q4K, Q4K, Q4K, 2048, 32, 4, D=64)[0] == 0         # TinyLlama: head size 64
    assert plan(Q80, Q80, Q80, Q80, 4096, 32, 8)[0] == 0               # a Q8_0 file: attn_output has no form in this launch
    assert plan(Q40, Q4K, Q4K, Q4K, 4096, 32, 8)[0] == 0
    assert plan(Q4K, Q4K, Q4K, Q4K, 3584, 32, 8)[0] == 0               # n_embd != n_head * head_dim
    assert plan(Q4K, Q4K, Q4K, Q4K, 1024, 8, 2)[0] > 0                 # the tiny test models' geometry (tests/test_gpu_model.py)
