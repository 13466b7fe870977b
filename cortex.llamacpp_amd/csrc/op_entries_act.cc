// op_entries_act.cc — per-op test entries of the activation, norm, rope and row kernels (csrc/act.hip, csrc/misc.hip): one launch at a time, as the model
// launches it.  Scaffolding: op_support.h.
#include "op_support.h"

using namespace mi355;

extern "C" {

int mi355_op_quantize_act(int32_t act_type, const float *x, int64_t n, int64_t rows, void *out_blocks) { return op_entry([&]() -> int {
    // Q8_0: any whole number of 32-element blocks; a Q8_K block is 256 elements
    if ((act_type != MI355_TYPE_Q8_K && act_type != MI355_TYPE_Q8_0) || n <= 0 || rows <= 0 || n % (act_type == MI355_TYPE_Q8_K ? 256 : 32)) { fail("bad args"); return MI355_ERR_ARG; }
    const bool q8k = act_type == MI355_TYPE_Q8_K;
    const size_t ob = ggml_row_bytes(q8k ? T_Q8_K : T_Q8_0, n) * rows;
    OpBufs b;
    const float *dx = b.upload(x, (size_t)n * rows * 4);
    ActBufs ab(b, (size_t)n, (size_t)rows + 1);
    uint8_t *dout = b.alloc(ob);
    b.check(q80_guard_set(ab, (size_t)n, (size_t)rows));
    if (!b.ok()) return oom();
    hipError_t e = launch_quantize(dx, (int)n, (int)rows, ab.q, q8k, !q8k, nullptr);
    if (e == hipSuccess) e = q8k ? launch_pack_q8k_blocks(ab.q, (int)n, (int)rows, dout, nullptr) : launch_pack_q80_blocks(ab.q, (int)n, (int)rows, dout, nullptr);
    if (const int rc = finish(e, "quantize_act")) return rc;
    if (!q8k && !q80_guard_intact(ab, (size_t)n, (size_t)rows)) { fail("quantize_act: the quantiser wrote past the last row"); return MI355_ERR_HIP; }
    return b.down(out_blocks, dout, ob).done("quantize_act");
}); }

// RMSNorm * weight and the Q8_0 quantisation of its rows in one launch, as a layer's norm_quant step runs it: the per-row kernel, from 32 rows on the wide
// prompt-batch one.  out_blocks: T rows of n / 32 ggml block_q8_0; y_f32 (optional): the f32 rows the blocks were made from.  n: any multiple of 32.
int mi355_op_rms_norm_quant(const float *x, const float *w, int64_t n, int64_t T, float eps, float *y_f32, void *out_blocks) { return op_entry([&]() -> int {
    if (!x || !w || !out_blocks || n <= 0 || T <= 0 || n % 32) { fail("bad args"); return MI355_ERR_ARG; }
    const size_t xb = (size_t)n * T * 4, ob = ggml_row_bytes(T_Q8_0, n) * T;
    OpBufs b;
    const float *dx = b.upload(x, xb), *dw = b.upload(w, (size_t)n * 4);  float *dy = b.alloc<float>(xb);  uint8_t *dout = b.alloc(ob);
    ActBufs ab(b, (size_t)n, (size_t)T + 1);
    b.check(q80_guard_set(ab, (size_t)n, (size_t)T));
    if (!b.ok()) return oom();
    hipError_t e = launch_rmsnorm_quant(dx, dw, (int)n, (int)T, eps, y_f32 ? dy : nullptr, &ab.q, false, true, nullptr);
    if (e == hipSuccess) e = launch_pack_q80_blocks(ab.q, (int)n, (int)T, dout, nullptr);
    if (const int rc = finish(e, "rms_norm_quant")) return rc;
    if (!q80_guard_intact(ab, (size_t)n, (size_t)T)) { fail("rms_norm_quant: the quantiser wrote past the last row"); return MI355_ERR_HIP; }
    if (y_f32) b.down(y_f32, dy, xb);
    return b.down(out_blocks, dout, ob).done("rms_norm_quant");
}); }

// silu(gate) * up and the Q8_0 quantisation of the result in one launch (a prompt batch's step between ffn_gate | ffn_up and ffn_down).  n: any multiple of 32.
int mi355_op_swiglu_quant(const float *gate, const float *up, int64_t n, int64_t T, void *out_blocks) { return op_entry([&]() -> int {
    if (!gate || !up || !out_blocks || n <= 0 || T <= 0 || n % 32) { fail("bad args"); return MI355_ERR_ARG; }
    const size_t xb = (size_t)n * T * 4, ob = ggml_row_bytes(T_Q8_0, n) * T;
    OpBufs b;
    const float *dg = b.upload(gate, xb), *du = b.upload(up, xb);  uint8_t *dout = b.alloc(ob);
    ActBufs ab(b, (size_t)n, (size_t)T + 1);
    b.check(q80_guard_set(ab, (size_t)n, (size_t)T));
    if (!b.ok()) return oom();
    hipError_t e = launch_swiglu_quant(dg, du, (int)n, (int)T, ab.q, false, true, nullptr, nullptr, nullptr);
    if (e == hipSuccess) e = launch_pack_q80_blocks(ab.q, (int)n, (int)T, dout, nullptr);
    if (const int rc = finish(e, "swiglu_quant")) return rc;
    if (!q80_guard_intact(ab, (size_t)n, (size_t)T)) { fail("swiglu_quant: the quantiser wrote past the last row"); return MI355_ERR_HIP; }
    return b.down(out_blocks, dout, ob).done("swiglu_quant");
}); }

// One producer of the MFMA kernels' activation, with Q8_K and the bh / bl planes as the model calls it; launch_mmq_prep's planes of the same rows beside them
int mi355_op_act_q8k_planes(int32_t producer, const float *x, const float *x2, const float *norm_w, float eps, int64_t n, int64_t T, void *out_blocks,
                            int8_t *out_bh, int8_t *out_bl, int8_t *prep_bh, int8_t *prep_bl, float *y_f32) { return op_entry([&]() -> int {
    if (producer < 0 || producer > 2 || !x || (producer == 1 && !norm_w) || (producer == 2 && !x2) || (producer != 1 && y_f32) || !out_blocks || !out_bh || !out_bl ||
        !prep_bh || !prep_bl || n <= 0 || n % 256 || n > (1 << 20) || T <= 0 || T > 4096) { fail("act_q8k_planes: bad arguments"); return MI355_ERR_ARG; }
    const size_t xb = (size_t)n * T * 4, pb = mmq_prep_bytes((int)n, (int)T), ob = ggml_row_bytes(T_Q8_K, n) * T;
    OpBufs b;
    const float *dx = b.upload(x, xb), *dx2 = producer == 2 ? b.upload(x2, xb) : nullptr, *dw = producer == 1 ? b.upload(norm_w, (size_t)n * 4) : nullptr;
    float *dyf = y_f32 ? b.alloc<float>(xb) : nullptr;  uint8_t *dout = b.alloc(ob);
    int8_t *bh = b.alloc<int8_t>(pb, 0xFF), *bl = b.alloc<int8_t>(pb, 0xFF), *ph = b.alloc<int8_t>(pb), *pl = b.alloc<int8_t>(pb);
    ActBufs ab(b, (size_t)n, (size_t)T);
    if (!b.ok()) return oom();
    hipError_t e;
    if (producer == 0) e = launch_quantize(dx, (int)n, (int)T, ab.q, true, false, nullptr, bh, bl);
    else if (producer == 1) e = launch_rmsnorm_quant(dx, dw, (int)n, (int)T, eps, dyf, &ab.q, true, false, nullptr, bh, bl);
    else e = launch_swiglu_quant(dx, dx2, (int)n, (int)T, ab.q, true, false, nullptr, bh, bl);
    if (e == hipSuccess) e = launch_mmq_prep(ab.q, (int)n, (int)T, ph, pl, nullptr);
    if (e == hipSuccess) e = launch_pack_q8k_blocks(ab.q, (int)n, (int)T, dout, nullptr);
    if (const int rc = finish(e, "act_q8k_planes")) return rc;
    if (y_f32) b.down(y_f32, dyf, xb);
    return b.down(out_blocks, dout, ob).down(out_bh, bh, pb).down(out_bl, bl, pb).down(prep_bh, ph, pb).down(prep_bl, pl, pb).done("act_q8k_planes");
}); }

int mi355_op_f32_to_bf16(const float *x, int64_t n, uint16_t *out) { return op_entry([&]() -> int {
    if (n <= 0 || n % 8) { fail("f32_to_bf16: n must be a positive multiple of 8"); return MI355_ERR_ARG; }
    OpBufs b;
    const float *dx = b.upload(x, (size_t)n * 4);  uint16_t *dy = b.alloc<uint16_t>((size_t)n * 2);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_f32_to_bf16(dx, dy, (size_t)n, nullptr), "f32_to_bf16")) return rc;
    return b.down(out, dy, (size_t)n * 2).done("f32_to_bf16");
}); }

int mi355_op_f32_to_f16(const float *x, int64_t n, uint16_t *out) { return op_entry([&]() -> int {
    if (!x || !out || n < 4 || n % 4) { fail("f32_to_f16: n must be a positive multiple of 4"); return MI355_ERR_ARG; }
    OpBufs b;
    const float *dx = b.upload(x, (size_t)n * 4);  uint16_t *dy = b.alloc<uint16_t>((size_t)n * 2);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_f32_to_f16(dx, dy, (size_t)n, nullptr), "f32_to_f16")) return rc;
    return b.down(out, dy, (size_t)n * 2).done("f32_to_f16");
}); }

int mi355_op_rms_norm_mul(const float *x, const float *w, int64_t n, int64_t T, float eps, float *y) { return op_entry([&]() -> int {
    if (n <= 0 || T <= 0 || n % 32) { fail("n must be a multiple of 32"); return MI355_ERR_ARG; }
    OpBufs b;
    const float *dx = b.upload(x, (size_t)n * T * 4), *dw = b.upload(w, (size_t)n * 4);  float *dy = b.alloc<float>((size_t)n * T * 4);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_rmsnorm_quant(dx, dw, (int)n, (int)T, eps, dy, nullptr, false, false, nullptr), "rms_norm")) return rc;
    return b.down(y, dy, (size_t)n * T * 4).done("rms_norm");
}); }

// rope in place, plain (ext_factor 0) or YaRN
int mi355_op_rope_yarn(float *x, int32_t n_head, int32_t head_dim, int32_t n_rot, const int32_t *pos, int64_t T,
                       float freq_base, float freq_scale, const float *freq_factors, int32_t neox,
                       float ext_factor, float attn_factor, float corr_lo, float corr_hi) { return op_entry([&]() -> int {
    const size_t nb = (size_t)T * n_head * head_dim * 4;
    OpBufs b;
    float *dx = b.upload(x, nb);  const int32_t *dp = b.upload(pos, (size_t)T * 4);
    const float *dff = freq_factors ? b.upload(freq_factors, (size_t)(n_rot / 2) * 4) : nullptr;
    if (!b.ok()) return oom();
    RopeArgs ra{n_rot, freq_base, freq_scale, dff, neox};
    ra.ext_factor = ext_factor; ra.attn_factor = attn_factor; ra.corr_lo = corr_lo; ra.corr_hi = corr_hi;
    if (const int rc = finish(launch_rope_inplace(dx, (int)T, n_head, head_dim, dp, ra, nullptr), "rope")) return rc;
    return b.down(x, dx, nb).done("rope");
}); }

int mi355_op_rope(float *x, int32_t n_head, int32_t head_dim, int32_t n_rot, const int32_t *pos, int64_t T,
                  float freq_base, float freq_scale, const float *freq_factors, int32_t neox) {
    const RopeArgs plain{};                                       // (the YaRN fields' defaults: no extrapolation mix, attn_factor 1)
    return mi355_op_rope_yarn(x, n_head, head_dim, n_rot, pos, T, freq_base, freq_scale, freq_factors, neox, plain.ext_factor, plain.attn_factor, plain.corr_lo, plain.corr_hi);
}

int mi355_op_get_rows(int32_t type, const void *table, int64_t K, int64_t n_rows, const int32_t *ids, int64_t n_ids, float *dst) { return op_entry([&]() -> int {
    if (!ggml_row_bytes(type, K)) { fail("get_rows: bad type / K"); return MI355_ERR_ARG; }
    OpBufs b;
    TestWeight w(b, type, K, n_rows);
    const int32_t *di = b.upload(ids, (size_t)n_ids * 4);  float *dd = b.alloc<float>((size_t)n_ids * K * 4);
    if (!b.ok()) return oom();
    if (const int rc = w.load(table, "get_rows (repack)")) return rc;
    if (const int rc = finish(launch_get_rows(type, w.t.data, K, di, (int)n_ids, dd, nullptr), "get_rows")) return rc;
    return b.down(dst, dd, (size_t)n_ids * K * 4).done("get_rows");
}); }

// launch_repack_rows on its own: the device rows come back whole, over a guard pattern
int mi355_op_repack_rows(int32_t type, const void *src_rows, int64_t K, int64_t n_rows, void *dst) { return op_entry([&]() -> int {
    const int be = ggml_block_elems(type);
    if (be == 0 || K <= 0 || n_rows <= 0 || K % be) { fail("repack_rows: bad type / K / n_rows"); return MI355_ERR_ARG; }
    const size_t grow = ggml_row_bytes(type, K), drow = dev_row_bytes(type, K);
    OpBufs b;
    const uint8_t *src = b.upload(src_rows, grow * n_rows);  uint8_t *dev = b.alloc(drow * n_rows, Q80_GUARD);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_repack_rows(type, src, dev, K, n_rows, nullptr), "repack_rows")) return rc;
    return b.down(dst, dev, drow * n_rows).done("repack_rows");
}); }

int mi355_op_swiglu(const float *gate, const float *up, int64_t n, float *y) { return op_entry([&]() -> int {
    OpBufs b;
    const float *g = b.upload(gate, (size_t)n * 4), *u = b.upload(up, (size_t)n * 4);  float *o = b.alloc<float>((size_t)n * 4);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_swiglu(g, u, o, n, nullptr), "swiglu")) return rc;
    return b.down(y, o, (size_t)n * 4).done("swiglu");
}); }

int mi355_op_soft_max(const float *x, const float *mask, int64_t n, int64_t rows, float scale, float *y) { return op_entry([&]() -> int {
    const size_t nb = (size_t)n * rows * 4;
    OpBufs b;
    const float *dx = b.upload(x, nb), *dm = mask ? b.upload(mask, nb) : nullptr;  float *dy = b.alloc<float>(nb);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_soft_max(dx, dm, dy, (int)n, (int)rows, scale, nullptr), "soft_max")) return rc;
    return b.down(y, dy, nb).done("soft_max");
}); }

int mi355_op_gather_rows_f32(const float *src, int64_t n_src_rows, int64_t n, const int32_t *rows, int64_t n_rows, float *dst) { return op_entry([&]() -> int {
    if (n_src_rows < 1 || n < 1 || n_rows < 1 || n > INT32_MAX || n_rows > 65535) { fail("gather_rows_f32: bad shape"); return MI355_ERR_ARG; }
    for (int64_t r = 0; r < n_rows; r++)
        if (rows[r] < 0 || rows[r] >= n_src_rows) { fail("gather_rows_f32: rows[" + std::to_string(r) + "] outside the source"); return MI355_ERR_ARG; }
    const size_t nsrc = (size_t)n_src_rows * (size_t)n * 4, nd = (size_t)n_rows * (size_t)n * 4;
    OpBufs b;
    const float *ds = b.upload(src, nsrc);  const int32_t *dr = b.upload(rows, (size_t)n_rows * 4);  float *dd = b.alloc<float>(nd);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_gather_rows_f32(ds, dr, (int)n_rows, (int)n, dd, nullptr), "gather_rows_f32")) return rc;
    return b.down(dst, dd, nd).done("gather_rows_f32");
}); }

int mi355_op_add_row_vec(const float *x, const float *v, int32_t E, int32_t T, float *y) { return op_entry([&]() -> int {
    if (!x || !v || !y || E < 1 || T < 1) { fail("add_row_vec: bad args"); return MI355_ERR_ARG; }
    const size_t rb = (size_t)E * 4, nb = rb * (size_t)T;
    OpBufs b;
    float *dx = b.alloc<float>(nb + rb);  const float *dv = b.upload(v, rb);
    b.copy_in(dx, x, nb);
    b.check(dx && hipMemset((uint8_t *)dx + nb, Q80_GUARD, rb) == hipSuccess);        // the guard row behind the T rows
    if (!b.ok()) return oom();
    const hipError_t e = launch_add_row_vec(dx, dv, E, T, nullptr);
    if (e == hipErrorInvalidValue) { fail("add_row_vec: the launcher refuses this shape (E % 32)"); return MI355_ERR_ARG; }
    if (const int rc = finish(e, "add_row_vec")) return rc;
    return b.down(y, dx, nb + rb).done("add_row_vec");
}); }

}  // extern "C"
