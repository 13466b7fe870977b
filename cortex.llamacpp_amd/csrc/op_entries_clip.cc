// op_entries_clip.cc — per-op test entries of the LLaVA image encoder's launches, one at a time (csrc/clip.hip, csrc/mmf.hip; tests/test_gpu_clip_ops.py).
// Scaffolding: op_support.h.
#include "op_support.h"

using namespace mi355;

extern "C" {

// The tower's attention.  The kernel is named by the function the launcher asks (clip_attn_choice): a refusal returns here, before anything is launched.
int mi355_op_clip_attn(const float *q, const float *k, const float *v, int64_t T, int32_t H, int32_t D, int32_t n_img, float *out, uint16_t *out_h, int32_t *path) { return op_entry([&]() -> int {
    if (!q || !k || !v || !out || !path || T < 1 || T > (1 << 20) || H < 1 || D < 4 || D % 4 || n_img < 1) { fail("clip_attn: bad args"); return MI355_ERR_ARG; }
    const ClipAttnChoice ch = clip_attn_choice((int)T, D);
    *path = ch.path;
    if (ch.path == CLIP_ATTN_REFUSED) { fail("clip_attn: no kernel for this head size and row count"); return MI355_ERR_ARG; }
    const size_t n = (size_t)n_img * T * H * D;
    OpBufs b;
    const float *dq = b.upload(q, n * 4), *dk = b.upload(k, n * 4), *dv = b.upload(v, n * 4);  float *dout = b.alloc<float>(n * 4);
    uint16_t *dh = b.alloc<uint16_t>(n * 2);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_clip_attn(dq, dk, dv, (int)T, H, D, dout, out_h ? dh : nullptr, n_img, nullptr), "clip_attn")) return rc;
    if (out_h) b.down(out_h, dh, n * 2);
    return b.down(out, dout, n * 4).done("clip_attn");
}); }

int mi355_op_mul_mat_f16_xh(const uint16_t *W, int64_t N, int64_t K, const float *x, int64_t T, int64_t ld_out, const float *bias, float scale, int32_t do_scale,
                            const float *resid, int32_t in_place, int32_t form, float *y_io) { return op_entry([&]() -> int {
    if (!W || !x || !y_io || N < 1 || K < 8 || K % 8 || T < 1 || ld_out < N || (form != 0 && form != 1) || (in_place && resid) ||
        (form == 1 && (ld_out != N || (do_scale && !bias)))) { fail("mul_mat_f16_xh: bad args"); return MI355_ERR_ARG; }
    const size_t yb = (size_t)T * ld_out * 4;
    OpBufs b;
    const uint8_t *dw = b.upload((const void *)W, (size_t)N * K * 2);
    const float *dx = b.upload(x, (size_t)T * K * 4), *dr = resid ? b.upload(resid, yb) : nullptr, *bs = bias ? b.upload(bias, (size_t)N * 4) : nullptr;
    uint16_t *dxh = b.alloc<uint16_t>((size_t)T * K * 2);  float *dy = b.upload(y_io, yb), *tmp = b.alloc<float>(form == 1 ? yb : 0);
    if (!b.ok()) return oom();
    const float *rs = in_place ? dy : dr;
    hipError_t e = hipSuccess;
    if (form == 0) {
        e = launch_f32_to_f16(dx, dxh, (size_t)T * K, nullptr);
        if (e == hipSuccess) e = launch_mmf16_xh(dw, (int)N, (int)K, dxh, (int)T, dy, (int)ld_out, rs, bs, scale, do_scale != 0, nullptr);
    } else {                                                    // host/clip.cc, MI355_CLIP_XH=0: the product into scratch when a residual follows
        float *dst = rs ? tmp : dy;
        e = launch_mmf16(dw, (int)N, (int)K, dx, (int)T, dst, (int)N, nullptr, nullptr);
        if (e == hipSuccess && bs) e = launch_clip_bias(dst, bs, (int)N, (int)T, scale, do_scale != 0, nullptr);
        if (e == hipSuccess && rs) e = launch_add(rs, dst, dy, (int64_t)T * N, nullptr);
    }
    if (const int rc = finish(e, "mul_mat_f16_xh")) return rc;
    return b.down(y_io, dy, yb).done("mul_mat_f16_xh");
}); }

int mi355_op_layer_norm(const float *x, const float *w, const float *b_in, int64_t n, int64_t T, float eps, int32_t in_place, float *y, uint16_t *y_h) { return op_entry([&]() -> int {
    if (!x || !w || !b_in || !y || n < 1 || T < 1) { fail("layer_norm: bad args"); return MI355_ERR_ARG; }
    const size_t nb = (size_t)n * T * 4;
    OpBufs b;
    float *dx = b.upload(x, nb);  const float *dw = b.upload(w, (size_t)n * 4), *db = b.upload(b_in, (size_t)n * 4);  float *o = in_place ? dx : b.alloc<float>(nb);
    uint16_t *dh = b.alloc<uint16_t>(nb / 2);
    if (!b.ok()) return oom();
    const hipError_t e = y_h ? launch_layer_norm_h(dx, dw, db, (int)n, (int)T, eps, o, dh, nullptr) : launch_layer_norm(dx, dw, db, (int)n, (int)T, eps, o, nullptr);
    if (const int rc = finish(e, "layer_norm")) return rc;
    if (y_h) b.down(y_h, dh, nb / 2);
    return b.down(y, o, nb).done("layer_norm");
}); }

int mi355_op_clip_gelu(const float *x, int64_t n, int32_t quick, float *y, uint16_t *y_h) { return op_entry([&]() -> int {
    if (!x || !y || n < 1) { fail("clip_gelu: bad args"); return MI355_ERR_ARG; }
    OpBufs b;
    float *dx = b.upload(x, (size_t)n * 4);  uint16_t *dh = b.alloc<uint16_t>((size_t)n * 2);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_clip_gelu(dx, (size_t)n, quick != 0, y_h ? dh : nullptr, nullptr), "clip_gelu")) return rc;
    if (y_h) b.down(y_h, dh, (size_t)n * 2);
    return b.down(y, dx, (size_t)n * 4).done("clip_gelu");
}); }

int mi355_op_clip_im2col(const float *img, int32_t S, int32_t P, int32_t ld, float *patches_io) { return op_entry([&]() -> int {
    if (!img || !patches_io || P < 1 || S < P || S % P || ld < 3 * P * P) { fail("clip_im2col: bad args"); return MI355_ERR_ARG; }
    const size_t ib = (size_t)3 * S * S * 4, pb = (size_t)(S / P) * (S / P) * ld * 4;
    OpBufs b;
    const float *di = b.upload(img, ib);  float *dp = b.upload(patches_io, pb);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_clip_im2col(di, S, P, ld, dp, nullptr), "clip_im2col")) return rc;
    return b.down(patches_io, dp, pb).done("clip_im2col");
}); }

int mi355_op_clip_embed(const float *patch, const float *cls, const float *pos, int32_t E, int32_t T, float *emb) { return op_entry([&]() -> int {
    if (!patch || !cls || !pos || !emb || E < 1 || T < 2) { fail("clip_embed: bad args"); return MI355_ERR_ARG; }
    const size_t rb = (size_t)E * 4;
    OpBufs b;
    const float *dpa = b.upload(patch, rb * (T - 1)), *dc = b.upload(cls, rb), *dpo = b.upload(pos, rb * T);  float *de = b.alloc<float>(rb * T);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_clip_embed(dpa, dc, dpo, E, T, de, nullptr), "clip_embed")) return rc;
    return b.down(emb, de, rb * T).done("clip_embed");
}); }

int mi355_op_clip_bias(float *x_io, const float *bias, int32_t n, int32_t T, float scale, int32_t do_scale) { return op_entry([&]() -> int {
    if (!x_io || !bias || n < 1 || T < 1) { fail("clip_bias: bad args"); return MI355_ERR_ARG; }
    const size_t nb = (size_t)n * T * 4;
    OpBufs b;
    float *dx = b.upload(x_io, nb);  const float *db = b.upload(bias, (size_t)n * 4);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_clip_bias(dx, db, n, T, scale, do_scale != 0, nullptr), "clip_bias")) return rc;
    return b.down(x_io, dx, nb).done("clip_bias");
}); }

int mi355_op_add_qkv_bias(float *q_io, float *k_io, float *v_io, const float *bq, const float *bk, const float *bv, int32_t nq, int32_t nkv, int32_t T) { return op_entry([&]() -> int {
    if (nq < 1 || nkv < 0 || T < 1 || (bq && !q_io) || (bk && !k_io) || (bv && !v_io) || ((bk || bv) && nkv < 1)) { fail("add_qkv_bias: bad args"); return MI355_ERR_ARG; }
    float *const xs[3] = {q_io, k_io, v_io};
    const float *const bs[3] = {bq, bk, bv};
    const size_t n[3] = {(size_t)nq, (size_t)nkv, (size_t)nkv};
    OpBufs b;
    float *dx[3] = {};
    const float *db[3] = {};
    for (int s = 0; s < 3; s++) {
        if (xs[s]) dx[s] = b.upload(xs[s], n[s] * T * 4);
        if (bs[s]) db[s] = b.upload(bs[s], n[s] * 4);
    }
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_add_qkv_bias(dx[0], dx[1], dx[2], db[0], db[1], db[2], nq, nkv, T, nullptr), "add_qkv_bias")) return rc;
    for (int s = 0; s < 3; s++)
        if (xs[s]) b.down(xs[s], dx[s], n[s] * T * 4);
    return b.done("add_qkv_bias");
}); }

}  // extern "C"
