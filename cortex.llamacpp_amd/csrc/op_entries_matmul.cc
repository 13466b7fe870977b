// op_entries_matmul.cc — per-op test entries of the mat-vec and mat-mul launches (csrc/mmvq*.hip, mmq*.hip, mmf*.hip, mmv_bf16.hip, lora.hip): one product with
// the launcher, the activation's producer and the epilogue the model gives it.  Scaffolding: op_support.h.
#include "op_support.h"

using namespace mi355;

namespace {
void use_device_cu_count() {
    hipDeviceProp_t prop;
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) set_num_cu(prop.multiProcessorCount);
}
// one weight of the mat-vec kernel's argument block, the activation from token t0 on
MMVQSeg mmvq_seg(const TestWeight &w, float *out, int ld_out) {
    MMVQSeg s{};
    s.W = w.t.data; s.out = out; s.type = w.t.type; s.n_rows = (int)w.t.N; s.ld_out = ld_out; s.row_bytes = w.t.row_bytes;
    return s;
}
void mmvq_act(MMVQArgs &a, const ActQuant &q, int64_t t0, int64_t K) {
    a.aq = q.qs + t0 * K; a.ad = q.d + t0 * (K / 256); a.abs = q.bsums + t0 * (K / 16);
    a.aq0 = q.qs0 + t0 * K; a.ad0 = q.d0 + t0 * (K / 32);
}

int op_mul_mat(int32_t type, const void *W, int64_t N, int64_t K, const float *x, int64_t T, const float *resid, float *y, int32_t *isum, int32_t *msum) {
    // the K-quants, IQ4_XS, TQ1_0 and TQ2_0: whole 256-blocks; the 32-element formats and f16 take any whole number of 32-element blocks
    if (!ggml_row_bytes(type, K) || K <= 0 || ((act_is_q80(type) || type == T_F16) ? K % 32 : K % 256)) { fail("bad type / K"); return MI355_ERR_ARG; }
    OpBufs b;
    TestWeight w(b, type, K, N);
    const float *dx = b.upload(x, (size_t)K * T * 4), *rs = resid ? b.upload(resid, (size_t)N * T * 4) : nullptr;  float *dy = b.alloc<float>((size_t)N * T * 4);
    ActBufs ab(b, (size_t)K, (size_t)T);
    if (!b.ok()) return oom();
    if (const int rc = w.load(W, "repack")) return rc;
    const uint8_t *wdev = w.t.data;
    const size_t drow = w.t.row_bytes;
    const bool quant = type_is_quant(type);
    if (resid && !(quant && ((mmq_q80_applicable(type, (int)K, (int)T)) || (mmq_q80_copy_bytes(type, N, (int)K) && mmq_q80_applicable(T_Q8_0, (int)K, (int)T) && g_op_mmq_planes)))) {
        fail("resid: only the Q8_0 prompt kernel's launches take one here"); return MI355_ERR_ARG;
    }
    hipError_t e;
    const char *what;
    if (quant) {
        e = launch_quantize(dx, (int)K, (int)T, ab.q, !act_is_q80(type), act_is_q80(type), nullptr);
        if (e != hipSuccess) return hip_fail(e, "quantize");
        if (mmq_q80_applicable(type, (int)K, (int)T)) {
            what = "mmq_q80";
            e = launch_mmq_q80(wdev, drow, (int)N, (int)K, (int)T, ab.q, dy, (int)N, rs, nullptr);
        } else if (mmq_q80_copy_bytes(type, N, (int)K) && mmq_q80_applicable(T_Q8_0, (int)K, (int)T) && g_op_mmq_planes) {   // Q4_0 / Q5_0 / IQ4_NL / Q4_1 / Q5_1 / MXFP4 prompt batches: exact Q8_0-layout copy
            what = "mmq_q80 (copy)";
            uint8_t *cp = b.alloc(mmq_q80_copy_bytes(type, N, (int)K));
            if (!b.ok()) return oom();
            e = launch_expand_q80_copy(type, wdev, drow, (int)N, (int)K, cp, nullptr);
            if (e == hipSuccess) e = launch_mmq_q80(cp, mmq_q80_copy_row_bytes(type, (int)K), (int)N, (int)K, (int)T, ab.q, dy, (int)N, rs, nullptr, mmq_q80_copy_form(type));
        } else if (g_op_mmq_ksplit && mmq_ksplit_applicable(type, (int)K, (int)T)) {
            what = "mmq_ksplit";
            int8_t *bh = b.alloc<int8_t>(mmq_prep_bytes((int)K, (int)T)), *bl = b.alloc<int8_t>(mmq_prep_bytes((int)K, (int)T));
            if (!b.ok()) return oom();
            e = launch_mmq_prep(ab.q, (int)K, (int)T, bh, bl, nullptr);
            if (e == hipSuccess) e = launch_mmq_ksplit(type, wdev, drow, (int)N, (int)K, (int)T, ab.q, bh, bl, dy, (int)N, nullptr, nullptr);
        } else if (mmq_applicable(type, (int)K, (int)T) || (type_is_planes_only(type) && T >= 32 && g_op_mmq_planes)) {   // (Q2_K / Q3_K / IQ4_XS / TQ1_0 / TQ2_0: planes only)
            what = "mmq";
            // K-split partial sums: only tensors with few rows split (a large N x T never does, and gets no workspace)
            const size_t ws_bytes = (size_t)4 * T * N * sizeof(float) <= ((size_t)256 << 20) ? (size_t)4 * T * N * sizeof(float) : 0;
            int8_t *bh = b.alloc<int8_t>(mmq_prep_bytes((int)K, (int)T)), *bl = b.alloc<int8_t>(mmq_prep_bytes((int)K, (int)T));
            uint8_t *pl = g_op_mmq_planes ? b.alloc(mmq_planes_bytes(type, N, (int)K)) : nullptr;
            MMQWorkspace wsp;
            if (g_op_mmq_planes && ws_bytes) { wsp.p = b.alloc<float>(ws_bytes); wsp.bytes = ws_bytes; }
            if (!b.ok()) return oom();
            e = launch_mmq_prep(ab.q, (int)K, (int)T, bh, bl, nullptr);
            if (e == hipSuccess && g_op_mmq_planes) e = launch_mmq_expand(type, wdev, drow, (int)N, (int)K, pl, nullptr);
            if (e == hipSuccess) e = g_op_mmq_planes ? launch_mmq_planes(type, pl, (int)N, (int)K, (int)T, ab.q, bh, bl, dy, (int)N, nullptr, nullptr, wsp)
                                                     : launch_mmq(type, wdev, drow, (int)N, (int)K, (int)T, ab.q, bh, bl, dy, (int)N, nullptr, nullptr);
        } else {
            what = "mmvq";
            e = for_token_chunks(T, [&](int64_t t0, int nt) {
                MMVQArgs a{};
                a.n_seg = 1; a.K = (int)K; a.T = nt; a.epi = EPI_STORE;
                a.seg[0] = mmvq_seg(w, dy + t0 * N, (int)N);
                mmvq_act(a, ab.q, t0, K);
                // Q4_1 / Q5_1 / MXFP4, one token: quantised in the mat-vec's prologue, as a decode step's ffn_down and head are - the weight stream takes Q8_0-activation
                // types only in that form (row pairs, single rows), the register ring with "mmvq_stream" 0; the same blocks, so the same result
                if (nt == 1 && (nib32_has_min(type) || nib32_has_e8(type)) && (K % 256) == 0) { a.fuse_mode = 2; a.nx = dx + t0 * K; }
                return launch_mmvq(a, nullptr);
            });
        }
        if (const int rc = finish(e, what)) return rc;
        if (isum && msum) {
            const int64_t nblk = act_is_q80(type) ? K / 32 : K / 256;
            int32_t *di = b.alloc<int32_t>((size_t)N * nblk * 4), *dm = b.alloc<int32_t>((size_t)N * nblk * 4);
            if (!b.ok()) return oom();
            for (int64_t t = 0; t < T; t++) {
                MMVQArgs a{};
                a.n_seg = 1; a.K = (int)K; a.T = 1; a.epi = EPI_STORE;
                a.seg[0] = mmvq_seg(w, nullptr, 0);
                mmvq_act(a, ab.q, t, K);
                if (const int rc = finish(launch_mmvq_ints(a, di, dm, nullptr), "mmvq_ints")) return rc;
                b.down(isum + t * N * nblk, di, (size_t)N * nblk * 4);
                b.down(msum + t * N * nblk, dm, (size_t)N * nblk * 4);
            }
        }
    } else {
        if (type == T_BF16) {
            // (the model path's choice for a bf16 tensor: the rows rounded to bf16 once, then the matrix cores from 8 tokens on, else the weight stream)
            what = "mul_mat (bf16)";
            uint16_t *xb = b.alloc<uint16_t>((size_t)K * T * 2);
            if (!b.ok()) return oom();
            e = launch_f32_to_bf16(dx, xb, (size_t)K * T, nullptr);
            if (e == hipSuccess) {
                if (mmbf16_applicable(type, (int)N, (int)K, (int)T, wdev, xb, dy) && (N & 3) == 0)
                    e = launch_mmbf16(wdev, (int)N, (int)K, xb, (int)T, dy, (int)N, nullptr, nullptr, 1.0f, false, nullptr);
                else {
                    MMVBF16Args a{};
                    a.n_seg = 1; a.K = (int)K; a.epi = EPI_STORE; a.xb = xb;
                    a.seg[0] = MMVBF16Seg{wdev, dy, nullptr, (int)N, (int)N, drow};
                    e = launch_mmv_bf16_tokens(a, (int)T, nullptr);
                }
            }
        } else {
            // (the model path's choice: batches against f16 tensors on the matrix cores, everything else one wave per row and token)
            what = "mmv_float";
            if (mmf16_applicable(type, (int)N, (int)K, (int)T, wdev, dx, dy) && (N & 3) == 0) e = launch_mmf16(wdev, (int)N, (int)K, dx, (int)T, dy, (int)N, nullptr, nullptr);
            else e = launch_mmv_float(type, wdev, (int)N, (int)K, dx, (int)T, dy, (int)N, nullptr, nullptr);
        }
        if (const int rc = finish(e, what)) return rc;
    }
    b.down(y, dy, (size_t)N * T * 4);
    return b.done("mul_mat");
}

// ffn_gate | ffn_up of a Q4_1 / Q5_1 / MXFP4 layer with SwiGLU, as Context::ffn_gate_up runs them: prompt batches through the two tensors' Q8_0-layout copies
// and the SwiGLU pass ("mmq_planes" 1, T >= 32), else the mat-vec with SwiGLU in its epilogue in chunks of 16, 8, 4, 2, 1 tokens
int op_ffn_gate_up_nib32(int32_t type, const void *Wg, const void *Wu, int64_t N, int64_t K, const float *x, int64_t T, float *y) {
    if (!ggml_row_bytes(type, K) || K <= 0 || K % 32 || N <= 0 || T <= 0) { fail("bad type / K"); return MI355_ERR_ARG; }
    OpBufs b;
    TestWeight wg(b, type, K, N), wu(b, type, K, N);
    const float *dx = b.upload(x, (size_t)K * T * 4);  float *dy = b.alloc<float>((size_t)N * T * 4), *du = b.alloc<float>((size_t)N * T * 4);
    ActBufs ab(b, (size_t)K, (size_t)T);
    if (!b.ok()) return oom();
    if (const int rc = wg.load(Wg, "ffn_gate_up (set-up)")) return rc;
    if (const int rc = wu.load(Wu, "ffn_gate_up (set-up)")) return rc;
    const TestWeight *ws[2] = {&wg, &wu};
    float *outs[2] = {dy, du};
    const size_t drow = wg.t.row_bytes;
    hipError_t e = hipSuccess;
    if (type == T_F16) {                                          // (Context::ffn_dense_gate_up's float branch: two products, then SwiGLU)
        for (int i = 0; i < 2 && e == hipSuccess; i++) {
            const uint8_t *w = ws[i]->t.data;
            if (mmf16_applicable(type, (int)N, (int)K, (int)T, w, dx, outs[i]) && (N & 3) == 0) e = launch_mmf16(w, (int)N, (int)K, dx, (int)T, outs[i], (int)N, nullptr, nullptr);
            else e = launch_mmv_float(type, w, (int)N, (int)K, dx, (int)T, outs[i], (int)N, nullptr, nullptr);
        }
        if (e == hipSuccess) e = launch_swiglu(dy, du, dy, N * T, nullptr);
        if (const int rc = finish(e, "ffn_gate_up (f16)")) return rc;
        b.down(y, dy, (size_t)N * T * 4);
        return b.done("ffn_gate_up");
    }
    e = launch_quantize(dx, (int)K, (int)T, ab.q, false, true, nullptr);
    if (e != hipSuccess) return hip_fail(e, "ffn_gate_up (set-up)");
    if (type == T_Q8_0 && mmq_q80_applicable(type, (int)K, (int)T)) {      // the prompt kernel on the weights themselves
        for (int i = 0; i < 2 && e == hipSuccess; i++) e = launch_mmq_q80(ws[i]->t.data, drow, (int)N, (int)K, (int)T, ab.q, outs[i], (int)N, nullptr, nullptr);
        if (e == hipSuccess) e = launch_swiglu(dy, du, dy, N * T, nullptr);
    } else if (type != T_Q8_0 && g_op_mmq_planes && mmq_q80_applicable(T_Q8_0, (int)K, (int)T)) {
        const size_t cb = mmq_q80_copy_bytes(type, N, (int)K), crow = mmq_q80_copy_row_bytes(type, (int)K);
        uint8_t *cp[2] = {b.alloc(cb), b.alloc(cb)};
        if (!b.ok()) return oom();
        for (int i = 0; i < 2 && e == hipSuccess; i++) e = launch_expand_q80_copy(type, ws[i]->t.data, drow, (int)N, (int)K, cp[i], nullptr);
        for (int i = 0; i < 2 && e == hipSuccess; i++) e = launch_mmq_q80(cp[i], crow, (int)N, (int)K, (int)T, ab.q, outs[i], (int)N, nullptr, nullptr, mmq_q80_copy_form(type));
        if (e == hipSuccess) e = launch_swiglu(dy, du, dy, N * T, nullptr);
    } else {
        e = for_token_chunks(T, [&](int64_t t0, int nt) {
            MMVQArgs a{};
            a.n_seg = 2; a.K = (int)K; a.T = nt; a.epi = EPI_SWIGLU;
            for (int i = 0; i < 2; i++) a.seg[i] = mmvq_seg(*ws[i], outs[i] + t0 * N, (int)N);
            a.aq0 = ab.q.qs0 + t0 * K; a.ad0 = ab.q.d0 + t0 * (K / 32);
            return launch_mmvq(a, nullptr);
        });
    }
    if (const int rc = finish(e, "ffn_gate_up")) return rc;
    b.down(y, dy, (size_t)N * T * 4);
    return b.done("ffn_gate_up");
}
}  // namespace

extern "C" {

int mi355_op_ffn_gate_up(int32_t type, const void *Wg, const void *Wu, int64_t N, int64_t K, const float *x, int64_t T, float *y) { return op_entry([&]() -> int {
    // the 32-element formats: any whole number of blocks (the K-quants below: their plane sets, whole 256-blocks); f16 as two products and the SwiGLU pass
    if (act_is_q80(type) || type == T_F16) return op_ffn_gate_up_nib32(type, Wg, Wu, N, K, x, T, y);
    const size_t pb = mmq_planes_bytes(type, N, (int)K);
    if (!ggml_row_bytes(type, K) || K % 256 || !pb || N % 32) { fail("bad type / K / N"); return MI355_ERR_ARG; }
    if (!mmq_planes_swiglu_ok(type, type, (int)N, (int)K, (int)T)) { fail("shape does not take the SwiGLU launch (set mmq_tiles = 4 to force it)"); return MI355_ERR_ARG; }
    OpBufs b;
    TestWeight w(b, type, K, N);                                // gate, then up: each through the device layout into its plane set
    uint8_t *pl[2] = {b.alloc(pb), b.alloc(pb)};
    const float *dx = b.upload(x, (size_t)K * T * 4);  float *dy = b.alloc<float>((size_t)N * T * 4);
    ActBufs ab(b, (size_t)K, (size_t)T);
    if (!b.ok()) return oom();
    for (int i = 0; i < 2; i++) {
        if (const int rc = w.load(i ? Wu : Wg, "ffn_gate_up")) return rc;
        if (const int rc = finish(launch_mmq_expand(type, w.t.data, w.t.row_bytes, (int)N, (int)K, pl[i], nullptr), "ffn_gate_up")) return rc;
    }
    hipError_t e = launch_quantize(dx, (int)K, (int)T, ab.q, true, false, nullptr);
    if (e == hipSuccess) e = launch_mmq_planes_swiglu(type, pl[0], pl[1], (int)N, (int)K, (int)T, ab.q, dy, (int)N, nullptr);
    if (const int rc = finish(e, "ffn_gate_up")) return rc;
    return b.down(y, dy, (size_t)N * T * 4).done("ffn_gate_up");
}); }

int mi355_op_mul_mat(int32_t type, const void *W, int64_t N, int64_t K, const float *x, int64_t T, float *y, int32_t *isum, int32_t *msum) {
    return op_entry([&]() -> int { return op_mul_mat(type, W, N, K, x, T, nullptr, y, isum, msum); });
}
int mi355_op_mul_mat_add(int32_t type, const void *W, int64_t N, int64_t K, const float *x, int64_t T, const float *resid, float *y) { return op_entry([&]() -> int {
    if (!resid) { fail("mul_mat_add: resid is null"); return MI355_ERR_ARG; }
    return op_mul_mat(type, W, N, K, x, T, resid, y, nullptr, nullptr);
}); }

// One token's mat-vec with the activation made in the launch's prologue, as a decode step's launches take it: norm_w set - RMSNorm(x) * norm_w, then Q8_0
// (fuse mode 1: Q | K | V, ffn_gate | ffn_up, the head); norm_w null - Q8_0 of x (mode 2: ffn_down).  The 32-element weight formats, K any multiple of 32 up
// to 8192.  The result has the bits of the quantiser's launch followed by mi355_op_mul_mat's.
int mi355_op_mul_mat_fused(int32_t type, const void *W, int64_t N, int64_t K, const float *x, const float *norm_w, float eps, float *y) { return op_entry([&]() -> int {
    if (!act_is_q80(type) || !ggml_row_bytes(type, K) || !W || !x || !y || N <= 0 || K <= 0 || K % 32 || K > 8192) { fail("bad type / K"); return MI355_ERR_ARG; }
    OpBufs b;
    TestWeight w(b, type, K, N);
    const float *dx = b.upload(x, (size_t)K * 4), *dw = norm_w ? b.upload(norm_w, (size_t)K * 4) : nullptr;  float *dy = b.alloc<float>((size_t)N * 4);
    if (!b.ok()) return oom();
    if (const int rc = w.load(W, "mul_mat_fused")) return rc;
    MMVQArgs a{};
    a.n_seg = 1; a.K = (int)K; a.T = 1; a.epi = EPI_STORE;
    a.seg[0] = mmvq_seg(w, dy, (int)N);
    a.fuse_mode = norm_w ? 1 : 2; a.nx = dx; a.nw = dw; a.neps = eps;
    if (const int rc = finish(launch_mmvq(a, nullptr), "mul_mat_fused")) return rc;
    return b.down(y, dy, (size_t)N * 4).done("mul_mat_fused");
}); }

// A decode step's mat-vec launch as the model issues it (make_seg / single_token_desc / mmvq_tokens of host/runtime.cc): up to three weight tensors over one
// activation, the epilogue, the prologue, the host copy, the selected-experts form.  Every output buffer is 0xFF bytes before the launch and comes back whole.
int mi355_op_mat_vec_step(int32_t n_seg, const int32_t *types, const void *const *W, const int64_t *N, int64_t K, const float *x, int64_t T, int32_t epi,
                          const float *resid, int32_t fuse, const float *norm_w, float eps, int32_t want_host_copy, int32_t n_sel, int32_t n_expert,
                          const int32_t *expert_ids, int64_t ld_pad, float *const *y, float *y_host, int32_t *path) { return op_entry([&]() -> int {
    const bool sel = n_sel > 0;
    if (n_seg < 1 || n_seg > 3 || !types || !W || !N || !x || !y || !path || K <= 0 || T < 1 || T > 17 || ld_pad < 0 || ld_pad > 64 || fuse < 0 || fuse > 2 ||
        (epi != EPI_STORE && epi != EPI_ADD && epi != EPI_SWIGLU) || (epi == EPI_ADD && (n_seg != 1 || !resid)) || (epi == EPI_SWIGLU && (n_seg != 2 || N[0] != N[1])) ||
        (fuse != 0 && T != 1) || (fuse == 1 && !norm_w) || (want_host_copy && (!y_host || T != 1)) ||
        (sel && (n_sel < 2 || n_sel > 8 || n_expert < 1 || !expert_ids || T != 1 || epi == EPI_ADD || want_host_copy || (epi == EPI_SWIGLU ? 1 : n_seg) != 1))) {
        fail("mat_vec_step: bad arguments"); return MI355_ERR_ARG;
    }
    for (int j = 0; j < n_sel; j++) if (expert_ids[j] < 0 || expert_ids[j] >= n_expert) { fail("mat_vec_step: expert id out of range"); return MI355_ERR_ARG; }
    const int64_t NE = sel ? n_expert : 1;
    const int64_t R = sel ? n_sel : T;                            // rows of every out buffer
    const int64_t XR = sel && fuse == 2 ? n_sel : T;              // rows of x: the selected experts' ffn_down quantises one row per expert
    bool need_q8k = false, need_q80 = false;
    for (int s = 0; s < n_seg; s++) {
        if (!type_is_quant(types[s]) || !ggml_row_bytes(types[s], K) || N[s] < 1 || !W[s] || (!y[s] && !(epi == EPI_SWIGLU && s == 1)) || ((act_is_q80(types[s]) ? K % 32 : K % 256) != 0)) { fail("mat_vec_step: bad segment"); return MI355_ERR_ARG; }
        (act_is_q80(types[s]) ? need_q80 : need_q8k) = true;
    }
    const int64_t ld0 = N[0] + ld_pad;
    OpBufs b;
    std::vector<TestWeight> w;
    float *dy[3] = {};
    for (int s = 0; s < n_seg; s++) {
        w.emplace_back(b, types[s], K, N[s], NE);
        dy[s] = b.alloc<float>((size_t)R * (N[s] + ld_pad) * 4, 0xFF);
    }
    const float *dx = b.upload(x, (size_t)K * XR * 4), *dnw = norm_w ? b.upload(norm_w, (size_t)K * 4) : nullptr, *dres = resid ? b.upload(resid, (size_t)R * ld0 * 4) : nullptr;
    const int32_t *esel = sel ? b.upload(expert_ids, (size_t)n_sel * 4) : nullptr;
    ActBufs ab(b, (size_t)K, (size_t)T);
    if (!b.ok()) return oom();
    for (int s = 0; s < n_seg; s++)
        if (const int rc = w[(size_t)s].load(W[s], "mat_vec_step (set-up)")) return rc;
    struct Pinned { float *p = nullptr; ~Pinned() { if (p) (void)hipHostFree(p); } } host;
    if (want_host_copy) {
        if (hipHostMalloc((void **)&host.p, (size_t)N[0] * 4, hipHostMallocDefault) != hipSuccess) { host.p = nullptr; fail("pinned alloc failed"); return MI355_ERR_OOM; }
        memset(host.p, 0xFF, (size_t)N[0] * 4);
    }
    use_device_cu_count();
    unsigned *ew = install_stream_error_word();
    hipError_t e = hipSuccess;
    if (fuse == 0) e = launch_quantize(dx, (int)K, (int)T, ab.q, need_q8k, need_q80, nullptr);
    MMVQTrace trace;
    MMVQSeg segs[3];
    for (int s = 0; s < n_seg; s++) segs[s] = make_seg(w[(size_t)s].t, dy[s], (int)(N[s] + ld_pad), s == 0 ? dres : nullptr, esel);
    if (e == hipSuccess) {
        if (sel) {                                                // (the two descriptions of Context::moe_selected_desc)
            MMVQArgs a = single_token_desc(n_seg, (int)K, epi, fuse, fuse ? dx : nullptr, fuse == 1 ? dnw : nullptr, fuse == 1 ? eps : 0.0f, ab.q);
            a.n_sel = n_sel; a.sel_out_stride = (int)ld0;
            if (fuse == 2) a.sel_nx_stride = (int)K;
            for (int s = 0; s < n_seg; s++) a.seg[s] = segs[s];
            trace.note(a);
            e = launch_mmvq(a, nullptr);
        } else {
            Fuse fz;
            fz.mode = fuse; fz.x = fuse ? dx : nullptr; fz.w = fuse == 1 ? dnw : nullptr; fz.eps = eps; fz.out_host = host.p;
            e = mmvq_tokens(segs, n_seg, (int)K, (int)T, epi, ab.q, nullptr, fz, &trace);
        }
    }
    int rc = finish(e, "mat_vec_step");
    if (rc == MI355_OK && ew && __atomic_exchange_n(ew, 0u, __ATOMIC_RELAXED)) { fail("mat_vec_step: a weight-stream kernel raised the stream error word"); rc = MI355_ERR_HIP; }
    for (int i = 0; i < 40; i++) path[i] = 0;
    for (size_t i = 0; i < trace.recs.size() && i < 5; i++) {
        const MMVQTrace::Rec &r = trace.recs[i];
        int32_t *p = path + i * 8;
        p[0] = r.T; p[1] = r.kernel;
        if (r.kernel == MMVQ_KERNEL_STREAM) { p[2] = r.form.role; p[3] = r.form.kb; p[4] = r.form.fast_ok; p[5] = r.form.down_early; p[6] = r.form.moe; p[7] = r.form.ternary; }
    }
    if (rc != MI355_OK) return rc;
    const int n_out = epi == EPI_SWIGLU ? 1 : n_seg;
    for (int s = 0; s < n_out; s++) b.down(y[s], dy[s], (size_t)R * (N[s] + ld_pad) * 4);
    if (host.p && b.ok()) memcpy(y_host, host.p, (size_t)N[0] * 4);
    return b.done("mat_vec_step");
}); }

// One mat-mul launch of a dense prompt batch or a batched decode step as the model issues it (Context::linear, linear_multi and the gate | up block of
// host/runtime.cc): the producer of the activation and of its bh / bl planes, the launcher, the epilogue, the residual in place.  Every out buffer is 0xFF bytes
// before the launch and comes back whole; a refused launch leaves them so and launches nothing.
int mi355_op_prompt_mul_mat(int32_t n_seg, const int32_t *types, const void *const *W, const int64_t *N, int64_t K, const float *x, int64_t T, int32_t epi,
                            const float *resid, int32_t in_place, int32_t prologue, const float *norm_w, float eps, int32_t form, int64_t ld_pad,
                            float *const *y, int32_t *path) { return op_entry([&]() -> int {
    if (n_seg < 1 || n_seg > 3 || !types || !W || !N || !x || !y || !path || K <= 0 || K % 256 || K > 65536 || T < 3 || T > 600 || ld_pad < 0 || ld_pad > 64) {
        fail("prompt_mul_mat: bad arguments"); return MI355_ERR_ARG;
    }
    const int n_out = epi == EPI_SWIGLU ? 1 : n_seg;
    for (int s = 0; s < n_seg; s++) if (N[s] < 1 || N[s] > (1 << 20) || !W[s] || (s < n_out && !y[s])) { fail("prompt_mul_mat: bad segment"); return MI355_ERR_ARG; }
    for (int i = 0; i < 8; i++) path[i] = 0;
    for (int s = 0; s < n_out; s++) memset(y[s], 0xFF, (size_t)T * (N[s] + ld_pad) * 4);       // what a refusal or a failure hands back
    auto refuse = [](const char *why) { fail(std::string("prompt_mul_mat: ") + why); return MI355_ERR_ARG; };
    if (epi != EPI_STORE && epi != EPI_ADD && epi != EPI_SWIGLU) return refuse("epi outside 0..2");
    if (epi == EPI_ADD && n_seg != 1) return refuse("a residual takes one tensor");
    if (epi == EPI_ADD && !resid) return refuse("epi 1 without resid");
    if (epi != EPI_ADD && (resid || in_place)) return refuse("resid / in_place without epi 1");
    if (epi == EPI_SWIGLU && (n_seg != 2 || N[0] != N[1])) return refuse("the SwiGLU pair is two tensors of one N");
    if (epi == EPI_SWIGLU && types[0] != types[1]) return refuse("the SwiGLU pair is two tensors of one type");
    if (prologue < 0 || prologue > 3 || (prologue == 1 && !norm_w)) return refuse("bad prologue");
    if (form < 0 || form > 3) return refuse("form outside 0..3");
    if (form == 3 && n_seg != 1) return refuse("the expansion on the fly takes one tensor");
    int64_t n_all = 0;
    for (int s = 0; s < n_seg; s++) {
        const int t = types[s];
        const bool kq = t == T_Q4_K || t == T_Q5_K || t == T_Q6_K, small = t == T_Q2_K || t == T_Q3_K || t == T_IQ4_XS;
        if (!kq && !(small && n_seg == 1 && (form == 0 || form == 2))) return refuse("a tensor type this launcher has no form for");
        n_all += N[s];
    }
    use_device_cu_count();
    // ---- device copies: rows in the device layout, the plane sets back to back in one arena (forms 0 and 2), out buffers, activation, workspace
    const bool want_planes = form == 0 || form == 2;
    size_t arena_bytes = 0, poff[3] = {};
    for (int s = 0; s < n_seg; s++) { poff[s] = arena_bytes; arena_bytes += mmq_planes_bytes(types[s], N[s], (int)K); }
    const size_t ws_bytes = (size_t)4 * T * n_all * sizeof(float);     // (the K-split partial sums: up to four splits of every segment)
    const size_t pb = mmq_prep_bytes((int)K, (int)T);
    OpBufs b;
    uint8_t *arena = b.alloc(want_planes ? arena_bytes : 16);
    MMQWorkspace wsp; wsp.p = b.alloc<float>(ws_bytes); wsp.bytes = ws_bytes;
    const float *dx = b.upload(x, (size_t)K * T * 4 * (prologue == 2 ? 2 : 1)), *dnw = norm_w ? b.upload(norm_w, (size_t)K * 4) : nullptr;
    int8_t *bh = b.alloc<int8_t>(pb, 0xFF), *bl = b.alloc<int8_t>(pb, 0xFF);
    ActBufs ab(b, (size_t)K, (size_t)T);
    std::vector<TestWeight> w;
    int rows[3], lds[3], tys[3];
    float *outs[3];
    const DevTensor *wp[3];
    for (int s = 0; s < n_seg; s++) {
        w.emplace_back(b, types[s], K, N[s]);
        if (want_planes) { w.back().t.planes = arena + poff[s]; w.back().t.planes_bytes = mmq_planes_bytes(types[s], N[s], (int)K); }
        rows[s] = (int)N[s]; lds[s] = (int)(N[s] + ld_pad); tys[s] = types[s]; outs[s] = b.alloc<float>((size_t)T * lds[s] * 4, 0xFF);
    }
    for (int s = 0; s < n_seg; s++) wp[s] = &w[(size_t)s].t;
    if (!b.ok()) return oom();
    // ---- which launch: the model's choice (form 0), or the launcher named; what the launcher would refuse is refused here, before anything is launched
    int kind = form, n_fused = n_seg;
    bool swiglu = epi == EPI_SWIGLU;
    if (form == 0) {
        const PromptMatmul pm = prompt_mul_mat_choice(epi == EPI_SWIGLU ? PM_ROLE_GATE_UP : n_seg == 1 ? PM_ROLE_ONE : PM_ROLE_MULTI, wp, n_seg, (int)K, (int)T, wsp);
        if (pm.form == PM_NONE) return refuse("the model has no MFMA launch for these tensors and this batch");
        if (epi == EPI_SWIGLU && !pm.swiglu) return refuse("the model runs SwiGLU behind this launch, in a pass of its own");
        kind = pm.form; n_fused = pm.n_fused;
    }
    MMQPlanesForm pf{};
    if (kind == PM_KSPLIT) {
        for (int s = 0; s < n_seg; s++) if (!mmq_ksplit_applicable(types[s], (int)K, (int)T)) return refuse("the K-split kernel does not take this type or batch");
    } else if (kind == PM_PLANES) {
        for (int s = 0; s < n_seg; s++) if (!mmq_applicable(types[s], (int)K, (int)T) && !(type_is_planes_only(types[s]) && T >= 32)) return refuse("the plane kernels take batches of 32 tokens and more");
        if (swiglu) {
            if (!mmq_planes_swiglu_ok(types[0], types[1], rows[0], (int)K, (int)T)) return refuse("launch_mmq_planes_swiglu does not take this shape");
            pf.kernel = MMQ_PLANES_LDS; pf.n_split = 1; pf.mixed = false;
        } else {
            if (form == 0 && n_fused < 2) n_fused = 1;              // (no two plane sets fuse: every tensor on its own, path describes the first)
            if (!mmq_planes_form(types[0], rows, n_fused, (int)K, (int)T, epi == EPI_ADD, wsp, tys, &pf)) return refuse("launch_mmq_planes_multi refuses these segments");
        }
    } else {
        if (!mmq_applicable(types[0], (int)K, (int)T)) return refuse("launch_mmq does not take this type or batch");
    }
    // ---- set-up: the rows in the device layout, their plane sets
    for (int s = 0; s < n_seg; s++) {
        if (const int rc = w[(size_t)s].load(W[s], "prompt_mul_mat (set-up)")) return rc;
        if (!want_planes) continue;
        if (const int rc = finish(launch_mmq_expand(types[s], wp[s]->data, wp[s]->row_bytes, (int)N[s], (int)K, wp[s]->planes, nullptr), "prompt_mul_mat (set-up)")) return rc;
    }
    // ---- the residual: in place it sits in the out buffer, as attn_output and ffn_down have it
    const size_t rbytes = (size_t)T * (N[0] + ld_pad) * 4;
    const float *rs = nullptr;
    if (epi == EPI_ADD) {
        if (in_place) { b.copy_in(outs[0], resid, rbytes); rs = outs[0]; }
        else rs = b.upload(resid, rbytes);
        if (!b.ok()) return oom();
    }
    // ---- the activation and its block-sum planes
    hipError_t e;
    if (prologue == 0) {
        e = launch_quantize(dx, (int)K, (int)T, ab.q, true, false, nullptr);
        if (e == hipSuccess) e = launch_mmq_prep(ab.q, (int)K, (int)T, bh, bl, nullptr);
    } else if (prologue == 1) e = launch_rmsnorm_quant(dx, dnw, (int)K, (int)T, eps, nullptr, &ab.q, true, false, nullptr, bh, bl);
    else if (prologue == 2) e = launch_swiglu_quant(dx, dx + (size_t)T * K, (int)K, (int)T, ab.q, true, false, nullptr, bh, bl);
    else e = launch_quantize(dx, (int)K, (int)T, ab.q, true, false, nullptr, bh, bl);
    if (e != hipSuccess) return hip_fail(e, "prompt_mul_mat (activation)");
    // ---- the launch
    if (kind == PM_KSPLIT) {
        MMQSeg sg[3];
        for (int s = 0; s < n_seg; s++) sg[s] = MMQSeg{wp[s]->data, wp[s]->row_bytes, rows[s], types[s], outs[s], lds[s], s == 0 ? rs : nullptr, 0};
        e = launch_mmq_ksplit_multi(sg, n_seg, (int)K, (int)T, ab.q, bh, bl, swiglu, nullptr);
        path[0] = 1; path[1] = mmq_ksplit_token_tiles((int)T); path[2] = 1;
    } else if (kind == PM_PLANES && swiglu) {
        e = launch_mmq_planes_swiglu(types[0], wp[0]->planes, wp[1]->planes, rows[0], (int)K, (int)T, ab.q, outs[0], lds[0], nullptr);
        path[0] = pf.kernel; path[2] = 1;
    } else if (kind == PM_PLANES) {
        e = launch_mmq_planes_multi(types[0], wp[0]->planes, rows, outs, lds, n_fused, (int)K, (int)T, ab.q, bh, bl, rs, nullptr, wsp, tys);
        for (int s = n_fused; s < n_seg && e == hipSuccess; s++)     // (form 0: the tensors the fused launch left out, each on its plane set as Context::linear_multi runs them)
            e = launch_mmq_planes(types[s], wp[s]->planes, rows[s], (int)K, (int)T, ab.q, bh, bl, outs[s], lds[s], nullptr, nullptr, wsp);
        path[0] = pf.kernel; path[2] = pf.n_split; path[3] = pf.mixed ? 1 : 0;
    } else {
        e = launch_mmq(types[0], wp[0]->data, wp[0]->row_bytes, rows[0], (int)K, (int)T, ab.q, bh, bl, outs[0], lds[0], rs, nullptr);
        path[0] = 5; path[2] = 1;
    }
    path[4] = swiglu ? 1 : 0; path[5] = prologue == 0 ? 1 : 0;
    if (const int rc = finish(e, "prompt_mul_mat")) return rc;
    for (int s = 0; s < n_out; s++) b.down(y[s], outs[s], (size_t)T * lds[s] * 4);
    return b.done("prompt_mul_mat");
}); }

int mi355_op_mul_mat_bf16(int32_t n_seg, const void *const *W, const int64_t *N, int64_t K, const float *x, int64_t T, const float *const *bias, const float *resid,
                          int32_t epi, int32_t path, int32_t tokens_per_launch, int32_t use_graph, float *const *y) { return op_entry([&]() -> int {
    if (n_seg < 1 || n_seg > 3 || !W || !N || !x || !y || K < 8 || K % 8 || (path == 2 && K % 16) || T < 1 || (epi != EPI_STORE && epi != EPI_ADD && epi != EPI_SWIGLU) || path < 0 || path > 2 ||
        (epi == EPI_ADD && (n_seg != 1 || !resid)) || (epi == EPI_SWIGLU && (n_seg != 2 || N[0] != N[1])) ||
        (tokens_per_launch != 0 && tokens_per_launch != 1 && tokens_per_launch != 2 && tokens_per_launch != 4 && tokens_per_launch != 8 && tokens_per_launch != 16)) {
        fail("mul_mat_bf16: bad arguments"); return MI355_ERR_ARG;
    }
    for (int s = 0; s < n_seg; s++) if (N[s] < 1 || !W[s]) { fail("mul_mat_bf16: bad segment"); return MI355_ERR_ARG; }
    const size_t row = (size_t)K * 2;
    const int n_out = epi == EPI_SWIGLU ? 1 : n_seg;
    OpBufs b;
    const uint8_t *dw[3] = {};
    const float *db[3] = {};
    float *dy[3] = {};
    for (int s = 0; s < n_seg; s++) {
        dw[s] = b.upload(W[s], row * (size_t)N[s]);
        db[s] = bias && bias[s] ? b.upload(bias[s], (size_t)N[s] * 4) : nullptr;
        dy[s] = b.alloc<float>((size_t)N[s] * T * 4);
    }
    const float *dx = b.upload(x, (size_t)K * T * 4), *dr = epi == EPI_ADD ? b.upload(resid, (size_t)N[0] * T * 4) : nullptr;
    uint16_t *xb = b.alloc<uint16_t>((size_t)K * T * 2);
    if (!b.ok()) return oom();
    struct Stream { hipStream_t s = nullptr; ~Stream() { if (s) (void)hipStreamDestroy(s); } } stream;
    hipError_t e = hipStreamCreate(&stream.s);
    if (e != hipSuccess) { stream.s = nullptr; return hip_fail(e, "mul_mat_bf16 (stream)"); }
    const hipStream_t st = stream.s;
    auto run = [&]() -> hipError_t {
        hipError_t e = launch_f32_to_bf16(dx, xb, (size_t)K * T, st);
        if (e != hipSuccess) return e;
        bool mfma = path == 2;
        if (path == 0) {                                      // the model path's choice (Context::linear_bf16)
            mfma = true;
            for (int s = 0; s < n_seg; s++) mfma = mfma && mmbf16_applicable(T_BF16, (int)N[s], (int)K, (int)T, dw[s], xb, dy[s]) && (N[s] & 3) == 0;
        }
        if (mfma) {
            for (int s = 0; s < n_seg && e == hipSuccess; s++) e = launch_mmbf16(dw[s], (int)N[s], (int)K, xb, (int)T, dy[s], (int)N[s], dr, db[s], 1.0f, false, st);
            if (e == hipSuccess && epi == EPI_SWIGLU) e = launch_swiglu(dy[0], dy[1], dy[0], (int64_t)T * N[0], st);
            return e;
        }
        MMVBF16Args a{};
        a.n_seg = n_seg; a.K = (int)K; a.epi = epi; a.resid = dr; a.xb = xb;
        for (int s = 0; s < n_seg; s++) a.seg[s] = MMVBF16Seg{dw[s], dy[s], db[s], (int)N[s], (int)N[s], row};
        if (tokens_per_launch == 0) return launch_mmv_bf16_tokens(a, (int)T, st);
        for (int64_t t0 = 0; t0 < T && e == hipSuccess; t0 += tokens_per_launch) {       // (tests: a fixed launch width; T must be a multiple of it)
            if (T - t0 < tokens_per_launch) return hipErrorInvalidValue;
            MMVBF16Args c = a;
            c.T = tokens_per_launch; c.xb = a.xb + t0 * K;
            if (a.resid) c.resid = a.resid + t0 * N[0];
            for (int s = 0; s < n_seg; s++) c.seg[s].out = a.seg[s].out + t0 * N[s];
            e = launch_mmv_bf16(c, st);
        }
        return e;
    };
    if (use_graph) {                                          // captured once, replayed twice: what a decode step's graph does with these launches
        hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr;
        e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
        if (e == hipSuccess) {
            const hipError_t er = run();
            const hipError_t ec = hipStreamEndCapture(st, &g);
            e = er != hipSuccess ? er : ec;
        }
        if (e == hipSuccess) e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipGraphLaunch(ge, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (ge) (void)hipGraphExecDestroy(ge);
        if (g) (void)hipGraphDestroy(g);
    } else {
        e = run();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) return hip_fail(e, "mul_mat_bf16");
    for (int s = 0; s < n_out; s++) b.down(y[s], dy[s], (size_t)N[s] * T * 4);
    return b.done("mul_mat_bf16");
}); }

// launch_lora_delta once: out[s][t][n] += scale[s] * B[s][n] . (A[s] x[t]) for n_seg segments over the rows x [T][K]; out[s] is [T][ld_out[s]], read and written
// back whole (the columns beyond N[s] come back as they went in unless the kernel wrote there)
int mi355_op_lora_delta(int32_t n_seg, const int32_t *type, const void *const *A, const void *const *B, const int32_t *r, const int64_t *N, const float *scale,
                        const float *x, int64_t K, int64_t T, const int64_t *ld_out, float *const *out) { return op_entry([&]() -> int {
    if (n_seg < 1 || n_seg > 3 || !type || !A || !B || !r || !N || !scale || !x || !ld_out || !out || K < 32 || K % 32 || K > (1 << 20) || T < 1 || T > 65536) { fail("bad args"); return MI355_ERR_ARG; }
    for (int s = 0; s < n_seg; s++)
        if ((type[s] != T_F32 && type[s] != T_F16) || r[s] < 1 || r[s] > LORA_MAX_R || N[s] < 1 || N[s] > (1 << 24) || ld_out[s] < N[s] || !A[s] || !B[s] || !out[s]) {
            fail("bad segment (F32 / F16 pairs, rank 1 .. 512, ld_out >= N)");
            return MI355_ERR_ARG;
        }
    OpBufs b;
    LoraSeg segs[3];
    const float *xd = b.upload(x, (size_t)T * K * 4);
    for (int s = 0; s < n_seg; s++) {
        const size_t es = type[s] == T_F16 ? 2 : 4;
        segs[s] = LoraSeg{b.upload(A[s], (size_t)r[s] * K * es), b.upload(B[s], (size_t)N[s] * r[s] * es), type[s], r[s], (int)N[s], scale[s],
                          b.upload(out[s], (size_t)T * ld_out[s] * 4), (int)ld_out[s]};
    }
    float *scratch = b.alloc<float>(lora_scratch_floats((int)T) * 4);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_lora_delta(segs, n_seg, xd, (int)K, (int)K, (int)T, scratch, nullptr), "lora_delta")) return rc;
    for (int s = 0; s < n_seg; s++) b.down(out[s], segs[s].out, (size_t)T * ld_out[s] * 4);
    return b.done("lora_delta");
}); }

// One grouped-expert launch of a prompt batch as Context::moe_grouped_planes / moe_grouped_q80 issue it (host/runtime.cc): the weights expanded expert by expert
// at the loader's stride (expand_prefill_planes), the grouped rows quantised, meta in moe_group_kernel's layout, rows_max = R.  Every out buffer is 0xFF bytes
// before the launch and comes back whole, guard rows included.
int mi355_op_moe_mul_mat_grouped(int32_t type, int32_t form, const void *W0, const void *W1, int32_t n_expert, int64_t N, int64_t K, const float *x,
                                 const int32_t *counts, int64_t R, int64_t ld_out, int64_t guard_rows, float *y0, float *y1) { return op_entry([&]() -> int {
    const bool planes = form == 0 || form == 1, two_w = form == 1 || form == 3, two_y = form == 3;
    if (form < 0 || form > 3 || !W0 || (two_w && !W1) || !x || !counts || !y0 || (two_y && !y1) || n_expert < 1 || n_expert > 256 || N < 1 || K < 1 || R < 1 ||
        R > 60 * 1024 || N > INT32_MAX || K > INT32_MAX || ld_out < N || ld_out > INT32_MAX || guard_rows < 0 || guard_rows > 1024) {
        fail("moe_mul_mat_grouped: bad arguments"); return MI355_ERR_ARG;
    }
    if (planes ? !mmq_planes_moe_ok(type, (int)N, (int)K) : !mmq_q80_moe_ok(type, (int)N, (int)K)) {
        fail(planes ? "moe_mul_mat_grouped: the grouped plane launch takes Q4_K / Q5_K / Q6_K / IQ4_XS / TQ1_0 / TQ2_0, N % 128 == 0, K % 256 == 0"
                    : "moe_mul_mat_grouped: the grouped Q8_0-copy launch takes MXFP4, N % 128 == 0, K % 32 == 0, 32 <= K <= 16384");
        return MI355_ERR_ARG;
    }
    std::vector<int32_t> meta((size_t)2 * n_expert + 1);
    int64_t sum = 0;
    for (int e = 0; e < n_expert; e++) {
        if (counts[e] < 0) { fail("moe_mul_mat_grouped: counts[" + std::to_string(e) + "] is negative"); return MI355_ERR_ARG; }
        meta[(size_t)e] = counts[e];
        meta[(size_t)n_expert + e] = (int32_t)sum;
        sum += counts[e];
        if (sum > R) break;
    }
    if (sum != R) { fail("moe_mul_mat_grouped: the counts do not add up to R"); return MI355_ERR_ARG; }
    meta[(size_t)2 * n_expert] = (int32_t)R;
    const size_t pb = planes ? mmq_planes_bytes(type, N, (int)K) : mmq_q80_copy_bytes(type, N, (int)K);
    const size_t stride = (pb + 255) & ~(size_t)255;             // (the loader's: every expert's set starts on 256 bytes)
    const int n_w = two_w ? 2 : 1, n_y = two_y ? 2 : 1;
    const size_t yb = (size_t)(R + guard_rows) * (size_t)ld_out * 4;
    OpBufs b;
    uint8_t *pl[2] = {};
    float *dy[2] = {};
    for (int i = 0; i < n_w; i++) pl[i] = b.alloc(stride * (size_t)n_expert);
    for (int i = 0; i < n_y; i++) dy[i] = b.alloc<float>(yb, 0xFF);
    const float *dx = b.upload(x, (size_t)K * R * 4);  const int32_t *dmeta = b.upload(meta.data(), meta.size() * 4);
    ActBufs ab(b, (size_t)K, (size_t)R);
    {
        OpBufs wb;                                               // (the rows in the device layout go once their plane sets exist)
        TestWeight w(wb, type, K, N, n_expert);
        if (!b.ok() || !wb.ok()) return oom();
        for (int i = 0; i < n_w; i++) {
            if (const int rc = w.load(i ? W1 : W0, "moe_mul_mat_grouped (weights)")) return rc;
            hipError_t e = hipSuccess;
            for (int64_t ex = 0; ex < n_expert && e == hipSuccess; ex++) {
                const uint8_t *src = w.t.data + (size_t)ex * w.t.row_bytes * (size_t)N;
                uint8_t *dst = pl[i] + (size_t)ex * stride;
                e = planes ? launch_mmq_expand(type, src, w.t.row_bytes, (int)N, (int)K, dst, nullptr) : launch_expand_q80_copy(type, src, w.t.row_bytes, (int)N, (int)K, dst, nullptr);
            }
            if (const int rc = finish(e, "moe_mul_mat_grouped (weights)")) return rc;
        }
    }
    hipError_t e = launch_quantize(dx, (int)K, (int)R, ab.q, planes, !planes, nullptr);
    if (e == hipSuccess) {
        if (form == 0) e = launch_mmq_planes_moe(type, pl[0], stride, n_expert, dmeta, (int)N, (int)K, (int)R, ab.q, dy[0], (int)ld_out, nullptr);
        else if (form == 1) e = launch_mmq_planes_swiglu_moe(type, pl[0], pl[1], stride, n_expert, dmeta, (int)N, (int)K, (int)R, ab.q, dy[0], (int)ld_out, nullptr);
        else {
            const uint8_t *w[2] = {pl[0], pl[1]};
            e = launch_mmq_q80_moe(type, w, dy, n_w, stride, n_expert, dmeta, (int)N, (int)K, (int)R, ab.q, (int)ld_out, nullptr);
        }
    }
    if (const int rc = finish(e, "moe_mul_mat_grouped")) return rc;
    b.down(y0, dy[0], yb);
    if (two_y) b.down(y1, dy[1], yb);
    return b.done("moe_mul_mat_grouped");
}); }

}  // extern "C"
