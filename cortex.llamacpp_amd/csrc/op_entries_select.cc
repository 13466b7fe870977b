// op_entries_select.cc — per-op test entries of the kernels that choose or gather: the MoE router, grouping and combine, arg-max, top-k, the speculative
// verify, token log-probs, KL, the importance-matrix collector (csrc/misc.hip, spec.hip, logprob.hip, imatrix.hip).  Scaffolding: op_support.h.
#include "op_support.h"

using namespace mi355;

extern "C" {

int mi355_op_moe_route(const float *logits, int64_t T, int32_t n_expert, int32_t k, int32_t *ids, float *w) { return op_entry([&]() -> int {
    if (T <= 0 || n_expert <= 0 || n_expert > 256 || k <= 0 || k > 64 || k > n_expert) { fail("moe_route: bad shape"); return MI355_ERR_ARG; }
    const size_t ns = (size_t)T * k * 4;
    OpBufs b;
    const float *dl = b.upload(logits, (size_t)T * n_expert * 4);  int32_t *di = b.alloc<int32_t>(ns);  float *dw = b.alloc<float>(ns);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_moe_route(dl, (int)T, n_expert, k, di, dw, nullptr), "moe_route")) return rc;
    return b.down(ids, di, ns).down(w, dw, ns).done("moe_route");
}); }

int mi355_op_moe_router(int32_t type, const void *gate_inp, int32_t n_expert, int64_t K, const float *x, int64_t T, int32_t k, int32_t fused,
                        const int32_t *forced, float *logits, int32_t *ids, float *w) { return op_entry([&]() -> int {
    if ((type != T_F32 && type != T_F16) || T <= 0 || K <= 0 || n_expert <= 0 || n_expert > 256 || k <= 0 || k > 64 || k > n_expert) {
        fail("moe_router: bad type or shape"); return MI355_ERR_ARG;
    }
    const size_t wb = (size_t)n_expert * K * (type == T_F32 ? 4 : 2), nl = (size_t)T * n_expert * 4, ns = (size_t)T * k * 4;
    OpBufs b;
    const uint8_t *dW = b.upload(gate_inp, wb);  const float *dx = b.upload(x, (size_t)T * K * 4);  float *dl = b.alloc<float>(nl), *dw = b.alloc<float>(ns);
    int32_t *di = b.alloc<int32_t>(ns);  const int32_t *fd = forced ? b.upload(forced, ns) : nullptr;
    if (!b.ok()) return oom();
    // fused: the one-launch router the single-token and prompt steps take for f32 / f16 gate_inp; else mmv_float, then the selection on its logits
    hipError_t e = fused ? launch_moe_router(type, dW, n_expert, (int)K, dx, (int)T, k, dl, di, dw, nullptr, fd)
                         : launch_mmv_float(type, dW, n_expert, (int)K, dx, (int)T, dl, n_expert, nullptr, nullptr);
    if (!fused && e == hipSuccess) e = launch_moe_route(dl, (int)T, n_expert, k, di, dw, nullptr, fd);
    if (const int rc = finish(e, "moe_router")) return rc;
    if (logits) b.down(logits, dl, nl);
    return b.down(ids, di, ns).down(w, dw, ns).done("moe_router");
}); }

int mi355_op_moe_group(const int32_t *ids, int64_t T, int32_t k, int32_t n_expert, int32_t *meta, int32_t *slot_of, int32_t *tok_of) { return op_entry([&]() -> int {
    if (n_expert < 1 || n_expert > 256) { fail("moe_group: n_expert outside [1, 256]"); return MI355_ERR_ARG; }
    if (T < 1 || k < 1 || T * (int64_t)k > 60 * 1024) { fail("moe_group: T * k outside [1, 61440]"); return MI355_ERR_ARG; }
    const size_t ns = (size_t)T * k, nm = ((size_t)2 * n_expert + 1) * 4;
    for (size_t i = 0; i < ns; i++)
        if (ids[i] < 0 || ids[i] >= n_expert) { fail("moe_group: ids[" + std::to_string(i) + "] outside [0, n_expert)"); return MI355_ERR_ARG; }
    OpBufs b;
    const int32_t *di = b.upload(ids, ns * 4);  int32_t *dm = b.alloc<int32_t>(nm), *dslot = b.alloc<int32_t>(ns * 4), *dtok = b.alloc<int32_t>(ns * 4);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_moe_group(di, (int)T, k, n_expert, dm, dslot, dtok, nullptr), "moe_group")) return rc;
    return b.down(meta, dm, nm).down(slot_of, dslot, ns * 4).down(tok_of, dtok, ns * 4).done("moe_group");
}); }

int mi355_op_moe_gather_act(const int8_t *qs, const float *d, const int16_t *bsums, const int8_t *qs0, const uint16_t *d0, int64_t T, int64_t K,
                            const int32_t *tok_of, int64_t n_rows, int8_t *qs_out, float *d_out, int16_t *bsums_out, int8_t *qs0_out, uint16_t *d0_out) { return op_entry([&]() -> int {
    if (T < 1 || n_rows < 1 || K < 1 || K > INT32_MAX || n_rows > INT32_MAX) { fail("moe_gather_act: bad shape"); return MI355_ERR_ARG; }
    if (K % 256) { fail("moe_gather_act: K is not a multiple of 256"); return MI355_ERR_ARG; }
    const bool q8k = qs != nullptr, q80 = qs0 != nullptr;
    if ((!q8k && !q80) || (q8k && (!d || !bsums || !qs_out || !d_out || !bsums_out)) || (q80 && (!d0 || !qs0_out || !d0_out))) {
        fail("moe_gather_act: an activation form needs all its planes, in and out"); return MI355_ERR_ARG;
    }
    for (int64_t r = 0; r < n_rows; r++)
        if (tok_of[r] < 0 || tok_of[r] >= T) { fail("moe_gather_act: tok_of[" + std::to_string(r) + "] outside [0, T)"); return MI355_ERR_ARG; }
    // plane p: bytes per row, source rows, destination rows (+ the guard row the caller filled)
    const size_t rb[5] = {(size_t)K, (size_t)(K / 256) * 4, (size_t)(K / 16) * 2, (size_t)K, (size_t)(K / 32) * 2};
    const void *in[5] = {qs, d, bsums, qs0, d0};
    void *out[5] = {qs_out, d_out, bsums_out, qs0_out, d0_out};
    const bool on[5] = {q8k, q8k, q8k, q80, q80};
    OpBufs b;
    uint8_t *s[5] = {}, *o[5] = {};
    for (int p = 0; p < 5; p++) {
        if (!on[p]) continue;
        s[p] = b.upload(in[p], rb[p] * (size_t)T);
        o[p] = b.upload(out[p], rb[p] * (size_t)(n_rows + 1));
    }
    const int32_t *dt = b.upload(tok_of, (size_t)n_rows * 4);
    if (!b.ok()) return oom();
    ActQuant src, dst;
    src.qs = (int8_t *)s[0]; src.d = (float *)s[1]; src.bsums = (int16_t *)s[2]; src.qs0 = (int8_t *)s[3]; src.d0 = (uint16_t *)s[4];
    dst.qs = (int8_t *)o[0]; dst.d = (float *)o[1]; dst.bsums = (int16_t *)o[2]; dst.qs0 = (int8_t *)o[3]; dst.d0 = (uint16_t *)o[4];
    if (const int rc = finish(launch_moe_gather_act(src, dt, (int)n_rows, (int)K, dst, nullptr), "moe_gather_act")) return rc;
    for (int p = 0; p < 5; p++)
        if (on[p]) b.down(out[p], o[p], rb[p] * (size_t)(n_rows + 1));
    return b.done("moe_gather_act");
}); }

int mi355_op_moe_combine(const float *x, const float *eo, const float *w, int64_t T, int32_t E, int32_t k, int32_t grouped, const int32_t *slot_of, float *y_out) { return op_entry([&]() -> int {
    if (T < 1 || E < 1 || k < 1 || T * (int64_t)E > INT32_MAX || T * (int64_t)k > INT32_MAX) { fail("moe_combine: bad shape"); return MI355_ERR_ARG; }
    if (grouped && !slot_of) { fail("moe_combine: the grouped form needs slot_of"); return MI355_ERR_ARG; }
    const size_t ns = (size_t)T * k, nx = (size_t)T * E * 4;
    if (grouped)
        for (size_t i = 0; i < ns; i++)
            if (slot_of[i] < 0 || (size_t)slot_of[i] >= ns) { fail("moe_combine: slot_of[" + std::to_string(i) + "] outside [0, T * k)"); return MI355_ERR_ARG; }
    OpBufs b;
    float *dx = b.upload(x, nx);  const float *de = b.upload(eo, nx * (size_t)k), *dw = b.upload(w, ns * 4);
    const int32_t *dslot = grouped ? b.upload(slot_of, ns * 4) : nullptr;
    if (!b.ok()) return oom();
    const hipError_t e = grouped ? launch_moe_scatter_combine(dx, de, dw, dslot, (int)T, E, k, nullptr) : launch_moe_combine(dx, de, dw, (int)T, E, k, (size_t)T * E, nullptr);
    if (const int rc = finish(e, "moe_combine")) return rc;
    return b.down(y_out, dx, nx).done("moe_combine");
}); }

// ---- the kernels that produce indices (csrc/misc.hip), one test entry each
int mi355_op_argmax_rows(const float *x, int64_t n, const int32_t *launches, int32_t n_launch, int32_t cap_rows, int32_t *out) { return op_entry([&]() -> int {
    if (n < 1 || n > INT32_MAX || n_launch < 1 || cap_rows < 1 || cap_rows > 65535) { fail("argmax_rows: bad shape"); return MI355_ERR_ARG; }
    size_t rows = 0;
    for (int i = 0; i < n_launch; i++) {
        if (launches[i] < 1 || launches[i] > cap_rows) { fail("argmax_rows: launch " + std::to_string(i) + " outside [1, cap_rows]"); return MI355_ERR_ARG; }
        rows += (size_t)launches[i];
    }
    OpBufs b;
    const float *dx = b.upload(x, rows * (size_t)n * 4);  int32_t *dout = b.alloc<int32_t>(rows * 4);
    float *ds = b.alloc<float>((size_t)cap_rows * 129 * 4);                               // (zero-filled: the ticket words start at 0, once)
    if (!b.ok()) return oom();
    hipError_t e = hipSuccess;
    size_t r0 = 0;
    for (int i = 0; i < n_launch && e == hipSuccess; i++) {                               // back to back on one scratch: no synchronisation in between
        e = launch_argmax_rows(dx + r0 * (size_t)n, (int)n, launches[i], dout + r0, ds, cap_rows, nullptr);
        r0 += (size_t)launches[i];
    }
    if (const int rc = finish(e, "argmax_rows")) return rc;
    return b.down(out, dout, rows * 4).done("argmax_rows");
}); }

int mi355_op_argmax_prob_rows(const float *x, int64_t n, int32_t rows, int32_t *idx_out, float *p_out) { return op_entry([&]() -> int {
    if (!x || !idx_out || !p_out || n < 1 || n > SPEC_MAX_N || rows < 1 || rows > 65535) { fail("argmax_prob_rows: bad shape"); return MI355_ERR_ARG; }
    OpBufs b;
    const float *dx = b.upload(x, (size_t)rows * (size_t)n * 4);  int32_t *di = b.alloc<int32_t>((size_t)rows * 4);
    float *dp = b.alloc<float>((size_t)rows * 4), *ds = b.alloc<float>(argmax_prob_scratch_words(rows) * 4);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_argmax_prob_rows(dx, (int)n, nullptr, rows, di, dp, ds, rows, nullptr), "argmax_prob_rows")) return rc;
    return b.down(idx_out, di, (size_t)rows * 4).down(p_out, dp, (size_t)rows * 4).done("argmax_prob_rows");
}); }

int mi355_op_topk_rows(const float *base, int64_t n, int32_t n_base_rows, const int32_t *rows, int32_t n_rows, int32_t k, const int32_t *adj_n,
                       const int32_t *adj_tok, const float *adj_bias, const int32_t *adj_cnt, const float *repeat, const float *freq, const float *present,
                       uint64_t *keys_out) { return op_entry([&]() -> int {
    if (n < 1 || n > INT32_MAX || n_base_rows < 1 || n_rows < 1 || n_rows > 65535) { fail("topk_rows: bad shape"); return MI355_ERR_ARG; }
    if (k < 1 || k > TOPK_MAX_K || k > n) { fail("topk_rows: k outside [1, min(n, " + std::to_string(TOPK_MAX_K) + ")]"); return MI355_ERR_ARG; }
    std::vector<TopkAdj> adjs((size_t)n_rows);
    for (int r = 0; r < n_rows; r++) {
        if (rows[r] < 0 || rows[r] >= n_base_rows) { fail("topk_rows: rows[" + std::to_string(r) + "] outside the base"); return MI355_ERR_ARG; }
        if (adj_n[r] < 0 || adj_n[r] > TOPK_MAX_ADJ) { fail("topk_rows: adj_n[" + std::to_string(r) + "] outside [0, " + std::to_string(TOPK_MAX_ADJ) + "]"); return MI355_ERR_ARG; }
        TopkAdj &a = adjs[(size_t)r];
        memset(&a, 0, sizeof a);
        a.n = adj_n[r]; a.repeat = repeat[r]; a.freq = freq[r]; a.present = present[r];
        const size_t o = (size_t)r * TOPK_MAX_ADJ;
        memcpy(a.tok, adj_tok + o, (size_t)a.n * sizeof(int)); memcpy(a.bias, adj_bias + o, (size_t)a.n * sizeof(float)); memcpy(a.cnt, adj_cnt + o, (size_t)a.n * sizeof(int));
    }
    const size_t nk = (size_t)n_rows * TOPK_MAX_K * 8;
    OpBufs b;
    const float *db = b.upload(base, (size_t)n_base_rows * (size_t)n * 4);  const int32_t *dr = b.upload(rows, (size_t)n_rows * 4);
    const TopkAdj *da = b.upload(adjs.data(), (size_t)n_rows * sizeof(TopkAdj));  uint8_t *ds = b.alloc(topk_scratch_bytes((int)n) * (size_t)n_rows);
    unsigned long long *dk = b.alloc<unsigned long long>(nk);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_topk_rows(db, (int)n, n_rows, dr, k, da, ds, dk, nullptr), "topk_rows")) return rc;
    std::vector<uint64_t> keys((size_t)n_rows * TOPK_MAX_K);
    if (b.down(keys.data(), dk, nk).ok())
        for (int r = 0; r < n_rows; r++) memcpy(keys_out + (size_t)r * k, keys.data() + (size_t)r * TOPK_MAX_K, (size_t)k * 8);
    return b.done("topk_rows");
}); }

int mi355_op_spec_verify(const float *logits, int64_t n, int32_t n_base_rows, const int32_t *rows, int32_t R, const int32_t *group_start, int32_t G,
                         const int32_t *draft, int32_t *ids_out, int32_t *n_accept_out) { return op_entry([&]() -> int {
    if (!logits || !rows || !group_start || !draft || !ids_out || !n_accept_out || n < 1 || n > SPEC_MAX_N || n_base_rows < 1 || R < 1 || R > SPEC_MAX_ROWS || G < 1 ||
        G > SPEC_MAX_GROUPS) { fail("spec_verify: bad shape (R <= 1088, G <= 64)"); return MI355_ERR_ARG; }
    for (int r = 0; r < R; r++)
        if (rows[r] < 0 || rows[r] >= n_base_rows) { fail("spec_verify: rows[" + std::to_string(r) + "] outside the base"); return MI355_ERR_ARG; }
    if (group_start[0] != 0 || group_start[G] != R) { fail("spec_verify: the groups do not cover rows 0 .. R - 1"); return MI355_ERR_ARG; }
    for (int g = 0; g < G; g++) {
        const int k1 = group_start[g + 1] - group_start[g];
        if (k1 < 1 || k1 > SPEC_MAX_DRAFT + 1) { fail("spec_verify: group " + std::to_string(g) + " outside 1 .. 17 rows"); return MI355_ERR_ARG; }
    }
    OpBufs b;
    const float *db = b.upload(logits, (size_t)n_base_rows * (size_t)n * 4);
    const int32_t *dr = b.upload(rows, (size_t)R * 4), *dg = b.upload(group_start, (size_t)(G + 1) * 4), *dd = b.upload(draft, (size_t)R * 4);
    int32_t *di = b.alloc<int32_t>((size_t)R * 4), *da = b.alloc<int32_t>((size_t)G * 4);  float *ds = b.alloc<float>(spec_verify_scratch_words(R) * 4);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_spec_verify(db, (int)n, dr, R, dg, G, dd, di, da, ds, R, nullptr), "spec_verify")) return rc;
    return b.down(ids_out, di, (size_t)R * 4).down(n_accept_out, da, (size_t)G * 4).done("spec_verify");
}); }

int mi355_op_token_logprob_rows(const float *base, int64_t n, int32_t n_base_rows, const int32_t *rows, const int32_t *targets, int32_t R, float *logprob_out,
                                int32_t *rank_out) { return op_entry([&]() -> int {
    if (!base || !targets || !logprob_out || !rank_out || n < 1 || n > SPEC_MAX_N || n_base_rows < 1 || R < 1 || R > 65535 || (!rows && R > n_base_rows)) {
        fail("token_logprob_rows: bad shape"); return MI355_ERR_ARG;
    }
    for (int r = 0; r < R; r++) {
        if (rows && (rows[r] < 0 || rows[r] >= n_base_rows)) { fail("token_logprob_rows: rows[" + std::to_string(r) + "] outside the base"); return MI355_ERR_ARG; }
        if (targets[r] < 0 || targets[r] >= n) { fail("token_logprob_rows: targets[" + std::to_string(r) + "] outside [0, n)"); return MI355_ERR_ARG; }
    }
    OpBufs b;
    const float *db = b.upload(base, (size_t)n_base_rows * (size_t)n * 4);
    const int32_t *dr = rows ? b.upload(rows, (size_t)R * 4) : nullptr, *dt = b.upload(targets, (size_t)R * 4);
    float *dl = b.alloc<float>((size_t)R * 4), *ds = b.alloc<float>(token_logprob_scratch_words(R) * 4);  int32_t *dk = b.alloc<int32_t>((size_t)R * 4);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_token_logprob_rows(db, (int)n, dr, dt, R, dl, dk, ds, R, nullptr), "token_logprob_rows")) return rc;
    return b.down(logprob_out, dl, (size_t)R * 4).down(rank_out, dk, (size_t)R * 4).done("token_logprob_rows");
}); }

int mi355_op_logits_kl_rows(const float *p, int32_t n_p_rows, const float *q, int32_t n_q_rows, int64_t n, const int32_t *rows_p, const int32_t *rows_q, int32_t R,
                            float *kl_out, int32_t *same_top_out) { return op_entry([&]() -> int {
    if (!p || !q || !kl_out || !same_top_out || n < 1 || n > SPEC_MAX_N || n_p_rows < 1 || n_q_rows < 1 || R < 1 || R > 65535 || (!rows_p && R > n_p_rows) ||
        (!rows_q && R > n_q_rows)) { fail("logits_kl_rows: bad shape"); return MI355_ERR_ARG; }
    for (int r = 0; r < R; r++)
        if ((rows_p && (rows_p[r] < 0 || rows_p[r] >= n_p_rows)) || (rows_q && (rows_q[r] < 0 || rows_q[r] >= n_q_rows))) {
            fail("logits_kl_rows: row " + std::to_string(r) + " outside its base"); return MI355_ERR_ARG;
        }
    OpBufs b;
    const float *dp = b.upload(p, (size_t)n_p_rows * (size_t)n * 4), *dq = b.upload(q, (size_t)n_q_rows * (size_t)n * 4);
    const int32_t *drp = rows_p ? b.upload(rows_p, (size_t)R * 4) : nullptr, *drq = rows_q ? b.upload(rows_q, (size_t)R * 4) : nullptr;
    float *dk = b.alloc<float>((size_t)R * 4), *ds = b.alloc<float>(logits_kl_scratch_words(R) * 4);  int32_t *dt = b.alloc<int32_t>((size_t)R * 4);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_logits_kl_rows(dp, dq, (int)n, drp, drq, R, dk, dt, ds, R, nullptr), "logits_kl_rows")) return rc;
    return b.down(kl_out, dk, (size_t)R * 4).down(same_top_out, dt, (size_t)R * 4).done("logits_kl_rows");
}); }

int mi355_op_imatrix_accum(const float *x, const float *x2, int64_t ld, int64_t K, int32_t R, const int32_t *row_src, int32_t n_src_rows, const int32_t *counts_per_mat,
                           int32_t n_mat, float *sum2_io, int32_t *count_io) { return op_entry([&]() -> int {
    if (!x || !sum2_io || !count_io || K < 32 || (K & 31) || K > INT32_MAX / 2 || ld < K || (ld & 3) || ld > INT32_MAX / 2 || R < 1 || R > IMX_MAX_ROWS || n_src_rows < 1 ||
        n_mat < 1 || n_mat > 256 || (n_mat > 1 && !counts_per_mat) || (!row_src && R > n_src_rows)) { fail("imatrix_accum: bad shape"); return MI355_ERR_ARG; }
    for (int r = 0; row_src && r < R; r++)
        if (row_src[r] < 0 || row_src[r] >= n_src_rows) { fail("imatrix_accum: row_src[" + std::to_string(r) + "] outside the source rows"); return MI355_ERR_ARG; }
    // meta as launch_moe_group leaves it: counts | exclusive offsets | total
    std::vector<int32_t> meta;
    if (counts_per_mat) {
        meta.assign((size_t)2 * n_mat + 1, 0);
        int64_t run = 0;
        for (int m = 0; m < n_mat; m++) {
            if (counts_per_mat[m] < 0) { fail("imatrix_accum: negative count"); return MI355_ERR_ARG; }
            meta[(size_t)m] = counts_per_mat[m]; meta[(size_t)n_mat + m] = (int32_t)std::min<int64_t>(run, R);
            run += counts_per_mat[m];
        }
        if (run != R) { fail("imatrix_accum: the counts do not add up to R"); return MI355_ERR_ARG; }
        meta[(size_t)2 * n_mat] = R;
    }
    const size_t nx = (size_t)n_src_rows * (size_t)ld * 4, ns = (size_t)(n_mat + 1) * (size_t)K * 4;
    const size_t slab_floats = imatrix_scratch_floats((int)K, R, n_mat);
    OpBufs b;
    const float *dx = b.upload(x, nx), *dx2 = x2 ? b.upload(x2, nx) : nullptr;
    const int32_t *dr = row_src ? b.upload(row_src, (size_t)R * 4) : nullptr, *dm = meta.empty() ? nullptr : b.upload(meta.data(), meta.size() * 4);
    float *dsum = b.upload(sum2_io, ns), *dslab = b.alloc<float>(slab_floats * 4);  int32_t *dcnt = b.upload(count_io, (size_t)n_mat * 4);
    if (!b.ok()) return oom();
    const hipError_t e = launch_imatrix_accum(dx, dx2, (int)ld, (int)K, R, dr, dm, n_mat, dsum, dcnt, dslab, slab_floats, nullptr);
    if (e == hipErrorInvalidValue) { fail("imatrix_accum: the launcher refuses this shape"); return MI355_ERR_ARG; }
    if (const int rc = finish(e, "imatrix_accum")) return rc;
    return b.down(sum2_io, dsum, ns).down(count_io, dcnt, (size_t)n_mat * 4).done("imatrix_accum");
}); }

}  // extern "C"
