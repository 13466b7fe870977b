// op_entries_attn.cc — per-op test entries of the attention and KV-cache kernels (csrc/attn.hip, attn_out.hip, attn_prefill.hip, kv_state.hip): one step's
// launches on a caller-supplied cache, as the model launches them.  Scaffolding: op_support.h.
#include "op_support.h"

using namespace mi355;

namespace {
RopeArgs rope_args(int n_rot, float freq_base, float freq_scale, const float *freq_factors, int neox) {
    RopeArgs ra{};
    ra.n_rot = n_rot; ra.freq_base = freq_base; ra.freq_scale = freq_scale; ra.freq_factors = freq_factors; ra.neox = neox;
    return ra;
}
// the chunk partials of a launch with a.splits / a.pf_splits set
void attn_workspace(OpBufs &b, AttnArgs &a) { a.part = b.alloc<float>(flash_attn_workspace_floats(a.T, a.H, a.D, std::max(a.splits, a.pf_splits)) * 4); }
// the single-token entries: the cells' sequence masks (null: every cell in sequence 0 only)
std::vector<uint64_t> cell_masks(const uint64_t *cell_seq, int n_cells) {
    return cell_seq ? std::vector<uint64_t>(cell_seq, cell_seq + n_cells) : std::vector<uint64_t>((size_t)n_cells, 1ull);
}
}  // namespace

extern "C" {

// flash_attn_ext over a caller-supplied cache and cell table (test entry): launch_flash_attn as a prompt batch or a generic step runs it.  cell_seq: the cells'
// sequence bit masks, q_seq: each query's sequence (0 .. 63); a query sees cell c < n_kv where cell_pos[c] >= 0, cell_pos[c] <= q_pos and bit q_seq of
// cell_seq[c] is set.  n_kv (1 .. n_cells) is what the kernels read from the device as the number of cells to scan; the grid, the splits and the workspace
// are sized for n_cells, as a step of a context whose high-water mark lies below the bound its launches were sized for.
int mi355_op_flash_attn_seq(const float *q, int64_t T, int32_t H, int32_t G, int32_t D, int32_t type_k, const void *k, int32_t type_v, const void *v,
                            int32_t n_cells, const int32_t *cell_pos, const uint64_t *cell_seq, const int32_t *q_pos, const int32_t *q_seq, int32_t n_kv,
                            float scale, float *out) { return op_entry([&]() -> int {
    if ((D != 64 && D != 128) || G < 1 || H < 1 || H % G || T < 1 || n_cells < 1) { fail("unsupported head geometry"); return MI355_ERR_ARG; }
    if (!kv_cache_type_ok(type_k) || !kv_cache_type_ok(type_v)) { fail("bad cache type"); return MI355_ERR_ARG; }
    if (!q || !k || !v || !cell_pos || !cell_seq || !q_pos || !q_seq || !out) { fail("flash_attn: null argument"); return MI355_ERR_ARG; }
    if (n_kv < 1 || n_kv > n_cells) { fail("flash_attn: n_kv outside [1, n_cells]"); return MI355_ERR_ARG; }
    for (int64_t t = 0; t < T; t++)
        if (q_seq[t] < 0 || q_seq[t] > 63) { fail("flash_attn: q_seq[" + std::to_string(t) + "] outside [0, 63]"); return MI355_ERR_ARG; }
    const size_t qb = (size_t)T * H * D * 4;
    OpBufs b;
    TestKVCache c(b, type_k, k, type_v, v, G, D, n_cells);
    float *dq = b.upload(q, qb), *dout = b.alloc<float>(qb);
    const AttnTables tb(b, n_cells, cell_pos, cell_seq, T, q_pos, q_seq, n_kv);
    AttnArgs a{};
    attn_inputs(a, c, T, H, scale, dq, dout, tb);
    a.splits = flash_attn_pick_splits((int)T, G, n_cells);
    a.pf_splits = flash_attn_prefill_splits((int)T, H, G, D, n_cells);
    attn_workspace(b, a);
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_flash_attn(a, nullptr), "flash_attn")) return rc;
    return b.down(out, dout, qb).done("flash_attn");
}); }

// ... with one sequence: every cell in sequence 0, every query of sequence 0, the whole table scanned
int mi355_op_flash_attn(const float *q, int64_t T, int32_t H, int32_t G, int32_t D, int32_t type_k, const void *k, int32_t type_v,
                        const void *v, int32_t n_cells, const int32_t *cell_pos, const int32_t *q_pos, float scale, float *out) { return op_entry([&]() -> int {
    if (T < 1 || n_cells < 1) { fail("unsupported head geometry"); return MI355_ERR_ARG; }
    const std::vector<uint64_t> seqm((size_t)n_cells, 1ull);
    const std::vector<int32_t> tseq((size_t)T, 0);
    return mi355_op_flash_attn_seq(q, T, H, G, D, type_k, k, type_v, v, n_cells, cell_pos, seqm.data(), q_pos, tseq.data(), n_cells, scale, out);
}); }

// How launch_flash_attn would split the keys of such a call: out[0] = flash_attn_pick_splits (the split kernel), out[1] = flash_attn_prefill_splits (the
// matrix-core prompt kernel), out[2] = 1 where the prompt kernel takes the call (test entry: a test states which splits its case runs with through this)
int mi355_op_flash_attn_plan(int64_t T, int32_t H, int32_t G, int32_t D, int32_t type_k, int32_t type_v, int32_t n_cells, int32_t *out) { return op_entry([&]() -> int {
    if ((D != 64 && D != 128) || G < 1 || H < 1 || H % G || T < 1 || T > INT32_MAX || n_cells < 1 || !out) { fail("unsupported head geometry"); return MI355_ERR_ARG; }
    AttnArgs a{};
    attn_shape(a, type_k, type_v, T, H, G, D, n_cells, 0.0f);
    out[0] = flash_attn_pick_splits((int)T, G, n_cells);
    out[1] = flash_attn_prefill_splits((int)T, H, G, D, n_cells);
    out[2] = flash_attn_prefill_applicable(a) && !(fa_v_acc_f16_enabled() && type_k == T_F16 && type_v == T_F16) ? 1 : 0;
    return MI355_OK;
}); }

// The attention block of ONE single-token step exactly as the decode path launches it (test entry): rope of q
// and of the token's K row, the K / V row quantised into the cache, attention over the visible cells, merge of the chunk partials, Q8_K quantisation and the
// attn_output mat-vec with its residual.  fused = 1: attn_out.hip (one launch); 0: the single-launch decode attention + the weight-stream mat-vec.
// k / v: the cache BEFORE the step as ggml-layout rows [n_cells][G * D] (the row at tok_cell is overwritten); cell_pos[tok_cell] must already be tok_pos.
// cell_seq (null: every cell in sequence 0 only) / tok_seq: the cells' sequence bit masks and the token's sequence, so that the cache may hold other sequences'
// cells; use_lists: the launch walks the token's chunk list (host/attn_chunks.h) as a step of a context with several sequences does.
int mi355_op_attn_step_seq(const float *q, const float *k_new, const float *v_new, int32_t H, int32_t G, int32_t D, int32_t type_k, const void *k, int32_t type_v,
                           const void *v, int32_t n_cells, const int32_t *cell_pos, const uint64_t *cell_seq, int32_t tok_pos, int32_t tok_seq, int32_t tok_cell,
                           int32_t use_lists, float rope_base, int32_t n_rot, float scale, int32_t type_o, const void *W_o, int64_t E, const float *resid,
                           int32_t fused, float *att_out, float *out, void *k_row_out, void *v_row_out) { return op_entry([&]() -> int {
    if ((D != 64 && D != 128) || G < 1 || H % G || n_cells < 1 || tok_cell < 0 || tok_cell >= n_cells) { fail("bad geometry"); return MI355_ERR_ARG; }
    if (tok_seq < 0 || tok_seq > 63) { fail("tok_seq outside [0, 63]"); return MI355_ERR_ARG; }
    if (!kv_cache_type_ok(type_k) || !kv_cache_type_ok(type_v)) { fail("bad cache type"); return MI355_ERR_ARG; }
    const int64_t K = (int64_t)H * D;
    const size_t kv_dim = (size_t)G * D;
    if (!ggml_row_bytes(type_o, K) || K % 256) { fail("bad attn_output type / K"); return MI355_ERR_ARG; }
    const std::vector<uint64_t> seqm = cell_masks(cell_seq, n_cells);
    const unsigned one = 1u;
    OpBufs b;
    TestKVCache c(b, type_k, k, type_v, v, G, D, n_cells);
    float *dq = b.upload(q, (size_t)K * 4), *datt = b.alloc<float>((size_t)K * 4), *dout = b.alloc<float>((size_t)E * 4);
    const float *dkn = b.upload(k_new, kv_dim * 4), *dvn = b.upload(v_new, kv_dim * 4), *dres = b.upload(resid, (size_t)E * 4);
    const AttnTables tb(b, n_cells, cell_pos, seqm.data(), 1, &tok_pos, &tok_seq, n_cells);
    const int32_t *dcell = b.upload(&tok_cell, 4);
    TestWeight wo(b, type_o, K, E);
    unsigned *dcnt = b.alloc<unsigned>(64 * ATT_SYNC_STRIDE * 4), *dflags = b.alloc<unsigned>(64 * ATT_SYNC_STRIDE * 4), *dserial = b.upload(&one, 4, 60);
    float *dcsb = b.alloc<float>((size_t)std::max(n_rot, 4) * 4 + 64);
    ActBufs ab(b, (size_t)K, 1);
    ChunkLists cl;
    if (use_lists) cl.make(b, n_cells, n_cells, cell_pos, seqm.data(), &tok_seq, 1);
    if (!b.ok()) return oom();
    if (const int rc = wo.load(W_o, "repack")) return rc;
    const RopeArgs ra = rope_args(n_rot, rope_base, 1.0f, nullptr, 0);
    hipError_t e = launch_rope_table(tb.tok_pos, 1, ra, dcsb, nullptr);
    if (e != hipSuccess) return hip_fail(e, "rope_table");
    AttnArgs a{};
    attn_inputs(a, c, 1, H, scale, dq, datt, tb);
    a.out_q = &ab.q; a.out_q8k = true; a.out_q80 = false;
    MMVQSeg so{};
    so.W = wo.t.data; so.out = dout; so.resid = dres; so.type = type_o; so.n_rows = (int)E; so.ld_out = (int)E; so.row_bytes = wo.t.row_bytes;
    a.splits = fused ? attn_out_fused_splits(a) : flash_attn_decode_splits(n_cells);
    if (use_lists) cl.apply(a);
    attn_workspace(b, a);
    if (fused) {
        if (!attn_out_fused_applicable(a, ra, so, (int)K, EPI_ADD)) { fail("attn_out.hip has no form for this shape"); return MI355_ERR_ARG; }
        unsigned long long *dgran = b.alloc<unsigned long long>(attn_out_granule_words((int)K) * 8);
        if (!b.ok()) return oom();
        e = launch_attn_out_fused(a, dcsb, ra, dkn, dvn, dcell, dcnt, dflags, dgran, 3, dserial, so, (int)K, EPI_ADD, nullptr);
        if (const int rc = finish(e, "attn_out_fused")) return rc;
    } else {
        if (!flash_attn_decode_fused_applicable(a, ra)) { fail("the single-launch decode attention has no form for this shape"); return MI355_ERR_ARG; }
        if (!b.ok()) return oom();
        e = launch_flash_attn_decode_fused(a, dcsb, ra, dkn, dvn, dcell, dcnt, nullptr);
        if (e != hipSuccess) return hip_fail(e, "flash_attn_decode_fused");
        MMVQArgs m{};
        m.n_seg = 1; m.K = (int)K; m.T = 1; m.epi = EPI_ADD; m.seg[0] = so;
        m.aq = ab.q.qs; m.ad = ab.q.d; m.abs = ab.q.bsums; m.aq0 = ab.q.qs0; m.ad0 = ab.q.d0;
        if (const int rc = finish(launch_mmvq(m, nullptr), "attn_output mat-vec")) return rc;
    }
    if (att_out) b.down(att_out, datt, (size_t)K * 4);
    if (out) b.down(out, dout, (size_t)E * 4);
    c.row_to_ggml(tok_cell, k_row_out, v_row_out);              // the cache row the step wrote, back in ggml block layout
    return b.done("attn_step");
}); }

int mi355_op_attn_step(const float *q, const float *k_new, const float *v_new, int32_t H, int32_t G, int32_t D, int32_t type_k, const void *k, int32_t type_v,
                       const void *v, int32_t n_cells, const int32_t *cell_pos, int32_t tok_pos, int32_t tok_cell, float rope_base, int32_t n_rot, float scale,
                       int32_t type_o, const void *W_o, int64_t E, const float *resid, int32_t fused, float *att_out, float *out, void *k_row_out, void *v_row_out) {
    return mi355_op_attn_step_seq(q, k_new, v_new, H, G, D, type_k, k, type_v, v, n_cells, cell_pos, nullptr, tok_pos, 0, tok_cell, 0, rope_base, n_rot, scale, type_o,
                                  W_o, E, resid, fused, att_out, out, k_row_out, v_row_out);
}

// The decode attention of ONE token of a qwen2 / qwen3 file as the decode path launches it (test entry): NEOX rope of q and of the token's K row - each head
// RMS-normalised and multiplied by q_norm / k_norm first where they are given (qwen3; null: no norm, the qwen2 path) - the K / V row quantised into the cache,
// attention over the visible cells and the merge of the chunk partials.  mode 1: the single-launch form of a single-token step (tickets, the last workgroup
// merges); 0: the store-fused form of a batched step (K / V stored inside the attention launch, merged by its own launch); 2: the generic path of prompt
// batches (rope_kv_store, then the split attention on the rotated q).  Cache arguments and outputs as mi355_op_attn_step.
// cell_seq (null: every cell in sequence 0 only), tok_seq, use_lists (modes 0 and 1 only): as mi355_op_attn_step_seq.
int mi355_op_attn_decode_neox_seq(const float *q, const float *k_new, const float *v_new, int32_t H, int32_t G, int32_t D, int32_t type_k, const void *k, int32_t type_v,
                                  const void *v, int32_t n_cells, const int32_t *cell_pos, const uint64_t *cell_seq, int32_t tok_pos, int32_t tok_seq, int32_t tok_cell,
                                  int32_t use_lists, float rope_base, float scale, const float *q_norm, const float *k_norm, float eps, int32_t mode, float *att_out,
                                  void *k_row_out, void *v_row_out) { return op_entry([&]() -> int {
    if ((D != 64 && D != 128) || G < 1 || H % G || n_cells < 1 || tok_cell < 0 || tok_cell >= n_cells || mode < 0 || mode > 2) { fail("bad geometry / mode"); return MI355_ERR_ARG; }
    if (tok_seq < 0 || tok_seq > 63 || (use_lists && mode == 2)) { fail("tok_seq outside [0, 63], or chunk lists asked of the generic path"); return MI355_ERR_ARG; }
    if (!kv_cache_type_ok(type_k) || !kv_cache_type_ok(type_v)) { fail("bad cache type"); return MI355_ERR_ARG; }
    const size_t K = (size_t)H * D, kv_dim = (size_t)G * D;
    const std::vector<uint64_t> seqm = cell_masks(cell_seq, n_cells);
    OpBufs b;
    TestKVCache c(b, type_k, k, type_v, v, G, D, n_cells);
    float *dq = b.upload(q, K * 4), *datt = b.alloc<float>(K * 4);  const float *dkn = b.upload(k_new, kv_dim * 4), *dvn = b.upload(v_new, kv_dim * 4);
    const AttnTables tb(b, n_cells, cell_pos, seqm.data(), 1, &tok_pos, &tok_seq, n_cells);
    const int32_t *dcell = b.upload(&tok_cell, 4);  unsigned *dcnt = b.alloc<unsigned>(64 * ATT_SYNC_STRIDE * 4);  float *dcsb = b.alloc<float>((size_t)D * 4 + 64);
    RopeArgs ra = rope_args(D, rope_base, 1.0f, nullptr, 1);
    ra.q_norm = q_norm ? b.upload(q_norm, (size_t)D * 4) : nullptr; ra.k_norm = k_norm ? b.upload(k_norm, (size_t)D * 4) : nullptr; ra.qk_eps = eps;
    ChunkLists cl;
    if (use_lists) cl.make(b, n_cells, n_cells, cell_pos, seqm.data(), &tok_seq, 1);
    if (!b.ok()) return oom();
    hipError_t e = launch_rope_table(tb.tok_pos, 1, ra, dcsb, nullptr);
    if (e != hipSuccess) return hip_fail(e, "rope_table");
    AttnArgs a{};
    attn_inputs(a, c, 1, H, scale, dq, datt, tb);
    if (mode == 2) {
        e = launch_rope_kv_store(dq, dkn, dvn, 1, H, G, D, tb.tok_pos, dcell, ra, a.kv, type_k, type_v, n_cells, dcsb, nullptr);
        if (e != hipSuccess) return hip_fail(e, "rope_kv_store");
        a.splits = flash_attn_pick_splits(1, G, n_cells);
        a.pf_splits = flash_attn_prefill_splits(1, H, G, D, n_cells);
        attn_workspace(b, a);
        if (!b.ok()) return oom();
        if (const int rc = finish(launch_flash_attn(a, nullptr), "flash_attn")) return rc;
    } else {
        a.splits = flash_attn_decode_splits(n_cells);
        if (use_lists) cl.apply(a);
        attn_workspace(b, a);
        if (!flash_attn_decode_applicable(a, ra) || (mode == 1 && !flash_attn_decode_fused_applicable(a, ra))) { fail("the decode attention has no form for this shape"); return MI355_ERR_ARG; }
        if (!b.ok()) return oom();
        if (mode == 1) e = launch_flash_attn_decode_fused(a, dcsb, ra, dkn, dvn, dcell, dcnt, nullptr);
        else e = launch_flash_attn_decode(a, dcsb, ra, nullptr, dkn, dvn, dcell);
        if (const int rc = finish(e, "flash_attn_decode")) return rc;
    }
    if (att_out) b.down(att_out, datt, K * 4);
    c.row_to_ggml(tok_cell, k_row_out, v_row_out);
    return b.done("attn_decode_neox");
}); }

int mi355_op_attn_decode_neox(const float *q, const float *k_new, const float *v_new, int32_t H, int32_t G, int32_t D, int32_t type_k, const void *k, int32_t type_v,
                              const void *v, int32_t n_cells, const int32_t *cell_pos, int32_t tok_pos, int32_t tok_cell, float rope_base, float scale,
                              const float *q_norm, const float *k_norm, float eps, int32_t mode, float *att_out, void *k_row_out, void *v_row_out) {
    return mi355_op_attn_decode_neox_seq(q, k_new, v_new, H, G, D, type_k, k, type_v, v, n_cells, cell_pos, nullptr, tok_pos, 0, tok_cell, 0, rope_base, scale, q_norm,
                                         k_norm, eps, mode, att_out, k_row_out, v_row_out);
}

// The K / V cache write of a batch on its own (test entry): the four launches that rotate K and write K / V rows into the cache,
// on a caller-supplied cache that crosses the boundary whole, in and out, as ggml-layout rows.  form 0: launch_rope_kv_store computing its angles, 1: on the
// table of launch_rope_table, 2: launch_rope_q_kv_store_fast, 3: launch_kv_store_fast.  A form that has no kernel for the arguments is refused, never launched.
int mi355_op_kv_store(int32_t form, float *q, const float *k, const float *v, int64_t T, int32_t H, int32_t G, int32_t D, int32_t n_rot, int32_t neox,
                      int32_t type_k, int32_t type_v, int32_t n_cells, const int32_t *tok_pos, const int32_t *tok_cell, float rope_base, float freq_scale,
                      const float *freq_factors, const float *q_norm, const float *k_norm, float eps, void *k_cache, void *v_cache) { return op_entry([&]() -> int {
    if (form < 0 || form > 3 || !k || !v || !tok_pos || !tok_cell || !k_cache || !v_cache || (form != 3 && !q)) { fail("bad form / null argument"); return MI355_ERR_ARG; }
    if (T < 1 || T > 4096 || H < 1 || G < 1 || D < 32 || D % 32 || n_rot < 2 || n_rot > D || n_rot % 2 || n_cells < 1) { fail("bad geometry"); return MI355_ERR_ARG; }
    if (!kv_cache_type_ok(type_k) || !kv_cache_type_ok(type_v)) { fail("bad cache type"); return MI355_ERR_ARG; }
    for (int64_t t = 0; t < T; t++)
        if (tok_cell[t] < 0 || tok_cell[t] >= n_cells) { fail("tok_cell outside the cache"); return MI355_ERR_ARG; }
    const size_t q_dim = (size_t)H * D, kv_dim = (size_t)G * D;
    if (form < 2 && ((size_t)n_rot + kv_dim) * 4 > 48 * 1024) { fail("n_head_kv * head_dim too wide for the generic kernel's LDS"); return MI355_ERR_ARG; }
    if (form < 2 && (q_norm || k_norm) && (n_rot != D || (D != 64 && D != 128))) { fail("the q / k norm works on whole heads of 64 or 128"); return MI355_ERR_ARG; }
    OpBufs b;
    TestKVCache c(b, type_k, k_cache, type_v, v_cache, G, D, n_cells);
    float *dq = b.upload_opt(q, (size_t)T * q_dim * 4), *dcsb = b.alloc<float>((size_t)T * n_rot * 4 + 64);
    const float *dkn = b.upload(k, (size_t)T * kv_dim * 4), *dvn = b.upload(v, (size_t)T * kv_dim * 4);
    const int32_t *dtp = b.upload(tok_pos, (size_t)T * 4), *dcell = b.upload(tok_cell, (size_t)T * 4);
    RopeArgs ra = rope_args(n_rot, rope_base, freq_scale, freq_factors ? b.upload(freq_factors, (size_t)(n_rot / 2) * 4, 16) : nullptr, neox ? 1 : 0);
    ra.q_norm = q_norm ? b.upload(q_norm, (size_t)D * 4) : nullptr; ra.k_norm = k_norm ? b.upload(k_norm, (size_t)D * 4) : nullptr; ra.qk_eps = eps;
    if (!b.ok()) return oom();
    if (form == 2 && !rope_q_kv_store_fast_applicable(H, G, D, type_k, type_v, ra)) { fail("the vectorised prompt store has no form for these arguments"); return MI355_ERR_ARG; }
    if (form == 3 && !kv_store_fast_applicable(G, D, type_k, type_v, ra)) { fail("the small-batch decode store has no form for these arguments"); return MI355_ERR_ARG; }
    hipError_t e = hipSuccess;
    if (form != 0) e = launch_rope_table(dtp, (int)T, ra, dcsb, nullptr);
    if (e != hipSuccess) return hip_fail(e, "rope_table");
    if (form < 2) e = launch_rope_kv_store(dq, dkn, dvn, (int)T, H, G, D, dtp, dcell, ra, c.view, type_k, type_v, n_cells, form == 1 ? dcsb : nullptr, nullptr);
    else if (form == 2) e = launch_rope_q_kv_store_fast(dq, dkn, dvn, (int)T, H, G, D, dcsb, ra, dcell, c.view, type_k, type_v, n_cells, nullptr);
    else e = launch_kv_store_fast(dkn, dvn, (int)T, G, D, dcsb, ra, dcell, c.view, type_k, type_v, n_cells, nullptr);
    if (const int rc = finish(e, "kv_store")) return rc;
    if (form != 3) b.down(q, dq, (size_t)T * q_dim * 4);
    c.rows_to_ggml(k_cache, v_cache);
    return b.done("kv_store");
}); }

// The attention of ONE batched single-token step - T tokens, up to 64, as a continuous-batching step holds them - in each form Context::attn_core launches it
// (test entry).  q [T][H * D] un-rotated, k_new / v_new [T][G * D]; k_cache / v_cache: the whole cache as ggml-layout rows [n_cells][G * D], in and out;
// cell_pos / cell_seq [n_cells] with the new cells already set (cell_pos[tok_cell[t]] = tok_pos[t], bit tok_seq[t] of cell_seq[tok_cell[t]]); n_kv: cells to
// scan (what the device reads), every launch is sized for n_cells.
//   mode 0: K rope + K / V store inside the attention launch (launch_flash_attn_decode with the new rows), every chunk of the cache scanned;
//   mode 1: the same launch on the per-token chunk lists of host/attn_chunks.h;
//   mode 2: launch_kv_store_fast, then launch_flash_attn_decode without the store, on the lists;
//   mode 3: the generic path, launch_rope_kv_store + launch_flash_attn.
// att_out [T][H * D]; q8k_out (nullable; H * D a multiple of 256): the Q8_K blocks of the T rows that the merge wrote for attn_output, as ggml block_q8_K.
// A shape or mode without a kernel is refused before anything is launched: more than 64 tokens, a token in several or in another token's sequence (modes 0
// and 1: no token may read another's new cell), what flash_attn_decode_applicable (modes 0 - 2) or kv_store_fast_applicable (the lists, mode 2) reject.
int mi355_op_attn_batch_step(const float *q, const float *k_new, const float *v_new, int64_t T, int32_t H, int32_t G, int32_t D, int32_t type_k, void *k_cache,
                             int32_t type_v, void *v_cache, int32_t n_cells, int32_t n_kv, const int32_t *cell_pos, const uint64_t *cell_seq, const int32_t *tok_pos,
                             const int32_t *tok_seq, const int32_t *tok_cell, float rope_base, int32_t n_rot, int32_t neox, float scale, int32_t mode,
                             float *att_out, void *q8k_out) {
    return mi355_op_attn_batch_step_planes(q, k_new, v_new, T, H, G, D, type_k, k_cache, type_v, v_cache, n_cells, n_kv, cell_pos, cell_seq, tok_pos, tok_seq, tok_cell,
                                           rope_base, n_rot, neox, scale, mode, att_out, q8k_out, nullptr, nullptr);
}
// bh_out / bl_out (both or neither, with q8k_out): the merge also writes the block sums of its Q8_K rows as the int8 planes of the MFMA kernels (AttnArgs out_bh /
// out_bl, what Context::attn_core sets for a K-quant attn_output); the planes are 0xFF bytes before the launch
int mi355_op_attn_batch_step_planes(const float *q, const float *k_new, const float *v_new, int64_t T, int32_t H, int32_t G, int32_t D, int32_t type_k, void *k_cache,
                                    int32_t type_v, void *v_cache, int32_t n_cells, int32_t n_kv, const int32_t *cell_pos, const uint64_t *cell_seq, const int32_t *tok_pos,
                                    const int32_t *tok_seq, const int32_t *tok_cell, float rope_base, int32_t n_rot, int32_t neox, float scale, int32_t mode,
                                    float *att_out, void *q8k_out, int8_t *bh_out, int8_t *bl_out) { return op_entry([&]() -> int {
    if ((bh_out != nullptr) != (bl_out != nullptr) || (bh_out && !q8k_out)) { fail("attn_batch_step: bh_out / bl_out come together and with q8k_out"); return MI355_ERR_ARG; }
    if (!q || !k_new || !v_new || !k_cache || !v_cache || !cell_pos || !cell_seq || !tok_pos || !tok_seq || !tok_cell || !att_out) { fail("attn_batch_step: null argument"); return MI355_ERR_ARG; }
    if (mode < 0 || mode > 3) { fail("attn_batch_step: mode outside [0, 3]"); return MI355_ERR_ARG; }
    if (T < 1 || T > 64) { fail("attn_batch_step: a batched step holds 1 .. 64 tokens"); return MI355_ERR_ARG; }
    if ((D != 64 && D != 128) || G < 1 || H < 1 || H % G || H / G > 8 || n_cells < 1 || n_kv < 1 || n_kv > n_cells || n_rot < 2 || n_rot > D || n_rot % 2) { fail("attn_batch_step: bad geometry"); return MI355_ERR_ARG; }
    if (!kv_cache_type_ok(type_k) || !kv_cache_type_ok(type_v)) { fail("attn_batch_step: bad cache type"); return MI355_ERR_ARG; }
    const size_t K = (size_t)H * D, kv_dim = (size_t)G * D;
    if (q8k_out && K % 256) { fail("attn_batch_step: Q8_K rows need n_head * head_dim to be a multiple of 256"); return MI355_ERR_ARG; }
    uint64_t seen = 0;
    for (int64_t t = 0; t < T; t++) {
        if (tok_seq[t] < 0 || tok_seq[t] > 63) { fail("attn_batch_step: tok_seq[" + std::to_string(t) + "] outside [0, 63]"); return MI355_ERR_ARG; }
        if (tok_cell[t] < 0 || tok_cell[t] >= n_kv) { fail("attn_batch_step: tok_cell[" + std::to_string(t) + "] outside the scanned cells"); return MI355_ERR_ARG; }
        const uint64_t bit = 1ull << tok_seq[t];
        if (mode < 2 && ((seen & bit) || cell_seq[tok_cell[t]] != bit)) { fail("attn_batch_step: the store-fused launch needs every token in one sequence of its own"); return MI355_ERR_ARG; }
        seen |= bit;
    }
    const RopeArgs ra = rope_args(n_rot, rope_base, 1.0f, nullptr, neox ? 1 : 0);
    AttnArgs a{};
    attn_shape(a, type_k, type_v, T, H, G, D, n_cells, scale);
    if (mode < 3 && !flash_attn_decode_applicable(a, ra)) { fail("attn_batch_step: the decode attention has no form for this shape"); return MI355_ERR_ARG; }
    if ((mode == 1 || mode == 2) && !kv_store_fast_applicable(G, D, type_k, type_v, ra)) { fail("attn_batch_step: the small-batch store has no form for these arguments (no chunk lists either)"); return MI355_ERR_ARG; }
    if (mode == 3 && ((size_t)n_rot + kv_dim) * 4 > 48 * 1024) { fail("attn_batch_step: n_head_kv * head_dim too wide for the generic store's LDS"); return MI355_ERR_ARG; }
    const size_t qb = (size_t)T * K * 4, blk = q8k_out ? ggml_row_bytes(T_Q8_K, (int64_t)K) * T : 0, pb = bh_out ? (size_t)T * (K / 16) : 0;
    OpBufs b;
    TestKVCache c(b, type_k, k_cache, type_v, v_cache, G, D, n_cells);
    float *dq = b.upload(q, qb), *datt = b.alloc<float>(qb), *dcsb = b.alloc<float>((size_t)T * n_rot * 4 + 64);
    const float *dkn = b.upload(k_new, (size_t)T * kv_dim * 4), *dvn = b.upload(v_new, (size_t)T * kv_dim * 4);
    const AttnTables tb(b, n_cells, cell_pos, cell_seq, T, tok_pos, tok_seq, n_kv);
    const int32_t *dcell = b.upload(tok_cell, (size_t)T * 4);  uint8_t *dblk = b.alloc(blk);  int8_t *dbh = b.alloc<int8_t>(pb, 0xFF), *dbl = b.alloc<int8_t>(pb, 0xFF);
    ActBufs ab(b, q8k_out ? K : 256, (size_t)T + 1);
    ChunkLists cl;
    if (mode == 1 || mode == 2) cl.make(b, n_kv, n_cells, cell_pos, cell_seq, tok_seq, (int)T);
    attn_inputs(a, c, T, H, scale, dq, datt, tb);
    if (q8k_out) { a.out_q = &ab.q; a.out_q8k = true; a.out_q80 = false; }
    if (bh_out) { a.out_bh = dbh; a.out_bl = dbl; }
    if (mode == 3) {
        a.splits = flash_attn_pick_splits((int)T, G, n_cells);
        a.pf_splits = flash_attn_prefill_splits((int)T, H, G, D, n_cells);
    } else {
        a.splits = flash_attn_decode_splits(n_cells);
        if (mode != 0) cl.apply(a);
    }
    attn_workspace(b, a);
    if (!b.ok()) return oom();
    hipError_t e = launch_rope_table(tb.tok_pos, (int)T, ra, dcsb, nullptr);
    if (e != hipSuccess) return hip_fail(e, "rope_table");
    if (mode == 3) {
        e = launch_rope_kv_store(dq, dkn, dvn, (int)T, H, G, D, tb.tok_pos, dcell, ra, a.kv, type_k, type_v, n_cells, dcsb, nullptr);
        if (e == hipSuccess) e = launch_flash_attn(a, nullptr);
    } else if (mode == 2) {
        e = launch_kv_store_fast(dkn, dvn, (int)T, G, D, dcsb, ra, dcell, a.kv, type_k, type_v, n_cells, nullptr);
        if (e == hipSuccess) e = launch_flash_attn_decode(a, dcsb, ra, nullptr);
    } else {
        e = launch_flash_attn_decode(a, dcsb, ra, nullptr, dkn, dvn, dcell);
    }
    if (e == hipSuccess && q8k_out) e = launch_pack_q8k_blocks(ab.q, (int)K, (int)T, dblk, nullptr);
    if (const int rc = finish(e, "attn_batch_step")) return rc;
    b.down(att_out, datt, qb);
    if (q8k_out) b.down(q8k_out, dblk, blk);
    if (bh_out) { b.down(bh_out, dbh, pb); b.down(bl_out, dbl, pb); }
    c.rows_to_ggml(k_cache, v_cache);
    return b.done("attn_batch_step");
}); }

// The K-shift on its own (test entry): one launch_k_shift over a caller-supplied K cache that crosses the boundary whole, in and out.
int mi355_op_k_shift(int32_t type_k, int32_t G, int32_t D, int32_t n_rot, int32_t neox, int32_t n_cells, const int32_t *delta, float rope_base, float freq_scale,
                     const float *freq_factors, float ext_factor, float attn_factor, float corr_lo, float corr_hi, void *k_cache) { return op_entry([&]() -> int {
    if (!delta || !k_cache || G < 1 || D < 32 || D % 32 || n_rot < 2 || n_rot > D || n_rot % 2 || n_cells < 1) { fail("bad geometry / null argument"); return MI355_ERR_ARG; }
    if (!kv_cache_type_ok(type_k)) { fail("bad cache type"); return MI355_ERR_ARG; }
    if (((size_t)n_rot + (size_t)G * D) * 4 > 48 * 1024) { fail("n_head_kv * head_dim too wide for the kernel's LDS"); return MI355_ERR_ARG; }
    OpBufs b;
    TestKVCache c(b, type_k, k_cache, type_k, nullptr, G, D, n_cells, false);
    const int32_t *dd = b.upload(delta, (size_t)n_cells * 4);
    RopeArgs ra = rope_args(n_rot, rope_base, freq_scale, freq_factors ? b.upload(freq_factors, (size_t)(n_rot / 2) * 4, 16) : nullptr, neox ? 1 : 0);
    ra.ext_factor = ext_factor; ra.attn_factor = attn_factor; ra.corr_lo = corr_lo; ra.corr_hi = corr_hi;
    if (!b.ok()) return oom();
    if (const int rc = finish(launch_k_shift(c.view, type_k, G, D, n_cells, dd, ra, nullptr), "k_shift")) return rc;
    c.rows_to_ggml(k_cache, nullptr);
    return b.done("k_shift");
}); }

}  // extern "C"

// The gather / scatter kernels of a sequence's state on their own (test entries): a cache of n_layer layers crosses the boundary as ggml-layout rows per layer and is
// uploaded into device planes; `cells` is checked here, as Context::state_seq_get / set check their own lists before they launch.
namespace {
struct StateOpCache {
    OpBufs b;
    std::vector<TestKVCache> layers;
    KVLayerView *table = nullptr;
    int32_t *cells = nullptr;
    uint8_t *rows = nullptr;
    size_t row_bytes = 0;
    int init(int type_k, int type_v, int n_layer, int G, int D, int n_cells, const void *const *k_rows, const void *const *v_rows, const int32_t *cell_list, int n, bool distinct) {
        if (!k_rows || !v_rows || !cell_list || n_layer < 1 || n_layer > 1024 || G < 1 || D < 32 || D % 32 || n_cells < 1 || n < 1 || n > n_cells) { fail("kv_state: bad geometry / null argument"); return MI355_ERR_ARG; }
        if (!kv_cache_type_ok(type_k) || !kv_cache_type_ok(type_v)) { fail("kv_state: bad cache type"); return MI355_ERR_ARG; }
        std::vector<char> seen((size_t)n_cells, 0);
        for (int i = 0; i < n; i++) {
            if (cell_list[i] < 0 || cell_list[i] >= n_cells) { fail("kv_state: cells[" + std::to_string(i) + "] outside the cache"); return MI355_ERR_ARG; }
            if (distinct && seen[(size_t)cell_list[i]]) { fail("kv_state: cells[" + std::to_string(i) + "] listed twice"); return MI355_ERR_ARG; }
            seen[(size_t)cell_list[i]] = 1;
        }
        for (int il = 0; il < n_layer; il++)
            if (!k_rows[il] || !v_rows[il]) { fail("kv_state: null layer"); return MI355_ERR_ARG; }
        std::vector<KVLayerView> views;
        layers.reserve((size_t)n_layer);
        for (int il = 0; il < n_layer; il++) {
            layers.emplace_back(b, type_k, k_rows[il], type_v, v_rows[il], G, D, n_cells);
            views.push_back(layers.back().view);
        }
        row_bytes = (size_t)n_layer * n * (kv_state_row_bytes(type_k, G, D) + kv_state_row_bytes(type_v, G, D));
        table = b.upload(views.data(), views.size() * sizeof(KVLayerView));
        cells = b.upload(cell_list, (size_t)n * 4);
        rows = b.alloc(row_bytes);
        return b.ok() ? MI355_OK : oom();
    }
};
}  // namespace

extern "C" {

int mi355_op_kv_state_pack(int32_t type_k, int32_t type_v, int32_t n_layer, int32_t G, int32_t D, int32_t n_cells, const void *const *k_rows, const void *const *v_rows,
                           const int32_t *cells, int32_t n, void *out) { return op_entry([&]() -> int {
    if (!out) { fail("kv_state_pack: null output"); return MI355_ERR_ARG; }
    StateOpCache c;
    if (const int rc = c.init(type_k, type_v, n_layer, G, D, n_cells, k_rows, v_rows, cells, n, false)) return rc;
    if (const int rc = finish(launch_kv_state_pack(c.table, n_layer, type_k, type_v, G, D, n_cells, c.cells, n, c.rows, nullptr), "kv_state_pack")) return rc;
    return c.b.down(out, c.rows, c.row_bytes).done("kv_state_pack");
}); }

int mi355_op_kv_state_unpack(int32_t type_k, int32_t type_v, int32_t n_layer, int32_t G, int32_t D, int32_t n_cells, const void *in, const int32_t *cells, int32_t n,
                             void *const *k_rows, void *const *v_rows) { return op_entry([&]() -> int {
    if (!in) { fail("kv_state_unpack: null input"); return MI355_ERR_ARG; }
    StateOpCache c;
    if (const int rc = c.init(type_k, type_v, n_layer, G, D, n_cells, k_rows, v_rows, cells, n, true)) return rc;
    if (!c.b.copy_in(c.rows, in, c.row_bytes)) return oom();
    if (const int rc = finish(launch_kv_state_unpack(c.table, n_layer, type_k, type_v, G, D, n_cells, c.cells, n, c.rows, nullptr), "kv_state_unpack")) return rc;
    for (int il = 0; il < n_layer; il++) c.layers[(size_t)il].rows_to_ggml(k_rows[il], v_rows[il]);
    return c.b.done("kv_state_unpack");
}); }

}  // extern "C"
