// op_support.h — what the per-op test entries (op_entries_*.cc) share with each other and with c_api.cc: the error plumbing of the C-ABI, an entry's prologue and
// epilogue, and the scaffolding a test entry stages its inputs with.  Internal: not installed, not part of include/.
#pragma once
#include "../../include/mi355_llama.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../host/attn_chunks.h"
#include "../host/runtime.h"

namespace mi355 {

// ---- c_api.cc: the one thread-local string behind mi355_last_error, the device check, the two switches mi355_debug_set_option sets for the mat-mul entries
void fail(const std::string &s);
bool need_device();
extern int g_op_mmq_planes, g_op_mmq_ksplit;

// No C++ exception may cross the C ABI (the reference's own rule for its plugin boundary, enginei.h): allocation failures
// and anything else thrown below an entry point become that entry point's error return and a last_error message.
#define MI355_GUARD(on_error, ...)                                              \
    try { __VA_ARGS__ }                                                         \
    catch (const std::bad_alloc &) { fail("out of host memory"); on_error; }    \
    catch (const std::exception &ex) { fail(std::string("internal error: ") + ex.what()); on_error; } \
    catch (...) { fail("internal error"); on_error; }

inline int hip_fail(hipError_t e, const char *what) {
    fail(std::string(what) + ": " + hipGetErrorString(e));
    return MI355_ERR_HIP;
}
inline int oom() { fail("device alloc/copy failed"); return MI355_ERR_OOM; }
// an entry's epilogue: wait for what it launched; 0 or the error return
inline int finish(hipError_t e, const char *what) {
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e == hipSuccess ? MI355_OK : hip_fail(e, what);
}
// an entry's prologue: the device first (tests/test_cabi_exports.py: -100 before any argument is looked at), then the body under the guard
template <typename F> int op_entry(F &&body) {
    if (!need_device()) return MI355_ERR_NO_DEVICE;
    MI355_GUARD(return MI355_ERR_OOM, return body();)
}

// The device buffers of one entry and whether every allocation and copy so far succeeded.  A null or zero-byte request still yields a valid 16-byte allocation.
class OpBufs {
    std::vector<void *> ptrs;
    bool good = true;
public:
    OpBufs() = default;
    OpBufs(const OpBufs &) = delete;
    OpBufs &operator=(const OpBufs &) = delete;
    ~OpBufs() { for (void *p : ptrs) (void)hipFree(p); }
    bool ok() const { return good; }
    bool check(bool step_ok) { good = good && step_ok; return step_ok; }
    // bytes filled with `fill` (every buffer starts defined: 0, or a test's 0xFF / guard pattern)
    template <typename T = uint8_t> T *alloc(size_t bytes, int fill = 0) {
        void *p = nullptr;
        ptrs.reserve(ptrs.size() + 1);
        if (!check(hipMalloc(&p, bytes ? bytes : 16) == hipSuccess)) return nullptr;
        ptrs.push_back(p);
        check(hipMemset(p, fill, bytes ? bytes : 16) == hipSuccess);
        return static_cast<T *>(p);
    }
    // bytes + pad zeroed, the first `bytes` of them from the host
    uint8_t *upload(const void *src, size_t bytes, size_t pad = 0) {
        uint8_t *p = alloc(bytes + pad);
        if (p && bytes) check(src && hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) == hipSuccess);
        return p;
    }
    template <typename T> T *upload(const T *src, size_t bytes, size_t pad = 0) { return reinterpret_cast<T *>(upload(static_cast<const void *>(src), bytes, pad)); }
    // an optional input: null leaves the bytes zero
    template <typename T> T *upload_opt(const T *src, size_t bytes) { return src ? upload(src, bytes) : alloc<T>(bytes); }
    bool copy_in(void *dev, const void *src, size_t bytes) { return check(dev && hipMemcpy(dev, src, bytes, hipMemcpyHostToDevice) == hipSuccess); }
    // read-backs chain: b.down(..).down(..).done("name")
    OpBufs &down(void *dst, const void *dev, size_t bytes) { check(dev && hipMemcpy(dst, dev, bytes, hipMemcpyDeviceToHost) == hipSuccess); return *this; }
    // the end of an entry: every read-back went through
    int done(const char *what) const {
        if (good) return MI355_OK;
        fail(std::string(what) + ": device alloc/copy failed");
        return MI355_ERR_HIP;
    }
};

struct ActBufs {
    ActQuant q;
    ActBufs(OpBufs &b, size_t K, size_t T) {
        q.qs = b.alloc<int8_t>(T * K); q.d = b.alloc<float>(T * (K / 256 + 1) * 4); q.bsums = b.alloc<int16_t>(T * (K / 16 + 1) * 2);
        q.qs0 = b.alloc<int8_t>(T * K); q.d0 = b.alloc<uint16_t>(T * (K / 32 + 1) * 2);
    }
};
// The quantiser hooks give the planes one row more than they ask for, filled with a pattern first and checked afterwards: a kernel that walks past the end
// of a row (its partial last 256-group) or of the last row lands there.
const int Q80_GUARD = 0xA5;
inline bool q80_guard_set(ActBufs &ab, size_t n, size_t rows) {
    return ab.q.qs0 && ab.q.d0 && hipMemset(ab.q.qs0 + rows * n, Q80_GUARD, n) == hipSuccess && hipMemset(ab.q.d0 + rows * (n / 32), Q80_GUARD, (n / 32) * 2) == hipSuccess;
}
inline bool q80_guard_intact(ActBufs &ab, size_t n, size_t rows) {
    std::vector<uint8_t> g(n + (n / 32) * 2);
    if (hipMemcpy(g.data(), ab.q.qs0 + rows * n, n, hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (hipMemcpy(g.data() + n, ab.q.d0 + rows * (n / 32), (n / 32) * 2, hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (uint8_t b : g) if (b != Q80_GUARD) return false;
    return true;
}

// A test weight: N rows per expert in the device layout, described as the loader describes a tensor.  load(): the host's ggml rows through launch_repack_rows.
struct TestWeight {
    DevTensor t;
    TestWeight(OpBufs &b, int type, int64_t K, int64_t N, int64_t n_expert = 1) {
        t.type = type; t.K = K; t.N = N; t.n_expert = n_expert; t.row_bytes = dev_row_bytes(type, K); t.bytes = t.row_bytes * (size_t)(N * n_expert);
        t.data = b.alloc(t.bytes);
    }
    int load(const void *rows, const char *what) {
        OpBufs tmp;
        const uint8_t *src = tmp.upload(rows, ggml_row_bytes(t.type, t.K) * (size_t)(t.N * t.n_expert));
        if (!tmp.ok() || !t.data) return oom();
        return finish(launch_repack_rows(t.type, src, t.data, t.K, t.N * t.n_expert, nullptr), what);
    }
};

// The token chunks of a batch that goes through the mat-vec kernel: 16, 8, 4, 2, 1 tokens, as Context::linear splits it.  f(t0, nt) launches one chunk.
template <typename F> hipError_t for_token_chunks(int64_t T, F &&f) {
    hipError_t e = hipSuccess;
    for (int64_t t0 = 0; t0 < T && e == hipSuccess;) {
        const int64_t rem = T - t0;
        const int nt = rem >= 16 ? 16 : rem >= 8 ? 8 : rem >= 4 ? 4 : rem >= 2 ? 2 : 1;
        e = f(t0, nt);
        t0 += nt;
    }
    return e;
}

// ---- the KV cache of an attention / cache test entry
inline bool kv_cache_type_ok(int type) { return type == T_F16 || type == T_Q8_0 || type == T_Q4_0; }
// ggml-layout cache rows [n_cells][G * D] (f16, q8_0 or q4_0 blocks) -> the device's head-major planes: codes [G][n_cells][...] and f16 block scales
inline void cache_planes_from_rows(int type, const void *rows, int G, int D, int n_cells, std::vector<uint8_t> &codes, std::vector<uint16_t> &scales) {
    const uint8_t *src = (const uint8_t *)rows;
    const size_t rb = ggml_row_bytes(type, (int64_t)G * D);
    if (type == T_F16) {
        codes.resize((size_t)G * n_cells * D * 2);
        for (int c = 0; c < n_cells; c++)
            for (int g = 0; g < G; g++) memcpy(&codes[(((size_t)g * n_cells + c) * D) * 2], src + (size_t)c * rb + (size_t)g * D * 2, (size_t)D * 2);
    } else {
        const int bb = ggml_block_bytes(type), cb = bb - 2;
        codes.resize((size_t)G * n_cells * (D / 32) * cb);
        scales.resize((size_t)G * n_cells * (D / 32));
        for (int c = 0; c < n_cells; c++)
            for (int g = 0; g < G; g++)
                for (int b = 0; b < D / 32; b++) {
                    const uint8_t *blk = src + (size_t)c * rb + ((size_t)g * (D / 32) + b) * bb;
                    memcpy(&scales[((size_t)g * n_cells + c) * (D / 32) + b], blk, 2);
                    memcpy(&codes[(((size_t)g * n_cells + c) * (D / 32) + b) * cb], blk + 2, (size_t)cb);
                }
    }
}
// ... and back: the cache row at `cell` in ggml block layout (dst: G * D elements' worth; null: nothing to do)
inline void cache_row_to_ggml(OpBufs &bufs, int type, const uint8_t *codes, const uint16_t *scales, int G, int D, int n_cells, int cell, void *dst) {
    if (!dst) return;
    uint8_t *o8 = (uint8_t *)dst;
    for (int g = 0; g < G; g++) {
        const size_t rowi = (size_t)g * n_cells + cell;
        if (type == T_F16) {
            if (!bufs.down(o8 + (size_t)g * D * 2, codes + rowi * D * 2, (size_t)D * 2).ok()) return;
        } else {
            const int bb = ggml_block_bytes(type), cb = bb - 2;
            std::vector<uint8_t> c((size_t)(D / 32) * cb);
            std::vector<uint16_t> sc((size_t)D / 32);
            if (!bufs.down(c.data(), codes + rowi * (D / 32) * cb, c.size()).down(sc.data(), scales + rowi * (D / 32), sc.size() * 2).ok()) return;
            for (int b = 0; b < D / 32; b++) {
                uint8_t *blk = o8 + ((size_t)g * (D / 32) + b) * bb;
                memcpy(blk, &sc[(size_t)b], 2);
                memcpy(blk + 2, &c[(size_t)b * cb], (size_t)cb);
            }
        }
    }
}
// ... and the whole cache: every cell of the device's planes back into ggml-layout rows [n_cells][G * D] (the inverse of cache_planes_from_rows)
inline void cache_rows_from_planes(OpBufs &bufs, int type, const uint8_t *codes, const uint16_t *scales, int G, int D, int n_cells, void *rows) {
    uint8_t *dst = (uint8_t *)rows;
    const size_t rb = ggml_row_bytes(type, (int64_t)G * D);
    const int cb = type == T_F16 ? 64 : type == T_Q8_0 ? 32 : 16, bb = type == T_F16 ? 64 : cb + 2;   // code bytes of 32 elements; bytes of their ggml block
    std::vector<uint8_t> c((size_t)G * n_cells * (D / 32) * cb);
    std::vector<uint16_t> sc(type == T_F16 ? 0 : (size_t)G * n_cells * (D / 32));
    bufs.down(c.data(), codes, c.size());
    if (!sc.empty()) bufs.down(sc.data(), scales, sc.size() * 2);
    if (!bufs.ok()) return;
    for (int cell = 0; cell < n_cells; cell++)
        for (int g = 0; g < G; g++)
            for (int b = 0; b < D / 32; b++) {
                const size_t bi = ((size_t)g * n_cells + cell) * (D / 32) + b;
                uint8_t *blk = dst + (size_t)cell * rb + ((size_t)g * (D / 32) + b) * bb;
                if (type != T_F16) { memcpy(blk, &sc[bi], 2); blk += 2; }
                memcpy(blk, &c[bi * cb], (size_t)cb);
            }
}
// One layer of a caller's cache on the device: K and (has_v) V rows converted to planes and uploaded.  The types are the caller's to check first
// (kv_cache_type_ok).  A failed copy, in or out, shows in bufs.ok().
struct TestKVCache {
    OpBufs &bufs;
    int type_k, type_v, G, D, n_cells;
    bool has_v;
    KVLayerView view{};
    TestKVCache(OpBufs &b, int type_k, const void *k_rows, int type_v, const void *v_rows, int G, int D, int n_cells, bool has_v = true)
        : bufs(b), type_k(type_k), type_v(type_v), G(G), D(D), n_cells(n_cells), has_v(has_v) {
        stage(type_k, k_rows, view.k, view.kd);
        if (has_v) stage(type_v, v_rows, view.v, view.vd);
    }
    // the row at `cell` (a null destination is skipped) / the whole cache, back in ggml layout
    void row_to_ggml(int cell, void *k_row, void *v_row) {
        cache_row_to_ggml(bufs, type_k, view.k, view.kd, G, D, n_cells, cell, k_row);
        cache_row_to_ggml(bufs, type_v, view.v, view.vd, G, D, n_cells, cell, v_row);
    }
    void rows_to_ggml(void *k_rows, void *v_rows) {
        cache_rows_from_planes(bufs, type_k, view.k, view.kd, G, D, n_cells, k_rows);
        if (has_v) cache_rows_from_planes(bufs, type_v, view.v, view.vd, G, D, n_cells, v_rows);
    }
private:
    void stage(int type, const void *rows, uint8_t *&codes, uint16_t *&scales) {
        std::vector<uint8_t> c;
        std::vector<uint16_t> s;
        cache_planes_from_rows(type, rows, G, D, n_cells, c, s);
        codes = bufs.upload(c.data(), c.size());
        scales = bufs.upload(s.data(), s.size() * 2, 16);
    }
};

// The cell table and the tokens' positions and sequences of an attention entry, and the number of cells the kernels read from the device
struct AttnTables {
    int32_t *cell_pos, *tok_pos, *tok_seq, *n_kv;
    uint64_t *cell_seq;
    AttnTables(OpBufs &b, int n_cells, const int32_t *cp, const uint64_t *cs, int64_t T, const int32_t *tp, const int32_t *ts, int32_t n_kv_scan)
        : cell_pos(b.upload(cp, (size_t)n_cells * 4)), tok_pos(b.upload(tp, (size_t)T * 4)), tok_seq(b.upload(ts, (size_t)T * 4)), n_kv(b.upload(&n_kv_scan, 4)),
          cell_seq(b.upload(cs, (size_t)n_cells * 8)) {}
};
// The fields every attention launch of a test entry sets alike: the shape (what the *_applicable questions read) ...
inline void attn_shape(AttnArgs &a, int type_k, int type_v, int64_t T, int H, int G, int D, int n_cells, float scale) {
    a.type_k = type_k; a.type_v = type_v; a.T = (int)T; a.H = H; a.G = G; a.D = D; a.n_ctx = n_cells; a.n_kv_max = n_cells; a.scale = scale;
}
// ... and the staged inputs
inline void attn_inputs(AttnArgs &a, const TestKVCache &c, int64_t T, int H, float scale, float *q, float *out, const AttnTables &tb) {
    attn_shape(a, c.type_k, c.type_v, T, H, c.G, c.D, c.n_cells, scale);
    a.q = q; a.out = out; a.kv = c.view;
    a.cell_pos = tb.cell_pos; a.cell_seq = tb.cell_seq; a.tok_pos = tb.tok_pos; a.tok_seq = tb.tok_seq; a.n_kv_dev = tb.n_kv;
}

// The per-token chunk lists of a test entry's step, built by the function the runtime builds its own with (host/attn_chunks.h) and laid out as Context keeps
// them: [64][stride] lists, then [64] counts.  grid: the chunk slots the launch gets (a.splits).
struct ChunkLists {
    int32_t *dev = nullptr;
    int stride = 0, lmax = 0, grid = 0;
    void make(OpBufs &b, int n_kv, int n_cells, const int32_t *cell_pos, const uint64_t *cell_seq, const int32_t *tok_seq, int T) {
        stride = (n_cells + ATTN_CHUNK_CELLS - 1) / ATTN_CHUNK_CELLS;
        std::vector<int32_t> h((size_t)64 * (stride + 1), 0);
        lmax = build_attn_chunk_lists(n_kv, n_cells, [&](int i, int32_t &p, uint64_t &m) { p = cell_pos[i]; m = cell_seq[i]; }, tok_seq, T, stride, h.data(),
                                      h.data() + (size_t)64 * stride);
        grid = attn_chunk_grid(lmax, stride);
        dev = b.upload(h.data(), h.size() * 4);
    }
    void apply(AttnArgs &a) const {
        a.tok_chunks = dev; a.tok_nchunks = dev + (size_t)64 * stride; a.chunk_stride = stride;
        a.splits = grid;
    }
};

}  // namespace mi355
