// kv_state.hip — a sequence's KV cells between the cache planes and portable ggml-layout rows (kernels.h launch_kv_state_pack / launch_kv_state_unpack).
//
// The cache keeps every layer as head-major planes, the codes and the f16 block scales of a quantised type apart (KVLayerView).  The portable form of n cells is,
// per layer, K rows [n][n_head_kv * head_dim] and then V rows likewise, each row in the ggml layout of its cache type: halves, 34-byte q8_0 blocks or 18-byte q4_0
// blocks - what mi355_op_flash_attn takes.  Both directions are plain copies, one launch for all layers:
//
//   grid (ceil(n / tile), 2 * n_layer), 256 threads; workgroup (x, y) owns cells [x * tile, ..) of the list for layer y / 2, K (y even) or V (y odd).
//   Its rows are one contiguous run of the portable side.  The run is assembled in LDS as it lies in memory, placed at the run's own address modulo 16, so the
//   portable side is moved in aligned 16-byte vectors (2-byte accesses only on a run's ragged first and last vector) whatever the 34- or 18-byte stride does to the
//   rows' alignment.  The plane side is moved in 16-byte pieces of a block's codes - lanes run along a cell's heads row, and along consecutive cells where the list
//   has them - and 2-byte scales, neighbouring lanes on neighbouring blocks.
//
// Bytes per launch: n * n_layer * (row_bytes_k + row_bytes_v) read and the same written, nothing else but the cell list.  No atomics; a workgroup touches only the
// cells of its own tile, so unpack leaves every other byte of every plane as it was.  The cell list must hold indices in [0, n_ctx), for unpack all different.
#include "kernels.h"

namespace mi355 {
namespace {

struct SideGeom { int cb, sb; };                       // bytes of a 32-element block's codes and of its scale (0: the type has none)
__host__ __device__ inline SideGeom side_geom(int type) {
    return type == T_F16 ? SideGeom{64, 0} : type == T_Q8_0 ? SideGeom{32, 2} : SideGeom{16, 2};
}

struct KVStateArgs {
    const KVLayerView *layers;
    const int32_t *cells;
    uint8_t *rows;
    int n, tile, G, nb, n_ctx;                         // nb: 32-element blocks of a head
    int type_k, type_v;
    unsigned rb_k, rb_v;                               // bytes of a portable K / V row
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <bool PACK> __global__ __launch_bounds__(256) void kv_state_kernel(KVStateArgs a) {
    extern __shared__ u32x4 lds4[];
    uint16_t *lds2 = reinterpret_cast<uint16_t *>(lds4);
    const int layer = (int)blockIdx.y >> 1, side = (int)blockIdx.y & 1;
    const int t0 = (int)blockIdx.x * a.tile;
    const int nt = min(a.tile, a.n - t0);
    if (nt <= 0) return;
    const KVLayerView lv = a.layers[layer];
    uint8_t *codes = side ? lv.v : lv.k;
    uint16_t *scales = side ? lv.vd : lv.kd;
    const SideGeom sg = side_geom(side ? a.type_v : a.type_k);
    const unsigned rb = side ? a.rb_v : a.rb_k;
    const int bb = sg.cb + sg.sb, ppb = sg.cb / 16, nb = a.nb, G = a.G;
    uint8_t *run = a.rows + (size_t)layer * a.n * ((size_t)a.rb_k + a.rb_v) + (side ? (size_t)a.n * a.rb_k : 0) + (size_t)t0 * rb;
    const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(run) & 15), len = (unsigned)nt * rb;
    uint8_t *base16 = run - mis;
    const int n_slots = (int)((mis + len + 15) / 16);
    const int tid = (int)threadIdx.x;

    if (!PACK) {                                       // the run -> LDS, as it lies in memory
        for (int s = tid; s < n_slots; s += 256) {
            const unsigned lo = (unsigned)s * 16;
            if (lo >= mis && lo + 16 <= mis + len) lds4[s] = *reinterpret_cast<const u32x4 *>(base16 + lo);
            else
                for (unsigned off = lo; off < lo + 16; off += 2)
                    if (off >= mis && off < mis + len) lds2[off / 2] = *reinterpret_cast<const uint16_t *>(base16 + off);
        }
        __syncthreads();
    }
    // codes: 16-byte pieces, ordered (head, cell of the tile, piece of the head) - a cell's head is contiguous in its plane, and so are consecutive cells
    const int per_cell = nb * ppb, n_pieces = G * nt * per_cell;
    for (int i = tid; i < n_pieces; i += 256) {
        const int g = i / (nt * per_cell), r = i - g * (nt * per_cell), t = r / per_cell, q = r - t * per_cell, b = q / ppb, p = q - b * ppb;
        const int cell = a.cells[t0 + t];
        if ((unsigned)cell >= (unsigned)a.n_ctx) continue;
        uint8_t *pl = codes + (((size_t)g * a.n_ctx + cell) * nb + b) * sg.cb + p * 16;
        uint16_t *im = lds2 + (mis + (unsigned)t * rb + (unsigned)(g * nb + b) * bb + sg.sb + p * 16) / 2;
        if (PACK) {
            const u32x4 v = *reinterpret_cast<const u32x4 *>(pl);
#pragma unroll
            for (int k = 0; k < 4; k++) { im[2 * k] = (uint16_t)(v[k] & 0xffff); im[2 * k + 1] = (uint16_t)(v[k] >> 16); }
        } else {
            u32x4 v;
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = (unsigned)im[2 * k] | ((unsigned)im[2 * k + 1] << 16);
            *reinterpret_cast<u32x4 *>(pl) = v;
        }
    }
    if (sg.sb) {
        const int n_sc = G * nt * nb;
        for (int i = tid; i < n_sc; i += 256) {
            const int g = i / (nt * nb), r = i - g * (nt * nb), t = r / nb, b = r - t * nb;
            const int cell = a.cells[t0 + t];
            if ((unsigned)cell >= (unsigned)a.n_ctx) continue;
            uint16_t *pl = scales + ((size_t)g * a.n_ctx + cell) * nb + b;
            uint16_t *im = lds2 + (mis + (unsigned)t * rb + (unsigned)(g * nb + b) * bb) / 2;
            if (PACK) *im = *pl; else *pl = *im;
        }
    }
    if (PACK) {                                        // LDS -> the run
        __syncthreads();
        for (int s = tid; s < n_slots; s += 256) {
            const unsigned lo = (unsigned)s * 16;
            if (lo >= mis && lo + 16 <= mis + len) *reinterpret_cast<u32x4 *>(base16 + lo) = lds4[s];
            else
                for (unsigned off = lo; off < lo + 16; off += 2)
                    if (off >= mis && off < mis + len) *reinterpret_cast<uint16_t *>(base16 + off) = lds2[off / 2];
        }
    }
}

bool kv_type_ok(int t) { return t == T_F16 || t == T_Q8_0 || t == T_Q4_0; }

template <bool PACK>
hipError_t launch(const KVLayerView *layers_dev, int n_layer, int type_k, int type_v, int G, int D, int n_ctx, const int32_t *cells_dev, int n, uint8_t *rows, hipStream_t st) {
    if (!layers_dev || !cells_dev || !rows || n_layer < 1 || n_layer > 32767 || G < 1 || D < 32 || D % 32 || n_ctx < 1 || n < 0 || !kv_type_ok(type_k) || !kv_type_ok(type_v))
        return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    KVStateArgs a{};
    a.layers = layers_dev; a.cells = cells_dev; a.rows = rows;
    a.n = n; a.G = G; a.nb = D / 32; a.n_ctx = n_ctx; a.type_k = type_k; a.type_v = type_v;
    const size_t rbk = kv_state_row_bytes(type_k, G, D), rbv = kv_state_row_bytes(type_v, G, D), rb_max = rbk > rbv ? rbk : rbv;
    if (rb_max + 32 > 64 * 1024) return hipErrorInvalidValue;                     // (a row must fit the workgroup's LDS: n_head_kv * head_dim <= 32736 halves)
    a.rb_k = (unsigned)rbk; a.rb_v = (unsigned)rbv;
    a.tile = kv_state_tile_cells(type_k, type_v, G, D);
    const size_t lds = ((size_t)a.tile * rb_max + 15 + 16) & ~(size_t)15;         // the image starts at the run's address modulo 16
    dim3 grid((unsigned)((n + a.tile - 1) / a.tile), (unsigned)(2 * n_layer));
    hipLaunchKernelGGL(kv_state_kernel<PACK>, grid, dim3(256), lds, st, a);
    return hipGetLastError();
}

}  // namespace

size_t kv_state_row_bytes(int type, int G, int D) {
    const SideGeom sg = side_geom(type);
    return (size_t)G * (size_t)(D / 32) * (size_t)(sg.cb + sg.sb);
}

int kv_state_tile_cells(int type_k, int type_v, int G, int D) {
    const size_t rbk = kv_state_row_bytes(type_k, G, D), rbv = kv_state_row_bytes(type_v, G, D), rb_max = rbk > rbv ? rbk : rbv;
    const size_t t = rb_max ? (size_t)16384 / rb_max : 64;                        // about 16 KB of rows per workgroup
    return (int)(t < 1 ? 1 : t > 64 ? 64 : t);
}

hipError_t launch_kv_state_pack(const KVLayerView *layers_dev, int n_layer, int type_k, int type_v, int G, int D, int n_ctx, const int32_t *cells_dev, int n, uint8_t *rows,
                                hipStream_t st) {
    return launch<true>(layers_dev, n_layer, type_k, type_v, G, D, n_ctx, cells_dev, n, rows, st);
}

hipError_t launch_kv_state_unpack(const KVLayerView *layers_dev, int n_layer, int type_k, int type_v, int G, int D, int n_ctx, const int32_t *cells_dev, int n,
                                  const uint8_t *rows, hipStream_t st) {
    return launch<false>(layers_dev, n_layer, type_k, type_v, G, D, n_ctx, cells_dev, n, const_cast<uint8_t *>(rows), st);
}

}  // namespace mi355
