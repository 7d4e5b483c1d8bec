// enc_ev.h -- Event Volume: EvParams, the tile body and its two kernels (k_ev_tile5 for up to five bins, k_ev_tile for up to kMaxK).
// Expects enc_tile.h (Owner, slice_sort, segments_order, the hot-tile list).  Exact f32 sums in stream order per cell.
#pragma once
#include "enc_tile.h"

namespace {
struct EvParams {
    int H, W, twl, tiles_x, bins;
    const WsHeader *hdr;
    float *out_f32;
    uint8_t *out_u8;
};

template <int NT, int C, int BINS>
__device__ __forceinline__ void ev_tile_body(const uint2 *rec, const uint32_t *base, const EvParams &q, int tile, int j0,
                                             uint32_t *cnt, uint2 *slot, uint32_t *red)
{
    constexpr int SLICE = slice_records(NT);
    const uint32_t beg = base[tile], end = base[tile + 1];
    float acc[C][BINS]; // cell (pixel, polarity) x time bin (BINS = 5 for the recipe's five bins, else kMaxK)
#pragma unroll
    for (int j = 0; j < C; ++j)
#pragma unroll
        for (int k = 0; k < BINS; ++k) acc[j][k] = 0.0f;
    const float binsf = (float)q.bins;
    for (uint32_t s0 = beg; s0 < end; s0 += SLICE) {
        const uint32_t span = end - s0 < (uint32_t)SLICE ? end - s0 : (uint32_t)SLICE;
        uint32_t c[C], o[C];
        slice_sort<NT, C>(rec, s0, span, [=](uint32_t m) { return local_cell<NT, C>(m, j0); }, cnt, slot, red, c, o);
        segments_order<C>(c, o, slot, SLICE - 1);
        uint32_t maxc = 0;
#pragma unroll
        for (int j = 0; j < C; ++j) maxc = c[j] > maxc ? c[j] : maxc;
        for (uint32_t a = 0; a < maxc; ++a) {
            uint32_t tv[C];
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const uint32_t at = o[j] + a;
                tv[j] = slot[at < SLICE - 1 ? at : SLICE - 1].x;
            }
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const bool live = a < c[j];
                const float ts = binsf * __uint_as_float(tv[j]); // t* = bins * float(t), generate_eventvolume.py:23
#pragma unroll
                for (int k = 0; k < BINS; ++k) { // bins beyond q.bins are accumulated but never stored
                    const float d = (float)(k + 1) - ts;
                    const float w = 1.0f - fabsf(d); // :28; negative weights -> 0 (:29) = skipped
                    const float na = acc[j][k] + w;
                    acc[j][k] = (live && w > 0.0f) ? na : acc[j][k];
                }
            }
        }
        __syncthreads();
    }
    const TileGeom g = tile_geom(tile, q.tiles_x, q.twl, q.H, q.W);
    const Owner<C> ow = make_owner<NT, C>(g, q.W, j0);
    const long long plane = (long long)q.H * q.W;
    const int ch = ow.p ? 0 : 1; // weights [p, 1 - p]: channel 0 = p == 1
#pragma unroll
    for (int j = 0; j < C; ++j) {
        if (ow.ok[j]) {
#pragma unroll
            for (int k = 0; k < BINS; ++k) {
                if (k < q.bins) {
                    const float v = acc[j][k] / 5.0f * 255.0f; // generate_eventvolume.py:37
                    const long long idx = (long long)(2 * k + ch) * plane + ow.pix[j];
                    if (q.out_f32) q.out_f32[idx] = v;
                    if (q.out_u8) q.out_u8[idx] = f32_to_u8(v > 255.0f ? 255.0f : v);
                }
            }
        }
    }
}

// grid = 4 * kMaxHot + n_tiles: the four quarters of every listed hot tile, then one workgroup per tile
template <int NT, int BINS>
__device__ __forceinline__ void ev_tile_kernel(const uint2 *rec, const uint32_t *base, const EvParams &q, int n_tiles)
{
    __shared__ uint32_t cnt[NT * CPT];
    __shared__ uint2 slot[slice_records(NT)];
    __shared__ uint32_t red[32];
    if (n_tiles < 0) { // small frame (-n_tiles tiles): every tile as four quarters, grid = 4 * tiles
        ev_tile_body<NT, 1, BINS>(rec, base, q, (int)blockIdx.x >> 2, (int)blockIdx.x & 3, cnt, slot, red);
        return;
    }
    if ((int)blockIdx.x >= 4 * kMaxHot) {
        const int tile = (int)blockIdx.x - 4 * kMaxHot;
        if (tile_is_listed(q.hdr, base, tile)) return; // hot: left to its quarters
        ev_tile_body<NT, CPT, BINS>(rec, base, q, tile, 0, cnt, slot, red);
    } else { // the long-running workgroups come first in the grid
        int tile, quarter;
        if (!pick_quarter(q.hdr, (int)blockIdx.x, tile, quarter)) return;
        ev_tile_body<NT, 1, BINS>(rec, base, q, tile, quarter, cnt, slot, red);
    }
}
// (two instantiations: the recipe's five bins keep five accumulators per cell instead of eight -- the loop over the bins is the
// kernel's VALU work)
template <int NT>
__global__ __launch_bounds__(NT) void k_ev_tile(const uint2 *rec, const uint32_t *base, EvParams q, int n_tiles)
{ ev_tile_kernel<NT, kMaxK>(rec, base, q, n_tiles); }
template <int NT>
__global__ __launch_bounds__(NT) void k_ev_tile5(const uint2 *rec, const uint32_t *base, EvParams q, int n_tiles)
{ ev_tile_kernel<NT, 5>(rec, base, q, n_tiles); }
} // namespace
