// enc_taf.h -- TAF: TafParams, the tile body (window-sorted fast loop, window-interleaved general loop, fused write-out), k_taf_tile
// and k_taf_tile_snap (the same body, which also writes a uint8 snapshot after chosen windows: frlw_taf_encode_chain).
// Expects enc_tile.h (Owner, slice_sort, segments_order, the hot-tile list), taf_fifo.h (the FIFO step) and leaky.h (the uint8 look-up).
#pragma once
#include "enc_tile.h"
#include "taf_fifo.h"

namespace {
struct TafParams {
    int H, W, twl, tiles_x, K, n_windows, flip;
    WsHeader *hdr;
    const uint32_t *leaky_thr; // level thresholds of uint8(leaky_transform(.)): the per-device table of leaky.hip
    float *state;    // (H, W, 2, K)
    float *view_f32; // (2K, H, W) or NULL
    uint8_t *out_u8; // (K, 2, H, W) or NULL
    unsigned long long emit_mask; // k_taf_tile_snap: bit w = a snapshot after window w
    uint8_t *snap_u8;             // k_taf_tile_snap: (popcount(emit_mask), K, 2, H, W), in window order
};

// SNAP: close_window(w) also writes the uint8 volume of the thread's cells into snapshot popcount(emit_mask below bit w) when bit
// w of emit_mask is set -- what the write-out would give if the call ended after window w.
template <int NT, int C, bool SNAP>
__device__ __forceinline__ void taf_tile_body(const uint2 *rec, const uint32_t *base, const TafParams &q, int tile,
                                              int j0, uint32_t *cnt, uint2 *slot, uint32_t *red, uint32_t *thr)
{
    constexpr int SLICE = slice_records(NT);
    const int t = threadIdx.x;
    const int K = q.K;
    for (int i = t; i < kLeakyLevels; i += NT) thr[i] = q.leaky_thr[i];
    __syncthreads(); // a tile without records reaches the write-out (which reads thr[]) without any other barrier
    const int cb = q.twl + 4; // cell bits
    const TileGeom g = tile_geom(tile, q.tiles_x, q.twl, q.H, q.W);
    const Owner<C> ow = make_owner<NT, C>(g, q.W, j0);
    const uint32_t beg = base[tile], end = base[tile + 1];
    const unsigned long long wmask = q.hdr->wmask; // windows that hold events (anywhere in the frame)
    float st[C][kMaxK], sum[C];
    uint32_t num[C];
    const auto sel = [=](uint32_t m) { return local_cell<NT, C>(m, j0); };

    auto load_state = [&]() {
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const float *src = q.state + (ow.pix[j] * 2 + ow.p) * K;
#pragma unroll
            for (int k = 0; k < kMaxK; ++k) st[j][k] = 0.0f;
            if (ow.ok[j]) {
                if (K == 8) {
                    const float4 a = ((const float4 *)src)[0], b = ((const float4 *)src)[1];
                    st[j][0] = a.x; st[j][1] = a.y; st[j][2] = a.z; st[j][3] = a.w;
                    st[j][4] = b.x; st[j][5] = b.y; st[j][6] = b.z; st[j][7] = b.w;
                } else {
#pragma unroll
                    for (int k = 0; k < kMaxK; ++k) if (k < K) st[j][k] = src[k];
                }
            }
            sum[j] = 0.0f;
            num[j] = 0u;
        }
    };
    // closes window w for the thread's cells: FIFO step (skipped when the window is empty in the whole
    // frame, generate_taf.py:40-41), accumulators back to zero.  SNAP: then the snapshot, if window w emits one (an empty
    // window emits too: the volume of the window before it)
    auto close_window = [&](int w) {
        const bool has = (wmask >> w) & 1ull;
#pragma unroll
        for (int j = 0; j < C; ++j) {
            if (has) fifo_step(st[j], K, true, num[j], fifo_mean(num[j], sum[j]));
            sum[j] = 0.0f;
            num[j] = 0u;
        }
        if constexpr (SNAP) {
            if ((q.emit_mask >> w) & 1ull) {
                const long long plane = (long long)q.H * q.W;
                uint8_t *dst = q.snap_u8 + (long long)__popcll(q.emit_mask & ((1ull << w) - 1ull)) * (2 * K) * plane;
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    if (!ow.ok[j]) continue;
                    // half a cell at a time: the look-up's guesses and table pairs of four slots are all that lives beside
                    // st[][] and the loop's counters (eight at once spill at NT = 1024, 128 VGPRs)
#pragma unroll
                    for (int k0 = 0; k0 < kMaxK; k0 += 4) {
                        const float v[4] = {st[j][k0], st[j][k0 + 1], st[j][k0 + 2], st[j][k0 + 3]};
                        uint8_t lv[4];
                        leaky_u8_lookup_n<4>(v, thr, lv);
#pragma unroll
                        for (int k = k0; k < k0 + 4; ++k) {
                            if (k < K) {
                                const int ko = q.flip ? (K - 1 - k) : k;
                                dst[(long long)(2 * ko + ow.p) * plane + ow.pix[j]] = lv[k - k0];
                            }
                        }
                    }
                }
            }
        }
    };

    // ---- fast path: the tile's records are window-sorted (always true for a time-sorted stream, the
    // partition being stable).  Slices of SLICE records, each counting-sorted by cell once, may span
    // several windows; the FIFO steps between them are block-uniform.
    PROF_BEGIN;
    load_state();
    bool bad = false;
    int cur_w = 0; // block-uniform: windows < cur_w are closed
    for (uint32_t s0 = beg; s0 < end; s0 += SLICE) {
        const uint32_t span = end - s0 < (uint32_t)SLICE ? end - s0 : (uint32_t)SLICE;
        const int wlo = (int)(rec[s0].x >> cb), whi = (int)(rec[s0 + span - 1].x >> cb);
        if (wlo < cur_w || whi < wlo || whi >= q.n_windows) { bad = true; break; }
        for (; cur_w < wlo; ++cur_w) close_window(cur_w);
        uint32_t c[C], o[C], a[C];
        PROF_MARK(0);
        slice_sort<NT, C>(rec, s0, span, sel, cnt, slot, red, c, o, cb);
        PROF_RESET;
        segments_order<C>(c, o, slot, SLICE - 1);
        PROF_MARK(4);
#pragma unroll
        for (int j = 0; j < C; ++j) a[j] = 0;
        for (int w = wlo; w <= whi; ++w) {
            // the cells advance together: one LDS read each per step, until none of them has a
            // record of window w next
            for (;;) {
                uint2 e[C];
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    const uint32_t at = o[j] + a[j];
                    e[j] = slot[at < SLICE - 1 ? at : SLICE - 1];
                }
                uint32_t any = 0u;
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    const bool take = a[j] < c[j] && (int)(e[j].y & 255u) == w;
                    const float nsum = sum[j] + __uint_as_float(e[j].x); // sum += t - 1 in stream order, generate_taf.py:26
                    sum[j] = take ? nsum : sum[j];
                    num[j] += take ? 1u : 0u;
                    a[j] += take ? 1u : 0u;
                    any |= take ? 1u : 0u;
                }
                if (!any) break;
            }
            if (w < whi) { close_window(w); cur_w = w + 1; }
        }
        PROF_MARK(5);
        bool viol = false; // a record whose window runs backwards inside its cell's segment
#pragma unroll
        for (int j = 0; j < C; ++j) viol |= a[j] != c[j];
        if (__syncthreads_or(viol)) { bad = true; break; }
        PROF_MARK(6);
    }
    if (!bad) {
        for (; cur_w < q.n_windows; ++cur_w) close_window(cur_w);
        PROF_MARK(7);
    } else {
        // ---- general path (stream not time-sorted): the state has not been written yet; the snapshots the abandoned loop
        // wrote (SNAP) are all written again below, every window being closed once more.  One pass per window over the whole
        // list, slices in list order, records selected by window.
        __syncthreads();
        if (t == 0) atomicAdd(&q.hdr->pad, 1u); // diagnostic: tiles on the general path
        load_state();
        for (int w = 0; w < q.n_windows; ++w) {
            for (uint32_t s0 = beg; s0 < end; s0 += SLICE) {
                const uint32_t span = end - s0 < (uint32_t)SLICE ? end - s0 : (uint32_t)SLICE;
                uint32_t c[C], o[C];
                slice_sort<NT, C>(rec, s0, span, [=](uint32_t m) { return (int)(m >> cb) == w ? sel(m) : -1; }, cnt, slot,
                                  red, c, o, cb);
                segments_order<C>(c, o, slot, SLICE - 1);
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    for (uint32_t x = 0; x < c[j]; ++x) sum[j] = sum[j] + __uint_as_float(slot[o[j] + x].x);
                    num[j] += c[j];
                }
                __syncthreads();
            }
            close_window(w);
        }
    }

    // ---- write-out: state, optional f32 view (2K, H, W), optional uint8 leaky transform
    const long long plane = (long long)q.H * q.W;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        if (!ow.ok[j]) continue;
        float *dst = q.state + (ow.pix[j] * 2 + ow.p) * K;
        if (K == 8) {
            ((float4 *)dst)[0] = make_float4(st[j][0], st[j][1], st[j][2], st[j][3]);
            ((float4 *)dst)[1] = make_float4(st[j][4], st[j][5], st[j][6], st[j][7]);
        } else {
#pragma unroll
            for (int k = 0; k < kMaxK; ++k) if (k < K) dst[k] = st[j][k];
        }
        if (q.view_f32) {
#pragma unroll
            for (int k = 0; k < kMaxK; ++k)
                if (k < K) q.view_f32[(long long)(2 * k + ow.p) * plane + ow.pix[j]] = st[j][k]; // :55
        }
        if (q.out_u8) {
            uint8_t lv[kMaxK];
            leaky_u8_lookup_n<kMaxK>(st[j], thr, lv); // the eight table look-ups in flight together
#pragma unroll
            for (int k = 0; k < kMaxK; ++k) {
                if (k < K) {
                    const int ko = q.flip ? (K - 1 - k) : k;
                    q.out_u8[(long long)(2 * ko + ow.p) * plane + ow.pix[j]] = lv[k];
                }
            }
        }
    }
    PROF_MARK(8);
}

// grid = 4 * kMaxHot + n_tiles: the four quarters of every listed hot tile, then one workgroup per tile
template <int NT>
__global__ __launch_bounds__(NT) void k_taf_tile(const uint2 *rec, const uint32_t *base, TafParams q, int n_tiles)
{
    __shared__ uint32_t cnt[NT * CPT];
    __shared__ uint2 slot[slice_records(NT)];
    __shared__ uint32_t red[48];
    __shared__ uint32_t thr[kLeakyLevels];
    if (n_tiles < 0) { // small frame (-n_tiles tiles): every tile as four quarters, grid = 4 * tiles
        taf_tile_body<NT, 1, false>(rec, base, q, (int)blockIdx.x >> 2, (int)blockIdx.x & 3, cnt, slot, red, thr);
        return;
    }
    if ((int)blockIdx.x >= 4 * kMaxHot) {
        const int tile = (int)blockIdx.x - 4 * kMaxHot;
        if (tile_is_listed(q.hdr, base, tile)) return; // hot: left to its quarters
        taf_tile_body<NT, CPT, false>(rec, base, q, tile, 0, cnt, slot, red, thr);
    } else { // the long-running workgroups come first in the grid
        int tile, quarter;
        if (!pick_quarter(q.hdr, (int)blockIdx.x, tile, quarter)) return;
        taf_tile_body<NT, 1, false>(rec, base, q, tile, quarter, cnt, slot, red, thr);
    }
}

// k_taf_tile with snapshots (frlw_taf_encode_chain): same grid, same three launch forms
template <int NT>
__global__ __launch_bounds__(NT) void k_taf_tile_snap(const uint2 *rec, const uint32_t *base, TafParams q, int n_tiles)
{
    __shared__ uint32_t cnt[NT * CPT];
    __shared__ uint2 slot[slice_records(NT)];
    __shared__ uint32_t red[48];
    __shared__ uint32_t thr[kLeakyLevels];
    if (n_tiles < 0) {
        taf_tile_body<NT, 1, true>(rec, base, q, (int)blockIdx.x >> 2, (int)blockIdx.x & 3, cnt, slot, red, thr);
        return;
    }
    if ((int)blockIdx.x >= 4 * kMaxHot) {
        const int tile = (int)blockIdx.x - 4 * kMaxHot;
        if (tile_is_listed(q.hdr, base, tile)) return;
        taf_tile_body<NT, CPT, true>(rec, base, q, tile, 0, cnt, slot, red, thr);
    } else {
        int tile, quarter;
        if (!pick_quarter(q.hdr, (int)blockIdx.x, tile, quarter)) return;
        taf_tile_body<NT, 1, true>(rec, base, q, tile, quarter, cnt, slot, red, thr);
    }
}
} // namespace
