// enc_eci.h -- Event Count Image: EciParams, k_eci_tile (general path), k_eci_scan (one launch for small calls).
// Expects enc_tile.h (Owner, CPT).  Integer counts by LDS atomics (order-free), table epilogue.
#pragma once
#include "enc_tile.h"

namespace {
struct EciParams {
    int H, W, twl, tiles_x;
    float lut[21]; // value * 255 after n sequential +0.05f adds, clamped (n >= 20 -> 255)
    float *out_f32;
    uint8_t *out_u8;
};

template <int NT>
__global__ __launch_bounds__(NT) void k_eci_tile(const uint2 *rec, const uint32_t *base, EciParams q)
{
    constexpr int NC = NT * CPT;
    __shared__ uint32_t cnt[NC];
    const int t = threadIdx.x, tile = blockIdx.x;
#pragma unroll
    for (int j = 0; j < CPT; ++j) cnt[t + NT * j] = 0;
    __syncthreads();
    const uint32_t beg = base[tile], end = base[tile + 1];
    for (uint32_t i = beg + t; i < end; i += NT) atomicAdd(&cnt[rec[i].x & (NC - 1)], 1u);
    __syncthreads();
    const TileGeom g = tile_geom(tile, q.tiles_x, q.twl, q.H, q.W);
    const Owner<CPT> ow = make_owner<NT, CPT>(g, q.W, 0);
    const long long plane = (long long)q.H * q.W;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        if (ow.ok[j]) {
            const uint32_t n = cnt[t + NT * j];
            const float v = q.lut[n > 20u ? 20u : n];
            const long long idx = ow.p * plane + ow.pix[j];
            if (q.out_f32) q.out_f32[idx] = v;
            if (q.out_u8) q.out_u8[idx] = f32_to_u8(v);
        }
    }
}

// Small calls (BASELINE.json configs[0]: 100 000 events on 304x240): the five launches of the general path -- histogram, two
// scans, scatter, tile kernel -- are 29 us of launch chain for 1.4 MB of data.  A count image needs no order at all: ONE launch in
// which every workgroup owns 2048 consecutive pixels (4096 counters in LDS), reads the WHOLE event array (0.8 MB out of the L2,
// 36 workgroups at 304x240) and counts the events that fall into its stretch; the 21-entry table turns the counts into the
// image.  The first workgroup also owns the call's status.  Used while events x workgroups stays small (frlw_eci_encode).
constexpr int kEciScanPix = 2048, kEciScanThreads = 1024;
template <bool HAS_MAP>
__global__ __launch_bounds__(kEciScanThreads) void k_eci_scan(const uint2 *data, long long n, const uint16_t *xmap, const uint16_t *ymap,
                                                              int map_w, int map_h, EciParams q, WsHeader *hdr)
{
    __shared__ uint32_t cnt[2 * kEciScanPix];
    __shared__ int serr;
    const int t = threadIdx.x;
    for (int i = t; i < 2 * kEciScanPix; i += kEciScanThreads) cnt[i] = 0u;
    if (t == 0) serr = 0;
    __syncthreads();
    const long long total = (long long)q.H * q.W; // (< 2^31: the host checks)
    const long long p0 = (long long)blockIdx.x * kEciScanPix;
    const bool check_status = blockIdx.x == 0;
    int err = 0;
    constexpr int RU = 16; // clamped loads in flight per thread, masked below (a workgroup's pass over the array is a chain of
                           // dependent iterations: with four loads per iteration 100 000 events took 25 round trips, 21 us)
    for (long long i0 = 0; i0 < n; i0 += RU * kEciScanThreads) {
        uint2 r[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const long long i = i0 + (long long)u * kEciScanThreads + t;
            r[u] = data[i < n ? i : n - 1];
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const bool live = i0 + (long long)u * kEciScanThreads + t < n;
            int x = (int)(r[u].y & 16383u), y = (int)((r[u].y >> 14) & 16383u);
            const uint32_t p = (r[u].y >> 28) & 1u;
            bool ok = live;
            if (HAS_MAP) {
                ok = ok && x < map_w && y < map_h;
                x = xmap[x < map_w ? x : 0];
                y = ymap[y < map_h ? y : 0];
            }
            // the reference indexes the flat cell 2 x + 2 W y + p (generate_eventcountimage.py:32): x >= W aliases into the next
            // row, only a flat pixel outside the frame raises.  (The range test below drops such an event in every workgroup; the
            // STATUS is the first workgroup's business alone: 36 workgroups repeat this loop, every instruction counts.)
            const uint32_t flat = (uint32_t)x + (uint32_t)q.W * (uint32_t)y, loc = flat - (uint32_t)p0;
            if (check_status && live && (!ok || flat >= (uint32_t)total)) err |= ST_INDEX;
            if (ok && loc < (uint32_t)kEciScanPix && flat < (uint32_t)total) atomicAdd(&cnt[(loc << 1) | p], 1u);
        }
    }
    if (err) atomicOr(&serr, err);
    __syncthreads();
    if (blockIdx.x == 0 && t == 0) { // every workgroup has seen every event: the first one speaks for the call
        hdr->status = serr;
        fold_sticky_status(hdr, serr);
    }
    for (int i = t; i < 2 * kEciScanPix; i += kEciScanThreads) {
        const int pol = i >= kEciScanPix ? 1 : 0;
        const long long pix = p0 + (i - pol * kEciScanPix);
        if (pix >= total) continue;
        const uint32_t c = cnt[((uint32_t)(i - pol * kEciScanPix) << 1) | (uint32_t)pol];
        const float v = q.lut[c > 20u ? 20u : c];
        const long long idx = (long long)pol * total + pix; // view (H, W, 2) -> permute (2, H, W), :36
        if (q.out_f32) q.out_f32[idx] = v;
        if (q.out_u8) q.out_u8[idx] = f32_to_u8(v);
    }
}
} // namespace
