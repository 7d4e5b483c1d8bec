// enc_tile.h -- what the tile kernels share: a thread's cells (Owner), the hot-tile list, the slice counting sort and its ordering pass.
// Expects frlw_common.h (WsHeader, TileGeom, wave_incl_scan, the constants).
#pragma once
#include "frlw_common.h"

namespace {
using namespace frlw;

constexpr int CPT = kCellsPerThread;

template <int C> struct Owner { // the C cells of thread t in a tile of NT threads
    int row[C];  // tile row of cell j
    int lx, p;   // pixel column inside the tile, polarity
    bool ok[C];
    long long pix[C]; // y * W + x
};

// Cell c = t + NT * j = (row << (twl + 1)) | (lx << 1) | p with a row of NT / 2 cells.  A whole-tile workgroup
// owns j = 0..3 (C = 4, j0 = 0); a quarter workgroup of a hot tile owns the single j = j0 (C = 1).
template <int NT, int C>
__device__ __forceinline__ Owner<C> make_owner(const TileGeom &g, int W, int j0)
{
    constexpr int RL = NT / 2;
    Owner<C> o;
    const int t = threadIdx.x;
    const int within = t & (RL - 1);
    o.lx = within >> 1;
    o.p = within & 1;
#pragma unroll
    for (int j = 0; j < C; ++j) {
        o.row[j] = 2 * (j0 + j) + (t >= RL ? 1 : 0);
        o.ok[j] = o.lx < g.nx && o.row[j] < g.ny;
        o.pix[j] = (long long)(g.y0 + o.row[j]) * W + g.x0 + o.lx;
    }
    return o;
}

// ---- skew: hot tiles ---------------------------------------------------------------------------------
// k_tilescan lists up to kMaxHot tiles that hold more than hot_thr records.  Their per-tile workgroups do
// nothing; 4 * kMaxHot workgroups in front of them in the grid give each listed tile to four workgroups of NT threads with ONE cell
// per thread (quarter q = the cells t + NT * q), i.e. four times the lanes on the per-cell sequential sums.
// Each quarter streams the tile's whole record list and keeps only its own cells.
__device__ __forceinline__ bool tile_is_listed(const WsHeader *hdr, const uint32_t *base, int tile)
{
    if (base[tile + 1] - base[tile] <= hdr->hot_thr) return false;
    const uint32_t n_hot = hdr->n_hot < (uint32_t)kMaxHot ? hdr->n_hot : (uint32_t)kMaxHot;
    for (uint32_t h = 0; h < n_hot; ++h) // more than kMaxHot hot tiles: the unlisted ones stay whole
        if ((int)hdr->hot[h] == tile) return true;
    return false;
}

__device__ __forceinline__ bool pick_quarter(const WsHeader *hdr, int idx, int &tile, int &quarter)
{
    const int h = idx >> 2;
    const uint32_t n_hot = hdr->n_hot < (uint32_t)kMaxHot ? hdr->n_hot : (uint32_t)kMaxHot;
    if ((uint32_t)h >= n_hot) return false;
    tile = (int)hdr->hot[h];
    quarter = idx & 3;
    return true;
}

#ifdef FRLW_TILE_PROF
// Developer build only (-DFRLW_TILE_PROF): per-phase cycle sums of the TAF tile kernel, thread 0 of each tile.
__device__ unsigned long long g_prof[16];
#define PROF_MARK(ph) do { const unsigned long long now_ = __builtin_readcyclecounter(); \
        if (threadIdx.x == 0) atomicAdd(&g_prof[ph], now_ - prof_t_); prof_t_ = now_; } while (0)
#define PROF_BEGIN unsigned long long prof_t_ = __builtin_readcyclecounter()
#define PROF_RESET prof_t_ = __builtin_readcyclecounter()
#else
#define PROF_MARK(ph) do { } while (0)
#define PROF_BEGIN do { } while (0)
#define PROF_RESET do { } while (0)
#endif

// ---- slice counting sort shared by EV and TAF --------------------------------------------------
// Sorts the records i in [s0, s0 + span) that `sel` maps to a local cell (sel(meta) >= 0; local cell =
// t + NT * j, j < C) by cell into slot[]; returns through (c[j], o[j]) the length and offset of the segments of
// this thread's C cells.  `cnt` has NT * C entries.
constexpr int kBatch = 8; // global loads in flight per thread in the two passes of slice_sort
// a slot is {value bits, position in the slice << 8 | window}: the widest slice's positions fit 24 bits, a window fits 8
static_assert(kSliceMult * 1024 <= (1 << 24) && FRLW_MAX_WINDOWS <= 256, "slice_sort's slot word");
template <int NT, int C, typename Sel>
__device__ __forceinline__ void slice_sort(const uint2 *rec, uint32_t s0, uint32_t span, Sel sel, uint32_t *cnt,
                                           uint2 *slot, uint32_t *red, uint32_t (&c)[C], uint32_t (&o)[C], int cb = 0)
{
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    constexpr int NW = NT / kWave;
    PROF_BEGIN;
#pragma unroll
    for (int j = 0; j < C; ++j) cnt[t + NT * j] = 0;
    __syncthreads();
    // batches of kBatch loads in flight per thread
    for (uint32_t i0 = s0 + t; i0 < s0 + span; i0 += kBatch * NT) {
        uint32_t m[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const uint32_t i = i0 + u * NT;
            m[u] = i < s0 + span ? rec[i].x : 0u;
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int cell = sel(m[u]);
            if (i0 + u * NT < s0 + span && cell >= 0) atomicAdd(&cnt[cell], 1u);
        }
    }
    __syncthreads();
    PROF_MARK(1);
    // exclusive scan in thread-major order: a thread's segments are adjacent
    uint32_t tot = 0;
#pragma unroll
    for (int j = 0; j < C; ++j) { c[j] = cnt[t + NT * j]; tot += c[j]; }
    const uint32_t inc = wave_incl_scan(tot);
    if (lane == kWave - 1) red[16 + wv] = inc;
    __syncthreads();
    uint32_t run = inc - tot;
    for (int k = 0; k < wv && k < NW; ++k) run += red[16 + k];
#pragma unroll
    for (int j = 0; j < C; ++j) { o[j] = run; cnt[t + NT * j] = run; run += c[j]; }
    __syncthreads();
    PROF_MARK(2);
    // Rounds of NT records with a barrier in between: slots of a later round always come after those
    // of an earlier one, so a cell's segment is out of order only among the few records of one round.
    for (uint32_t g0 = s0; g0 < s0 + span; g0 += kBatch * NT) {
        uint2 r[kBatch]; // the loads of kBatch rounds are issued together
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const uint32_t i = g0 + u * NT + t;
            r[u] = i < s0 + span ? rec[i] : make_uint2(0u, 0u);
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            if (g0 + u * NT >= s0 + span) break; // block-uniform
            const uint32_t i = g0 + u * NT + t;
            const int cell = sel(r[u].x);
            if (i < s0 + span && cell >= 0) {
                const uint32_t sl = atomicAdd(&cnt[cell], 1u);
                // one 8-byte LDS entry per record: {value bits, position in the slice << 8 | window}
                slot[sl] = make_uint2(r[u].y, ((i - s0) << 8) | ((r[u].x >> cb) & 255u));
            }
            __syncthreads();
        }
    }
    PROF_MARK(3);
}

// Slots were handed out by LDS atomics in arrival order; restore stream order inside the C segments
// of this thread.  Only records of the same round (NT consecutive records) can be swapped, so a segment
// is a run of tiny permuted blocks -- nearly always pairs.  One bubble pass, the cells in lock-step
// (independent LDS reads in flight per step, selects instead of branches), repairs every adjacent inversion;
// a segment it cannot repair (an element that has to move two or more places: three or more records of
// one pixel within NT events) is finished by an insertion sort afterwards.
template <int C>
__device__ __forceinline__ void segments_order(const uint32_t (&c)[C], const uint32_t (&o)[C], uint2 *slot,
                                               uint32_t last_slot)
{
    uint32_t maxc = 0, below[C];
    uint2 top[C]; // largest element so far = what slot[o + x - 1] holds
    bool deep[C];
#pragma unroll
    for (int j = 0; j < C; ++j) {
        maxc = c[j] > maxc ? c[j] : maxc;
        top[j] = make_uint2(0u, 0u);
        below[j] = 0u;
        deep[j] = false;
    }
    for (uint32_t x = 0; x < maxc; ++x) {
        uint2 e[C];
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const uint32_t at = o[j] + x;
            e[j] = slot[at < last_slot ? at : last_slot];
        }
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const bool live = x < c[j];
            const bool inv = live && e[j].y < top[j].y; // .y orders by position in the slice
            const bool fwd = live && !inv;
            deep[j] |= inv && e[j].y < below[j];
            if (inv) { // adjacent inversion: e goes under top
                slot[o[j] + x - 1] = e[j];
                slot[o[j] + x] = top[j];
            }
            below[j] = inv ? e[j].y : (fwd ? top[j].y : below[j]);
            top[j].x = fwd ? e[j].x : top[j].x;
            top[j].y = fwd ? e[j].y : top[j].y;
        }
    }
#pragma unroll
    for (int j = 0; j < C; ++j) {
        if (!deep[j]) continue;
        for (uint32_t x = 1; x < c[j]; ++x) {
            const uint2 e = slot[o[j] + x];
            uint32_t b = x;
            while (b > 0 && slot[o[j] + b - 1].y > e.y) { slot[o[j] + b] = slot[o[j] + b - 1]; --b; }
            slot[o[j] + b] = e;
        }
    }
}

// local cell of a record for a workgroup that owns the cells j0 .. j0 + C - 1 of every thread (-1: not ours)
template <int NT, int C>
__device__ __forceinline__ int local_cell(uint32_t meta, int j0)
{
    const int cell = (int)(meta & (uint32_t)(NT * kCellsPerThread - 1));
    if (C == kCellsPerThread) return cell;
    return (cell / NT) == j0 ? (cell & (NT - 1)) : -1;
}

constexpr int slice_records(int nt) { return kSliceMult * nt; } // records counting-sorted per pass by a tile of nt threads
} // namespace
