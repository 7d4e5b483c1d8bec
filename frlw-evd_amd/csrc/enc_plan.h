// enc_plan.h -- the general path's host planner: tuning knobs, Plan / make_plan (tiles, chunks, workspace layout), the scatter's LDS sizes, the tile grid, the ECI table.
// Expects nothing: no HIP header, no HIP type (tests/host/enc_plan_check.cpp builds it with the host compiler alone).
#pragma once
#include "frlw_consts.h"
#include "frlw_evd.h"
#include <stdint.h>

namespace frlw {
// One knob of the caller's frlw_tuning_t: a field that lies outside the caller's `struct_size` (an older header) or is
// negative takes the default.
inline int tuning_knob(const frlw_tuning_t *tu, int32_t frlw_tuning_t::*f, int dflt)
{
    if (!tu) return dflt;
    const size_t end = (size_t)((const char *)&(tu->*f) - (const char *)tu) + sizeof(int32_t);
    if ((size_t)tu->struct_size < end) return dflt;
    const int v = (int)(tu->*f);
    return v >= 0 ? v : dflt;
}
inline bool tuning_valid(const frlw_tuning_t *tu) { return !tu || (tu->struct_size >= 8 && tu->struct_size <= 4096); }

struct Plan {
    int twl, tiles_x, tiles_y, n_tiles;
    int bpw;          // batches of 64 events per wavefront
    long long chunk;  // events per partition workgroup = 1024 * bpw
    int units, slabs; // partition workgroups, slabs of 32
    unsigned hot_thr; // a tile with more records than this is shared by several workgroups (EV / TAF)
    int staged;       // < 0: by size
    int quarter_below, no_lut;
    size_t off_counts, off_slabtot, off_base, off_errs, off_tlut, off_records, bytes;
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

inline bool make_plan(long long n, int H, int W, const frlw_tuning_t *tuning, Plan &p)
{
    if (H <= 0 || W <= 0 || n < 0) return false;
    const auto knob = [&](int32_t frlw_tuning_t::*f, int dflt) { return tuning_knob(tuning, f, dflt); };
    p.twl = knob(&frlw_tuning_t::tile_width_log2, W > 512 ? 8 : 6);
    if (p.twl < 6 || p.twl > 8) return false;
    for (;; ++p.twl) { // tall frames (a batch of sequences stacked along y): widen the tiles to stay under kMaxTiles
        const int tw = 1 << p.twl;
        p.tiles_x = (W + tw - 1) / tw;
        p.tiles_y = (H + kTileH - 1) / kTileH;
        p.n_tiles = p.tiles_x * p.tiles_y;
        if (p.n_tiles <= kMaxTiles || p.twl == 8) break;
    }
    if (p.n_tiles > kMaxTiles) return false;
    // Workgroup chunk = kPartThreads * bpw events.  32 / kPartWaves partition workgroups fit on a CU, i.e.
    // `slots` at a time on the chip: pick bpw so that the workgroup count lands just under a multiple of
    // `slots` (whole rounds) with the longest chunk (= longest contiguous run per tile) that allows.
    const long long slots = 256ll * (32 / kPartWaves);
    int bpw = kMaxBpw;
    for (int rounds = 1; rounds <= 64; ++rounds) {
        const long long want = (n + slots * rounds * kPartThreads - 1) / (slots * rounds * kPartThreads);
        if (want <= kMaxBpw) { bpw = (int)(want < 1 ? 1 : want); break; }
    }
    p.bpw = knob(&frlw_tuning_t::batches_per_wave, bpw);
    if (p.bpw < 1 || p.bpw > kMaxBpw) return false;
    p.chunk = (long long)kPartThreads * p.bpw;
    p.units = (int)((n + p.chunk - 1) / p.chunk);
    if (p.units < 1) p.units = 1;
    p.slabs = (p.units + kSlabUnits - 1) / kSlabUnits;
    size_t off = kHeaderBytes;
    p.off_counts = off;  off = align_up(off + (size_t)p.units * p.n_tiles * 4, 256);
    p.off_slabtot = off; off = align_up(off + (size_t)p.slabs * p.n_tiles * 4, 256);
    p.off_base = off;    off = align_up(off + (size_t)(p.n_tiles + 1) * 4, 256);
    p.off_errs = off;    off = align_up(off + (size_t)p.units * 4, 256);
    p.off_tlut = off;    off = align_up(off + (size_t)(kMaxTlut + 1) * 4, 256);
    p.off_records = off; off = align_up(off + (size_t)(n > 0 ? n : 1) * 8, 256);
    p.bytes = off;
    // more than two slices and more than 4x the mean: worth sharing (frlw_tuning_t::hot_tile_records: tests force it)
    const long long slice2 = 2ll * kSliceMult * (4 << p.twl), mean4 = 4 * (n / p.n_tiles);
    const long long thr = slice2 > mean4 ? slice2 : mean4;
    p.hot_thr = (unsigned)knob(&frlw_tuning_t::hot_tile_records, thr > 0x7fffffffll ? 0x7fffffff : (int)thr);
    p.staged = knob(&frlw_tuning_t::staged_scatter, -1);
    p.quarter_below = knob(&frlw_tuning_t::quarter_below, 1024);
    p.no_lut = knob(&frlw_tuning_t::no_value_table, 0);
    return true;
}

// ---- k_scatter's dynamic LDS: gs[n_tiles] u32 | wcnt[16][n_tiles] u16 | tag[16][n_tiles] u8; the staged form adds behind them,
// at stage_off (16-aligned), loff[n_tiles + 2] u32 | stage[kStageCap] uint2 | stile[kStageCap] u16
constexpr int kStageCap = 4096; // records staged in LDS per write-out window of the staged scatter
constexpr size_t stage_off(int n_tiles)
{
    const size_t nt2 = (size_t)((n_tiles + 1) & ~1);
    return ((size_t)n_tiles * 4 + (size_t)kPartWaves * nt2 * 2 + (size_t)kPartWaves * n_tiles + 15) & ~(size_t)15;
}
struct ScatterLds { size_t hist, direct, staged_bytes; bool staged; }; // bytes for k_hist and k_scatter's two forms; which form runs
inline ScatterLds scatter_lds(const Plan &p, long long n)
{
    const size_t nt = (size_t)p.n_tiles, nt2 = (nt + 1) & ~(size_t)1;
    ScatterLds l = {nt * 4, nt * 4 + kPartWaves * nt2 * 2 + kPartWaves * nt + 16,
                    stage_off(p.n_tiles) + ((nt + 2 + 1) & ~(size_t)1) * 4 + (size_t)kStageCap * 8 + (size_t)kStageCap * 2 + 16, false};
    // staged write-out pays off for long streams with long chunks (10 M events: -11 us); on short ones the extra
    // barriers cost more than the write traffic saves (GEN1-shaped 1 M events: 66 -> 74 us).
    // frlw_tuning_t::staged_scatter forces it.
    l.staged = (p.staged >= 0 ? p.staged != 0 : (p.bpw >= 4 && n >= 3000000)) && l.staged_bytes <= 150 * 1024;
    return l;
}

// ---- the grid of the Event Volume / TAF tile kernels: the four quarters of every listed hot tile in front of the per-tile
// workgroups (skew).  A frame whose tiles do not even give every SIMD of the chip one wavefront (GEN1: 150 tiles x 4 wavefronts
// on 1024 SIMDs) runs ALL its tiles as quarters: four times the wavefronts, one cell per thread, each quarter streaming its tile.
struct TileGrid { bool all_quarters; int blocks, n_tiles_arg; }; // n_tiles_arg = the kernels' n_tiles: negative = all quarters
inline TileGrid tile_grid(const Plan &p)
{
    const bool q = p.n_tiles * ((4 << p.twl) / kWave) <= p.quarter_below;
    return {q, q ? p.n_tiles * 4 : p.n_tiles + kMaxHot * 4, q ? -p.n_tiles : p.n_tiles};
}

// The Event Count Image's table, generate_eventcountimage.py:32-34,41: n sequential f32 adds of 0.05f, > 1 -> 1, * 255
inline void eci_lut(float (&lut)[21])
{
    volatile float acc = 0.0f;
    lut[0] = 0.0f;
    for (int n = 1; n <= 20; ++n) {
        acc = acc + 0.05f;
        float v = acc;
        lut[n] = (v > 1.0f ? 1.0f : v) * 255.0f;
    }
}
} // namespace frlw
