// taf_decode.h -- a DAT record -> (bin, 4-byte record word, window): FastGeom, the workspace header, the decode functions.
// Expects frlw_common.h (ST_*, kSelftestOffset) and taf_plan.h (constants, SeqTab).
#pragma once
#include "frlw_common.h"
#include "taf_plan.h"

namespace {
using namespace frlw;
struct FastGeom {
    const uint2 *data;
    const uint16_t *xmap, *ymap;
    int map_w, map_h;
    int H, W, twl, thl, tiles_x, T;
    int bpw;      // batches of 64 events per wavefront of a partition workgroup = ceil(run / 64)
    int chunk_ev; // events per chunk (one scatter workgroup), a multiple of 16, <= 8192
    int run;      // events per wavefront of the scatter workgroup = chunk_ev / 16
    long long n_total; // records in the array (loads never go past it)
    int y_lo, H_full;  // row-stripe sharding of one frame: this call encodes rows [y_lo, y_lo + H) of an H_full-row frame; events
                       // of other rows are skipped (not an error); H_full == H, y_lo == 0: the whole frame
    int n_windows, wb;
    uint32_t win, win_magic;
    int bin_shift, bin_mask; // direct mode (FastPlan): bin = tile << 4 | sub-tile of the cell; otherwise 0, 0: bin = tile
    int simple;   // the call meets the conditions of the SIMPLE decode (below): decided on the host
    uint32_t span; // n_windows * win when that fits 32 bits (SIMPLE)
    int m24;      // SIMPLE and span < 2^24 and win_magic < 2^24 (win > 256): the window division of an in-span event fits the
                  // full-rate 24-bit multiplies (simple_taf_fields_valid); decided on the host
    double rcp; // 1 / (win + 1e-8) (TAF) or 1 / win (Event Volume), IEEE f64, computed ONCE on the host: kf_hist checks that
                // multiplying by it gives every r of the window the float the division gives; the tile kernels multiply
};

struct FastHeader {
    int32_t status; // ST_* flags; same offset as WsHeader::status (frlw_encoder_status reads it)
    uint32_t filtered_tiles; // diagnostic: sub-tiles whose records were not window-sorted (unsorted stream)
    unsigned long long wmask[kMaxSeq]; // bit w set <=> window w of the sequence holds at least one event
    uint32_t mul_bad; // != 0: float(r * (1 / den)) differs from float(r / den) for some r in [0, win]: use the table
    // chunk-major partition: where the next (sequence, tile) list goes in rec2[] / the next split segment id (the header is
    // zeroed by a memset node in front of kf_scatter_cm; placement order is whatever order the workgroups arrive in -- the
    // lists themselves, and everything computed from them, do not depend on it)
    uint32_t rec_cursor, seg_cursor;
    // kf_scatter_cm's first workgroup resets everything above and then publishes the call's epoch here; the other workgroups
    // touch the header only at their very end and only once they see that epoch (no memset node: 4.8 us of every call)
    uint32_t epoch;
};
static_assert(sizeof(FastHeader) <= kSelftestOffset, "header");

// ---- decode ----------------------------------------------------------------------------------------
struct FastEv {
    int tile;      // < 0: not encoded (err says why)
    uint32_t word; // r << (12 + wb) | window << 12 | cell
    uint32_t window;
    int err;
};

// src/io/dat_events_tools.py:96-98 (bit fields), generate_taf.py:197-203 (window), :215-219 (coordinate scaling via the
// maps); the flat index x + W * y of generate_taf.py:23 aliases x >= W into the next row like the general path.
// EV (Event Volume, generate_eventvolume.py:139-141): t0 = t_end - window; events with t <= t0 are dropped like the
// harness' `events_[:, 2] > end_time - time_window` filter, an event behind t_end is outside the contract (ST_SPAN);
// word = (t - t0) << 12 | cell, one "window".
// SIMPLE (chosen per call on the host, FastGeom::simple): whole frame (no row stripe), every sequence's t0 in [0, 2^32), the
// span n_windows * win below 2^32, win >= 2 -- then the time arithmetic is 32-bit, the stripe test disappears and the window
// needs ONE correction step after the multiply-high (floor(2^32 / win) under-estimates the quotient by less than one).  Same
// results as the general form on such calls; 14 of the decode's 52 VALU instructions less in kf_hist and kf_scatter.
// SAE (Surface of Active Events, generate_surfaceofactiveevents.py:72, :176-190; an EV-shaped decode): events outside the frame
// and events at or in front of t0 = now - window are dropped without an error, there is no upper time bound, and the record's
// time field is replaced by the caller with the event's position in its sequence (the consumer wants the LAST writer).
// SAE == 2 (Event Count Image, generate_eventcountimage.py:19-41): the Event Volume decode -- x >= W aliases into the next row,
// a flat pixel outside the frame is an error -- without any time bound (the host passes t0 = -1: every event is kept).
// The flat index x + W * y of generate_taf.py:23: x >= W aliases into the next row.  false: the flat pixel lies outside the frame.
__device__ __forceinline__ bool fast_alias(const FastGeom &G, int &x, int &y)
{
    if (x >= G.W || y >= G.H_full) {
        const long long flat = (long long)x + (long long)G.W * y;
        if (flat >= (long long)G.H_full * G.W) return false;
        y = (int)(flat / G.W);
        x = (int)(flat - (long long)y * G.W);
    }
    return true;
}

// The two halves of the SIMPLE TAF decode that do not depend on where the event's time lies.
// simple_cell: the cell inside the tile and the bin.  BINS = false: the caller knows bin_shift == 0 and bin_mask == 0 (tile bins).
// (y >> thl < tiles_y and tiles_x are both at most kMaxFastTiles: the 24-bit multiply of the tile row is exact.)
template <bool BINS = true>
__device__ __forceinline__ uint32_t simple_cell(const FastGeom &G, uint32_t x, uint32_t y, uint32_t p, uint32_t &tile)
{
    const uint32_t tw1 = (1u << G.twl) - 1u, th1 = (1u << G.thl) - 1u;
    const uint32_t cell = ((((y & th1) << G.twl) | (x & tw1)) << 1) | p;
    tile = __umul24(y >> G.thl, (uint32_t)G.tiles_x) + (x >> G.twl);
    if (BINS) tile = (tile << G.bin_shift) | ((cell >> 8) & (uint32_t)G.bin_mask);
    return cell;
}
// simple_window: z = floor(relu / win) and the remainder, by a multiply-high and ONE correction step (floor(2^32 / win)
// under-estimates the quotient by less than one).  M24: relu, win_magic and win are all below 2^24 (FastGeom::m24 and an
// in-span event), so the high and the low 32 bits of the 48-bit products are what the full-rate 24-bit multiplies give.
template <bool M24 = false>
__device__ __forceinline__ uint32_t simple_window(const FastGeom &G, uint32_t relu, uint32_t &rem)
{
    uint32_t z = M24 ? __umulhi(relu & 0xffffffu, G.win_magic & 0xffffffu) : __umulhi(relu, G.win_magic); // floor(rel / win) or one less
    uint32_t zw;
    if (M24) asm("v_mul_u32_u24 %0, %1, %2" : "=v"(zw) : "s"(G.win), "v"(z)); // (__umul24 here comes out as the quarter-rate v_mul_lo_u32)
    else zw = z * G.win;
    rem = relu - zw;
    if (rem >= G.win) { ++z; rem -= G.win; }
    return z;
}

// The SIMPLE TAF fields of an in-frame event at time t: window, tile (bin) and record word.  false: t is outside
// [t0, t0 + span] (ST_SPAN); the fields are computed either way, so a caller can select instead of branching (kf_scatter_cm).
template <bool BINS = true>
__device__ __forceinline__ bool simple_taf_fields(const FastGeom &G, int x, int y, uint32_t p, uint32_t t, uint32_t t0lo, uint32_t &tile,
                                                  uint32_t &word, uint32_t &window)
{
    const uint32_t relu = t - t0lo;
    uint32_t rem, z = simple_window(G, relu, rem);
    if (z >= (uint32_t)G.n_windows) { z = (uint32_t)G.n_windows - 1u; rem = G.win; } // t == end of the last window
    const uint32_t cell = simple_cell<BINS>(G, (uint32_t)x, (uint32_t)y, p, tile);
    window = z;
    word = (rem << (kCellBits + G.wb)) | (z << kCellBits) | cell;
    return !(t < t0lo || relu > G.span);
}

// The same fields of an event the caller KNOWS to be inside the frame and strictly inside the span (relu < span: the window
// is below n_windows without the clamp), of a call with tile bins and FastGeom::m24 -- kf_scatter_cm's all-valid batches.
__device__ __forceinline__ void simple_taf_fields_valid(const FastGeom &G, uint32_t x, uint32_t y, uint32_t p, uint32_t relu, uint32_t &tile,
                                                        uint32_t &word, uint32_t &window)
{
    uint32_t rem;
    const uint32_t z = simple_window<true>(G, relu, rem);
    const uint32_t cell = simple_cell<false>(G, x, y, p, tile);
    window = z;
    word = (rem << (kCellBits + G.wb)) | (z << kCellBits) | cell;
}

template <bool HAS_MAP, bool EV = false, bool SIMPLE = false, int SAE = 0>
__device__ __forceinline__ FastEv fast_decode(const FastGeom &G, uint2 r, long long t0)
{
    FastEv o;
    o.tile = -1; o.word = 0; o.window = 0; o.err = 0;
    int x = (int)(r.y & 16383u), y = (int)((r.y >> 14) & 16383u);
    const uint32_t p = (r.y >> 28) & 1u;
    if (HAS_MAP) {
        if (x >= G.map_w || y >= G.map_h) { o.err = ST_INDEX; return o; }
        x = G.xmap[x];
        y = G.ymap[y];
    }
    if (SAE == 1 && (x >= G.W || y >= G.H_full)) return o; // generate_surfaceofactiveevents.py:72
    if (!fast_alias(G, x, y)) { o.err = ST_INDEX; return o; }
    if (SIMPLE) {
        const uint32_t t0lo = (uint32_t)t0, relu = r.x - t0lo;
        if (EV) {
            if (r.x <= t0lo) return o; // generate_eventvolume.py:139: not an error, not encoded
            if (!SAE && relu > G.win) { o.err = ST_SPAN; return o; }
            const int tw1e = (1 << G.twl) - 1, th1e = (1 << G.thl) - 1;
            const uint32_t celle = (uint32_t)((((y & th1e) << G.twl) | (x & tw1e)) << 1) | p;
            o.tile = (((y >> G.thl) * G.tiles_x + (x >> G.twl)) << G.bin_shift) | (int)((celle >> 8) & (uint32_t)G.bin_mask);
            o.word = (relu << kCellBits) | celle;
            return o;
        }
        uint32_t tile, word, window; // (kf_scatter_cm's LEAN phase A calls the same two helpers without the early returns)
        if (!simple_taf_fields(G, x, y, p, r.x, t0lo, tile, word, window)) { o.err = ST_SPAN; return o; }
        o.tile = (int)tile;
        o.window = window;
        o.word = word;
        return o;
    }
    y -= G.y_lo; // row-stripe sharding: another rank owns the rows outside [y_lo, y_lo + H)
    if ((unsigned)y >= (unsigned)G.H) return o;
    const long long rel = (long long)r.x - t0;
    if (EV) {
        if (rel <= 0) return o; // generate_eventvolume.py:139: not an error, not encoded
        if (!SAE && rel > (long long)G.win) { o.err = ST_SPAN; return o; }
        const int tw1e = (1 << G.twl) - 1, th1e = (1 << G.thl) - 1;
        const uint32_t celle = (uint32_t)((((y & th1e) << G.twl) | (x & tw1e)) << 1) | p;
        o.tile = (((y >> G.thl) * G.tiles_x + (x >> G.twl)) << G.bin_shift) | (int)((celle >> 8) & (uint32_t)G.bin_mask);
        o.word = ((uint32_t)rel << kCellBits) | celle;
        return o;
    }
    if (rel < 0 || rel > (long long)G.n_windows * G.win) { o.err = ST_SPAN; return o; }
    const uint32_t relu = (uint32_t)rel;
    uint32_t z = __umulhi(relu, G.win_magic); // floor(rel / win) - {0, 1, 2}
    uint32_t rem = relu - z * G.win;
    if (rem >= G.win) { ++z; rem -= G.win; }
    if (rem >= G.win) { ++z; rem -= G.win; }
    if (z >= (uint32_t)G.n_windows) { z = (uint32_t)G.n_windows - 1u; rem = G.win; } // t == end of the last window
    const int tw1 = (1 << G.twl) - 1, th1 = (1 << G.thl) - 1;
    const uint32_t cell = (uint32_t)((((y & th1) << G.twl) | (x & tw1)) << 1) | p;
    o.tile = (((y >> G.thl) * G.tiles_x + (x >> G.twl)) << G.bin_shift) | (int)((cell >> 8) & (uint32_t)G.bin_mask);
    o.window = z;
    o.word = (rem << (kCellBits + G.wb)) | (z << kCellBits) | cell;
    return o;
}

// largest s with first[s] <= v (first[0] = 0; empty sequences repeat a value: the last of them wins, like a linear walk).
// Bisection: the table sits in the kernel arguments, every probe is a DEPENDENT scalar load -- the linear walk this replaces
// cost a 64-sequence call up to 64 of them per chunk and wavefront (66 M scalar instructions in kf_hist for 64 M events).
__device__ __forceinline__ int seq_of(const int *first, int n_seq, int v)
{
    int lo = 0, hi = n_seq;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (v >= first[mid]) lo = mid; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int seq_of_chunk(const SeqTab &S, int chunk) { return seq_of(S.chunk0, S.n_seq, chunk); }
} // namespace
