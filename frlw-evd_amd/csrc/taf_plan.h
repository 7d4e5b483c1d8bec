// taf_plan.h -- the host planner of the fast path (taf_fast.hip): tile shape, partition mode, chunk size, workspace layout, size query.
// Pure host arithmetic: NO HIP header and no HIP type, so tests/host/taf_plan_check.cpp runs it without a GPU.
// Expects nothing before it.
#pragma once
#include "frlw_consts.h"
#include "frlw_evd.h"
#include <stdint.h>

namespace {
using namespace frlw; // kWave, kMaxBpw, kHeaderBytes
constexpr int kFT = 1024;                 // threads of every workgroup here
constexpr int kFW = kFT / kWave;          // 16 wavefronts
constexpr int kCellBits = 12;
constexpr int kCells = 1 << kCellBits;    // cells (pixel x polarity) per tile
constexpr int kSubCells = kCells / kFW;   // 256 cells owned by one wavefront of the tile kernel
constexpr int kPixLog = 11;               // log2 pixels per tile
constexpr int kMaxSeq = FRLW_MAX_SEQUENCES;
constexpr int kMaxFastTiles = 1024;       // tiles per sequence (LDS of the scatter workgroup: 72 B per tile)
constexpr int kMaxPairs = 8192;           // (sequence, tile) pairs per call (LDS of the tile scan: one round)
constexpr int kMaxBinPairs = 65536;       // (sequence, bin) pairs per call in the direct mode (the tile scan runs in rounds)
constexpr int kFastSlab = 32;             // chunks per slab of the two-level column scan
constexpr int ST_MULBAD = 8;              // per-chunk flag next to the ST_* error bits (not an error)
constexpr int kSplitSeg = 8192;           // records one workgroup of the sub-tile split handles
constexpr int kBigBpw = 20;               // 64-event batches per wavefront of the one-workgroup-per-CU form of kf_scatter_cm
#ifndef FRLW_WHOLE_SEGS
#define FRLW_WHOLE_SEGS 4 /* measured: 8 -> 4 takes 7 % (TAF hot spot at 10 M events) to 15 % (Event Volume batch with hot spots) off skewed calls, uniform calls unchanged; 3 sends ordinary 25 000-record GEN1 tiles through the segments (+9 %) */
#endif
constexpr int kSplitWhole = FRLW_WHOLE_SEGS * kSplitSeg; // tiles up to this many records are split by ONE workgroup (kf_split_whole) ...
#ifndef FRLW_FEW_PAIRS
#define FRLW_FEW_PAIRS 256
#endif
constexpr int kFewPairs = FRLW_FEW_PAIRS;             // ... unless the call has fewer (sequence, tile) pairs than this: one workgroup per
                                           // tile would leave most CUs idle (one GEN1 stream: 20 tiles of 50 000 records took
                                           // 31 us), so every tile above one segment goes through the segment kernels
constexpr int kColMax = 4096; // chunks per sequence a consumer keeps in LDS (32 KB); longer sequences take the histogram path
constexpr int kColDirect = 2047; // chunks per sequence the walk's column fits (two arrays over the wavefronts' plane areas)
constexpr int kColEv = 511;       // chunks per sequence a wavefront's column holds

struct SeqTab { // kernel argument, built on the host
    int n_seq;
    int chunk0[kMaxSeq + 1];    // first chunk of sequence s; [n_seq] = total
    int slab0[kMaxSeq + 1];     // first slab
    long long ev0[kMaxSeq + 1]; // first event
    long long t0[kMaxSeq];      // t_start
};

struct FastPlan {
    int twl, thl, tiles_x, tiles_y, T;
    // Direct mode (small calls on small frames): the partition's bins are the 256-cell SUB-TILES (16 per tile) instead of the tiles, so kf_scatter's output
    // already is sub-tile-major and the second-level split (kf_split_whole / kf_split_place: a read + write of every record)
    // is not run at all.  Possible while a sequence has at most kMaxFastTiles bins (the scatter workgroup keeps 16 counters
    // per bin in LDS): the GEN1 / 304x240 class of frames (36 tiles = 576 bins), not 1280x720 (450 tiles = 7200 bins).
    int direct, TB, bin_shift, pairs_b; // bins per sequence (T or 16 T), log2 of bins per tile, (sequence, bin) pairs
    int big;                            // chunk-major partition with chunks above 8192 events (kf_scatter_cm<.., kBigBpw>)
    int bpw, chunk;
    int chunks, slabs, pairs;
    size_t off_counts, off_slabtot, off_base, off_sub, off_seg0, off_segcnt, off_errs, off_tlut, off_records, off_records2, bytes;
    size_t off_sub_end, off_segdesc; // chunk-major partition: list ends, pair of every split segment
    size_t off_wst, off_wst_flag;    // TileP::wst / wst_flag
    int max_seq_chunks;              // chunks of the longest sequence (the column a chunk-major consumer keeps in LDS)
    int max_segs;
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Tile shape: 2^twl x 2^(11 - twl) pixels, the one that covers the frame with the fewest tiles (ties: the widest,
// longest contiguous rows).
enum : int { DIRECT_OFF = 0, DIRECT_AUTO = 1, DIRECT_FORCE = 2 };
bool fast_plan(long long n, int n_seq, int H, int W, FastPlan &p, int direct_mode = DIRECT_AUTO, int min_bpw = 0, bool cm = false)
{
    if (H <= 0 || W <= 0 || n < 0 || n_seq < 1 || n_seq > kMaxSeq || n >= (1ll << 31)) return false;
    long long best = -1;
    for (int twl = 5; twl <= 8; ++twl) {
        const int tw = 1 << twl, th = 1 << (kPixLog - twl);
        const long long t = (long long)((W + tw - 1) / tw) * ((H + th - 1) / th);
        if (best < 0 || t <= best) { best = t; p.twl = twl; }
    }
    p.thl = kPixLog - p.twl;
    p.tiles_x = (W + (1 << p.twl) - 1) >> p.twl;
    p.tiles_y = (H + (1 << p.thl) - 1) >> p.thl;
    p.T = p.tiles_x * p.tiles_y;
    if (p.T > kMaxFastTiles || (long long)p.T * n_seq > kMaxPairs) return false;
    p.pairs = p.T * n_seq;
    // AUTO: calls with few (sequence, tile) pairs whose tiles hold more than one split segment on average -- the launch-bound
    // ones (one GEN1 stream of 1 M events: 52 -> 42 us; eight: 150 -> 136 us; tools/time_direct.py).  With many pairs
    // kf_split_whole is the cheaper second level (64 GEN1 streams: 820 us against 876 direct), with few events per tile the
    // 576-bin scatter costs more than the whole-tile split it replaces (one stream of 250 k events: 40 us against 46):
    // there only when forced (frlw_tuning_t::direct_bins = 1).
    // Chunk-major partition (cm): the consumers of a direct-mode call gather their own lists -- two launches in all -- so every
    // call with few pairs goes that way, however few events a pair holds (5 sequences of 70 k events on 97x131: 36 us against 55).
    p.direct = (direct_mode != DIRECT_OFF && kFW * p.T <= kMaxFastTiles && (long long)kFW * p.T * n_seq <= kMaxBinPairs &&
                (direct_mode == DIRECT_FORCE || (p.pairs < 2 * kFewPairs && (cm || n >= (long long)kSplitSeg * p.pairs)))) ? 1 : 0;
    p.TB = p.direct ? kFW * p.T : p.T;
    p.bin_shift = p.direct ? 4 : 0;
    p.pairs_b = p.TB * n_seq;
    // Chunk size: the partition kernels run two workgroups per CU (512 at a time), and a grid that is not a whole number
    // of such rounds ends on a part-filled one (10 M events in chunks of 8192 = 2.4 rounds: the last one 38 % full).  So
    // the stream is cut into 512 * k chunks with the smallest k whose chunks fit the 8192-event staging area.
    // (cm with min_bpw above kMaxBpw: the one-workgroup-per-CU form of kf_scatter_cm, chunks up to kBigBpw batches per
    // wavefront in 256 * k chunks -- tile bins only, and only while staging area + counters fit the CU's LDS)
    // Default: frames with many tiles and streams long enough to fill two rounds of 256 such chunks -- where the ordinary chunks
    // would leave a consumer runs of a dozen records (10 M events at 1280x720: 164 us against 171 with 8192-event chunks and 177
    // with the histogram partition; 3 M events: 113 against 111 -- hence the lower bound; 64 GEN1 streams have 200-record runs
    // either way and lose 1.5 % to the lower occupancy)
    const bool big = cm && !p.direct && (min_bpw > kMaxBpw || (min_bpw == 0 && p.TB >= 256 && n >= 6000000)) &&
                     (long long)kFW * p.TB * 4 + (p.TB + 2) * 4 + (long long)kFT * kBigBpw * 4 + 64 <= 150 * 1024;
    p.big = big ? 1 : 0;
    long long cap = (long long)kFT * (big ? kBigBpw : kMaxBpw);
    const long long round = big ? 256 : 512;
    if (p.direct) { // 16 counters per bin: shorter chunks keep the scatter workgroup at two per CU (78 KB of LDS)
        const long long lds_cap = ((79ll * 1024 - 16 - (long long)kFW * p.TB * 4 - (p.TB + 2) * 4) / 6) / 16 * 16;
        if (lds_cap >= 2048 && lds_cap < cap) cap = lds_cap;
    }
    long long k = (n + round * cap - 1) / (round * cap);
    if (k < 1) k = 1;
    long long ce = (n + round * k - 1) / (round * k);
    ce = (ce + 15) / 16 * 16;
    // cm: a consumer gathers one run per chunk, so a call that cannot fill 512 workgroups anyway takes the largest chunks there are
    // (one GEN1 stream: 144 chunks of 6944 events instead of 509 of 1968: 32 us against 50)
    if (cm && k == 1) ce = cap;
    if (ce < 1024) ce = 1024; // tiny calls: keep whole 64-event batches per wavefront
    // frlw_tuning_t::batches_per_wave: at least this many 64-event batches per wavefront (only ever LARGER chunks than the
    // default: the workspace query budgets the default's chunk count)
    if (min_bpw > 0 && ce < (long long)min_bpw * kFT) ce = (long long)min_bpw * kFT;
    if (ce > cap) ce = cap;
    p.chunk = (int)ce;
    p.bpw = (p.chunk / kFW + kWave - 1) / kWave;
    return true;
}

// The workspace layout: ONE list of tables, laid out from (chunk count, slab count, events, window, plan).  fast_layout calls it
// with the call's own counts, the size query (frlw_taf_batch_workspace_bytes) with its upper bounds: what the query budgets
// is by construction what a call lays out.
void layout_offsets(FastPlan &p, size_t chunks, size_t slabs, long long n, size_t win)
{
    const size_t n_rec = (size_t)(n > 0 ? n : 1);
    size_t off = kHeaderBytes;
    auto take = [&off](size_t bytes) { const size_t at = off; off = align_up(off + bytes, 256); return at; };
    p.max_segs = 2 * (int)(n / kSplitSeg) + 1; // tiles above the whole-tile limit (>= one segment): full segments + one partial each
    p.off_counts = take(chunks * p.TB * 4);
    p.off_slabtot = take(slabs * p.TB * 4);
    p.off_base = take((size_t)(p.pairs_b + 1) * 4);
    p.off_sub = take(((size_t)p.pairs * kFW + 1) * 4);
    p.off_seg0 = take((size_t)(p.pairs_b + 1) * 4);
    p.off_segcnt = take((size_t)p.max_segs * kFW * 4);
    p.off_errs = take(chunks * 4);
    p.off_tlut = take((win + 1) * 4);
    p.off_records = take(n_rec * 4);
    p.off_records2 = take(n_rec * 4);
    p.off_sub_end = take(((size_t)p.pairs * kFW + 1) * 4);
    p.off_segdesc = take((size_t)p.max_segs * 4);
    p.off_wst = take((size_t)p.pairs * kFW * (FRLW_MAX_WINDOWS + 1) * 4);
    p.off_wst_flag = take((size_t)p.pairs * 4);
    p.bytes = off;
}

// per-sequence chunk / slab tables + workspace layout
bool fast_layout(const int64_t *seq_offsets, const int64_t *t_start, int n_seq, FastPlan &p, SeqTab &S, uint32_t win)
{
    S.n_seq = n_seq;
    int c = 0, sl = 0;
    p.max_seq_chunks = 1;
    for (int s = 0; s < n_seq; ++s) {
        const long long n_s = seq_offsets[s + 1] - seq_offsets[s];
        if (n_s < 0) return false;
        S.chunk0[s] = c;
        S.slab0[s] = sl;
        S.ev0[s] = seq_offsets[s];
        S.t0[s] = t_start[s];
        int cs = (int)((n_s + p.chunk - 1) / p.chunk);
        if (cs < 1) cs = 1; // an empty sequence keeps one (empty) chunk: no special cases downstream
        if (cs > p.max_seq_chunks) p.max_seq_chunks = cs;
        c += cs;
        sl += (cs + kFastSlab - 1) / kFastSlab;
    }
    S.chunk0[n_seq] = c;
    S.slab0[n_seq] = sl;
    S.ev0[n_seq] = seq_offsets[n_seq];
    p.chunks = c;
    p.slabs = sl;
    layout_offsets(p, (size_t)c, (size_t)sl, seq_offsets[n_seq] - seq_offsets[0], win); // (every sequence has a chunk: c, sl >= 1)
    return true;
}

// LDS of a scatter workgroup (the layouts: kf_scatter / kf_scatter_cm, taf_partition.h)
inline size_t scatter_lds_bytes(int T, int chunk) { return (size_t)kFW * T * 4 + (size_t)(T + 2) * 4 + (size_t)chunk * 4 + (size_t)chunk * 2 + 16; }
inline size_t scatter_cm_lds_bytes(int T, int chunk) { return (size_t)kFW * T * 4 + (size_t)(T + 2) * 4 + (size_t)chunk * 4 + 16; }

// chunk-major partition or histogram partition?  frlw_tuning_t::chunk_major = 0 forces the histogram partition; otherwise the
// chunk-major one runs wherever a consumer can hold a sequence's column of the directory in LDS (cm_fits).  Measured (us, chunk-major against histogram partition): one
// GEN1 stream 32 / 42, 5 x 70 k events on 97x131 34 / 55, 3 M events at 1280x720 111 / 133, 10 M events 164 / 177, 64 GEN1
// streams 808 / 861, Event Volume x64 736 / 787; the skewed variants give some of it back (25 % of 10 M events in one blob:
// 298 / 287 -- the split segments of a skewed tile are only known after the split kernel, so their counting pass is a launch
// of its own).
enum : int { CM_OFF = 0, CM_AUTO = -1, CM_ON = 1 };
inline bool cm_fits(const FastPlan &p, bool ev)
{
    const int col = p.direct ? (ev ? kColEv : kColDirect) : kColMax;
    return p.max_seq_chunks <= col && p.chunk <= 65535;
}

// plan + layout of one batch call (tries the chunk-major plan first where the knob allows it).  The three knobs as plain ints:
// frlw_tuning_t::chunk_major (CM_*), batches_per_wave (0: the plan's own) and direct_bins (below 0: automatic)
inline int plan_select(int knob, int bpw, int direct, bool ev, int n_seq, int H, int W, const int64_t *seq_offsets, const int64_t *t0,
                       int64_t window_us, FastPlan &p, SeqTab &S, bool &cm)
{
    const long long n = seq_offsets[n_seq] - seq_offsets[0];
    const int dmode = direct < 0 ? (int)DIRECT_AUTO : (direct != 0 ? (int)DIRECT_FORCE : (int)DIRECT_OFF);
    cm = false;
    if (knob != CM_OFF) {
        if (!fast_plan(n, n_seq, H, W, p, dmode, bpw, true)) return FRLW_ERR_UNSUPPORTED;
        if (!fast_layout(seq_offsets, t0, n_seq, p, S, (uint32_t)window_us)) return FRLW_ERR_ARG;
        cm = cm_fits(p, ev);
    }
    if (!cm) {
        if (!fast_plan(n, n_seq, H, W, p, dmode, bpw, false)) return FRLW_ERR_UNSUPPORTED;
        if (!fast_layout(seq_offsets, t0, n_seq, p, S, (uint32_t)window_us)) return FRLW_ERR_ARG;
    }
    return FRLW_OK;
}

// frlw_taf_batch_workspace_bytes: what plan_select's layout never exceeds (tests/test_taf_plan_cpu.py checks it over a grid)
inline size_t batch_workspace_bytes(int64_t n_events, int n_seq, int H, int W, int64_t window_us)
{
    if (window_us < 1 || window_us >= (1ll << 20)) return 0;
    size_t need = 0;
    for (int mode = 0; mode < 4; ++mode) { // the largest of the partition modes (the call's tuning and size pick one)
        const int direct = mode & 1, cm = mode >> 1;
        FastPlan p;
        if (!fast_plan(n_events, n_seq, H, W, p, direct ? DIRECT_FORCE : DIRECT_OFF, 0, cm != 0)) return 0;
        if (direct && !p.direct) continue;
        // the layout depends on how the events are spread over the sequences only through the chunk count: every sequence
        // can add one partly filled chunk and one partly filled slab
        const size_t chunks = (size_t)(n_events + p.chunk - 1) / p.chunk + n_seq;
        const size_t slabs = chunks / kFastSlab + n_seq + 1;
        layout_offsets(p, chunks, slabs, n_events, (size_t)window_us);
        if (p.bytes > need) need = p.bytes;
    }
    return need;
}

// The plan of the two-launch form for one call of n events on an H x W frame, or false when the call is not eligible (shared by
// sae_fast_try and by frlw_encoder_workspace_bytes: the size query must cover what the call will ask for).
inline bool sae_fast_plan(long long n, int H, int W, long long t0v, FastPlan &p, SeqTab &S)
{
    // positions + 1 must fit the 20 bits above the 12-bit cell; tiny calls gain nothing
    if (n < 16384 || n >= (1ll << 20) - 1) return false;
    const int64_t offs[2] = {0, (int64_t)n};
    const int64_t t0[1] = {(int64_t)t0v};
    if (!fast_plan(n, 1, H, W, p, DIRECT_FORCE, 0, true) || !p.direct) return false; // frames of at most 64 tiles (the 304x240 class)
    {   // at least ~64 chunks: the plan's largest-chunk rule (one GEN1 stream of 1 M events: 144 chunks) would leave a
        // 100 000-event call with 15 scatter workgroups on 256 CUs
        long long ce = ((n + 63) / 64 + 15) / 16 * 16;
        if (ce < 1024) ce = 1024;
        if (ce < p.chunk) { p.chunk = (int)ce; p.bpw = (p.chunk / kFW + kWave - 1) / kWave; }
    }
    if (!fast_layout(offs, t0, 1, p, S, 1u)) return false;
    if (p.max_seq_chunks > kColEv || p.chunk > 65535 || p.big) return false;
    if (scatter_cm_lds_bytes(p.TB, p.chunk) > 160 * 1024) return false;
    return true;
}
} // namespace
