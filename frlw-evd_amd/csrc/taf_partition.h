// taf_partition.h -- the first level, a stable partition of the events by bin: the histogram partition (kf_hist, kf_slabscan,
// kf_tilescan, kf_scatter) and the chunk-major one (kf_scatter_cm), with the developer timeline macros (*PROF).
// Expects taf_decode.h (and through it taf_plan.h, frlw_common.h).
#pragma once
#include "taf_decode.h"
#include <stddef.h>

namespace {
__host__ __device__ inline uint32_t whole_max_of(int pairs) { return pairs < kFewPairs ? (uint32_t)kSplitSeg : (uint32_t)kSplitWhole; }
__host__ __device__ inline uint32_t split_segments(uint32_t n, uint32_t whole_max) { return n > whole_max ? (n + kSplitSeg - 1) / kSplitSeg : 0u; }

// ---- 1. histogram ------------------------------------------------------------------------------------
// Persistent workgroups (two per CU) walk the chunks grid-stride; a thread takes eight records of a chunk as four 16-byte
// loads (the order inside a chunk does not matter for a histogram) and has the NEXT chunk's loads in flight while it
// decodes and counts this one: the read of the 8-byte records runs at the copy rate instead of in bursts.
struct HistSpan { // wave-uniform description of one chunk's records
    long long first; // index of the first record the loads cover (a 16-byte boundary; may lie one record in front of the chunk)
    long long begin, end;
    long long t0;
};

__device__ __forceinline__ HistSpan hist_span(const FastGeom &G, const SeqTab &S, int chunk, int n_chunks)
{
    HistSpan L;
    L.begin = L.end = L.first = 0;
    L.t0 = 0;
    if (chunk >= n_chunks) return L;
    const int s = seq_of_chunk(S, chunk);
    L.t0 = S.t0[s];
    L.begin = S.ev0[s] + (long long)(chunk - S.chunk0[s]) * G.chunk_ev;
    L.end = L.begin + G.chunk_ev < S.ev0[s + 1] ? L.begin + G.chunk_ev : S.ev0[s + 1];
    if (L.end < L.begin) L.end = L.begin;
    // record pairs on 16-byte boundaries: step one record back if the chunk starts on the odd half of a pair (stays
    // inside the array unless the array itself starts there: then the loads are merely unaligned)
    L.first = L.begin - (long long)((reinterpret_cast<uintptr_t>(G.data + L.begin) >> 3) & 1u);
    if (L.first < 0) L.first = L.begin;
    return L;
}

// Loads without branches (a load under a lane condition becomes its own basic block with its own s_waitcnt: eight
// serialized round trips to HBM): every thread reads SOME pair of the chunk -- its own, or the chunk's last one -- and the
// validity of the two records is decided afterwards from the indices.
__device__ __forceinline__ uint32_t hist_pairs(const HistSpan &L) // whole pairs inside [first, end): both records exist
{
    long long cover = L.end - L.first;
    if (cover > 2ll * (kMaxBpw / 2) * kFT) cover = 2ll * (kMaxBpw / 2) * kFT;
    return (uint32_t)(cover >> 1);
}

__device__ __forceinline__ void hist_issue(const FastGeom &G, const HistSpan &L, uint4 (&v)[kMaxBpw / 2])
{
    const uint32_t pairs = hist_pairs(L);
    if (pairs > 0) { // wave-uniform
        const uint4 *src = (const uint4 *)(G.data + L.first);
#pragma unroll
        for (int j = 0; j < kMaxBpw / 2; ++j) {
            const uint32_t pj = (uint32_t)(j * kFT) + threadIdx.x;
            v[j] = src[pj < pairs ? pj : pairs - 1u];
        }
    }
}

template <bool HAS_MAP, bool EV = false, bool SIMPLE = false>
__global__ __launch_bounds__(kFT) __attribute__((amdgpu_waves_per_eu(8, 8))) void kf_hist(FastGeom G, SeqTab S, uint32_t *counts,
                                                                                         int32_t *errs, float *tlut_w, int n_chunks)
{
    extern __shared__ uint32_t lds[];
    uint32_t *hist = lds; // [T]
    __shared__ int serr;
    const int tid = threadIdx.x;
    for (int b = tid; b < G.T; b += kFT) hist[b] = 0;
    if (tid == 0) serr = 0;
    int mul_err = 0;
    if (EV) {
        // Event Volume: tlut[r] = float(r / window) (generate_eventvolume.py:141, :23: t.float()), r = t - (t_end - window);
        // the same exhaustive check decides whether the tile kernels may multiply by 1 / window instead
        const double den = (double)G.win, rcp = G.rcp;
        for (long long r = (long long)blockIdx.x * kFT + tid; r <= (long long)G.win; r += (long long)gridDim.x * kFT) {
            const float exact = (float)((double)r / den);
            if ((float)((double)r * rcp) != exact) mul_err = ST_MULBAD;
            tlut_w[r] = exact;
        }
    } else if (tlut_w) {
        // tlut[r] = float(r / (win + 1e-8)) - 1 (generate_taf.py:215, :26): one correctly rounded f64 division per
        // distinct in-window time instead of one per event
        // The walk kernel would rather multiply by 1 / den than gather from the table: allowed only if that gives the
        // same float for EVERY r of the domain, which is checked right here, exhaustively, per call.
        const double den = (double)G.win + 1e-8, rcp = G.rcp;
        for (long long r = (long long)blockIdx.x * kFT + tid; r <= (long long)G.win; r += (long long)gridDim.x * kFT) {
            const float exact = (float)((double)r / den);
            if ((float)((double)r * rcp) != exact) mul_err = ST_MULBAD;
            tlut_w[r] = exact - 1.0f;
        }
    }
    uint4 cur[kMaxBpw / 2], nxt[kMaxBpw / 2];
    HistSpan Lc, Ln = hist_span(G, S, (int)blockIdx.x, n_chunks);
    hist_issue(G, Ln, nxt);
    if (mul_err) atomicOr(&serr, mul_err);
    __syncthreads();
    for (int chunk = (int)blockIdx.x; chunk < n_chunks; chunk += (int)gridDim.x) {
        Lc = Ln;
#pragma unroll
        for (int j = 0; j < kMaxBpw / 2; ++j) cur[j] = nxt[j];
        Ln = hist_span(G, S, chunk + (int)gridDim.x, n_chunks);
        hist_issue(G, Ln, nxt);
        int err = 0;
        const uint32_t pairs = hist_pairs(Lc);
        const bool skip_first = Lc.first != Lc.begin; // the first record of pair 0 lies in front of the chunk
#pragma unroll
        for (int j = 0; j < kMaxBpw / 2; ++j) {
            const uint32_t pj = (uint32_t)(j * kFT + tid);
            if (pj < pairs && !(skip_first && pj == 0u)) {
                const FastEv o = fast_decode<HAS_MAP, EV, SIMPLE>(G, make_uint2(cur[j].x, cur[j].y), Lc.t0);
                err |= o.err;
                if (o.tile >= 0) atomicAdd(&hist[o.tile], 1u);
            }
            if (pj < pairs) {
                const FastEv o = fast_decode<HAS_MAP, EV, SIMPLE>(G, make_uint2(cur[j].z, cur[j].w), Lc.t0);
                err |= o.err;
                if (o.tile >= 0) atomicAdd(&hist[o.tile], 1u);
            }
        }
        // what the whole pairs leave over -- the odd record at the chunk's end (also when the chunk starts on the odd half of
        // a pair and is covered from one record earlier): at most one, fetched by one thread
        if (tid == 0 && Lc.end > Lc.begin && Lc.first + 2ll * pairs < Lc.end) { // (an EMPTY chunk covered from one record earlier has nothing left over)
            const FastEv o = fast_decode<HAS_MAP, EV, SIMPLE>(G, G.data[Lc.end - 1], Lc.t0);
            err |= o.err;
            if (o.tile >= 0) atomicAdd(&hist[o.tile], 1u);
        }
        if (err) atomicOr(&serr, err);
        __syncthreads();
        uint32_t *row = counts + (long long)chunk * G.T;
        for (int b = tid; b < G.T; b += kFT) { row[b] = hist[b]; hist[b] = 0u; }
        if (tid == 0) { errs[chunk] = serr; serr = 0; }
        __syncthreads();
    }
}

// ---- 2. scans ----------------------------------------------------------------------------------------
// counts[c][b], c in one slab of 32 chunks of ONE sequence -> exclusive prefix over c (in place), slabtot[slab][b]
__device__ __forceinline__ void slabscan_one(const SeqTab &S, uint32_t *counts, int T, uint32_t *slabtot, int slab, int b)
{
    const int s = seq_of(S.slab0, S.n_seq, slab);
    const int c0 = S.chunk0[s] + (slab - S.slab0[s]) * kFastSlab, cend = S.chunk0[s + 1];
    uint32_t v[kFastSlab];
#pragma unroll
    for (int k = 0; k < kFastSlab; ++k) v[k] = (c0 + k < cend) ? counts[(long long)(c0 + k) * T + b] : 0u;
    uint32_t run = 0;
#pragma unroll
    for (int k = 0; k < kFastSlab; ++k) {
        const uint32_t t = v[k];
        v[k] = run;
        run += t;
    }
#pragma unroll
    for (int k = 0; k < kFastSlab; ++k)
        if (c0 + k < cend) counts[(long long)(c0 + k) * T + b] = v[k];
    slabtot[(long long)slab * T + b] = run;
}
__global__ __launch_bounds__(kWave) void kf_slabscan(SeqTab S, uint32_t *counts, int T, uint32_t *slabtot)
{
    const int b = blockIdx.x * kWave + threadIdx.x;
    if (b < T) slabscan_one(S, counts, T, slabtot, blockIdx.y, b);
}

// slabtot[slab][b] -> exclusive prefix over the slabs of each sequence (in place); exclusive scan over the
// (sequence, tile) pairs -> base[0..pairs]; resets the header and folds the per-chunk error flags into it.
// (small calls -- at most kInlineSlabScan (slab, tile) columns -- run the slab scan here too: one launch less)
constexpr int kInlineSlabScan = 8192;
__global__ __launch_bounds__(kFT) void kf_tilescan(SeqTab S, uint32_t *slabtot, int T, uint32_t *base, uint32_t *seg0,
                                                   FastHeader *hdr, const int32_t *errs, int chunks, uint32_t *counts_inline,
                                                   int slabs_inline, int no_segments)
{
    if (counts_inline) {
        for (int i = threadIdx.x; i < slabs_inline * T; i += kFT) slabscan_one(S, counts_inline, T, slabtot, i / T, i % T);
        __syncthreads(); // the totals are read back below by other threads of this workgroup
    }
    __shared__ uint32_t tot[kMaxPairs];
    __shared__ uint32_t wsum[kFW], wsum2[kFW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int pairs = S.n_seq * T; // (T = bins per sequence: tiles, or sub-tiles in the direct mode)
    if (tid == 0) { hdr->status = 0; hdr->filtered_tiles = 0u; hdr->mul_bad = 0u; }
    if (tid < kMaxSeq) hdr->wmask[tid] = 0ull;
    __syncthreads();
    {
        int e = 0;
        for (int c = tid; c < chunks; c += kFT) e |= errs[c];
        if (e & ~ST_MULBAD) atomicOr(&hdr->status, e & ~ST_MULBAD);
        if (e & ST_MULBAD) hdr->mul_bad = 1u;
    }
    // two exclusive scans over the (sequence, bin) pairs: records -> base[], split segments (kSplitSeg records each, at least
    // one per pair; none in the direct mode) -> seg0[]; rounds of kMaxPairs pairs (the direct mode has up to 65 536)
    const uint32_t whole_max = no_segments ? 0xffffffffu : whole_max_of(pairs);
    uint32_t carry = 0, scarry = 0;
    for (int p0 = 0; p0 < pairs; p0 += kMaxPairs) {
        const int np = pairs - p0 < kMaxPairs ? pairs - p0 : kMaxPairs;
        for (int idx = tid; idx < np; idx += kFT) {
            const int gi = p0 + idx, s = gi / T, b = gi - s * T;
            uint32_t run = 0;
            const int sl1 = S.slab0[s + 1];
            for (int sl = S.slab0[s]; sl < sl1; sl += 8) { // 8 independent loads in flight, then the 8 prefix stores
                uint32_t v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = sl + k < sl1 ? slabtot[(long long)(sl + k) * T + b] : 0u;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (sl + k < sl1) slabtot[(long long)(sl + k) * T + b] = run;
                    run += v[k];
                }
            }
            tot[idx] = run;
        }
        __syncthreads();
        const int per = (np + kFT - 1) / kFT;
        const int b0 = tid * per;
        int b1 = b0 + per;
        if (b1 > np) b1 = np;
        uint32_t sum = 0, ssum = 0;
        for (int b = b0; b < b1; ++b) { sum += tot[b]; ssum += split_segments(tot[b], whole_max); }
        uint32_t inc = sum, sinc = ssum;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const uint32_t v = __shfl_up(inc, off), v2 = __shfl_up(sinc, off);
            if (lane >= off) { inc += v; sinc += v2; }
        }
        if (lane == kWave - 1) { wsum[wv] = inc; wsum2[wv] = sinc; }
        __syncthreads();
        uint32_t pre = 0, spre = 0, all = 0, sall = 0;
        for (int k = 0; k < kFW; ++k) {
            if (k < wv) { pre += wsum[k]; spre += wsum2[k]; }
            all += wsum[k]; sall += wsum2[k];
        }
        uint32_t run = carry + pre + inc - sum, srun = scarry + spre + sinc - ssum;
        for (int b = b0; b < b1; ++b) {
            base[p0 + b] = run;
            seg0[p0 + b] = srun;
            run += tot[b];
            srun += split_segments(tot[b], whole_max);
        }
        carry += all;
        scarry += sall;
        __syncthreads(); // tot / wsum are reused by the next round
    }
    if (tid == 0) { base[pairs] = carry; seg0[pairs] = scarry; }
    if (tid == 0) fold_sticky_status(hdr, hdr->status); // all error flags are in since the barrier behind the fold above
}

// ---- 3. stable scatter ---------------------------------------------------------------------------------
// LDS (dynamic, scatter_lds_bytes): wcnt[16][T] u32 | loff[T + 1] u32 | stage[chunk] u32 | stile[chunk] u16  (78.6 KB at T = 450 with
// 8192-event chunks: two workgroups per CU)
template <bool HAS_MAP, bool EV = false, bool SIMPLE = false>
__global__ __launch_bounds__(kFT) void kf_scatter(FastGeom G, SeqTab S, const uint32_t *counts, const uint32_t *slabtot,
                                                  const uint32_t *base, uint32_t *records, FastHeader *hdr)
{
    extern __shared__ uint32_t lds[];
    const int T = G.T;
    uint32_t *wcnt_all = lds;                  // [16][T]: per-wavefront running counts, then prefixes
    uint32_t *loff = wcnt_all + (size_t)kFW * T; // [T + 1] slot of tile b's first record in the staged chunk; after
                                                 // the staging: global slot of that record MINUS its staged slot
    uint32_t *stage = loff + ((T + 2) & ~1);
    uint16_t *stile = (uint16_t *)(stage + G.chunk_ev);
    __shared__ uint32_t wtot[kFW];
    __shared__ unsigned long long wg_seen;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6; // (NOT readfirstlane: with the wavefront index in an SGPR this kernel ran 60 % longer, measured)
    const int chunk = (int)chunk_of_block(blockIdx.x, gridDim.x);
    const int s = seq_of_chunk(S, chunk);
    uint32_t *wcnt = wcnt_all + (size_t)wv * T;
    for (int b = tid; b < kFW * T; b += kFT) wcnt_all[b] = 0;
    if (tid == 0) wg_seen = 0ull;
    __syncthreads();

    const long long chunk_begin = S.ev0[s] + (long long)(chunk - S.chunk0[s]) * G.chunk_ev;
    const long long wave_begin = chunk_begin + (long long)wv * G.run; // wavefront w owns the w-th run of the chunk
    const long long left = S.ev0[s + 1] - wave_begin;
    const uint32_t nloc = left < (long long)G.run ? (uint32_t)(left < 0 ? 0 : left) : (uint32_t)G.run;
    const long long t0 = S.t0[s];
    uint2 q[kMaxBpw];
    if (nloc > 0) { // wave-uniform.  No load under a lane condition (each would wait for its own data: eight serialized round
                    // trips): lanes behind the run's end re-read its last event and are masked by `i < nloc` below
        const uint2 *src = G.data + wave_begin;
#pragma unroll
        for (int j = 0; j < kMaxBpw; ++j) {
            const uint32_t i = (uint32_t)(j * kWave + lane);
            q[j] = src[i < nloc ? i : nloc - 1u];
        }
    }
    // global slot of this chunk's run in every tile (needed after the ranks: issue the loads now)
    const int slab = S.slab0[s] + (chunk - S.chunk0[s]) / kFastSlab;
    // (three loads without a lane condition, summed only where the sum is needed: inside an `if (tid < T)` the compiler
    // waits for them -- and for the event loads in front of them -- right here)
    const int tcl = tid < T ? tid : 0;
    const uint32_t gs_a = base[s * T + tcl], gs_b = slabtot[(long long)slab * T + tcl], gs_c = counts[(long long)chunk * T + tcl];
    // ---- phase A: stream rank of every event inside (wavefront, tile): batches of 64 consecutive events, one
    // returning LDS atomic each -- same-address lanes are served in lane order, and a wavefront's LDS instructions in
    // program order, so the returned count is the number of earlier events of the wavefront's run in the same tile.
    uint32_t where[kMaxBpw], word[kMaxBpw];
    unsigned long long wseen = 0ull;
#pragma unroll
    for (int j = 0; j < kMaxBpw; ++j) {
        where[j] = 0xffffffffu;
        word[j] = 0u;
        if (j < G.bpw) {
            const uint32_t i = (uint32_t)(j * kWave + lane);
            if (i < nloc) {
                const FastEv o = fast_decode<HAS_MAP, EV, SIMPLE>(G, q[j], t0);
                if (o.tile >= 0) {
                    const uint32_t r = atomicAdd(&wcnt[o.tile], 1u);
                    where[j] = ((uint32_t)o.tile << 16) | r;
                    word[j] = o.word;
                    wseen |= 1ull << o.window;
                }
            }
        }
    }
    __syncthreads();
    // ---- phase B: per tile, exclusive prefix of the 16 wavefront counts; chunk-local offsets of the tiles
    uint32_t mine = 0; // records of tile `tid` in this chunk
    for (int b = tid; b < T; b += kFT) {
        uint32_t run = 0;
#pragma unroll
        for (int w = 0; w < kFW; ++w) {
            const uint32_t v = wcnt_all[(size_t)w * T + b];
            wcnt_all[(size_t)w * T + b] = run;
            run += v;
        }
        mine = run;
    }
    const uint32_t inc = wave_incl_scan(mine);
    if (lane == kWave - 1) wtot[wv] = inc;
    __syncthreads();
    uint32_t pre = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kFW; ++k) { if (k < wv) pre += wtot[k]; total += wtot[k]; }
    if (tid < T) loff[tid] = pre + inc - mine;
    __syncthreads();
    // ---- phase C: stage the chunk tile-major in LDS, then leave in one linear sweep: consecutive threads write
    // consecutive records of a tile's run (whole lines instead of 64 scattered 4-byte stores)
#pragma unroll
    for (int j = 0; j < kMaxBpw; ++j) {
        if (j < G.bpw && where[j] != 0xffffffffu) {
            const uint32_t b = where[j] >> 16;
            const uint32_t slot = loff[b] + wcnt[b] + (where[j] & 0xffffu);
            stage[slot] = word[j];
            stile[slot] = (uint16_t)b;
        }
    }
    // which windows of the sequence hold events at all ("all(forward)", generate_taf.py:40): OR inside the wavefront,
    // inside the workgroup, and touch the global word only for bits it does not show yet
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)wseen, off), hi = __shfl_xor((unsigned)(wseen >> 32), off);
        wseen |= ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 0 && wseen) atomicOr(&wg_seen, wseen);
    __syncthreads();
    if (tid < T) loff[tid] = (gs_a + gs_b + gs_c) - loff[tid]; // wraps around harmlessly (mod 2^32)
    __syncthreads();
    for (uint32_t qi = tid; qi < total; qi += kFT) records[loff[stile[qi]] + qi] = stage[qi];
    if (tid == 0) {
        const unsigned long long m = wg_seen;
        const unsigned long long have = __hip_atomic_load(&hdr->wmask[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (m & ~have) atomicOr(&hdr->wmask[s], m);
    }
}

// ---- 3'. chunk-major scatter: the partition WITHOUT a histogram pass (round 4) -----------------------------------------
// kf_hist exists only so that kf_scatter knows, before it writes, where every (chunk, bin) run goes in a bin-major array --
// a whole extra pass over the 8-byte events (80 MB and 19 us at 10 M events) plus two scan launches.  Here the scatter
// workgroup sorts its chunk by bin in LDS exactly as before and writes it out AS IT IS, chunk-major: chunk c's records
// occupy rec[first event of c - first event of the call ...) in one linear sweep (whole lines, no per-record address), and
// the chunk leaves one directory row dir[c][bin] = count << 16 | offset of the bin's run inside the chunk.  A bin's list is
// then the concatenation of its runs in chunk order -- still stream order -- and whoever consumes the bin reads its column
// of the directory (a few hundred to a few thousand entries), prefix-sums it in LDS and gathers the runs (col_*, taf_column.h).
// The kernel also does what kf_hist did on the side: the per-call value table + the check that multiplying by 1 / den gives
// the same floats, the data-dependent status (straight into the header: no per-chunk flags to fold), the window masks.

// MAXB: 64-event batches per wavefront the registers hold.  8: 64 VGPRs, two workgroups per CU, chunks up to 8192 events.
// kBigBpw: 128 VGPRs, ONE workgroup per CU, chunks up to 20 480 events (LDS: 80 KB of staging + the counters) -- for large
// calls with tile bins, where a consumer gathers one run per chunk: 10 M events at 1280x720 leave 512 chunks with 43-record
// runs instead of 1536 with 14-record ones.
#ifndef FRLW_SCATTER_AHEAD
#define FRLW_SCATTER_AHEAD 4
#endif
// (-DFRLW_SPLIT_PROF, the timeline of kf_split_whole<true>: the reader of the sums, frlw_debug_walk_prof in taf_fast.hip, is compiled for
// the two older names; a build with the split's name alone borrows the scatter's, with the scatter's own stamps left out)
#if defined(FRLW_SPLIT_PROF) && !defined(FRLW_WALK_PROF) && !defined(FRLW_SCAT_PROF)
#define FRLW_SCAT_PROF
#define FRLW_SCAT_PROF_READER_ONLY
#endif
#if defined(FRLW_WALK_PROF) || defined(FRLW_SCAT_PROF) // developer timeline of kf_taf_walk / kf_scatter_cm / kf_split_whole<true> (tools/enc_lab.cpp prints it): cycles between stamps, summed over workgroups
constexpr int kProfWgs = 131072;
__device__ unsigned long long g_walk_prof[kProfWgs * 9];
#define XPROF(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); pd_[i] += t_ - tp_; tp_ = t_; } while (0)
#define XPROF_INIT() unsigned long long tp_ = __builtin_amdgcn_s_memtime(), pd_[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}
#define XPROF_END() do { if (threadIdx.x == 0 && blockIdx.x < kProfWgs) for (int i_ = 0; i_ < 9; ++i_) g_walk_prof[blockIdx.x * 9 + i_] += pd_[i_]; } while (0)
#endif
#ifdef FRLW_WALK_PROF
#define WPROF(i) XPROF(i)
#define WPROF_INIT() XPROF_INIT()
#define WPROF_END() XPROF_END()
#else
#define WPROF(i) do { } while (0)
#define WPROF_INIT() do { } while (0)
#define WPROF_END() do { } while (0)
#endif
#if defined(FRLW_SCAT_PROF) && !defined(FRLW_SCAT_PROF_READER_ONLY)
#define SPROF(i) XPROF(i)
#define SPROF_INIT() XPROF_INIT()
#define SPROF_END() XPROF_END()
#define SPROF_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define SPROF(i) do { } while (0)
#define SPROF_INIT() do { } while (0)
#define SPROF_END() do { } while (0)
#define SPROF_DRAIN() do { } while (0)
#endif
// kf_split_whole<true> (taf_split.h), stamps of thread 0's wavefront: 0 column loaded | 1 cursor value in hand | 2 barrier in front of
// the gather passed | 3 last gather load issued | 4 tickets done | 5 prefixes done | 6, 7 the two barriers of every staging chunk
// (summed over the chunks) | 8 end.  PPROF_CURSOR(n) waits for thread 0's returning add and for nothing younger: its wavefront has
// issued eight loads per staging chunk behind it, and loads and returning adds come back in the order they were issued.
#ifdef FRLW_SPLIT_PROF
#define PPROF(i) XPROF(i)
#define PPROF_INIT() XPROF_INIT()
#define PPROF_END() XPROF_END()
#define PPROF_CURSOR(n) do { /* s_waitcnt vmcnt(8 | 16 | 24 | 32), the other counters untouched */ \
        if ((n) <= 8192u) __builtin_amdgcn_s_waitcnt(0x0F78); else if ((n) <= 16384u) __builtin_amdgcn_s_waitcnt(0x4F70); \
        else if ((n) <= 24576u) __builtin_amdgcn_s_waitcnt(0x4F78); else __builtin_amdgcn_s_waitcnt(0x8F70); } while (0)
#else
#define PPROF(i) do { } while (0)
#define PPROF_INIT() do { } while (0)
#define PPROF_END() do { } while (0)
#define PPROF_CURSOR(n) do { } while (0)
#endif
template <bool HAS_MAP, bool EV = false, bool SIMPLE = false, int MAXB = kMaxBpw, int SAE = 0>
__global__ __launch_bounds__(kFT) __attribute__((amdgpu_waves_per_eu(MAXB > kMaxBpw ? 4 : 8, MAXB > kMaxBpw ? 4 : 8))) void kf_scatter_cm(FastGeom G, SeqTab S, uint32_t *dir, uint32_t *records, FastHeader *hdr, float *tlut_w,
                                                     uint32_t epoch)
{
    extern __shared__ uint32_t lds[];
    const int T = G.T;
    uint32_t *wcnt_all = lds;                    // [16][T]: per-wavefront running counts, then prefixes
    uint32_t *loff = wcnt_all + (size_t)kFW * T; // [T + 1] slot of bin b's first record in the staged chunk
    uint32_t *stage = loff + ((T + 2) & ~1);
    __shared__ uint32_t wtot[kFW];
    __shared__ unsigned long long wg_seen;
    __shared__ int serr;
    // LEAN (TAF calls with the SIMPLE decode: the headline's form): phase A below decodes without early returns, and wv goes
    // through readfirstlane, so that the compiler knows a wavefront's run (src, nloc, its counter row) is wave-uniform and keeps
    // it in SGPRs.  (Not in the other forms: there the extra SGPRs cost spills -- DESIGN.md 3.11.)
    constexpr bool LEAN = SIMPLE && !EV && !HAS_MAP && SAE == 0;
    const int tid = threadIdx.x, lane = tid & 63, wv = LEAN ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
    SPROF_INIT();
    const int chunk = (int)chunk_of_block(blockIdx.x, gridDim.x);
    const int s = seq_of_chunk(S, chunk);
    uint32_t *wcnt = wcnt_all + (size_t)wv * T;
    for (int b = tid; b < kFW * T; b += kFT) wcnt_all[b] = 0;
    if (tid == 0) { wg_seen = 0ull; serr = 0; }
    if (blockIdx.x == 0 && epoch != 0u) {
        // The header's per-call words are reset HERE, by the workgroup the dispatcher starts first, instead of by a memset node
        // in front of the kernel.  Every other workgroup writes to the header only at its very end and only after it has seen
        // this call's epoch (published below, behind the reset): the first workgroup is resident before any other one starts,
        // so that wait always ends (and is bounded all the same, below).  epoch == 0: the call is being captured into a graph --
        // a host-made epoch would be baked into the node and every replay after the first would find it published already --
        // so launch_fast_cm put a reset kernel in front instead and nobody resets or waits here.
        uint32_t *h32 = (uint32_t *)hdr;
        for (int i = tid; i < (int)(offsetof(FastHeader, epoch) / 4); i += kFT) h32[i] = 0u;
        if (tid == 0) { // an EARLIER call's stall verdict goes; this call's own (a workgroup that gave up before we started) stays
            uint32_t *sw = (uint32_t *)((char *)hdr + kStallOffset);
            const uint32_t was = __hip_atomic_load(sw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (was != 0u && was != epoch) atomicCAS(sw, was, 0u);
        }
        __threadfence();
        __syncthreads();
        if (tid == 0) __hip_atomic_store(&hdr->epoch, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }

    const long long chunk_begin = S.ev0[s] + (long long)(chunk - S.chunk0[s]) * G.chunk_ev;
    const long long wave_begin = chunk_begin + (long long)wv * G.run; // wavefront w owns the w-th run of the chunk
    const long long left = S.ev0[s + 1] - wave_begin;
    const uint32_t nloc = left < (long long)G.run ? (uint32_t)(left < 0 ? 0 : left) : (uint32_t)G.run;
    const long long t0 = S.t0[s];
    // The chunk's events: kAhead batches per wavefront are requested here, batch j + kAhead when batch j is ranked (phase A).
    // All MAXB at once (the form until round 5) fills the CU's memory queue -- 160 KB per CU, every CU of the part in the same
    // burst -- and the wavefronts then stand at the ISSUE of their loads until HBM has served the queue: 8 of a workgroup's 26 us
    // in front of the first decoded event (developer timeline, -DFRLW_SCAT_PROF).
    constexpr int kAhead = MAXB > FRLW_SCATTER_AHEAD ? FRLW_SCATTER_AHEAD : MAXB;
    uint2 q[MAXB];
    const uint2 *src = G.data + wave_begin;
    const uint32_t last = nloc - 1u;
    if (nloc > 0) { // wave-uniform; no load under a lane condition: lanes behind the run's end re-read its last event
#pragma unroll
        for (int j = 0; j < kAhead; ++j) q[j] = src[min((uint32_t)(j * kWave + lane), last)];
    }
    int pre_err = 0;
    // the per-call value table, spread over the grid while the event loads fly (generate_taf.py:215,:26 /
    // generate_eventvolume.py:141,:23): tlut[r] and the exhaustive check "float(r * (1 / den)) == float(r / den) for every r"
    if (tlut_w) {
        const double den = EV ? (double)G.win : (double)G.win + 1e-8, rcp = G.rcp;
        bool bad = false;
        for (long long r = (long long)blockIdx.x * kFT + tid; r <= (long long)G.win; r += (long long)gridDim.x * kFT) {
            const float exact = (float)((double)r / den);
            bad |= (float)((double)r * rcp) != exact;
            tlut_w[r] = EV ? exact : exact - 1.0f;
        }
        // kept in a register until phase A's flags are OR-ed in BEHIND the barrier below: `serr` is zeroed by thread 0 in front
        // of that barrier, and an atomicOr from another wavefront here could land before the zero and be lost
        if (bad) pre_err = ST_MULBAD;
    }
    // The barrier that publishes the zeroed counters must NOT wait for the event loads: __syncthreads() drains vmcnt, and the
    // burst of a whole chunk (160 KB per CU, every CU of the part at once: HBM-bound, 8 of a workgroup's 26 us) would have to
    // land before the first event is decoded.  A raw s_barrier behind the LDS writes only: the compiler's counted waits
    // (loads return in order) then let batch j be ranked while batches j + 1 ... are still on their way.
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    SPROF(0);
    SPROF(1);
    // ---- phase A: stream rank of every event inside (wavefront, bin), one returning LDS atomic each (lane order = stream order)
    // LEAN: fast_decode<false, false, true>'s two helpers without its early returns -- every value is computed for every lane and
    // one mask `ok` decides, so the hot path has no nest of exec-mask branches with their default-value moves.  Same records,
    // flags and window masks as fast_decode.
    // FASTBLK (LEAN, 20 batches: the headline's form, which never has direct bins -- taf_plan.h, `big`): a batch whose 64 lanes
    // all hold an event inside the frame and strictly inside the span takes a block without any lane condition -- full EXEC, no
    // error word, no `ok` / `live` selects, no clamp of the window (relu == span, the one valid case that needs it, goes the
    // slow way with the errors), the window division in full-rate 24-bit multiplies, a 32-bit window mask.  One vote per batch
    // decides, over compares the decode needs anyway; every other batch runs the LEAN code below as it was.  nfast: the run's
    // full batches, or 0 where the call does not allow the block (FastGeom::m24; more than 32 windows; t0 + span past 2^32,
    // where `relu >= span` alone would not see t < t0).  Same records, flags and window masks either way.
    constexpr bool FASTBLK = LEAN && MAXB > kMaxBpw;
    uint32_t where[MAXB], word[MAXB];
    unsigned long long wseen = 0ull;
    uint32_t wseen32 = 0u;
    int err = pre_err;
    const uint32_t t0lo = (uint32_t)t0;
    const uint32_t nfast = FASTBLK && G.m24 && G.n_windows <= 32 && t0lo <= ~G.span ? nloc >> 6 : 0u;
#pragma unroll
    for (int j = 0; j < MAXB; ++j) {
        where[j] = 0xffffffffu;
        word[j] = 0u;
        if (j + kAhead < MAXB) {
            if (nloc > 0 && j + kAhead < G.bpw) // wave-uniform
                q[j + kAhead] = src[min((uint32_t)((j + kAhead) * kWave + lane), last)];
            asm volatile("" ::: "memory"); // (the request stays HERE: hoisted to the top it is the burst again)
        }
        bool fast = false; // wave-uniform
        uint32_t fx = 0u, fy = 0u, frel = 0u;
        if (FASTBLK && (uint32_t)j < nfast) {
            fx = q[j].y & 16383u; fy = (q[j].y >> 14) & 16383u; frel = q[j].x - t0lo;
            // (three ballots, not one over the OR: the compiler then takes each compare's lane mask as it is)
            fast = (__builtin_amdgcn_ballot_w64(fx >= (uint32_t)G.W) | __builtin_amdgcn_ballot_w64(fy >= (uint32_t)G.H_full) |
                    __builtin_amdgcn_ballot_w64(frel >= G.span)) == 0ull;
        }
        if (fast) {
            uint32_t tile, w, z;
            simple_taf_fields_valid(G, fx, fy, (q[j].y >> 28) & 1u, frel, tile, w, z);
            const uint32_t r = atomicAdd(&wcnt[tile], 1u);
            wseen32 |= 1u << z;
            word[j] = w;
            where[j] = (tile << 16) | r;
        } else if (j < G.bpw) {
            const uint32_t i = (uint32_t)(j * kWave + lane);
            if (LEAN) {
                if (nloc > 0) { // wave-uniform: an empty run has loaded nothing
                    int x = (int)(q[j].y & 16383u), y = (int)((q[j].y >> 14) & 16383u);
                    const uint32_t p = (q[j].y >> 28) & 1u;
                    const bool ib = !fast_alias(G, x, y);
                    uint32_t tile, w, z;
                    const bool sb = !simple_taf_fields<!FASTBLK>(G, x, y, p, q[j].x, t0lo, tile, w, z);
                    const bool live = i < nloc, ok = live && !ib && !sb;
                    if (live && !ok) err |= ib ? ST_INDEX : ST_SPAN; // (no lane of a valid call)
                    uint32_t r = 0u;
                    if (ok) {
                        r = atomicAdd(&wcnt[tile], 1u);
                        wseen |= 1ull << z;
                    }
                    where[j] = ok ? (tile << 16) | r : 0xffffffffu;
                    word[j] = w;
                }
            } else if (i < nloc) {
                const FastEv o = fast_decode<HAS_MAP, EV, SIMPLE, SAE>(G, q[j], t0);
                err |= o.err;
                if (o.tile >= 0) {
                    const uint32_t r = atomicAdd(&wcnt[o.tile], 1u);
                    where[j] = ((uint32_t)o.tile << 16) | r;
                    // SAE: the event's position in its sequence + 1 (below 2^20: the host checks; a record is never 0) in place of the time field
                    word[j] = SAE ? ((uint32_t)(wave_begin - S.ev0[s] + (long long)i + 1) << kCellBits) | (o.word & (uint32_t)(kCells - 1)) : o.word;
                    wseen |= 1ull << o.window;
                }
            }
        }
    }
    wseen |= wseen32;
    if (err) atomicOr(&serr, err);
    SPROF(2);
    __syncthreads();
    SPROF(3);
    // ---- phase B: per bin (thread = bin: T <= kFT), exclusive prefix of the 16 wavefront counts; chunk-local offsets of the bins.
    // The prefixes stay in registers until the bin's slot in the staged chunk is known and go back to LDS ONCE, slot included:
    // phase C then reads one table per record
    uint32_t mine = 0; // records of bin `tid` in this chunk
    uint32_t pv[kFW];
    {
        const int b = tid < T ? tid : 0;
#pragma unroll
        for (int w = 0; w < kFW; ++w) {
            pv[w] = mine;
            mine += wcnt_all[(size_t)w * T + b];
        }
        if (tid >= T) mine = 0u;
    }
    const uint32_t inc = wave_incl_scan(mine);
    if (lane == kWave - 1) wtot[wv] = inc;
    __syncthreads();
    uint32_t pre = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kFW; ++k) { if (k < wv) pre += wtot[k]; total += wtot[k]; }
    const uint32_t my_off = pre + inc - mine;
    if (tid < T) {
#pragma unroll
        for (int w = 0; w < kFW; ++w) wcnt_all[(size_t)w * T + tid] = pv[w] + my_off;
        // the directory is BIN-major, dir[bin][chunk] (every chunk writes its entry of all T bins: T scattered 4-byte stores
        // per workgroup): a consumer reads its bin's column as ONE contiguous stretch -- chunk-major rows made every consumer's
        // first step 512 loads from 512 lines (5 of the 30 us of a kf_split_whole workgroup)
        dir[(long long)tid * (long long)gridDim.x + chunk] = (mine << 16) | my_off;
    }
    __syncthreads();
    SPROF(4);
    // ---- phase C: stage the chunk bin-major in LDS
#pragma unroll
    for (int j = 0; j < MAXB; ++j) {
        if (j < G.bpw && where[j] != 0xffffffffu) {
            const uint32_t b = where[j] >> 16;
            stage[wcnt[b] + (where[j] & 0xffffu)] = word[j];
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)wseen, off), hi = __shfl_xor((unsigned)(wseen >> 32), off);
        wseen |= ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 0 && wseen) atomicOr(&wg_seen, wseen);
    __syncthreads();
    SPROF(5);
    // ---- phase D: the staged chunk leaves as it is, one linear sweep into the chunk's own stretch of rec[]
    // (16-byte LDS reads and global stores where both ends are 16-byte aligned -- every chunk of a one-sequence call -- then the
    // last total % 4 words one by one; the layout of rec[] is the same either way)
    uint32_t *dst = records + (chunk_begin - S.ev0[0]);
    uint32_t q4 = 0u;
    if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(stage)) & 15u) == 0u) {
        q4 = total & ~3u;
        for (uint32_t qi = 4u * tid; qi < q4; qi += 4u * kFT) *reinterpret_cast<uint4 *>(dst + qi) = *reinterpret_cast<const uint4 *>(stage + qi);
    }
    for (uint32_t qi = q4 + tid; qi < total; qi += kFT) dst[qi] = stage[qi];
    SPROF(6);
    SPROF_DRAIN();
    SPROF(7);
    SPROF_END();
    if (tid == 0) {
        if (epoch != 0u) {
            // bounded: ~2^22 polls of >= 128 cycles (a fraction of a second; the wait is normally over before it starts).  A part
            // or a scheduler that does not start workgroup 0 first ends the call with ST_STALL (FRLW_ERR_HIP) instead of a hang.
            uint32_t polls = 0u;
            while (__hip_atomic_load(&hdr->epoch, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != epoch) {
                if (++polls > (1u << 22)) break;
                __builtin_amdgcn_s_sleep(2);
            }
            if (polls > (1u << 22)) { // (not hdr->status: a workgroup 0 that starts later would zero it; see kStallOffset)
                atomicExch((uint32_t *)((char *)hdr + kStallOffset), epoch);
                fold_sticky_status(hdr, ST_STALL);
                return;
            }
        }
        const unsigned long long m = wg_seen;
        const unsigned long long have = __hip_atomic_load(&hdr->wmask[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (m & ~have) atomicOr(&hdr->wmask[s], m);
        const int e = serr;
        if (e & ~ST_MULBAD) { atomicOr(&hdr->status, e & ~ST_MULBAD); fold_sticky_status(hdr, e & ~ST_MULBAD); }
        if (e & ST_MULBAD) hdr->mul_bad = 1u; // (every writer stores the same value)
    }
}
} // namespace
