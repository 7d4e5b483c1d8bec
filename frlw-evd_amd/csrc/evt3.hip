// evt3.hip -- Prophesee EVT 3.0 words -> DAT8 event records on the device ("EVT 3.0 decode").
//
// The decoder is a sequential state machine; evt3_state.h states its state as a record that composes associatively, so the
// stream is cut into chunks of kChunkWords words and decoded in two calls of stream-ordered launches:
//   frlw_evt3_count:  k_evt3_summary      one workgroup per chunk -> the chunk's state record
//                     k_evt3_scan_states  one workgroup: exclusive scan of the chunk records, seeded by the carried-in state
//                     k_evt3_count        one workgroup per chunk, with its carried-in state: what it emits, drops and counts
//                     k_evt3_scan_counts  one workgroup: exclusive scan of the emit counts, the counters, the carried-out state
//   frlw_evt3_emit:   k_evt3_emit         one workgroup per chunk: per-lane state and offsets again, every record written once
// No kernel waits on another workgroup, no atomic decides where a record goes, nothing is staged per chunk: a lane writes its
// records straight to out[offset of its chunk + records of the lanes before it ..].
#include "frlw_common.h"
#include "evt3_state.h"

using namespace frlw;

namespace {
constexpr int kThreads = 256;                          // four wavefronts
constexpr int kWaves = kThreads / kWave;
constexpr int kLaneWords = 32;                         // a lane's contiguous piece: four 16-byte loads
constexpr int kLaneDwords = kLaneWords / 2;
constexpr int kChunkWords = kThreads * kLaneWords;     // 8192 words = 16 KiB per workgroup
constexpr int kScanThreads = 256;                      // the two single-workgroup scans
constexpr long long kMaxWords = 1ll << 31;
static_assert(kWave == 64, "64-lane ballots and shuffles");

enum : int { EVT3_ST_TIME = 1, EVT3_ST_CAPACITY = 2, EVT3_ST_PLAN = 4 };

// what is carried from call to call beside the state record: the t (unshifted) of the last event emitted so far
struct Carry {
    Evt3State s;
    uint32_t has_last_t;
    uint32_t pad;
    unsigned long long last_t;
};

// first kHeaderBytes of the workspace (status first, like every workspace header of the library)
struct Evt3Header {
    int32_t status;
    uint32_t pad;
    Carry out;
    unsigned long long events, before_sync, out_of_frame, triggers, other_words, time_loops, unsorted, first_t, last_t, min_t, max_t;
};
static_assert(sizeof(Evt3Header) <= kHeaderBytes, "header");

// what one chunk emits and drops, decoded with its carried-in state
struct ChunkCount {
    uint32_t n, has;                                   // records emitted; has: n != 0
    uint32_t before_sync, out_of_frame, triggers, other_words, unsorted, pad;
    unsigned long long first_t, last_t, min_t, max_t;  // unshifted; valid when has
};

struct Tally {
    uint32_t n, before_sync, out_of_frame, triggers, other_words, unsorted, has;
    unsigned long long first_t, last_t, min_t, max_t;
};

struct Plan3 {
    Evt3State *sum;    // [n_chunks] the chunk's own record
    Evt3State *pre;    // [n_chunks] the state in front of the chunk
    ChunkCount *cnt;   // [n_chunks]
    unsigned long long *off; // [n_chunks] records emitted in front of the chunk
};

__host__ __device__ inline long long chunks_of(long long n_words) { return (n_words + kChunkWords - 1) / kChunkWords; }

inline size_t plan_bytes(long long n_chunks)
{
    return (size_t)n_chunks * (2 * sizeof(Evt3State) + sizeof(ChunkCount) + sizeof(unsigned long long));
}

inline Plan3 plan_of(void *ws, long long n_chunks)
{
    Plan3 p;
    char *b = (char *)ws + kHeaderBytes;
    p.cnt = (ChunkCount *)b;               b += (size_t)n_chunks * sizeof(ChunkCount);
    p.off = (unsigned long long *)b;       b += (size_t)n_chunks * sizeof(unsigned long long);
    p.sum = (Evt3State *)b;                b += (size_t)n_chunks * sizeof(Evt3State);
    p.pre = (Evt3State *)b;
    return p;
}

// A record to / from the plan as three 8-byte accesses (a struct assignment in a loop goes through scratch).
__device__ __forceinline__ void store_state(Evt3State *dst, const Evt3State &s)
{
    uint2 *d = reinterpret_cast<uint2 *>(dst);
    d[0] = make_uint2(s.flags, s.loops);
    d[1] = make_uint2(s.first_high, s.last_high);
    d[2] = make_uint2(s.low_y, s.base);
}
__device__ __forceinline__ Evt3State load_state(const Evt3State *src)
{
    const uint2 *p = reinterpret_cast<const uint2 *>(src);
    const uint2 a = p[0], b = p[1], c = p[2];
    Evt3State s = {a.x, a.y, b.x, b.y, c.x, c.y};
    return s;
}

// ---- a lane's piece ------------------------------------------------------------------------------------------------
// 32 words in 16 registers; words at or beyond n_words read as 0xFFFF and are never decoded (cnt says how many are real).
__device__ __forceinline__ int load_piece(const uint16_t *words, long long n_words, long long first, bool aligned, uint32_t (&w)[kLaneDwords])
{
    const long long left = n_words - first;
    const int cnt = left >= kLaneWords ? kLaneWords : (left > 0 ? (int)left : 0);
    if (cnt == kLaneWords && aligned) {
        const uint4 *p = reinterpret_cast<const uint4 *>(words + first);
#pragma unroll
        for (int q = 0; q < kLaneDwords / 4; ++q) {
            const uint4 v = p[q];
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kLaneDwords; ++k) {
            const uint32_t lo = 2 * k < cnt ? (uint32_t)words[first + 2 * k] : 0xFFFFu;
            const uint32_t hi = 2 * k + 1 < cnt ? (uint32_t)words[first + 2 * k + 1] : 0xFFFFu;
            w[k] = lo | (hi << 16);
        }
    }
    return cnt;
}

__device__ __forceinline__ uint32_t word_of(const uint32_t (&w)[kLaneDwords], int k) { return (w[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu; }

__device__ __forceinline__ Evt3State summarise(const uint32_t (&w)[kLaneDwords], int cnt)
{
    Evt3State s = evt3_identity();
#pragma unroll
    for (int k = 0; k < kLaneWords; ++k)
        if (k < cnt) evt3_step(s, word_of(w, k));
    return s;
}

// ---- the workgroup's scan of the lane records ----------------------------------------------------------------------
__device__ __forceinline__ Evt3State shfl_up_state(const Evt3State &s, int d)
{
    Evt3State r;
    r.flags = __shfl_up(s.flags, d, kWave);
    r.loops = __shfl_up(s.loops, d, kWave);
    r.first_high = __shfl_up(s.first_high, d, kWave);
    r.last_high = __shfl_up(s.last_high, d, kWave);
    r.low_y = __shfl_up(s.low_y, d, kWave);
    r.base = __shfl_up(s.base, d, kWave);
    return r;
}

// Lanes are composed in wavefront order by shuffles, the wavefronts through LDS.  Returns the record of everything in front of
// this lane (seed first); *total = the record of the whole workgroup without the seed.  All kThreads threads call it.
__device__ __forceinline__ Evt3State block_scan_states(const Evt3State &mine, const Evt3State &seed, Evt3State *wave_tot /* LDS [kWaves] */,
                                                       Evt3State *total)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    Evt3State inc = mine;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const Evt3State up = shfl_up_state(inc, d);
        if (lane >= d) inc = evt3_compose(up, inc);
    }
    Evt3State exc = shfl_up_state(inc, 1);
    if (lane == 0) exc = evt3_identity();
    if (lane == kWave - 1) wave_tot[wave] = inc;
    __syncthreads();
    Evt3State before = seed, all = evt3_identity();
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
        const Evt3State t = wave_tot[v];
        if (v < wave) before = evt3_compose(before, t);
        all = evt3_compose(all, t);
    }
    if (total) *total = all;
    return evt3_compose(before, exc);
}

// ---- decoding a piece ----------------------------------------------------------------------------------------------
template <bool EMIT>
__device__ __forceinline__ void one_event(Tally &T, const Evt3State &s, uint32_t x, uint32_t p, uint2 *out, unsigned long long pos,
                                          unsigned long long shift, unsigned long long capacity)
{
    const unsigned long long t = evt3_time(s);
    if (EMIT) {
        const unsigned long long at = pos + T.n;
        if (at < capacity) out[at] = make_uint2((uint32_t)(t - shift), x | (evt3_y(s) << 14) | (p << 28));
    } else {
        if (T.has) {
            T.unsorted += t < T.last_t ? 1u : 0u;
            T.min_t = t < T.min_t ? t : T.min_t;
            T.max_t = t > T.max_t ? t : T.max_t;
        } else {
            T.first_t = T.min_t = T.max_t = t;
            T.has = 1u;
        }
        T.last_t = t;
    }
    T.n += 1u;
}

// The piece decoded from state s (the state in front of the lane's first word).  EMIT: records to out[pos ..], guarded by
// capacity; else the tallies.
template <bool EMIT>
__device__ __forceinline__ void walk(const uint32_t (&w)[kLaneDwords], int cnt, Evt3State s, uint32_t W, uint32_t H, Tally &T, uint2 *out,
                                     unsigned long long pos, unsigned long long shift, unsigned long long capacity)
{
    constexpr uint32_t kSync = EVT3_HAS_HIGH | EVT3_HAS_Y;
#pragma unroll
    for (int k = 0; k < kLaneWords; ++k) {
        if (k < cnt) {
            const uint32_t word = word_of(w, k), type = word >> 12;
            if (type == EVT3_ADDR_X) {
                const uint32_t x = word & 0x7FFu;
                if ((s.flags & kSync) != kSync) T.before_sync += 1u;
                else if (x >= W || evt3_y(s) >= H) T.out_of_frame += 1u;
                else one_event<EMIT>(T, s, x, (word >> 11) & 1u, out, pos, shift, capacity);
            } else if (type == EVT3_VECT_12 || type == EVT3_VECT_8) {
                const uint32_t width = type == EVT3_VECT_12 ? 12u : 8u;
                const uint32_t mask = word & ((1u << width) - 1u);
                const uint32_t bits = (uint32_t)__popc(mask);
                if ((s.flags & (kSync | EVT3_HAS_BASE)) != (kSync | EVT3_HAS_BASE)) {
                    T.before_sync += bits;
                } else {
                    // bits whose x = base + i lies inside the frame
                    const uint32_t room = (evt3_y(s) < H && s.base < W) ? (W - s.base < width ? W - s.base : width) : 0u;
                    uint32_t in = mask & ((1u << room) - 1u);
                    T.out_of_frame += bits - (uint32_t)__popc(in);
                    const uint32_t p = (s.flags & EVT3_VP) ? 1u : 0u;
                    while (in) {
                        const uint32_t i = (uint32_t)__ffs((int)in) - 1u;
                        in &= in - 1u;
                        one_event<EMIT>(T, s, s.base + i, p, out, pos, shift, capacity);
                    }
                }
            } else if (type == EVT3_EXT_TRIGGER) {
                T.triggers += 1u;
            } else if (type != EVT3_ADDR_Y && type != EVT3_VECT_BASE_X && type != EVT3_TIME_LOW && type != EVT3_TIME_HIGH) {
                T.other_words += 1u;
            }
            evt3_step(s, word);
        }
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kWave);
    return v;
}

// ---- launch 1: the chunk's state record ----------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_evt3_summary(const uint16_t *words, long long n_words, int aligned, Evt3State *sum)
{
    __shared__ Evt3State wave_tot[kWaves];
    const long long chunk = blockIdx.x;
    uint32_t w[kLaneDwords];
    const int cnt = load_piece(words, n_words, chunk * kChunkWords + (long long)threadIdx.x * kLaneWords, aligned != 0, w);
    Evt3State total;
    block_scan_states(summarise(w, cnt), evt3_identity(), wave_tot, &total);
    if (threadIdx.x == 0) store_state(sum + chunk, total);
}

// ---- launch 2: exclusive scan of the chunk records -----------------------------------------------------------------
// One workgroup: a thread composes a contiguous range of chunks, the kScanThreads range records are scanned like the lane records
// of a chunk, every thread walks its range again with its carried-in state.
__global__ __launch_bounds__(kScanThreads) void k_evt3_scan_states(const Evt3State *sum, Evt3State *pre, long long n_chunks, uint32_t seed_flags,
                                                                 uint32_t seed_loops, uint32_t seed_first_high, uint32_t seed_last_high,
                                                                 uint32_t seed_low_y, uint32_t seed_base, Evt3Header *hdr)
{
    const Evt3State seed = {seed_flags, seed_loops, seed_first_high, seed_last_high, seed_low_y, seed_base}; // (a struct argument costs scratch)
    __shared__ Evt3State wave_tot[kWaves];
    static_assert(kScanThreads == kThreads, "block_scan_states scans kThreads records");
    const long long per = (n_chunks + kScanThreads - 1) / kScanThreads;
    const long long lo = per * threadIdx.x < n_chunks ? per * threadIdx.x : n_chunks;
    const long long hi = lo + per < n_chunks ? lo + per : n_chunks;
    Evt3State s = evt3_identity();
    for (long long c = lo; c < hi; ++c) s = evt3_compose(s, load_state(sum + c));
    Evt3State total;
    s = block_scan_states(s, seed, wave_tot, &total);
    if (threadIdx.x == 0) store_state(&hdr->out.s, evt3_compose(seed, total));
    for (long long c = lo; c < hi; ++c) {
        store_state(pre + c, s);
        s = evt3_compose(s, load_state(sum + c));
    }
}

// ---- launch 3: what each chunk emits and drops ---------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_evt3_count(const uint16_t *words, long long n_words, int aligned, uint32_t W, uint32_t H,
                                                         const Evt3State *pre, ChunkCount *out)
{
    __shared__ Evt3State wave_tot[kWaves];
    __shared__ unsigned long long s_last[kThreads];
    __shared__ unsigned long long s_ball[kWaves];
    __shared__ uint32_t s_part[kWaves][6];
    __shared__ unsigned long long s_ext[kWaves][4]; // first_t, last_t, min_t, max_t of a wavefront
    const long long chunk = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t w[kLaneDwords];
    const int cnt = load_piece(words, n_words, chunk * kChunkWords + (long long)threadIdx.x * kLaneWords, aligned != 0, w);
    const Evt3State s = block_scan_states(summarise(w, cnt), load_state(pre + chunk), wave_tot, nullptr);
    Tally T = {};
    walk<false>(w, cnt, s, W, H, T, nullptr, 0ull, 0ull, 0ull);

    // the lane in front of this one that emitted something: one more unsorted event where its last t is larger
    const unsigned long long ball = __ballot(T.has != 0u);
    s_last[threadIdx.x] = T.last_t;
    if (lane == 0) s_ball[wave] = ball;
    __syncthreads();
    if (T.has) {
        int prev = -1;
        unsigned long long m = ball & lanemask_lt();
        for (int v = wave; v >= 0 && prev < 0; --v) {
            if (m) prev = v * kWave + 63 - __clzll((long long)m);
            else if (v > 0) m = s_ball[v - 1];
        }
        if (prev >= 0 && T.first_t < s_last[prev]) T.unsorted += 1u;
    }
    // sums, and the wavefront's first / last / min / max
    const uint32_t sums[5] = {wave_sum(T.n), wave_sum(T.before_sync), wave_sum(T.out_of_frame), wave_sum(T.triggers), wave_sum(T.other_words)};
    const uint32_t uns = wave_sum(T.unsorted);
    unsigned long long mn = T.has ? T.min_t : ~0ull, mx = T.has ? T.max_t : 0ull;
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const unsigned long long a = __shfl_xor(mn, d, kWave), b = __shfl_xor(mx, d, kWave);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    const int first_lane = ball ? __ffsll((long long)ball) - 1 : 0, last_lane = ball ? 63 - __clzll((long long)ball) : 0;
    const unsigned long long ft = __shfl(T.first_t, first_lane, kWave), lt = __shfl(T.last_t, last_lane, kWave);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 5; ++j) s_part[wave][j] = sums[j];
        s_ext[wave][0] = ft; s_ext[wave][1] = lt; s_ext[wave][2] = mn; s_ext[wave][3] = mx;
        s_part[wave][5] = uns;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ChunkCount c = {};
        c.min_t = ~0ull;
        bool seen = false;
        for (int v = 0; v < kWaves; ++v) {
            c.n += s_part[v][0]; c.before_sync += s_part[v][1]; c.out_of_frame += s_part[v][2]; c.triggers += s_part[v][3];
            c.other_words += s_part[v][4]; c.unsorted += s_part[v][5];
            if (s_ball[v]) {
                if (!seen) c.first_t = s_ext[v][0];
                seen = true;
                c.last_t = s_ext[v][1];
                c.min_t = s_ext[v][2] < c.min_t ? s_ext[v][2] : c.min_t;
                c.max_t = s_ext[v][3] > c.max_t ? s_ext[v][3] : c.max_t;
            }
        }
        c.has = seen ? 1u : 0u;
        if (!seen) c.min_t = 0ull;
        out[chunk] = c;
    }
}

// ---- launch 4: offsets, counters, the carried-out state ------------------------------------------------------------
struct RangeCount {
    unsigned long long n, before_sync, out_of_frame, triggers, other_words, unsorted, first_t, last_t, min_t, max_t;
    uint32_t has;
};

__device__ __forceinline__ void fold(RangeCount &r, unsigned long long n, unsigned long long bs, unsigned long long oof, unsigned long long tr,
                                     unsigned long long ow, unsigned long long uns, uint32_t has, unsigned long long ft,
                                     unsigned long long lt, unsigned long long mn, unsigned long long mx)
{
    r.n += n; r.before_sync += bs; r.out_of_frame += oof; r.triggers += tr; r.other_words += ow; r.unsorted += uns;
    if (has) {
        if (r.has) {
            r.unsorted += ft < r.last_t ? 1ull : 0ull;
            r.min_t = mn < r.min_t ? mn : r.min_t;
            r.max_t = mx > r.max_t ? mx : r.max_t;
        } else {
            r.first_t = ft; r.min_t = mn; r.max_t = mx;
            r.has = 1u;
        }
        r.last_t = lt;
    }
}

__global__ __launch_bounds__(kScanThreads) void k_evt3_scan_counts(const ChunkCount *cnt, unsigned long long *off, long long n_chunks,
                                                                 Carry in, Evt3Header *hdr)
{
    __shared__ RangeCount part[kScanThreads];
    __shared__ unsigned long long start[kScanThreads];
    const long long per = (n_chunks + kScanThreads - 1) / kScanThreads;
    const long long lo = per * threadIdx.x < n_chunks ? per * threadIdx.x : n_chunks;
    const long long hi = lo + per < n_chunks ? lo + per : n_chunks;
    RangeCount r = {};
    for (long long c = lo; c < hi; ++c) {
        const ChunkCount k = cnt[c];
        fold(r, k.n, k.before_sync, k.out_of_frame, k.triggers, k.other_words, k.unsorted, k.has, k.first_t, k.last_t, k.min_t, k.max_t);
    }
    part[threadIdx.x] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        RangeCount all = {};
        // the call's own first event is compared with the last one of the calls before it, but first_t / min_t / max_t are
        // this call's alone
        unsigned long long boundary = 0ull;
        for (int i = 0; i < kScanThreads; ++i) {
            const RangeCount t = part[i];
            start[i] = all.n;
            if (t.has && !all.has && in.has_last_t && t.first_t < in.last_t) boundary += 1ull;
            fold(all, t.n, t.before_sync, t.out_of_frame, t.triggers, t.other_words, t.unsorted, t.has, t.first_t, t.last_t, t.min_t, t.max_t);
        }
        hdr->status = 0;
        hdr->events = all.n; hdr->before_sync = all.before_sync; hdr->out_of_frame = all.out_of_frame; hdr->triggers = all.triggers;
        hdr->other_words = all.other_words; hdr->unsorted = all.unsorted + boundary;
        hdr->time_loops = (unsigned long long)(hdr->out.s.loops - in.s.loops); // (out.s: k_evt3_scan_states, the launch before)
        hdr->first_t = all.has ? all.first_t : 0ull; hdr->last_t = all.has ? all.last_t : 0ull;
        hdr->min_t = all.has ? all.min_t : 0ull; hdr->max_t = all.has ? all.max_t : 0ull;
        hdr->out.has_last_t = (all.has || in.has_last_t) ? 1u : 0u;
        hdr->out.pad = 0u;
        hdr->out.last_t = all.has ? all.last_t : in.last_t;
    }
    __syncthreads();
    unsigned long long at = start[threadIdx.x];
    for (long long c = lo; c < hi; ++c) {
        off[c] = at;
        at += cnt[c].n;
    }
}

// ---- the emit launch -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_evt3_emit(const uint16_t *words, long long n_words, int aligned, uint32_t W, uint32_t H,
                                                        const Evt3State *pre, const ChunkCount *cnt, const unsigned long long *off,
                                                        Evt3Header *hdr, uint2 *out, unsigned long long capacity, int time_shift)
{
    __shared__ Evt3State wave_tot[kWaves];
    __shared__ uint32_t s_wave_n[kWaves];
    const long long chunk = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    // refusals that hold for the whole call: every workgroup reads the same header and takes the same way out
    const unsigned long long events = hdr->events;
    const unsigned long long shift = (time_shift && (hdr->out.s.flags & EVT3_HAS_HIGH)) ? (unsigned long long)hdr->out.s.first_high << 12 : 0ull;
    int refuse = 0;
    if (events && (hdr->min_t < shift || hdr->max_t - shift > 0xFFFFFFFFull)) refuse |= EVT3_ST_TIME;
    if (events > capacity) refuse |= EVT3_ST_CAPACITY;
    if (refuse) {
        if (chunk == 0 && threadIdx.x == 0) atomicOr(&hdr->status, refuse);
        return;
    }
    const ChunkCount mine = cnt[chunk];
    if (mine.n == 0u) return;
    uint32_t w[kLaneDwords];
    const int n_real = load_piece(words, n_words, chunk * kChunkWords + (long long)threadIdx.x * kLaneWords, aligned != 0, w);
    const Evt3State s = block_scan_states(summarise(w, n_real), load_state(pre + chunk), wave_tot, nullptr);
    Tally T = {};
    walk<false>(w, n_real, s, W, H, T, nullptr, 0ull, 0ull, 0ull);
    const uint32_t inc = wave_incl_scan(T.n);
    if (lane == kWave - 1) s_wave_n[wave] = inc;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
        const uint32_t t = s_wave_n[v];
        before += v < wave ? t : 0u;
        total += t;
    }
    if (total != mine.n) { // the plan of the count call does not fit these words: write nothing
        if (threadIdx.x == 0) atomicOr(&hdr->status, EVT3_ST_PLAN);
        return;
    }
    Tally E = {};
    walk<true>(w, n_real, s, W, H, E, out, off[chunk] + before + (inc - T.n), shift, capacity);
}

int status_code3(int st)
{
    if (st & EVT3_ST_TIME) return FRLW_ERR_SPAN;
    if (st & EVT3_ST_CAPACITY) return FRLW_ERR_ARG;
    if (st & EVT3_ST_PLAN) return FRLW_ERR_HIP;
    return FRLW_OK;
}

int check_common(const void *words, long long n_words, int width, int height, const void *workspace, size_t workspace_bytes)
{
    if (!workspace || n_words < 0 || n_words > kMaxWords || (!words && n_words > 0)) return FRLW_ERR_ARG;
    if (width < 1 || width > 2048 || height < 1 || height > 2048) return FRLW_ERR_ARG;
    if (workspace_bytes < frlw_evt3_workspace_bytes(n_words)) return FRLW_ERR_WORKSPACE;
    return FRLW_OK;
}
} // namespace

extern "C" {

size_t frlw_evt3_workspace_bytes(int64_t n_words)
{
    if (n_words < 0 || n_words > kMaxWords) return 0;
    return kHeaderBytes + align_up(plan_bytes(chunks_of(n_words)), 256);
}

int frlw_evt3_geometry(int *chunk_words, int *lane_words)
{
    if (!chunk_words || !lane_words) return FRLW_ERR_ARG;
    *chunk_words = kChunkWords;
    *lane_words = kLaneWords;
    return FRLW_OK;
}

int frlw_evt3_count(const uint16_t *words, int64_t n_words, int width, int height, const frlw_evt3_state_t *state_in, void *workspace,
                    size_t workspace_bytes, frlw_stream_t stream)
{
    if (const int rc = check_common(words, n_words, width, height, workspace, workspace_bytes)) return rc;
    if (state_in && state_in->struct_size != (int32_t)sizeof(frlw_evt3_state_t)) return FRLW_ERR_ARG;
    static_assert(sizeof(frlw_evt3_state_t) == 8 + sizeof(Carry), "frlw_evt3_state_t = struct_size + the carry");
    Carry in = {};
    in.s = evt3_identity();
    if (state_in) {
        in.s.flags = state_in->flags; in.s.loops = state_in->loops; in.s.first_high = state_in->first_high;
        in.s.last_high = state_in->last_high; in.s.low_y = state_in->low_y; in.s.base = state_in->base;
        in.has_last_t = state_in->has_last_t ? 1u : 0u;
        in.last_t = state_in->last_t;
    }
    hipStream_t s = (hipStream_t)stream;
    const long long n_chunks = chunks_of(n_words);
    const Plan3 p = plan_of(workspace, n_chunks);
    Evt3Header *hdr = (Evt3Header *)workspace;
    const int aligned = ((uintptr_t)words & 15u) == 0;
    if (n_chunks) hipLaunchKernelGGL(k_evt3_summary, dim3((unsigned)n_chunks), dim3(kThreads), 0, s, words, (long long)n_words, aligned, p.sum);
    hipLaunchKernelGGL(k_evt3_scan_states, dim3(1), dim3(kScanThreads), 0, s, p.sum, p.pre, n_chunks, in.s.flags, in.s.loops,
                       in.s.first_high, in.s.last_high, in.s.low_y, in.s.base, hdr);
    if (n_chunks)
        hipLaunchKernelGGL(k_evt3_count, dim3((unsigned)n_chunks), dim3(kThreads), 0, s, words, (long long)n_words, aligned, (uint32_t)width,
                           (uint32_t)height, p.pre, p.cnt);
    hipLaunchKernelGGL(k_evt3_scan_counts, dim3(1), dim3(kScanThreads), 0, s, p.cnt, p.off, n_chunks, in, hdr);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}

int frlw_evt3_emit(const uint16_t *words, int64_t n_words, int width, int height, void *workspace, size_t workspace_bytes, void *out,
                   int64_t capacity, int time_shift, frlw_stream_t stream)
{
    if (const int rc = check_common(words, n_words, width, height, workspace, workspace_bytes)) return rc;
    if (capacity < 0 || (!out && capacity > 0)) return FRLW_ERR_ARG;
    const long long n_chunks = chunks_of(n_words);
    if (!n_chunks) return FRLW_OK;
    const Plan3 p = plan_of(workspace, n_chunks);
    const int aligned = ((uintptr_t)words & 15u) == 0;
    HIP_TRY(hipMemsetAsync(workspace, 0, sizeof(int32_t), (hipStream_t)stream)); // the status is this emit's alone
    hipLaunchKernelGGL(k_evt3_emit, dim3((unsigned)n_chunks), dim3(kThreads), 0, (hipStream_t)stream, words, (long long)n_words, aligned,
                       (uint32_t)width, (uint32_t)height, p.pre, p.cnt, p.off, (Evt3Header *)workspace, (uint2 *)out,
                       (unsigned long long)capacity, time_shift ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}

int frlw_evt3_result(const void *workspace, frlw_stream_t stream, frlw_evt3_counters_t *counters, frlw_evt3_state_t *state_out,
                     int *status_out)
{
    if (!workspace || !counters || counters->struct_size != (int32_t)sizeof(frlw_evt3_counters_t)) return FRLW_ERR_ARG;
    if (state_out && state_out->struct_size != (int32_t)sizeof(frlw_evt3_state_t)) return FRLW_ERR_ARG;
    Evt3Header h;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(&h, workspace, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    counters->events = h.events; counters->before_sync = h.before_sync; counters->out_of_frame = h.out_of_frame;
    counters->triggers = h.triggers; counters->other_words = h.other_words; counters->time_loops = h.time_loops;
    counters->unsorted = h.unsorted; counters->first_t = h.first_t; counters->last_t = h.last_t;
    counters->min_t = h.min_t; counters->max_t = h.max_t;
    if (state_out) {
        state_out->flags = h.out.s.flags; state_out->loops = h.out.s.loops; state_out->first_high = h.out.s.first_high;
        state_out->last_high = h.out.s.last_high; state_out->low_y = h.out.s.low_y; state_out->base = h.out.s.base;
        state_out->has_last_t = h.out.has_last_t; state_out->last_t = h.out.last_t;
    }
    if (status_out) *status_out = status_code3(h.status);
    return FRLW_OK;
}

} // extern "C"
