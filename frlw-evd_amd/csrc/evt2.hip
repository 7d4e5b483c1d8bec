// evt2.hip -- Prophesee EVT 2.0 / EVT 2.1 words -> DAT8 event records on the device ("EVT 2.0 and EVT 2.1 decode").
//
// One set of kernels for both encodings.  An EVT 2.0 word (32 bits) has the layout of the UPPER half of an EVT 2.1 word (64 bits):
// type, the low six bits of t, x, y; the lower half of an EVT 2.1 word is a mask of 32 events at x + i, where an EVT 2.0 word
// stands for the single event at x.  So the kernels see every word as (hi, mask) and the template fixes mask = 1 for EVT 2.0.
// The only state a word needs from the words before it is the clock (evt2_state.h), a record that composes associatively, so the
// stream is cut into chunks and decoded by the plan of evt3.hip, in two calls of stream-ordered launches:
//   frlw_evt2_count:  k_evt2_summary<E>   one workgroup per chunk -> the chunk's state record
//                     k_evt2_scan_states  one workgroup: exclusive scan of the chunk records, seeded by the carried-in state
//                     k_evt2_count<E>     one workgroup per chunk, with its carried-in state: what it emits, drops and counts
//                     k_evt2_scan_counts  one workgroup: exclusive scan of the emit counts, the counters, the carried-out state
//   frlw_evt2_emit:   k_evt2_emit<E>      one workgroup per chunk: per-lane state and offsets again, every record written once
// No kernel waits on another workgroup, no atomic decides where a record goes, nothing is staged per chunk: a lane writes its
// records straight to out[offset of its chunk + records of the lanes before it ..].
#include "frlw_common.h"
#include "evt2_state.h"

using namespace frlw;

namespace {
constexpr int kThreads = 256;                          // four wavefronts
constexpr int kWaves = kThreads / kWave;
constexpr int kLaneDwords = 16;                        // a lane's contiguous piece: 64 bytes, four 16-byte loads
constexpr int kScanThreads = 256;                      // the two single-workgroup scans
constexpr long long kMaxWords = 1ll << 31;
static_assert(kWave == 64, "64-lane ballots and shuffles");

template <int E> struct Enc;
template <> struct Enc<FRLW_EVT_20> { static constexpr int kWordDwords = 1; };
template <> struct Enc<FRLW_EVT_21> { static constexpr int kWordDwords = 2; };
template <int E> constexpr int lane_words() { return kLaneDwords / Enc<E>::kWordDwords; }   // 16 / 8 words
template <int E> constexpr int chunk_words() { return kThreads * lane_words<E>(); }         // 4096 / 2048 words = 16 KiB

inline int lane_words_of(int encoding) { return encoding == FRLW_EVT_21 ? lane_words<FRLW_EVT_21>() : lane_words<FRLW_EVT_20>(); }
inline int chunk_words_of(int encoding) { return kThreads * lane_words_of(encoding); }
inline bool known(int encoding) { return encoding == FRLW_EVT_20 || encoding == FRLW_EVT_21; }

enum : int { EVT2_ST_TIME = 1, EVT2_ST_CAPACITY = 2, EVT2_ST_PLAN = 4 };

// what is carried from call to call beside the state record: the t (unshifted) of the last event emitted so far
struct Carry {
    Evt2State s;
    uint32_t has_last_t;
    uint32_t pad;
    unsigned long long last_t;
};

// first kHeaderBytes of the workspace (status first, like every workspace header of the library)
struct Evt2Header {
    int32_t status;
    uint32_t pad;
    Carry out;
    unsigned long long events, before_sync, out_of_frame, triggers, other_words, time_loops, unsorted, first_t, last_t, min_t, max_t;
};
static_assert(sizeof(Evt2Header) <= kHeaderBytes, "header");

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

struct Plan2 {
    Evt2State *sum;    // [n_chunks] the chunk's own record
    Evt2State *pre;    // [n_chunks] the state in front of the chunk
    ChunkCount *cnt;   // [n_chunks]
    unsigned long long *off; // [n_chunks] records emitted in front of the chunk
};

inline long long chunks_of(int encoding, long long n_words)
{
    const long long c = chunk_words_of(encoding);
    return (n_words + c - 1) / c;
}

inline size_t plan_bytes(long long n_chunks)
{
    return (size_t)n_chunks * (2 * sizeof(Evt2State) + sizeof(ChunkCount) + sizeof(unsigned long long));
}

inline Plan2 plan_of(void *ws, long long n_chunks)
{
    Plan2 p;
    char *b = (char *)ws + kHeaderBytes;
    p.cnt = (ChunkCount *)b;               b += (size_t)n_chunks * sizeof(ChunkCount);
    p.off = (unsigned long long *)b;       b += (size_t)n_chunks * sizeof(unsigned long long);
    p.sum = (Evt2State *)b;                b += (size_t)n_chunks * sizeof(Evt2State);
    p.pre = (Evt2State *)b;
    return p;
}

// A record to / from the plan as two 8-byte accesses.
__device__ __forceinline__ void store_state(Evt2State *dst, const Evt2State &s)
{
    uint2 *d = reinterpret_cast<uint2 *>(dst);
    d[0] = make_uint2(s.flags, s.loops);
    d[1] = make_uint2(s.first_high, s.last_high);
}
__device__ __forceinline__ Evt2State load_state(const Evt2State *src)
{
    const uint2 *p = reinterpret_cast<const uint2 *>(src);
    const uint2 a = p[0], b = p[1];
    Evt2State s = {a.x, a.y, b.x, b.y};
    return s;
}

// ---- a lane's piece ------------------------------------------------------------------------------------------------
// 64 bytes in 16 registers.  `words` points at 32-bit units; `first` and `n_words` count words of the encoding.  Words at or beyond
// n_words read as all ones and are never decoded (the return value says how many are real).  aligned: the base pointer is
// 16-byte aligned; else the loads are one word wide (4 bytes for EVT 2.0, 8 for EVT 2.1: the alignment a word pointer has).
template <int E>
__device__ __forceinline__ int load_piece(const uint32_t *words, long long n_words, long long first, bool aligned, uint32_t (&w)[kLaneDwords])
{
    constexpr int kLaneWords = lane_words<E>();
    const long long left = n_words - first;
    const int cnt = left >= kLaneWords ? kLaneWords : (left > 0 ? (int)left : 0);
    const uint32_t *base = words + first * Enc<E>::kWordDwords;
    if (cnt == kLaneWords && aligned) {
        const uint4 *p = reinterpret_cast<const uint4 *>(base);
#pragma unroll
        for (int q = 0; q < kLaneDwords / 4; ++q) {
            const uint4 v = p[q];
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
    } else if (E == FRLW_EVT_21) {
        const uint2 *p = reinterpret_cast<const uint2 *>(base);
#pragma unroll
        for (int k = 0; k < kLaneWords; ++k) {
            const uint2 v = k < cnt ? p[k] : make_uint2(~0u, ~0u);
            w[2 * k] = v.x; w[2 * k + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kLaneWords; ++k) w[k] = k < cnt ? base[k] : ~0u;
    }
    return cnt;
}

// word k of the piece as (upper half, event mask)
template <int E> __device__ __forceinline__ uint32_t hi_of(const uint32_t (&w)[kLaneDwords], int k) { return E == FRLW_EVT_21 ? w[2 * k + 1] : w[k]; }
template <int E> __device__ __forceinline__ uint32_t mask_of(const uint32_t (&w)[kLaneDwords], int k) { return E == FRLW_EVT_21 ? w[2 * k] : 1u; }

template <int E>
__device__ __forceinline__ Evt2State summarise(const uint32_t (&w)[kLaneDwords], int cnt)
{
    Evt2State s = evt2_identity();
#pragma unroll
    for (int k = 0; k < lane_words<E>(); ++k)
        if (k < cnt) evt2_step(s, hi_of<E>(w, k));
    return s;
}

// ---- the workgroup's scan of the lane records ----------------------------------------------------------------------
__device__ __forceinline__ Evt2State shfl_up_state(const Evt2State &s, int d)
{
    Evt2State r;
    r.flags = __shfl_up(s.flags, d, kWave);
    r.loops = __shfl_up(s.loops, d, kWave);
    r.first_high = __shfl_up(s.first_high, d, kWave);
    r.last_high = __shfl_up(s.last_high, d, kWave);
    return r;
}

// Lanes are composed in wavefront order by shuffles, the wavefronts through LDS.  Returns the record of everything in front of
// this lane (seed first); *total = the record of the whole workgroup without the seed.  All kThreads threads call it.
__device__ __forceinline__ Evt2State block_scan_states(const Evt2State &mine, const Evt2State &seed, Evt2State *wave_tot /* LDS [kWaves] */,
                                                       Evt2State *total)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    Evt2State inc = mine;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const Evt2State up = shfl_up_state(inc, d);
        if (lane >= d) inc = evt2_compose(up, inc);
    }
    Evt2State exc = shfl_up_state(inc, 1);
    if (lane == 0) exc = evt2_identity();
    if (lane == kWave - 1) wave_tot[wave] = inc;
    __syncthreads();
    Evt2State before = seed, all = evt2_identity();
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
        const Evt2State t = wave_tot[v];
        if (v < wave) before = evt2_compose(before, t);
        all = evt2_compose(all, t);
    }
    if (total) *total = all;
    return evt2_compose(before, exc);
}

// ---- decoding a piece ----------------------------------------------------------------------------------------------
// The piece decoded from state s (the state in front of the lane's first word).  EMIT: records to out[pos ..], guarded by
// capacity; else the tallies.  The events of one word share their t, so the tallies take a word's events as one step.
template <int E, bool EMIT>
__device__ __forceinline__ void walk(const uint32_t (&w)[kLaneDwords], int cnt, Evt2State s, uint32_t W, uint32_t H, Tally &T, uint2 *out,
                                     unsigned long long pos, unsigned long long shift, unsigned long long capacity)
{
#pragma unroll
    for (int k = 0; k < lane_words<E>(); ++k) {
        if (k < cnt) {
            const uint32_t hi = hi_of<E>(w, k), type = hi >> 28;
            if (type <= EVT2_CD_ON) {
                const uint32_t mask = mask_of<E>(w, k), bits = (uint32_t)__popc(mask);
                if (!(s.flags & EVT2_HAS_HIGH)) {
                    T.before_sync += bits;
                } else {
                    const uint32_t x = (hi >> 11) & 0x7FFu, y = hi & 0x7FFu;
                    // bits whose x + i lies inside the frame
                    const uint32_t room = (y < H && x < W) ? W - x : 0u;
                    uint32_t in = room >= 32u ? mask : mask & ((1u << room) - 1u);
                    const uint32_t n_in = (uint32_t)__popc(in);
                    T.out_of_frame += bits - n_in;
                    const unsigned long long t = evt2_time(s, hi >> 22);
                    if (EMIT) {
                        const uint32_t tw = (uint32_t)(t - shift), yp = (y << 14) | (type << 28);
                        unsigned long long at = pos + T.n;
                        while (in) {
                            const uint32_t i = (uint32_t)__ffs((int)in) - 1u;
                            in &= in - 1u;
                            if (at < capacity) out[at] = make_uint2(tw, (x + i) | yp);
                            ++at;
                        }
                    } else if (n_in) {
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
                    T.n += n_in;
                }
            } else if (type == EVT2_TIME_HIGH) {
                evt2_time_high(s, hi & 0x0FFFFFFFu);
            } else if (type == EVT2_EXT_TRIGGER) {
                T.triggers += 1u;
            } else {
                T.other_words += 1u;
            }
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
template <int E>
__global__ __launch_bounds__(kThreads) void k_evt2_summary(const uint32_t *words, long long n_words, int aligned, Evt2State *sum)
{
    __shared__ Evt2State wave_tot[kWaves];
    const long long chunk = blockIdx.x;
    uint32_t w[kLaneDwords];
    const int cnt = load_piece<E>(words, n_words, chunk * chunk_words<E>() + (long long)threadIdx.x * lane_words<E>(), aligned != 0, w);
    Evt2State total;
    block_scan_states(summarise<E>(w, cnt), evt2_identity(), wave_tot, &total);
    if (threadIdx.x == 0) store_state(sum + chunk, total);
}

// ---- launch 2: exclusive scan of the chunk records -----------------------------------------------------------------
// One workgroup: a thread composes a contiguous range of chunks, the kScanThreads range records are scanned like the lane records
// of a chunk, every thread walks its range again with its carried-in state.
__global__ __launch_bounds__(kScanThreads) void k_evt2_scan_states(const Evt2State *sum, Evt2State *pre, long long n_chunks, uint32_t seed_flags,
                                                                 uint32_t seed_loops, uint32_t seed_first_high, uint32_t seed_last_high,
                                                                 Evt2Header *hdr)
{
    const Evt2State seed = {seed_flags, seed_loops, seed_first_high, seed_last_high};
    __shared__ Evt2State wave_tot[kWaves];
    static_assert(kScanThreads == kThreads, "block_scan_states scans kThreads records");
    const long long per = (n_chunks + kScanThreads - 1) / kScanThreads;
    const long long lo = per * threadIdx.x < n_chunks ? per * threadIdx.x : n_chunks;
    const long long hi = lo + per < n_chunks ? lo + per : n_chunks;
    Evt2State s = evt2_identity();
    for (long long c = lo; c < hi; ++c) s = evt2_compose(s, load_state(sum + c));
    Evt2State total;
    s = block_scan_states(s, seed, wave_tot, &total);
    if (threadIdx.x == 0) store_state(&hdr->out.s, evt2_compose(seed, total));
    for (long long c = lo; c < hi; ++c) {
        store_state(pre + c, s);
        s = evt2_compose(s, load_state(sum + c));
    }
}

// ---- launch 3: what each chunk emits and drops ---------------------------------------------------------------------
template <int E>
__global__ __launch_bounds__(kThreads) void k_evt2_count(const uint32_t *words, long long n_words, int aligned, uint32_t W, uint32_t H,
                                                         const Evt2State *pre, ChunkCount *out)
{
    __shared__ Evt2State wave_tot[kWaves];
    __shared__ unsigned long long s_last[kThreads];
    __shared__ unsigned long long s_ball[kWaves];
    __shared__ uint32_t s_part[kWaves][6];
    __shared__ unsigned long long s_ext[kWaves][4]; // first_t, last_t, min_t, max_t of a wavefront
    const long long chunk = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t w[kLaneDwords];
    const int cnt = load_piece<E>(words, n_words, chunk * chunk_words<E>() + (long long)threadIdx.x * lane_words<E>(), aligned != 0, w);
    const Evt2State s = block_scan_states(summarise<E>(w, cnt), load_state(pre + chunk), wave_tot, nullptr);
    Tally T = {};
    walk<E, false>(w, cnt, s, W, H, T, nullptr, 0ull, 0ull, 0ull);

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

__global__ __launch_bounds__(kScanThreads) void k_evt2_scan_counts(const ChunkCount *cnt, unsigned long long *off, long long n_chunks,
                                                                 Carry in, Evt2Header *hdr)
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
        hdr->time_loops = (unsigned long long)(hdr->out.s.loops - in.s.loops); // (out.s: k_evt2_scan_states, the launch before)
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
template <int E>
__global__ __launch_bounds__(kThreads) void k_evt2_emit(const uint32_t *words, long long n_words, int aligned, uint32_t W, uint32_t H,
                                                        const Evt2State *pre, const ChunkCount *cnt, const unsigned long long *off,
                                                        Evt2Header *hdr, uint2 *out, unsigned long long capacity, int time_shift)
{
    __shared__ Evt2State wave_tot[kWaves];
    __shared__ uint32_t s_wave_n[kWaves];
    const long long chunk = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    // refusals that hold for the whole call: every workgroup reads the same header and takes the same way out
    const unsigned long long events = hdr->events;
    const unsigned long long shift = (time_shift && (hdr->out.s.flags & EVT2_HAS_HIGH)) ? (unsigned long long)hdr->out.s.first_high << 6 : 0ull;
    int refuse = 0;
    if (events && (hdr->min_t < shift || hdr->max_t - shift > 0xFFFFFFFFull)) refuse |= EVT2_ST_TIME;
    if (events > capacity) refuse |= EVT2_ST_CAPACITY;
    if (refuse) {
        if (chunk == 0 && threadIdx.x == 0) atomicOr(&hdr->status, refuse);
        return;
    }
    const ChunkCount mine = cnt[chunk];
    if (mine.n == 0u) return;
    uint32_t w[kLaneDwords];
    const int n_real = load_piece<E>(words, n_words, chunk * chunk_words<E>() + (long long)threadIdx.x * lane_words<E>(), aligned != 0, w);
    const Evt2State s = block_scan_states(summarise<E>(w, n_real), load_state(pre + chunk), wave_tot, nullptr);
    Tally T = {};
    walk<E, false>(w, n_real, s, W, H, T, nullptr, 0ull, 0ull, 0ull);
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
        if (threadIdx.x == 0) atomicOr(&hdr->status, EVT2_ST_PLAN);
        return;
    }
    Tally E2 = {};
    walk<E, true>(w, n_real, s, W, H, E2, out, off[chunk] + before + (inc - T.n), shift, capacity);
}

int status_code2(int st)
{
    if (st & EVT2_ST_TIME) return FRLW_ERR_SPAN;
    if (st & EVT2_ST_CAPACITY) return FRLW_ERR_ARG;
    if (st & EVT2_ST_PLAN) return FRLW_ERR_HIP;
    return FRLW_OK;
}

int check_common(int encoding, const void *words, long long n_words, int width, int height, const void *workspace, size_t workspace_bytes)
{
    if (!known(encoding) || !workspace || n_words < 0 || n_words > kMaxWords || (!words && n_words > 0)) return FRLW_ERR_ARG;
    if ((uintptr_t)words & (encoding == FRLW_EVT_21 ? 7u : 3u)) return FRLW_ERR_ARG; // a word pointer is aligned to its words
    if (width < 1 || width > 2048 || height < 1 || height > 2048) return FRLW_ERR_ARG;
    if (workspace_bytes < frlw_evt2_workspace_bytes(encoding, n_words)) return FRLW_ERR_WORKSPACE;
    return FRLW_OK;
}

template <int E>
void launch_count(const uint32_t *words, long long n_words, int aligned, uint32_t W, uint32_t H, const Plan2 &p, long long n_chunks,
                  const Carry &in, Evt2Header *hdr, hipStream_t s)
{
    if (n_chunks) hipLaunchKernelGGL(k_evt2_summary<E>, dim3((unsigned)n_chunks), dim3(kThreads), 0, s, words, n_words, aligned, p.sum);
    hipLaunchKernelGGL(k_evt2_scan_states, dim3(1), dim3(kScanThreads), 0, s, p.sum, p.pre, n_chunks, in.s.flags, in.s.loops,
                       in.s.first_high, in.s.last_high, hdr);
    if (n_chunks) hipLaunchKernelGGL(k_evt2_count<E>, dim3((unsigned)n_chunks), dim3(kThreads), 0, s, words, n_words, aligned, W, H, p.pre, p.cnt);
    hipLaunchKernelGGL(k_evt2_scan_counts, dim3(1), dim3(kScanThreads), 0, s, p.cnt, p.off, n_chunks, in, hdr);
}
} // namespace

extern "C" {

size_t frlw_evt2_workspace_bytes(int encoding, int64_t n_words)
{
    if (!known(encoding) || n_words < 0 || n_words > kMaxWords) return 0;
    return kHeaderBytes + align_up(plan_bytes(chunks_of(encoding, n_words)), 256);
}

int frlw_evt2_geometry(int encoding, int *chunk_words, int *lane_words)
{
    if (!known(encoding) || !chunk_words || !lane_words) return FRLW_ERR_ARG;
    *chunk_words = chunk_words_of(encoding);
    *lane_words = lane_words_of(encoding);
    return FRLW_OK;
}

int frlw_evt2_count(int encoding, const void *words, int64_t n_words, int width, int height, const frlw_evt2_state_t *state_in,
                    void *workspace, size_t workspace_bytes, frlw_stream_t stream)
{
    if (const int rc = check_common(encoding, words, n_words, width, height, workspace, workspace_bytes)) return rc;
    if (state_in && state_in->struct_size != (int32_t)sizeof(frlw_evt2_state_t)) return FRLW_ERR_ARG;
    static_assert(sizeof(frlw_evt2_state_t) == 8 + sizeof(Carry), "frlw_evt2_state_t = struct_size + the carry");
    Carry in = {};
    in.s = evt2_identity();
    if (state_in) {
        in.s.flags = state_in->flags & EVT2_HAS_HIGH; in.s.loops = state_in->loops; in.s.first_high = state_in->first_high;
        in.s.last_high = state_in->last_high;
        in.has_last_t = state_in->has_last_t ? 1u : 0u;
        in.last_t = state_in->last_t;
    }
    const long long n_chunks = chunks_of(encoding, n_words);
    const Plan2 p = plan_of(workspace, n_chunks);
    const int aligned = ((uintptr_t)words & 15u) == 0;
    if (encoding == FRLW_EVT_21)
        launch_count<FRLW_EVT_21>((const uint32_t *)words, n_words, aligned, (uint32_t)width, (uint32_t)height, p, n_chunks, in,
                                  (Evt2Header *)workspace, (hipStream_t)stream);
    else
        launch_count<FRLW_EVT_20>((const uint32_t *)words, n_words, aligned, (uint32_t)width, (uint32_t)height, p, n_chunks, in,
                                  (Evt2Header *)workspace, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}

int frlw_evt2_emit(int encoding, const void *words, int64_t n_words, int width, int height, void *workspace, size_t workspace_bytes,
                   void *out, int64_t capacity, int time_shift, frlw_stream_t stream)
{
    if (const int rc = check_common(encoding, words, n_words, width, height, workspace, workspace_bytes)) return rc;
    if (capacity < 0 || (!out && capacity > 0)) return FRLW_ERR_ARG;
    const long long n_chunks = chunks_of(encoding, n_words);
    if (!n_chunks) return FRLW_OK;
    const Plan2 p = plan_of(workspace, n_chunks);
    const int aligned = ((uintptr_t)words & 15u) == 0;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(workspace, 0, sizeof(int32_t), s)); // the status is this emit's alone
    if (encoding == FRLW_EVT_21)
        hipLaunchKernelGGL(k_evt2_emit<FRLW_EVT_21>, dim3((unsigned)n_chunks), dim3(kThreads), 0, s, (const uint32_t *)words, (long long)n_words,
                           aligned, (uint32_t)width, (uint32_t)height, p.pre, p.cnt, p.off, (Evt2Header *)workspace, (uint2 *)out,
                           (unsigned long long)capacity, time_shift ? 1 : 0);
    else
        hipLaunchKernelGGL(k_evt2_emit<FRLW_EVT_20>, dim3((unsigned)n_chunks), dim3(kThreads), 0, s, (const uint32_t *)words, (long long)n_words,
                           aligned, (uint32_t)width, (uint32_t)height, p.pre, p.cnt, p.off, (Evt2Header *)workspace, (uint2 *)out,
                           (unsigned long long)capacity, time_shift ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}

int frlw_evt2_result(const void *workspace, frlw_stream_t stream, frlw_evt3_counters_t *counters, frlw_evt2_state_t *state_out,
                     int *status_out)
{
    if (!workspace || !counters || counters->struct_size != (int32_t)sizeof(frlw_evt3_counters_t)) return FRLW_ERR_ARG;
    if (state_out && state_out->struct_size != (int32_t)sizeof(frlw_evt2_state_t)) return FRLW_ERR_ARG;
    Evt2Header h;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(&h, workspace, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    counters->events = h.events; counters->before_sync = h.before_sync; counters->out_of_frame = h.out_of_frame;
    counters->triggers = h.triggers; counters->other_words = h.other_words; counters->time_loops = h.time_loops;
    counters->unsorted = h.unsorted; counters->first_t = h.first_t; counters->last_t = h.last_t;
    counters->min_t = h.min_t; counters->max_t = h.max_t;
    if (state_out) {
        state_out->flags = h.out.s.flags; state_out->loops = h.out.s.loops; state_out->first_high = h.out.s.first_high;
        state_out->last_high = h.out.s.last_high; state_out->has_last_t = h.out.has_last_t; state_out->last_t = h.out.last_t;
    }
    if (status_out) *status_out = status_code2(h.status);
    return FRLW_OK;
}

} // extern "C"
