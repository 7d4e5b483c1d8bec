// evt_plan.h -- the chunked count-and-emit plan the EVT decoders share ("EVT 3.0 decode": the plan as built).
//
// A decoder whose state after a run of words is a record that composes associatively (evt3_state.h, evt2_state.h) cuts its stream
// into chunks of 16 KiB and decodes it in two calls of stream-ordered launches:
//   count<C>:  k_evt_summary<C>        one workgroup per chunk -> the chunk's state record
//              k_evt_scan_states<Ops>  one workgroup: exclusive scan of the chunk records, seeded by the carried-in state
//              k_evt_count<C>          one workgroup per chunk, with its carried-in state: what it emits, drops and counts
//              k_evt_scan_counts<S>    one workgroup: exclusive scan of the emit counts, the counters, the carried-out state
//   emit<C>:   k_evt_emit<C>           one workgroup per chunk: per-lane state and offsets again, every record written once
// No kernel waits on another workgroup, no atomic decides where a record goes, nothing is staged per chunk: a lane writes its
// records straight to out[offset of its chunk + records of the lanes before it ..].
//
// Everything here is the plan's; what an encoding adds is a codec C (evt3.hip, evt2.hip):
//   C::Ops        the state: Ops::State (alignas(8), 32-bit fields only, among them flags, loops, first_high), Ops::identity(),
//                 Ops::compose(a, b), Ops::kHasHigh (the flag "a TIME_HIGH was seen"), Ops::kShiftBits (time shift = first_high << it)
//   C::Word       what the words pointer points at; C::kLaneWords words of the encoding make a lane's 64-byte piece
//   C::load_piece(words, n_words, first, aligned, w) -> how many of the piece's words are real
//   C::summarise(w, cnt) -> the piece's state record
//   C::walk<EMIT>(w, cnt, s, W, H, T, out, pos, shift, capacity)   the piece decoded from state s: EMIT: records to out[pos ..],
//                 guarded by capacity; else the tallies
// This header is included by more than one translation unit: all of it has internal linkage.
#pragma once
#include "frlw_common.h"

namespace frlw {
namespace {
constexpr int kThreads = 256;                          // four wavefronts
constexpr int kWaves = kThreads / kWave;
constexpr int kLaneDwords = 16;                        // a lane's contiguous piece: 64 bytes, four 16-byte loads
constexpr int kScanThreads = 256;                      // the two single-workgroup scans
constexpr long long kMaxWords = 1ll << 31;
static_assert(kWave == 64, "64-lane ballots and shuffles");

enum : int { EVT_ST_TIME = 1, EVT_ST_CAPACITY = 2, EVT_ST_PLAN = 4 };

// what is carried from call to call beside the state record: the t (unshifted) of the last event emitted so far
template <class S> struct Carry {
    S s;
    uint32_t has_last_t;
    uint32_t pad;
    unsigned long long last_t;
};

// first kHeaderBytes of the workspace (status first, like every workspace header of the library)
template <class S> struct EvtHeader {
    int32_t status;
    uint32_t pad;
    Carry<S> out;
    unsigned long long events, before_sync, out_of_frame, triggers, other_words, time_loops, unsorted, first_t, last_t, min_t, max_t;
};

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

template <class S> struct Plan {
    S *sum;            // [n_chunks] the chunk's own record
    S *pre;            // [n_chunks] the state in front of the chunk
    ChunkCount *cnt;   // [n_chunks]
    unsigned long long *off; // [n_chunks] records emitted in front of the chunk
};

template <class C> constexpr int chunk_words() { return kThreads * C::kLaneWords; }     // 16 KiB per workgroup
template <class C> inline long long chunks_of(long long n_words) { return (n_words + chunk_words<C>() - 1) / chunk_words<C>(); }

template <class S> inline size_t plan_bytes(long long n_chunks)
{
    return (size_t)n_chunks * (2 * sizeof(S) + sizeof(ChunkCount) + sizeof(unsigned long long));
}

template <class S> inline Plan<S> plan_of(void *ws, long long n_chunks)
{
    Plan<S> p;
    char *b = (char *)ws + kHeaderBytes;
    p.cnt = (ChunkCount *)b;               b += (size_t)n_chunks * sizeof(ChunkCount);
    p.off = (unsigned long long *)b;       b += (size_t)n_chunks * sizeof(unsigned long long);
    p.sum = (S *)b;                        b += (size_t)n_chunks * sizeof(S);
    p.pre = (S *)b;
    return p;
}

// ---- a state record as its 32-bit fields ---------------------------------------------------------------------------
template <class S> struct Fields {
    static_assert(alignof(S) == 8 && sizeof(S) % 8 == 0, "a state record: pairs of 32-bit fields");
    uint32_t f[sizeof(S) / 4];
};

// A record to / from the plan as 8-byte accesses (a struct assignment in a loop goes through scratch).
template <class S> __device__ __forceinline__ void store_state(S *dst, const S &s)
{
    const Fields<S> v = __builtin_bit_cast(Fields<S>, s);
    uint2 *d = reinterpret_cast<uint2 *>(dst);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(S) / 8); ++i) d[i] = make_uint2(v.f[2 * i], v.f[2 * i + 1]);
}
template <class S> __device__ __forceinline__ S load_state(const S *src)
{
    const uint2 *p = reinterpret_cast<const uint2 *>(src);
    Fields<S> v;
#pragma unroll
    for (int i = 0; i < (int)(sizeof(S) / 8); ++i) {
        const uint2 a = p[i];
        v.f[2 * i] = a.x; v.f[2 * i + 1] = a.y;
    }
    return __builtin_bit_cast(S, v);
}

// ---- the workgroup's scan of the lane records ----------------------------------------------------------------------
template <class S> __device__ __forceinline__ S shfl_up_state(const S &s, int d)
{
    Fields<S> v = __builtin_bit_cast(Fields<S>, s);
#pragma unroll
    for (int i = 0; i < (int)(sizeof(S) / 4); ++i) v.f[i] = __shfl_up(v.f[i], d, kWave);
    return __builtin_bit_cast(S, v);
}

// Lanes are composed in wavefront order by shuffles, the wavefronts through LDS.  Returns the record of everything in front of
// this lane (seed first); *total = the record of the whole workgroup without the seed.  All kThreads threads call it.
template <class Ops>
__device__ __forceinline__ typename Ops::State block_scan_states(const typename Ops::State &mine, const typename Ops::State &seed,
                                                                 typename Ops::State *wave_tot /* LDS [kWaves] */, typename Ops::State *total)
{
    using S = typename Ops::State;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    S inc = mine;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const S up = shfl_up_state(inc, d);
        if (lane >= d) inc = Ops::compose(up, inc);
    }
    S exc = shfl_up_state(inc, 1);
    if (lane == 0) exc = Ops::identity();
    if (lane == kWave - 1) wave_tot[wave] = inc;
    __syncthreads();
    S before = seed, all = Ops::identity();
#pragma unroll
    for (int v = 0; v < kWaves; ++v) {
        const S t = wave_tot[v];
        if (v < wave) before = Ops::compose(before, t);
        all = Ops::compose(all, t);
    }
    if (total) *total = all;
    return Ops::compose(before, exc);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kWave);
    return v;
}

// ---- launch 1: the chunk's state record ----------------------------------------------------------------------------
template <class C, class S = typename C::Ops::State>
__global__ __launch_bounds__(kThreads) void k_evt_summary(const typename C::Word *words, long long n_words, int aligned, S *sum)
{
    __shared__ S wave_tot[kWaves];
    const long long chunk = blockIdx.x;
    uint32_t w[kLaneDwords];
    const int cnt = C::load_piece(words, n_words, chunk * chunk_words<C>() + (long long)threadIdx.x * C::kLaneWords, aligned != 0, w);
    S total;
    block_scan_states<typename C::Ops>(C::summarise(w, cnt), C::Ops::identity(), wave_tot, &total);
    if (threadIdx.x == 0) store_state(sum + chunk, total);
}

// ---- launch 2: exclusive scan of the chunk records -----------------------------------------------------------------
// One workgroup: a thread composes a contiguous range of chunks, the kScanThreads range records are scanned like the lane records
// of a chunk, every thread walks its range again with its carried-in state.  The seed is in.s: the carry by value, as
// k_evt_scan_counts takes it, costs no scratch (tests/test_evt*_cpu.py read the compiler's resource remarks).
template <class Ops, class S = typename Ops::State>
__global__ __launch_bounds__(kScanThreads) void k_evt_scan_states(const S *sum, S *pre, long long n_chunks, Carry<S> in, EvtHeader<S> *hdr)
{
    const S seed = in.s;
    __shared__ S wave_tot[kWaves];
    static_assert(kScanThreads == kThreads, "block_scan_states scans kThreads records");
    const long long per = (n_chunks + kScanThreads - 1) / kScanThreads;
    const long long lo = per * threadIdx.x < n_chunks ? per * threadIdx.x : n_chunks;
    const long long hi = lo + per < n_chunks ? lo + per : n_chunks;
    S s = Ops::identity();
    for (long long c = lo; c < hi; ++c) s = Ops::compose(s, load_state(sum + c));
    S total;
    s = block_scan_states<Ops>(s, seed, wave_tot, &total);
    if (threadIdx.x == 0) store_state(&hdr->out.s, Ops::compose(seed, total));
    for (long long c = lo; c < hi; ++c) {
        store_state(pre + c, s);
        s = Ops::compose(s, load_state(sum + c));
    }
}

// ---- launch 3: what each chunk emits and drops ---------------------------------------------------------------------
template <class C, class S = typename C::Ops::State>
__global__ __launch_bounds__(kThreads) void k_evt_count(const typename C::Word *words, long long n_words, int aligned, uint32_t W, uint32_t H,
                                                        const S *pre, ChunkCount *out)
{
    __shared__ S wave_tot[kWaves];
    __shared__ unsigned long long s_last[kThreads];
    __shared__ unsigned long long s_ball[kWaves];
    __shared__ uint32_t s_part[kWaves][6];
    __shared__ unsigned long long s_ext[kWaves][4]; // first_t, last_t, min_t, max_t of a wavefront
    const long long chunk = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t w[kLaneDwords];
    const int cnt = C::load_piece(words, n_words, chunk * chunk_words<C>() + (long long)threadIdx.x * C::kLaneWords, aligned != 0, w);
    const S s = block_scan_states<typename C::Ops>(C::summarise(w, cnt), load_state(pre + chunk), wave_tot, nullptr);
    Tally T = {};
    C::template walk<false>(w, cnt, s, W, H, T, nullptr, 0ull, 0ull, 0ull);

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

template <class S>
__global__ __launch_bounds__(kScanThreads) void k_evt_scan_counts(const ChunkCount *cnt, unsigned long long *off, long long n_chunks, Carry<S> in,
                                                                  EvtHeader<S> *hdr)
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
        hdr->time_loops = (unsigned long long)(hdr->out.s.loops - in.s.loops); // (out.s: k_evt_scan_states, the launch before)
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
template <class C, class S = typename C::Ops::State>
__global__ __launch_bounds__(kThreads) void k_evt_emit(const typename C::Word *words, long long n_words, int aligned, uint32_t W, uint32_t H,
                                                       const S *pre, const ChunkCount *cnt, const unsigned long long *off, EvtHeader<S> *hdr,
                                                       uint2 *out, unsigned long long capacity, int time_shift)
{
    __shared__ S wave_tot[kWaves];
    __shared__ uint32_t s_wave_n[kWaves];
    const long long chunk = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    // refusals that hold for the whole call: every workgroup reads the same header and takes the same way out
    const unsigned long long events = hdr->events;
    const unsigned long long shift =
        (time_shift && (hdr->out.s.flags & C::Ops::kHasHigh)) ? (unsigned long long)hdr->out.s.first_high << C::Ops::kShiftBits : 0ull;
    int refuse = 0;
    if (events && (hdr->min_t < shift || hdr->max_t - shift > 0xFFFFFFFFull)) refuse |= EVT_ST_TIME;
    if (events > capacity) refuse |= EVT_ST_CAPACITY;
    if (refuse) {
        if (chunk == 0 && threadIdx.x == 0) atomicOr(&hdr->status, refuse);
        return;
    }
    const ChunkCount mine = cnt[chunk];
    if (mine.n == 0u) return;
    uint32_t w[kLaneDwords];
    const int n_real = C::load_piece(words, n_words, chunk * chunk_words<C>() + (long long)threadIdx.x * C::kLaneWords, aligned != 0, w);
    const S s = block_scan_states<typename C::Ops>(C::summarise(w, n_real), load_state(pre + chunk), wave_tot, nullptr);
    Tally T = {};
    C::template walk<false>(w, n_real, s, W, H, T, nullptr, 0ull, 0ull, 0ull);
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
        if (threadIdx.x == 0) atomicOr(&hdr->status, EVT_ST_PLAN);
        return;
    }
    Tally E = {};
    C::template walk<true>(w, n_real, s, W, H, E, out, off[chunk] + before + (inc - T.n), shift, capacity);
}

// ---- the host side -------------------------------------------------------------------------------------------------
inline int status_code(int st)
{
    if (st & EVT_ST_TIME) return FRLW_ERR_SPAN;
    if (st & EVT_ST_CAPACITY) return FRLW_ERR_ARG;
    if (st & EVT_ST_PLAN) return FRLW_ERR_HIP;
    return FRLW_OK;
}

template <class C> inline size_t workspace_bytes(long long n_words)
{
    if (n_words < 0 || n_words > kMaxWords) return 0;
    return kHeaderBytes + align_up(plan_bytes<typename C::Ops::State>(chunks_of<C>(n_words)), 256);
}

template <class C> inline int check_common(const void *words, long long n_words, int width, int height, const void *workspace, size_t ws_bytes)
{
    if (!workspace || n_words < 0 || n_words > kMaxWords || (!words && n_words > 0)) return FRLW_ERR_ARG;
    if (width < 1 || width > 2048 || height < 1 || height > 2048) return FRLW_ERR_ARG;
    if (ws_bytes < workspace_bytes<C>(n_words)) return FRLW_ERR_WORKSPACE;
    return FRLW_OK;
}

// The count call: four launches that leave the plan, the counters and the carried-out state in the workspace.  The caller has
// passed the arguments through check_common and checked its own state_in behind that, so a workspace that is too small is
// reported before a state_in of the wrong size.
template <class C, class S = typename C::Ops::State>
inline int count(const void *words, long long n_words, int width, int height, const Carry<S> &in, void *workspace, frlw_stream_t stream)
{
    static_assert(sizeof(EvtHeader<S>) <= kHeaderBytes, "header");
    const typename C::Word *wp = (const typename C::Word *)words;
    hipStream_t s = (hipStream_t)stream;
    const long long n_chunks = chunks_of<C>(n_words);
    const Plan<S> p = plan_of<S>(workspace, n_chunks);
    EvtHeader<S> *hdr = (EvtHeader<S> *)workspace;
    const int aligned = ((uintptr_t)words & 15u) == 0;
    if (n_chunks) hipLaunchKernelGGL(k_evt_summary<C>, dim3((unsigned)n_chunks), dim3(kThreads), 0, s, wp, n_words, aligned, p.sum);
    hipLaunchKernelGGL(k_evt_scan_states<typename C::Ops>, dim3(1), dim3(kScanThreads), 0, s, p.sum, p.pre, n_chunks, in, hdr);
    if (n_chunks)
        hipLaunchKernelGGL(k_evt_count<C>, dim3((unsigned)n_chunks), dim3(kThreads), 0, s, wp, n_words, aligned, (uint32_t)width,
                           (uint32_t)height, p.pre, p.cnt);
    hipLaunchKernelGGL(k_evt_scan_counts<S>, dim3(1), dim3(kScanThreads), 0, s, p.cnt, p.off, n_chunks, in, hdr);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}

// The emit call: one launch on the same words and the plan the count call left.
template <class C, class S = typename C::Ops::State>
inline int emit(const void *words, long long n_words, int width, int height, void *workspace, size_t ws_bytes, void *out, int64_t capacity,
                int time_shift, frlw_stream_t stream)
{
    if (const int rc = check_common<C>(words, n_words, width, height, workspace, ws_bytes)) return rc;
    if (capacity < 0 || (!out && capacity > 0)) return FRLW_ERR_ARG;
    const long long n_chunks = chunks_of<C>(n_words);
    if (!n_chunks) return FRLW_OK;
    const Plan<S> p = plan_of<S>(workspace, n_chunks);
    const int aligned = ((uintptr_t)words & 15u) == 0;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(workspace, 0, sizeof(int32_t), s)); // the status is this emit's alone
    hipLaunchKernelGGL(k_evt_emit<C>, dim3((unsigned)n_chunks), dim3(kThreads), 0, s, (const typename C::Word *)words, n_words, aligned,
                       (uint32_t)width, (uint32_t)height, p.pre, p.cnt, p.off, (EvtHeader<S> *)workspace, (uint2 *)out,
                       (unsigned long long)capacity, time_shift ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return FRLW_OK;
}

// Synchronises the stream; the counters, the carried-out state (carry may be null) and the status of the last emit to the host.
template <class S> inline int result(const void *workspace, frlw_stream_t stream, frlw_evt3_counters_t *counters, Carry<S> *carry, int *status_out)
{
    if (!workspace || !counters || counters->struct_size != (int32_t)sizeof(frlw_evt3_counters_t)) return FRLW_ERR_ARG;
    EvtHeader<S> h;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(&h, workspace, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    counters->events = h.events; counters->before_sync = h.before_sync; counters->out_of_frame = h.out_of_frame;
    counters->triggers = h.triggers; counters->other_words = h.other_words; counters->time_loops = h.time_loops;
    counters->unsorted = h.unsorted; counters->first_t = h.first_t; counters->last_t = h.last_t;
    counters->min_t = h.min_t; counters->max_t = h.max_t;
    if (carry) *carry = h.out;
    if (status_out) *status_out = status_code(h.status);
    return FRLW_OK;
}

} // namespace
} // namespace frlw
