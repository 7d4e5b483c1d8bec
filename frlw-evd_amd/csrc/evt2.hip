// evt2.hip -- Prophesee EVT 2.0 / EVT 2.1 words -> DAT8 event records on the device ("EVT 2.0 and EVT 2.1 decode").
//
// One codec template for both encodings.  An EVT 2.0 word (32 bits) has the layout of the UPPER half of an EVT 2.1 word (64 bits):
// type, the low six bits of t, x, y; the lower half of an EVT 2.1 word is a mask of 32 events at x + i, where an EVT 2.0 word
// stands for the single event at x.  So the codec sees every word as (hi, mask) and the template fixes mask = 1 for EVT 2.0.
// The only state a word needs from the words before it is the clock (evt2_state.h), a record that composes associatively, so the
// stream is cut into chunks and decoded by the chunked count-and-emit plan of evt_plan.h: its five kernels, its workspace and its
// host drivers.  This file holds what is EVT 2.x's own: the codec (a lane's piece of 16 / 8 words, the piece's state record, the
// walk that takes a word's events as one step) and the frlw_evt2_* entry points.
#include "evt_plan.h"
#include "evt2_state.h"

using namespace frlw;

namespace {
struct Evt2Ops {
    using State = Evt2State;
    static constexpr uint32_t kHasHigh = EVT2_HAS_HIGH;
    static constexpr int kShiftBits = 6;
    static __host__ __device__ __forceinline__ State identity() { return evt2_identity(); }
    static __host__ __device__ __forceinline__ State compose(const State &a, const State &b) { return evt2_compose(a, b); }
};

template <int E> struct Evt2Codec {
    static_assert(E == FRLW_EVT_20 || E == FRLW_EVT_21, "EVT 2.0 or EVT 2.1");
    using Ops = Evt2Ops;
    using Word = uint32_t;                                 // the words pointer counts 32-bit units
    static constexpr int kWordDwords = E == FRLW_EVT_21 ? 2 : 1;
    static constexpr int kLaneWords = kLaneDwords / kWordDwords;                        // 16 / 8 words: 4096 / 2048 words a chunk

    // ---- a lane's piece --------------------------------------------------------------------------------------------
    // 64 bytes in 16 registers.  `words` points at 32-bit units; `first` and `n_words` count words of the encoding.  Words at or
    // beyond n_words read as all ones and are never decoded (the return value says how many are real).  aligned: the base pointer
    // is 16-byte aligned; else the loads are one word wide (4 bytes for EVT 2.0, 8 for EVT 2.1: the alignment a word pointer has).
    static __device__ __forceinline__ int load_piece(const uint32_t *words, long long n_words, long long first, bool aligned,
                                                     uint32_t (&w)[kLaneDwords])
    {
        const long long left = n_words - first;
        const int cnt = left >= kLaneWords ? kLaneWords : (left > 0 ? (int)left : 0);
        const uint32_t *base = words + first * kWordDwords;
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
    static __device__ __forceinline__ uint32_t hi_of(const uint32_t (&w)[kLaneDwords], int k) { return E == FRLW_EVT_21 ? w[2 * k + 1] : w[k]; }
    static __device__ __forceinline__ uint32_t mask_of(const uint32_t (&w)[kLaneDwords], int k) { return E == FRLW_EVT_21 ? w[2 * k] : 1u; }

    static __device__ __forceinline__ Evt2State summarise(const uint32_t (&w)[kLaneDwords], int cnt)
    {
        Evt2State s = evt2_identity();
#pragma unroll
        for (int k = 0; k < kLaneWords; ++k)
            if (k < cnt) evt2_step(s, hi_of(w, k));
        return s;
    }

    // ---- decoding a piece ------------------------------------------------------------------------------------------
    // The piece decoded from state s (the state in front of the lane's first word).  EMIT: records to out[pos ..], guarded by
    // capacity; else the tallies.  The events of one word share their t, so the tallies take a word's events as one step.
    template <bool EMIT>
    static __device__ __forceinline__ void walk(const uint32_t (&w)[kLaneDwords], int cnt, Evt2State s, uint32_t W, uint32_t H, Tally &T,
                                                uint2 *out, unsigned long long pos, unsigned long long shift, unsigned long long capacity)
    {
#pragma unroll
        for (int k = 0; k < kLaneWords; ++k) {
            if (k < cnt) {
                const uint32_t hi = hi_of(w, k), type = hi >> 28;
                if (type <= EVT2_CD_ON) {
                    const uint32_t mask = mask_of(w, k), bits = (uint32_t)__popc(mask);
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
};

inline bool known(int encoding) { return encoding == FRLW_EVT_20 || encoding == FRLW_EVT_21; }

// f(codec of `encoding`), for an encoding that is known()
template <class F> inline auto with_codec(int encoding, F f)
{
    return encoding == FRLW_EVT_21 ? f(Evt2Codec<FRLW_EVT_21>()) : f(Evt2Codec<FRLW_EVT_20>());
}

// what the shared argument check does not know: the encoding, and that a word pointer is aligned to its words
inline int check_encoding(int encoding, const void *words)
{
    if (!known(encoding) || ((uintptr_t)words & (encoding == FRLW_EVT_21 ? 7u : 3u))) return FRLW_ERR_ARG;
    return FRLW_OK;
}
} // namespace

extern "C" {

size_t frlw_evt2_workspace_bytes(int encoding, int64_t n_words)
{
    if (!known(encoding)) return 0;
    return with_codec(encoding, [&](auto c) { return workspace_bytes<decltype(c)>(n_words); });
}

int frlw_evt2_geometry(int encoding, int *chunk_words_out, int *lane_words)
{
    if (!known(encoding) || !chunk_words_out || !lane_words) return FRLW_ERR_ARG;
    *lane_words = with_codec(encoding, [](auto c) { return decltype(c)::kLaneWords; });
    *chunk_words_out = kThreads * *lane_words;
    return FRLW_OK;
}

int frlw_evt2_count(int encoding, const void *words, int64_t n_words, int width, int height, const frlw_evt2_state_t *state_in,
                    void *workspace, size_t workspace_bytes, frlw_stream_t stream)
{
    if (const int rc = check_encoding(encoding, words)) return rc;
    return with_codec(encoding, [&](auto c) {
        using C = decltype(c);
        if (const int rc = check_common<C>(words, n_words, width, height, workspace, workspace_bytes)) return rc;
        if (state_in && state_in->struct_size != (int32_t)sizeof(frlw_evt2_state_t)) return (int)FRLW_ERR_ARG;
        static_assert(sizeof(frlw_evt2_state_t) == 8 + sizeof(Carry<Evt2State>), "frlw_evt2_state_t = struct_size + the carry");
        Carry<Evt2State> in = {};
        in.s = evt2_identity();
        if (state_in) {
            in.s.flags = state_in->flags & EVT2_HAS_HIGH; in.s.loops = state_in->loops; in.s.first_high = state_in->first_high;
            in.s.last_high = state_in->last_high;
            in.has_last_t = state_in->has_last_t ? 1u : 0u;
            in.last_t = state_in->last_t;
        }
        return count<C>(words, n_words, width, height, in, workspace, stream);
    });
}

int frlw_evt2_emit(int encoding, const void *words, int64_t n_words, int width, int height, void *workspace, size_t workspace_bytes,
                   void *out, int64_t capacity, int time_shift, frlw_stream_t stream)
{
    if (const int rc = check_encoding(encoding, words)) return rc;
    return with_codec(encoding, [&](auto c) {
        return emit<decltype(c)>(words, n_words, width, height, workspace, workspace_bytes, out, capacity, time_shift, stream);
    });
}

int frlw_evt2_result(const void *workspace, frlw_stream_t stream, frlw_evt3_counters_t *counters, frlw_evt2_state_t *state_out,
                     int *status_out)
{
    if (state_out && state_out->struct_size != (int32_t)sizeof(frlw_evt2_state_t)) return FRLW_ERR_ARG;
    Carry<Evt2State> c;
    if (const int rc = result<Evt2State>(workspace, stream, counters, &c, status_out)) return rc;
    if (state_out) {
        state_out->flags = c.s.flags; state_out->loops = c.s.loops; state_out->first_high = c.s.first_high;
        state_out->last_high = c.s.last_high; state_out->has_last_t = c.has_last_t; state_out->last_t = c.last_t;
    }
    return FRLW_OK;
}

} // extern "C"
