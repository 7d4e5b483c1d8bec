// evt3.hip -- Prophesee EVT 3.0 words -> DAT8 event records on the device ("EVT 3.0 decode").
//
// The decoder is a sequential state machine; evt3_state.h states its state as a record that composes associatively, so the
// stream is cut into chunks and decoded by the chunked count-and-emit plan of evt_plan.h: its five kernels, its workspace and its
// host drivers.  This file holds what is EVT 3.0's own: the codec (a lane's piece of 32 words, the piece's state record, the
// word-by-word walk that emits or tallies) and the frlw_evt3_* entry points.
#include "evt_plan.h"
#include "evt3_state.h"

using namespace frlw;

namespace {
struct Evt3Codec {
    struct Ops {
        using State = Evt3State;
        static constexpr uint32_t kHasHigh = EVT3_HAS_HIGH;
        static constexpr int kShiftBits = 12;
        static __host__ __device__ __forceinline__ State identity() { return evt3_identity(); }
        static __host__ __device__ __forceinline__ State compose(const State &a, const State &b) { return evt3_compose(a, b); }
    };
    using Word = uint16_t;
    static constexpr int kLaneWords = 32;                  // a lane's contiguous piece: four 16-byte loads
    static_assert(kLaneWords == 2 * kLaneDwords, "two words a register");

    // ---- a lane's piece --------------------------------------------------------------------------------------------
    // 32 words in 16 registers; words at or beyond n_words read as 0xFFFF and are never decoded (cnt says how many are real).
    static __device__ __forceinline__ int load_piece(const uint16_t *words, long long n_words, long long first, bool aligned,
                                                     uint32_t (&w)[kLaneDwords])
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

    static __device__ __forceinline__ uint32_t word_of(const uint32_t (&w)[kLaneDwords], int k) { return (w[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu; }

    static __device__ __forceinline__ Evt3State summarise(const uint32_t (&w)[kLaneDwords], int cnt)
    {
        Evt3State s = evt3_identity();
#pragma unroll
        for (int k = 0; k < kLaneWords; ++k)
            if (k < cnt) evt3_step(s, word_of(w, k));
        return s;
    }

    // ---- decoding a piece ------------------------------------------------------------------------------------------
    template <bool EMIT>
    static __device__ __forceinline__ void one_event(Tally &T, const Evt3State &s, uint32_t x, uint32_t p, uint2 *out, unsigned long long pos,
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
    static __device__ __forceinline__ void walk(const uint32_t (&w)[kLaneDwords], int cnt, Evt3State s, uint32_t W, uint32_t H, Tally &T,
                                                uint2 *out, unsigned long long pos, unsigned long long shift, unsigned long long capacity)
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
};
} // namespace

extern "C" {

size_t frlw_evt3_workspace_bytes(int64_t n_words) { return workspace_bytes<Evt3Codec>(n_words); }

int frlw_evt3_geometry(int *chunk_words_out, int *lane_words)
{
    if (!chunk_words_out || !lane_words) return FRLW_ERR_ARG;
    *chunk_words_out = chunk_words<Evt3Codec>();
    *lane_words = Evt3Codec::kLaneWords;
    return FRLW_OK;
}

int frlw_evt3_count(const uint16_t *words, int64_t n_words, int width, int height, const frlw_evt3_state_t *state_in, void *workspace,
                    size_t workspace_bytes, frlw_stream_t stream)
{
    if (const int rc = check_common<Evt3Codec>(words, n_words, width, height, workspace, workspace_bytes)) return rc;
    if (state_in && state_in->struct_size != (int32_t)sizeof(frlw_evt3_state_t)) return FRLW_ERR_ARG;
    static_assert(sizeof(frlw_evt3_state_t) == 8 + sizeof(Carry<Evt3State>), "frlw_evt3_state_t = struct_size + the carry");
    Carry<Evt3State> in = {};
    in.s = evt3_identity();
    if (state_in) {
        in.s.flags = state_in->flags; in.s.loops = state_in->loops; in.s.first_high = state_in->first_high;
        in.s.last_high = state_in->last_high; in.s.low_y = state_in->low_y; in.s.base = state_in->base;
        in.has_last_t = state_in->has_last_t ? 1u : 0u;
        in.last_t = state_in->last_t;
    }
    return count<Evt3Codec>(words, n_words, width, height, in, workspace, stream);
}

int frlw_evt3_emit(const uint16_t *words, int64_t n_words, int width, int height, void *workspace, size_t workspace_bytes, void *out,
                   int64_t capacity, int time_shift, frlw_stream_t stream)
{
    return emit<Evt3Codec>(words, n_words, width, height, workspace, workspace_bytes, out, capacity, time_shift, stream);
}

int frlw_evt3_result(const void *workspace, frlw_stream_t stream, frlw_evt3_counters_t *counters, frlw_evt3_state_t *state_out,
                     int *status_out)
{
    if (state_out && state_out->struct_size != (int32_t)sizeof(frlw_evt3_state_t)) return FRLW_ERR_ARG;
    Carry<Evt3State> c;
    if (const int rc = result<Evt3State>(workspace, stream, counters, &c, status_out)) return rc;
    if (state_out) {
        state_out->flags = c.s.flags; state_out->loops = c.s.loops; state_out->first_high = c.s.first_high;
        state_out->last_high = c.s.last_high; state_out->low_y = c.s.low_y; state_out->base = c.s.base;
        state_out->has_last_t = c.has_last_t; state_out->last_t = c.last_t;
    }
    return FRLW_OK;
}

} // extern "C"
