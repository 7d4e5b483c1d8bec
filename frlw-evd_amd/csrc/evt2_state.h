// evt2_state.h -- the EVT 2.0 / EVT 2.1 decoder state after a run of words, and how two such records compose (DESIGN.md,
// "EVT 2.0 and EVT 2.1 decode").  No HIP header and no HIP type: evt2.hip includes it for the device,
// tests/host/evt2_state_check.cpp for the host.
//
// Both encodings carry the same state: the clock.  An event word holds its own x, y, p and the low six bits of its t, so the only
// thing a word needs from the words before it is the latest EVT_TIME_HIGH and the wraps counted so far.  A record summarises a RUN
// of words without knowing what came before it; evt2_compose(a, b) is the record of the run "a then b", it is associative,
// evt2_identity() is its neutral element, and the record of a stream from its first word on is the state of the sequential
// decoder behind its last word (first_high / last_high mean nothing while EVT2_HAS_HIGH is clear).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FRLW_EVT2_HD __host__ __device__ inline
#else
#define FRLW_EVT2_HD inline
#endif

namespace frlw {

enum : uint32_t {
    EVT2_HAS_HIGH = 1u, // an EVT_TIME_HIGH was seen: first_high / last_high hold values
};

// word types (bits 31..28 of an EVT 2.0 word, bits 63..60 of an EVT 2.1 word)
enum : uint32_t { EVT2_CD_OFF = 0x0, EVT2_CD_ON = 0x1, EVT2_TIME_HIGH = 0x8, EVT2_EXT_TRIGGER = 0xA };
constexpr uint32_t kEvt2WrapSlack = 10; // a TIME_HIGH more than this many steps below its predecessor is a clock wrap

struct alignas(8) Evt2State {
    uint32_t flags;      // EVT2_HAS_HIGH
    uint32_t loops;      // clock wraps counted inside the run
    uint32_t first_high; // value (28 bits) of the run's first EVT_TIME_HIGH
    uint32_t last_high;  // ... and of its last
};

FRLW_EVT2_HD Evt2State evt2_identity()
{
    Evt2State s = {0u, 0u, 0u, 0u};
    return s;
}

// The record of the run "a then b".
FRLW_EVT2_HD Evt2State evt2_compose(const Evt2State &a, const Evt2State &b)
{
    if (!(b.flags & EVT2_HAS_HIGH)) return a;
    if (!(a.flags & EVT2_HAS_HIGH)) return b;
    Evt2State r;
    r.flags = EVT2_HAS_HIGH;
    r.loops = a.loops + b.loops + ((b.first_high + kEvt2WrapSlack < a.last_high) ? 1u : 0u); // the wrap on the boundary
    r.first_high = a.first_high;
    r.last_high = b.last_high;
    return r;
}

// The one-word run "EVT_TIME_HIGH v" composed behind `s`, in place.  Every other word leaves the state as it is.
FRLW_EVT2_HD void evt2_time_high(Evt2State &s, uint32_t v)
{
    if (s.flags & EVT2_HAS_HIGH) {
        s.loops += (v + kEvt2WrapSlack < s.last_high) ? 1u : 0u;
    } else {
        s.first_high = v;
        s.flags = EVT2_HAS_HIGH;
    }
    s.last_high = v;
}

// The state update of a word given by its upper 32 bits (an EVT 2.0 word is its own upper half; bits 31..0 of an EVT 2.1
// EVT_TIME_HIGH are ignored).
FRLW_EVT2_HD void evt2_step(Evt2State &s, uint32_t hi)
{
    if ((hi >> 28) == EVT2_TIME_HIGH) evt2_time_high(s, hi & 0x0FFFFFFFu);
}

// t of an event word with the low bits `low` decoded in state s, before any shift.
FRLW_EVT2_HD uint64_t evt2_time(const Evt2State &s, uint32_t low)
{
    return ((uint64_t)s.loops << 34) | ((uint64_t)s.last_high << 6) | (uint64_t)(low & 63u);
}

} // namespace frlw
