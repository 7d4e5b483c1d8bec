// evt3_state.h -- the EVT 3.0 decoder state after a run of words, and how two such records compose ("EVT 3.0
// decode").  No HIP header and no HIP type: evt3.hip includes it for the device, tests/host/evt3_state_check.cpp for the host.
//
// A record summarises a RUN of words without knowing what came before it: which fields the run sets and to what, and what it
// adds where it sets nothing.  evt3_compose(a, b) is the record of the run "a then b"; it is associative, evt3_identity() is
// its neutral element, and the record of a stream from its first word on is the state of the sequential decoder behind its
// last word (fields whose flag is clear are "unset": their values mean nothing then).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FRLW_EVT3_HD __host__ __device__ inline
#else
#define FRLW_EVT3_HD inline
#endif

namespace frlw {

enum : uint32_t {
    EVT3_HAS_HIGH = 1u, // an EVT_TIME_HIGH was seen: first_high / last_high hold values
    EVT3_HAS_LOW = 2u,  // an EVT_TIME_LOW was seen (low counts as 0 before the first one)
    EVT3_HAS_Y = 4u,    // an EVT_ADDR_Y was seen
    EVT3_HAS_BASE = 8u, // a VECT_BASE_X was seen: base = its x plus the 12s and 8s since
    EVT3_VP = 16u,      // the polarity of that VECT_BASE_X
};

// word types (bits 15..12)
enum : uint32_t {
    EVT3_ADDR_Y = 0x0, EVT3_ADDR_X = 0x2, EVT3_VECT_BASE_X = 0x3, EVT3_VECT_12 = 0x4, EVT3_VECT_8 = 0x5, EVT3_TIME_LOW = 0x6,
    EVT3_TIME_HIGH = 0x8, EVT3_EXT_TRIGGER = 0xA,
};
constexpr uint32_t kEvt3WrapSlack = 10; // a TIME_HIGH more than this many steps below its predecessor is a clock wrap

struct alignas(8) Evt3State {
    uint32_t flags;      // EVT3_*
    uint32_t loops;      // clock wraps counted inside the run
    uint32_t first_high; // value of the run's first EVT_TIME_HIGH
    uint32_t last_high;  // ... and of its last
    uint32_t low_y;      // last EVT_TIME_LOW | last EVT_ADDR_Y << 16
    uint32_t base;       // HAS_BASE: x of the last VECT_BASE_X + the vector widths since; else the widths of the whole run
};

FRLW_EVT3_HD Evt3State evt3_identity()
{
    Evt3State s = {0u, 0u, 0u, 0u, 0u, 0u};
    return s;
}

FRLW_EVT3_HD uint32_t evt3_low(const Evt3State &s) { return s.low_y & 0xFFFFu; }
FRLW_EVT3_HD uint32_t evt3_y(const Evt3State &s) { return s.low_y >> 16; }

// The record of the run "a then b".
FRLW_EVT3_HD Evt3State evt3_compose(const Evt3State &a, const Evt3State &b)
{
    Evt3State r;
    r.flags = (a.flags | b.flags) & ~EVT3_VP;
    r.loops = a.loops + b.loops;
    if (b.flags & EVT3_HAS_HIGH) {
        r.last_high = b.last_high;
        if (a.flags & EVT3_HAS_HIGH) {
            r.first_high = a.first_high;
            r.loops += (b.first_high + kEvt3WrapSlack < a.last_high) ? 1u : 0u; // the wrap on the boundary
        } else {
            r.first_high = b.first_high;
        }
    } else {
        r.first_high = a.first_high;
        r.last_high = a.last_high;
    }
    const uint32_t low = (b.flags & EVT3_HAS_LOW) ? (b.low_y & 0xFFFFu) : (a.low_y & 0xFFFFu);
    const uint32_t y = (b.flags & EVT3_HAS_Y) ? (b.low_y & 0xFFFF0000u) : (a.low_y & 0xFFFF0000u);
    r.low_y = low | y;
    if (b.flags & EVT3_HAS_BASE) {
        r.base = b.base;
        r.flags |= b.flags & EVT3_VP;
    } else {
        r.base = a.base + b.base; // no VECT_BASE_X in b: its vector widths add to whatever a left
        r.flags |= a.flags & EVT3_VP;
    }
    return r;
}

// The record of the one-word run `w` composed behind `s`, in place: what the decoder's state update of the format table does
// (emitting and counting is the caller's business; a vector word advances base whether or not its events are emitted).
FRLW_EVT3_HD void evt3_step(Evt3State &s, uint32_t w)
{
    const uint32_t type = (w >> 12) & 0xFu, v = w & 0xFFFu;
    switch (type) {
    case EVT3_ADDR_Y:
        s.low_y = (s.low_y & 0xFFFFu) | ((v & 0x7FFu) << 16);
        s.flags |= EVT3_HAS_Y;
        break;
    case EVT3_VECT_BASE_X:
        s.base = v & 0x7FFu;
        s.flags = (s.flags & ~EVT3_VP) | EVT3_HAS_BASE | ((v & 0x800u) ? EVT3_VP : 0u);
        break;
    case EVT3_VECT_12:
        s.base += 12u;
        break;
    case EVT3_VECT_8:
        s.base += 8u;
        break;
    case EVT3_TIME_LOW:
        s.low_y = (s.low_y & 0xFFFF0000u) | v;
        s.flags |= EVT3_HAS_LOW;
        break;
    case EVT3_TIME_HIGH:
        if (s.flags & EVT3_HAS_HIGH) {
            s.loops += (v + kEvt3WrapSlack < s.last_high) ? 1u : 0u;
        } else {
            s.first_high = v;
            s.flags |= EVT3_HAS_HIGH;
        }
        s.last_high = v;
        break;
    default:
        break;
    }
}

// t of an event decoded in state s, before any shift.
FRLW_EVT3_HD uint64_t evt3_time(const Evt3State &s)
{
    return ((uint64_t)s.loops << 24) | ((uint64_t)s.last_high << 12) | (uint64_t)(s.low_y & 0xFFFFu);
}

} // namespace frlw
