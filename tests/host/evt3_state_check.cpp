// Host check of csrc/evt3_state.h (no HIP): the state record of a run of EVT 3.0 words and its compose.
//
// For 300 random word streams (vectors, clock wraps, small backward steps, junk in front of the sync words, trigger / other words
// in between): the stream is cut into runs of every length 1 .. kMaxRun; each run is summarised from the identity with evt3_step;
// the run records are composed left to right and as a balanced tree.  Both must equal, byte for byte, the summary of the whole
// stream (associativity, and step == compose with a one-word run), and that summary must equal the final state of a sequential
// decoder written here from the format table (fields that were never set are compared by their flag only).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "evt3_state.h"

using frlw::Evt3State;

namespace {
constexpr int kStreams = 300, kWords = 700, kMaxRun = 67;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

// the decoder of the format table, nothing shared with the header under test
struct Seq {
    bool has_high = false, has_low = false, has_y = false, has_base = false;
    uint32_t first_high = 0, high = 0, loops = 0, low = 0, y = 0, base = 0, vp = 0;
    void word(uint32_t w)
    {
        const uint32_t type = w >> 12, v = w & 0xFFF;
        if (type == 0x0) { y = v & 0x7FF; has_y = true; }
        else if (type == 0x3) { base = v & 0x7FF; vp = v >> 11; has_base = true; }
        else if (type == 0x4) { if (has_base) base += 12; }
        else if (type == 0x5) { if (has_base) base += 8; }
        else if (type == 0x6) { low = v; has_low = true; }
        else if (type == 0x8) {
            if (has_high && v + 10 < high) loops += 1;
            if (!has_high) first_high = v;
            high = v;
            has_high = true;
        }
    }
};

std::vector<uint16_t> random_stream(int s)
{
    std::vector<uint16_t> w(kWords);
    const int junk = (int)(rnd() % 40);              // words in front of which no setter appears
    uint32_t high = rnd() & 0xFFF;
    for (int i = 0; i < kWords; ++i) {
        const uint32_t r = rnd() % 100;
        uint32_t type, v = rnd() & 0xFFF;
        if (i < junk) type = (r < 40) ? 0x2 : (r < 60) ? 0x4 : (r < 70) ? 0x5 : (r < 80) ? 0xA : 0xE;
        else if (r < 30) type = 0x2;
        else if (r < 42) type = 0x4;
        else if (r < 50) type = 0x5;
        else if (r < 58) type = 0x3;
        else if (r < 68) type = 0x0;
        else if (r < 78) type = 0x6;
        else if (r < 90) {
            type = 0x8;
            const uint32_t how = rnd() % 10;
            if (how < 5) high = (high + 1 + rnd() % 3) & 0xFFF;          // forward, wraps at 4095 -> 0
            else if (how < 7) high = high >= 12 ? high - (9 + rnd() % 3) : high; // back by 9, 10 or 11: only 11 is a wrap
            else if (how < 8) high = rnd() & 0xFFF;                       // anywhere
            else high = (s & 1) ? 4095 : 0;                               // the two ends of the clock
            v = high;
        } else type = (r < 94) ? 0xA : (r < 96) ? 0x7 : (r < 98) ? 0xF : 0x1;
        w[i] = (uint16_t)((type << 12) | v);
    }
    return w;
}

Evt3State summary(const uint16_t *w, int n)
{
    Evt3State s = frlw::evt3_identity();
    for (int i = 0; i < n; ++i) frlw::evt3_step(s, w[i]);
    return s;
}

Evt3State tree(const std::vector<Evt3State> &r, size_t lo, size_t hi)
{
    if (hi - lo == 1) return r[lo];
    const size_t mid = lo + (hi - lo) / 2;
    return frlw::evt3_compose(tree(r, lo, mid), tree(r, mid, hi));
}

bool same(const Evt3State &a, const Evt3State &b) { return memcmp(&a, &b, sizeof(a)) == 0; }

bool equals_sequential(const Evt3State &s, const Seq &q)
{
    using namespace frlw;
    if (((s.flags & EVT3_HAS_HIGH) != 0) != q.has_high || ((s.flags & EVT3_HAS_LOW) != 0) != q.has_low ||
        ((s.flags & EVT3_HAS_Y) != 0) != q.has_y || ((s.flags & EVT3_HAS_BASE) != 0) != q.has_base)
        return false;
    if (s.loops != q.loops) return false;
    if (q.has_high && (s.first_high != q.first_high || s.last_high != q.high)) return false;
    if (evt3_low(s) != q.low) return false; // 0 before the first EVT_TIME_LOW
    if (q.has_y && evt3_y(s) != q.y) return false;
    if (q.has_base && (s.base != q.base || ((s.flags & EVT3_VP) != 0) != (q.vp != 0))) return false;
    if (q.has_high && evt3_time(s) != (((uint64_t)q.loops << 24) | ((uint64_t)q.high << 12) | q.low)) return false;
    return true;
}
} // namespace

int main()
{
    long long failed = 0, cuts = 0;
    for (int s = 0; s < kStreams; ++s) {
        const std::vector<uint16_t> w = random_stream(s);
        const Evt3State whole = summary(w.data(), kWords);
        Seq q;
        for (int i = 0; i < kWords; ++i) q.word(w[i]);
        if (!equals_sequential(whole, q)) { ++failed; printf("stream %d: summary != sequential decoder\n", s); }
        for (int run = 1; run <= kMaxRun; ++run) {
            std::vector<Evt3State> recs;
            for (int lo = 0; lo < kWords; lo += run) recs.push_back(summary(w.data() + lo, lo + run <= kWords ? run : kWords - lo));
            Evt3State left = frlw::evt3_identity();
            for (const Evt3State &r : recs) left = frlw::evt3_compose(left, r);
            const Evt3State bal = tree(recs, 0, recs.size());
            ++cuts;
            if (!same(left, whole) || !same(bal, whole)) {
                ++failed;
                if (failed < 10) printf("stream %d run %d: left-to-right %d balanced %d\n", s, run, (int)same(left, whole), (int)same(bal, whole));
            }
        }
        // carried state: the prefix record composed with the rest, cut at every word
        for (int cut = 0; cut <= kWords; cut += 1 + (int)(rnd() % 5)) {
            const Evt3State a = summary(w.data(), cut), b = summary(w.data() + cut, kWords - cut);
            if (!same(frlw::evt3_compose(a, b), whole)) { ++failed; if (failed < 10) printf("stream %d cut %d\n", s, cut); }
        }
    }
    printf("%d streams of %d words, runs of 1 .. %d (%lld cuttings), %lld failed\n", kStreams, kWords, kMaxRun, cuts, failed);
    return failed ? 1 : 0;
}
