// Host check of csrc/evt2_state.h (no HIP): the clock record of a run of EVT 2.0 / EVT 2.1 words and its compose.
//
// For 300 random streams of EVT_TIME_HIGH, event and no-effect words (given by their upper 32 bits, which is all the state looks
// at): the stream is cut into runs of every length 1 .. kMaxRun; each run is summarised from the identity with evt2_step; the run
// records are composed left to right and as a balanced tree.  Both must equal, byte for byte, the summary of the whole stream
// (associativity, and step == compose with a one-word run), and that summary must equal the final state of a sequential decoder
// written here from the format table.  Every prefix / suffix pair must compose to the whole; the identity must be neutral on both
// sides of every run record; and a wrap whose two EVT_TIME_HIGH words fall on either side of a run boundary must be counted once.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "evt2_state.h"

using frlw::Evt2State;

namespace {
constexpr int kStreams = 300, kWords = 700, kMaxRun = 67;
constexpr uint32_t kTop = (1u << 28) - 1u;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

// the clock of the format table, nothing shared with the header under test
struct Seq {
    bool has_high = false;
    uint32_t first_high = 0, high = 0, loops = 0;
    void word(uint32_t hi)
    {
        if ((hi >> 28) != 0x8) return;
        const uint32_t v = hi & 0x0FFFFFFF;
        if (has_high && v + 10 < high) loops += 1;
        if (!has_high) first_high = v;
        high = v;
        has_high = true;
    }
    uint64_t time(uint32_t low) const { return ((uint64_t)loops << 34) | ((uint64_t)high << 6) | low; }
};

std::vector<uint32_t> random_stream(int s)
{
    std::vector<uint32_t> w(kWords);
    const int junk = (int)(rnd() % 40);              // words in front of which no EVT_TIME_HIGH appears
    uint32_t high = (s % 3 == 0) ? kTop - rnd() % 20 : rnd() & kTop;
    for (int i = 0; i < kWords; ++i) {
        const uint32_t r = rnd() % 100;
        uint32_t type, v = rnd() & kTop;
        if (i < junk || r < 60) type = r & 1;        // an event word
        else if (r < 85) {
            type = 0x8;
            const uint32_t how = rnd() % 10;
            if (how < 5) high = (high + 1 + rnd() % 3) & kTop;                       // forward, wraps at 2^28 - 1 -> 0
            else if (how < 7) high = high >= 12 ? high - (9 + rnd() % 3) : high;     // back by 9, 10 or 11: only 11 is a wrap
            else if (how < 8) high = rnd() & kTop;                                   // anywhere
            else high = (s & 1) ? kTop : 0;                                          // the two ends of the clock
            v = high;
        } else type = (r < 90) ? 0xA : (r < 94) ? 0xE : (r < 97) ? 0xF : 0x3;
        w[i] = (type << 28) | v;
    }
    return w;
}

Evt2State summary(const uint32_t *w, int n)
{
    Evt2State s = frlw::evt2_identity();
    for (int i = 0; i < n; ++i) frlw::evt2_step(s, w[i]);
    return s;
}

Evt2State tree(const std::vector<Evt2State> &r, size_t lo, size_t hi)
{
    if (hi - lo == 1) return r[lo];
    const size_t mid = lo + (hi - lo) / 2;
    return frlw::evt2_compose(tree(r, lo, mid), tree(r, mid, hi));
}

bool same(const Evt2State &a, const Evt2State &b) { return memcmp(&a, &b, sizeof(a)) == 0; }

bool equals_sequential(const Evt2State &s, const Seq &q)
{
    if (((s.flags & frlw::EVT2_HAS_HIGH) != 0) != q.has_high) return false;
    if (s.loops != q.loops) return false;
    if (q.has_high && (s.first_high != q.first_high || s.last_high != q.high)) return false;
    if (q.has_high && frlw::evt2_time(s, 37u) != q.time(37u)) return false;
    return true;
}
} // namespace

int main()
{
    long long failed = 0, cuts = 0, boundary_wraps = 0;
    for (int s = 0; s < kStreams; ++s) {
        const std::vector<uint32_t> w = random_stream(s);
        const Evt2State whole = summary(w.data(), kWords);
        Seq q;
        for (int i = 0; i < kWords; ++i) q.word(w[i]);
        if (!equals_sequential(whole, q)) { ++failed; printf("stream %d: summary != sequential decoder\n", s); }
        for (int run = 1; run <= kMaxRun; ++run) {
            std::vector<Evt2State> recs;
            for (int lo = 0; lo < kWords; lo += run) recs.push_back(summary(w.data() + lo, lo + run <= kWords ? run : kWords - lo));
            Evt2State left = frlw::evt2_identity();
            uint32_t inside = 0;
            for (const Evt2State &r : recs) {
                left = frlw::evt2_compose(left, r);
                inside += r.loops;
                if (!same(frlw::evt2_compose(frlw::evt2_identity(), r), r) || !same(frlw::evt2_compose(r, frlw::evt2_identity()), r)) {
                    ++failed;
                    if (failed < 10) printf("stream %d run %d: the identity is not neutral\n", s, run);
                }
            }
            const Evt2State bal = tree(recs, 0, recs.size());
            ++cuts;
            boundary_wraps += (long long)(whole.loops - inside); // wraps no run saw: their two words lie in different runs
            if (inside > whole.loops || !same(left, whole) || !same(bal, whole)) {
                ++failed;
                if (failed < 10) printf("stream %d run %d: left-to-right %d balanced %d\n", s, run, (int)same(left, whole), (int)same(bal, whole));
            }
        }
        // carried state: the prefix record composed with the rest, against the whole and against the sequential decoder cut there
        for (int cut = 0; cut <= kWords; cut += 1 + (int)(rnd() % 5)) {
            const Evt2State a = summary(w.data(), cut), b = summary(w.data() + cut, kWords - cut);
            Seq p;
            for (int i = 0; i < cut; ++i) p.word(w[i]);
            if (!same(frlw::evt2_compose(a, b), whole) || !equals_sequential(a, p)) { ++failed; if (failed < 10) printf("stream %d cut %d\n", s, cut); }
        }
    }
    if (boundary_wraps == 0) { ++failed; printf("no wrap fell on a run boundary: the streams do not test it\n"); }
    printf("%d streams of %d words, runs of 1 .. %d (%lld cuttings, %lld wraps on run boundaries), %lld failed\n", kStreams, kWords, kMaxRun,
           cuts, boundary_wraps, failed);
    return failed ? 1 : 0;
}
