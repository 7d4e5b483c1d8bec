// walk_mean_check.cpp -- csrc/taf_mean.h on the CPU, without HIP: mean_by_recip(sum, (float)n, R[n]) against the division it
// replaces in kf_taf_walk, sum / ((float)n + 1e-8f), BIT FOR BIT, for every count n of the table (0 ... kMeanTab - 1).
// Built with the host compiler at -O2 -ffp-contract=off by tests/test_walk_mean_cpu.py; exit status 0 = no mismatch.
//
//   walk_mean_check            the quick sets, one line per set (seconds):
//     edges     sum = +0, -0 (every n); -n and its two f32 neighbours (n >= 1: a count of 0 has no sum but +-0)
//     stride    every f32 in [-n, -2^-24] that is a multiple of 2^-24 -- what a sequential f32 sum of n values k * 2^-24 in [-1, 0]
//               can be -- taken with an odd stride through the bit patterns
//     binades   the 4096 f32 values on either side of every power of two 2^-24 ... <= n (multiples of 2^-24 or not)
//     random    10^6 seeded values per n that are NOT multiples of 2^-24 (all of those lie in (-1/2, 0)): half uniform there, half
//               with a uniform exponent 2^-60 ... 2^-2 (the short form rests on an exact residual, i.e. on no underflow, not on
//               the multiples)
//   walk_mean_check --full [threads]   EVERY f32 in [-n, -2^-24] and +-0 for every n: 1.6e10 comparisons, at most 16 threads
#include "taf_mean.h"

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t bits_of(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

static float g_tab[frlw::kMeanTab];
static std::atomic<long long> g_reported{0};

// one comparison; returns 1 on a mismatch (the first twenty are printed with the set they belong to)
static inline int differs(const char *set, int n, float sum)
{
    const float want = sum / ((float)n + 1e-8f);
    const float got = frlw::mean_by_recip(sum, (float)n, g_tab[n]);
    if (bits_of(want) == bits_of(got)) return 0;
    if (g_reported.fetch_add(1) < 20)
        fprintf(stderr, "MISMATCH [%s] n = %d  sum = %a (0x%08x)  division %a (0x%08x)  by reciprocal %a (0x%08x)\n", set, n, sum, bits_of(sum),
                want, bits_of(want), got, bits_of(got));
    return 1;
}

static bool multiple_of_2m24(float x) { const float y = x * 16777216.0f; return y == floorf(y); } // (exact scaling: |x| <= 64)

static const uint32_t kLowBits = 0x33800000u; // 2^-24
static const uint32_t kSign = 0x80000000u;

struct Tally { long long checked = 0, bad = 0; };

static void report(const char *set, const Tally &t, Tally &all)
{
    printf("%-8s %13lld comparisons  %lld mismatches\n", set, t.checked, t.bad);
    all.checked += t.checked;
    all.bad += t.bad;
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull; // splitmix64, seeded: the same values on every run
static uint64_t rnd()
{
    uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static int quick()
{
    Tally all;
    {
        Tally t;
        for (int n = 0; n < frlw::kMeanTab; ++n) {
            t.bad += differs("edges", n, 0.0f) + differs("edges", n, -0.0f);
            t.checked += 2;
            if (n == 0) continue;
            const float m = -(float)n;
            t.bad += differs("edges", n, m) + differs("edges", n, nextafterf(m, 0.0f)) + differs("edges", n, nextafterf(m, -INFINITY));
            t.checked += 3;
        }
        report("edges", t, all);
    }
    {
        Tally t;
        const uint32_t stride = 61u; // odd: every residue of the low mantissa bits comes up
        for (int n = 1; n < frlw::kMeanTab; ++n) {
            const uint32_t top = bits_of((float)n);
            for (uint32_t b = kLowBits + (uint32_t)n; b <= top; b += stride) { // (another phase of the stride for every n)
                const float x = from_bits(b);
                if (!multiple_of_2m24(x)) continue;
                t.bad += differs("stride", n, -x);
                ++t.checked;
            }
        }
        report("stride", t, all);
    }
    {
        Tally t;
        for (int n = 1; n < frlw::kMeanTab; ++n)
            for (int e = -24; e <= 5 && ldexpf(1.0f, e) <= (float)n; ++e) {
                const uint32_t c = bits_of(ldexpf(1.0f, e));
                for (uint32_t b = c - 4096u; b <= c + 4096u; ++b) {
                    t.bad += differs("binades", n, from_bits(b | kSign));
                    ++t.checked;
                }
            }
        report("binades", t, all);
    }
    {
        Tally t;
        for (int n = 1; n < frlw::kMeanTab; ++n)
            for (int i = 0; i < 1000000;) {
                float x;
                // (every f32 of magnitude >= 1/2 IS a multiple of 2^-24: the others of [-n, 0] all lie in (-1/2, 0), whatever n)
                if (i & 1) {
                    x = (float)((double)(rnd() >> 11) * (0.5 / 9007199254740992.0)); // uniform in [0, 1/2)
                } else { // a uniform exponent 2^-60 ... 2^-2, a uniform mantissa
                    const int e = -60 + (int)(rnd() % 59u);
                    x = ldexpf(1.0f + (float)(rnd() & 0x7fffffu) * (1.0f / 8388608.0f), e);
                }
                if (!(x > 0.0f) || x >= 0.5f || multiple_of_2m24(x)) continue;
                t.bad += differs("random", n, -x);
                ++t.checked;
                ++i;
            }
        report("random", t, all);
    }
    printf("walk_mean_check quick: %lld comparisons, %lld mismatches\n", all.checked, all.bad);
    return all.bad == 0 ? 0 : 1;
}

static int full(int threads)
{
    if (threads < 1) threads = 1;
    if (threads > 16) threads = 16;
    std::atomic<long long> checked{0}, bad{0};
    std::atomic<int> next{0};
    long long bad_n[frlw::kMeanTab] = {};
    // work items: (n, slice of the bit patterns kLowBits ... bits(n)); 64 slices per n keep the threads level
    const int kSlices = 64;
    auto work = [&]() {
        for (;;) {
            const int item = next.fetch_add(1);
            if (item >= frlw::kMeanTab * kSlices) break;
            const int n = item / kSlices, sl = item % kSlices;
            long long c = 0, m = 0;
            if (sl == 0) { m += differs("full", n, 0.0f) + differs("full", n, -0.0f); c += 2; }
            if (n > 0) {
                const uint64_t lo = kLowBits, count = (uint64_t)bits_of((float)n) - lo + 1u;
                const uint64_t b0 = lo + count * (uint64_t)sl / kSlices, b1 = lo + count * (uint64_t)(sl + 1) / kSlices;
                for (uint64_t b = b0; b < b1; ++b) m += differs("full", n, from_bits((uint32_t)b | kSign));
                c += (long long)(b1 - b0);
            }
            checked += c;
            bad += m;
            if (m) __atomic_fetch_add(&bad_n[n], m, __ATOMIC_RELAXED);
        }
    };
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) pool.emplace_back(work);
    for (auto &t : pool) t.join();
    for (int n = 0; n < frlw::kMeanTab; ++n)
        if (bad_n[n]) printf("n = %d: %lld mismatches\n", n, bad_n[n]);
    printf("walk_mean_check full: n = 0 ... %d, every f32 sum in [-n, -2^-24] and +-0: %lld comparisons, %lld mismatches\n", frlw::kMeanTab - 1,
           checked.load(), bad.load());
    return bad.load() == 0 ? 0 : 1;
}

int main(int argc, char **argv)
{
    for (int n = 0; n < frlw::kMeanTab; ++n) g_tab[n] = frlw::mean_recip_entry(n);
    if (argc > 1 && !strcmp(argv[1], "--full")) return full(argc > 2 ? atoi(argv[2]) : 16);
    return quick();
}
