// xcd_map_check.cpp -- the workgroup -> item mapping of csrc/xcd_map.h checked on the CPU, without HIP: for every grid size n in
// 1 ... 8200 (argv[1] overrides the upper end) and a few of the largest grids a consumer launches xcd_owned_index(., n) is a bijection of [0, n); the blocks k, k + 8, k + 16, ... of
// one XCD take consecutive ascending items; the eight ranges tile [0, n) in the order of k with sizes that differ by at most one;
// chunk_of_block is the same function.  Compiled with -DFRLW_NO_XCD_REMAP (the A/B arm) both must be the identity.
// Built with -fsanitize=address,undefined by tests/test_xcd_map_cpu.py; exit status 0 = all held.
#include "xcd_map.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

static long long g_checks = 0, g_failed = 0;
static unsigned g_n = 0, g_b = 0;
#define CHECK(cond)                                                                                       \
    do {                                                                                                  \
        ++g_checks;                                                                                       \
        if (!(cond) && ++g_failed <= 20) fprintf(stderr, "FAILED %s  [n = %u, block = %u]\n", #cond, g_n, g_b); \
    } while (0)

// usable in a constant expression (the kernels' callers may rely on it)
static_assert(frlw::xcd_owned_index(0u, 1u) == 0ll && frlw::chunk_of_block(0u, 1u) == 0ll, "constexpr");

int main(int argc, char **argv)
{
    const unsigned n_max = argc > 1 ? (unsigned)strtoul(argv[1], nullptr, 10) : 8200u;
    std::vector<unsigned char> seen;
    std::vector<unsigned> sizes;
    for (unsigned n = 1; n <= n_max; ++n) sizes.push_back(n);
    // the largest grids the consumers launch: 16 sub-tiles x 7200 tiles (1280x720), x 4096 / 8192 (sequence, tile) pairs, and odd ones
    for (unsigned n : {115200u, 65536u, 131072u, 131071u, 100003u}) sizes.push_back(n);
    for (unsigned n : sizes) {
        g_n = n;
        seen.assign(n, 0);
        for (unsigned b = 0; b < n; ++b) {
            g_b = b;
            const long long i = frlw::xcd_owned_index(b, n);
            CHECK(i >= 0 && i < (long long)n);
            if (i >= 0 && i < (long long)n) { CHECK(seen[i] == 0); seen[i] = 1; } // into [0, n) and injective: a bijection
            CHECK(frlw::chunk_of_block(b, n) == i);
#ifdef FRLW_NO_XCD_REMAP
            CHECK(i == (long long)b);
#else
            if (b + 8 < n) CHECK(frlw::xcd_owned_index(b + 8, n) == i + 1); // one XCD's blocks: consecutive, ascending
#endif
        }
#ifndef FRLW_NO_XCD_REMAP
        // the ranges: XCD k owns [start_k, start_k + size_k), start_0 = 0, start_{k+1} = start_k + size_k, the last one ends at n
        unsigned next = 0, lo = n, hi = 0;
        for (unsigned k = 0; k < 8; ++k) {
            g_b = k;
            const unsigned size = k < n ? (n - k + 7) / 8 : 0u; // blocks k, k + 8, ... below n
            if (size) CHECK(frlw::xcd_owned_index(k, n) == (long long)next);
            next += size;
            if (size < lo) lo = size;
            if (size > hi) hi = size;
        }
        CHECK(next == n);
        CHECK(hi - lo <= 1);
#endif
    }
    printf("xcd_map_check: grids 1 .. %u and 5 large ones, %lld checks, %lld failed\n", n_max, g_checks, g_failed);
    return g_failed ? 1 : 0;
}
