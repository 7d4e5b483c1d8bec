// xcd_map.h -- which item of a list a workgroup takes, so that neighbouring items go through the same L2.  No HIP type: the
// arithmetic is plain C++ and is checked on the CPU (tests/host/xcd_map_check.cpp).
#pragma once

#if defined(__HIPCC__)
#define FRLW_XCD_HD __host__ __device__ __forceinline__
#else
#define FRLW_XCD_HD inline
#endif

namespace frlw {
// Workgroups are handed to the 8 XCDs round-robin (block b runs on XCD b % 8) and every XCD has its own L2.  Of n_blocks items
// XCD k owns the contiguous range [start_k, start_{k+1}) -- the eight ranges tile [0, n_blocks) in the order of k, the first
// n_blocks % 8 of them one item longer -- and block (i - start_k) * 8 + k takes item i: a bijection of [0, n_blocks) in which
// the blocks k, k + 8, k + 16, ... of one XCD take consecutive items.  Items that share cache lines with their neighbours
// (a chunk's stretch of records on the writing side, the runs of neighbouring bins inside it on the reading side) then meet
// in ONE L2.  The round-robin placement is a speed assumption only: whatever the hardware does, every item is taken once.
// FRLW_NO_XCD_REMAP (A/B arm): the identity, for producers and consumers alike.
constexpr FRLW_XCD_HD long long xcd_owned_index(unsigned block, unsigned n_blocks)
{
#ifdef FRLW_NO_XCD_REMAP
    return (void)n_blocks, block;
#else
    const unsigned k = block & 7u, idx = block >> 3, q = n_blocks >> 3, r = n_blocks & 7u;
    return (long long)k * q + (k < r ? k : r) + idx;
#endif
}

// The producer's name for it (kf_scatter, kf_scatter_cm): chunk c of the stream is written by the block that owns it.
constexpr FRLW_XCD_HD long long chunk_of_block(unsigned block, unsigned n_blocks) { return xcd_owned_index(block, n_blocks); }
} // namespace frlw
