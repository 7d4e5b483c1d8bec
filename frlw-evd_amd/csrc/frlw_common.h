// frlw_common.h -- what every encoder unit shares: wavefront primitives, the workspace header and status words, tile geometry,
// f32_to_u8, HIP_TRY / grid_for, the cross-unit declarations.  Includes enc_plan.h, enc_decode.h and leaky.h for its users.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <atomic>

#include "frlw_consts.h" // kWave, kMaxBpw, kHeaderBytes, the tile / partition constants
#include "frlw_evd.h"
#include "xcd_map.h"
#include "enc_plan.h"

namespace frlw {
static_assert(kMaxK == FRLW_MAX_BINS, "a cell keeps FRLW_MAX_BINS FIFO slots / bins in registers");

// Inclusive prefix sum over the 64 lanes of a wavefront in the vector ALU (DPP row shifts inside the rows of 16 lanes, then
// the row totals by row_bcast15 / row_bcast31): six adds, no LDS crossbar round trips (a __shfl_up scan is six dependent
// ds_bpermute).  All lanes must be active.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false); // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false); // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false); // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false); // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); // row_bcast15 into rows 1 and 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); // row_bcast31 into rows 2 and 3
    return v;
}
// Maximum over the 64 lanes of a wavefront, returned wave-uniform (same DPP ladder, v_max instead of v_add; the total
// ends up in lane 63).  All lanes must be active.
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
    auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
    v = mx(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

enum Kind : int { KIND_ECI = 0, KIND_EV = 1, KIND_SAE = 2, KIND_TAF = 3 };
enum : int { ST_INDEX = 1, ST_POLARITY = 2, ST_SPAN = 4, /* 8: taf_fast.hip ST_MULBAD (not an error) */ ST_STALL = 16 /* a bounded device-side wait ran out: FRLW_ERR_HIP */ };

// First kHeaderBytes of the workspace.
struct WsHeader {
    int32_t status; // ST_* flags
    uint32_t pad;
    unsigned long long wmask; // bit w set <=> TAF window w holds at least one encoded event
    uint32_t n_hot;           // tiles with more than hot_thr records (may exceed kMaxHot; only the listed ones are split)
    uint32_t hot_thr;
    uint32_t hot[kMaxHot];
};
static_assert(sizeof(WsHeader) <= kHeaderBytes, "header");
static_assert(FRLW_MAX_WINDOWS <= 64, "wmask keeps one bit per TAF window");
// Two words at the end of the header outlive the per-call reset: `sticky` is the OR of the status of every encoder call
// since frlw_workspace_init / the last frlw_encoder_deferred_status (unchecked callers read it once per batch or epoch
// instead of synchronising after every call); the 24 bytes in front of it receive the one-time LDS self-test result.
constexpr size_t kStickyOffset = kHeaderBytes - 8;
// ... and `stall`, 8 bytes in front of `sticky`: the epoch of a fast-path call one of whose workgroups gave up its bounded wait
// for the header reset (ST_STALL).  It lies OUTSIDE the range workgroup 0 resets, so a workgroup 0 that starts late cannot
// wipe the verdict of its own call; workgroup 0 (and the captured form's reset kernel) clears it only when it belongs to an
// EARLIER call.  frlw_encoder_status reports FRLW_ERR_HIP while it is set.
constexpr size_t kStallOffset = kHeaderBytes - 16;
constexpr size_t kSelftestOffset = kHeaderBytes - 64;
static_assert(sizeof(WsHeader) <= kSelftestOffset, "header tail");
__device__ __forceinline__ void fold_sticky_status(void *hdr, int status) { if (status) atomicOr((int *)((char *)hdr + kStickyOffset), status); }

__device__ __forceinline__ uint64_t lanemask_lt() { return (1ull << (threadIdx.x & 63)) - 1ull; }

struct TileGeom { int x0, y0, nx, ny; }; // nx, ny: valid pixels of this tile

__device__ __forceinline__ TileGeom tile_geom(int tile, int tiles_x, int twl, int H, int W)
{
    TileGeom g;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int tw = 1 << twl;
    g.x0 = tx << twl;
    g.y0 = ty << kTileHLog;
    g.nx = W - g.x0 < tw ? W - g.x0 : tw;
    g.ny = H - g.y0 < kTileH ? H - g.y0 : kTileH;
    return g;
}

// float -> uint8 the way numpy's .astype(np.uint8) does it on the reference's x86 hosts: truncate to int32
// (cvttss2si: NaN / inf / out-of-range give INT_MIN), then keep the low byte.  v_cvt_i32_f32 saturates
// instead, so the out-of-range case is made explicit.  (Only reachable with state values > 0, i.e. events
// the harness placed after the last window.)
__device__ __forceinline__ uint8_t f32_to_u8(float v)
{
    const int i = (v >= -2147483648.0f && v < 2147483648.0f) ? (int)v : (int)0x80000000;
    return (uint8_t)i;
}

// Source index of torch's interpolate(mode='nearest'): min(floor(dst * scale), in - 1) with scale = float(in) / float(out).
// The one statement of the rule: the resize and sample-transform kernels of elementwise.hip and the renderer (render.hip).
__device__ __forceinline__ int nearest_src(int dst, float scale, int in_size)
{
    const int s = (int)floorf((float)dst * scale);
    return s > in_size - 1 ? in_size - 1 : s;
}

// ---- host side: what partition_events hands to the tile launch (leaky_thr: TAF only, the per-device threshold table of leaky.hip)
struct Partitioned { const uint2 *records; const uint32_t *base; WsHeader *hdr; const uint32_t *leaky_thr; Plan plan; };

int hip_fail(hipError_t e, const char *what, int line);

// frlw_sae_encode through the chunk-major partition of taf_fast.hip (two launches): FRLW_OK = launched, 1 = not eligible
// (nothing launched), negative = error.
int sae_fast_try(const frlw_events_t *ev, int H, int W, const float *lam, int n_lamda, const float *mem_in, float *mem_out,
                 long long now, long long window_us, float *out_f32, uint8_t *out_u8, void *workspace, size_t workspace_bytes,
                 hipStream_t st);

// Workspace bytes the two-launch form asks for (0: the call is not eligible) and the per-process launch counters behind
// frlw_encoder_path_counts: [0] SAE two-launch, [1] SAE general, [2] ECI two-launch, [3] ECI single-launch scan / general.
size_t sae_fast_workspace_bytes(long long n, int H, int W);
extern std::atomic<unsigned long long> g_path_counts[4];
// behind frlw_encoder_chain_counts (encoders_batch.hip): [0] frlw_sae_encode_chain, [1] frlw_ev_encode_ranges
extern std::atomic<unsigned long long> g_chain_counts[2];

// hist -> scans -> stable scatter: tile-major 8-byte records {window << (twl + 4) | cell, f32 bits}.
int partition_events(const frlw_events_t *ev, int H, int W, int kind, long long t0, long long win, int n_windows, int time_filter,
                     void *ws, size_t ws_bytes, hipStream_t s, Partitioned &out);

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return frlw::hip_fail(e_, #expr, __LINE__); } while (0)

inline int grid_for(long long n, int block)
{
    long long g = (n + block - 1) / block;
    if (g > 256 * 8) g = 256 * 8;
    if (g < 1) g = 1;
    return (int)g;
}
} // namespace frlw

#include "enc_decode.h"
#include "leaky.h"
