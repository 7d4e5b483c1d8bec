// frlw_consts.h -- the constants host-only code (taf_plan.h, enc_plan.h) shares with the kernels: no HIP header, no HIP type.
#pragma once
#include <stddef.h>
namespace frlw {
constexpr int kWave = 64;
constexpr int kMaxBpw = 8;            // batches of 64 events per wavefront per workgroup chunk (registers!)
constexpr size_t kHeaderBytes = 1024; // the first bytes of every workspace: its header (WsHeader, frlw_common.h)
// A tile is (1 << twl) pixels wide and 8 rows high; twl = 8 for frames wider than 512 px, else 6
// (measured best on MI355X; frlw_tuning_t::tile_width_log2 overrides for experiments).
// One tile = one workgroup of the tile kernels = NT = 4 << twl threads owning 4 cells each
// (cell = (pixel, polarity)).  A tile row is a whole number of wavefronts of consecutive cells,
// so the (H, W, 2, K) state and the (C, H, W) outputs are read / written in full lines.
constexpr int kTileH = 8;
constexpr int kTileHLog = 3;
constexpr int kCellsPerThread = 4;
constexpr int kMaxTiles = 2048;   // LDS of the scatter workgroup: 52 B per tile
constexpr int kMaxTlut = 1 << 16; // longest TAF window (us) served by the value table
constexpr int kPartThreads = 1024; // partition workgroup = 16 wavefronts
constexpr int kPartWaves = kPartThreads / kWave;
constexpr int kSlabUnits = 32;    // workgroups per slab of the two-level column scan
constexpr int kMaxHot = 32;     // tiles per encode whose cells are split over several workgroups (skew)
constexpr int kSliceMult = 16;  // records per thread in one LDS counting-sort slice of the EV / TAF tile kernels
constexpr int kMaxK = 8;        // TAF FIFO depth / Event Volume bins a cell keeps in registers (FRLW_MAX_BINS)
} // namespace frlw
