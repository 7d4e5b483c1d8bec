// frlw_consts.h -- the constants host-only code (taf_plan.h) shares with the kernels: no HIP header, no HIP type.
#pragma once
#include <stddef.h>
namespace frlw {
constexpr int kWave = 64;
constexpr int kMaxBpw = 8;            // batches of 64 events per wavefront per workgroup chunk (registers!)
constexpr size_t kHeaderBytes = 1024; // the first bytes of every workspace: its header (WsHeader, frlw_common.h)
} // namespace frlw
