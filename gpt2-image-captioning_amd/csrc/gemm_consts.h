// The constants the GEMM launch planner (gemm_plan.cpp, host-only) shares with the kernels. No HIP dependency.
#pragma once

namespace icap {

constexpr int GBM = 128, GBN = 128, GNT = 256;  // default 128x128 tile, 256 threads
constexpr int SK_WAVES = 8;                     // waves of a skinny-GEMM block

// Activation kinds of an epilogue instantiation (template int ACT; the forms are described in gemm_common.h)
constexpr int ACT_OFF = 0, ACT_ANY = 1, ACT_FWD = 16, ACT_BWD = 32;
// LayerNorm statistics hand-off, or-ed into the kind: producer / consumer
constexpr int ACT_LNS = 256, ACT_LNF = 512;

}  // namespace icap
