// Host-only helpers shared by every unit of the icap library: error reporting, argument checks, the dropout
// threshold, the diagnostic build's environment switch. No HIP header: gemm_plan.cpp compiles with a plain host
// compiler.
#pragma once

// Diagnostic build only (make stamps: -DICAP_STAMPS): A/B overrides of the kernel choice read from the process
// environment (tools/ab). The product library reads one environment variable, ICAP_GROUP128 (gemm.hip: the grouped
// launch's 128 x 128 body, for A/B runs and the bitwise tests); every other choice in it is a function of the call's
// arguments and diag_env returns its default at compile time.
#ifdef ICAP_STAMPS
#include <cstdlib>
static inline int diag_env(const char* name, int dflt) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : dflt;
}
#else
static constexpr int diag_env(const char*, int dflt) { return dflt; }
#endif
#include <stdint.h>
#include <string>

#include "icap.h"

namespace icap {

// ---- error reporting (thread-local, C-ABI icap_last_error) -------------------
void set_error(const std::string& msg);

#define ICAP_REQUIRE(cond, msg)                 \
  do {                                          \
    if (!(cond)) {                              \
      ::icap::set_error(std::string(msg));      \
      return ICAP_ERR_ARG;                      \
    }                                           \
  } while (0)

inline uint32_t drop_threshold(float p) {
  double t = (double)p * 4294967296.0;
  if (t >= 4294967295.0) t = 4294967295.0;
  if (t < 0) t = 0;
  return (uint32_t)t;
}

}  // namespace icap
