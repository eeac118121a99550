// Stand-alone host check of the grouped launch's tile choice (gemm_plan.cpp gemm_group_plan; icap_gemm_group). Reads
// one group per line from standard input — "cus force128 M N [M N ...]" — and prints its plan:
// "big|small total swap tiles_m x tiles_n ...". Built by `make group_check` with the host compiler under ASan + UBSan;
// tests/test_gemm_group256_cpu.py runs it over a table of shapes.
#include <cstdio>
#include <sstream>
#include <string>
#include <iostream>

#include "gemm_plan.h"

namespace icap {
void set_error(const std::string&) {}
}  // namespace icap
using namespace icap;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    int cus = 0, force = 0, n = 0;
    int64_t M[GROUP_MAX], N[GROUP_MAX];
    if (!(in >> cus >> force)) continue;
    while (n < GROUP_MAX && (in >> M[n] >> N[n])) ++n;
    const GroupPlan gp = gemm_group_plan(M, N, n, cus, force != 0);
    std::printf("%s %lld %u", gp.big ? "big" : "small", (long long)gp.total, gp.swap);
    for (int i = 0; i < n; ++i) std::printf(" %dx%d", gp.tiles_m[i], gp.tiles_n[i]);
    std::printf("\n");
  }
  return 0;
}
