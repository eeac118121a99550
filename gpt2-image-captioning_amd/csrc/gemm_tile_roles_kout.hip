#include "gemm_launch.h"

namespace icap {

// Variant 31 (round 6): the K-outer weight-gradient products (dW = dY^T X over token rows, icap_gemm_args.trans_ab) on
// the split-role ring of gemm_tile.h: 4 MFMA waves of 64 x 64 reading ds_read_b64_tr_b16 fragments from the T10 (b)
// images + 4 LDS-DMA waves, 4 stages of 32 KiB, one block per CU walking tiles x splits; splits go through the slabs
// and the reduce pass.
int launch_tile_roles_kout(const GemmPlan& pl, const icap_gemm_args& p, int nks, hipStream_t s) {
  return launch_tile_forms<bf16_t, KINDS_ALL, V_ROLES_KOUT>(pl, p, nks, s);
}

// A group of K-outer products in ONE launch (icap_gemm_group, round 6): every block walks the concatenated tile list of
// the group (product i owns tile ids [tstart[i], tstart[i + 1])) with the variant-31 body, unsplit — so a layer's four
// weight-gradient products fill the chip together (432 tiles at the mapper's shape) without split-K slabs or a reduce
// pass. Each output tile is the variant-31 (and the K-outer tile kernel's) unsplit MFMA chain: bitwise equal to
// running the products one by one with split_k = 1.
constexpr TileVariantInfo KG = *tile_variant(V_ROLES_KOUT);
__global__ __launch_bounds__(KG.threads(), (KG.minb * KG.threads() / 64 + 3) / 4) void gemm_group_kernel(GemmGroup g) {
  const int total = g.tstart[g.n];
  for (int b = blockIdx.x; b < total; b += gridDim.x) {
    int i = 0;
    while (i + 1 < g.n && b >= g.tstart[i + 1]) ++i;
    const icap_gemm_args p = g.a[i];
    const int tn = g.tiles_n[i];
    const int tm = (g.tstart[i + 1] - g.tstart[i]) / tn;
    gemm_body<bf16_t, float, KG.nst, KG.minb, KG.wm, KG.wn, KG.tm, KG.tn, KG.kout, ACT_OFF, KG.roles>(p, tn, 1, g.nk[i], 0u, 1.f,
                                                                                                  b - g.tstart[i], tm, p.M);
  }
}

// The same group on 128 x 256 tiles (round 10), for groups that then fit one round of one block per compute unit (a
// mapper layer: 216 weight-gradient tiles + 27 exchanged bias tiles on 256 CUs, where the 128 x 128 body walks 486 in
// 1.9 rounds): 8 MFMA waves of 64 x 64 (two per SIMD) + 4 LDS-DMA waves on a ring of 3 stages of 64 k-rows x
// (128 + 256) columns (48 KiB each; the B image has 512-byte k-rows, gemm_tile.h kout_off). The k-step of a K-outer
// body is bound by its ds_read_b64_tr_b16 fragment reads, not by the fetch, and two reading waves
// per SIMD keep the LDS busier than one wave of 64 x 128 does: 0.91 against 1.03 us per k-step. Per output element the
// chain is the 128 x 128 body's: the same 16 x 16 x 32 MFMA over the same order of 64-deep k-steps, so the same bits.
// It is no row of TILE_VARIANTS: icap_gemm never plans it.
__global__ __launch_bounds__(768, 3) void gemm_group256_kernel(GemmGroup g) {
  const int total = g.tstart[g.n];
  for (int b = blockIdx.x; b < total; b += gridDim.x) {
    int i = 0;
    while (i + 1 < g.n && b >= g.tstart[i + 1]) ++i;
    const icap_gemm_args p = g.a[i];
    const int tn = g.tiles_n[i];
    const int tm = (g.tstart[i + 1] - g.tstart[i]) / tn;
    gemm_body<bf16_t, float, 3, 1, 2, 4, 4, 4, true, ACT_OFF, true>(p, tn, 1, g.nk[i], 0u, 1.f, b - g.tstart[i], tm, p.M,
                                                                   (g.swap >> i) & 1u);
  }
}

void launch_group_kout(const GemmGroup& g, int cus, bool big, hipStream_t s) {
  const int total = g.tstart[g.n];
  const dim3 grid((unsigned)(total < cus ? total : cus));
  if (big) hipLaunchKernelGGL(gemm_group256_kernel, grid, dim3(768), 0, s, g);
  else hipLaunchKernelGGL(gemm_group_kernel, grid, dim3(KG.threads()), 0, s, g);
}

}  // namespace icap
