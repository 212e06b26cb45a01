// Ordered-statistic detector kernels of the blah2 engine (gfx950 / MI355X only).
// Included by detect.hip alone: this header defines kernels, so a second unit must not include it.
//
//   oscfar1d_kernel   OS-CFAR along delay with the geometry of cfar1d_kernel (CfarDetector1D.cpp:23-100)
//   oscfar2d_kernel   OS-CFAR over the 2-D window of blah2hip_cfar2d_*: a tile + halo of |z|^2 in LDS
//
// No reference counterpart (the reference only averages its training cells); the rule is include/blah2hip.h's.
#pragma once

#include <hip/hip_runtime.h>

#include "blah2hip.h"
#include "cfar_kernels.hpp"

namespace blah2 {

// --------------------------------------------------------------------------
// The rule, for a cell under test c with n in-bounds training cells p_1 .. p_n (p = |z|^2 in fp64, formed as
// cfar1d_kernel forms it):
//   hit  <=>  n >= 1  and  #{ i : alpha[n] * p_i < p_c } >= rank[n]
// which is p_c > alpha[n] * x_(k), k = rank[n], x_(k) the k-th smallest training cell (multiplying by alpha > 0 and
// rounding is monotone), without forming x_(k): no sort, a count of n multiply-compares.  The special values follow
// from the compare alone: a NaN or +Inf training cell is never "below", a NaN cell under test is above nothing, and
// alpha[0] = NaN (no training cell) never counts.  There is no first pass that discards cells: every tested cell
// takes its n compares.
struct OsCfarArgs {
  CfarArgs c;           // alpha: the ordered-statistic factors [2*nTrain+1]
  const uint32_t *rank; // [2*nTrain+1]: k(n)
};

// row_detect's geometry (cfar_kernels.hpp), and a count of n multiply-compares over the two runs
template <bool STAGED>
__global__ __launch_bounds__(256) void oscfar1d_kernel(OsCfarArgs oa)
{
  row_detect<STAGED>(oa.c, [&](int l0, int l1, int t0, int t1, auto sqv, int j) {
    const int n = max(l1 - l0, 0) + (t1 - t0);
    if (n == 0) return false;
    const double al = oa.c.alpha[n], sj = sqv(j);
    const uint32_t need = oa.rank[n];
    uint32_t below = 0;
    for (int k = l0; k < l1; k++) below += (al * sqv(k) < sj) ? 1u : 0u;
    for (int k = t0; k < t1; k++) below += (al * sqv(k) < sj) ? 1u : 0u;
    return below >= need;
  });
}

// --------------------------------------------------------------------------
// The 2-D window of cfar2d_kernel (rectangle minus guard box, in-bounds cells only, delay column 0 never trains).
// A workgroup of four waves owns O2_ROWS x O2_COLS cells under test; |z|^2 of the tile and its halo (hR = nGf + nTf
// rows, hC = nGd + nTd columns on either side) goes to LDS as fp64 with every cell that does not train -- outside the
// map, or in delay column 0 -- written as +Inf: alpha * Inf is never below anything, so such a cell takes no rank and
// the count loop needs no bounds test.  n follows from the clipped window as in cfar2d_kernel.
// lane <-> column, wave <-> four neighbouring rows, a lane's four cells one after the other.  Per cell and training
// cell: one ds_read_b64 (lanes on neighbouring doubles: conflict-free, two LDS cycles per wave), one fp64 multiply, one
// compare, one add, in straight runs along the window's rows.  (A first form read each value once for the up to four
// cells it trains and chose the cells by wave-uniform branches per value: 6.1 x the averaging kernel's time at 1025 x
// 2048, against 1.6 x for this one -- the branches, not the LDS reads, were the cost)  The cell under test is read from
// the map itself (column 0 is +Inf in LDS), the same arithmetic.
// LDS: (16 + 2 hR)(64 + 2 hC | 1) doubles: 15.6 KB for the 17 x 9 window, 74 KB at the halo limits (hR 24, hC 40).
constexpr int O2_ROWS = 16, O2_COLS = HALO_COLS, O2_M = 4;
__host__ inline size_t o2_lds_bytes(int hC, int hR) { return (size_t)(O2_ROWS + 2 * hR) * halo_pitch(hC) * sizeof(double); }

struct OsCfar2dArgs {
  Cfar2dArgs d;         // alpha: the ordered-statistic factors; sat unused
  const uint32_t *rank; // [maxN + 1]
};

__global__ __launch_bounds__(256) void oscfar2d_kernel(OsCfar2dArgs oa)
{
  const Cfar2dArgs &a = oa.d;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double *T = reinterpret_cast<double *>(smem);
  const int hR = a.ngF + a.ntF, hC = a.ngD + a.ntD;
  const int SP = halo_pitch(hC);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nD = a.nD, nC = a.nDelay;
  const int j0 = blockIdx.x * O2_COLS, i0 = blockIdx.y * O2_ROWS, cpi = blockIdx.z;
  const cf *map = a.map + (size_t)cpi * nD * nC;
  halo_fill(T, map, nD, nC, i0, j0, O2_ROWS, hR, hC, __builtin_huge_val(), wave, lane);
  __syncthreads();

  // this lane's four cells: rows i0 + 4 wave + m of column j0 + lane
  const int j = j0 + lane, o = wave * O2_M;
  auto clampi = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
  auto cols = [](int c0, int c1) { return max(c1, 1) - max(c0, 1); }; // column 0 never trains
  const bool jok = j < nC && j + a.delayMin >= a.minDelay;
  const int nColsAll = cols(clampi(j - hC, 0, nC), clampi(j + hC + 1, 0, nC));
  const int nColsGuard = cols(clampi(j - a.ngD, 0, nC), clampi(j + a.ngD + 1, 0, nC));
  double p[O2_M], al[O2_M];
  uint32_t need[O2_M], below[O2_M];
  bool any = false;
#pragma unroll
  for (int m = 0; m < O2_M; m++) {
    const int i = i0 + o + m;
    p[m] = al[m] = __builtin_nan(""); // a cell that is not tested: nothing is below NaN
    need[m] = 0xFFFFFFFFu;
    below[m] = 0;
    if (jok && i < nD && !(fabs(a.doppler[i]) < a.minDoppler)) {
      const int n = (clampi(i + hR + 1, 0, nD) - clampi(i - hR, 0, nD)) * nColsAll -
                    (clampi(i + a.ngF + 1, 0, nD) - clampi(i - a.ngF, 0, nD)) * nColsGuard;
      if (n > 0) {
        p[m] = cell_power(map[(size_t)i * nC + j]);
        al[m] = a.alpha[n];
        need[m] = oa.rank[n];
        any = true;
      }
    }
  }
  if (!__any(any)) return; // (no barrier follows)

  // Cell m's window is the tile rows o + m .. o + m + 2 hR, columns lane .. lane + 2 hC.  Its rows are walked as runs of
  // neighbouring columns -- a whole row outside the guard rows, the nTd columns either side of the guard inside them -- so
  // the loop body is a read, a multiply, a compare and an add, and the only branches are the runs' ends.
#define O2_RUN(C0, C1)                                                                    \
  _Pragma("unroll 8") for (int c = (C0); c < (C1); c++) cnt += (alm * row[c] < pm) ? 1u : 0u
#pragma unroll
  for (int m = 0; m < O2_M; m++) {
    if (!__any(need[m] != 0xFFFFFFFFu)) continue; // a row none of whose cells is tested (wave-uniform)
    const double alm = al[m], pm = p[m];
    uint32_t cnt = 0;
    for (int r = 0; r <= 2 * hR; r++) {
      const double *row = T + (o + m + r) * SP + lane;
      if (r < a.ntF || r > a.ntF + 2 * a.ngF) {
        O2_RUN(0, 2 * hC + 1);
      } else { // a guard row: the training columns left and right of the guard box
        O2_RUN(0, a.ntD);
        O2_RUN(a.ntD + 2 * a.ngD + 1, 2 * hC + 1);
      }
    }
    below[m] = cnt;
  }
#undef O2_RUN

  const double noise = a.metrics[2 * cpi];
#pragma unroll
  for (int m = 0; m < O2_M; m++) {
    if (below[m] >= need[m]) append_hit(a.hits, a.count, a.cap, cpi, i0 + o + m, j, p[m], noise);
  }
}

} // namespace blah2
