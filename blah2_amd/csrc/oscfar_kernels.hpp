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

// One workgroup per Doppler row like cfar1d_kernel; leading cells need k > 0, trailing k >= 0 (CfarDetector1D.cpp:61,
// :68), rows with |doppler| < minDoppler and cells with delay < minDelay are not tested (:40, :53).  STAGED: the row's
// |z|^2 in LDS as fp64 (lanes read neighbouring doubles: no bank conflict); false: rows longer than the LDS holds,
// |z|^2 from the L2-resident row.
template <bool STAGED>
__global__ __launch_bounds__(256) void oscfar1d_kernel(OsCfarArgs oa)
{
  const CfarArgs &a = oa.c;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double *sq = reinterpret_cast<double *>(smem);
  const int row = blockIdx.x, cpi = blockIdx.y;
  if (fabs(a.doppler[row]) < a.minDoppler) return;
  const cf *z = a.map + ((size_t)cpi * a.nD + row) * a.nDelay;
  auto sqv = [&](int k) -> double {
    if (STAGED) return sq[k];
    const cf c = z[k];
    return (double)c.x * (double)c.x + (double)c.y * (double)c.y;
  };
  if (STAGED) {
    for (int j = threadIdx.x; j < a.nDelay; j += blockDim.x) {
      const cf c = z[j];
      sq[j] = (double)c.x * (double)c.x + (double)c.y * (double)c.y;
    }
    __syncthreads();
  }
  const double noisePower = a.metrics[2 * cpi];
  for (int j = threadIdx.x; j < a.nDelay; j += blockDim.x) {
    if ((a.delayAxis ? a.delayAxis[j] : j + a.delayMin) < a.minDelay) continue;
    // the two runs of training cells, clipped to the row: [l0, l1) before the guard (never column 0), [t0, t1) behind it
    const int l0 = max(j - a.nGuard - a.nTrain, 1), l1 = min(j - a.nGuard, a.nDelay);
    const int t0 = max(j + a.nGuard + 1, 0), t1 = min(j + a.nGuard + a.nTrain + 1, a.nDelay);
    const int n = max(l1 - l0, 0) + max(t1 - t0, 0);
    if (n == 0) continue;
    const double al = a.alpha[n], sj = sqv(j);
    const uint32_t need = oa.rank[n];
    uint32_t below = 0;
    for (int k = l0; k < l1; k++) below += (al * sqv(k) < sj) ? 1u : 0u;
    for (int k = t0; k < t1; k++) below += (al * sqv(k) < sj) ? 1u : 0u;
    if (below >= need) {
      const uint32_t slot = atomicAdd(&a.count[cpi], 1u);
      if (slot < a.cap) {
        blah2hip_hit_t h;
        h.row = row;
        h.col = j;
        h.snr = 5.0 * log10(sj) - noisePower;
        a.hits[(size_t)cpi * a.cap + slot] = h;
      }
    }
  }
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
constexpr int O2_ROWS = 16, O2_COLS = 64, O2_M = 4;
__host__ __device__ inline int o2_pitch(int hC) { return (O2_COLS + 2 * hC) | 1; }
__host__ inline size_t o2_lds_bytes(int hC, int hR) { return (size_t)(O2_ROWS + 2 * hR) * o2_pitch(hC) * sizeof(double); }

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
  const int SP = o2_pitch(hC), SC = O2_COLS + 2 * hC, SR = O2_ROWS + 2 * hR;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nD = a.nD, nC = a.nDelay;
  const int j0 = blockIdx.x * O2_COLS, i0 = blockIdx.y * O2_ROWS, cpi = blockIdx.z;
  const cf *map = a.map + (size_t)cpi * nD * nC;
  const double inf = __builtin_huge_val();

  for (int r = wave; r < SR; r += 4) {
    const int i = i0 - hR + r;
    const bool rok = i >= 0 && i < nD;
    for (int c = lane; c < SC; c += 64) {
      const int j = j0 - hC + c;
      double v = inf;
      if (rok && j >= 1 && j < nC) {
        const cf q = map[(size_t)i * nC + j];
        v = (double)q.x * (double)q.x + (double)q.y * (double)q.y;
      }
      T[r * SP + c] = v;
    }
  }
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
        const cf q = map[(size_t)i * nC + j];
        p[m] = (double)q.x * (double)q.x + (double)q.y * (double)q.y;
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
    if (below[m] < need[m]) continue;
    const uint32_t slot = atomicAdd(&a.count[cpi], 1u);
    if (slot < a.cap) {
      blah2hip_hit_t h;
      h.row = i0 + o + m;
      h.col = j;
      h.snr = 5.0 * log10(p[m]) - noise;
      a.hits[(size_t)cpi * a.cap + slot] = h;
    }
  }
}

} // namespace blah2
