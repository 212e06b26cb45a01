// Greatest-of / smallest-of detector kernels of the blah2 engine (gfx950 / MI355X only).
// Included by detect.hip alone: this header defines kernels, so a second unit must not include it.
//
//   gocfar1d_kernel   GO / SO CFAR along delay with the geometry of cfar1d_kernel (CfarDetector1D.cpp:23-100)
//   gocfar2d_kernel   the same halves averaged over 2 hR + 1 Doppler rows: a tile + halo of |z|^2 and its column sums in LDS
//
// No reference counterpart (the reference only averages its whole window); the rule is include/blah2hip.h's.
#pragma once

#include <hip/hip_runtime.h>

#include "blah2hip.h"
#include "cfar_kernels.hpp"

namespace blah2 {

// --------------------------------------------------------------------------
// The rule, for a cell under test c whose leading half has a in-bounds cells of sum S_A and whose lagging half has b of
// sum S_B (p = |z|^2 in fp64, formed as cfar1d_kernel forms it; the sums from 0.0 in ascending index):
//   a, b >= 1:   hA = p_c > alpha * (S_A / a),  hB = p_c > alpha * (S_B / b);   greatest-of: hA and hB,  smallest-of: hA or hB
//   one empty:   p_c > alpha * (S / (a + b)) over the other half, alpha the cell-averaging factor
//   both empty:  no hit
// -- one divide, one multiply and one compare per half; no max or min is formed, so a NaN half never supports a hit and a
// NaN cell under test never hits.  The factor comes from a table on the device, indexed by what fixes (a, b):
//   alpha[((rows - 1) (nT + 1) + cL) (nT + 1) + cR],   a = rows cL, b = rows cR
// rows the window's in-bounds Doppler rows (1 for the 1-D detector), cL and cR the in-bounds training columns of the halves,
// 0 .. nT each.  detect.hip fills the entries the map's geometry reaches and leaves the others NaN.
__device__ inline bool gocfar_decide(double p, double al, double SA, double SB, int na, int nb, uint32_t kind)
{
  if (na > 0 && nb > 0) {
    const bool hA = p > al * (SA / (double)na), hB = p > al * (SB / (double)nb);
    return kind == BLAH2HIP_CFAR_GO ? (hA && hB) : (hA || hB);
  }
  return p > al * ((na > 0 ? SA : SB) / (double)(na + nb));
}

struct GoCfarArgs {
  CfarArgs c; // alpha: the table above with rows = 1, (nTrain + 1)^2 doubles
  uint32_t kind;
};

// row_detect's geometry (cfar_kernels.hpp): cfar1d_kernel's loads and adds, in two sums, plus a second divide, multiply and
// compare
template <bool STAGED>
__global__ __launch_bounds__(256) void gocfar1d_kernel(GoCfarArgs ga)
{
  row_detect<STAGED>(ga.c, [&](int l0, int l1, int t0, int t1, auto sqv, int j) {
    const int na = max(l1 - l0, 0), nb = t1 - t0;
    if (na + nb == 0) return false;
    double SA = 0.0, SB = 0.0;
    for (int k = l0; k < l1; k++) SA += sqv(k);
    for (int k = t0; k < t1; k++) SB += sqv(k);
    return gocfar_decide(sqv(j), ga.c.alpha[na * (ga.c.nTrain + 1) + nb], SA, SB, na, nb, ga.kind);
  });
}

// --------------------------------------------------------------------------
// The 2-D detector: the halves of the 1-D detector (nGd guard and nTd training columns either side), each over the rows
// i - hR .. i + hR inside the map; the columns j - nGd .. j + nGd train in no row.  A workgroup of four waves owns
// G2_ROWS x G2_COLS cells under test.  |z|^2 of the tile and its halo (hR rows, hC = nGd + nTd columns on either side)
// goes to LDS as fp64, every cell that does not train -- outside the map, or in delay column 0 -- as 0.0: p >= +0, so adding
// it changes no bit of a sum and the loops need no bounds test; the counts a and b follow from the clipped window.
// Then, in the fixed order of the definition,
//   C[r][c] = sum over the 2 hR + 1 rows of tile column c for the cells' row r, ascending, from 0.0   once per (row, column),
//                                                                                                      shared by the 2 nTd cells that use it
//   S_A = sum_{c < nTd} C[r][lane + c],   S_B = sum_{c < nTd} C[r][lane + hC + nGd + 1 + c]             ascending, from 0.0
// -- additions only: no sliding add-and-subtract, no prefix table.  lane <-> column, wave <-> four neighbouring rows in
// both steps, so a wave reads the column sums it wrote; lanes read neighbouring doubles (ds_read_b64 of 32 lanes over 64
// banks: conflict-free at any pitch; the odd pitch is oscfar2d_kernel's).  The cell under test is read from the map itself
// (column 0 is 0.0 in LDS).  Per tile (2 hR + 1) 16 (64 + 2 hC) + 2 nTd 16 64 LDS reads: 23 808 for the 17 x 9 window's extent
// (hR 4, nGd 2, nTd 6), where oscfar2d_kernel reads each of a cell's 138 training cells: 141 312.
// LDS: (16 + 2 hR + 16)(64 + 2 hC | 1) doubles: 25.3 KB for hR 4, hC 8; 90.6 KB at the halo limits (hR 24, hC 40).
constexpr int G2_ROWS = 16, G2_COLS = HALO_COLS, G2_M = 4;
__host__ inline size_t g2_lds_bytes(int hC, int hR) { return (size_t)(2 * G2_ROWS + 2 * hR) * halo_pitch(hC) * sizeof(double); }

struct GoCfar2dArgs {
  Cfar2dArgs d; // ngD, ntD: the halves; ntF: hR (ngF 0); alpha: the table above, (2 hR + 1)(nTd + 1)^2 doubles; sat unused
  uint32_t kind;
};

__global__ __launch_bounds__(256) void gocfar2d_kernel(GoCfar2dArgs ga)
{
  const Cfar2dArgs &a = ga.d;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int hR = a.ntF, g = a.ngD, t = a.ntD, hC = g + t;
  const int SP = halo_pitch(hC), SC = G2_COLS + 2 * hC, SR = G2_ROWS + 2 * hR;
  double *P = reinterpret_cast<double *>(smem), *Cs = P + SR * SP;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nD = a.nD, nC = a.nDelay;
  const int j0 = blockIdx.x * G2_COLS, i0 = blockIdx.y * G2_ROWS, cpi = blockIdx.z;
  const cf *map = a.map + (size_t)cpi * nD * nC;

  halo_fill(P, map, nD, nC, i0, j0, G2_ROWS, hR, hC, 0.0, wave, lane);
  __syncthreads();

  // the column sums of this wave's four rows of cells: the cells' row o + m spans the tile rows o + m .. o + m + 2 hR
  const int o = wave * G2_M;
#pragma unroll
  for (int m = 0; m < G2_M; m++) {
    if (i0 + o + m >= nD) break; // (wave-uniform)
    for (int c = lane; c < SC; c += 64) {
      const double *q = P + (o + m) * SP + c;
      double s = 0.0;
#pragma unroll 4
      for (int r = 0; r <= 2 * hR; r++) s += q[r * SP];
      Cs[(o + m) * SP + c] = s;
    }
  }
  __syncthreads();

  // this lane's four cells: rows i0 + 4 wave + m of column j0 + lane
  const int j = j0 + lane;
  auto clampi = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
  if (!(j < nC && j + a.delayMin >= a.minDelay)) return; // (no barrier follows)
  const int cL = max(min(j - g, nC) - max(j - hC, 1), 0);
  const int cR = min(j + hC + 1, nC) - min(j + g + 1, nC);
  if (cL + cR == 0) return;
  const double noise = a.metrics[2 * cpi];
#pragma unroll
  for (int m = 0; m < G2_M; m++) {
    const int i = i0 + o + m;
    if (i >= nD) break;
    if (fabs(a.doppler[i]) < a.minDoppler) continue;
    const int rows = clampi(i + hR + 1, 0, nD) - clampi(i - hR, 0, nD);
    const double *row = Cs + (o + m) * SP + lane;
    double SA = 0.0, SB = 0.0;
#pragma unroll 4
    for (int c = 0; c < t; c++) SA += row[c];
#pragma unroll 4
    for (int c = 0; c < t; c++) SB += row[hC + g + 1 + c];
    const double p = cell_power(map[(size_t)i * nC + j]);
    const double al = a.alpha[((rows - 1) * (t + 1) + cL) * (t + 1) + cR];
    if (gocfar_decide(p, al, SA, SB, rows * cL, rows * cR, ga.kind)) append_hit(a.hits, a.count, a.cap, cpi, i, j, p, noise);
  }
}

} // namespace blah2
