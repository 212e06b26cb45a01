// Multi-carrier integration (gfx950 / MI355X only): the power maps of C carriers summed on ONE Doppler axis.  No reference
// counterpart.  The definition is include/blah2hip.h's.  Included by carriers.hip alone: this header defines a kernel.
//
//   carrier_sum_kernel<C>   S = sum_c w_c (a_lo |M_c[row]|^2 + a_hi |M_c[row + 1]|^2) per cell, out = (sqrt(scale S), 0),
//                           and the per-workgroup partials of Map::set_metrics of every output map.
//
// An echo of one range rate sits in another Doppler row of every carrier's map, so the sum is a gather along the Doppler
// axis.  For a given (carrier, output row) the table entry (row, a_lo, a_hi) is the same along the row, so a wave works
// along the delay axis of ONE output row: track_sum_kernel's shape.  The row index is made wave-uniform with readfirstlane
// and every table load stands in front of the kernel's first global store, so the compiler may keep the entries in scalar
// registers; the a_hi != 0 branch is wave-uniform with them.  A lane loads 8 bytes (one cell), a wave 512 contiguous bytes
// of a source row, masked at the map's right edge; every carrier's loads of a row (up to 2 C = 16) are issued before the
// arithmetic.  Plain loads, not streaming ones: with linear interpolation, or ratios above 1, a source row is read by two
// or three output rows, and L2 should serve the repeats.  No LDS besides block_metrics_partial's.  A workgroup is four
// waves over a tile of 64 columns x 8 rows, two rows a wave: the Doppler kernels' tile, so the handle's metrics partials
// suffice (one per 512 cells).
#pragma once

#include <hip/hip_runtime.h>

#include "blah2hip.h"
#include "metrics_core.hpp"

namespace blah2 {

constexpr int CAR_COLS = 64, CAR_ROWS = 8; // a workgroup's tile: 4 waves of 2 rows

// one (carrier, output row) of the table blah2hip_amb_set_carriers uploads: 16 bytes, one scalar load
struct CarrierEntry {
  int32_t row;    // the lower source row, 0 .. nD - 1
  float aLo, aHi; // its weight and that of row + 1; aHi == 0: row + 1 is not read
  uint32_t pad;
};

struct CarrierArgs {
  const cf *in;            // [C][nCpi][nD][nDelay]
  const CarrierEntry *tab; // [C][nD]
  cf *out;                 // [nCpi][nD][nDelay]
  double *partSum;         // [nCpi][gridDim.x]: metrics_kernel's layout
  float *partMax;
  float w[BLAH2HIP_MAX_CARRIERS]; // in the launch arguments: wave-uniform, read by scalar loads
  float scale;             // 1 / sum_c w_c, rounded to fp32 on the host
  int32_t nD, nDelay;
  uint32_t nCpi;
  uint32_t strips;         // ceil(nDelay / 64)
};

// grid (strips * ceil(nD / 8), nCpi), 256 threads.  The branch around a row is wave-uniform, and every wave reaches the
// barrier of block_metrics_partial.
template <int C>
__global__ __launch_bounds__(256) void carrier_sum_kernel(CarrierArgs a)
{
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const uint32_t strip = blockIdx.x % a.strips, group = blockIdx.x / a.strips, o = blockIdx.y;
  const int32_t nD = a.nD, nDelay = a.nDelay;
  const int32_t d = (int32_t)(strip * CAR_COLS) + lane;
  const bool live = d < nDelay;
  const size_t cells = (size_t)nD * nDelay;
  const size_t carStride = (size_t)a.nCpi * cells;
  const cf *cpi = a.in + (size_t)o * cells + (live ? d : 0);
  float z[2] = {0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int32_t j = (int32_t)(group * CAR_ROWS) + wave * 2 + i;
    if (j < nD) {
      CarrierEntry e[C];
      cf lo[C], hi[C];
#pragma unroll
      for (int c = 0; c < C; c++) {
        e[c] = a.tab[(size_t)c * nD + j];
        // the host's table keeps row in [0, nD - 1] and aHi == 0 at row nD - 1; the clamps only keep a load inside the map
        const int32_t r0 = min(max(e[c].row, 0), nD - 1), r1 = min(r0 + 1, nD - 1);
        const cf *m = cpi + (size_t)c * carStride;
        lo[c] = cmake(0.f, 0.f);
        hi[c] = cmake(0.f, 0.f);
        if (live) lo[c] = m[(size_t)r0 * nDelay];
        if (e[c].aHi != 0.f) {
          if (live) hi[c] = m[(size_t)r1 * nDelay];
        }
      }
      float S = 0.f;
#pragma unroll
      for (int c = 0; c < C; c++) {
        const float pLo = fmaf(lo[c].x, lo[c].x, __fmul_rn(lo[c].y, lo[c].y));
        float q = __fmul_rn(e[c].aLo, pLo);
        if (e[c].aHi != 0.f) {
          const float pHi = fmaf(hi[c].x, hi[c].x, __fmul_rn(hi[c].y, hi[c].y));
          q = fmaf(e[c].aHi, pHi, q);
        }
        S = fmaf(a.w[c], q, S);
      }
      z[i] = sqrtf(__fmul_rn(a.scale, S));
    }
  }
  // the stores, behind every table load; Map::set_metrics of the cells as written (a zero cell is -inf, as in nci_kernel)
  double lsum = 0.0;
  float lmax = 0.f;
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int32_t j = (int32_t)(group * CAR_ROWS) + wave * 2 + i;
    if (j < nD && live) {
      a.out[(size_t)o * cells + (size_t)j * nDelay + d] = cmake(z[i], 0.f);
      const float db = db_of(cmake(z[i], 0.f));
      lsum += (double)db;
      lmax = fmaxf(lmax, db);
    }
  }
  const size_t part = (size_t)o * gridDim.x + blockIdx.x;
  block_metrics_partial(lsum, lmax, a.partSum + part, a.partMax + part);
}

// carrier_sum_kernel<C> for the table's carrier count
inline void launch_carrier_sum(uint32_t C, dim3 grid, hipStream_t st, const CarrierArgs &a)
{
  switch (C) {
#define B2_CAR(N) case N: hipLaunchKernelGGL(carrier_sum_kernel<N>, grid, dim3(256), 0, st, a); break;
  B2_CAR(1) B2_CAR(2) B2_CAR(3) B2_CAR(4) B2_CAR(5) B2_CAR(6) B2_CAR(7) B2_CAR(8)
#undef B2_CAR
  }
}

} // namespace blah2
