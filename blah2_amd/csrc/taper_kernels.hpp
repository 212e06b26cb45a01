// Doppler taper of finished delay-Doppler maps: a cosine-sum slow-time window as a circular stencil along the Doppler
// rows (gfx950 / MI355X only).  No reference counterpart: Ambiguity.cpp:152-169 transforms the pulses unwindowed.
// Included by taper.hip alone: this header defines kernels, so a second unit must not include it.
//
//   taper_kernel<P>   M'[j][d] = t_0 M[j][d] + sum_{m=1..P} t_m (M[(j-m) mod nD][d] + M[(j+m) mod nD][d]) for every cell
//                     of n_maps maps, with the per-workgroup partials of Map::set_metrics (Map.cpp:187-206) of every
//                     output map.  The window w[i] = sum_p (-1)^p a_p cos(2 pi p i / nD) on the pulses in front of the
//                     Doppler transform is this stencil behind it, with t_0 = a_0, t_m = (-1)^m a_m / 2: the reference's
//                     row order is a rotation of the transform's, so circular neighbours stay neighbours.
//
// A thread OWNS one delay column of its strip of 256 and walks a segment of Doppler rows downwards with the input rows
// it needs in a ring of registers.  The walk is unrolled by the ring length R, so the slot of the q-th input row,
// q mod R, is a constant in every copy of the body and the ring stays in registers (nci_kernel's ring, along the
// Doppler axis).  R = 2P + 1 + TAPER_AHEAD: the 2P + 1 rows under the stencil and the rows whose loads are in flight
// ahead of the row being computed.  Every input cell comes from HBM once per segment; the 2P halo rows at a segment's
// ends are read by both neighbours.  Row indices wrap modulo nD.
//
// Every access is 8 bytes per lane, 512 contiguous bytes a wave, so the kernel is the same at every placement of the
// rows (with an odd nDelay consecutive rows alternate between 16-byte aligned and 8 bytes off, with an odd cell count
// consecutive maps too).  The walk is straight-line code with a lane mask on the stores: a lane past the row's end
// reads the row's last cell, a step past the segment's end its last row (never stored or counted), so that the wait
// in front of a row's arithmetic counts the loads issued behind it instead of draining them.
#pragma once

#include <hip/hip_runtime.h>

#include "blah2hip.h"
#include "metrics_core.hpp"

namespace blah2 {

struct TaperArgs {
  const cf *in;    // [nMaps][nD][nDelay]
  cf *out;         // [nMaps][nD][nDelay]
  double *partSum; // [nMaps][gridDim.x * gridDim.y]: metrics_kernel's layout
  float *partMax;
  float t[BLAH2HIP_MAX_TAPER_SIDE + 1]; // in the launch arguments: wave-uniform, read by scalar loads
  uint32_t nD, nDelay;
  uint32_t segRows; // Doppler rows per segment (the last one may be shorter)
};

typedef float taper_v2 __attribute__((ext_vector_type(2)));

// Rows in flight ahead of the stencil's own: a strip has few waves for this chip (one thread per column), so what a
// thread keeps in flight decides the rate
constexpr int TAPER_AHEAD = 8;
constexpr int TAPER_COLS = 256; // columns per strip: one per thread

// grid (strips, segments, maps), 256 threads.  No branch but the loop's (uniform over the workgroup) and the store's lane mask.
template <int P>
__global__ __launch_bounds__(256) void taper_kernel(TaperArgs a)
{
  constexpr int W = 2 * P + 1, R = W + TAPER_AHEAD;
  const uint32_t nD = a.nD, nDelay = a.nDelay;
  const uint32_t col = blockIdx.x * TAPER_COLS + threadIdx.x;
  const bool on = col < nDelay;
  const uint32_t cc = on ? col : nDelay - 1; // the column the lane reads: its own, or the row's last cell
  const uint32_t r0 = blockIdx.y * a.segRows;
  const uint32_t n = nD - r0 < a.segRows ? nD - r0 : a.segRows; // output rows r0 .. r0 + n - 1
  const uint32_t T = n + 2 * P;                                 // input rows: q = 0 .. T - 1 is row (r0 - P + q) mod nD
  const size_t mapOff = (size_t)blockIdx.z * nD * nDelay;
  const taper_v2 *in = reinterpret_cast<const taper_v2 *>(a.in + mapOff) + cc; // the lane's cell of the map's row 0
  taper_v2 *pout = reinterpret_cast<taper_v2 *>(a.out + mapOff + (size_t)r0 * nDelay) + cc; // ... of the next output row

  // The walk is straight-line code: a load is issued at every step, and behind the segment's last input row it reads
  // that row again (the same address: nothing new comes from HBM); the steps behind the last output row compute cells
  // that are neither stored nor counted.
  taper_v2 ring[R];
  uint32_t row = r0 >= (uint32_t)P ? r0 - P : r0 + nD - P; // the row of the next load (nD >= 2P + 1 > P)
  uint32_t q = 0;                                          // ... and its index in the segment's input rows
  // the first R - 1 input rows: those under the first output row but its last, and the rows in flight
#pragma unroll
  for (int k = 0; k < R - 1; k++) {
    ring[k] = in[(size_t)row * nDelay];
    if (++q < T) row = row + 1 == nD ? 0 : row + 1;
  }
  ring[R - 1] = taper_v2{0.f, 0.f};

  double lsum = 0.0;
  float lmax = 0.f;
#pragma unroll 1
  for (uint32_t base = 0; base < n; base += R) {
#pragma unroll
    for (int s = 0; s < R; s++) {
      const uint32_t i = base + s; // output row r0 + i from the input rows i .. i + 2P, slots (s + m) mod R
      const bool live = on && i < n;
      // the slot of input row i - 1 is free: the load of input row i + R - 1 goes there
      ring[(s + R - 1) % R] = in[(size_t)row * nDelay];
      if (++q < T) row = row + 1 == nD ? 0 : row + 1;
      // per component: t_0 M[j], then fma(t_m, M[j - m]) and fma(t_m, M[j + m]) for m = 1 .. P -- 2P + 1 roundings
      const taper_v2 c = ring[(s + P) % R];
      float re = __fmul_rn(a.t[0], c[0]), im = __fmul_rn(a.t[0], c[1]);
#pragma unroll
      for (int m = 1; m <= P; m++) {
        const taper_v2 lo = ring[(s + P - m) % R], hi = ring[(s + P + m) % R];
        re = fmaf(a.t[m], lo[0], re);
        im = fmaf(a.t[m], lo[1], im);
        re = fmaf(a.t[m], hi[0], re);
        im = fmaf(a.t[m], hi[1], im);
      }
      if (live) *pout = taper_v2{re, im};
      pout += nDelay;
      // Map::set_metrics of the cells as written; a zero cell is -inf, as in the Doppler kernels' epilogues.  A step
      // without a cell adds 0 and leaves the max (which starts at 0) alone.
      const float db = db_of(cmake(re, im));
      lsum += live ? (double)db : 0.0;
      lmax = fmaxf(lmax, live ? db : 0.f);
    }
  }
  // one (sum, max) partial per workgroup; metrics_kernel folds a map's partials in index order
  const size_t part = (size_t)blockIdx.z * (gridDim.x * gridDim.y) + blockIdx.y * gridDim.x + blockIdx.x;
  block_metrics_partial(lsum, lmax, a.partSum + part, a.partMax + part);
}

// taper_kernel<P> for the stencil's half width
inline void launch_taper(uint32_t P, dim3 grid, hipStream_t st, const TaperArgs &a)
{
  switch (P) {
#define B2_TAPER(N) case N: hipLaunchKernelGGL(taper_kernel<N>, grid, dim3(256), 0, st, a); break;
  B2_TAPER(0) B2_TAPER(1) B2_TAPER(2) B2_TAPER(3) B2_TAPER(4)
#undef B2_TAPER
  }
}

} // namespace blah2
