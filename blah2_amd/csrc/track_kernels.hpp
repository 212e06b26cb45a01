// Integration along tracks (gfx950 / MI355X only): the integrator's window sums taken along the walk of an echo in delay
// and, for a bank of drift hypotheses, in Doppler.  No reference counterpart.  The definition is include/blah2hip.h's.
// Included by integrate.hip alone, behind integrate_kernels.hpp: this header defines kernels and uses nci_power.
//
//   track_power_kernel   p[c] = sum_k w_k |M_k[c]|^2 of the call's CPIs into the ring of fp32 planes, plane (g0 + c) mod R.
//                        nci_power itself, on nci_kernel's ownership of two adjacent cells per thread, a group of NCI_GROUP
//                        CPIs per workgroup: every input cell comes from HBM once, by streaming loads, and p has
//                        nci_kernel's bits.
//   track_sum_kernel     S_k = sum over the ages a = W - 1 .. 0 of p[g - a][jr(j,k,a)][d + s(j,k,a)], the strongest k per
//                        cell, out = (sqrt(scale S), 0), the index byte and the metrics partials.
//
// For a given (row, hypothesis, age) the source row jr and the shift s are the same along the row, so a wave works along the
// delay axis of ONE row: it reads the (jr, s) pair by a scalar load from the table the host built (the row index is made
// wave-uniform with readfirstlane, and every table load stands in front of the kernel's first global store, so that the
// compiler may keep them scalar), and gathers 4 bytes per lane at d + s -- 256 contiguous bytes a wave, masked at the map's
// ends.  No LDS for the gather.  The running best (S, k) stays in registers across the bank.  A workgroup is four waves
// over a tile of 64 columns x 8 rows, two rows a wave: the Doppler kernels' tile, so the handle's metrics partials suffice
// (one per 512 cells).
#pragma once

#include <hip/hip_runtime.h>

#include "blah2hip.h"
#include "integrate_kernels.hpp"
#include "metrics_core.hpp"

namespace blah2 {

constexpr int TRK_COLS = 64, TRK_ROWS = 8; // a workgroup's tile: 4 waves of 2 rows
constexpr int TRK_AGES = 4;                // gathers a lane keeps in flight

struct TrackPowerArgs {
  NciArgs n;        // nci_power's: in [K][nCpi][cells], w, K, cells, nCpi
  float *ring;      // [ringLen][cells]
  uint32_t ringLen; // W - 1 + max_cpi
  uint32_t slot0;   // the plane of the call's first CPI: g0 mod ringLen
};

// grid (G, ceil(nCpi / NCI_GROUP)), 256 threads, G * 256 >= the map's units of two cells
__global__ __launch_bounds__(256) void track_power_kernel(TrackPowerArgs a)
{
  const size_t cells = a.n.cells;
  const size_t nUnits = (cells + 1) / 2;
  const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool on = u < nUnits;
  const size_t i0 = 2 * u;
  const bool two = on && i0 + 1 < cells; // an odd cell count: the last unit is one cell
  const uint32_t c0 = blockIdx.y * NCI_GROUP;
  const uint32_t n = a.n.nCpi - c0 < (uint32_t)NCI_GROUP ? a.n.nCpi - c0 : (uint32_t)NCI_GROUP;
  const cf *first = a.n.in + (size_t)c0 * cells;
  float p0[NCI_GROUP], p1[NCI_GROUP];
  nci_power(a.n, first + i0, (uintptr_t)first, cells, (size_t)a.n.nCpi * cells, n, on, two, p0, p1);
#pragma unroll
  for (int t = 0; t < NCI_GROUP; t++) {
    if ((uint32_t)t < n) {
      const uint32_t slot = (a.slot0 + c0 + t) % a.ringLen;
      float *plane = a.ring + (size_t)slot * cells;
      // a plane of an odd cell count may start 4 bytes off an 8-byte boundary: a wave-uniform choice per plane
      if (!((uintptr_t)plane & 7) && two) {
        *reinterpret_cast<nci_v2 *>(plane + i0) = nci_v2{p0[t], p1[t]};
      } else {
        if (on) plane[i0] = p0[t];
        if (two) plane[i0 + 1] = p1[t];
      }
    }
  }
}

struct TrackSumArgs {
  const float *ring;  // [ringLen][nD][nDelay]
  const int2 *tab;    // [K][W][nD]: (jr, s); jr < 0: the row lies outside the map
  cf *out;            // [nOut][nD][nDelay]
  uint8_t *index;     // [nOut][nD][nDelay], or nullptr
  double *partSum;    // [nOut][gridDim.x]: metrics_kernel's layout
  float *partMax;
  float scale;        // 1 / (W sum_k w_k), rounded to fp32 on the host
  int32_t nD, nDelay;
  uint32_t W, K;      // window, hypotheses
  uint32_t ringLen;
  uint32_t slotFirst; // the plane of the CPI at which the first window ends: first_end mod ringLen
  uint32_t hopMod;    // hop mod ringLen
  uint32_t strips;    // ceil(nDelay / 64)
};

// grid (strips * ceil(nD / 8), nOut), 256 threads.  The branch around a row is wave-uniform, and every wave reaches the barrier
// of block_metrics_partial.
__global__ __launch_bounds__(256) void track_sum_kernel(TrackSumArgs a)
{
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const uint32_t strip = blockIdx.x % a.strips, group = blockIdx.x / a.strips, o = blockIdx.y;
  const int32_t nD = a.nD, nDelay = a.nDelay;
  const int32_t d = (int32_t)(strip * TRK_COLS) + lane;
  const size_t cells = (size_t)nD * nDelay;
  const uint32_t R = a.ringLen;
  const uint32_t slotG = (a.slotFirst + (uint32_t)(((uint64_t)o * a.hopMod) % R)) % R; // the plane of age 0
  float z[2] = {0.f, 0.f};
  uint32_t kBest[2] = {0, 0};
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int32_t j = (int32_t)(group * TRK_ROWS) + wave * 2 + i;
    if (j < nD) {
      float best = 0.f;
      uint32_t bk = 0;
      for (uint32_t k = 0; k < a.K; k++) {
        const int2 *tk = a.tab + (size_t)k * a.W * nD + j;
        float S = 0.f; // a term that is left out adds +0: no bit changes, and the sum starts at the oldest valid term
        for (int32_t a0 = (int32_t)a.W - 1; a0 >= 0; a0 -= TRK_AGES) {
          float v[TRK_AGES];
#pragma unroll
          for (int t = 0; t < TRK_AGES; t++) {
            v[t] = 0.f;
            const int32_t age = a0 - t;
            if (age >= 0) {
              const int2 e = tk[(size_t)age * nD];
              const int32_t col = d + e.y;
              if (e.x >= 0 && col >= 0 && col < nDelay) {
                const uint32_t slot = slotG >= (uint32_t)age ? slotG - (uint32_t)age : slotG + R - (uint32_t)age;
                v[t] = a.ring[(size_t)slot * cells + (size_t)e.x * nDelay + col];
              }
            }
          }
#pragma unroll
          for (int t = 0; t < TRK_AGES; t++) S = __fadd_rn(S, v[t]);
        }
        if (k == 0) {
          best = S; // a NaN S_0 stays: no compare below is true against it
        } else if (S > best) {
          best = S;
          bk = k;
        }
      }
      z[i] = sqrtf(__fmul_rn(a.scale, best));
      kBest[i] = bk;
    }
  }
  // the stores, behind every table load; Map::set_metrics of the cells as written (a zero cell is -inf, as in nci_kernel)
  double lsum = 0.0;
  float lmax = 0.f;
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int32_t j = (int32_t)(group * TRK_ROWS) + wave * 2 + i;
    if (j < nD && d < nDelay) {
      const size_t at = (size_t)o * cells + (size_t)j * nDelay + d;
      a.out[at] = cmake(z[i], 0.f);
      if (a.index) a.index[at] = (uint8_t)kBest[i];
      const float db = db_of(cmake(z[i], 0.f));
      lsum += (double)db;
      lmax = fmaxf(lmax, db);
    }
  }
  const size_t part = (size_t)o * gridDim.x + blockIdx.x;
  block_metrics_partial(lsum, lmax, a.partSum + part, a.partMax + part);
}

} // namespace blah2
