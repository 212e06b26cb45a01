// The end of a CPI's detection list on the device (gfx950 / MI355X only).
// Included by detect.hip alone: this header defines kernels, so a second unit must not include it.
//
//   detect_finish_kernel           Centroid::process, then Interpolate::process     Centroid.cpp:19-73, Interpolate.cpp:20-91
//
// blah2.cpp:285-287 runs CfarDetector1D -> Centroid -> Interpolate per CPI.  The detector kernels leave a list of
// blah2hip_hit_t per CPI on the device; this kernel turns it into the final list next to the map it came from, so neither
// the hits nor the map cross the host link.  It restates the host functions blah2hip_centroid / blah2hip_interpolate
// (detect.hip), which restate the reference, quirk by quirk.
//
// All paths are relative to the reference's src/.
#pragma once

#include <hip/hip_runtime.h>

#include "blah2hip.h"
#include "fft_wg.hpp"

namespace blah2 {

constexpr int DET_BLOCK = 256;  // threads of a workgroup = hits of a block (one thread per hit i)
constexpr int DET_TILE = 1024;  // hits j staged in LDS at a time, 24 bytes each

struct DetectArgs {
  const cf *map;              // [nCpi][nD][nDelay]
  const double *metrics;      // [nCpi][2]
  const double *doppler;      // [nD] Hz, the handle's axis
  const blah2hip_hit_t *hits; // [nCpi][cap], arbitrary order
  const uint32_t *count;      // [nCpi]; more than cap: the first cap records are the list
  blah2hip_det_t *out;        // [nCpi][capOut]
  uint32_t *countOut;         // [nCpi]
  uint32_t *appended;         // [nCpi] tiled form: records appended so far; zero between launches
  uint32_t *tickets;          // [nCpi] tiled form: workgroups of the CPI that are done; zero between launches
  int32_t nD, nDelay, delayMin;
  int32_t nCentroidDelay;
  double boxDoppler;          // nDoppler * resolutionDoppler, rounded once on the host like Centroid.cpp:38-39 does
  uint32_t cap, capOut;
  int32_t doCentroid, doDelay, doDoppler;
};

struct DetTileEntry { double delay, doppler, snr; };

// 10*log10|z| - noisePower of one map cell in fp64 (Interpolate.cpp:50-52)
__device__ __forceinline__ double det_cell(const cf *row, int col, double noisePower)
{
  const cf z = row[col];
  return 10.0 * log10(hypot((double)z.x, (double)z.y)) - noisePower;
}

// One thread per hit i.  A CPI's hits are dealt in blocks of DET_BLOCK to the workgroups of its grid row (blockIdx.x of
// gridDim.x, grid-stride); a workgroup beyond the last block of the CPI's list leaves at once.
//
// Centroid: hit i is dropped when some j lies strictly inside its box with a strictly larger snr (equal snr: both stay).
// The list goes through LDS in tiles of DET_TILE entries (delay, doppler, snr); all lanes read the same entry (a broadcast),
// a wave skips the rest of the list once every lane of it is decided and the workgroup leaves the tile loop when all its
// waves are.  The box is the host's: uint16_t delay limits that wrap below zero, fp64 Doppler limits whose product was
// rounded before the sum (no fused multiply-add: a hit exactly nDoppler rows away sits on the box's edge, and the edge is
// decided by that rounding).
//
// Interpolate on the survivors, the delay branch first; the Doppler branch stores its estimate into the delay branch's
// variable like the reference does (:80).  Records outside the map (a list the caller built) are ignored altogether.
//
// TILED = false: one workgroup per CPI (gridDim.x == 1), the append counter lives in LDS and nothing but the result touches
// global memory.  TILED = true: the CPI's workgroups append through appended[cpi]; the last one to take a ticket copies
// the total to countOut[cpi] and zeroes both words for the next launch -- no memset in front of the kernel.
template <bool TILED>
__global__ __launch_bounds__(DET_BLOCK) void detect_finish_kernel(DetectArgs a)
{
#pragma clang fp contract(off) // the host functions round every product; so does this kernel
  __shared__ DetTileEntry tile[DET_TILE];
  __shared__ uint32_t ldsCount;
  const int cpi = blockIdx.y, t = threadIdx.x;
  const uint32_t n = min(a.count[cpi], a.cap);
  const uint32_t blocks = (n + DET_BLOCK - 1) / DET_BLOCK;
  // the workgroups that have a block of this list (at least one, so that an empty list still gets its count written)
  const uint32_t workers = max(1u, min(blocks, (uint32_t)gridDim.x));
  if (blockIdx.x >= workers) return;
  const blah2hip_hit_t *hits = a.hits + (size_t)cpi * a.cap;
  const cf *map = a.map + (size_t)cpi * a.nD * a.nDelay;
  const double noisePower = a.metrics[2 * cpi];
  blah2hip_det_t *out = a.out + (size_t)cpi * a.capOut;
  if (!TILED) {
    if (t == 0) ldsCount = 0;
    __syncthreads();
  }

  for (uint32_t b = blockIdx.x; b < blocks; b += workers) {
    const uint32_t i = b * DET_BLOCK + t;
    blah2hip_hit_t me;
    me.row = -1; me.col = -1; me.snr = 0.0;
    if (i < n) me = hits[i];
    const bool valid = i < n && (uint32_t)me.row < (uint32_t)a.nD && (uint32_t)me.col < (uint32_t)a.nDelay;
    const double delay = (double)(me.col + a.delayMin);       // CfarDetector1D.cpp:88
    const double doppler = valid ? a.doppler[me.row] : 0.0;   // :89
    bool keep = valid;

    if (a.doCentroid) {
      // Centroid.cpp:36-39
      const double lo = (double)(uint16_t)((int)delay - a.nCentroidDelay);
      const double hi = (double)(uint16_t)((int)delay + a.nCentroidDelay);
      const double flo = __dsub_rn(doppler, a.boxDoppler);
      const double fhi = __dadd_rn(doppler, a.boxDoppler);
      for (uint32_t j0 = 0; j0 < n; j0 += DET_TILE) {
        // (also the barrier behind the previous tile's readers)
        if (!__syncthreads_or(keep)) break;
        const uint32_t tn = min((uint32_t)DET_TILE, n - j0);
        for (uint32_t e = t; e < tn; e += DET_BLOCK) {
          const blah2hip_hit_t h = hits[j0 + e];
          DetTileEntry w;
          if ((uint32_t)h.row < (uint32_t)a.nD && (uint32_t)h.col < (uint32_t)a.nDelay) {
            w.delay = (double)(h.col + a.delayMin);
            w.doppler = a.doppler[h.row];
            w.snr = h.snr;
          } else { // never inside a box: NaN compares false
            w.delay = w.doppler = w.snr = __builtin_nan("");
          }
          tile[e] = w;
        }
        __syncthreads();
        for (uint32_t e0 = 0; e0 < tn; e0 += 8) {
          if (!__any(keep)) break; // this wave is decided
          const uint32_t e1 = min(e0 + 8, tn);
          for (uint32_t e = e0; e < e1; e++) {
            const DetTileEntry w = tile[e];
            // Centroid.cpp:51-56 (j == i never drops i: snr[i] < snr[i] is false)
            if (w.delay > lo && w.delay < hi && w.doppler > flo && w.doppler < fhi && me.snr < w.snr) keep = false;
          }
        }
      }
    }

    // Interpolate.cpp:38-86
    double intDelay = delay, intDoppler = doppler, intSnrDelay = me.snr;
    const double intSnrDoppler = me.snr; // never updated in the reference
    if (keep && a.doDelay) {
      if (me.col == 0 || me.col == a.nDelay - 1) { // :46-49 the first or last delay bin
        keep = false;
      } else {
        const cf *row = map + (size_t)me.row * a.nDelay;
        const double s0 = det_cell(row, me.col - 1, noisePower), s1 = det_cell(row, me.col, noisePower),
                     s2 = det_cell(row, me.col + 1, noisePower);
        if (s1 < s0 || s1 < s2) { // :54-58 the peak is lower than a neighbour
          keep = false;
        } else {
          const double off = (s0 - s2) / (2 * (s0 - (2 * s1) + s2));
          intSnrDelay = s1 - (((s0 - s2) * off) / 4);
          intDelay = delay + off;
        }
      }
    }
    if (keep && a.doDoppler) {
      if (me.row == 0 || me.row == a.nD - 1) { // :67-70 the first or last Doppler bin
        keep = false;
      } else {
        const cf *col = map + (size_t)me.row * a.nDelay + me.col;
        const double s0 = det_cell(col, -a.nDelay, noisePower), s1 = det_cell(col, 0, noisePower), s2 = det_cell(col, a.nDelay, noisePower);
        if (s1 < s0 || s1 < s2) {
          keep = false;
        } else {
          const double off = (s0 - s2) / (2 * (s0 - (2 * s1) + s2));
          intSnrDelay = s1 - (((s0 - s2) * off) / 4); // sic, :80
          intDoppler = doppler + ((a.doppler[1] - a.doppler[0]) * off);
        }
      }
    }

    // append: one atomic per wave, the lanes' slots follow from the ballot
    const uint64_t mask = __ballot(keep);
    if (mask) {
      const uint32_t lanesBefore = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
      uint32_t base = 0;
      if (lanesBefore == 0 && keep) { // the wave's first surviving lane
        const uint32_t k = (uint32_t)__popcll(mask);
        base = TILED ? __hip_atomic_fetch_add(a.appended + cpi, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                     : atomicAdd(&ldsCount, k);
      }
      base = __shfl(base, __ffsll((unsigned long long)mask) - 1);
      const uint32_t slot = base + lanesBefore;
      if (keep && slot < a.capOut) {
        blah2hip_det_t d;
        d.row = me.row;
        d.col = me.col;
        d.delay = intDelay;
        d.doppler = intDoppler;
        // :86 std::max(std::max(intSnrDelay, intSnrDoppler), snr): a NaN first argument stays
        const double m = intSnrDelay < intSnrDoppler ? intSnrDoppler : intSnrDelay;
        d.snr = m < me.snr ? me.snr : m;
        out[slot] = d;
      }
    }
  }

  // every atomic above has returned its value to its wave before that wave arrives here
  __syncthreads();
  if (t == 0) {
    if (!TILED) {
      a.countOut[cpi] = ldsCount;
    } else {
      const uint32_t tk = __hip_atomic_fetch_add(a.tickets + cpi, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (tk == workers - 1) { // the CPI's last workgroup: the total, and both words back to zero for the next launch
        a.countOut[cpi] = __hip_atomic_exchange(a.appended + cpi, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.tickets + cpi, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

} // namespace blah2
