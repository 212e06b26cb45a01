// A receiver array behind the Doppler stage (gfx950 / MI355X only).  No reference counterpart: blah2 has one
// surveillance channel.
//
//   beamform_kernel    M_b = sum_k w[b][k] M_k for every beam b in ONE pass over the K channel maps, with the
//                      per-workgroup partials of Map::set_metrics (Map.cpp:187-206) of every beam map
//   snapshot_kernel    the K channel cells under every detection of a list (what a bearing is computed from)
//
// The cross-ambiguity map is linear in the surveillance channel, so the map of the beam y_b = sum_k w[b][k] y_k is the
// same combination of the channel maps blah2hip_amb_process_multi_dev left in HBM: a further beam costs one more map
// written, not a range + Doppler chain.
#pragma once

#include <hip/hip_runtime.h>

#include "blah2hip.h"
#include "kernels.hpp"

namespace blah2 {

struct BeamArgs {
  const cf *in;    // [K][nCpi][cells]
  cf *out;         // [nBeams][nCpi][cells]
  double *partSum; // [nBeams * nCpi][gridDim.x]: metrics_kernel's layout over the virtual CPIs b * nCpi + c
  float *partMax;
  uint32_t cells, nCpi, nBeams;
  cf w[BLAH2HIP_MAX_BEAMS][BLAH2HIP_MAX_SURV]; // in the launch arguments: wave-uniform, read by scalar loads
};

template <int V> struct BeamVec;
template <> struct BeamVec<1> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct BeamVec<2> { typedef float type __attribute__((ext_vector_type(4))); };

// V adjacent cells from cell i of the CPI on: the K loads first (all in flight together), then beam after beam.  The
// beam loop is unrolled to its limit behind a wave-uniform test so that weights and partials are statically indexed.
// Per component the sum is a chain of fused multiply-adds in the order k = 0 .. K-1: 2K roundings, each at most 2^-24
// of sum_k |w_k| |M_k|; a weight of exactly 1 or 0 passes a cell through bit for bit.
template <int K, int V>
__device__ __forceinline__ void beam_cells(const BeamArgs &a, const cf *in, cf *out, size_t chStride, size_t i,
                                           double (&lsum)[BLAH2HIP_MAX_BEAMS], float (&lmax)[BLAH2HIP_MAX_BEAMS])
{
  typedef typename BeamVec<V>::type vec;
  vec m[K];
#pragma unroll
  for (int k = 0; k < K; k++) m[k] = *reinterpret_cast<const vec *>(in + k * chStride + i);
#pragma unroll
  for (int b = 0; b < BLAH2HIP_MAX_BEAMS; b++) {
    if (b < (int)a.nBeams) {
      vec r;
#pragma unroll
      for (int v = 0; v < V; v++) {
        float re = 0.f, im = 0.f;
#pragma unroll
        for (int k = 0; k < K; k++) {
          const cf w = a.w[b][k];
          const float mx = m[k][2 * v], my = m[k][2 * v + 1];
          re = fmaf(-w.y, my, k ? fmaf(w.x, mx, re) : w.x * mx);
          im = fmaf(w.y, mx, k ? fmaf(w.x, my, im) : w.x * my);
        }
        r[2 * v] = re;
        r[2 * v + 1] = im;
        const float db = db_of(cmake(re, im)); // a zero cell is -inf here, as in the Doppler kernels' epilogues
        lsum[b] += (double)db;
        lmax[b] = fmaxf(lmax[b], db);
      }
      *reinterpret_cast<vec *>(out + b * chStride + i) = r;
    }
  }
}

// grid (G, nCpi), 256 threads.  A workgroup strides over its CPI in units of V cells; V = 2 (16-byte accesses) needs
// every channel's and every beam's copy of a CPI to start at the same offset modulo 16 bytes (the host checks it): a CPI
// that starts 8 bytes off -- every odd one of a map with an odd cell count -- then has a one-cell head, and whatever is
// left behind the last pair is a one-cell tail; both go through 8-byte accesses in workgroup 0.  V = 1 otherwise.
template <int K, int V>
__global__ __launch_bounds__(256) void beamform_kernel(BeamArgs a)
{
  const uint32_t cpi = blockIdx.y;
  const size_t cells = a.cells;
  const cf *in = a.in + cpi * cells;
  cf *out = a.out + cpi * cells;
  const size_t chStride = (size_t)a.nCpi * cells; // a channel's (and a beam's) block of nCpi maps
  double lsum[BLAH2HIP_MAX_BEAMS];
  float lmax[BLAH2HIP_MAX_BEAMS];
#pragma unroll
  for (int b = 0; b < BLAH2HIP_MAX_BEAMS; b++) { lsum[b] = 0.0; lmax[b] = 0.f; }

  const size_t head = V == 2 ? (size_t)(((uintptr_t)in >> 3) & 1) : 0;
  const size_t nUnits = (cells - head) / V;
  for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < nUnits; u += (size_t)gridDim.x * 256)
    beam_cells<K, V>(a, in, out, chStride, head + u * V, lsum, lmax);
  if (V == 2 && blockIdx.x == 0) {
    const size_t nLeft = head + ((cells - head) & 1);
    if (threadIdx.x < nLeft) beam_cells<K, 1>(a, in, out, chStride, (threadIdx.x == 0 && head) ? 0 : cells - 1, lsum, lmax);
  }

  // one (sum, max) partial per workgroup and beam; metrics_kernel folds them in index order
#pragma unroll
  for (int b = 0; b < BLAH2HIP_MAX_BEAMS; b++) {
    if (b < (int)a.nBeams) {
      if (b) __syncthreads(); // thread 0 has read the previous beam's wave partials
      const size_t part = ((size_t)b * a.nCpi + cpi) * gridDim.x + blockIdx.x;
      block_metrics_partial(lsum[b], lmax[b], a.partSum + part, a.partMax + part);
    }
  }
}

// beamform_kernel<K, V> for the call's channel count, 16-byte (V = 2) or 8-byte (V = 1) accesses
template <int V> inline void launch_beamform(uint32_t K, dim3 grid, hipStream_t st, const BeamArgs &a)
{
  switch (K) {
  case 1: hipLaunchKernelGGL((beamform_kernel<1, V>), grid, dim3(256), 0, st, a); break;
  case 2: hipLaunchKernelGGL((beamform_kernel<2, V>), grid, dim3(256), 0, st, a); break;
  case 3: hipLaunchKernelGGL((beamform_kernel<3, V>), grid, dim3(256), 0, st, a); break;
  case 4: hipLaunchKernelGGL((beamform_kernel<4, V>), grid, dim3(256), 0, st, a); break;
  case 5: hipLaunchKernelGGL((beamform_kernel<5, V>), grid, dim3(256), 0, st, a); break;
  case 6: hipLaunchKernelGGL((beamform_kernel<6, V>), grid, dim3(256), 0, st, a); break;
  case 7: hipLaunchKernelGGL((beamform_kernel<7, V>), grid, dim3(256), 0, st, a); break;
  default: hipLaunchKernelGGL((beamform_kernel<8, V>), grid, dim3(256), 0, st, a); break;
  }
}

struct SnapArgs {
  const cf *map;              // [nSurv][nCpi][nD][nDelay]
  const blah2hip_det_t *dets; // [nLists][cap]
  const uint32_t *count;      // [nLists]; more than cap: the first cap records are the list
  cf *snap;                   // [nLists][cap][nSurv]
  uint32_t nSurv, nCpi, cap, nLists;
  int32_t nD, nDelay;
};

// One thread per record slot (list l, index i).  Slots behind the list's count and records outside the map are left
// unwritten.
__global__ __launch_bounds__(256) void snapshot_kernel(SnapArgs a)
{
  const size_t total = (size_t)a.nLists * a.cap;
  const size_t cells = (size_t)a.nD * a.nDelay;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
    const uint32_t l = (uint32_t)(t / a.cap), i = (uint32_t)(t % a.cap);
    if (i >= a.count[l]) continue;
    const int32_t row = a.dets[t].row, col = a.dets[t].col;
    if (row < 0 || row >= a.nD || col < 0 || col >= a.nDelay) continue;
    const cf *z = a.map + (l % a.nCpi) * cells + (size_t)row * a.nDelay + col;
    for (uint32_t k = 0; k < a.nSurv; k++) a.snap[t * a.nSurv + k] = z[(size_t)k * a.nCpi * cells];
  }
}

} // namespace blah2
