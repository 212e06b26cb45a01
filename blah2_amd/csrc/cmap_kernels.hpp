// Clutter-map CFAR (Nitzberg) and the gate it puts behind the spatial detectors (gfx950 / MI355X only).
// No reference counterpart: blah2 thresholds a cell against its neighbours in one map, never against its own past.
// Included by detect.hip alone: this header defines kernels, so a second unit must not include it.
//
//   cmap_kernel        per cell and CPI, in time order: u = |M|^2 (times the CPI's level), exceeds <=> u > alpha[age] b, then
//                      b <- b + (u - b) / min(age + 1, T).  One launch per call, every map cell from HBM once.
//   hits_gate_kernel   keeps the records of a hit list whose cell exceeded, in their order.
//
// The definition is in include/blah2hip.h.  cmap_kernel has nci_kernel's shape (integrate_kernels.hpp): a thread OWNS two
// adjacent cells by cell index -- cells 2u and 2u + 1 of every map -- and walks the call's CPIs in order with b of both
// cells in registers; b comes from the handle's fp32 plane at the start (not at age 0: the first CPI overwrites it) and goes
// back once at the end.  The access width follows the plane: a map that starts on a 16-byte boundary is read 16 bytes per
// thread, one that starts 8 bytes off (every other map of an odd cell count) as two 8-byte halves, a wave-uniform choice
// per plane; an exceed plane on an even address takes both bytes of a thread in one store.  The walk goes in groups of
// CMAP_GROUP CPIs, all loads of a group in flight before its arithmetic.
//
// What is the same in every lane stays out of the vector unit's way: the age and so alpha[min(age, 16 T)] and 1 / k come
// from the launch arguments and a scalar load; the level s[c] needs an fp64 exp10, which lane l of every wave computes for
// CPI c0 + l once per 64 CPIs -- one pass through the routine for 64 CPIs -- and the walk reads it back with a lane read.
#pragma once

#include <hip/hip_runtime.h>

#include "blah2hip.h"
#include "fft_wg.hpp"

namespace blah2 {

constexpr int CMAP_GROUP = 8;    // CPIs whose loads are in flight together; divides 64 (a group never straddles a level refill)
constexpr int CMAP_AGES = 16;    // the table holds alpha[0 .. CMAP_AGES * T]; later ages read its last entry

struct CmapArgs {
  const cf *map;         // [nCpi][cells]
  const double *metrics; // [nCpi][2]
  const double *doppler; // [nD] Hz
  const double *alpha;   // [CMAP_AGES * memory + 1]
  float *bg;             // [cells]: b
  blah2hip_hit_t *hits;  // [nCpi][cap], or nullptr (then count is nullptr too)
  uint32_t *count;       // [nCpi]
  uint8_t *exceed;       // [nCpi][cells], or nullptr
  float *level;          // [nCpi], or nullptr
  uint32_t cells, nCpi;
  int32_t nDelay, delayMin, minDelay;
  double minDoppler;
  uint32_t cap;
  uint32_t age0;   // the map's age at the call's first CPI, clipped to CMAP_AGES * memory by the host (nothing looks further)
  uint32_t memory; // T
  uint32_t normalise;
};

typedef float cm_v2 __attribute__((ext_vector_type(2)));
typedef float cm_v4 __attribute__((ext_vector_type(4)));

// One cell of one CPI: the decision on b as it stands, then the update.  age, alpha and r are wave-uniform.
__device__ __forceinline__ bool cmap_cell(cm_v2 z, bool norm, float s, uint32_t age, double alpha, float r, float &b, float &p)
{
  p = fmaf(z[0], z[0], __fmul_rn(z[1], z[1]));
  const float u = norm ? __fmul_rn(p, s) : p;
  if (!(fabsf(u) < __builtin_inff())) return false; // NaN or Inf: neither exceeds nor updates
  const bool ex = age >= 1 && (double)u > alpha * (double)b;
  b = age == 0 ? u : fmaf(r, __fsub_rn(u, b), b);
  return ex;
}

// append_hit (cfar_kernels.hpp) for an fp32 power, the CPI's level loaded behind the cap test
__device__ __forceinline__ void cmap_hit(const CmapArgs &a, uint32_t c, int row, int col, float p)
{
  const uint32_t slot = atomicAdd(&a.count[c], 1u);
  if (slot < a.cap) {
    blah2hip_hit_t h;
    h.row = row;
    h.col = col;
    h.snr = 5.0 * log10((double)p) - a.metrics[2 * c];
    a.hits[(size_t)c * a.cap + slot] = h;
  }
}

// grid (G), 256 threads, G * 256 >= the map's units of two cells: one unit per thread
__global__ __launch_bounds__(256) void cmap_kernel(CmapArgs a)
{
  constexpr int P = CMAP_GROUP;
  const size_t cells = a.cells;
  const size_t nUnits = (cells + 1) / 2;
  const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool on = u < nUnits;
  const size_t i0 = 2 * u;
  const bool two = on && i0 + 1 < cells; // an odd cell count: the last unit is one cell
  const bool norm = a.normalise != 0;
  const int lane = threadIdx.x & 63;

  // the list's skips are the same in every CPI (blah2hip_cfar1d_dev's: |doppler[row]| < minDoppler, delay < minDelay)
  int row0 = 0, col0 = 0, row1 = 0, col1 = 0;
  bool rep0 = false, rep1 = false;
  if (a.hits && on) {
    row0 = (int)(i0 / (size_t)a.nDelay);
    col0 = (int)(i0 - (size_t)row0 * a.nDelay);
    rep0 = !(fabs(a.doppler[row0]) < a.minDoppler) && !(col0 + a.delayMin < a.minDelay);
    if (two) {
      row1 = col0 + 1 < a.nDelay ? row0 : row0 + 1;
      col1 = col0 + 1 < a.nDelay ? col0 + 1 : 0;
      rep1 = !(fabs(a.doppler[row1]) < a.minDoppler) && !(col1 + a.delayMin < a.minDelay);
    }
  }

  float b0 = 0.f, b1 = 0.f; // age 0: the plane is not read (a cell that is not finite then starts from 0)
  if (a.age0 != 0) {
    if (two) {
      const cm_v2 v = *reinterpret_cast<const cm_v2 *>(a.bg + i0);
      b0 = v[0];
      b1 = v[1];
    } else if (on) {
      b0 = a.bg[i0];
    }
  }

  const uint32_t last = CMAP_AGES * a.memory;
  const uint32_t cellBytes = a.cells * (uint32_t)sizeof(cf); // (mod 2^32)
  const cf *pin = a.map + i0;
  uint32_t inLow = (uint32_t)(uintptr_t)a.map; // the low address bits decide the alignment: 32 of them are plenty
  uint8_t *pex = a.exceed ? a.exceed + i0 : nullptr;
  uint32_t exLow = (uint32_t)(uintptr_t)a.exceed;
  float sv = 1.f; // lane l: the level of CPI (c0 & ~63) + l
  for (uint32_t c0 = 0; c0 < a.nCpi; c0 += P) {
    if ((c0 & 63) == 0) {
      const uint32_t cc = c0 + lane;
      if (norm) sv = cc < a.nCpi ? (float)exp10(-a.metrics[2 * cc] / 5.0) : 1.f;
      if (a.level && blockIdx.x == 0 && threadIdx.x < 64 && cc < a.nCpi) a.level[cc] = sv;
    }
    const uint32_t n = a.nCpi - c0 < (uint32_t)P ? a.nCpi - c0 : (uint32_t)P;
    cm_v2 lo[P], hi[P];
#pragma unroll
    for (int t = 0; t < P; t++) {
      lo[t] = cm_v2{0.f, 0.f};
      hi[t] = cm_v2{0.f, 0.f};
      if ((uint32_t)t < n) {
        const cf *cell = pin + t * cells;
        if (!((inLow + (uint32_t)t * cellBytes) & 15) && two) {
          const cm_v4 v = __builtin_nontemporal_load(reinterpret_cast<const cm_v4 *>(cell));
          lo[t] = cm_v2{v[0], v[1]};
          hi[t] = cm_v2{v[2], v[3]};
        } else {
          if (on) lo[t] = __builtin_nontemporal_load(reinterpret_cast<const cm_v2 *>(cell));
          if (two) hi[t] = __builtin_nontemporal_load(reinterpret_cast<const cm_v2 *>(cell + 1));
        }
      }
    }
#pragma unroll
    for (int t = 0; t < P; t++) {
      if ((uint32_t)t < n) {
        const uint32_t c = c0 + t;
        const uint32_t age = a.age0 + c; // age0 <= 16 T and c < max_batch: no overflow
        const double alpha = a.alpha[age < last ? age : last];
        const uint32_t k = age + 1 < a.memory ? age + 1 : a.memory;
        const float r = __fdiv_rn(1.f, (float)k);
        const float s = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sv), (int)(c & 63)));
        float p0 = 0.f, p1 = 0.f;
        const bool e0 = on && cmap_cell(lo[t], norm, s, age, alpha, r, b0, p0);
        const bool e1 = two && cmap_cell(hi[t], norm, s, age, alpha, r, b1, p1);
        if (e0 && rep0) cmap_hit(a, c, row0, col0, p0);
        if (e1 && rep1) cmap_hit(a, c, row1, col1, p1);
        if (pex) {
          if (!(exLow & 1) && two) {
            *reinterpret_cast<uint16_t *>(pex) = (uint16_t)((e0 ? 1u : 0u) | (e1 ? 0x100u : 0u));
          } else {
            if (on) pex[0] = e0 ? 1 : 0;
            if (two) pex[1] = e1 ? 1 : 0;
          }
          pex += cells;
          exLow += a.cells;
        }
      }
    }
    pin += (size_t)n * cells;
    inLow += n * cellBytes;
  }

  if (two) *reinterpret_cast<cm_v2 *>(a.bg + i0) = cm_v2{b0, b1};
  else if (on) a.bg[i0] = b0;
}

struct GateArgs {
  const uint8_t *exceed;      // [nCpi][nD][nDelay]
  const blah2hip_hit_t *hits; // [nCpi][cap]
  const uint32_t *count;      // [nCpi]; more than cap: the first cap records are the list
  blah2hip_hit_t *out;        // [nCpi][cap]
  uint32_t *countOut;         // [nCpi]
  int32_t nD, nDelay;
  uint32_t cap;
};

// grid (nCpi), 256 threads.  The list goes by in chunks of 256 records, one per thread: a wave's survivors are counted with a
// ballot, a thread's place among them is the ballot's bits below its lane, and the waves' totals go through LDS (two sets in
// turn: one barrier per chunk) -- so record i of the output is the i-th survivor of the input.  A record outside the map is
// dropped.  The output holds at most as many records as the input: it never passes cap.
__global__ __launch_bounds__(256) void hits_gate_kernel(GateArgs a)
{
  __shared__ uint32_t wtot[2][4];
  const int cpi = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t n = min(a.count[cpi], a.cap);
  const blah2hip_hit_t *hits = a.hits + (size_t)cpi * a.cap;
  blah2hip_hit_t *out = a.out + (size_t)cpi * a.cap;
  const uint8_t *ex = a.exceed + (size_t)cpi * a.nD * a.nDelay;
  uint32_t kept = 0;
  int set = 0;
  for (uint32_t i0 = 0; i0 < n; i0 += 256, set ^= 1) {
    const uint32_t i = i0 + t;
    blah2hip_hit_t h;
    h.row = -1;
    h.col = -1;
    h.snr = 0.0;
    bool keep = false;
    if (i < n) {
      h = hits[i];
      keep = h.row >= 0 && h.row < a.nD && h.col >= 0 && h.col < a.nDelay && ex[(size_t)h.row * a.nDelay + h.col] != 0;
    }
    const unsigned long long m = __ballot(keep);
    const uint32_t before = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[set][wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t at = kept, total = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      at += w < wave ? wtot[set][w] : 0u;
      total += wtot[set][w];
    }
    if (keep) out[at + before] = h;
    kept += total;
  }
  if (t == 0) a.countOut[cpi] = kept;
}

} // namespace blah2
