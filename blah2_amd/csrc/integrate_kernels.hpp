// Non-coherent integration of delay-Doppler maps over surveillance channels and consecutive CPIs (gfx950 / MI355X only).
// No reference counterpart: blah2 detects on single maps.
// Included by integrate.hip alone: this header defines kernels, so a second unit must not include it.
//
//   nci_kernel<W>   p[g] = sum_k w_k |M_k[g]|^2 per cell, out[g] = (sqrt(scale (p[g-W+1] + ... + p[g])), 0) for the CPIs g
//                   at which a window of W ends, with the per-workgroup partials of Map::set_metrics (Map.cpp:187-206)
//                   of every output map.  One pass over the call's maps: every input cell comes from HBM once,
//                   whatever W and the hop are.
//
// A thread OWNS two adjacent cells (cells 2u and 2u + 1 of every map, u its unit) and walks the call's CPIs in order with
// the last values of p of both cells in a ring of registers.  The walk is unrolled by the ring length R (nci_ring: W - 1
// older CPIs and a group of new ones), so the slot of CPI c, c mod R, is a constant in every copy of the body and the ring
// stays in registers (an array indexed at run time would go to scratch): cfar2d_stream_kernel's row ring, along the CPI axis.  No running sum: every window is added up on its
// own, oldest CPI first, so a NaN or Inf cell touches the windows that hold it and nothing else.
//
// The W - 1 values in front of a call's first CPI come from the integrator's history planes (fp32, written by the call
// before with the very values it summed: a p taken from there is bit-equal to one computed inside a call), and the last
// W - 1 values of the call go back there -- stored while the walk passes them, or moved up from the old planes when the call
// is shorter than the history.
//
// Ownership is by CELL INDEX, not by address: CPI after CPI a thread needs the same cells, and with an odd cell count
// consecutive maps alternate between 16-byte aligned and 8 bytes off, so no pairing is aligned in all of them
// (beamform_kernel's one-cell head works there because its CPIs are independent).  The access width follows the plane
// instead: a plane (one channel's map of one CPI, one output map) that starts on a 16-byte boundary is read or written 16
// bytes per thread, one that starts 8 bytes off as two 8-byte halves of the same 16 bytes -- a wave-uniform choice per
// plane.  The same mapping in every call is also what makes the metrics independent of how the CPIs were cut into calls:
// the partial of (output map, workgroup) is the same sum over the same cells in the same order.
#pragma once

#include <hip/hip_runtime.h>

#include "blah2hip.h"
#include "metrics_core.hpp"

namespace blah2 {

constexpr int NCI_MAX_WINDOW = 16;

struct NciArgs {
  const cf *in;    // [K][nCpi][cells]
  cf *out;         // [nOut][cells]
  float *hist;     // [W - 1][cells]: plane i - 1 holds p of the CPI W - i in front of the call's first one, i = 1 .. W - 1
  double *partSum; // [nOut][gridDim.x]: metrics_kernel's layout
  float *partMax;
  float w[BLAH2HIP_MAX_SURV]; // in the launch arguments: wave-uniform, read by scalar loads
  float scale;     // 1 / (W sum_k w_k), rounded to fp32 on the host
  uint32_t cells, nCpi, K;
  uint32_t firstOut;  // index in the call of the first CPI at which a window ends (>= nCpi: none)
  uint32_t hop;       // CPIs from one window's end to the next (clipped to nCpi by the host: no overflow)
  uint32_t histValid; // history planes that hold a CPI: min(CPIs since the reset, W - 1), the planes W - histValid .. W - 1
};

typedef float nci_v2 __attribute__((ext_vector_type(2)));
typedef float nci_v4 __attribute__((ext_vector_type(4)));

// The walk goes in groups of NCI_GROUP CPIs: first p of the group's CPIs -- the loads of one channel for all of them in
// flight together, then the arithmetic -- then the windows that end inside the group, their stores and ONE barrier for
// their metrics.  A map has few threads for this chip (one per two cells: 1.6 waves a SIMD at 513 x 411), so what a thread
// keeps in flight decides the rate.  The ring has room for the group on top of the W - 1 older CPIs its windows reach
// back to, rounded up to whole groups so that the unrolled walk keeps every slot a constant.
constexpr int NCI_GROUP = 4;
constexpr int nci_ring(int W) { return (W - 1 + NCI_GROUP + NCI_GROUP - 1) / NCI_GROUP * NCI_GROUP; }

// p of the thread's two cells for the n <= NCI_GROUP CPIs from `pin` on: `pin` points at the thread's first cell in
// channel 0's map of the first of them, which starts at the address `base`; the CPIs are `cells` cells apart, the channels
// chStride.  Input cells are used once: streaming loads.  |M|^2 = fma(re, re, im im), then p = fma(w_k, |M_k|^2, p) from
// 0 in the order k = 0 .. K - 1: K + 2 roundings per cell, every term non-negative.  CPIs behind the n-th give 0.
__device__ __forceinline__ void nci_power(const NciArgs &a, const cf *pin, uintptr_t base, size_t cells, size_t chStride, uint32_t n,
                                          bool on, bool two, float (&p0)[NCI_GROUP], float (&p1)[NCI_GROUP])
{
#pragma unroll
  for (int t = 0; t < NCI_GROUP; t++) { p0[t] = 0.f; p1[t] = 0.f; }
  for (uint32_t k = 0; k < a.K; k++) {
    nci_v2 lo[NCI_GROUP], hi[NCI_GROUP];
#pragma unroll
    for (int t = 0; t < NCI_GROUP; t++) {
      lo[t] = nci_v2{0.f, 0.f};
      hi[t] = nci_v2{0.f, 0.f};
      if ((uint32_t)t < n) {
        const cf *cell = pin + t * cells;
        if (!((base + t * cells * sizeof(cf)) & 15) && two) {
          const nci_v4 v = __builtin_nontemporal_load(reinterpret_cast<const nci_v4 *>(cell));
          lo[t] = nci_v2{v[0], v[1]};
          hi[t] = nci_v2{v[2], v[3]};
        } else {
          if (on) lo[t] = __builtin_nontemporal_load(reinterpret_cast<const nci_v2 *>(cell));
          if (two) hi[t] = __builtin_nontemporal_load(reinterpret_cast<const nci_v2 *>(cell + 1));
        }
      }
    }
    const float wk = a.w[k];
#pragma unroll
    for (int t = 0; t < NCI_GROUP; t++) {
      p0[t] = fmaf(wk, fmaf(lo[t][0], lo[t][0], __fmul_rn(lo[t][1], lo[t][1])), p0[t]);
      p1[t] = fmaf(wk, fmaf(hi[t][0], hi[t][0], __fmul_rn(hi[t][1], hi[t][1])), p1[t]);
    }
    pin += chStride;
    base += chStride * sizeof(cf);
  }
}

// grid (G), 256 threads, G * 256 >= the map's units: one unit per thread (blah2hip_nci_create has made sure that the handle
// holds a partial per workgroup and map).  Every branch around a barrier is uniform over the workgroup.
template <int W>
__global__ __launch_bounds__(256) void nci_kernel(NciArgs a)
{
  constexpr int R = nci_ring(W), P = NCI_GROUP;
  // the waves' (sum, max) of a group's windows, two sets in turn: a set is written again two barriers after thread t read it
  __shared__ double wsum[2][P][4];
  __shared__ float wmax[2][P][4];
  const size_t cells = a.cells;
  const size_t nUnits = (cells + 1) / 2;
  const size_t chStride = (size_t)a.nCpi * cells;
  const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool on = u < nUnits;
  const size_t i0 = 2 * u;
  const bool two = on && i0 + 1 < cells; // an odd cell count: the last unit is one cell
  const int wave = threadIdx.x >> 6;
  float r0[R], r1[R]; // slot c mod R: p of the call's CPI c
  const uint32_t histValid = a.histValid, stay = (uint32_t)W > a.nCpi ? (uint32_t)W - a.nCpi : 0; // planes stay .. W - 1 move up

  // history plane i: the CPI W - i in front of this call, c = i - W, slot R - W + i.  A call shorter than the history: the
  // planes that stay in it move up by nCpi (every thread moves its own cells, and reads a plane before it writes it: plane
  // i - nCpi is read, if at all, in an earlier turn than plane i).
#pragma unroll
  for (int i = 0; i < R; i++) { r0[i] = 0.f; r1[i] = 0.f; }
  {
    const float *hp = a.hist + i0;
    float *hq = a.hist + i0; // where plane W - stay + 1, the first that stays, moves: plane 1
#pragma unroll
    for (int i = 1; i < W; i++) {
      if ((uint32_t)(W - i) <= histValid) {
        if (on) r0[R - W + i] = hp[0];
        if (two) r1[R - W + i] = hp[1];
        if ((uint32_t)(W - i) < stay) {
          if (on) hq[0] = r0[R - W + i];
          if (two) hq[1] = r1[R - W + i];
        }
      }
      if ((uint32_t)(W - i) < stay) hq += cells;
      hp += cells;
    }
  }

  // Loop-carried pointers, a map further per CPI (the thread's own cells; the planes' alignment is tested on the
  // uniform base addresses): derived from c they are R sets of constants in scalar registers, which then spill
  const cf *pin = a.in + i0;
  cf *pout = a.out + i0;
  float *hst = a.hist + (size_t)(W - 1 > (int)a.nCpi ? W - 1 - a.nCpi : 0) * cells + i0; // the plane of the first CPI that stays
  uintptr_t inBase = (uintptr_t)a.in, outBase = (uintptr_t)a.out;
  uint32_t o = 0, next = a.firstOut, set = 0;
  for (uint32_t base = 0; base < a.nCpi; base += R) {
#pragma unroll
    for (int s = 0; s < R; s += P) {
      const uint32_t c0 = base + s;
      if (c0 < a.nCpi) {
        const uint32_t n = a.nCpi - c0 < (uint32_t)P ? a.nCpi - c0 : (uint32_t)P;
        float p0[P], p1[P];
        nci_power(a, pin, inBase, cells, chStride, n, on, two, p0, p1);
        pin += n * cells;
        inBase += n * cells * sizeof(cf);
        uint32_t outAt[P]; // the output map of the window that ends at CPI c0 + t, or none
        double lsum[P];
        float lmax[P];
        bool any = false;
#pragma unroll
        for (int t = 0; t < P; t++) {
          const uint32_t c = c0 + t;
          outAt[t] = ~0u;
          if ((uint32_t)t < n) {
            r0[s + t] = p0[t];
            r1[s + t] = p1[t];
            // one of the call's last W - 1 CPIs: into the history, plane c + W - nCpi
            if (W > 1 && c + W > a.nCpi) {
              if (on) hst[0] = p0[t];
              if (two) hst[1] = p1[t];
              hst += cells;
            }
            if (c == next) {
              // the window that ends here: slots s + t - W + 1 .. s + t (mod R), oldest first
              float s0 = r0[(s + t + R - W + 1) % R], s1 = r1[(s + t + R - W + 1) % R];
#pragma unroll
              for (int q = W - 2; q >= 0; q--) {
                s0 = __fadd_rn(s0, r0[(s + t + R - q) % R]);
                s1 = __fadd_rn(s1, r1[(s + t + R - q) % R]);
              }
              const float z0 = sqrtf(__fmul_rn(a.scale, s0)), z1 = sqrtf(__fmul_rn(a.scale, s1));
              if (!(outBase & 15) && two) {
                *reinterpret_cast<nci_v4 *>(pout) = nci_v4{z0, 0.f, z1, 0.f};
              } else {
                if (on) *reinterpret_cast<nci_v2 *>(pout) = nci_v2{z0, 0.f};
                if (two) *reinterpret_cast<nci_v2 *>(pout + 1) = nci_v2{z1, 0.f};
              }
              pout += cells;
              outBase += cells * sizeof(cf);
              // Map::set_metrics of the cells as written; a zero cell is -inf, as in the Doppler kernels' epilogues
              lsum[t] = 0.0;
              lmax[t] = 0.f;
              if (on) {
                const float db = db_of(cmake(z0, 0.f));
                lsum[t] = (double)db;
                lmax[t] = fmaxf(lmax[t], db);
              }
              if (two) {
                const float db = db_of(cmake(z1, 0.f));
                lsum[t] += (double)db;
                lmax[t] = fmaxf(lmax[t], db);
              }
              wave_sum_max(lsum[t], lmax[t]);
              if ((threadIdx.x & 63) == 0) { wsum[set][t][wave] = lsum[t]; wmax[set][t][wave] = lmax[t]; }
              outAt[t] = o++;
              next += a.hop;
              any = true;
            }
          }
        }
        // one (sum, max) partial per workgroup and map, block_metrics_partial's fold (metrics_core.hpp) for the group's
        // windows behind one barrier, window t by thread t; metrics_kernel folds the partials in index order
        if (any) {
          __syncthreads();
#pragma unroll
          for (int t = 0; t < P; t++) {
            if (outAt[t] != ~0u && threadIdx.x == t) {
              double sum = 0.0;
              float m = 0.f; // Map.cpp:193: the running max starts at 0
              for (int w = 0; w < 4; w++) { sum += wsum[set][t][w]; m = fmaxf(m, wmax[set][t][w]); }
              const size_t part = (size_t)outAt[t] * gridDim.x + blockIdx.x;
              a.partSum[part] = sum;
              a.partMax[part] = m;
            }
          }
          set ^= 1;
        }
      }
    }
  }
}

// nci_kernel<W> for the integrator's window
inline void launch_nci(uint32_t W, dim3 grid, hipStream_t st, const NciArgs &a)
{
  switch (W) {
#define B2_NCI(N) case N: hipLaunchKernelGGL(nci_kernel<N>, grid, dim3(256), 0, st, a); break;
  B2_NCI(1) B2_NCI(2) B2_NCI(3) B2_NCI(4) B2_NCI(5) B2_NCI(6) B2_NCI(7) B2_NCI(8)
  B2_NCI(9) B2_NCI(10) B2_NCI(11) B2_NCI(12) B2_NCI(13) B2_NCI(14) B2_NCI(15) B2_NCI(16)
#undef B2_NCI
  }
}

} // namespace blah2
