// Doppler-rate bank: the Doppler sum of a map row taken along the echo's range walk AND its chirp, for a bank of K rates, with
// the strongest hypothesis kept per cell (gfx950 / MI355X only).  No reference counterpart: Ambiguity.cpp:152-169 sums the
// pulses of one delay column with a fixed Doppler.  Included by rate.hip alone: this header defines a kernel, so a second
// unit must not include it.
//
//   rate_bank_kernel   M_k[j][d] = sum_i [0 <= d + s(j,i) < nDelay] (R[i][d + s(j,i)] c_k[i]) W[(i src(j)) mod nD],
//                      out[j][d] = M_k*[j][d], index[j][d] = k*: the smallest k with the largest fp32 power x x + y y;
//                      s(j,i) and src(j) are migrate_kernels.hpp's (s = 0 with no table), c_k[i] the fp32 chirp table of
//                      blah2hip_amb_set_rates.  A candidate with q[k] == 0 in a zero-shift row is the input map's cell.  With
//                      the per-workgroup partials of Map::set_metrics (Map.cpp:187-206) of every output map.
//
// migrate_kernel's structure with one more axis.  A workgroup owns RATE_ROWS = 16 rows of a strip of 64 delay columns: a lane
// is a column, each of the four waves holds four rows, and a thread's eight accumulator slots are 4 rows x 2 hypotheses.  The
// bank goes in passes of two hypotheses; a pass is migrate_kernel's loop over blocks of RATE_BLK = 32 pulses:
//   1. 512 shifts (16 rows x 32 pulses), two per thread, with the host formula's bits; their smallest and largest give the
//      window of columns the block reads;
//   2. the window (whole 16-column tiles) of the block's pulses goes into LDS once a pass, zeros where the map has no column,
//      the shifts as 16-bit LDS cell offsets beside it, and the pass's two chirp values per pulse beside those.  A window too
//      wide for the 32 KiB is staged in runs of fewer pulses -- the order of the sum stays;
//   3. per pulse a wave reads its four offsets (one 8-byte LDS read) and the two chirps (one 16-byte LDS read), the same
//      addresses in every lane, then one 8-byte cell per row; the cell is multiplied by the chirp, then by the twiddle
//      (incremental index into exp(-2 pi i k / nD), wave-uniform: scalar loads) -- once per hypothesis.
// A block's sum is added into the running sum.  After a pass the two candidates meet the running best (value, power, index),
// which stays in registers, in the order of k: the first of equal powers wins.  The shifts and the order of the additions
// depend on (j, k, i) alone: equal inputs give equal bits at every placement, every n_maps and every position in the bank.
// Multiplying by c = (1, -0) (q = 0) returns a non-zero cell's bits, so bank {0} is migrate_kernel's sum.
#pragma once

#include <hip/hip_runtime.h>

#include "blah2hip.h"
#include "metrics_core.hpp"
#include "range_core.hpp"

namespace blah2 {

struct RateArgs {
  const cf *R;        // tiled range map of the last process call, see rmap_index()
  const cf *in;       // [nMaps][nD][nDelay]: read in zero-shift rows, and only where the bank holds a zero rate
  cf *out;            // [nMaps][nD][nDelay]: may be `in`
  uint8_t *index;     // [nMaps][nD][nDelay] or nullptr
  const cf *W;        // exp(-2 pi i k / nD), [nD]
  const double *half; // [nD] half walks h[j], or nullptr: no walk
  const cf *chirp;    // [nRates][nD]: c_k[i]
  double *partSum;    // [nMaps][gridDim.x * gridDim.y]: metrics_kernel's layout
  float *partMax;
  int32_t nD, nDelay, nTiles;
  uint32_t nRates, zeroRates; // bit k of zeroRates: q[k] == 0
};

constexpr int RATE_COLS = 64;                    // delay columns per workgroup: one per lane
constexpr int RATE_RPT = 4;                      // rows per thread
constexpr int RATE_HPT = 2;                      // hypotheses per thread and pass
constexpr int RATE_WAVES = 4;
constexpr int RATE_ROWS = RATE_RPT * RATE_WAVES; // rows per workgroup
constexpr int RATE_BLK = 32;                     // pulses per block of the summation (MIG_BLK)
constexpr int RATE_LDS_CELLS = 4096;             // staged cells: 32 pulses of a 128-column window
static_assert(((RATE_COLS + 2 * BLAH2HIP_MAX_MIGRATION + 30 + 15) / 16) * 16 <= RATE_LDS_CELLS, "one pulse of the widest window fits the stage");
static_assert(RATE_LDS_CELLS <= 65536, "cell offsets are 16 bits");
static_assert(BLAH2HIP_MAX_RATES <= 32, "zeroRates is a 32-bit mask");

typedef float rate_v2 __attribute__((ext_vector_type(2)));
typedef float rate_v4 __attribute__((ext_vector_type(4)));

// s(j, i): the bits of the host formula -- one fp64 multiply, ties to even (migrate_shift)
__device__ __forceinline__ int rate_shift(double h, int i, int nD) { return (int)rint(__dmul_rn(h, (double)(2 * i - (nD - 1)))); }

// grid (column strips, row groups, maps), 256 threads
__global__ __launch_bounds__(64 * RATE_WAVES) void rate_bank_kernel(RateArgs a)
{
  __shared__ __attribute__((aligned(16))) rate_v2 stage[RATE_LDS_CELLS];
  __shared__ __attribute__((aligned(16))) uint16_t offs[RATE_BLK][RATE_ROWS]; // [pulse of the block][row of the workgroup]
  __shared__ __attribute__((aligned(16))) rate_v4 chirps[RATE_BLK];           // [pulse of the block]: c_k0, c_k1 of the pass
  __shared__ int redLo[RATE_WAVES], redHi[RATE_WAVES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nD = a.nD, nDelay = a.nDelay, nTiles = a.nTiles;
  const int nRates = (int)a.nRates;
  const int c0 = blockIdx.x * RATE_COLS, col = c0 + lane;
  const int o0 = blockIdx.y * RATE_ROWS;
  const size_t cells = (size_t)nD * nDelay;
  const rate_v2 *Rm = reinterpret_cast<const rate_v2 *>(a.R) + (size_t)blockIdx.z * nTiles * nD * 16;

  // the wave's rows: Doppler index of the transform, zero-shift and in-the-map flags
  int src[RATE_RPT];
  uint32_t zmask = 0, vmask = 0; // bit kk: row kk has zero shift; row kk lies in the map
#pragma unroll
  for (int kk = 0; kk < RATE_RPT; kk++) {
    const int o = o0 + wave * RATE_RPT + kk;
    const int oc = o < nD ? o : nD - 1;
    src[kk] = (oc + nD / 2 + 1) % nD;
    if (!a.half || rate_shift(a.half[oc], nD - 1, nD) == 0) zmask |= 1u << kk;
    if (o < nD) vmask |= 1u << kk;
  }
  zmask = __builtin_amdgcn_readfirstlane(zmask);
  vmask = __builtin_amdgcn_readfirstlane(vmask);

  // the running best of every row of the thread
  cf best[RATE_RPT];
  float bestP[RATE_RPT];
  uint32_t bestK = 0; // eight bits a row
#pragma unroll
  for (int kk = 0; kk < RATE_RPT; kk++) {
    best[kk] = cmake(0.f, 0.f);
    bestP[kk] = 0.f;
  }

  // the shifts this thread works out in every block: row tid & 15 of the workgroup, pulses (tid >> 4) + 16 q of the block
  const int tr = tid & (RATE_ROWS - 1), tp = tid >> 4;
  const double hr = a.half ? a.half[min(o0 + tr, nD - 1)] : 0.0;
  const int sub = tid & 15, sp = tid >> 4; // staging: column of the tile, first pulse of the run

  for (int k0 = 0; k0 < nRates; k0 += RATE_HPT) {
    const int k1 = min(k0 + 1, nRates - 1); // an odd bank's last pass sums its last hypothesis twice and uses it once
    const bool z0 = (a.zeroRates >> k0) & 1u, z1 = (a.zeroRates >> k1) & 1u;
    // rows of the wave that need a sum in this pass: those in the map, less the zero-shift rows when both rates are zero
    const bool waveActive = (vmask & ~((z0 && z1) ? zmask : 0u)) != 0;
    cf acc[RATE_RPT * RATE_HPT];
#pragma unroll
    for (int s = 0; s < RATE_RPT * RATE_HPT; s++) acc[s] = cmake(0.f, 0.f);

    // a workgroup of copied candidates stages nothing
    if (__syncthreads_or(waveActive)) {
      int idx[RATE_RPT];
#pragma unroll
      for (int kk = 0; kk < RATE_RPT; kk++) idx[kk] = 0;
      const cf *ch0 = a.chirp + (size_t)k0 * nD, *ch1 = a.chirp + (size_t)k1 * nD;

      for (int ib = 0; ib < nD; ib += RATE_BLK) {
        const int nb = min(RATE_BLK, nD - ib);
        // 1. shifts, and the block's smallest and largest
        int sv[RATE_BLK / 16];
        int lo = INT_MAX, hi = INT_MIN;
#pragma unroll
        for (int q = 0; q < RATE_BLK / 16; q++) {
          const int pl = tp + 16 * q;
          sv[q] = rate_shift(hr, ib + min(pl, nb - 1), nD);
          lo = min(lo, sv[q]);
          hi = max(hi, sv[q]);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          lo = min(lo, __shfl_xor(lo, off));
          hi = max(hi, __shfl_xor(hi, off));
        }
        if (lane == 0) { redLo[wave] = lo; redHi[wave] = hi; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < RATE_WAVES; w++) {
          lo = min(lo, redLo[w]);
          hi = max(hi, redHi[w]);
        }
        // the window in whole tiles (>> floors: c0 + lo may be negative), and the pulses of a run
        const int t0 = (c0 + lo) >> 4, t1 = (c0 + RATE_COLS - 1 + hi) >> 4;
        const int nT = t1 - t0 + 1, Wc = nT * 16;
        const int P = min(RATE_BLK, RATE_LDS_CELLS / Wc); // >= 1: the static_assert above and set_migration's bound on the shifts
#pragma unroll
        for (int q = 0; q < RATE_BLK / 16; q++) {
          const int pl = tp + 16 * q;
          offs[pl][tr] = (uint16_t)((pl % P) * Wc + (c0 + sv[q] - t0 * 16)); // lane 0's cell of (pulse, row) in the stage
        }
        if (tid < RATE_BLK) { // the pass's chirps of the block's pulses
          const int i = ib + min(tid, nb - 1);
          const cf u = ch0[i], v = ch1[i];
          chirps[tid] = rate_v4{u.x, u.y, v.x, v.y};
        }

        cf blk[RATE_RPT * RATE_HPT];
#pragma unroll
        for (int s = 0; s < RATE_RPT * RATE_HPT; s++) blk[s] = cmake(0.f, 0.f);
        for (int cs = 0; cs < nb; cs += P) {
          const int pn = min(P, nb - cs);
          // 2. the run's pulses of the window: sixteen lanes a 128-byte line, two pulses a thread and tile in flight
          for (int tl = 0; tl < nT; tl++) {
            const int tile = t0 + tl;
            const bool cin = tile >= 0 && tile < nTiles && tile * 16 + sub < nDelay;
            const rate_v2 *src0 = Rm + ((size_t)(cin ? tile : 0) * nD + (ib + cs)) * 16 + sub;
            const bool in0 = cin && sp < pn, in1 = cin && sp + 16 < pn;
            const rate_v2 v0 = in0 ? src0[(size_t)sp * 16] : rate_v2{0.f, 0.f};
            const rate_v2 v1 = in1 ? src0[(size_t)(sp + 16) * 16] : rate_v2{0.f, 0.f};
            if (sp < pn) stage[sp * Wc + tl * 16 + sub] = v0;
            if (sp + 16 < pn) stage[(sp + 16) * Wc + tl * 16 + sub] = v1;
          }
          __syncthreads();
          // 3. the sums
          if (waveActive) {
            for (int p = 0; p < pn; p++) {
              const uint2 o = *reinterpret_cast<const uint2 *>(&offs[cs + p][wave * RATE_RPT]);
              const uint32_t e[RATE_RPT] = {o.x & 0xffffu, o.x >> 16, o.y & 0xffffu, o.y >> 16};
              const rate_v4 c = chirps[cs + p];
#pragma unroll
              for (int kk = 0; kk < RATE_RPT; kk++) {
                const rate_v2 r = stage[e[kk] + lane];
                const cf w = a.W[idx[kk]];
#pragma unroll
                for (int hh = 0; hh < RATE_HPT; hh++) {
                  const float cx = c[2 * hh], cy = c[2 * hh + 1];
                  // the fused operations spelt out, as the compiler contracts migrate_kernel's r * w: one product rounded,
                  // the other fused into the sum (bank {0} has to give that kernel's bits)
                  const float zx = fmaf(r[0], cx, -(r[1] * cy));
                  const float zy = fmaf(r[1], cx, r[0] * cy);
                  blk[kk * RATE_HPT + hh].x += fmaf(zx, w.x, -(zy * w.y));
                  blk[kk * RATE_HPT + hh].y += fmaf(zy, w.x, zx * w.y);
                }
                idx[kk] += src[kk];
                if (idx[kk] >= nD) idx[kk] -= nD;
              }
            }
          }
          __syncthreads(); // the stage, the offsets, the chirps and the two reduction words are free again
        }
#pragma unroll
        for (int s = 0; s < RATE_RPT * RATE_HPT; s++) acc[s] = cadd(acc[s], blk[s]);
      }
    }

    // the pass's candidates meet the running best, in the order of k
#pragma unroll
    for (int hh = 0; hh < RATE_HPT; hh++) {
      const int k = k0 + hh;
      if (k < nRates) {
        const bool zk = hh ? z1 : z0;
#pragma unroll
        for (int kk = 0; kk < RATE_RPT; kk++) {
          const int o = o0 + wave * RATE_RPT + kk;
          cf v = acc[kk * RATE_HPT + hh];
          if (zk && ((zmask >> kk) & 1u) && o < nD && col < nDelay) v = a.in[(size_t)blockIdx.z * cells + (size_t)o * nDelay + col];
          const float p = v.x * v.x + v.y * v.y;
          if (k == 0 || p > bestP[kk]) {
            best[kk] = v;
            bestP[kk] = p;
            bestK = (bestK & ~(0xffu << (8 * kk))) | ((uint32_t)k << (8 * kk));
          }
        }
      }
    }
  }

  // rows out, Map::set_metrics of the cells as written (a zero cell is -inf, as in the Doppler kernels)
  double lsum = 0.0;
  float lmax = 0.f;
#pragma unroll
  for (int kk = 0; kk < RATE_RPT; kk++) {
    const int o = o0 + wave * RATE_RPT + kk;
    if (o < nD && col < nDelay) {
      const size_t cell = (size_t)blockIdx.z * cells + (size_t)o * nDelay + col;
      a.out[cell] = best[kk];
      if (a.index) a.index[cell] = (uint8_t)((bestK >> (8 * kk)) & 0xffu);
      const float db = db_of(best[kk]);
      lsum += (double)db;
      lmax = fmaxf(lmax, db);
    }
  }
  const size_t part = (size_t)blockIdx.z * (gridDim.x * gridDim.y) + blockIdx.y * gridDim.x + blockIdx.x;
  block_metrics_partial(lsum, lmax, a.partSum + part, a.partMax + part);
}

} // namespace blah2
