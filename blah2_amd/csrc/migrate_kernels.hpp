// Range-migration compensation: the Doppler sum of a map row taken along the echo's walk through the delay columns
// (gfx950 / MI355X only).  No reference counterpart: Ambiguity.cpp:152-169 sums the pulses of one delay column.
// Included by migrate.hip alone: this header defines a kernel, so a second unit must not include it.
//
//   migrate_kernel   M'[j][d] = sum_i [0 <= d + s(j,i) < nDelay] R[i][d + s(j,i)] W[(i src(j)) mod nD],
//                    s(j,i) = (int) rint(h[j] * (double)(2i - (nD - 1))),  src(j) = (j + nD/2 + 1) mod nD,
//                    for every row j whose shifts are not all zero; a zero-shift row (rint(h[j] (nD - 1)) == 0) is copied
//                    from the input map.  With the per-workgroup partials of Map::set_metrics (Map.cpp:187-206) of every
//                    output map.
//
// A workgroup owns MIG_ROWS = 32 rows of a strip of 64 delay columns: a lane is a column, each of the four waves holds
// eight rows, and every wave sums ALL pulses of its rows in index order (doppler_dft_kernel's arithmetic without its
// first-pulse subtraction, which needs a fixed column; no split of the pulse axis, no reduction).  Per block of MIG_BLK =
// 32 pulses:
//   1. 1024 shifts (32 rows x 32 pulses), four per thread: one fp64 multiply and a round to nearest even -- the host
//      formula's bits.  Their smallest and largest give the window of columns this block reads;
//   2. the window (whole 16-column tiles: 128-byte lines of the tiled range map) of the block's pulses goes into LDS
//      once, zeros where the map has no column (outside 0 .. nDelay - 1: the tiles' padding columns are never read), and the
//      shifts as 16-bit LDS cell offsets beside it.  A window too wide for the 32 KiB (rows whose shifts differ by more
//      than 64 cells: only a table that is not smooth) is staged in runs of fewer pulses -- the order of the sum stays;
//   3. per pulse a wave reads its eight offsets (one 16-byte LDS read, the same address in every lane), then one 8-byte
//      cell per row, twiddles by the incremental index from exp(-2 pi i k / nD) (wave-uniform: scalar loads).
// A block's sum is added into the running sum (doppler_dft_kernel's comment gives the reason).  The shifts and the order
// of the additions depend on (j, i) alone: equal inputs give equal bits at every placement and every n_maps.
#pragma once

#include <hip/hip_runtime.h>

#include "blah2hip.h"
#include "metrics_core.hpp"
#include "range_core.hpp"

namespace blah2 {

struct MigrateArgs {
  const cf *R;        // tiled range map of the last process call, see rmap_index()
  const cf *in;       // [nMaps][nD][nDelay]: read in zero-shift rows only
  cf *out;            // [nMaps][nD][nDelay]: may be `in`
  const cf *W;        // exp(-2 pi i k / nD), [nD]
  const double *half; // [nD] half walks h[j]
  double *partSum;    // [nMaps][gridDim.x * gridDim.y]: metrics_kernel's layout
  float *partMax;
  int32_t nD, nDelay, nTiles;
};

constexpr int MIG_COLS = 64;                    // delay columns per workgroup: one per lane
constexpr int MIG_KPT = 8;                      // rows per thread
constexpr int MIG_WAVES = 4;
constexpr int MIG_ROWS = MIG_KPT * MIG_WAVES;   // rows per workgroup
constexpr int MIG_BLK = 32;                     // pulses per block of the summation (DOP_BLK)
constexpr int MIG_LDS_CELLS = 4096;             // staged cells: 32 pulses of a 128-column window
// the widest window: 64 columns, shifts from -MAX to +MAX, and up to 15 columns of tile alignment at either end
static_assert(((MIG_COLS + 2 * BLAH2HIP_MAX_MIGRATION + 30 + 15) / 16) * 16 <= MIG_LDS_CELLS, "one pulse of the widest window fits the stage");
static_assert(MIG_LDS_CELLS <= 65536, "cell offsets are 16 bits");

typedef float mig_v2 __attribute__((ext_vector_type(2)));

// s(j, i): the bits of the host formula -- one fp64 multiply (no contraction: there is nothing to fuse it with), ties to even
__device__ __forceinline__ int migrate_shift(double h, int i, int nD) { return (int)rint(__dmul_rn(h, (double)(2 * i - (nD - 1)))); }

// grid (column strips, row groups, maps), 256 threads
__global__ __launch_bounds__(64 * MIG_WAVES) void migrate_kernel(MigrateArgs a)
{
  __shared__ __attribute__((aligned(16))) mig_v2 stage[MIG_LDS_CELLS];
  __shared__ __attribute__((aligned(16))) uint16_t offs[MIG_BLK][MIG_ROWS]; // [pulse of the block][row of the workgroup]
  __shared__ int redLo[MIG_WAVES], redHi[MIG_WAVES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nD = a.nD, nDelay = a.nDelay, nTiles = a.nTiles;
  const int c0 = blockIdx.x * MIG_COLS, col = c0 + lane;
  const int o0 = blockIdx.y * MIG_ROWS;
  const size_t cells = (size_t)nD * nDelay;
  const mig_v2 *Rm = reinterpret_cast<const mig_v2 *>(a.R) + (size_t)blockIdx.z * nTiles * nD * 16;

  // the wave's rows: Doppler index of the transform, running twiddle index, zero-shift flags
  int src[MIG_KPT], idx[MIG_KPT];
  cf acc[MIG_KPT];
  uint32_t zmask = 0; // bit kk: row kk is copied (zero shift) or lies behind the map's last row
#pragma unroll
  for (int kk = 0; kk < MIG_KPT; kk++) {
    const int o = o0 + wave * MIG_KPT + kk;
    const int oc = o < nD ? o : nD - 1;
    src[kk] = (oc + nD / 2 + 1) % nD;
    idx[kk] = 0;
    acc[kk] = cmake(0.f, 0.f);
    if (o >= nD || migrate_shift(a.half[oc], nD - 1, nD) == 0) zmask |= 1u << kk;
  }
  zmask = __builtin_amdgcn_readfirstlane(zmask);
  const bool waveActive = zmask != (1u << MIG_KPT) - 1;

  // a workgroup of copied rows stages nothing
  if (__syncthreads_or(waveActive)) {
    // the shifts this thread works out in every block: row tid & 31 of the workgroup, pulses (tid >> 5) + 8 q of the block
    const int tr = tid & (MIG_ROWS - 1), tp = tid >> 5;
    const double hr = a.half[min(o0 + tr, nD - 1)];
    const int sub = tid & 15, sp = tid >> 4; // staging: column of the tile, first pulse of the run

    for (int ib = 0; ib < nD; ib += MIG_BLK) {
      const int nb = min(MIG_BLK, nD - ib);
      // 1. shifts, and the block's smallest and largest
      int sv[MIG_BLK / 8];
      int lo = INT_MAX, hi = INT_MIN;
#pragma unroll
      for (int q = 0; q < MIG_BLK / 8; q++) {
        const int pl = tp + 8 * q;
        sv[q] = migrate_shift(hr, ib + min(pl, nb - 1), nD);
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
      for (int w = 0; w < MIG_WAVES; w++) {
        lo = min(lo, redLo[w]);
        hi = max(hi, redHi[w]);
      }
      // the window in whole tiles (>> floors: c0 + lo may be negative), and the pulses of a run
      const int t0 = (c0 + lo) >> 4, t1 = (c0 + MIG_COLS - 1 + hi) >> 4;
      const int nT = t1 - t0 + 1, Wc = nT * 16;
      const int P = min(MIG_BLK, MIG_LDS_CELLS / Wc); // >= 1: the static_assert above and set_migration's bound on the shifts
#pragma unroll
      for (int q = 0; q < MIG_BLK / 8; q++) {
        const int pl = tp + 8 * q;
        offs[pl][tr] = (uint16_t)((pl % P) * Wc + (c0 + sv[q] - t0 * 16)); // lane 0's cell of (pulse, row) in the stage
      }

      cf blk[MIG_KPT];
#pragma unroll
      for (int kk = 0; kk < MIG_KPT; kk++) blk[kk] = cmake(0.f, 0.f);
      for (int cs = 0; cs < nb; cs += P) {
        const int pn = min(P, nb - cs);
        // 2. the run's pulses of the window: sixteen lanes a 128-byte line, two pulses a thread and tile in flight
        for (int tl = 0; tl < nT; tl++) {
          const int tile = t0 + tl;
          const bool cin = tile >= 0 && tile < nTiles && tile * 16 + sub < nDelay;
          const mig_v2 *src0 = Rm + ((size_t)(cin ? tile : 0) * nD + (ib + cs)) * 16 + sub;
          const bool in0 = cin && sp < pn, in1 = cin && sp + 16 < pn;
          const mig_v2 v0 = in0 ? src0[(size_t)sp * 16] : mig_v2{0.f, 0.f};
          const mig_v2 v1 = in1 ? src0[(size_t)(sp + 16) * 16] : mig_v2{0.f, 0.f};
          if (sp < pn) stage[sp * Wc + tl * 16 + sub] = v0;
          if (sp + 16 < pn) stage[(sp + 16) * Wc + tl * 16 + sub] = v1;
        }
        __syncthreads();
        // 3. the sums
        if (waveActive) {
          for (int p = 0; p < pn; p++) {
            const uint4 o = *reinterpret_cast<const uint4 *>(&offs[cs + p][wave * MIG_KPT]);
            const uint32_t e[MIG_KPT] = {o.x & 0xffffu, o.x >> 16, o.y & 0xffffu, o.y >> 16, o.z & 0xffffu, o.z >> 16, o.w & 0xffffu, o.w >> 16};
#pragma unroll
            for (int kk = 0; kk < MIG_KPT; kk++) {
              const mig_v2 r = stage[e[kk] + lane];
              const cf w = a.W[idx[kk]];
              blk[kk].x += r[0] * w.x - r[1] * w.y;
              blk[kk].y += r[0] * w.y + r[1] * w.x;
              idx[kk] += src[kk];
              if (idx[kk] >= nD) idx[kk] -= nD;
            }
          }
        }
        __syncthreads(); // the stage, the offsets and the two reduction words are free again
      }
#pragma unroll
      for (int kk = 0; kk < MIG_KPT; kk++) acc[kk] = cadd(acc[kk], blk[kk]);
    }
  }

  // rows out, copied rows through, Map::set_metrics of the cells as written (a zero cell is -inf, as in the Doppler kernels)
  double lsum = 0.0;
  float lmax = 0.f;
  const bool inPlace = a.in == a.out;
#pragma unroll
  for (int kk = 0; kk < MIG_KPT; kk++) {
    const int o = o0 + wave * MIG_KPT + kk;
    if (o < nD && col < nDelay) {
      const size_t cell = (size_t)blockIdx.z * cells + (size_t)o * nDelay + col;
      const bool copied = (zmask >> kk) & 1u;
      const cf v = copied ? a.in[cell] : acc[kk];
      if (!(copied && inPlace)) a.out[cell] = v;
      const float db = db_of(v);
      lsum += (double)db;
      lmax = fmaxf(lmax, db);
    }
  }
  const size_t part = (size_t)blockIdx.z * (gridDim.x * gridDim.y) + blockIdx.y * gridDim.x + blockIdx.x;
  block_metrics_partial(lsum, lmax, a.partSum + part, a.partMax + part);
}

} // namespace blah2
