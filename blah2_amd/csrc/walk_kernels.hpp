// Walk sums: the Doppler sum of a map row taken along the echo's walk through the delay columns -- range-migration
// compensation -- and, for a bank of K Doppler rates, along its chirp as well, with the strongest hypothesis kept per cell
// (gfx950 / MI355X only).  No reference counterpart: Ambiguity.cpp:152-169 sums the pulses of one delay column with a fixed
// Doppler.  Included by walk.hip alone: this header defines a kernel, so a second unit must not include it.
//
//   walk_sum_kernel<RPT, HPT>   M_k[j][d] = sum_i [0 <= d + s(j,i) < nDelay] (R[i][d + s(j,i)] c_k[i]) W[(i src(j)) mod nD],
//                               s(j,i) = (int) rint(h[j] * (double)(2i - (nD - 1)))  (0 with no table),
//                               src(j) = (j + nD/2 + 1) mod nD,  c_k[i] the fp32 chirp table of blah2hip_amb_set_rates,
//                               out[j][d] = M_k*[j][d], index[j][d] = k*: the smallest k with the largest fp32 power x x + y y.
//                               A candidate with q[k] == 0 in a zero-shift row (rint(h[j] (nD - 1)) == 0) is the input map's
//                               cell.  With the per-workgroup partials of Map::set_metrics (Map.cpp:187-206) of every
//                               output map.
//
// A workgroup owns ROWS = 4 RPT rows of a strip of 64 delay columns: a lane is a column, each of the four waves holds RPT rows,
// and a thread's eight accumulator slots are RPT rows x HPT hypotheses.  The bank goes in passes of HPT hypotheses, and in a
// pass every wave sums ALL pulses of its rows in index order (doppler_dft_kernel's arithmetic without its first-pulse
// subtraction, which needs a fixed column; no split of the pulse axis, no reduction).  Per block of WALK_BLK = 32 pulses:
//   1. 32 ROWS shifts, 32 ROWS / 256 per thread: one fp64 multiply and a round to nearest even -- the host formula's bits.
//      Their smallest and largest give the window of columns this block reads;
//   2. the window (whole 16-column tiles: 128-byte lines of the tiled range map) of the block's pulses goes into LDS once a
//      pass, zeros where the map has no column (outside 0 .. nDelay - 1: the tiles' padding columns are never read), the
//      shifts as 16-bit LDS cell offsets beside it, and the pass's chirp values per pulse beside those.  A window too wide for
//      the 32 KiB (rows whose shifts differ by more than 64 cells: only a table that is not smooth) is staged in runs of fewer
//      pulses -- the order of the sum stays;
//   3. per pulse a wave reads its RPT offsets (one LDS read of 2 RPT bytes) and the chirps (one 16-byte LDS read), the same
//      addresses in every lane, then one 8-byte cell per row; the cell is multiplied by the chirp, then by the twiddle
//      (incremental index into exp(-2 pi i k / nD), wave-uniform: scalar loads) -- once per hypothesis.
// A block's sum is added into the running sum (doppler_dft_kernel's comment gives the reason).  After a pass the candidates
// meet the running best (value, power, index), which stays in registers, in the order of k: the first of equal powers wins.
// The shifts and the order of the additions depend on (j, k, i) alone: equal inputs give equal bits at every placement, every
// n_maps and every position in the bank.
//
// The two shapes, and no others:
//   <8, 1>  blah2hip_amb_migrate_dev: 32 rows a workgroup, one hypothesis with c = 1 and q = 0, so one pass; no chirp array in
//           LDS and no chirp multiply, no index plane, no running best; a copied row is not stored when out is in;
//   <4, 2>  blah2hip_amb_rate_bank_dev: 16 rows a workgroup, two hypotheses a pass.
// Both run the one multiply-accumulate line below, and multiplying by c = (1, -0) returns a non-zero cell's bits: bank {0}
// with a table is <8, 1>'s sum.
#pragma once

#include <hip/hip_runtime.h>

#include "blah2hip.h"
#include "metrics_core.hpp"
#include "range_core.hpp"

namespace blah2 {

struct WalkArgs {
  const cf *R;        // tiled range map of the last process call, see rmap_index()
  const cf *in;       // [nMaps][nD][nDelay]: read in zero-shift rows, and only where the bank holds a zero rate
  cf *out;            // [nMaps][nD][nDelay]: may be `in`
  uint8_t *index;     // [nMaps][nD][nDelay] or nullptr
  const cf *W;        // exp(-2 pi i k / nD), [nD]
  const double *half; // [nD] half walks h[j], or nullptr: no walk
  const cf *chirp;    // [nRates][nD]: c_k[i]; this and the next two for HPT > 1 only
  double *partSum;    // [nMaps][gridDim.x * gridDim.y]: metrics_kernel's layout
  float *partMax;
  int32_t nD, nDelay, nTiles;
  uint32_t nRates, zeroRates; // bit k of zeroRates: q[k] == 0
};

constexpr int WALK_COLS = 64;        // delay columns per workgroup: one per lane
constexpr int WALK_WAVES = 4;
constexpr int WALK_BLK = 32;         // pulses per block of the summation (DOP_BLK)
constexpr int WALK_LDS_CELLS = 4096; // staged cells: 32 pulses of a 128-column window
// the widest window: 64 columns, shifts from -MAX to +MAX, and up to 15 columns of tile alignment at either end
static_assert(((WALK_COLS + 2 * BLAH2HIP_MAX_MIGRATION + 30 + 15) / 16) * 16 <= WALK_LDS_CELLS, "one pulse of the widest window fits the stage");
static_assert(WALK_LDS_CELLS <= 65536, "cell offsets are 16 bits");
static_assert(BLAH2HIP_MAX_RATES <= 32, "zeroRates is a 32-bit mask");

typedef float walk_v2 __attribute__((ext_vector_type(2)));
typedef float walk_v4 __attribute__((ext_vector_type(4)));

// s(j, i): the bits of the host formula -- one fp64 multiply (no contraction: there is nothing to fuse it with), ties to even
__device__ __forceinline__ int walk_shift(double h, int i, int nD) { return (int)rint(__dmul_rn(h, (double)(2 * i - (nD - 1)))); }

// grid (column strips, row groups, maps), 256 threads
template <int RPT, int HPT>
__global__ __launch_bounds__(64 * WALK_WAVES) void walk_sum_kernel(WalkArgs a)
{
  static_assert((RPT == 8 && HPT == 1) || (RPT == 4 && HPT == 2), "the two shapes of the header's comment");
  constexpr int ROWS = RPT * WALK_WAVES;   // rows per workgroup
  constexpr int PSTEP = 256 / ROWS;        // a thread's shifts: row tid % ROWS, pulses tid / ROWS + PSTEP q of the block
  constexpr int SHIFTS = WALK_BLK / PSTEP; // of them
  constexpr int SLOTS = RPT * HPT;
  typedef uint32_t offs_v __attribute__((ext_vector_type(RPT / 2)));
  __shared__ __attribute__((aligned(16))) walk_v2 stage[WALK_LDS_CELLS];
  __shared__ __attribute__((aligned(16))) uint16_t offs[WALK_BLK][ROWS];     // [pulse of the block][row of the workgroup]
  __shared__ __attribute__((aligned(16))) walk_v4 chirps[HPT > 1 ? WALK_BLK : 1]; // [pulse of the block]: c_k0, c_k1 of the pass
  __shared__ int redLo[WALK_WAVES], redHi[WALK_WAVES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nD = a.nD, nDelay = a.nDelay, nTiles = a.nTiles;
  const int nRates = HPT > 1 ? (int)a.nRates : 1;
  const uint32_t zeroRates = HPT > 1 ? a.zeroRates : 1u;
  const int c0 = blockIdx.x * WALK_COLS, col = c0 + lane;
  const int o0 = blockIdx.y * ROWS;
  const size_t cells = (size_t)nD * nDelay;
  const walk_v2 *Rm = reinterpret_cast<const walk_v2 *>(a.R) + (size_t)blockIdx.z * nTiles * nD * 16;

  // the wave's rows: Doppler index of the transform, zero-shift and in-the-map flags
  int src[RPT];
  uint32_t zmask = 0, vmask = 0; // bit kk: row kk has zero shift; row kk lies in the map
#pragma unroll
  for (int kk = 0; kk < RPT; kk++) {
    const int o = o0 + wave * RPT + kk;
    const int oc = o < nD ? o : nD - 1;
    src[kk] = (oc + nD / 2 + 1) % nD;
    if (!a.half || walk_shift(a.half[oc], nD - 1, nD) == 0) zmask |= 1u << kk;
    if (o < nD) vmask |= 1u << kk;
  }
  zmask = __builtin_amdgcn_readfirstlane(zmask);
  vmask = __builtin_amdgcn_readfirstlane(vmask);

  // the running best of every row of the thread (HPT == 1: the one candidate)
  cf best[RPT];
  float bestP[RPT];
  uint32_t bestK = 0; // eight bits a row
#pragma unroll
  for (int kk = 0; kk < RPT; kk++) {
    best[kk] = cmake(0.f, 0.f);
    bestP[kk] = 0.f;
  }

  const int tr = tid & (ROWS - 1), tp = tid / ROWS;
  const double hr = a.half ? a.half[min(o0 + tr, nD - 1)] : 0.0;
  const int sub = tid & 15, sp = tid >> 4; // staging: column of the tile, first pulse of the run

  for (int k0 = 0; k0 < nRates; k0 += HPT) {
    const int k1 = min(k0 + 1, nRates - 1); // an odd bank's last pass sums its last hypothesis twice and uses it once
    const bool z0 = (zeroRates >> k0) & 1u, z1 = (zeroRates >> k1) & 1u;
    // rows of the wave that need a sum in this pass: those in the map, less the zero-shift rows when both rates are zero
    const bool waveActive = (vmask & ~((z0 && z1) ? zmask : 0u)) != 0;
    cf acc[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; s++) acc[s] = cmake(0.f, 0.f);

    // a workgroup of copied candidates stages nothing
    if (__syncthreads_or(waveActive)) {
      int idx[RPT];
#pragma unroll
      for (int kk = 0; kk < RPT; kk++) idx[kk] = 0;
      const cf *ch0 = a.chirp + (size_t)k0 * nD, *ch1 = a.chirp + (size_t)k1 * nD;

      for (int ib = 0; ib < nD; ib += WALK_BLK) {
        const int nb = min(WALK_BLK, nD - ib);
        // 1. shifts, and the block's smallest and largest
        int sv[SHIFTS];
        int lo = INT_MAX, hi = INT_MIN;
#pragma unroll
        for (int q = 0; q < SHIFTS; q++) {
          const int pl = tp + PSTEP * q;
          sv[q] = walk_shift(hr, ib + min(pl, nb - 1), nD);
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
        for (int w = 0; w < WALK_WAVES; w++) {
          lo = min(lo, redLo[w]);
          hi = max(hi, redHi[w]);
        }
        // the window in whole tiles (>> floors: c0 + lo may be negative), and the pulses of a run
        const int t0 = (c0 + lo) >> 4, t1 = (c0 + WALK_COLS - 1 + hi) >> 4;
        const int nT = t1 - t0 + 1, Wc = nT * 16;
        const int P = min(WALK_BLK, WALK_LDS_CELLS / Wc); // >= 1: the static_assert above and set_migration's bound on the shifts
#pragma unroll
        for (int q = 0; q < SHIFTS; q++) {
          const int pl = tp + PSTEP * q;
          offs[pl][tr] = (uint16_t)((pl % P) * Wc + (c0 + sv[q] - t0 * 16)); // lane 0's cell of (pulse, row) in the stage
        }
        if constexpr (HPT > 1) {
          if (tid < WALK_BLK) { // the pass's chirps of the block's pulses
            const int i = ib + min(tid, nb - 1);
            const cf u = ch0[i], v = ch1[i];
            chirps[tid] = walk_v4{u.x, u.y, v.x, v.y};
          }
        }

        cf blk[SLOTS];
#pragma unroll
        for (int s = 0; s < SLOTS; s++) blk[s] = cmake(0.f, 0.f);
        for (int cs = 0; cs < nb; cs += P) {
          const int pn = min(P, nb - cs);
          // 2. the run's pulses of the window: sixteen lanes a 128-byte line, two pulses a thread and tile in flight
          for (int tl = 0; tl < nT; tl++) {
            const int tile = t0 + tl;
            const bool cin = tile >= 0 && tile < nTiles && tile * 16 + sub < nDelay;
            const walk_v2 *src0 = Rm + ((size_t)(cin ? tile : 0) * nD + (ib + cs)) * 16 + sub;
            const bool in0 = cin && sp < pn, in1 = cin && sp + 16 < pn;
            const walk_v2 v0 = in0 ? src0[(size_t)sp * 16] : walk_v2{0.f, 0.f};
            const walk_v2 v1 = in1 ? src0[(size_t)(sp + 16) * 16] : walk_v2{0.f, 0.f};
            if (sp < pn) stage[sp * Wc + tl * 16 + sub] = v0;
            if (sp + 16 < pn) stage[(sp + 16) * Wc + tl * 16 + sub] = v1;
          }
          __syncthreads();
          // 3. the sums
          if (waveActive) {
            for (int p = 0; p < pn; p++) {
              const offs_v o = *reinterpret_cast<const offs_v *>(&offs[cs + p][wave * RPT]);
              uint32_t e[RPT];
#pragma unroll
              for (int kk = 0; kk < RPT; kk++) e[kk] = (kk & 1) ? o[kk / 2] >> 16 : o[kk / 2] & 0xffffu;
              walk_v4 c;
              if constexpr (HPT > 1) c = chirps[cs + p];
#pragma unroll
              for (int kk = 0; kk < RPT; kk++) {
                const walk_v2 r = stage[e[kk] + lane];
                const cf w = a.W[idx[kk]];
#pragma unroll
                for (int hh = 0; hh < HPT; hh++) {
                  // the fused operations spelt out, so that both shapes round alike: one product rounded, the other fused,
                  // then the add into the block's sum
                  float zx = r[0], zy = r[1];
                  if constexpr (HPT > 1) {
                    const float cx = c[2 * hh], cy = c[2 * hh + 1];
                    zx = fmaf(r[0], cx, -(r[1] * cy));
                    zy = fmaf(r[1], cx, r[0] * cy);
                  }
                  blk[kk * HPT + hh].x += fmaf(zx, w.x, -(zy * w.y));
                  blk[kk * HPT + hh].y += fmaf(zy, w.x, zx * w.y);
                }
                idx[kk] += src[kk];
                if (idx[kk] >= nD) idx[kk] -= nD;
              }
            }
          }
          __syncthreads(); // the stage, the offsets, the chirps and the two reduction words are free again
        }
#pragma unroll
        for (int s = 0; s < SLOTS; s++) acc[s] = cadd(acc[s], blk[s]);
      }
    }

    // the pass's candidates meet the running best, in the order of k
#pragma unroll
    for (int hh = 0; hh < HPT; hh++) {
      const int k = k0 + hh;
      if (k < nRates) {
        const bool zk = hh ? z1 : z0;
#pragma unroll
        for (int kk = 0; kk < RPT; kk++) {
          const int o = o0 + wave * RPT + kk;
          cf v = acc[kk * HPT + hh];
          if (zk && ((zmask >> kk) & 1u) && o < nD && col < nDelay) v = a.in[(size_t)blockIdx.z * cells + (size_t)o * nDelay + col];
          if constexpr (HPT == 1) {
            best[kk] = v;
          } else {
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
  }

  // rows out, Map::set_metrics of the cells as written (a zero cell is -inf, as in the Doppler kernels)
  double lsum = 0.0;
  float lmax = 0.f;
  const bool inPlace = a.in == a.out;
#pragma unroll
  for (int kk = 0; kk < RPT; kk++) {
    const int o = o0 + wave * RPT + kk;
    if (o < nD && col < nDelay) {
      const size_t cell = (size_t)blockIdx.z * cells + (size_t)o * nDelay + col;
      // HPT == 1: a copied row of an in-place call is the cell that is there
      if (!(HPT == 1 && ((zmask >> kk) & 1u) && inPlace)) a.out[cell] = best[kk];
      if constexpr (HPT > 1) {
        if (a.index) a.index[cell] = (uint8_t)((bestK >> (8 * kk)) & 0xffu);
      }
      const float db = db_of(best[kk]);
      lsum += (double)db;
      lmax = fmaxf(lmax, db);
    }
  }
  const size_t part = (size_t)blockIdx.z * (gridDim.x * gridDim.y) + blockIdx.y * gridDim.x + blockIdx.x;
  block_metrics_partial(lsum, lmax, a.partSum + part, a.partMax + part);
}

} // namespace blah2
