// Kernels of ddc.hip: the digital down-converter (mix, low-pass, decimate; blah2hip_ddc_*).
//   ddc_kernel<R, CB>   a tile of consecutive outputs of one row, every carrier, both channels
//   ddc_tail_kernel     behind it on the same stream: the stream's last T - 1 samples into the history, the position advanced
//   ddc_reset_kernel    the history zeroed, the position set
// Output m (absolute index) of carrier c is v_c[m] = p_c[m] sum_t g_c[t] u[m D - t]: g_c[t] = fp32(h[t] exp(+2 pi i f_c t / fs))
// is made in fp64 at create, p_c[m] = exp(-2 pi i frac(r_c m)), r_c = f_c D / fs in fp64, once per output.
//
// Phase.  frac(r m) = fma(r, m, -rint(r m)): the exact product less the whole number next to it, rounded once, so that only
// r's own rounding remains, and the phasor is the rounding of an fp64 sincospi.  No fp32 product f n is ever formed.
//
// Arithmetic.  Per output and channel 4 T fp32 fused multiply-adds in tap order t = T - 1 ... 0 (where the plan splits the
// taps: in 2 or 4 runs of consecutive taps, their sums added in run order), always the same chain for a handle: an output's
// bits depend on its samples and its index only, not on the tile, the row or the call it falls into.
// Error per output against the exact sum with the rounded taps, in units of 2^-24 sum_t |g[t]| |u[m D - t]|: the two
// chains of 2 T multiply-adds per component 2 T sqrt 2 <= 3 T, the rounded phasor 0.71, its fp32 complex product 2,
// the fp64 phase 2 pi 2^-53 |r| m (nothing at m < 2^45): under the contract's 3 T + 8.
//
// LDS image.  Lanes own neighbouring outputs, which read the window D samples apart: at even D a bank conflict.  The
// window is therefore stored by polyphase: sample w of the window (w = 0 at the tile's first output's oldest tap) sits at
// [w mod D][w div D], a row of Lp entries per phase, one entry the 16 bytes (x.re, x.im, y.re, y.im).  For a tap the lanes
// then read consecutive entries of one row: ds_read_b128 on consecutive 16-byte words, conflict-free in each of its
// lane groups.  Lp is odd, so the staging's ds_write_b128 of consecutive samples (rows apart, 4 Lp dwords) spreads its
// groups of 8 lanes over all 32 banks.  A thread owns outputs tid, tid + blockDim, ... (R of them): a loaded tap serves
// 2 R complex products, a loaded sample CB carriers.  The taps come through scalar loads (uniform index, read-only
// table [carrier][T - 1 - t]), not through LDS: at 8 carriers of 1024 taps they alone would be 64 KB.
#pragma once

#include "range_core.hpp"

namespace blah2 {

__device__ __forceinline__ cf ddc_mul(cf a, cf b) { return cmake(fmaf(-a.y, b.y, a.x * b.x), fmaf(a.y, b.x, a.x * b.y)); }

// a tap read through the constant address space: the table is written before the launch and by nobody during it, and the
// index is uniform, so the loads are scalar
typedef __attribute__((address_space(4))) const float DdcTap;

constexpr int DDC_LDS_SAMPLES = 5120; // entries of 16 bytes: 80 KB, two workgroups a CU

constexpr int DDC_PART_SAMPLES = 768; // ... of which the segments' partial sums take this much where the taps are split

struct DdcPlan { uint32_t tile, threads, R, Lp, TR; };

// Outputs per workgroup for (D, T): the largest of 1024, 512, 256, 192 whose polyphase image fits DDC_LDS_SAMPLES; above
// 256 halved while the lead-in stays under a sixteenth of the tile's own samples (a smaller image: more workgroups a
// CU).  Where not even 192 fit (large D T) the tile is 128, 64 or what fits below that, TR = 128 or 64 lanes own its outputs
// and the 256 threads are 2 or 4 SEGMENTS of TR lanes that split the taps between them (64 threads a workgroup at two
// workgroups a CU would leave a CU two waves); their partial sums meet in LDS behind the image.
__host__ __device__ static inline DdcPlan ddc_plan(uint32_t D, uint32_t T)
{
  const uint32_t lead = (T - 1 + D - 1) / D; // entries per phase row the lead-in takes
  uint32_t fit = DDC_LDS_SAMPLES / D - lead - 1;
  DdcPlan p;
  if (fit >= 192) {
    p.tile = fit >= 1024 ? 1024 : fit >= 512 ? 512 : fit >= 256 ? 256 : 192;
    while (p.tile > 256 && (uint64_t)(T - 1) * 16 <= (uint64_t)(p.tile / 2) * D) p.tile /= 2;
    p.threads = p.tile >= 256 ? 256 : 192;
    p.TR = p.threads;
  } else {
    fit = (DDC_LDS_SAMPLES - DDC_PART_SAMPLES) / D - lead - 1;
    p.tile = fit >= 128 ? 128 : fit >= 64 ? 64 : fit;
    p.threads = 256;
    p.TR = p.tile > 64 ? 128 : 64;
  }
  p.R = (p.tile + p.TR - 1) / p.TR;
  p.Lp = (p.tile + lead) | 1;
  return p;
}

// dynamic LDS of a launch: the image, and the partial sums where the taps are split
__host__ __device__ static inline size_t ddc_lds_bytes(uint32_t D, const DdcPlan &p)
{
  return ((size_t)D * p.Lp + (p.threads > p.TR ? DDC_PART_SAMPLES : 0)) * 16;
}

struct DdcArgs {
  const void *x, *y;     // the call's input in its format (y unused with FMT_I16)
  uint64_t inStride;     // samples from row to row
  uint32_t nIn, nOut;    // samples, outputs per row
  int fmt;
  const cf *hist;        // [2][T - 1]: the stream's samples in front of row 0, x then y
  const cf *taps;        // [carriers padded to CB][T]: entry s is g_c[T - 1 - s]
  const double *r;       // [carriers padded]
  const uint64_t *pos;   // absolute index of row 0's first output
  cf *outX, *outY;
  uint64_t outStride, carrierStride;
  uint32_t D, T, C, tile, Lp, TR;
};

// sample i (it may be negative: the rows in front, then the history) of row `row`, both channels
__device__ __forceinline__ float4 ddc_load(const DdcArgs &a, uint32_t row, int64_t i)
{
  if (i < 0) {
    const int64_t j = (int64_t)row * a.nIn + i;
    if (j < 0) {
      const int64_t H = (int64_t)a.T - 1;
      const cf vx = a.hist[H + j], vy = a.hist[2 * H + j];
      return make_float4(vx.x, vx.y, vy.x, vy.y);
    }
    row = (uint32_t)(j / a.nIn);
    i = j % a.nIn;
  }
  const uint64_t e = (uint64_t)row * a.inStride + (uint64_t)i;
  if (a.fmt == BLAH2HIP_FMT_C32) {
    const cf vx = ((const cf *)a.x)[e], vy = ((const cf *)a.y)[e];
    return make_float4(vx.x, vx.y, vy.x, vy.y);
  }
  if (a.fmt == BLAH2HIP_FMT_I16) { // I1 Q1 I2 Q2
    const short4 v = ((const short4 *)a.x)[e];
    return make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
  }
  const char2 vx = ((const char2 *)a.x)[e], vy = ((const char2 *)a.y)[e];
  return make_float4((float)vx.x, (float)vx.y, (float)vy.x, (float)vy.y);
}

// grid (tiles, rows), `threads` of the plan, dynamic LDS ddc_lds_bytes()
template <int R, int CB> __global__ __launch_bounds__(256) void ddc_kernel(DdcArgs a)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char ddc_lds[];
  float4 *win = (float4 *)ddc_lds;
  const uint32_t tid = threadIdx.x, BD = blockDim.x, row = blockIdx.y;
  const uint32_t o0 = blockIdx.x * a.tile;
  const uint32_t nT = min(a.tile, a.nOut - o0);
  const uint32_t D = a.D, T = a.T, Lp = a.Lp;

  // the window: samples o0 D - (T - 1) ... (o0 + nT - 1) D of the row
  const uint32_t W = (nT - 1) * D + T;
  const int64_t i0 = (int64_t)o0 * D - (int64_t)(T - 1);
  {
    // sample w to [w mod D][w div D]: one division a thread, then steps of blockDim
    const uint32_t dq = BD / D, dph = BD - dq * D;
    uint32_t q = tid / D, ph = tid - q * D;
    for (uint32_t w = tid; w < W; w += BD) {
      win[ph * Lp + q] = ddc_load(a, row, i0 + w);
      q += dq;
      ph += dph;
      if (ph >= D) { ph -= D; q++; }
    }
  }
  __syncthreads();

  // lane `lane` of segment `seg` (uniform in a wave: TR is a multiple of 64) sums the taps s0 ... s1 - 1 of its outputs
  const uint32_t TR = a.TR, G = BD / TR;
  const uint32_t seg = __builtin_amdgcn_readfirstlane(tid / TR), lane = tid - seg * TR;
  const uint32_t Tseg = (T + G - 1) / G, s0 = min(T, seg * Tseg), s1 = min(T, s0 + Tseg);
  constexpr int NV = 4 * R * CB; // sums a thread
  float *part = (float *)(win + (size_t)D * Lp); // [G - 1][NV][TR]

  const uint32_t Cpad = (a.C + CB - 1) / CB * CB;
  for (uint32_t cb = 0; cb < Cpad; cb += CB) {
    float xr[R][CB], xi[R][CB], yr[R][CB], yi[R][CB];
#pragma unroll
    for (int k = 0; k < R; k++)
#pragma unroll
      for (int c = 0; c < CB; c++) xr[k][c] = xi[k][c] = yr[k][c] = yi[k][c] = 0.f;
    const DdcTap *g = (const DdcTap *)(uintptr_t)(a.taps + (size_t)cb * T);
    uint32_t ph = s0 % D;
    // (a tile below 64 outputs leaves lanes without one: they stay inside the image)
    const float4 *p = win + (lane < a.tile ? lane : 0) + (size_t)ph * Lp + s0 / D;
    const DdcTap *gp = g + 2 * (size_t)s0;
#pragma unroll 4
    for (uint32_t s = s0; s < s1; s++, gp += 2) { // tap T - 1 - s: window sample m D + s of output m, phase row s mod D, entry m + s div D
      float4 u[R];
#pragma unroll
      for (int k = 0; k < R; k++) u[k] = p[k * TR];
#pragma unroll
      for (int c = 0; c < CB; c++) {
        const cf gc = cmake(gp[2 * (size_t)c * T], gp[2 * (size_t)c * T + 1]);
#pragma unroll
        for (int k = 0; k < R; k++) {
          xr[k][c] = fmaf(gc.x, u[k].x, xr[k][c]);
          xr[k][c] = fmaf(-gc.y, u[k].y, xr[k][c]);
          xi[k][c] = fmaf(gc.x, u[k].y, xi[k][c]);
          xi[k][c] = fmaf(gc.y, u[k].x, xi[k][c]);
          yr[k][c] = fmaf(gc.x, u[k].z, yr[k][c]);
          yr[k][c] = fmaf(-gc.y, u[k].w, yr[k][c]);
          yi[k][c] = fmaf(gc.x, u[k].w, yi[k][c]);
          yi[k][c] = fmaf(gc.y, u[k].z, yi[k][c]);
        }
      }
      p += Lp;
      if (++ph == D) { ph = 0; p -= (size_t)D * Lp - 1; }
    }
    if (G > 1) { // segments 1 ... leave their sums, segment 0 adds them in segment order: the same chain for every output
      if (seg > 0) {
        float *d = part + (size_t)(seg - 1) * NV * TR + lane;
#pragma unroll
        for (int k = 0; k < R; k++)
#pragma unroll
          for (int c = 0; c < CB; c++) {
            d[(4 * (k * CB + c) + 0) * TR] = xr[k][c];
            d[(4 * (k * CB + c) + 1) * TR] = xi[k][c];
            d[(4 * (k * CB + c) + 2) * TR] = yr[k][c];
            d[(4 * (k * CB + c) + 3) * TR] = yi[k][c];
          }
      }
      __syncthreads();
      if (seg == 0)
        for (uint32_t g2 = 1; g2 < G; g2++) {
          const float *d = part + (size_t)(g2 - 1) * NV * TR + lane;
#pragma unroll
          for (int k = 0; k < R; k++)
#pragma unroll
            for (int c = 0; c < CB; c++) {
              xr[k][c] += d[(4 * (k * CB + c) + 0) * TR];
              xi[k][c] += d[(4 * (k * CB + c) + 1) * TR];
              yr[k][c] += d[(4 * (k * CB + c) + 2) * TR];
              yi[k][c] += d[(4 * (k * CB + c) + 3) * TR];
            }
        }
      __syncthreads(); // (the next carrier block's sums go to the same place)
    }
    if (seg != 0) continue;
    const uint64_t m0 = *a.pos + (uint64_t)row * a.nOut + o0;
#pragma unroll
    for (int k = 0; k < R; k++) {
      const uint32_t m = lane + k * TR;
      if (m >= nT) continue;
#pragma unroll
      for (int c = 0; c < CB; c++) {
        if (cb + c >= a.C) continue;
        const double dm = (double)(m0 + m), r = a.r[cb + c];
        // frac(r m): the whole number next to the rounded product taken from the exact one inside one fused multiply-add
        // (written as the fma itself: a product minus its own rounding, plus that difference, is contracted into this
        // fma by the compiler and then counts the residual twice)
        const double fr = fma(r, dm, -rint(r * dm));
        double sn, cs;
        sincospi(2.0 * fr, &sn, &cs);
        const cf ps = cmake((float)cs, -(float)sn);
        const size_t o = (size_t)(cb + c) * a.carrierStride + (size_t)row * a.outStride + o0 + m;
        a.outX[o] = ddc_mul(ps, cmake(xr[k][c], xi[k][c]));
        a.outY[o] = ddc_mul(ps, cmake(yr[k][c], yi[k][c]));
      }
    }
  }
}

struct DdcTailArgs {
  const void *x, *y;
  uint64_t inStride;
  uint32_t nIn, nRows, nOut;
  int fmt;
  cf *hist;
  uint64_t *pos;
  uint32_t T;
};

// One workgroup of 256 threads.  The new history is the last T - 1 samples of (history, rows): every entry is read into
// registers, then a barrier, then written, so a call shorter than the history shifts it in place.
__global__ __launch_bounds__(256) void ddc_tail_kernel(DdcTailArgs t)
{
  const uint32_t H = t.T - 1;
  const int64_t total = (int64_t)t.nRows * t.nIn;
  DdcArgs a{};
  a.x = t.x; a.y = t.y; a.inStride = t.inStride; a.nIn = t.nIn; a.fmt = t.fmt; a.hist = t.hist; a.T = t.T;
  float4 v[(BLAH2HIP_MAX_DDC_TAPS + 255) / 256];
#pragma unroll
  for (int k = 0; k < (BLAH2HIP_MAX_DDC_TAPS + 255) / 256; k++) {
    const uint32_t e = threadIdx.x + k * 256;
    v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < H) { // stream sample total - H + e, counted from row 0's first
      const int64_t j = total - H + e;
      v[k] = j < 0 ? ddc_load(a, 0, j) : ddc_load(a, (uint32_t)(j / t.nIn), j % t.nIn);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < (BLAH2HIP_MAX_DDC_TAPS + 255) / 256; k++) {
    const uint32_t e = threadIdx.x + k * 256;
    if (e < H) {
      t.hist[e] = cmake(v[k].x, v[k].y);
      t.hist[H + e] = cmake(v[k].z, v[k].w);
    }
  }
  if (threadIdx.x == 0) *t.pos += (uint64_t)t.nRows * t.nOut;
}

__global__ __launch_bounds__(256) void ddc_reset_kernel(cf *hist, uint32_t n, uint64_t *pos, uint64_t first)
{
  for (uint32_t e = threadIdx.x; e < n; e += 256) hist[e] = cmake(0.f, 0.f);
  if (threadIdx.x == 0) *pos = first;
}

} // namespace blah2
