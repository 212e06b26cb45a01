// Device code of the clutter filter (clutter.hip): the FFT correlations, the reduction of their partials, the overlap-save
// FIR in its two forms, the direct fp64 correlations of short blocks and the long filters' plane kernels.  The Toeplitz
// solve's kernels are clutter_solve_kernels.hpp's.  Included by clutter.hip alone, which defines B2_SPLIT_BUTTERFLIES
// ahead of fft_wg.hpp (see there).
#pragma once

#include <hip/hip_runtime.h>

#include "clutter_handle.hpp"
#include "fft_wg.hpp"
#include "range_core.hpp"
#include "bufload.hpp"

#include <stdint.h>

namespace blah2 {
namespace clutter {

// WienerHopf.cpp:67: xs[i] = x[(i - delayMin) % N] with (i - delayMin) evaluated in
// uint32.  Without a division (i < N, |delayMin| < N):
//   delayMin <= 0: i + |delayMin| < 2N                     -> one conditional subtract
//   delayMin > 0 : i >= delayMin -> i - delayMin < N
//                  i <  delayMin -> the uint32 difference wraps to 2^32 + i - delayMin,
//                                   whose residue is (i + wrapC) mod N, wrapC = (2^32 - delayMin) mod N
// thresh = max(delayMin, 0), sub = delayMin as uint32, wrapC precomputed on the host.
struct XsMap {
  uint32_t N, thresh, sub, wrapC;
};
__device__ __forceinline__ uint32_t xs_index(uint32_t i, const XsMap &m)
{
  uint32_t j = (i >= m.thresh) ? i - m.sub : i + m.wrapC;
  return j >= m.N ? j - m.N : j;
}
inline XsMap xs_map(int32_t delayMin, uint32_t N)
{
  const uint32_t thresh = delayMin > 0 ? (uint32_t)delayMin : 0u;
  return {N, thresh, (uint32_t)delayMin, (uint32_t)(((1ull << 32) - (uint64_t)thresh) % N)};
}
// n < 2N -> n mod N
__device__ __forceinline__ uint32_t wrapN(uint32_t n, uint32_t N) { return n >= N ? n - N : n; }
// Sample n0 + m of a circular window of F samples, for any n0 + m < N + F.  A lag below nBins <= N pairs a sample below N
// with one below N + nBins - 1 <= 2N - 1, so what lies at 2N - 1 and beyond (only a CPI shorter than the transform has it)
// reaches no lag that is kept: it is clamped to an index inside the CPI, not reduced
__device__ __forceinline__ uint32_t wrapWin(uint32_t n, uint32_t N) { return wrapN(min(n, 2u * N - 1u), N); }

// XCD-aware walk over the segments of a CPI.  Neighbouring segments read overlapping windows (F samples
// for segLen = F - nBins + 1 new ones: 2x at nBins = F/2), and workgroups are dispatched round-robin
// over the 8 XCDs, each with its own L2: with the natural map (workgroup b takes segments b, b + G, ...)
// the two readers of a shared half-window sit on different XCDs and both fetch it from HBM (measured,
// profiles/r02_cfg3_full: 10.3 GB fetched for 5.1 GB of input).  Here every XCD owns one contiguous
// eighth of the segments, and in each round its G/8 workgroups take G/8 CONSECUTIVE segments, so the
// overlaps are served by that XCD's L2.  gridDim.x must be a multiple of 8.
struct SegWalk {
  int base, step, first, count; // segments base + first + k*step, while first + k*step < count
};
__device__ __forceinline__ SegWalk seg_walk(int nSeg)
{
  const int xcd = blockIdx.x & 7, l = blockIdx.x >> 3, gx = gridDim.x >> 3;
  const int s8 = (nSeg + 7) >> 3;
  SegWalk w;
  w.base = xcd * s8;
  w.step = gx;
  w.first = l;
  w.count = min(s8, nSeg - w.base); // may be <= 0 for the last XCDs of a short CPI
  return w;
}

// In: InC32 (two complex fp32 planes) or InI16 (the .rspduo words, range_core.hpp); in.lx / in.ly read sample i of
// the reference / surveillance channel
// One channel of a CPI as something indexable by sample: a plain `const cf *` for the fp32 planes (the kernels are then
// token for token what they were: the correlation kernels sit at the 256-register cap, and reaching the same loads through
// an accessor object made the register allocator spill 34 values in the inner loop), a converting view for the .rspduo words.
struct I16Chan {
  const int16_t *p; // first int16 of this channel's (I, Q) pair in sample 0
  __device__ __forceinline__ cf operator[](uint32_t i) const
  {
    const uint32_t w = *reinterpret_cast<const uint32_t *>(p + 4 * (size_t)i); // (I, Q) as one 4-byte load
    return cmake((float)(int16_t)(w & 0xffffu), (float)(int16_t)(w >> 16));
  }
};
struct I8Chan { // a plane of int8 (I, Q) pairs (range_core.hpp InI8)
  const int8_t *p;
  __device__ __forceinline__ cf operator[](uint32_t i) const
  {
    const uint32_t w = *reinterpret_cast<const uint16_t *>(p + 2 * (size_t)i); // (I, Q) as one 2-byte load
    return cmake((float)(int8_t)(w & 0xffu), (float)(int8_t)(w >> 8));
  }
};
template <class In> struct ChanOf;
template <> struct ChanOf<InC32> {
  using type = const cf *;
  static __device__ __forceinline__ type x(const void *px, const void *, int64_t i) { return (const cf *)px + i; }
  static __device__ __forceinline__ type y(const void *, const void *py, int64_t i) { return (const cf *)py + i; }
};
template <> struct ChanOf<InI16> {
  using type = I16Chan;
  static __device__ __forceinline__ type x(const void *px, const void *, int64_t i) { return I16Chan{(const int16_t *)px + 4 * i}; }
  static __device__ __forceinline__ type y(const void *px, const void *, int64_t i) { return I16Chan{(const int16_t *)px + 4 * i + 2}; }
};
template <> struct ChanOf<InI8> {
  using type = I8Chan;
  static __device__ __forceinline__ type x(const void *px, const void *, int64_t i) { return I8Chan{(const int8_t *)px + 2 * i}; }
  static __device__ __forceinline__ type y(const void *, const void *py, int64_t i) { return I8Chan{(const int8_t *)py + 2 * i}; }
};

// one channel of a CPI as the raw-buffer channel type of bufload.hpp (sample stride, raw word, conversion)
template <class In> struct BufChanOf;
template <> struct BufChanOf<InC32> {
  using X = ChanC32;
  using Y = ChanC32;
  static __device__ __forceinline__ const void *x(const void *px, const void *, int64_t i) { return (const cf *)px + i; }
  static __device__ __forceinline__ const void *y(const void *, const void *py, int64_t i) { return (const cf *)py + i; }
};
template <> struct BufChanOf<InI16> {
  using X = ChanI16;
  using Y = ChanI16;
  static __device__ __forceinline__ const void *x(const void *px, const void *, int64_t i) { return (const int16_t *)px + 4 * i; }
  static __device__ __forceinline__ const void *y(const void *px, const void *, int64_t i) { return (const int16_t *)px + 4 * i + 2; }
};
template <> struct BufChanOf<InI8> {
  using X = ChanI8;
  using Y = ChanI8;
  static __device__ __forceinline__ const void *x(const void *px, const void *, int64_t i) { return (const int8_t *)px + 2 * i; }
  static __device__ __forceinline__ const void *y(const void *, const void *py, int64_t i) { return (const int8_t *)py + 2 * i; }
};
// Does the window [src0, src0 + F) of the shifted reference channel map to ONE contiguous run of x, and where does it
// start?  xs_index is i - sub from `thresh` on (then mod N): contiguous unless the window starts before `thresh` (or
// before sample 0) or runs over the end of the CPI, which only the first and last windows of a CPI do.  *cnt = the samples
// of the window that exist (src < N); the rest is zero padding.
__device__ __forceinline__ bool xs_window_plain(int src0, int F, const XsMap &m, uint32_t *j0, int *cnt)
{
  const int64_t left = (int64_t)m.N - src0;
  *cnt = (int)(left < F ? (left < 0 ? 0 : left) : F);
  *j0 = (uint32_t)src0 - m.sub;
  return src0 >= 0 && (uint32_t)src0 >= m.thresh && (uint64_t)*j0 + (uint32_t)*cnt <= m.N;
}

// ---- the FFT correlations: one kernel pair for one channel and for several against ONE reference -------------------------
// r = xs against xs belongs to the reference alone, and so does the spectrum every b_k is formed against.  Both kernels
// carry the surveillance channel as a compile-time tile:
//   WITH_R, NB = 1: r and b_0 of (x, y_0).  The per-channel call (launch_clutter: rows = 2, row0 = 1, the layout
//     [nCpi][2][nJobs][nBins]) and the first pass of blah2hip_clutter_process_multi_dev_fmt are this one instantiation
//     (half-window: two, see PAIR there);
//   !WITH_R, NB = 1 | 2: the channels behind the first, one or two per pass: the reference's spectrum once more (one
//     transform per segment), then one window transform and accB_c += Y_c conj(.) per channel.  No xs window transform and
//     no r accumulation: their registers hold the second channel, so no instantiation needs more than the first pass.
// Per channel the segment walk, the job count and the order of the accumulation are the first pass's: r and every b_k are
// the bits of the per-channel call.  Transforms per segment for K channels: windowed 3 + (K - 1) + ceil((K - 1) / 2)
// against 3K, half-window 2 + (K - 1) + ceil((K - 1) / 2) against 2K.
constexpr int CORR_TILE = 2;
struct CorrArgs {
  const void *x;  // InC32, InI8: the reference plane; InI16: the interleaved buffer (the y planes are not read)
  const void *y0; // this pass's first surveillance plane
  int64_t cpiStride;
  uint32_t N;
  XsMap xs;
  int32_t nBins;
  union { // the form's segmentation in one place
    struct { int32_t segLen, nSeg; } win; // windowed: the plan's segments
    struct { int32_t nSeg, per; } half;   // half-window: nSeg = ceil(N / (F/2)), per = segments per workgroup
  };
  int32_t nJobs;
  const cf *tw;
  cf *partial;        // [nCpi][rows][nJobs][nBins]: row 0 = r, row 1 + k = b_k
  float scale;
  // KEEP x ... scale where they are and add new fields behind `scale`: these are the offsets the single-channel kernels'
  // arguments had.  With the planes as an array in front and both forms' fields side by side, 9 of 15 timed cases of the
  // <true, 1> kernels were 0.1 ... 1.4 % slower, their vector code unchanged (mechanism not known)
  int32_t rows;       // rows of `partial` per CPI
  const void *y1;     // the pass's second plane (NB = 2)
  int32_t row0;       // the row of y0's b
  __device__ __forceinline__ const void *y(int c) const { return c ? y1 : y0; } // c is a constant after unrolling
};

// the end of both kernels: inverse transform of one accumulator, its first nBins lags into the workgroup's row of the partials
// (one call per accumulator: a runtime-selected register array would be demoted to scratch)
template <int R3> __device__ __forceinline__ void corr_finish(const CorrArgs &a, int t, cf *acc, int rows, int row, const cf *tw1, const cf *tw3, cf *P, cf *Q)
{
  using W = WgFft<R3>;
  W::inv_s1(t, acc, tw3, P);
  __syncthreads();
  W::inv_s2(t, acc, P, Q);
  __syncthreads();
  W::inv_s3(t, acc, tw1, Q);
  const int cpi = blockIdx.y;
  cf *dst = a.partial + (((size_t)cpi * rows + row) * a.nJobs + blockIdx.x) * a.nBins;
#pragma unroll
  for (int c = 0; c < 16; c++) {
    const int k = t + W::T * c;
    if (k < a.nBins) dst[k] = cmake(acc[c].x * a.scale, acc[c].y * a.scale);
  }
  __syncthreads();
}

// grid (nJobs, nCpi): per segment FFT(x' = zero-padded xs segment) ONCE, then the
// xs window (-> r) and the y windows (-> b_c) against it; the partial correlations
// accumulate in registers across the workgroup's segments.
// (F = 4096: built for ONE workgroup of 256 threads per SIMD set -- 257 registers are what the three live windows, two
// accumulators and two twiddle sets need there, and at the two-workgroup cap of 256 one value went to scratch in every
// build of rounds 2-5.  With r that instantiation only runs for filters of 2050 ... 4081 taps: the half-window form takes the rest.)
template <int R3, class In, bool WITH_R, int NB>
__global__ __launch_bounds__(16 * R3, R3 == 16 ? 1 : 2) void clutter_corr_kernel(CorrArgs a)
{
  static_assert(NB >= 1 && NB <= CORR_TILE && (!WITH_R || NB == 1), "r rides with the first channel alone");
  using W = WgFft<R3>;
  constexpr int T = W::T;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cf *P = reinterpret_cast<cf *>(smem);
  cf *Q = P + W::A_ELEMS;
  const int t = threadIdx.x;
  const int cpi = blockIdx.y;
  const typename ChanOf<In>::type X = ChanOf<In>::x(a.x, nullptr, (int64_t)cpi * a.cpiStride);
  cf tw1[15], tw3[16];
  W::load_twiddles(t, a.tw, tw1, tw3);

  cf accR[16], accB[NB][16];
#pragma unroll
  for (int e = 0; e < 16; e++) {
    accR[e] = cmake(0.f, 0.f);
#pragma unroll
    for (int c = 0; c < NB; c++) accB[c][e] = cmake(0.f, 0.f);
  }
  const SegWalk sw = seg_walk(a.win.nSeg);
  for (int r = sw.first; r < sw.count; r += sw.step) {
    const int g = sw.base + r;
    const uint32_t n0 = (uint32_t)g * (uint32_t)a.win.segLen;
    cf v[16], wv[16], yw[NB][16];
    uint32_t j0;
    int xcnt;
    const bool whole = (uint64_t)n0 + 16 * T <= a.N; // the window does not run around the end of the CPI
    const bool plain = whole && xs_window_plain((int)n0, 16 * T, a.xs, &j0, &xcnt); // all but a CPI's first and last windows: immediates only
    auto load_y = [&](int c) { // c is a constant after unrolling
      if (plain) {
        using CY = typename BufChanOf<In>::Y;
        const __amdgpu_buffer_rsrc_t yd = make_rsrc_b(BufChanOf<In>::y(a.x, a.y(c), (int64_t)cpi * a.cpiStride + n0), 16 * T * CY::STRIDE);
#pragma unroll
        for (int k = 0; k < 16; k++) yw[c][k] = RawBuiltin<CY>::cvt(RawBuiltin<CY>::ld(yd, (t + T * k) * CY::STRIDE, 0));
      } else {
        const typename ChanOf<In>::type Y = ChanOf<In>::y(a.x, a.y(c), (int64_t)cpi * a.cpiStride);
#pragma unroll
        for (int k = 0; k < 16; k++) yw[c][k] = Y[wrapWin(n0 + (uint32_t)(t + T * k), a.N)];
      }
    };
    if (plain) {
      using CX = typename BufChanOf<In>::X;
      const __amdgpu_buffer_rsrc_t xd = make_rsrc_b(BufChanOf<In>::x(a.x, nullptr, (int64_t)cpi * a.cpiStride + j0), 16 * T * CX::STRIDE);
#pragma unroll
      for (int k = 0; k < 16; k++) wv[k] = RawBuiltin<CX>::cvt(RawBuiltin<CX>::ld(xd, (t + T * k) * CX::STRIDE, 0));
    } else {
#pragma unroll
      for (int k = 0; k < 16; k++) wv[k] = X[xs_index(wrapWin(n0 + (uint32_t)(t + T * k), a.N), a.xs)];
    }
    // all the loads of the segment first (the y window is consumed last) -- except at F = 4096 with r, where the kernel sits
    // at the 256-register cap: there the y window is requested inside the second transform (its 32 registers are free until
    // then), which removed the one spilled register (8 bytes of scratch per lane) of rounds 2-5
    if (!WITH_R || R3 < 16) load_y(0);
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int m = t + T * k;
      v[k] = (m < a.win.segLen && n0 + (uint32_t)m < a.N) ? wv[k] : cmake(0.f, 0.f); // x' = the same samples, cut to the segment
    }
    W::fwd_s1(t, v, tw1, P);
    __syncthreads();
    W::fwd_s2(t, v, P, Q);
    __syncthreads();
    W::fwd_s3(t, v, tw3, Q); // v = X' spectrum
    if (WITH_R) {
      W::fwd_s1(t, wv, tw1, P);
      __syncthreads();
      W::fwd_s2(t, wv, P, Q);
      if (R3 == 16) load_y(0); // behind the second transform's last exchange write: wv's 32 registers are about to be consumed
      __syncthreads();
      W::fwd_s3(t, wv, tw3, Q);
#pragma unroll
      for (int e = 0; e < 16; e++) accR[e] = cmacc(accR[e], wv[e], v[e]);
    }
#pragma unroll
    for (int c = 0; c < NB; c++) {
      W::fwd_s1(t, yw[c], tw1, P);
      __syncthreads();
      W::fwd_s2(t, yw[c], P, Q);
      if (c + 1 < NB) load_y(c + 1); // the next channel's window behind this transform's last exchange write: five register sets, as with r
      __syncthreads();
      W::fwd_s3(t, yw[c], tw3, Q);
#pragma unroll
      for (int e = 0; e < 16; e++) accB[c][e] = cmacc(accB[c][e], yw[c][e], v[e]);
    }
    __syncthreads();
  }
  if (WITH_R) corr_finish<R3>(a, t, accR, a.rows, 0, tw1, tw3, P, Q);
  corr_finish<R3>(a, t, accB[0], a.rows, a.row0, tw1, tw3, P, Q);
  if (NB > 1) corr_finish<R3>(a, t, accB[NB - 1], a.rows, a.row0 + 1, tw1, tw3, P, Q);
}

// Half-window form of the same correlations, for filters with many taps (nBins - 1 <= F/2): cut the
// CPI into segments of exactly L = F/2 samples; with X_g, Y_g the transforms of the zero-padded
// segments, the window [segment g, segment g+1] has the spectrum X_g + (-1)^m X_{g+1} (a shift by F/2
// samples is the sign of the frequency index), so -- grouping every pair (n, n+k) by the segment that
// holds its LATER sample --
//     r = sum_g X_g conj(X_g + (-1)^m X_{g-1}),      b = sum_g Y_g conj(X_g + (-1)^m X_{g-1}):
// TWO transforms per L samples instead of three per F - nBins + 1, every sample read once, and only
// the previous segment's X to keep (the register budget of the windowed form).  A workgroup walks a
// contiguous run of segments (one extra transform for the segment in front of its run).  The
// sequence is treated as zero-extended to a whole number of segments; what that leaves out of the
// CIRCULAR correlations over N -- the pairs whose later sample wraps to the head of the CPI -- is one
// more product, tail (last nBins-1 samples of xs) against head (first nBins-1 of xs / y) shifted by
// tau = nBins - 1, i.e. times W_F^(tau m), done by the last workgroup.  Mathematically identical.
// In the passes without r, z = X_g + (-1)^m X_{g-1} takes the previous segment's registers as soon as it is formed, and the
// channels' transforms follow one after the other against it: five register sets at NB = 2, the count of the pass with r.
// (F = 4096 with two channels: built for ONE workgroup per SIMD set, like the windowed kernel -- at the 256-register cap
// of two the allocator put 1 value of the segment loop and 62 of the wrap-around product into scratch.)
// PAIR: the per-channel call's instantiation, its partials [nCpi][2][nJobs][nBins] known at compile time (rows = 2, row0 = 1).
// With the rows as run-time arguments this kernel's vector code was the same and the launch 0.5 ... 1.8 % slower at F = 2048 on
// int8 planes (every one of 6 legs above every one of 18); with PAIR nothing is left that differs from what was measured fast.
template <int R3, class In, bool WITH_R, int NB, bool PAIR = false>
__global__ __launch_bounds__(16 * R3, (R3 == 16 && NB == 2) ? 1 : 2) void clutter_corr_half_kernel(CorrArgs a)
{
  static_assert(NB >= 1 && NB <= CORR_TILE && (!WITH_R || NB == 1), "r rides with the first channel alone");
  static_assert(!PAIR || WITH_R, "the pair of rows is r and b");
  using W = WgFft<R3>;
  constexpr int T = W::T, L = W::F / 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cf *P = reinterpret_cast<cf *>(smem);
  cf *Q = P + W::A_ELEMS;
  const int t = threadIdx.x;
  const int cpi = blockIdx.y;
  const typename ChanOf<In>::type X = ChanOf<In>::x(a.x, nullptr, (int64_t)cpi * a.cpiStride);
  cf tw1[15], tw3[16];
  W::load_twiddles(t, a.tw, tw1, tw3);
  // (-1)^m for this thread's spectrum registers: m = q + 16 r + 256 s with q = (t + T j) / 16 and T a
  // multiple of 32, so the parity of m is that of t / 16
  const float sgn = ((t >> 4) & 1) ? -1.f : 1.f;

  auto fwd = [&](cf *v) {
    W::fwd_s1(t, v, tw1, P);
    __syncthreads();
    W::fwd_s2(t, v, P, Q);
    __syncthreads();
    W::fwd_s3(t, v, tw3, Q);
    __syncthreads();
  };
  // first L samples of a zero-padded window starting at sample n0 of xs / of y (zero beyond N)
  // Through buffer descriptors over exactly the `len` samples: the range check is the zero padding.  xs is read that
  // way where the stretch maps to one contiguous run of x (xs_window_plain: everywhere but at a CPI's ends).
  using CX = typename BufChanOf<In>::X;
  using CY = typename BufChanOf<In>::Y;
  auto load_xs = [&](uint32_t n0, uint32_t len, cf *v) {
    uint32_t j0;
    int cnt;
    if (xs_window_plain((int)n0, (int)len, a.xs, &j0, &cnt) && cnt == (int)len) {
      const __amdgpu_buffer_rsrc_t d = make_rsrc_b(BufChanOf<In>::x(a.x, nullptr, (int64_t)cpi * a.cpiStride + j0), (int)len * CX::STRIDE);
#pragma unroll
      for (int k = 0; k < 8; k++) v[k] = RawBuiltin<CX>::cvt(RawBuiltin<CX>::ld(d, (t + T * k) * CX::STRIDE, 0));
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const uint32_t m = (uint32_t)(t + T * k);
        const bool inr = m < len;
        const cf s = X[xs_index(inr ? n0 + m : 0u, a.xs)];
        v[k] = inr ? s : cmake(0.f, 0.f);
      }
    }
#pragma unroll
    for (int k = 8; k < 16; k++) v[k] = cmake(0.f, 0.f);
  };
  auto load_y = [&](int c, uint32_t n0, uint32_t len, cf *v) {
    const __amdgpu_buffer_rsrc_t d = make_rsrc_b(BufChanOf<In>::y(a.x, a.y(c), (int64_t)cpi * a.cpiStride + n0), (int)len * CY::STRIDE);
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = RawBuiltin<CY>::cvt(RawBuiltin<CY>::ld(d, (t + T * k) * CY::STRIDE, 0));
#pragma unroll
    for (int k = 8; k < 16; k++) v[k] = cmake(0.f, 0.f);
  };
  auto seg_len = [&](int g) { return min((uint32_t)L, a.N - (uint32_t)g * (uint32_t)L); };

  cf accR[16], accB[NB][16], prevX[16];
#pragma unroll
  for (int e = 0; e < 16; e++) {
    accR[e] = cmake(0.f, 0.f);
    prevX[e] = cmake(0.f, 0.f);
#pragma unroll
    for (int c = 0; c < NB; c++) accB[c][e] = cmake(0.f, 0.f);
  }
  const int g0 = blockIdx.x * a.half.per, g1 = min(g0 + a.half.per, a.half.nSeg);
  if (g0 > 0 && g0 < g1) { // the segment in front of the run (a full one)
    load_xs((uint32_t)(g0 - 1) * (uint32_t)L, (uint32_t)L, prevX);
    fwd(prevX);
  }
  for (int g = g0; g < g1; g++) {
    const uint32_t n0 = (uint32_t)g * (uint32_t)L, len = seg_len(g);
    cf v[16], yv[16];
    load_xs(n0, len, v);
    if (WITH_R) load_y(0, n0, len, yv); // with the xs segment: both requests in front of the first transform
    fwd(v);
    if constexpr (WITH_R) {
      // both transforms, then ONE pass over the registers: z never leaves its register pair and X_g takes X_{g-1}'s place
      // as it is consumed
      fwd(yv);
#pragma unroll
      for (int e = 0; e < 16; e++) {
        const cf z = cmake(v[e].x + sgn * prevX[e].x, v[e].y + sgn * prevX[e].y); // X_g + (-1)^m X_{g-1}
        accR[e] = cmacc(accR[e], v[e], z);
        accB[0][e] = cmacc(accB[0][e], yv[e], z);
        prevX[e] = v[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 16; e++) prevX[e] = cmake(v[e].x + sgn * prevX[e].x, v[e].y + sgn * prevX[e].y); // z, kept for every channel
#pragma unroll
      for (int c = 0; c < NB; c++) {
        load_y(c, n0, len, yv);
        fwd(yv);
#pragma unroll
        for (int e = 0; e < 16; e++) accB[c][e] = cmacc(accB[c][e], yv[e], prevX[e]);
      }
#pragma unroll
      for (int e = 0; e < 16; e++) prevX[e] = v[e];
    }
  }
  if (blockIdx.x == (unsigned)a.nJobs - 1 && a.nBins > 1) { // the wrap-around pairs
    const uint32_t tau = (uint32_t)a.nBins - 1;
    cf v[16], yv[16];
    load_xs(a.N - tau, tau, prevX); // tail of xs
    if (WITH_R) { // all three requests in front of the transforms: this workgroup ends the launch
      load_xs(0u, tau, v);    // head of xs
      load_y(0, 0u, tau, yv); // head of y
    }
    fwd(prevX);
    if (WITH_R) {
      fwd(v);
      fwd(yv);
    }
#pragma unroll
    for (int j = 0; j < W::NP; j++)
#pragma unroll
      for (int sidx = 0; sidx < R3; sidx++) {
        const int e = j * R3 + sidx;
        const int p16 = t + T * j;                         // 16 q + r
        const int m = (p16 >> 4) + 16 * (p16 & 15) + 256 * sidx;
        const cf ph = a.tw[((uint32_t)m * tau) & (W::F - 1)]; // W_F^(tau m): the head sits tau samples behind the tail
        const cf z = cmulc(prevX[e], ph);                  // conj(phase) * X_tail
        if constexpr (WITH_R) {
          accR[e] = cmacc(accR[e], v[e], z);
          accB[0][e] = cmacc(accB[0][e], yv[e], z);
        } else {
          prevX[e] = z; // kept for every channel
        }
      }
    if constexpr (!WITH_R) {
#pragma unroll
      for (int c = 0; c < NB; c++) {
        load_y(c, 0u, tau, yv); // head of y
        fwd(yv);
#pragma unroll
        for (int e = 0; e < 16; e++) accB[c][e] = cmacc(accB[c][e], yv[e], prevX[e]);
      }
    }
  }
  const int rows = PAIR ? 2 : a.rows, row0 = PAIR ? 1 : a.row0;
  if (WITH_R) corr_finish<R3>(a, t, accR, rows, 0, tw1, tw3, P, Q);
  corr_finish<R3>(a, t, accB[0], rows, row0, tw1, tw3, P, Q);
  if (NB > 1) corr_finish<R3>(a, t, accB[NB - 1], rows, row0 + 1, tw1, tw3, P, Q);
}

// grid (ceil(nBins/16), 2, nCpi) x 1024: fixed-order fp64 sum over the jobs.  A block takes 16 bins (128-byte rows) and cuts the
// jobs into 64 interleaved slices (thread = bin + 16 slice): a lone CPI has up to 512 partials per bin, which one thread per bin
// summed as 64 dependent rounds of L2 latency (27.8 us of the 171 us a lone CPI's full chain took at configs[1], round 4);
// the slices' sums meet in LDS and are added in slice order -- the same order every run.
constexpr int RED_SLICES = 64; // 1024 threads: a lone CPI's 512 partials per bin are 4 dependent rounds of 2 loads per thread (16 slices: 16 rounds, 9.8 us)
__global__ __launch_bounds__(16 * RED_SLICES) void clutter_reduce_kernel(SolveArgs a)
{
  __shared__ double sx[RED_SLICES][16], sy[RED_SLICES][16];
  const int bin = threadIdx.x & 15, slice = threadIdx.x >> 4;
  const int k = blockIdx.x * 16 + bin, mode = blockIdx.y, cpi = blockIdx.z;
  if (a.epoch && blockIdx.x == 0 && threadIdx.x == 0 && mode == 0 && cpi == 0) { // one thread per launch; the solve kernel behind the boundary reads it
    const uint32_t e = *a.epoch + 1u;
    *a.epoch = e ? e : 1u;
  }
  double ax = 0.0, ay = 0.0;
  if (k < a.nBins) {
    const cf *p = a.partial + ((size_t)cpi * 2 + mode) * a.nJobs * a.nBins + k;
    // two interleaved accumulators: the loads of a pair of rounds are independent
    double bx = 0.0, by = 0.0;
    int j = slice;
    for (; j + RED_SLICES < a.nJobs; j += 2 * RED_SLICES) {
      const cf u = p[(size_t)j * a.nBins], v = p[(size_t)(j + RED_SLICES) * a.nBins];
      ax += (double)u.x; ay += (double)u.y;
      bx += (double)v.x; by += (double)v.y;
    }
    if (j < a.nJobs) { const cf u = p[(size_t)j * a.nBins]; ax += (double)u.x; ay += (double)u.y; }
    ax += bx; ay += by;
  }
  sx[slice][bin] = ax;
  sy[slice][bin] = ay;
  __syncthreads();
  if (slice == 0 && k < a.nBins) {
    double tx = sx[0][bin], ty = sy[0][bin];
#pragma unroll 8
    for (int q = 1; q < RED_SLICES; q++) { tx += sx[q][bin]; ty += sy[q][bin]; } // in slice order: the same sum every run
    a.rb[((size_t)cpi * 2 + mode) * a.nBins + k] = {tx, ty};
  }
}

// ---- overlap-save FIR: y_out = y - (w * xs)[0..N) ----------------------------
struct FirArgs {
  const void *x, *y;
  cf *yout;
  int64_t cpiStride, outStride;
  uint32_t N;
  XsMap xs;
  int32_t nBins, segLen, nSeg;
  const cf *w;       // [nCpi][nBins]
  const int32_t *ok; // [nCpi]
  const cf *tw;
  float scale;
  int32_t carry;     // segLen = F/2: the upper half of a block's x window is the lower half of the next block's (see the kernel)
};

// SKIP_BAD (blah2hip_clutter_process_multi_dev_fmt): a CPI whose matrix is not positive definite is left unwritten
// instead of passed through -- the workgroup leaves before it reads a sample
template <int R3, class In, bool SKIP_BAD = false> __global__ __launch_bounds__(16 * R3, 2) void clutter_fir_kernel(FirArgs a)
{
  using W = WgFft<R3>;
  constexpr int T = W::T;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cf *P = reinterpret_cast<cf *>(smem);
  cf *Q = P + W::A_ELEMS;
  const int t = threadIdx.x;
  const int cpi = blockIdx.y;
  const typename ChanOf<In>::type X = ChanOf<In>::x(a.x, a.y, (int64_t)cpi * a.cpiStride);
  const typename ChanOf<In>::type Y = ChanOf<In>::y(a.x, a.y, (int64_t)cpi * a.cpiStride);
  cf *O = a.yout + (int64_t)cpi * a.outStride;
  const bool ok = a.ok[cpi] != 0;
  if (SKIP_BAD && !ok) return; // uniform: one flag per CPI
  cf tw1[15], tw3[16];
  W::load_twiddles(t, a.tw, tw1, tw3);

  // spectrum of the taps (zero-padded to F), pre-scaled by 1/F, kept in registers -- all but the LARGEST tap, which is applied
  // in the time domain (below): with a direct path 58 dB above the noise, w * xs is a thousand times what is left of y, and
  // the transform's rounding of that one product (3.5 eps of it, incoherent) was the map's largest error behind a deep
  // cancellation (fixture deep_cancel: 0.0063 dB on a cell 19 dB under the mean level); one fma rounds it once
  cf ws[16];
  float bestMag = -1.f;
  int bestIdx = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int m = t + T * k;
    const cf wv = a.w[(size_t)cpi * a.nBins + min(m, a.nBins - 1)];
    const float keep = (m < a.nBins) ? a.scale : 0.f; // branch-free: the 16 loads go out together
    ws[k] = cmake(wv.x * keep, wv.y * keep);
    const float mag = (m < a.nBins) ? wv.x * wv.x + wv.y * wv.y : -1.f;
    if (mag > bestMag) { bestMag = mag; bestIdx = m; } // (ascending m: ties go to the lower index)
  }
  { // the workgroup's argmax: a butterfly over the lanes, then the waves' winners through the exchange buffer (free here); ties go
    // to the lower index, so every workgroup of the CPI picks the same tap
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float mu = __shfl_xor(bestMag, off);
      const int iu = __shfl_xor(bestIdx, off);
      if (mu > bestMag || (mu == bestMag && iu < bestIdx)) { bestMag = mu; bestIdx = iu; }
    }
    if (T > 64) {
      float *sm = reinterpret_cast<float *>(P);
      int *si = reinterpret_cast<int *>(P) + T / 64;
      if ((t & 63) == 0) { sm[t >> 6] = bestMag; si[t >> 6] = bestIdx; }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < T / 64; u++) {
        const float mu = sm[u];
        const int iu = si[u];
        if (mu > bestMag || (mu == bestMag && iu < bestIdx)) { bestMag = mu; bestIdx = iu; }
      }
      __syncthreads();
    }
  }
  const int k0 = bestIdx;
  const cf w0 = a.w[(size_t)cpi * a.nBins + k0];
#pragma unroll
  for (int k = 0; k < 16; k++)
    if (t + T * k == k0) ws[k] = cmake(0.f, 0.f);
  W::fwd_s1(t, ws, tw1, P);
  __syncthreads();
  W::fwd_s2(t, ws, P, Q);
  __syncthreads();
  W::fwd_s3(t, ws, tw3, Q);
  __syncthreads();

  const int hist = a.nBins - 1; // samples of history in front of each block
  const int N = (int)a.N;       // < 2^31 - 8192 (checked at create): 32-bit sample indices throughout
  // CARRY (a.carry, filters with nBins - 1 close below F/2, i.e. cfg 3's 2047 taps on F = 4096): the planner makes the blocks
  // exactly F/2 = 8 T samples long, a workgroup walks CONSECUTIVE blocks, and the upper half of a block's window
  // [n0 - hist, n0 - hist + F) is the lower half of the next block's, register for register (x'[t + T (k + 8)] -> x'[t + T k]):
  // eight loads per thread and block instead of sixteen, and x is read once.  (With blocks of F - hist samples every
  // sample of x was requested twice, and 43 % of the second requests went to HBM: 1.145 x the algorithmic bytes.)  It is a traffic
  // measure, not a speed-up: the kernel's time did not move (58.0 against 57.7 us/CPI at cfg 3) -- what bounds it is the
  // barrier-separated phases of two workgroups per CU, not the loads.  Otherwise: the XCD-aware strided walk, whole windows.
  const SegWalk sw = seg_walk(a.nSeg);
  int rFirst = sw.first, rStep = sw.step, rEnd = sw.count;
  if (a.carry) { // this workgroup's contiguous run inside its XCD's eighth
    const int per = (max(sw.count, 0) + sw.step - 1) / sw.step;
    rFirst = sw.first * per;
    rEnd = min(rFirst + per, sw.count);
    rStep = 1;
  }
  cf keep[8];
  bool have = false;
  // eight values v[k0 .. k0 + 7] of the window that starts at sample src0 of xs: x'[src0 + t + T k], zero outside [0, N)
  auto load_half = [&](cf *dst, int src0) {
    uint32_t j0;
    int xcnt;
    if (xs_window_plain(src0, 8 * T, a.xs, &j0, &xcnt)) {
      using CX = typename BufChanOf<In>::X;
      const __amdgpu_buffer_rsrc_t xd = make_rsrc_b(BufChanOf<In>::x(a.x, a.y, (int64_t)cpi * a.cpiStride + j0), xcnt * CX::STRIDE);
#pragma unroll
      for (int k = 0; k < 8; k++) dst[k] = RawBuiltin<CX>::cvt(RawBuiltin<CX>::ld(xd, (t + T * k) * CX::STRIDE, 0));
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int src = src0 + t + T * k;
        const bool inr = src >= 0 && src < N;
        const cf xv = X[xs_index(inr ? (uint32_t)src : 0u, a.xs)];
        dst[k] = inr ? xv : cmake(0.f, 0.f);
      }
    }
  };
  for (int r = rFirst; r < rEnd; r += rStep) {
    const int g = sw.base + r;
    const int n0 = g * a.segLen;
    cf v[16], yv[16];
    uint32_t j0;
    int xcnt;
    if (a.carry) {
      if (have) {
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = keep[k];
      } else {
        load_half(v, n0 - hist);
      }
      load_half(v + 8, n0 - hist + 8 * T);
#pragma unroll
      for (int k = 0; k < 8; k++) keep[k] = v[8 + k];
      have = true;
      // (requesting the NEXT block's new half here, into eight more registers, so that it lands during this block's two
      // transforms, measured 60.8 against 58.0 us/CPI at cfg 3: not adopted)
    } else if (xs_window_plain(n0 - hist, 16 * T, a.xs, &j0, &xcnt)) { // all but the first and last windows of a CPI
      using CX = typename BufChanOf<In>::X;
      const __amdgpu_buffer_rsrc_t xd = make_rsrc_b(BufChanOf<In>::x(a.x, a.y, (int64_t)cpi * a.cpiStride + j0), xcnt * CX::STRIDE);
#pragma unroll
      for (int k = 0; k < 16; k++) v[k] = RawBuiltin<CX>::cvt(RawBuiltin<CX>::ld(xd, (t + T * k) * CX::STRIDE, 0));
    } else {
#pragma unroll
      for (int k = 0; k < 16; k++) {
        const int m = t + T * k;
        const int src = n0 - hist + m;
        const bool inr = src >= 0 && src < N;
        const cf xv = X[xs_index(inr ? (uint32_t)src : 0u, a.xs)];
        v[k] = inr ? xv : cmake(0.f, 0.f);
      }
    }
    // y of the output samples, and later the stores: descriptors over exactly this block's new samples [n0, n0 + min(segLen,
    // N - n0)), register k at offset m - hist -- history rows (negative) and rows beyond the block are outside the range, so
    // the loads return zeros that are never stored and the stores are dropped: no predicate, no branch per element
    const int cnt = min(a.segLen, N - n0);
    using CY = typename BufChanOf<In>::Y;
    const __amdgpu_buffer_rsrc_t yd = make_rsrc_b(BufChanOf<In>::y(a.x, a.y, (int64_t)cpi * a.cpiStride + n0), cnt * CY::STRIDE);
    const __amdgpu_buffer_rsrc_t od = make_rsrc_b(O + n0, cnt * 8);
#pragma unroll
    for (int k = 0; k < 16; k++) yv[k] = RawBuiltin<CY>::cvt(RawBuiltin<CY>::ld(yd, (t + T * k - hist) * CY::STRIDE, 0));
    cf xdir[16]; // the window k0 samples earlier: register c holds xs[n - k0] of the output sample n that register c writes
    if (ok) {
      W::fwd_s1(t, v, tw1, P);
      __syncthreads();
      W::fwd_s2(t, v, P, Q);
      __syncthreads();
      W::fwd_s3(t, v, tw3, Q);
#pragma unroll
      for (int e = 0; e < 16; e++) v[e] = cmul(v[e], ws[e]);
      // (requested here: the samples arrive during the inverse transform; most of their lines are in L2 from the window above)
      if (xs_window_plain(n0 - hist - k0, 16 * T, a.xs, &j0, &xcnt)) {
        using CX = typename BufChanOf<In>::X;
        const __amdgpu_buffer_rsrc_t xd = make_rsrc_b(BufChanOf<In>::x(a.x, a.y, (int64_t)cpi * a.cpiStride + j0), xcnt * CX::STRIDE);
#pragma unroll
        for (int k = 0; k < 16; k++) xdir[k] = RawBuiltin<CX>::cvt(RawBuiltin<CX>::ld(xd, (t + T * k) * CX::STRIDE, 0));
      } else {
#pragma unroll
        for (int k = 0; k < 16; k++) {
          const int src = n0 - hist - k0 + t + T * k;
          const bool inr = src >= 0 && src < N;
          const cf xv = X[xs_index(inr ? (uint32_t)src : 0u, a.xs)];
          xdir[k] = inr ? xv : cmake(0.f, 0.f);
        }
      }
      __syncthreads();
      W::inv_s1(t, v, tw3, P);
      __syncthreads();
      W::inv_s2(t, v, P, Q);
      __syncthreads();
      W::inv_s3(t, v, tw1, Q);
      __syncthreads();
    }
    // the largest tap in the time domain: y - w0 xs[n - k0] - (the other taps' convolution); xs[i < 0] = 0 -- the convolution
    // is linear, WienerHopf.cpp:125-160 -- is the window's own zero fill
#pragma unroll
    for (int c = 0; c < 16; c++)
      bufstore_c32(od, (t + T * c - hist) * 8, ok ? csub(csub(yv[c], cmul(w0, xdir[c])), v[c]) : yv[c]); // not PD: surveillance channel passes through
  }
}

// ---- the FIR with taps per BLOCK of the CPI (blah2hip_clutter_create_ex, n_blocks > 1) ------------------------------------
// The CPI of N samples is cut into B blocks of L = N / B; block j of CPI c is virtual CPI v = c B + j with taps w_v and flag
// ok_v of its own (estimated on the block's L samples alone).  The filter's HISTORY runs on across the block edges:
//     y_out[n] = y[n] - sum_k w_v[k] xs[n - k]   for n in block j,   xs[i] = x[(i - delayMin) mod N] over the WHOLE CPI,
// zero fill in front of sample 0 of the CPI only.  This is clutter_fir_kernel's overlap-save pass (whole windows, the largest
// tap in the time domain by the same argmax rule) on another grid: a workgroup serves ONE virtual CPI -- it transforms that
// block's taps once -- and walks the block's own segments n0 = j L + g segLen, cnt = min(segLen, L - g segLen), so that no
// segment straddles a block edge; the windows [n0 - hist, n0 - hist + F) reach back into block j - 1 through the CPI-level
// XsMap.  The y loads and the stores are descriptors over exactly the cnt new samples, as there.
// (The tap preamble is written out a second time: taken out into one forceinline function for both kernels it changed the
// register allocation of four of clutter_fir_kernel's fifteen instantiations -- 101 -> 99 SGPRs for the int16 words,
// 254 -> 256 VGPRs for <16, InC32, true> -- and that kernel's code is the n_blocks = 1 contract.)
// Grid: a block has few segments (ceil(L / segLen)) and a launch many virtual CPIs, so seg_walk -- eight XCDs times the
// workgroups of ONE CPI -- would leave most workgroups without a segment.  Here the launch is flat: workgroups are dealt
// round-robin over the 8 XCDs, so workgroup b runs on XCD b & 7; virtual CPI v is served by XCD v & 7 alone, by gx workgroups
// in consecutive dispatch slots of that XCD, which take segments job, job + gx, ...: neighbouring windows (they overlap by
// hist samples) meet in one L2, and only the padding of nVirt to a multiple of 8 is idle.
struct FirBlocksArgs {
  const void *x, *y;
  cf *yout;
  int64_t cpiStride, outStride;
  XsMap xs;          // of the CPI (N samples), not of the block
  int32_t nBins, segLen, nSeg; // nSeg = segments per BLOCK
  int32_t L, B, nVirt, gx;     // block length, blocks per CPI, virtual CPIs of the launch, workgroups per virtual CPI
  const cf *w;       // [nVirt][nBins]
  const int32_t *ok; // [nVirt]
  const cf *tw;
  float scale;
};

template <int R3, class In> __global__ __launch_bounds__(16 * R3, 2) void clutter_fir_blocks_kernel(FirBlocksArgs a)
{
  using W = WgFft<R3>;
  constexpr int T = W::T;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cf *P = reinterpret_cast<cf *>(smem);
  cf *Q = P + W::A_ELEMS;
  const int t = threadIdx.x;
  const int slot = blockIdx.x >> 3;
  const int vc = (slot / a.gx) * 8 + (blockIdx.x & 7), job = slot % a.gx;
  if (vc >= a.nVirt) return; // uniform: the padding of the launch
  const int cpi = vc / a.B, blk = vc - cpi * a.B;
  const typename ChanOf<In>::type X = ChanOf<In>::x(a.x, a.y, (int64_t)cpi * a.cpiStride);
  cf *O = a.yout + (int64_t)cpi * a.outStride;
  const bool ok = a.ok[vc] != 0;
  cf tw1[15], tw3[16];
  W::load_twiddles(t, a.tw, tw1, tw3);

  // spectrum of the block's taps, all but the largest (clutter_fir_kernel)
  const cf *wv_ = a.w + (size_t)vc * a.nBins;
  cf ws[16];
  float bestMag = -1.f;
  int bestIdx = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int m = t + T * k;
    const cf wv = wv_[min(m, a.nBins - 1)];
    const float keep = (m < a.nBins) ? a.scale : 0.f;
    ws[k] = cmake(wv.x * keep, wv.y * keep);
    const float mag = (m < a.nBins) ? wv.x * wv.x + wv.y * wv.y : -1.f;
    if (mag > bestMag) { bestMag = mag; bestIdx = m; } // (ascending m: ties go to the lower index)
  }
  {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float mu = __shfl_xor(bestMag, off);
      const int iu = __shfl_xor(bestIdx, off);
      if (mu > bestMag || (mu == bestMag && iu < bestIdx)) { bestMag = mu; bestIdx = iu; }
    }
    if (T > 64) {
      float *sm = reinterpret_cast<float *>(P);
      int *si = reinterpret_cast<int *>(P) + T / 64;
      if ((t & 63) == 0) { sm[t >> 6] = bestMag; si[t >> 6] = bestIdx; }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < T / 64; u++) {
        const float mu = sm[u];
        const int iu = si[u];
        if (mu > bestMag || (mu == bestMag && iu < bestIdx)) { bestMag = mu; bestIdx = iu; }
      }
      __syncthreads();
    }
  }
  const int k0 = bestIdx;
  const cf w0 = wv_[k0];
#pragma unroll
  for (int k = 0; k < 16; k++)
    if (t + T * k == k0) ws[k] = cmake(0.f, 0.f);
  W::fwd_s1(t, ws, tw1, P);
  __syncthreads();
  W::fwd_s2(t, ws, P, Q);
  __syncthreads();
  W::fwd_s3(t, ws, tw3, Q);
  __syncthreads();

  const int hist = a.nBins - 1;
  const int N = (int)a.xs.N;
  const int blk0 = blk * a.L; // first sample of the block in its CPI
  using CX = typename BufChanOf<In>::X;
  using CY = typename BufChanOf<In>::Y;
  // sixteen values of the window that starts at sample src0 of the CPI's xs: zero outside [0, N)
  auto load_window = [&](cf *dst, int src0) {
    uint32_t j0;
    int xcnt;
    if (xs_window_plain(src0, 16 * T, a.xs, &j0, &xcnt)) { // the interior: one contiguous run of x, immediates only
      const __amdgpu_buffer_rsrc_t xd = make_rsrc_b(BufChanOf<In>::x(a.x, a.y, (int64_t)cpi * a.cpiStride + j0), xcnt * CX::STRIDE);
#pragma unroll
      for (int k = 0; k < 16; k++) dst[k] = RawBuiltin<CX>::cvt(RawBuiltin<CX>::ld(xd, (t + T * k) * CX::STRIDE, 0));
    } else {
#pragma unroll
      for (int k = 0; k < 16; k++) {
        const int src = src0 + t + T * k;
        const bool inr = src >= 0 && src < N;
        const cf xv = X[xs_index(inr ? (uint32_t)src : 0u, a.xs)];
        dst[k] = inr ? xv : cmake(0.f, 0.f);
      }
    }
  };
  for (int g = job; g < a.nSeg; g += a.gx) {
    const int off = g * a.segLen;
    const int n0 = blk0 + off, cnt = min(a.segLen, a.L - off); // the block's own grid: the last segment ends with the block
    cf v[16], yv[16];
    load_window(v, n0 - hist);
    const __amdgpu_buffer_rsrc_t yd = make_rsrc_b(BufChanOf<In>::y(a.x, a.y, (int64_t)cpi * a.cpiStride + n0), cnt * CY::STRIDE);
    const __amdgpu_buffer_rsrc_t od = make_rsrc_b(O + n0, cnt * 8);
#pragma unroll
    for (int k = 0; k < 16; k++) yv[k] = RawBuiltin<CY>::cvt(RawBuiltin<CY>::ld(yd, (t + T * k - hist) * CY::STRIDE, 0));
    cf xdir[16];
    if (ok) {
      W::fwd_s1(t, v, tw1, P);
      __syncthreads();
      W::fwd_s2(t, v, P, Q);
      __syncthreads();
      W::fwd_s3(t, v, tw3, Q);
#pragma unroll
      for (int e = 0; e < 16; e++) v[e] = cmul(v[e], ws[e]);
      load_window(xdir, n0 - hist - k0); // register c: xs[n - k0] of the output sample n that register c writes
      __syncthreads();
      W::inv_s1(t, v, tw3, P);
      __syncthreads();
      W::inv_s2(t, v, P, Q);
      __syncthreads();
      W::inv_s3(t, v, tw1, Q);
      __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < 16; c++)
      bufstore_c32(od, (t + T * c - hist) * 8, ok ? csub(csub(yv[c], cmul(w0, xdir[c])), v[c]) : yv[c]); // a block that is not PD passes through
  }
}

// ---- correlations of a SHORT block, lag by lag in fp64 ----------------------------------------------------------------------
// A block of L samples with nBins taps has the matrix of a circular autocorrelation over L: at L = nBins a full circulant whose
// eigenvalues are the reference's power spectrum -- cond(A) 4e4 ... 9e5 on white references of 2047 samples, 1e2 at L = 1.5
// nBins, 5e1 at 2 nBins, 2e1 from 3 nBins on (fp64, CPU).  The transforms' fp32 partials carry 1e-7 of r[0]; times such a
// condition number that moved the filtered channel by 1e-2 of itself at L = nBins (measured; the gate is 1e-4).  So a block
// child with L < 2 nBins forms r and b directly: a thread per lag, the L products summed in order in fp64 (exact products of
// fp32 samples, 1e-13 of the sum), written where the reduction would have put them.  L nBins products per block and row: at most
// 2 nBins^2, nothing beside the solve there -- and not a path for long blocks (L nBins grows where the transforms' L log F
// does not).  Deterministic: one fixed-order sum per lag.
struct CorrDirectArgs {
  const void *x, *y;
  int64_t cpiStride; // of the caller's CPIs; block j of CPI c starts at c cpiStride + j L
  XsMap xs;          // of the block (N = L)
  int32_t nBins, B, lagTiles;
  dcx *rb;           // [nVirt][2][nBins]: r then b
};
template <class In> __global__ __launch_bounds__(256) void clutter_corr_direct_kernel(CorrDirectArgs a)
{
  const int vc = blockIdx.x / a.lagTiles, k = (blockIdx.x - vc * a.lagTiles) * 256 + threadIdx.x, mode = blockIdx.y;
  if (k >= a.nBins) return;
  const int cpi = vc / a.B, blk = vc - cpi * a.B;
  const uint32_t L = a.xs.N;
  const int64_t base = (int64_t)cpi * a.cpiStride + (int64_t)blk * L;
  const typename ChanOf<In>::type X = ChanOf<In>::x(a.x, a.y, base);
  const typename ChanOf<In>::type Y = ChanOf<In>::y(a.x, a.y, base);
  double sx = 0.0, sy = 0.0;
  uint32_t m = (uint32_t)k; // (n + k) mod L; k < nBins <= L
  for (uint32_t n = 0; n < L; n++) {
    const cf u = X[xs_index(n, a.xs)];
    const cf s = mode ? Y[m] : X[xs_index(m, a.xs)];
    // s conj(u)
    sx = __builtin_fma((double)s.x, (double)u.x, __builtin_fma((double)s.y, (double)u.y, sx));
    sy = __builtin_fma((double)s.y, (double)u.x, __builtin_fma(-(double)s.x, (double)u.y, sy));
    m = (m + 1u == L) ? 0u : m + 1u;
  }
  a.rb[((size_t)vc * 2 + mode) * a.nBins + k] = {sx, sy};
}

// a long filter's result into the caller's plane, CPI by CPI where ok (the multi entry point leaves the others unwritten)
__global__ __launch_bounds__(256) void long_out_kernel(const cf *src, cf *dst, uint32_t N, int64_t dstStride, const int32_t *ok)
{
  const uint32_t m = blockIdx.x * 256u + threadIdx.x;
  if (m >= N || !ok[blockIdx.y]) return;
  dst[(int64_t)blockIdx.y * dstStride + m] = src[(size_t)blockIdx.y * N + m];
}

// ---- LONG filters: more taps than one transform holds --------------------------------------------------------------
// WienerHopf.cpp takes any nBins (a dense nBins x nBins Cholesky and FFTs of the whole CPI).  The kernels above hold
// nBins <= F - 15 = 4081.  Beyond that -- any nBins <= nSamples -- the same
// kernels run chunk by chunk of LONG_C = 2048 lags / taps on rotated or shifted copies of the channels:
//   b[cC + j] = sum_n y[n] conj(xs[n - cC - j]) = the child's b[j] with y rotated by cC            (circular, :100-108)
//   r[cC + j] = the same with xs in y's place                                                       (:76-84)
//   y - (w * xs) = y - sum_c (w[cC ...] * xs delayed by cC, zeros shifted in)                       (linear, :125-160)
// with xs[i] = x[(uint32(i) - uint32(delayMin)) mod N] (:61-70, the reference's own unsigned arithmetic).  One child handle
// (first lag = this filter's) does the correlations, a second (first lag 0: its xs IS its x) the FIR passes; the solve is
// clutter_solve_kernel<11, true, 768>.  fp32 planes only.  A rarely used form, built for coverage rather than speed: 2 nChunks - 1
// correlation passes and nChunks FIR passes over the CPI, ~1 us per order of the solve.
constexpr int LONG_C = 2048;

// planes [nCpi][N] out of planes [nCpi][N] (every index below 2^31: no overflow in uint32):
// MODE 0: dst[m] = src[(m + off) mod N]                      (y rotated)
// MODE 1: dst[m] = xs[(m + off) mod N]                       (xs rotated; src = x)
// MODE 2: dst[m] = m >= off ? xs[m - off] : 0                (xs delayed, zeros shifted in; src = x)
// xs[i] = x[(uint32(i) - uint32(delayMin)) mod N]: the reference's own unsigned arithmetic (WienerHopf.cpp:61-70)
// (A first version with the mode as a run-time argument and a grid-stride loop faulted on gfx950 -- in a stand-alone
// program too; this one is one sample per thread and a compile-time mode.)
template <int MODE>
__global__ __launch_bounds__(256) void long_plane_kernel(const cf *src, cf *dst, uint32_t N, uint32_t off, uint32_t dmin)
{
  const cf *s = src + (size_t)blockIdx.y * N;
  cf *d = dst + (size_t)blockIdx.y * N;
  const uint32_t m = blockIdx.x * 256u + threadIdx.x;
  if (m >= N) return;
  cf v = cmake(0.f, 0.f);
  if (MODE == 0) v = s[(m + off) % N];
  if (MODE == 1) v = s[(((m + off) % N) - dmin) % N];
  if (MODE == 2 && m >= off) v = s[((m - off) - dmin) % N];
  d[m] = v;
}

// which 0: the child's b -> b[cC + j]; 1: the child's r -> r[cC + j] (chunk 0); 2: the child's b -> r[cC + j]
__global__ __launch_bounds__(256) void long_gather_kernel(const dcx *sub, dcx *big, int C, int n, int c, int which)
{
  const int j = blockIdx.x * 256 + threadIdx.x, cpi = blockIdx.y;
  const int k = c * C + j;
  if (j >= C || k >= n) return;
  const dcx v = sub[((size_t)cpi * 2 + (which == 1 ? 0 : 1)) * C + j];
  big[((size_t)cpi * 2 + (which == 0 ? 1 : 0)) * n + k] = v;
}

// the FIR child's taps of chunk c: w[cC + j], zeros behind the filter's last tap
__global__ __launch_bounds__(256) void long_taps_kernel(const cf *w, cf *wsub, int C, int n, int c)
{
  const int j = blockIdx.x * 256 + threadIdx.x, cpi = blockIdx.y;
  if (j >= C) return;
  const int k = c * C + j;
  wsub[(size_t)cpi * C + j] = k < n ? w[(size_t)cpi * n + k] : cmake(0.f, 0.f);
}

} // namespace clutter
} // namespace blah2
