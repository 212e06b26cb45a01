// A receiver array behind the Doppler stage (gfx950 / MI355X only).  No reference counterpart: blah2 has one
// surveillance channel.
// Included by array.hip alone: this header defines kernels, so a second unit must not include it.
//
//   beamform_kernel    M_b = sum_k w[b][k] M_k for every beam b in ONE pass over the K channel maps, with the
//                      per-workgroup partials of Map::set_metrics (Map.cpp:187-206) of every beam map
//   snapshot_kernel    the K channel cells under every detection of a list (what a bearing is computed from)
//   array_cov_kernel   the K x K array covariance of the channel maps over a training rectangle, per CPI, in fp64
//   cov_fold_kernel    ... its per-workgroup partials folded in index order into the Hermitian matrix
//   mvdr_weights_kernel  minimum-variance (Capon) weights from that covariance: an fp64 Cholesky solve per CPI and beam
//   bearing_kernel     the bearing of every detection: its snapshot scanned over a steering table, whitened by that
//                      covariance's Cholesky factor (the adaptive matched filter) or not (Bartlett), in fp64
// ... and in front of the whole chain, on the K sample planes themselves:
//   sample_cov_kernel  the K x K array covariance of the channels' SAMPLES over a window of the CPI, per CPI, in fp64
//                      (complex fp32 planes, or int8 (I, Q) planes: exact); cov_fold_kernel finishes it
//   beam_samples_kernel / beam_samples_wdev_kernel
//                      y_b = sum_k w[b][k] y_k for every beam b in ONE pass over the K sample planes: each beam plane is
//                      then one surveillance channel to the clutter filter and the range + Doppler chain
//
// The cross-ambiguity map is linear in the surveillance channel, so the map of the beam y_b = sum_k w[b][k] y_k is the
// same combination of the channel maps blah2hip_amb_process_multi_dev left in HBM: a further beam costs one more map
// written, not a range + Doppler chain.
#pragma once

#include <hip/hip_runtime.h>

#include "blah2hip.h"
#include "metrics_core.hpp"

#include <type_traits>

namespace blah2 {

// f(std::integral_constant<int, K>()) for the call's channel count K = 1 .. BLAH2HIP_MAX_SURV: how every launcher below
// picks the kernel that is instantiated for K channels (inlined: a launcher is the switch, not a call of it)
template <class F> __attribute__((always_inline)) inline void with_channel_count(uint32_t K, F f)
{
  switch (K) {
  case 1: f(std::integral_constant<int, 1>()); break;
  case 2: f(std::integral_constant<int, 2>()); break;
  case 3: f(std::integral_constant<int, 3>()); break;
  case 4: f(std::integral_constant<int, 4>()); break;
  case 5: f(std::integral_constant<int, 5>()); break;
  case 6: f(std::integral_constant<int, 6>()); break;
  case 7: f(std::integral_constant<int, 7>()); break;
  case 8: f(std::integral_constant<int, 8>()); break;
  }
}

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
// of sum_k |w_k| |M_k|; a weight of exactly 1 or 0 passes a cell through bit for bit.  The weights w[b][k] are the launch
// arguments' (W = BLAH2HIP_MAX_SURV) or the CPI's own, read from the device up front (W = K): the operations and their
// order are the same, so equal weights give equal bits.
template <int K, int V, int W>
__device__ __forceinline__ void beam_cells(const BeamArgs &a, const cf (&wts)[BLAH2HIP_MAX_BEAMS][W], const cf *in, cf *out,
                                           size_t chStride, size_t i, double (&lsum)[BLAH2HIP_MAX_BEAMS],
                                           float (&lmax)[BLAH2HIP_MAX_BEAMS])
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
          const cf w = wts[b][k];
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
template <int K, int V, int W>
__device__ __forceinline__ void beam_run(const BeamArgs &a, const cf (&wts)[BLAH2HIP_MAX_BEAMS][W])
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
    beam_cells<K, V>(a, wts, in, out, chStride, head + u * V, lsum, lmax);
  if (V == 2 && blockIdx.x == 0) {
    const size_t nLeft = head + ((cells - head) & 1);
    if (threadIdx.x < nLeft) beam_cells<K, 1>(a, wts, in, out, chStride, (threadIdx.x == 0 && head) ? 0 : cells - 1, lsum, lmax);
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

// one set of weights for every CPI, in the launch arguments (blah2hip_amb_beamform_dev)
template <int K, int V>
__global__ __launch_bounds__(256) void beamform_kernel(BeamArgs a)
{
  beam_run<K, V>(a, a.w);
}

// the CPI's own weights wdev[cpi][b][k] on the device (blah2hip_amb_beamform_wdev; a.w is unused): blockIdx.y is the CPI, so
// they are uniform over the workgroup and read once, before the first cell
template <int K, int V>
__global__ __launch_bounds__(256) void beamform_wdev_kernel(BeamArgs a, const cf *wdev)
{
  cf wts[BLAH2HIP_MAX_BEAMS][K];
  const cf *wd = wdev + (size_t)blockIdx.y * a.nBeams * K;
#pragma unroll
  for (int b = 0; b < BLAH2HIP_MAX_BEAMS; b++) {
#pragma unroll
    for (int k = 0; k < K; k++) wts[b][k] = b < (int)a.nBeams ? wd[b * K + k] : cmake(0.f, 0.f);
  }
  beam_run<K, V>(a, wts);
}

// beamform_kernel<K, V> (or beamform_wdev_kernel<K, V>) for the call's channel count, 16-byte (V = 2) or 8-byte (V = 1)
// accesses
template <int V, bool WDEV> inline void launch_beamform(uint32_t K, dim3 grid, hipStream_t st, const BeamArgs &a, const cf *wdev)
{
  with_channel_count(K, [&](auto k) {
    if (WDEV) hipLaunchKernelGGL((beamform_wdev_kernel<decltype(k)::value, V>), grid, dim3(256), 0, st, a, wdev);
    else hipLaunchKernelGGL((beamform_kernel<decltype(k)::value, V>), grid, dim3(256), 0, st, a);
  });
}

struct SnapArgs {
  const cf *map;              // [nSurv][nCpi][nD][nDelay]
  const blah2hip_det_t *dets; // [nLists][cap]
  const uint32_t *count;      // [nLists]; more than cap: the first cap records are the list
  cf *snap;                   // [nLists][cap][nSurv]
  uint32_t nSurv, nCpi, cap, nLists;
  int32_t nD, nDelay;
};

// The cell under record i of list l in channel map 0 of the list's CPI l mod nCpi -- channel k lies k * nCpi * cells
// further on -- or nullptr where the slot lies behind the list's count or the record's row or column outside the map.
__device__ __forceinline__ const cf *snap_cell(const cf *map, const blah2hip_det_t *dets, const uint32_t *count, uint32_t cap,
                                               uint32_t nCpi, int32_t nD, int32_t nDelay, uint32_t l, uint32_t i)
{
  if (i >= count[l]) return nullptr;
  const blah2hip_det_t *d = dets + (size_t)l * cap + i;
  const int32_t row = d->row, col = d->col;
  if (row < 0 || row >= nD || col < 0 || col >= nDelay) return nullptr;
  return map + (l % nCpi) * ((size_t)nD * nDelay) + (size_t)row * nDelay + col;
}

// One thread per record slot (list l, index i).  Slots behind the list's count and records outside the map are left
// unwritten.
__global__ __launch_bounds__(256) void snapshot_kernel(SnapArgs a)
{
  const size_t total = (size_t)a.nLists * a.cap;
  const size_t cells = (size_t)a.nD * a.nDelay;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
    const cf *z = snap_cell(a.map, a.dets, a.count, a.cap, a.nCpi, a.nD, a.nDelay, (uint32_t)(t / a.cap), (uint32_t)(t % a.cap));
    if (!z) continue;
    for (uint32_t k = 0; k < a.nSurv; k++) a.snap[t * a.nSurv + k] = z[(size_t)k * a.nCpi * cells];
  }
}

// ---- adaptive beams: array covariance and minimum-variance weights -----------------------------------------------------
struct CovArgs {
  const cf *in;    // [K][nCpi][nD][nDelay]
  double *part;    // [nCpi][gridDim.x][K * K] per-workgroup partials, packed as below
  size_t chStride; // nCpi * nD * nDelay
  uint32_t cells, nDelay;
  uint32_t row0, col0, nRows, width; // the training rectangle
};

// R[c][i][j] = sum over the rectangle of M_i conj(M_j), per CPI c.  grid (G, nCpi), 256 threads.  A thread walks the
// rectangle's cells t = r * width + q with a stride of gridDim.x * 256 (row and column are carried along, no division in
// the loop), loads the K channel cells first (8-byte loads, all in flight together) and then updates the upper triangle:
// K real sums for the diagonal and K (K - 1) / 2 complex ones above it, K * K fp64 accumulators (128 VGPRs at K = 8).
// A product of two fp32 values is exact in fp64, so every accumulator update is one fp64 fused multiply-add: no fp32
// rounding at all, every addition fp64 -- inside the arithmetic contract of blah2hip_amb_covariance_dev, whose bound
// allows fp32 products.  The K * K sums are packed into one K x K array of doubles: [i][j] with i <= j holds
// Re R[i][j], [j][i] with i < j holds Im R[i][j].  The workgroup's partial is the lanes' sums folded by a butterfly, then
// the four waves' in order; cov_fold_kernel adds the partials in index order.  No floating-point atomics.
template <int K>
__global__ __launch_bounds__(256) void array_cov_kernel(CovArgs a)
{
  __shared__ double wpart[4][K * K];
  const uint32_t cpi = blockIdx.y;
  const cf *in = a.in + (size_t)cpi * a.cells + (size_t)a.row0 * a.nDelay + a.col0;
  double acc[K * K];
#pragma unroll
  for (int e = 0; e < K * K; e++) acc[e] = 0.0;

  const uint64_t n = (uint64_t)a.nRows * a.width;
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  const uint32_t dr = (uint32_t)(stride / a.width), dq = (uint32_t)(stride % a.width);
  uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t r = (uint32_t)(t / a.width), q = (uint32_t)(t % a.width);
  for (; t < n; t += stride) {
    const cf *p = in + (size_t)r * a.nDelay + q;
    cf m[K];
#pragma unroll
    for (int k = 0; k < K; k++) m[k] = p[k * a.chStride];
    double x[K], y[K];
#pragma unroll
    for (int k = 0; k < K; k++) { x[k] = (double)m[k].x; y[k] = (double)m[k].y; }
#pragma unroll
    for (int i = 0; i < K; i++) {
      acc[i * K + i] = fma(y[i], y[i], fma(x[i], x[i], acc[i * K + i]));
#pragma unroll
      for (int j = i + 1; j < K; j++) {
        acc[i * K + j] = fma(y[i], y[j], fma(x[i], x[j], acc[i * K + j]));  // Re M_i conj(M_j)
        acc[j * K + i] = fma(-x[i], y[j], fma(y[i], x[j], acc[j * K + i])); // Im M_i conj(M_j)
      }
    }
    r += dr;
    q += dq;
    if (q >= a.width) { q -= a.width; r++; }
  }

#pragma unroll
  for (int e = 0; e < K * K; e++) {
    double v = acc[e];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) wpart[threadIdx.x >> 6][e] = v;
  }
  __syncthreads();
  if (threadIdx.x < K * K) {
    const int e = threadIdx.x;
    a.part[((size_t)cpi * gridDim.x + blockIdx.x) * (K * K) + e] = ((wpart[0][e] + wpart[1][e]) + wpart[2][e]) + wpart[3][e];
  }
}

inline void launch_array_cov(uint32_t K, dim3 grid, hipStream_t st, const CovArgs &a)
{
  with_channel_count(K, [&](auto k) { hipLaunchKernelGGL((array_cov_kernel<decltype(k)::value>), grid, dim3(256), 0, st, a); });
}

// grid (nCpi), 64 threads: thread e < K * K adds entry e of the CPI's nParts partials in index order, then the packed sums
// become cov[c][i][j] (re, im): both triangles, R[j][i] the exact conjugate of R[i][j], the diagonal's imaginary part 0.
__global__ __launch_bounds__(64) void cov_fold_kernel(const double *part, uint32_t nParts, uint32_t K, double *cov)
{
  __shared__ double s[BLAH2HIP_MAX_SURV * BLAH2HIP_MAX_SURV];
  const uint32_t cpi = blockIdx.x, e = threadIdx.x, KK = K * K;
  if (e < KK) {
    double v = 0.0;
    for (uint32_t g = 0; g < nParts; g++) v += part[((size_t)cpi * nParts + g) * KK + e];
    s[e] = v;
  }
  __syncthreads();
  if (e < KK) {
    const uint32_t i = e / K, j = e % K;
    double *o = cov + 2 * ((size_t)cpi * KK + e);
    if (i == j) { o[0] = s[e]; o[1] = 0.0; }
    else if (i < j) { o[0] = s[i * K + j]; o[1] = s[j * K + i]; }
    else { o[0] = s[j * K + i]; o[1] = -s[i * K + j]; }
  }
}

struct MvdrArgs {
  const double *cov; // [nCpi][K][K] (re, im)
  cf *w;             // [nCpi][nBeams][K]
  int32_t *ok;       // [nCpi] or nullptr
  double loading;
  uint32_t nBeams;
  cf steer[BLAH2HIP_MAX_BEAMS][BLAH2HIP_MAX_SURV]; // in the launch arguments
};

// R_l = R + loading (tr R / K) I from the lower triangle of R ([K][K] (re, im)) and its Cholesky factor R_l = L L^H, left
// in the lower triangle of lr / li (the diagonal is real), everything in fp64 registers (K is a template parameter, every
// loop unrolled).  False where a pivot is not finite or not positive (an all-zero matrix; a NaN anywhere in the triangle
// reaches a pivot).  The statements are mvdr_weights_kernel's own, which keeps them inline: moved into a function they compile
// to other fused multiply-adds, and that kernel's bits are a contract.
template <int K>
__device__ __forceinline__ bool cholesky_loaded(const double *R, double loading, double (&lr)[K][K], double (&li)[K][K])
{
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < K; i++) {
#pragma unroll
    for (int j = 0; j <= i; j++) { lr[i][j] = R[2 * (i * K + j)]; li[i][j] = R[2 * (i * K + j) + 1]; }
    tr += lr[i][i];
  }
  const double delta = loading * (tr / K);
  bool good = true;
#pragma unroll
  for (int j = 0; j < K; j++) {
    double d = lr[j][j] + delta;
#pragma unroll
    for (int p = 0; p < j; p++) d -= lr[j][p] * lr[j][p] + li[j][p] * li[j][p];
    if (!(d > 0.0) || !(d < __builtin_huge_val())) good = false;
    const double piv = sqrt(d), inv = 1.0 / piv;
    lr[j][j] = piv;
#pragma unroll
    for (int i = j + 1; i < K; i++) {
      double sr = lr[i][j], si = li[i][j];
#pragma unroll
      for (int p = 0; p < j; p++) { // - L[i][p] conj(L[j][p])
        sr -= lr[i][p] * lr[j][p] + li[i][p] * li[j][p];
        si -= li[i][p] * lr[j][p] - lr[i][p] * li[j][p];
      }
      lr[i][j] = sr * inv;
      li[i][j] = si * inv;
    }
  }
  return good;
}

// L y = a by forward substitution; returns y^H y, summed in the order i = 0 .. K-1
template <int K>
__device__ __forceinline__ double forward_solve(const double (&lr)[K][K], const double (&li)[K][K], const double (&ar)[K],
                                                const double (&ai)[K], double (&yr)[K], double (&yi)[K])
{
  double den = 0.0;
#pragma unroll
  for (int i = 0; i < K; i++) {
    double sr = ar[i], si = ai[i];
#pragma unroll
    for (int p = 0; p < i; p++) {
      sr -= lr[i][p] * yr[p] - li[i][p] * yi[p];
      si -= lr[i][p] * yi[p] + li[i][p] * yr[p];
    }
    yr[i] = sr / lr[i][i];
    yi[i] = si / lr[i][i];
    den += yr[i] * yr[i] + yi[i] * yi[i];
  }
  return den;
}

// grid (nCpi), 64 threads: thread b < nBeams computes beam b of its CPI, everything in fp64 registers (K is a template
// parameter, every loop unrolled).  R_l = R + loading (tr R / K) I from the lower triangle of cov; Cholesky R_l = L L^H;
// L y = a, L^H x = y; h = x / (a^H x) with a^H x = y^H y; w = conj(h) rounded to fp32.  A pivot that is not finite or
// not positive (an all-zero CPI, a NaN anywhere in the triangle reaches a pivot) fails the CPI: ok = 0 and the
// conventional conj(a) / (a^H a).  Every thread of a CPI factorises the same matrix the same way (K <= 8: cheaper than
// sharing the factor), so they agree on ok.
template <int K>
__global__ __launch_bounds__(64) void mvdr_weights_kernel(MvdrArgs a)
{
  const uint32_t cpi = blockIdx.x, b = threadIdx.x;
  if (b >= a.nBeams) return;
  const double *R = a.cov + 2 * (size_t)cpi * K * K;
  double lr[K][K], li[K][K]; // lower triangle: R_l, overwritten by L
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < K; i++) {
#pragma unroll
    for (int j = 0; j <= i; j++) { lr[i][j] = R[2 * (i * K + j)]; li[i][j] = R[2 * (i * K + j) + 1]; }
    tr += lr[i][i];
  }
  const double delta = a.loading * (tr / K);
  bool good = true;
#pragma unroll
  for (int j = 0; j < K; j++) {
    double d = lr[j][j] + delta;
#pragma unroll
    for (int p = 0; p < j; p++) d -= lr[j][p] * lr[j][p] + li[j][p] * li[j][p];
    if (!(d > 0.0) || !(d < __builtin_huge_val())) good = false;
    const double piv = sqrt(d), inv = 1.0 / piv;
    lr[j][j] = piv;
#pragma unroll
    for (int i = j + 1; i < K; i++) {
      double sr = lr[i][j], si = li[i][j];
#pragma unroll
      for (int p = 0; p < j; p++) { // - L[i][p] conj(L[j][p])
        sr -= lr[i][p] * lr[j][p] + li[i][p] * li[j][p];
        si -= li[i][p] * lr[j][p] - lr[i][p] * li[j][p];
      }
      lr[i][j] = sr * inv;
      li[i][j] = si * inv;
    }
  }
  double ar[K], ai[K];
#pragma unroll
  for (int k = 0; k < K; k++) { ar[k] = (double)a.steer[b][k].x; ai[k] = (double)a.steer[b][k].y; }
  double hr[K], hi[K];
  if (good) {
    double yr[K], yi[K], den = 0.0;
#pragma unroll
    for (int i = 0; i < K; i++) { // L y = a
      double sr = ar[i], si = ai[i];
#pragma unroll
      for (int p = 0; p < i; p++) {
        sr -= lr[i][p] * yr[p] - li[i][p] * yi[p];
        si -= lr[i][p] * yi[p] + li[i][p] * yr[p];
      }
      yr[i] = sr / lr[i][i];
      yi[i] = si / lr[i][i];
      den += yr[i] * yr[i] + yi[i] * yi[i];
    }
#pragma unroll
    for (int i = K - 1; i >= 0; i--) { // L^H x = y
      double sr = yr[i], si = yi[i];
#pragma unroll
      for (int p = i + 1; p < K; p++) { // - conj(L[p][i]) x[p]
        sr -= lr[p][i] * hr[p] + li[p][i] * hi[p];
        si -= lr[p][i] * hi[p] - li[p][i] * hr[p];
      }
      hr[i] = sr / lr[i][i];
      hi[i] = si / lr[i][i];
    }
#pragma unroll
    for (int k = 0; k < K; k++) { hr[k] /= den; hi[k] /= den; }
  } else {
    double den = 0.0;
#pragma unroll
    for (int k = 0; k < K; k++) den += ar[k] * ar[k] + ai[k] * ai[k];
#pragma unroll
    for (int k = 0; k < K; k++) { hr[k] = ar[k] / den; hi[k] = ai[k] / den; }
  }
  cf *w = a.w + ((size_t)cpi * a.nBeams + b) * K;
#pragma unroll
  for (int k = 0; k < K; k++) w[k] = cmake((float)hr[k], (float)-hi[k]);
  if (b == 0 && a.ok) a.ok[cpi] = good ? 1 : 0;
}

inline void launch_mvdr_weights(uint32_t K, uint32_t nCpi, hipStream_t st, const MvdrArgs &a)
{
  with_channel_count(K, [&](auto k) { hipLaunchKernelGGL((mvdr_weights_kernel<decltype(k)::value>), dim3(nCpi), dim3(64), 0, st, a); });
}

// ---- a bearing per detection ----------------------------------------------------------------------------------------------
struct BearingArgs {
  const cf *map;              // [K][nCpi][nD][nDelay]
  const blah2hip_det_t *dets; // [nLists][cap]
  const uint32_t *count;      // [nLists]; more than cap: the first cap records are the list
  const double *cov;          // [nCpi][K][K] (re, im), or nullptr: the Bartlett scan
  const cf *steer;            // [nGrid][K]
  blah2hip_bearing_t *out;    // [nLists][cap]
  double loading;
  uint32_t nCpi, cap, nGrid, wrap;
  int32_t nD, nDelay;
};

constexpr uint32_t BEARING_CHUNK = 16; // records a workgroup scans per table it builds: four per wave

// P(g) = |u_g^H t|^2 from the normalised table: 4 K fused multiply-adds in the order k = 0 .. K-1, then the squares
template <int K>
__device__ __forceinline__ double bearing_power(const double (&ur)[K][BLAH2HIP_MAX_BEARING_GRID],
                                                const double (&ui)[K][BLAH2HIP_MAX_BEARING_GRID], uint32_t g,
                                                const double (&tr)[K], const double (&ti)[K])
{
  double pr = 0.0, pi = 0.0;
#pragma unroll
  for (int k = 0; k < K; k++) { // conj(u) t
    const double x = ur[k][g], y = ui[k][g];
    pr = fma(y, ti[k], fma(x, tr[k], pr));
    pi = fma(-y, tr[k], fma(x, ti[k], pi));
  }
  return pr * pr + pi * pi;
}

// grid (X, nLists), 256 threads.  List l belongs to CPI l mod nCpi.  A workgroup whose first record lies behind the list's
// count returns at once; the others
//   1. factorise the CPI's R_l = L L^H, every thread the same matrix in its own registers as in mvdr_weights_kernel (cov
//      == nullptr or a failed pivot: L = I, adaptive = 0 -- the SAME code then runs on the identity, so an identity
//      covariance, a failed one and no covariance give the same bits),
//   2. whiten and normalise the steering table, thread per grid point: v_g = L^-1 a_g, u_g = v_g / sqrt(v_g^H v_g) (0 where
//      v_g^H v_g is 0), into LDS as ur / ui [k][g] -- lanes of consecutive g read consecutive 8-byte words, no bank
//      conflict; 2 * K * 384 doubles, 48 KB at K = 8,
//   3. walk chunks of BEARING_CHUNK records with a stride of gridDim.x, one wave per record: the K cells through
//      snap_cell, t = L^-1 s in every lane, P(g) = |u_g^H t|^2 for g = lane, lane + 64, ...; the lane keeps its first
//      largest P, a butterfly folds the 64 (P, g) pairs with the lower index on equal P; the two neighbours' powers come
//      from the same table through the same function, so they carry the scan's bits; lane 0 writes the record.
// Everything is fp64 (the fp32 cells and steering entries convert exactly).  No atomics: a record is a function of its
// inputs alone.
template <int K>
__global__ __launch_bounds__(256) void bearing_kernel(BearingArgs a)
{
  __shared__ double ur[K][BLAH2HIP_MAX_BEARING_GRID], ui[K][BLAH2HIP_MAX_BEARING_GRID];
  const uint32_t l = blockIdx.y;
  const uint32_t n = min(a.count[l], a.cap);
  if ((uint64_t)blockIdx.x * BEARING_CHUNK >= n) return; // uniform over the workgroup, before any barrier

  double lr[K][K], li[K][K];
  bool adaptive = false;
  if (a.cov) adaptive = cholesky_loaded<K>(a.cov + 2 * (size_t)(l % a.nCpi) * K * K, a.loading, lr, li);
  if (!adaptive) {
#pragma unroll
    for (int i = 0; i < K; i++) {
#pragma unroll
      for (int j = 0; j <= i; j++) { lr[i][j] = i == j ? 1.0 : 0.0; li[i][j] = 0.0; }
    }
  }

  for (uint32_t g = threadIdx.x; g < a.nGrid; g += 256) {
    double ar[K], ai[K], vr[K], vi[K];
#pragma unroll
    for (int k = 0; k < K; k++) { const cf s = a.steer[(size_t)g * K + k]; ar[k] = (double)s.x; ai[k] = (double)s.y; }
    const double vv = forward_solve<K>(lr, li, ar, ai, vr, vi);
    const double rs = vv > 0.0 ? 1.0 / sqrt(vv) : 0.0;
#pragma unroll
    for (int k = 0; k < K; k++) { ur[k][g] = vr[k] * rs; ui[k][g] = vi[k] * rs; }
  }
  __syncthreads();

  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t chStride = (size_t)a.nCpi * a.nD * a.nDelay;
  for (uint64_t first = (uint64_t)blockIdx.x * BEARING_CHUNK; first < n; first += (uint64_t)gridDim.x * BEARING_CHUNK) {
    const uint32_t end = (uint32_t)min((uint64_t)n, first + BEARING_CHUNK);
    for (uint32_t i = (uint32_t)first + wave; i < end; i += 4) { // uniform over the wave
      const cf *z = snap_cell(a.map, a.dets, a.count, a.cap, a.nCpi, a.nD, a.nDelay, l, i);
      if (!z) continue;
      double sr[K], si[K];
      bool zero = true, finite = true;
#pragma unroll
      for (int k = 0; k < K; k++) {
        const cf c = z[(size_t)k * chStride];
        sr[k] = (double)c.x;
        si[k] = (double)c.y;
        zero = zero && c.x == 0.f && c.y == 0.f;
        finite = finite && fabsf(c.x) < __builtin_huge_valf() && fabsf(c.y) < __builtin_huge_valf();
      }
      blah2hip_bearing_t rec = {-1, 0, 0.0, 0.0, 0.0};
      if (!zero && finite) {
        double tr[K], ti[K];
        const double tt = forward_solve<K>(lr, li, sr, si, tr, ti);
        double best = -1.0; // every P is >= 0; a NaN (a steering entry that is not finite) never wins
        uint32_t bg = 0xFFFFFFFFu;
        for (uint32_t g = lane; g < a.nGrid; g += 64) {
          const double p = bearing_power<K>(ur, ui, g, tr, ti);
          if (p > best) { best = p; bg = g; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double op = __shfl_xor(best, off);
          const uint32_t og = (uint32_t)__shfl_xor((int)bg, off);
          if (op > best || (op == best && og < bg)) { best = op; bg = og; }
        }
        if (bg < a.nGrid) {
          double offset = 0.0;
          const bool inner = bg > 0 && bg + 1 < a.nGrid;
          if (inner || a.wrap) {
            const double pm = bearing_power<K>(ur, ui, bg > 0 ? bg - 1 : a.nGrid - 1, tr, ti);
            const double pp = bearing_power<K>(ur, ui, bg + 1 < a.nGrid ? bg + 1 : 0, tr, ti);
            const double den = (pm - 2.0 * best) + pp;
            if (den < 0.0) offset = 0.5 * (pm - pp) / den;
          }
          rec.index = (int32_t)bg;
          rec.adaptive = adaptive ? 1 : 0;
          rec.offset = offset;
          rec.power = best;
          rec.coherence = tt > 0.0 ? best / tt : 0.0;
        }
      }
      if (lane == 0) a.out[(size_t)l * a.cap + i] = rec;
    }
  }
}

inline void launch_bearing(uint32_t K, dim3 grid, hipStream_t st, const BearingArgs &a)
{
  with_channel_count(K, [&](auto k) { // (a bearing needs two channels)
    if constexpr (decltype(k)::value >= 2) hipLaunchKernelGGL((bearing_kernel<decltype(k)::value>), grid, dim3(256), 0, st, a);
  });
}

// ---- the array in the sample domain: covariance and beam planes of the K channels' samples ------------------------------
// A channel is a plane of complex fp32 samples or of int8 (I, Q) pairs (BLAH2HIP_FMT_I8: 2 bytes per sample, 2-byte
// aligned).  COVW: the samples of sample_cov_kernel's wide access (16 and 8 bytes).
struct SampC32 { static constexpr int BYTES = 8, COVW = 2; };
struct SampI8 { static constexpr int BYTES = 2, COVW = 4; };

// V adjacent samples of a plane in one access, from an address aligned to V * BYTES; get<v>: sample v as fp32 (every int8
// value converts exactly)
template <class Ch, int V> struct SampRaw;
template <> struct SampRaw<SampC32, 1> {
  typedef float type __attribute__((ext_vector_type(2)));
  template <int v> static __device__ __forceinline__ cf get(const type &r) { return cmake(r[0], r[1]); }
};
template <> struct SampRaw<SampC32, 2> {
  typedef float type __attribute__((ext_vector_type(4)));
  template <int v> static __device__ __forceinline__ cf get(const type &r) { return cmake(r[2 * v], r[2 * v + 1]); }
};
__device__ __forceinline__ cf samp_i8(uint32_t w) { return cmake((float)(int8_t)(w & 0xffu), (float)(int8_t)((w >> 8) & 0xffu)); }
template <> struct SampRaw<SampI8, 1> {
  typedef uint16_t type;
  template <int v> static __device__ __forceinline__ cf get(const type &r) { return samp_i8(r); }
};
template <> struct SampRaw<SampI8, 2> {
  typedef uint32_t type;
  template <int v> static __device__ __forceinline__ cf get(const type &r) { return samp_i8(r >> (16 * v)); }
};
template <> struct SampRaw<SampI8, 4> {
  typedef uint32_t type __attribute__((ext_vector_type(2)));
  template <int v> static __device__ __forceinline__ cf get(const type &r) { return samp_i8(r[v >> 1] >> (16 * (v & 1))); }
};

// samples in front of the first address aligned to V * BYTES, at most n
template <class Ch, int V> __device__ __forceinline__ uint32_t samp_head(const char *p, uint32_t n)
{
  if (V == 1) return 0;
  const uint32_t at = (uint32_t)(((uintptr_t)p / Ch::BYTES) & (V - 1));
  return min(n, (V - at) & (V - 1));
}

struct SampCovArgs {
  const void *y[BLAH2HIP_MAX_SURV]; // the K planes
  double *part;                     // [nCpi][gridDim.x][K * K] per-workgroup partials, packed as array_cov_kernel's
  uint64_t cpiStride;               // samples from CPI to CPI
  uint32_t s0, n;                   // the training window: n samples from sample s0 of the CPI
};

// sample v of each of K accesses into the K * K packed sums: array_cov_kernel's update, one fp64 fused multiply-add per
// product (fp32 x fp32 and int8 x int8 are both exact in fp64)
template <int K, class Raw, int v>
__device__ __forceinline__ void cov_update(const typename Raw::type (&m)[K], double (&acc)[K * K])
{
  double x[K], y[K];
#pragma unroll
  for (int k = 0; k < K; k++) { const cf s = Raw::template get<v>(m[k]); x[k] = (double)s.x; y[k] = (double)s.y; }
#pragma unroll
  for (int i = 0; i < K; i++) {
    acc[i * K + i] = fma(y[i], y[i], fma(x[i], x[i], acc[i * K + i]));
#pragma unroll
    for (int j = i + 1; j < K; j++) {
      acc[i * K + j] = fma(y[i], y[j], fma(x[i], x[j], acc[i * K + j]));  // Re y_i conj(y_j)
      acc[j * K + i] = fma(-x[i], y[j], fma(y[i], x[j], acc[j * K + i])); // Im y_i conj(y_j)
    }
  }
}

// V adjacent samples from sample i of the window on: the K loads first (all in flight together), then sample after sample
template <int K, class Ch, int V>
__device__ __forceinline__ void cov_samples(const char *const (&p)[K], size_t i, double (&acc)[K * K])
{
  typedef SampRaw<Ch, V> Raw;
  typename Raw::type m[K];
#pragma unroll
  for (int k = 0; k < K; k++) m[k] = *reinterpret_cast<const typename Raw::type *>(p[k] + i * Ch::BYTES);
  // sample after sample, the scheduler kept from converting them all ahead: at K = 8 the K * K sums fill half the registers
  cov_update<K, Raw, 0>(m, acc);
  if (V > 1) {
    __builtin_amdgcn_sched_barrier(0);
    cov_update<K, Raw, (V > 1 ? 1 : 0)>(m, acc);
  }
  if (V > 2) {
    __builtin_amdgcn_sched_barrier(0);
    cov_update<K, Raw, (V > 2 ? 2 : 0)>(m, acc);
    __builtin_amdgcn_sched_barrier(0);
    cov_update<K, Raw, (V > 2 ? 3 : 0)>(m, acc);
  }
}

// R[c][i][j] = sum over s0 <= n < s0 + a.n of y_i[c * cpiStride + n] conj(y_j[c * cpiStride + n]), per CPI c: array_cov_kernel
// over a window of samples instead of a rectangle of cells.  grid (G, nCpi), 256 threads; the same K * K packed fp64 sums,
// the same fold (butterfly over the lanes, the four waves in order, one partial per workgroup, cov_fold_kernel adds them
// in index order).  No floating-point atomics.  fp32 planes: array_cov_kernel's arithmetic and contract.  int8 planes:
// every product is an integer of at most 2^14 and every sum one below 2^53 (2^32 samples would be needed to get there), so
// every fused multiply-add and every addition of the folds is exact: the result is the integer sum, whatever the grid.
// V = 1: one sample per access.  V = Ch::COVW: accesses of V samples (16 bytes of fp32 pairs, 8 bytes of int8 pairs) from
// the first aligned sample of the window on; the host picks it where every channel's window of a CPI starts at the same
// offset modulo the access (it may differ from CPI to CPI).  The at most V - 1 samples in front and behind go through
// single-sample accesses in workgroup 0.
template <int K, class Ch, int V>
__global__ __launch_bounds__(256) void sample_cov_kernel(SampCovArgs a)
{
  __shared__ double wpart[4][K * K];
  const uint32_t cpi = blockIdx.y;
  const char *p[K];
#pragma unroll
  for (int k = 0; k < K; k++) p[k] = (const char *)a.y[k] + ((size_t)cpi * a.cpiStride + a.s0) * Ch::BYTES;
  double acc[K * K];
#pragma unroll
  for (int e = 0; e < K * K; e++) acc[e] = 0.0;

  const uint32_t head = samp_head<Ch, V>(p[0], a.n);
  const uint32_t nUnits = (a.n - head) / V;
  for (uint64_t u = blockIdx.x * 256 + threadIdx.x; u < nUnits; u += gridDim.x * 256)
    cov_samples<K, Ch, V>(p, head + (size_t)u * V, acc);
  if (V > 1 && blockIdx.x == 0) {
    const uint32_t done = head + nUnits * V; // the tail starts here
    if (threadIdx.x < head + (a.n - done)) cov_samples<K, Ch, 1>(p, threadIdx.x < head ? threadIdx.x : done + (threadIdx.x - head), acc);
  }

#pragma unroll
  for (int e = 0; e < K * K; e++) {
    double v = acc[e];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) wpart[threadIdx.x >> 6][e] = v;
  }
  __syncthreads();
  if (threadIdx.x < K * K) {
    const int e = threadIdx.x;
    a.part[((size_t)cpi * gridDim.x + blockIdx.x) * (K * K) + e] = ((wpart[0][e] + wpart[1][e]) + wpart[2][e]) + wpart[3][e];
  }
}

template <class Ch, int V> inline void launch_sample_cov(uint32_t K, dim3 grid, hipStream_t st, const SampCovArgs &a)
{
  with_channel_count(K, [&](auto k) { hipLaunchKernelGGL((sample_cov_kernel<decltype(k)::value, Ch, V>), grid, dim3(256), 0, st, a); });
}

struct BeamSampArgs {
  const void *y[BLAH2HIP_MAX_SURV]; // the K input planes
  cf *out[BLAH2HIP_MAX_BEAMS];      // the beam planes
  uint64_t cpiStride, beamStride;   // samples from CPI to CPI, in and out
  uint32_t nSamples, nBeams;
  cf w[BLAH2HIP_MAX_BEAMS][BLAH2HIP_MAX_SURV]; // in the launch arguments: wave-uniform, read by scalar loads
};

// V adjacent samples from sample i of the CPI on: the K loads first (all in flight together), then beam after beam, the
// beam loop unrolled to its limit behind a wave-uniform test as in beam_cells.  Per component the sum is beam_cells' chain
// of fused multiply-adds in the order k = 0 .. K-1, written out again here so that beamform_kernel's code, whose bits are a
// contract, is not touched: 2K roundings, a weight of exactly 1 or 0 passes a sample (int8: its exact conversion) through.
template <int K, class Ch, int V, int W>
__device__ __forceinline__ void beam_samples(const BeamSampArgs &a, const cf (&wts)[BLAH2HIP_MAX_BEAMS][W], const char *const (&p)[K],
                                             size_t outOff, size_t i)
{
  typedef SampRaw<Ch, V> Raw;
  typedef typename BeamVec<V>::type vec;
  typename Raw::type m[K];
#pragma unroll
  for (int k = 0; k < K; k++) m[k] = *reinterpret_cast<const typename Raw::type *>(p[k] + i * Ch::BYTES);
  cf s[K][V];
#pragma unroll
  for (int k = 0; k < K; k++) {
    s[k][0] = Raw::template get<0>(m[k]);
    if (V == 2) s[k][V - 1] = Raw::template get<V - 1>(m[k]);
  }
#pragma unroll
  for (int b = 0; b < BLAH2HIP_MAX_BEAMS; b++) {
    if (b < (int)a.nBeams) {
      vec r;
#pragma unroll
      for (int v = 0; v < V; v++) {
        float re = 0.f, im = 0.f;
#pragma unroll
        for (int k = 0; k < K; k++) {
          const cf w = wts[b][k];
          const float mx = s[k][v].x, my = s[k][v].y;
          re = fmaf(-w.y, my, k ? fmaf(w.x, mx, re) : w.x * mx);
          im = fmaf(w.y, mx, k ? fmaf(w.x, my, im) : w.x * my);
        }
        r[2 * v] = re;
        r[2 * v + 1] = im;
      }
      *reinterpret_cast<vec *>(a.out[b] + outOff + i) = r;
    }
  }
}

// grid (G, nCpi), 256 threads.  A workgroup strides over its CPI in units of V samples.  V = 2 (16-byte stores; 16-byte
// loads of fp32 pairs, 4-byte loads of int8 pairs) needs every input plane's and every beam plane's copy of a CPI to start at
// the same parity of sample with respect to its access (the host checks it CPI by CPI): a CPI that starts one sample off then has
// a one-sample head, and whatever is left behind the last pair is a one-sample tail; both go through single-sample accesses
// in workgroup 0.  V = 1 otherwise.  Samples from nSamples on -- the gap up to beamStride -- are not written.
template <int K, class Ch, int V, int W>
__device__ __forceinline__ void beam_samples_run(const BeamSampArgs &a, const cf (&wts)[BLAH2HIP_MAX_BEAMS][W])
{
  const uint32_t cpi = blockIdx.y;
  const char *p[K];
#pragma unroll
  for (int k = 0; k < K; k++) p[k] = (const char *)a.y[k] + (size_t)cpi * a.cpiStride * Ch::BYTES;
  const size_t outOff = (size_t)cpi * a.beamStride;
  const uint32_t head = samp_head<Ch, V>(p[0], a.nSamples);
  const uint32_t nUnits = (a.nSamples - head) / V;
  for (uint64_t u = blockIdx.x * 256 + threadIdx.x; u < nUnits; u += gridDim.x * 256)
    beam_samples<K, Ch, V>(a, wts, p, outOff, head + (size_t)u * V);
  if (V == 2 && blockIdx.x == 0) {
    const uint32_t done = head + nUnits * V;
    if (threadIdx.x < head + (a.nSamples - done))
      beam_samples<K, Ch, 1>(a, wts, p, outOff, threadIdx.x < head ? threadIdx.x : done + (threadIdx.x - head));
  }
}

// one set of weights for every CPI, in the launch arguments (blah2hip_amb_beam_samples_dev)
template <int K, class Ch, int V>
__global__ __launch_bounds__(256) void beam_samples_kernel(BeamSampArgs a)
{
  beam_samples_run<K, Ch, V>(a, a.w);
}

// the CPI's own weights wdev[cpi][b][k] on the device (blah2hip_amb_beam_samples_wdev; a.w is unused), read once before the
// first sample as in beamform_wdev_kernel: the operations and their order are the same, so equal weights give equal bits
template <int K, class Ch, int V>
__global__ __launch_bounds__(256) void beam_samples_wdev_kernel(BeamSampArgs a, const cf *wdev)
{
  cf wts[BLAH2HIP_MAX_BEAMS][K];
  const cf *wd = wdev + (size_t)blockIdx.y * a.nBeams * K;
#pragma unroll
  for (int b = 0; b < BLAH2HIP_MAX_BEAMS; b++) {
#pragma unroll
    for (int k = 0; k < K; k++) wts[b][k] = b < (int)a.nBeams ? wd[b * K + k] : cmake(0.f, 0.f);
  }
  beam_samples_run<K, Ch, V>(a, wts);
}

template <class Ch, int V, bool WDEV> inline void launch_beam_samples(uint32_t K, dim3 grid, hipStream_t st, const BeamSampArgs &a, const cf *wdev)
{
  with_channel_count(K, [&](auto k) {
    if (WDEV) hipLaunchKernelGGL((beam_samples_wdev_kernel<decltype(k)::value, Ch, V>), grid, dim3(256), 0, st, a, wdev);
    else hipLaunchKernelGGL((beam_samples_kernel<decltype(k)::value, Ch, V>), grid, dim3(256), 0, st, a);
  });
}

} // namespace blah2
