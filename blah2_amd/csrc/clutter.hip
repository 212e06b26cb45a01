// WienerHopf clutter filter on gfx950 (include/blah2hip.h, clutter section).
//
// Reference: /root/reference/src/process/clutter/WienerHopf.cpp:58-163.  With
//   xs[i] = x[(i - delayMin) mod N]                       (:67, uint32 arithmetic)
//   r[k]  = sum_n xs[(n+k) mod N] conj(xs[n])             (:76-84,  k < nBins)
//   b[k]  = sum_n  y[(n+k) mod N] conj(xs[n])             (:100-108)
//   A[i][j] = r[i-j]  (Hermitian Toeplitz, :85-97),  A w = b   (:111-122)
//   y_out[n] = y[n] - sum_k w[k] xs[n-k],  xs[m<0] = 0    (:125-160)
// nBins = delayMax - delayMin (no +1, :12).
//
// The reference does this with 4 FFTs + 2 IFFTs of length N and 3 of length
// N+nBins+1, plus a dense Cholesky.  None of those long transforms is needed:
//   * r and b are nBins lags of a circular correlation -> the same segmented
//     on-chip FFT correlation as the range kernel (clutter_corr_kernel),
//     partial sums per workgroup, reduced in fp64;
//   * A is Hermitian Toeplitz -> Levinson recursion in fp64, O(nBins^2), with Schur
//     residual recursions in place of its inner products (clutter_solve_kernel: one
//     workgroup per CPI, one barrier per order).  The reference's chol() fails exactly
//     when A is not positive definite; the recursion detects the same condition
//     (a prediction-error factor 1-|e|^2 <= 0 or r[0] <= 0) -> ok = 0;
//   * the FIR is an overlap-save convolution on the on-chip FFT
//     (clutter_fir_kernel), one pass over x and y.
// Results are mathematically identical to the reference's (same linear
// system, same linear convolution); arithmetic is fp32 for the transforms and
// fp64 for the reduction and the solve.
//
// This unit: the planner, the correlation and FIR launches and the C API; kernels in clutter_kernels.hpp.  The solve with
// its two entry points is clutter_solve.hip; clutter_handle.hpp holds the handle and what crosses between the units.
// the correlation kernels run at 244-256 VGPRs: keep the butterflies as single-instruction statements
// (fft_wg.hpp; the grouped form spills 5-33 registers here and costs 3.6 %, measured)
#define B2_SPLIT_BUTTERFLIES 1
#include <hip/hip_runtime.h>

#include "clutter_handle.hpp"
#include "clutter_kernels.hpp"

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <vector>

using namespace blah2;
using namespace blah2::clutter;

namespace {

// what a launch_clutter call runs (the long form and the block form drive their children piecewise)
enum Stages : int { ESTIMATE_CORR = 1 /* correlations + reduction */, ESTIMATE_SOLVE = 2, FIR = 4, ALL_STAGES = 7 };

// (multiples of 8: the segment walk is XCD-aware, see seg_walk)
inline int up8(int v) { return std::max(8, (v + 7) & ~7); }
// residency of the correlation and FIR kernels: 4 workgroups per CU (LDS)
inline int resident_slots(const blah2hip_clutter_s *h) { return 4 * h->numCU; }
// dynamic LDS of every kernel on WgFft<R3>: its two exchange buffers
template <int R3> constexpr size_t fft_lds() { return (size_t)(WgFft<R3>::A_ELEMS + WgFft<R3>::B_ELEMS) * sizeof(cf); }

// the multi-channel buffers (multi_alloc builds them); the caller has synchronised the device
hipError_t multi_free(blah2hip_clutter_s *h)
{
  for (void **p : {(void **)&h->d_partialM, (void **)&h->d_rbM, (void **)&h->d_wM, (void **)&h->d_okM}) {
    if (*p) { hipError_t e = hipFree(*p); if (e != hipSuccess) return e; }
    *p = nullptr;
  }
  h->multiK = 0; h->multiJobs = 0;
  if (h->lastSurv) { h->lastSurv = 0; h->lastOk = nullptr; }
  return hipSuccess;
}

// Transform length, segmentation, correlation form and the buffers sized by them (create, and again when
// BLAH2HIP_CLUTTER_OPT_FFT_LEN / _CORR re-plan).  F - nBins + 1 useful samples per F log F work.
int clutter_plan(blah2hip_clutter_s *h)
{
  const int nBins = h->nBins;
  int bestR3 = 0;
  double best = 1e300;
  for (int r3 : {4, 8, 16}) {
    const int F = 256 * r3;
    if (h->fftLenForce && F != h->fftLenForce) continue;
    const int L = F - nBins + 1;
    if (L < 16) continue;
    // measured per-point speed of the three transform kernels (tools/gpu_diag.py)
    const double cost = (double)F * std::log2((double)F) / (double)L * (r3 == 16 ? 1.4 : (r3 == 4 ? 1.08 : 1.0));
    if (cost < best) { best = cost; bestR3 = r3; }
  }
  if (!bestR3) CFAIL(BLAH2HIP_ERR_UNSUPPORTED, "nBins too large for the on-chip transform lengths (<= 4096)");
  h->r3 = bestR3; h->F = 256 * bestR3;
  h->segLen = h->F - nBins + 1;
  // a filter whose history is just under half the transform: blocks of exactly F/2 samples, so that consecutive windows
  // overlap by whole registers and the FIR kernel carries the overlap instead of reading it again (clutter_fir_kernel)
  h->firCarry = h->segLen >= h->F / 2 && h->segLen <= h->F / 2 + h->F / 64 && !h->firNoCarry;
  if (h->firCarry) h->segLen = h->F / 2;
  h->nSeg = (int)((h->N + (uint32_t)h->segLen - 1) / (uint32_t)h->segLen);
  // correlations: windowed form 3 transforms per segLen samples, half-window form 2 per F/2
  // (needs nBins - 1 <= F/2 and at least nBins samples)
  const bool halfOk = (nBins - 1 <= h->F / 2) && ((uint32_t)nBins <= h->N);
  h->corrHalf = halfOk && (4.0 / h->F < 3.0 / h->segLen);
  if (h->corrForce == BLAH2HIP_CLUTTER_CORR_HALF) {
    if (!halfOk) CFAIL(BLAH2HIP_ERR_UNSUPPORTED, "the half-window correlation needs nBins - 1 <= F/2 and nBins <= nSamples");
    h->corrHalf = true;
  }
  if (h->corrForce == BLAH2HIP_CLUTTER_CORR_WINDOW) h->corrHalf = false;
  h->nJobs = up8(std::min(h->nSeg, 2 * h->numCU)); // partial correlations per CPI (x2 modes in one workgroup)
  h->corrGrid = 0; // a forced grid was checked against the previous plan's nJobs
  h->firGrid = up8(std::min(h->nSeg, 8 * h->numCU));
  std::vector<cf> tw(h->F);
  for (int k = 0; k < h->F; k++) {
    const double a = -2.0 * M_PI * (double)k / (double)h->F;
    tw[k] = cmake((float)std::cos(a), (float)std::sin(a));
  }
  if (h->d_tw) CHIP(hipFree(h->d_tw));
  h->d_tw = nullptr;
  if (h->d_partial) CHIP(hipFree(h->d_partial));
  h->d_partial = nullptr;
  CHIP(multi_free(h)); // sized by this plan's job count: the next multi call builds them again
  CHIP(hipMalloc(&h->d_tw, h->F * sizeof(cf)));
  CHIP(hipMemcpy(h->d_tw, tw.data(), h->F * sizeof(cf), hipMemcpyHostToDevice));
  CHIP(hipMalloc(&h->d_partial, (size_t)h->maxBatch * 2 * h->nJobs * nBins * sizeof(cf)));
  return BLAH2HIP_OK;
}

// Workgroups per CPI of the correlation and FIR kernels at a batch of nCpi.  They shrink as the batch grows: a correlation
// workgroup ends with two inverse transforms and a partial write, a FIR workgroup starts with the transform of the taps --
// per-workgroup costs that a long walk over segments amortises.  Two resident generations' worth keeps the tail short.
// planned: the planner's nJobs whatever BLAH2HIP_CLUTTER_OPT_CORR_GRID says (multi_alloc: the buffer must hold those too)
void clutter_grids(const blah2hip_clutter_s *h, uint32_t nCpi, int *nJobs, int *firGrid, bool planned = false)
{
  const int perCpi = up8((2 * resident_slots(h) + (int)nCpi - 1) / (int)nCpi);
  *nJobs = std::min(h->nJobs, perCpi);
  *firGrid = std::min(h->firGrid, perCpi);
  if (h->corrGrid && !planned) *nJobs = h->corrGrid; // a multiple of 8 up to h->nJobs (blah2hip_clutter_set_option)
}

// The run-time transform length (r3 = F / 256) and sample format as compile-time arguments: f(R3, In) with R3 a
// std::integral_constant and In a value of the format's type.  WITH_I16 = false for the multi entry point, which has
// refused BLAH2HIP_FMT_I16 by then: nothing of its path is instantiated for InI16.
template <bool WITH_I16 = true, class F> int dispatch_r3_fmt(int r3, int fmt, F &&f)
{
  auto on_fmt = [&](auto R3) {
    if constexpr (WITH_I16)
      if (fmt == BLAH2HIP_FMT_I16) return f(R3, InI16{});
    if (fmt == BLAH2HIP_FMT_I8) return f(R3, InI8{});
    return f(R3, InC32{});
  };
  switch (r3) {
  case 4: return on_fmt(std::integral_constant<int, 4>{});
  case 8: return on_fmt(std::integral_constant<int, 8>{});
  default: return on_fmt(std::integral_constant<int, 16>{});
  }
}

// the plan's part of the correlation kernels' arguments; the caller adds the planes, the partials and their rows
CorrArgs corr_args(const blah2hip_clutter_s *h, const XsMap &xs, int nJobs, int64_t stride)
{
  CorrArgs ca{};
  ca.cpiStride = stride; ca.N = h->N; ca.xs = xs; ca.nBins = h->nBins; ca.nJobs = nJobs;
  ca.tw = h->d_tw; ca.scale = 1.0f / (float)h->F;
  if (h->corrHalf) {
    ca.half.nSeg = (int)((h->N + (uint32_t)(h->F / 2) - 1) / (uint32_t)(h->F / 2)); ca.half.per = (ca.half.nSeg + nJobs - 1) / nJobs;
  } else {
    ca.win.segLen = h->segLen; ca.win.nSeg = h->nSeg;
  }
  return ca;
}

// One correlation launch in the plan's form (windowed or half-window), with the LDS attribute of the instantiation it
// launches (once per (device, kernel), see context.hip).
//   pair: the per-channel call, r and b_0 into [nCpi][2][nJobs][nBins] (the half-window form has that layout compiled in);
//   otherwise a pass of the multi-channel call: withR -- r and b_0 -- or nb = 1 | 2 channels behind the first.
// The passes of the multi-channel call are not instantiated for InI16, whose words carry one surveillance channel.
template <int R3, class In> int launch_corr(blah2hip_clutter_s *h, const CorrArgs &ca, dim3 grid, bool withR, int nb, bool pair, hipStream_t st)
{
  auto go = [&](auto *kern) -> int {
    CHIP(blah2hip_ensure_lds_((const void *)kern, (int)fft_lds<R3>()));
    hipLaunchKernelGGL(kern, grid, dim3(WgFft<R3>::T), fft_lds<R3>(), st, ca);
    return BLAH2HIP_OK;
  };
  const bool half = h->corrHalf;
  if (pair) return half ? go(clutter_corr_half_kernel<R3, In, true, 1, true>) : go(clutter_corr_kernel<R3, In, true, 1>);
  if constexpr (!std::is_same<In, InI16>::value) {
    if (withR) return half ? go(clutter_corr_half_kernel<R3, In, true, 1>) : go(clutter_corr_kernel<R3, In, true, 1>);
    if (nb == 1) return half ? go(clutter_corr_half_kernel<R3, In, false, 1>) : go(clutter_corr_kernel<R3, In, false, 1>);
    return half ? go(clutter_corr_half_kernel<R3, In, false, 2>) : go(clutter_corr_kernel<R3, In, false, 2>);
  }
  CFAIL(BLAH2HIP_ERR_INVALID, "internal: BLAH2HIP_FMT_I16 has no multi-channel correlation");
}

// the plan's part of clutter_fir_kernel's arguments; the caller adds the planes, the taps and their flags
FirArgs fir_args(const blah2hip_clutter_s *h, const XsMap &xs, int64_t stride, int64_t outStride)
{
  FirArgs fa{};
  fa.cpiStride = stride; fa.outStride = outStride; fa.N = h->N; fa.xs = xs;
  fa.nBins = h->nBins; fa.segLen = h->segLen; fa.nSeg = h->nSeg; fa.tw = h->d_tw;
  fa.scale = 1.0f / (float)h->F;
  fa.carry = h->firCarry ? 1 : 0;
  return fa;
}

// stages: which of the three this call runs (the solve only behind the correlations).
// groups > 1 (the block form, launch_clutter_blocks, where the caller's CPIs do not lie back to back): the nCpi CPIs are
// `groups` runs of nCpi / groups CPIs, `stride` apart inside a run, run q starting groupStride samples behind run q - 1.
// The correlations are then one launch per run into that run's rows of the partials; the reduction and the solve stay one
// launch over all nCpi, and the grid per CPI is the one a single launch over nCpi has, so the results are its bits.
template <int R3, class In> int launch_clutter(blah2hip_clutter_s *h, const void *px, const void *py, uint32_t nCpi,
                                               int64_t stride, cf *yout, int64_t outStride, int32_t *ok, hipStream_t st,
                                               int stages = ALL_STAGES, uint32_t groups = 1, int64_t groupStride = 0)
{
  const XsMap xs = xs_map(h->delayMin, h->N);
  int nJobs, firGrid;
  clutter_grids(h, nCpi, &nJobs, &firGrid);
  if (stages & ESTIMATE_CORR) {
    h->lastCorrGrid = nJobs;
    CHIP(h->timer.tic(BLAH2HIP_CK_CORR, st));
    const uint32_t perRun = nCpi / groups;
    for (uint32_t q = 0; q < groups; q++) {
      // (bytes per sample: 8 for the fp32 planes and the int16 words, 2 for the int8 planes; py is NULL with the int16 words)
      const int64_t qoff = (int64_t)q * groupStride * BufChanOf<In>::X::STRIDE;
      const void *qx = (const char *)px + qoff;
      const void *qy = py ? (const char *)py + qoff : nullptr;
      CorrArgs ca = corr_args(h, xs, nJobs, stride);
      ca.x = qx; ca.y0 = ca.y1 = qy; ca.rows = 2; ca.row0 = 1; // r and b: [nCpi][2][nJobs][nBins]
      ca.partial = h->d_partial + (size_t)q * perRun * 2 * nJobs * h->nBins;
      { const int rc_ = launch_corr<R3, In>(h, ca, dim3(nJobs, perRun), true, 1, true, st); if (rc_) return rc_; }
    }
    CHIP(hipGetLastError());
    CHIP(h->timer.toc(BLAH2HIP_CK_CORR, st));

    SolveArgs sa;
    sa.partial = h->d_partial; sa.rb = h->d_rb; sa.w = h->d_w; sa.ok = ok; sa.nBins = h->nBins; sa.nJobs = nJobs;
    sa.epoch = h->d_epoch;
    CHIP(h->timer.tic(BLAH2HIP_CK_REDUCE, st));
    hipLaunchKernelGGL(clutter_reduce_kernel, dim3((h->nBins + 15) / 16, 2, nCpi), dim3(16 * RED_SLICES), 0, st, sa);
    CHIP(h->timer.toc(BLAH2HIP_CK_REDUCE, st));
    if (stages & ESTIMATE_SOLVE) { const int rc_ = launch_solve(h, sa, nCpi, st); if (rc_) return rc_; }
  }

  if (yout && (stages & FIR)) { // nullptr: the taps only (blah2hip_clutter_estimate_dev_fmt: the FIR runs fused into the range kernel)
    CHIP(blah2hip_ensure_lds_((const void *)clutter_fir_kernel<R3, In>, (int)fft_lds<R3>()));
    FirArgs fa = fir_args(h, xs, stride, outStride);
    fa.x = px; fa.y = py; fa.yout = yout; fa.w = h->d_w; fa.ok = ok;
    CHIP(h->timer.tic(BLAH2HIP_CK_FIR, st));
    hipLaunchKernelGGL((clutter_fir_kernel<R3, In>), dim3(firGrid, nCpi), dim3(WgFft<R3>::T), fft_lds<R3>(), st, fa);
    CHIP(hipGetLastError());
    CHIP(h->timer.toc(BLAH2HIP_CK_FIR, st));
  }
  note_last(h, ok, st);
  return BLAH2HIP_OK;
}

// the rule for clutter_corr_direct_kernel (a planner override of the correlation form takes the child back to the transforms)
inline bool corr_direct(const blah2hip_clutter_s *c)
{
  return c->blockChild && c->corrForce == BLAH2HIP_CLUTTER_CORR_AUTO && (uint64_t)c->N < 2ull * (uint64_t)c->nBins;
}

// ---- taps per block of the CPI -------------------------------------------------------------------------------------------
// Estimation: block j of CPI c is virtual CPI c B + j of the child handle (CPIs of L = N / B samples: shift and correlations
// circular inside the block), through the existing correlation, reduction and solve kernels.  Virtual CPI v starts at
// c stride + j L: where the caller's CPIs lie back to back (stride == N, or one CPI) that is ONE launch over nCpi B CPIs of
// stride L; otherwise one correlation launch per CPI (B virtual CPIs of stride L each) into that CPI's rows of the partials,
// and still one reduction and one solve over all of them (launch_clutter's `groups`).  Then clutter_fir_blocks_kernel.
template <int R3, class In> int launch_clutter_blocks(blah2hip_clutter_s *h, const void *px, const void *py, uint32_t nCpi,
                                                      int64_t stride, cf *yout, int64_t outStride, int32_t *ok, hipStream_t st)
{
  blah2hip_clutter_s *c = h->blk;
  const uint32_t B = h->nBlocks, L = h->N / B, V = nCpi * B;
  const bool flat = nCpi == 1 || stride == (int64_t)h->N;
  if (corr_direct(c)) { // short blocks: r and b lag by lag in fp64, straight into the solve's input
    CorrDirectArgs da;
    da.x = px; da.y = py; da.cpiStride = stride;
    da.xs = xs_map(c->delayMin, L);
    da.nBins = c->nBins; da.B = (int32_t)B; da.lagTiles = (c->nBins + 255) / 256; da.rb = c->d_rb;
    CHIP(c->timer.tic(BLAH2HIP_CK_CORR, st));
    hipLaunchKernelGGL((clutter_corr_direct_kernel<In>), dim3(V * (uint32_t)da.lagTiles, 2), dim3(256), 0, st, da);
    CHIP(hipGetLastError());
    CHIP(c->timer.toc(BLAH2HIP_CK_CORR, st));
    CHIP(c->timer.tic(BLAH2HIP_CK_REDUCE, st)); // nothing to reduce: the launch that bumps the look-ahead solve's epoch
    launch_solve_epoch(c->d_epoch, st);
    CHIP(c->timer.toc(BLAH2HIP_CK_REDUCE, st));
    { const int rc_ = launch_solve(c, solve_args(c, c->d_rb, c->d_w, ok), V, st); if (rc_) return rc_; }
    note_last(c, ok, st);
    c->lastCorrGrid = 0;
  } else {
    const int rc_ = launch_clutter<R3, In>(c, px, py, V, (int64_t)L, nullptr, 0, ok, st, ESTIMATE_CORR | ESTIMATE_SOLVE,
                                           flat ? 1u : nCpi, stride);
    if (rc_) return rc_;
  }
  note_last(h, ok, st);
  if (!yout) return BLAH2HIP_OK; // the taps only (blah2hip_clutter_estimate_dev_fmt)

  CHIP(blah2hip_ensure_lds_((const void *)clutter_fir_blocks_kernel<R3, In>, (int)fft_lds<R3>()));
  FirBlocksArgs fa;
  fa.x = px; fa.y = py; fa.yout = yout; fa.cpiStride = stride; fa.outStride = outStride;
  fa.xs = xs_map(h->delayMin, h->N);
  fa.nBins = c->nBins; fa.segLen = c->segLen; fa.nSeg = c->nSeg; // the child's plan: segments of a block
  fa.L = (int32_t)L; fa.B = (int32_t)B; fa.nVirt = (int32_t)V;
  // workgroups per virtual CPI: two resident generations over the launch (clutter_grids), at most one per segment
  fa.gx = std::max(1, std::min(c->nSeg, (2 * resident_slots(c) + (int)V - 1) / (int)V));
  fa.w = c->d_w; fa.ok = ok; fa.tw = c->d_tw; fa.scale = 1.0f / (float)c->F;
  const uint32_t grid = (V + 7) / 8 * 8 * (uint32_t)fa.gx;
  CHIP(h->timer.tic(BLAH2HIP_CK_FIR, st));
  hipLaunchKernelGGL((clutter_fir_blocks_kernel<R3, In>), dim3(grid), dim3(WgFft<R3>::T), fft_lds<R3>(), st, fa);
  CHIP(hipGetLastError());
  CHIP(h->timer.toc(BLAH2HIP_CK_FIR, st));
  return BLAH2HIP_OK;
}

// ---- several surveillance channels against one reference ----------------------------------------------------------------
// Buffers for K channels (the first multi call, one that asks for more channels than the handle has seen, or the first
// with a forced correlation grid that the partials do not hold): blocking.
int multi_alloc(blah2hip_clutter_s *h, uint32_t K)
{
  const size_t forced = (size_t)h->maxBatch * (size_t)h->corrGrid;
  if (K <= h->multiK && forced <= h->multiJobs) return BLAH2HIP_OK;
  // the largest n_cpi x (workgroups per CPI) a launch can have: by the planner's grids always (a forced grid may be taken
  // back with the buffers in place), and by a forced grid at the whole batch where that is more
  size_t jobs = 0;
  if (!h->subCorr) {
    for (uint32_t c = 1; c <= h->maxBatch; c++) {
      int nJobs, firGrid;
      clutter_grids(h, c, &nJobs, &firGrid, true);
      jobs = std::max(jobs, (size_t)c * nJobs);
    }
    jobs = std::max(jobs, forced);
  }
  K = std::max(K, h->multiK);
  CHIP(hipDeviceSynchronize()); // smaller buffers may still be in use by enqueued work
  CHIP(multi_free(h));
  const size_t rows = (K + 2) & ~1u, n = (size_t)h->nBins;
  if (!h->subCorr) {
    CHIP(hipMalloc(&h->d_partialM, jobs * rows * n * sizeof(cf)));
    CHIP(hipMemset(h->d_partialM, 0, jobs * rows * n * sizeof(cf))); // (the padding row of an even K is summed like the others)
    h->multiJobs = jobs;
  }
  CHIP(hipMalloc(&h->d_rbM, (size_t)h->maxBatch * rows * n * sizeof(dcx)));
  CHIP(hipMemset(h->d_rbM, 0, (size_t)h->maxBatch * rows * n * sizeof(dcx)));
  CHIP(hipMalloc(&h->d_wM, (size_t)K * h->maxBatch * n * sizeof(cf)));
  CHIP(hipMalloc(&h->d_okM, (size_t)K * h->maxBatch * sizeof(int32_t)));
  h->multiK = K;
  return BLAH2HIP_OK;
}

// launch_clutter for K channels: correlations (the reference's part once per pass), one reduction over 1 + K rows per CPI,
// one recursion per CPI with K right-hand sides, then the FIR kernel per channel.  Everything sized by nCpi as launch_clutter
// sizes it.  ok: [K][nCpi].
template <int R3, class In> int launch_clutter_multi(blah2hip_clutter_s *h, const void *px, const void *const *pys, uint32_t K,
                                                     uint32_t nCpi, int64_t stride, void *const *youts, int64_t outStride,
                                                     int32_t *ok, hipStream_t st)
{
  const XsMap xs = xs_map(h->delayMin, h->N);
  int nJobs, firGrid;
  clutter_grids(h, nCpi, &nJobs, &firGrid);
  h->lastCorrGrid = nJobs;
  const int rows = (int)((K + 2) & ~1u);

  CorrArgs ca = corr_args(h, xs, nJobs, stride);
  ca.x = px; ca.partial = h->d_partialM; ca.rows = rows;
  CHIP(h->timer.tic(BLAH2HIP_CK_CORR, st));
  for (uint32_t k = 0; k < K;) { // r and b_0, then the other channels in pairs
    const uint32_t nb = k == 0 ? 1u : std::min<uint32_t>(CORR_TILE, K - k);
    ca.y0 = pys[k]; ca.y1 = pys[k + nb - 1]; ca.row0 = 1 + (int)k;
    { const int rc_ = launch_corr<R3, In>(h, ca, dim3(nJobs, nCpi), k == 0, (int)nb, false, st); if (rc_) return rc_; }
    k += nb;
  }
  CHIP(hipGetLastError());
  CHIP(h->timer.toc(BLAH2HIP_CK_CORR, st));

  // clutter_reduce_kernel sums pairs of rows: [nCpi][rows] is [nCpi rows / 2][2]
  SolveArgs ra;
  ra.partial = h->d_partialM; ra.rb = h->d_rbM; ra.w = nullptr; ra.ok = nullptr; ra.nBins = h->nBins; ra.nJobs = nJobs;
  ra.epoch = nullptr; // the look-ahead solve's mailboxes are not used here
  CHIP(h->timer.tic(BLAH2HIP_CK_REDUCE, st));
  hipLaunchKernelGGL(clutter_reduce_kernel, dim3((h->nBins + 15) / 16, 2, nCpi * (uint32_t)(rows / 2)), dim3(16 * RED_SLICES), 0, st, ra);
  CHIP(hipGetLastError());
  CHIP(h->timer.toc(BLAH2HIP_CK_REDUCE, st));

  SolveMultiArgs ma;
  ma.rb = h->d_rbM; ma.w = h->d_wM; ma.ok = ok; ma.nBins = h->nBins; ma.rows = rows; ma.nSurv = (int)K; ma.nCpi = (int)nCpi;
  CHIP(h->timer.tic(BLAH2HIP_CK_SOLVE, st));
  { const int rc_ = launch_solve_multi(h, ma, st); if (rc_) return rc_; }
  CHIP(hipGetLastError());
  CHIP(h->timer.toc(BLAH2HIP_CK_SOLVE, st));
  h->lastForm = BLAH2HIP_CLUTTER_SOLVE_STEPWISE; h->lastE = 0; h->lastG = 1;

  if (youts) { // the taps only otherwise (as blah2hip_clutter_estimate_dev_fmt)
    CHIP(blah2hip_ensure_lds_((const void *)clutter_fir_kernel<R3, In, true>, (int)fft_lds<R3>()));
    FirArgs fa = fir_args(h, xs, stride, outStride);
    fa.x = px;
    CHIP(h->timer.tic(BLAH2HIP_CK_FIR, st));
    for (uint32_t k = 0; k < K; k++) {
      fa.y = pys[k]; fa.yout = (cf *)youts[k]; fa.w = h->d_wM + (size_t)k * nCpi * h->nBins; fa.ok = ok + (size_t)k * nCpi;
      hipLaunchKernelGGL((clutter_fir_kernel<R3, In, true>), dim3(firGrid, nCpi), dim3(WgFft<R3>::T), fft_lds<R3>(), st, fa);
    }
    CHIP(hipGetLastError());
    CHIP(h->timer.toc(BLAH2HIP_CK_FIR, st));
  }
  return BLAH2HIP_OK;
}

// A long filter (clutter_kernels.hpp, "LONG filters"): the correlations chunk by chunk on subCorr, one solve of all nBins
// orders on this handle, the FIR chunk by chunk on subFir.  skipBad: the multi entry point leaves CPIs that are not
// positive definite unwritten.
int long_process(blah2hip_clutter_s *h, const cf *d_x, const cf *d_y, uint32_t nCpi, int64_t stride, cf *yout, int64_t outStride,
                 int32_t *ok, hipStream_t st, bool skipBad = false)
{
  const uint32_t N = h->N, dmin = (uint32_t)h->delayMin;
  const int n = h->nBins, C = LONG_C;
  const size_t plane = (size_t)h->maxBatch * N;
  cf *xp = h->d_long, *yp = xp + plane, *wp = yp + plane;
  const dim3 pg((N + 255) / 256, nCpi), gg((C + 255) / 256, nCpi);
  blah2hip_clutter_s *sc = h->subCorr, *sf = h->subFir;
  // private copies with the children's stride (the caller's may differ from N); the output is built in the copy of y.
  // A lone CPI has no second row: the entry points take any stride with it (0 included), and a pitch below the row width
  // is refused by the runtime, so the pitches are N there.
  const size_t inPitch = (nCpi == 1 ? (size_t)N : (size_t)stride) * sizeof(cf), outPitch = (nCpi == 1 ? (size_t)N : (size_t)outStride) * sizeof(cf);
  CHIP(hipMemcpy2DAsync(xp, (size_t)N * sizeof(cf), d_x, inPitch, (size_t)N * sizeof(cf), nCpi, hipMemcpyDeviceToDevice, st));
  CHIP(hipMemcpy2DAsync(yp, (size_t)N * sizeof(cf), d_y, inPitch, (size_t)N * sizeof(cf), nCpi, hipMemcpyDeviceToDevice, st));
  // the child's correlations of xp against the plane `other`, its r or b (long_gather_kernel's `which`) into chunk c of ours
  auto corr_pass = [&](const cf *other, int c, int which) -> int {
    const int rc = launch_clutter<16, InC32>(sc, xp, other, nCpi, (int64_t)N, nullptr, 0, ok, st, ESTIMATE_CORR);
    if (rc) return rc;
    long_gather_kernel<<<gg, 256, 0, st>>>(sc->d_rb, h->d_rb, C, n, c, which);
    return BLAH2HIP_OK;
  };
  for (int c = 0; c < h->nChunks; c++) {
    if (c > 0) long_plane_kernel<0><<<pg, 256, 0, st>>>(yp, wp, N, (uint32_t)(c * C), 0u);
    int rc = corr_pass(c > 0 ? wp : yp, c, 0);
    if (rc) return rc;
    if (c == 0) {
      long_gather_kernel<<<gg, 256, 0, st>>>(sc->d_rb, h->d_rb, C, n, c, 1);
    } else {
      long_plane_kernel<1><<<pg, 256, 0, st>>>(xp, wp, N, (uint32_t)(c * C), dmin);
      rc = corr_pass(wp, c, 2);
      if (rc) return rc;
    }
    CHIP(hipGetLastError());
  }
  { const int rc = launch_solve(h, solve_args(h, h->d_rb, h->d_w, ok), nCpi, st); if (rc) return rc; }
  if (yout) {
    CHIP(h->timer.tic(BLAH2HIP_CK_FIR, st));
    for (int c = 0; c < h->nChunks; c++) {
      long_taps_kernel<<<gg, 256, 0, st>>>(h->d_w, sf->d_w, C, n, c);
      long_plane_kernel<2><<<pg, 256, 0, st>>>(xp, wp, N, (uint32_t)(c * C), dmin);
      CHIP(hipGetLastError());
      const int rc = launch_clutter<16, InC32>(sf, wp, yp, nCpi, (int64_t)N, yp, (int64_t)N, ok, st, FIR); // in place: y -= w_c * xs_c
      if (rc) return rc;
    }
    if (skipBad) {
      long_out_kernel<<<pg, 256, 0, st>>>(yp, yout, N, outStride, ok);
      CHIP(hipGetLastError());
    } else {
      CHIP(hipMemcpy2DAsync(yout, outPitch, yp, (size_t)N * sizeof(cf), (size_t)N * sizeof(cf), nCpi, hipMemcpyDeviceToDevice, st));
    }
    CHIP(h->timer.toc(BLAH2HIP_CK_FIR, st));
  }
  note_last(h, ok, st);
  return BLAH2HIP_OK;
}

// blah2hip_clutter_process_dev_fmt, and with `estimate` blah2hip_clutter_estimate_dev_fmt: no output plane, the taps only
int filter_one_channel(blah2hip_clutter_t h, int fmt, const void *d_x, const void *d_y, uint32_t n_cpi, uint64_t cpi_stride,
                       void *d_y_out, uint64_t out_stride, int32_t *d_ok, void *stream, bool estimate)
{
  if (!h || !d_x || (!estimate && !d_y_out)) CFAIL(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (fmt != BLAH2HIP_FMT_C32 && fmt != BLAH2HIP_FMT_I16 && fmt != BLAH2HIP_FMT_I8)
    CFAIL(BLAH2HIP_ERR_INVALID, "clutter filter input: BLAH2HIP_FMT_C32, BLAH2HIP_FMT_I16 or BLAH2HIP_FMT_I8");
  if (fmt != BLAH2HIP_FMT_I16 && !d_y) CFAIL(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (n_cpi == 0 || n_cpi > h->maxBatch) CFAIL(BLAH2HIP_ERR_INVALID, "n_cpi outside [1, max_batch]");
  if (estimate) {
    if (n_cpi > 1 && cpi_stride < h->N) CFAIL(BLAH2HIP_ERR_INVALID, "cpi_stride < nSamples");
  } else {
#ifndef B2_EXPERIMENT_ALIASED_CPIS // tools/gpu_cfg3_bytes.py
    if (n_cpi > 1 && (cpi_stride < h->N || out_stride < h->N)) CFAIL(BLAH2HIP_ERR_INVALID, "cpi_stride / out_stride < nSamples");
#endif
  }
  CHIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  int32_t *ok = d_ok ? d_ok : (h->blk ? h->blk->d_ok : h->d_ok);
  // in-place operation (FMT_C32, d_y_out == d_y) is safe: every output sample is read (as y) by the one
  // thread that writes it, and x is never written
  const int64_t cs = (int64_t)cpi_stride, os = (int64_t)out_stride;
  cf *yo = (cf *)d_y_out;
  if (fmt == BLAH2HIP_FMT_I16) d_y = nullptr; // the surveillance channel rides in the reference's words
  if (h->blk) // d_ok: [n_cpi][n_blocks]
    return dispatch_r3_fmt(h->blk->r3, fmt, [&](auto R3, auto in) {
      return launch_clutter_blocks<decltype(R3)::value, decltype(in)>(h, d_x, d_y, n_cpi, cs, yo, os, ok, st);
    });
  if (h->subCorr) {
    if (fmt == BLAH2HIP_FMT_I8) CFAIL(BLAH2HIP_ERR_UNSUPPORTED, "a long filter (more than 4081 taps) takes fp32 planes only, not BLAH2HIP_FMT_I8");
    if (fmt != BLAH2HIP_FMT_C32) CFAIL(BLAH2HIP_ERR_UNSUPPORTED, "a long filter (more than 4081 taps) takes fp32 planes only");
    return long_process(h, (const cf *)d_x, (const cf *)d_y, n_cpi, cs, yo, os, ok, st);
  }
  return dispatch_r3_fmt(h->r3, fmt, [&](auto R3, auto in) {
    return launch_clutter<decltype(R3)::value, decltype(in)>(h, d_x, d_y, n_cpi, cs, yo, os, ok, st);
  });
}

// what blah2hip_clutter_create and _create_ex both ask of the filter's geometry
int check_geometry(int32_t delay_min, int32_t delay_max, uint32_t n_samples)
{
  if (delay_max <= delay_min) CFAIL(BLAH2HIP_ERR_INVALID, "clutter filter needs delayMax > delayMin");
  if (n_samples > 0x7fffffffu - 8192u) CFAIL(BLAH2HIP_ERR_UNSUPPORTED, "nSamples >= 2^31 - 8192 (32-bit sample indices)");
  return BLAH2HIP_OK;
}

// blah2hip_clutter_set_option, an input of the plan: set it, wait for enqueued work (the buffers may still be in use) and
// plan again; where that fails, back to the previous, valid plan with the first failure's code and text
template <class T> int replan_with(blah2hip_clutter_s *h, T &field, T value)
{
  const T prev = field;
  field = value;
  CHIP(hipSetDevice(h->device));
  CHIP(hipDeviceSynchronize());
  const int rc = clutter_plan(h);
  if (rc) {
    const std::string msg = blah2hip_last_error();
    field = prev;
    (void)clutter_plan(h);
    blah2hip_set_error_(msg.c_str());
  }
  return rc;
}

} // namespace

extern "C" {

int blah2hip_clutter_create(int32_t delay_min, int32_t delay_max, uint32_t n_samples, int device,
                            uint32_t max_batch, blah2hip_clutter_t *out)
{
  if (!out) CFAIL(BLAH2HIP_ERR_INVALID, "out is NULL");
  *out = nullptr;
  { const int rc_ = check_geometry(delay_min, delay_max, n_samples); if (rc_) return rc_; }
  if (n_samples == 0) CFAIL(BLAH2HIP_ERR_INVALID, "nSamples must be positive");
  if ((uint64_t)(delay_min < 0 ? -(int64_t)delay_min : (int64_t)delay_min) >= n_samples)
    CFAIL(BLAH2HIP_ERR_INVALID, "|delayMin| >= nSamples");
  const int nBins = delay_max - delay_min;
  if (max_batch == 0) max_batch = 1;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    CFAIL(BLAH2HIP_ERR_NO_DEVICE, "no HIP device visible (the HIP path is the only path)");
  if (device < 0 || device >= ndev) CFAIL(BLAH2HIP_ERR_INVALID, "device index out of range");
  CHIP(hipSetDevice(device));
  // beyond one transform (nBins > F - 15 = 4081): the long form, chunks of LONG_C taps on two child handles (long_process);
  // its one-workgroup solve holds one fp64 vector of nBins in LDS, eight indices per thread
  const bool isLong = nBins > 4096 - 15;
  // (more taps than samples: the reference reads its nSamples correlation lags out of bounds, WienerHopf.cpp:76-108)
  if (isLong && (uint32_t)nBins > n_samples) CFAIL(BLAH2HIP_ERR_UNSUPPORTED, "a long filter (more than 4081 taps) needs nBins <= nSamples");
  if ((uint32_t)nBins > n_samples) CFAIL(BLAH2HIP_ERR_INVALID, "more taps than samples: the clutter filter needs delayMax - delayMin <= nSamples");
  auto *h = new blah2hip_clutter_s;
  // everything that can fail runs inside `build`; a partially built handle is torn down by destroy()
  auto build = [&]() -> int {
  h->device = device;
  h->delayMin = delay_min; h->delayMax = delay_max;
  h->N = n_samples; h->maxBatch = max_batch; h->nBins = nBins;
  hipDeviceProp_t prop;
  CHIP(hipGetDeviceProperties(&prop, device));
  h->numCU = prop.multiProcessorCount;
  CHIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  CHIP(hipMalloc(&h->d_rb, (size_t)max_batch * 2 * nBins * sizeof(dcx)));
  CHIP(hipMalloc(&h->d_w, (size_t)max_batch * nBins * sizeof(cf)));
  CHIP(hipMalloc(&h->d_ok, max_batch * sizeof(int32_t)));
  if (isLong) {
    h->nChunks = (nBins + LONG_C - 1) / LONG_C;
    h->solveForm = BLAH2HIP_CLUTTER_SOLVE_STEPWISE;
    { const int rc_ = blah2hip_clutter_create(delay_min, delay_min + LONG_C, n_samples, device, max_batch, &h->subCorr); if (rc_) return rc_; }
    { const int rc_ = blah2hip_clutter_create(0, LONG_C, n_samples, device, max_batch, &h->subFir); if (rc_) return rc_; }
    h->r3 = h->subFir->r3; h->F = h->subFir->F; h->segLen = h->subFir->segLen; h->nSeg = h->subFir->nSeg;
    CHIP(hipMalloc(&h->d_long, (size_t)3 * max_batch * n_samples * sizeof(cf)));
    CHIP(hipMalloc(&h->d_solveWs, (size_t)max_batch * (4 * (size_t)nBins + 2) * sizeof(dcx)));
    CHIP(hipMalloc(&h->d_epoch, 4 * sizeof(uint32_t)));
    CHIP(hipMemset(h->d_epoch, 0, 4 * sizeof(uint32_t)));
    return BLAH2HIP_OK;
  }
  { const int rc_ = clutter_plan(h); if (rc_) return rc_; }
  { const int rc_ = solve_la_alloc(h); if (rc_) return rc_; }
  return BLAH2HIP_OK;
  };
  const int rc = build();
  if (rc != BLAH2HIP_OK) {
    blah2hip_clutter_destroy(h);
    return rc;
  }
  *out = h;
  return BLAH2HIP_OK;
}

int blah2hip_clutter_create_ex(int32_t delay_min, int32_t delay_max, uint32_t n_samples, uint32_t n_blocks, int device,
                               uint32_t max_batch, blah2hip_clutter_t *out)
{
  if (!out) CFAIL(BLAH2HIP_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (n_blocks == 0) CFAIL(BLAH2HIP_ERR_INVALID, "n_blocks must be positive");
  if (n_samples % n_blocks != 0) CFAIL(BLAH2HIP_ERR_INVALID, "nSamples is not a multiple of n_blocks (equal blocks only)");
  if (n_blocks == 1) return blah2hip_clutter_create(delay_min, delay_max, n_samples, device, max_batch, out);
  { const int rc_ = check_geometry(delay_min, delay_max, n_samples); if (rc_) return rc_; }
  if (max_batch == 0) max_batch = 1;
  if ((uint64_t)max_batch * n_blocks > 0x7fffffffull) CFAIL(BLAH2HIP_ERR_INVALID, "max_batch * n_blocks exceeds 2^31 - 1");
  const int64_t nBins = (int64_t)delay_max - delay_min;
  const uint32_t L = n_samples / n_blocks;
  if (nBins > 4096 - 15) CFAIL(BLAH2HIP_ERR_UNSUPPORTED, "a long filter (more than 4081 taps) has no block form");
  // (the reference reads its correlation lags out of bounds on a block shorter than the filter, WienerHopf.cpp:76-108)
  if ((int64_t)L < nBins) CFAIL(BLAH2HIP_ERR_UNSUPPORTED, "blocks shorter than the filter: nSamples / n_blocks < delayMax - delayMin");
  blah2hip_clutter_t blk = nullptr;
  // everything of the estimation: the plan for CPIs of L samples and its checks (|delayMin| < L, device, ...)
  { const int rc_ = blah2hip_clutter_create(delay_min, delay_max, L, device, max_batch * n_blocks, &blk); if (rc_) return rc_; }
  blk->blockChild = true;
  { const int rc_ = solve_la_alloc(blk); if (rc_) { blah2hip_clutter_destroy(blk); return rc_; } } // mailboxes for every plan such a handle can be given
  auto *h = new blah2hip_clutter_s;
  h->device = device;
  h->delayMin = delay_min; h->delayMax = delay_max;
  h->N = n_samples; h->maxBatch = max_batch; h->nBins = (int32_t)nBins;
  h->nBlocks = n_blocks; h->blk = blk;
  h->numCU = blk->numCU;
  const hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    blah2hip_set_error_((std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(e)).c_str());
    blah2hip_clutter_destroy(h);
    return BLAH2HIP_ERR_HIP;
  }
  *out = h;
  return BLAH2HIP_OK;
}

int blah2hip_clutter_destroy(blah2hip_clutter_t h)
{
  if (!h) return BLAH2HIP_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->blk) (void)blah2hip_clutter_destroy(h->blk);
  if (h->subCorr) (void)blah2hip_clutter_destroy(h->subCorr);
  if (h->subFir) (void)blah2hip_clutter_destroy(h->subFir);
  for (void *p : {(void *)h->d_tw, (void *)h->d_partial, (void *)h->d_rb, (void *)h->d_w, (void *)h->d_ok,
                  (void *)h->d_stage, (void *)h->d_mail, (void *)h->d_epoch, (void *)h->d_long, (void *)h->d_solveWs,
                  (void *)h->d_partialM, (void *)h->d_rbM, (void *)h->d_wM, (void *)h->d_okM})
    if (p) (void)hipFree(p);
  h->timer.destroy();
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return BLAH2HIP_OK;
}

int blah2hip_clutter_get_dims(blah2hip_clutter_t h, uint32_t *n_bins, uint32_t *fft_len, uint32_t *seg_len)
{
  if (!h) CFAIL(BLAH2HIP_ERR_INVALID, "NULL handle");
  const blah2hip_clutter_s *p = h->blk ? h->blk : h; // blocks: the plan is the block's
  if (n_bins) *n_bins = (uint32_t)p->nBins;
  if (fft_len) *fft_len = (uint32_t)p->F;
  if (seg_len) *seg_len = (uint32_t)p->segLen;
  return BLAH2HIP_OK;
}

int blah2hip_clutter_get_info(blah2hip_clutter_t h, int what, int64_t *value)
{
  if (!h || !value) CFAIL(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (what == BLAH2HIP_CLUTTER_INFO_BLOCKS) { *value = h->nBlocks; return BLAH2HIP_OK; }
  if (h->blk) { // the estimation is the child's; the block FIR reads every window whole
    if (what == BLAH2HIP_CLUTTER_INFO_FIR_CARRY) { *value = 0; return BLAH2HIP_OK; }
    return blah2hip_clutter_get_info(h->blk, what, value);
  }
  switch (what) {
  case BLAH2HIP_CLUTTER_INFO_SOLVE_FORM: *value = h->lastForm; return BLAH2HIP_OK;
  case BLAH2HIP_CLUTTER_INFO_SOLVE_E: *value = h->lastE; return BLAH2HIP_OK;
  case BLAH2HIP_CLUTTER_INFO_SOLVE_G: *value = h->lastG; return BLAH2HIP_OK;
  case BLAH2HIP_CLUTTER_INFO_CORR_FORM: { // the long form's correlations are its first child's
    const blah2hip_clutter_s *p = h->subCorr ? h->subCorr : h;
    *value = corr_direct(p) ? BLAH2HIP_CLUTTER_CORR_DIRECT : (p->corrHalf ? BLAH2HIP_CLUTTER_CORR_HALF : BLAH2HIP_CLUTTER_CORR_WINDOW);
    return BLAH2HIP_OK;
  }
  case BLAH2HIP_CLUTTER_INFO_FIR_CARRY: *value = (h->subFir ? h->subFir : h)->firCarry ? 1 : 0; return BLAH2HIP_OK;
  case BLAH2HIP_CLUTTER_INFO_CHUNKS: *value = h->nChunks; return BLAH2HIP_OK;
  case BLAH2HIP_CLUTTER_INFO_CORR_GRID: *value = (h->subCorr ? h->subCorr : h)->lastCorrGrid; return BLAH2HIP_OK;
  case BLAH2HIP_CLUTTER_INFO_SOLVE_FAULT:
  case BLAH2HIP_CLUTTER_INFO_SOLVE_RETRIES: {
    // the stream the handle's last call ran on, not the device (a poll in a pipeline must not stall other streams and
    // handles); both words in one copy
    uint32_t v[2] = {0, 0};
    CHIP(hipSetDevice(h->device));
    CHIP(hipStreamSynchronize(h->lastStream));
    if (h->d_epoch) CHIP(hipMemcpy(v, h->d_epoch + 1, sizeof v, hipMemcpyDeviceToHost));
    *value = what == BLAH2HIP_CLUTTER_INFO_SOLVE_FAULT ? v[0] : v[1];
    return BLAH2HIP_OK;
  }
  default: CFAIL(BLAH2HIP_ERR_INVALID, "unknown info");
  }
}

int blah2hip_clutter_read_last(blah2hip_clutter_t h, uint32_t cpi, float *w, double *rb, int *ok)
{
  if (!h) CFAIL(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (h->blk) return blah2hip_clutter_read_last(h->blk, cpi, w, rb, ok); // virtual CPI c n_blocks + j
  const bool multi = h->lastSurv != 0; // behind a multi call: virtual CPI k n_cpi + c, in the multi buffers
  if (multi && cpi >= h->lastSurv * h->lastNCpi) CFAIL(BLAH2HIP_ERR_INVALID, "cpi index out of range (virtual CPIs of the last multi call)");
  if (!multi && cpi >= h->maxBatch) CFAIL(BLAH2HIP_ERR_INVALID, "cpi index out of range");
  CHIP(hipSetDevice(h->device));
  CHIP(hipDeviceSynchronize());
  const size_t n = (size_t)h->nBins;
  if (w) CHIP(hipMemcpy(w, (multi ? h->d_wM : h->d_w) + (size_t)cpi * n, n * sizeof(cf), hipMemcpyDeviceToHost));
  if (rb && multi) {
    const size_t k = cpi / h->lastNCpi, c = cpi % h->lastNCpi, rows = (h->lastSurv + 2) & ~1u;
    CHIP(hipMemcpy(rb, h->d_rbM + c * rows * n, n * sizeof(dcx), hipMemcpyDeviceToHost));
    CHIP(hipMemcpy(rb + 2 * n, h->d_rbM + (c * rows + 1 + k) * n, n * sizeof(dcx), hipMemcpyDeviceToHost));
  } else if (rb) {
    CHIP(hipMemcpy(rb, h->d_rb + (size_t)cpi * 2 * n, 2 * n * sizeof(dcx), hipMemcpyDeviceToHost));
  }
  if (ok) {
    int32_t v = 0;
    if (!h->lastOk) CFAIL(BLAH2HIP_ERR_INVALID, "no process call yet"); // (a multi call has set it)
    CHIP(hipMemcpy(&v, h->lastOk + cpi, sizeof(int32_t), hipMemcpyDeviceToHost));
    *ok = v;
  }
  return BLAH2HIP_OK;
}

int blah2hip_clutter_set_option(blah2hip_clutter_t h, int option, int64_t value)
{
  if (!h) CFAIL(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (h->blk) return blah2hip_clutter_set_option(h->blk, option, value); // the plan (for CPIs of one block) and the solve are the child's
  if (h->subCorr) CFAIL(BLAH2HIP_ERR_UNSUPPORTED, "a long filter (more than 4081 taps) has one plan: no options");
  switch (option) {
  case BLAH2HIP_CLUTTER_OPT_SOLVE_K:
    if (value != 0 && value != 1 && value != 2 && value != 4) CFAIL(BLAH2HIP_ERR_INVALID, "indices per thread: 0 (auto), 1, 2 or 4");
    if (value && (int64_t)h->nBins > 1024 * value) CFAIL(BLAH2HIP_ERR_UNSUPPORTED, "nBins needs more indices per thread");
    h->solveK = (int)value;
    return BLAH2HIP_OK;
  case BLAH2HIP_CLUTTER_OPT_SOLVE_FORM:
    if (value < BLAH2HIP_CLUTTER_SOLVE_AUTO || value > BLAH2HIP_CLUTTER_SOLVE_LOOKAHEAD)
      CFAIL(BLAH2HIP_ERR_INVALID, "solve form: BLAH2HIP_CLUTTER_SOLVE_AUTO, _STEPWISE or _LOOKAHEAD");
    h->solveForm = (int)value;
    return BLAH2HIP_OK;
  case BLAH2HIP_CLUTTER_OPT_SOLVE_E: {
    if (value != 0 && value != 2 && value != 3 && value != 6 && value != 12)
      CFAIL(BLAH2HIP_ERR_INVALID, "indices per lane of the look-ahead solve: 0 (by launch size), 2, 3, 6 or 12");
    const int prev = h->solveE;
    h->solveE = (int)value;
    CHIP(hipSetDevice(h->device));
    CHIP(hipDeviceSynchronize()); // the mailboxes may still be in use by enqueued work
    const int rc = solve_la_alloc(h);
    if (rc) h->solveE = prev;
    return rc;
  }
  case BLAH2HIP_CLUTTER_OPT_SOLVE_SPIN_LIMIT:
    if (value < 0 || value > (int64_t)0x7fffffff) CFAIL(BLAH2HIP_ERR_INVALID, "polls per bounded wait: 0 (default) ... 2^31 - 1");
    h->spinLimit = (uint32_t)value;
    return BLAH2HIP_OK;
  case BLAH2HIP_CLUTTER_OPT_CORR_GRID:
    if (value != 0 && (value < 8 || value > (int64_t)h->nJobs || (value & 7))) {
      const std::string msg = "correlation grid: 0 (planner) or a multiple of 8 from 8 to " + std::to_string(h->nJobs) +
                              ", the plan's workgroups per CPI";
      CFAIL(BLAH2HIP_ERR_INVALID, msg.c_str());
    }
    h->corrGrid = (int)value; // (the multi-channel partials follow in multi_alloc, at the next multi call)
    return BLAH2HIP_OK;
  case BLAH2HIP_CLUTTER_OPT_FIR_CARRY:
    if (value != 0 && value != 1) CFAIL(BLAH2HIP_ERR_INVALID, "FIR carry: 0 or 1");
    return replan_with(h, h->firNoCarry, value == 0);
  case BLAH2HIP_CLUTTER_OPT_FFT_LEN:
    if (value != 0 && value != 1024 && value != 2048 && value != 4096)
      CFAIL(BLAH2HIP_ERR_INVALID, "clutter transform length: 0 (planner), 1024, 2048 or 4096");
    return replan_with(h, h->fftLenForce, (int)value);
  case BLAH2HIP_CLUTTER_OPT_CORR:
    if (value < BLAH2HIP_CLUTTER_CORR_AUTO || value > BLAH2HIP_CLUTTER_CORR_WINDOW)
      CFAIL(BLAH2HIP_ERR_INVALID, "correlation form: BLAH2HIP_CLUTTER_CORR_AUTO, _HALF or _WINDOW");
    return replan_with(h, h->corrForce, (int)value);
  default: CFAIL(BLAH2HIP_ERR_INVALID, "unknown option");
  }
}

int blah2hip_clutter_set_timing(blah2hip_clutter_t h, int enable)
{
  if (!h) CFAIL(BLAH2HIP_ERR_INVALID, "NULL handle");
  h->timer.enabled = enable != 0;
  if (h->subCorr) h->subCorr->timer.enabled = enable != 0; // the long form: correlations and reduction are the child's launches
  if (h->blk) h->blk->timer.enabled = enable != 0;         // blocks: everything but the FIR
  return BLAH2HIP_OK;
}

int blah2hip_clutter_get_timing(blah2hip_clutter_t h, double *ms_total, uint32_t *launches)
{
  if (!h || !ms_total || !launches) CFAIL(BLAH2HIP_ERR_INVALID, "NULL argument");
  CHIP(hipSetDevice(h->device));
  CHIP(hipDeviceSynchronize());
  CHIP(h->timer.collect(ms_total, launches));
  auto add_child_timing = [&](blah2hip_clutter_s *child, std::initializer_list<int> kinds) -> int {
    double ms[BLAH2HIP_CK_COUNT];
    uint32_t nl[BLAH2HIP_CK_COUNT];
    CHIP(child->timer.collect(ms, nl));
    for (int k : kinds) { ms_total[k] += ms[k]; launches[k] += nl[k]; }
    return BLAH2HIP_OK;
  };
  // the long form: correlations + reduction are the first child's (its FIR passes and solve are bracketed on this handle)
  if (h->subCorr) { const int rc_ = add_child_timing(h->subCorr, {BLAH2HIP_CK_CORR, BLAH2HIP_CK_REDUCE}); if (rc_) return rc_; }
  // blocks: correlations, reduction and solve are bracketed on the child, the FIR on this handle
  if (h->blk) { const int rc_ = add_child_timing(h->blk, {BLAH2HIP_CK_CORR, BLAH2HIP_CK_REDUCE, BLAH2HIP_CK_SOLVE}); if (rc_) return rc_; }
  return BLAH2HIP_OK;
}

int blah2hip_clutter_process_dev_fmt(blah2hip_clutter_t h, int fmt, const void *d_x, const void *d_y, uint32_t n_cpi,
                                     uint64_t cpi_stride, void *d_y_out, uint64_t out_stride, int32_t *d_ok, void *stream)
{
  return filter_one_channel(h, fmt, d_x, d_y, n_cpi, cpi_stride, d_y_out, out_stride, d_ok, stream, false);
}

int blah2hip_clutter_estimate_dev_fmt(blah2hip_clutter_t h, int fmt, const void *d_x, const void *d_y, uint32_t n_cpi,
                                      uint64_t cpi_stride, int32_t *d_ok, void *stream)
{
  return filter_one_channel(h, fmt, d_x, d_y, n_cpi, cpi_stride, nullptr, 0, d_ok, stream, true);
}

int blah2hip_clutter_process_multi_dev_fmt(blah2hip_clutter_t h, int fmt, const void *d_x, const void *const *d_y, uint32_t n_surv,
                                           uint32_t n_cpi, uint64_t cpi_stride, void *const *d_y_out, uint64_t out_stride,
                                           int32_t *d_ok, void *stream)
{
  if (!h || !d_x || !d_y) CFAIL(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (h->blk) CFAIL(BLAH2HIP_ERR_UNSUPPORTED, "taps per block (n_blocks > 1) have no form for several surveillance channels");
  if (fmt == BLAH2HIP_FMT_I16)
    CFAIL(BLAH2HIP_ERR_UNSUPPORTED, "BLAH2HIP_FMT_I16 carries one surveillance channel in the reference's words: several channels need planes of their own");
  if (fmt != BLAH2HIP_FMT_C32 && fmt != BLAH2HIP_FMT_I8)
    CFAIL(BLAH2HIP_ERR_INVALID, "clutter filter input of several channels: BLAH2HIP_FMT_C32 or BLAH2HIP_FMT_I8");
  if (n_surv == 0) CFAIL(BLAH2HIP_ERR_INVALID, "n_surv is 0");
  if (n_surv > BLAH2HIP_MAX_SURV) CFAIL(BLAH2HIP_ERR_INVALID, "n_surv exceeds BLAH2HIP_MAX_SURV");
  for (uint32_t k = 0; k < n_surv; k++) {
    if (!d_y[k]) CFAIL(BLAH2HIP_ERR_INVALID, ("NULL surveillance plane " + std::to_string(k)).c_str());
    if (d_y_out && !d_y_out[k]) CFAIL(BLAH2HIP_ERR_INVALID, ("NULL output plane " + std::to_string(k)).c_str());
  }
  if (n_cpi == 0 || n_cpi > h->maxBatch) CFAIL(BLAH2HIP_ERR_INVALID, "n_cpi outside [1, max_batch]");
  if (n_cpi > 1 && (cpi_stride < h->N || (d_y_out && out_stride < h->N))) CFAIL(BLAH2HIP_ERR_INVALID, "cpi_stride / out_stride < nSamples");
  CHIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  { const int rc_ = multi_alloc(h, n_surv); if (rc_) return rc_; }
  int32_t *ok = d_ok ? d_ok : h->d_okM;
  const int64_t cs = (int64_t)cpi_stride, os = (int64_t)out_stride;
  int rc = BLAH2HIP_OK;
  if (h->subCorr) { // a long filter: the per-channel path, channel by channel; nothing is shared
    if (fmt != BLAH2HIP_FMT_C32) CFAIL(BLAH2HIP_ERR_UNSUPPORTED, "a long filter (more than 4081 taps) takes fp32 planes only, not BLAH2HIP_FMT_I8");
    const size_t n = (size_t)h->nBins, rows = (n_surv + 2) & ~1u;
    for (uint32_t k = 0; k < n_surv && !rc; k++) {
      rc = long_process(h, (const cf *)d_x, (const cf *)d_y[k], n_cpi, cs, d_y_out ? (cf *)d_y_out[k] : nullptr, os, ok + (size_t)k * n_cpi, st, true);
      if (rc) break;
      // taps and correlations into the virtual-CPI layout
      CHIP(hipMemcpyAsync(h->d_wM + (size_t)k * n_cpi * n, h->d_w, (size_t)n_cpi * n * sizeof(cf), hipMemcpyDeviceToDevice, st));
      if (k == 0)
        CHIP(hipMemcpy2DAsync(h->d_rbM, rows * n * sizeof(dcx), h->d_rb, 2 * n * sizeof(dcx), n * sizeof(dcx), n_cpi, hipMemcpyDeviceToDevice, st));
      CHIP(hipMemcpy2DAsync(h->d_rbM + (1 + k) * n, rows * n * sizeof(dcx), h->d_rb + n, 2 * n * sizeof(dcx), n * sizeof(dcx), n_cpi, hipMemcpyDeviceToDevice, st));
    }
  } else {
    rc = dispatch_r3_fmt<false>(h->r3, fmt, [&](auto R3, auto in) {
      return launch_clutter_multi<decltype(R3)::value, decltype(in)>(h, d_x, d_y, n_surv, n_cpi, cs, d_y_out, os, ok, st);
    });
  }
  if (rc) return rc;
  note_last(h, ok, st, n_surv, n_cpi);
  return BLAH2HIP_OK;
}

int blah2hip_clutter_taps_dev(blah2hip_clutter_t h, const float **d_w, uint32_t *n_bins, int32_t *delay_min)
{
  if (!h) CFAIL(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (h->blk) return blah2hip_clutter_taps_dev(h->blk, d_w, n_bins, delay_min); // [n_cpi n_blocks][n_bins]
  if (d_w) *d_w = reinterpret_cast<const float *>(h->lastSurv ? h->d_wM : h->d_w);
  if (n_bins) *n_bins = (uint32_t)h->nBins;
  if (delay_min) *delay_min = h->delayMin;
  return BLAH2HIP_OK;
}

int blah2hip_clutter_process_dev(blah2hip_clutter_t h, const void *d_x, const void *d_y, uint32_t n_cpi,
                                 uint64_t cpi_stride, void *d_y_out, int32_t *d_ok, void *stream)
{
  return blah2hip_clutter_process_dev_fmt(h, BLAH2HIP_FMT_C32, d_x, d_y, n_cpi, cpi_stride, d_y_out, cpi_stride, d_ok, stream);
}

int blah2hip_clutter_process_c32(blah2hip_clutter_t h, const float *x, const float *y, uint32_t n, float *y_out, int *ok)
{
  if (!h || !x || !y || !ok) CFAIL(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (n != h->N) CFAIL(BLAH2HIP_ERR_INVALID, "n differs from the nSamples the filter was created for");
  CHIP(hipSetDevice(h->device));
  const size_t plane = (size_t)h->N;
  if (h->stageElems < 3 * plane) {
    if (h->d_stage) CHIP(hipFree(h->d_stage));
    h->d_stage = nullptr;
    CHIP(hipMalloc(&h->d_stage, 3 * plane * sizeof(cf)));
    h->stageElems = 3 * plane;
  }
  cf *dx = h->d_stage, *dy = dx + plane, *dout = dy + plane;
  CHIP(hipMemcpyAsync(dx, x, plane * sizeof(cf), hipMemcpyHostToDevice, h->stream));
  CHIP(hipMemcpyAsync(dy, y, plane * sizeof(cf), hipMemcpyHostToDevice, h->stream));
  int32_t *dok = h->blk ? h->blk->d_ok : h->d_ok;
  int rc = blah2hip_clutter_process_dev(h, dx, dy, 1, plane, dout, dok, h->stream);
  if (rc) return rc;
  std::vector<int32_t> oks(h->nBlocks, 0);
  CHIP(hipMemcpyAsync(oks.data(), dok, oks.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  CHIP(hipStreamSynchronize(h->stream));
  int32_t okv = 1; // the AND over the blocks (one flag without blocks)
  for (int32_t v : oks) okv = okv && v;
  *ok = okv;
  if (okv && y_out) CHIP(hipMemcpy(y_out, dout, plane * sizeof(cf), hipMemcpyDeviceToHost));
  return BLAH2HIP_OK;
}

int blah2hip_clutter_process_c64(blah2hip_clutter_t h, const double *x, const double *y, uint32_t n, double *y_out, int *ok)
{
  if (!h || !x || !y || !ok) CFAIL(BLAH2HIP_ERR_INVALID, "NULL argument");
  std::vector<float> fx(2 * (size_t)n), fy(2 * (size_t)n), fo(y_out ? 2 * (size_t)n : 0);
  for (size_t i = 0; i < 2 * (size_t)n; i++) { fx[i] = (float)x[i]; fy[i] = (float)y[i]; }
  int rc = blah2hip_clutter_process_c32(h, fx.data(), fy.data(), n, y_out ? fo.data() : nullptr, ok);
  if (rc) return rc;
  if (*ok && y_out)
    for (size_t i = 0; i < 2 * (size_t)n; i++) y_out[i] = (double)fo[i];
  return BLAH2HIP_OK;
}

} // extern "C"
