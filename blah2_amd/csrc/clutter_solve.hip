// The Toeplitz solve of the WienerHopf clutter filter (clutter.hip): A w = b with A[i][j] = r[i-j], WienerHopf.cpp:85-122.
// Every instantiation of a solve kernel lives in this unit -- the one-workgroup recursion (clutter_solve_kernel, its
// multi-channel and global-memory forms) and the look-ahead form on several workgroups per CPI (solve_la.hpp) -- with
// their launch paths and the two entry points that are only a solve.
// (fft_wg.hpp comes in through range_core.hpp: the filter's units keep its butterflies as single-instruction statements)
#define B2_SPLIT_BUTTERFLIES 1
#include <hip/hip_runtime.h>

#include "clutter_handle.hpp"
#include "clutter_solve_kernels.hpp"

#include <algorithm>

namespace blah2 {
namespace clutter {

namespace {

// Resident workgroups per instantiation (occupancy x CUs): what sla::choose_plan may count on for plans whose workgroups
// wait for each other.
template <int E> hipError_t solve_la_capacity_e(blah2hip_clutter_s *h, int i)
{
  int b4 = 0, b8 = 0;
  hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b4, sla::clutter_solve_la_kernel<E, 4>, 256, 0);
  if (e != hipSuccess) return e;
  e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&b8, sla::clutter_solve_la_kernel<E, 8>, 512, 0);
  if (e != hipSuccess) return e;
  h->laCap[i][0] = std::max(1, b4) * h->numCU;
  h->laCap[i][1] = std::max(1, b8) * h->numCU;
  return hipSuccess;
}
hipError_t solve_la_capacity(blah2hip_clutter_s *h)
{
  hipError_t e = solve_la_capacity_e<2>(h, 0);
  if (e == hipSuccess) e = solve_la_capacity_e<3>(h, 1);
  if (e == hipSuccess) e = solve_la_capacity_e<6>(h, 2);
  if (e == hipSuccess) e = solve_la_capacity_e<12>(h, 3);
  return e;
}
int solve_la_cap(const blah2hip_clutter_s *h, int E, int NW)
{
  const int i = E == 2 ? 0 : (E == 3 ? 1 : (E == 6 ? 2 : 3));
  return h->laCap[i][NW == 8 ? 1 : 0];
}

template <int E> void launch_solve_la(const sla::Args &a, int grid, int nw, hipStream_t st)
{
  if (nw == 4) hipLaunchKernelGGL((sla::clutter_solve_la_kernel<E, 4>), dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((sla::clutter_solve_la_kernel<E, 8>), dim3(grid), dim3(512), 0, st, a);
}

// The one-workgroup recursion's shape: one index per thread up to 1024 taps (measured: more, smaller threads win while the
// recursion is latency-bound), 2 up to 2048, 4 above; whole waves
void solve_threads(const blah2hip_clutter_s *h, int *kper, int *nt)
{
  *kper = h->solveK ? h->solveK : (h->nBins > 2048 ? 4 : (h->nBins > 1024 ? 2 : 1));
  *nt = std::min(1024, 64 * ((h->nBins + 64 * *kper - 1) / (64 * *kper)));
}

void launch_solve_stepwise(blah2hip_clutter_s *h, const SolveArgs &sa, uint32_t nCpi, hipStream_t st)
{
  if (h->d_solveWs) { // the long filters: the recursion on vectors in global memory
    hipLaunchKernelGGL(clutter_solve_big_kernel, dim3(nCpi), dim3(1024), 0, st, sa, h->d_solveWs);
    return;
  }
  const size_t sl = ((size_t)2 * (h->nBins + 1)) * sizeof(dcx) + 2 * sizeof(SolveScal);
  int kper, nt;
  solve_threads(h, &kper, &nt);
  if (kper == 1) hipLaunchKernelGGL(clutter_solve_kernel<1>, dim3(nCpi), dim3(nt), sl, st, sa);
  else if (kper == 2) hipLaunchKernelGGL(clutter_solve_kernel<2>, dim3(nCpi), dim3(nt), sl, st, sa);
  else hipLaunchKernelGGL(clutter_solve_kernel<4>, dim3(nCpi), dim3(nt), sl, st, sa);
}

template <int KI, int NS> int launch_solve_multi_ns(const SolveMultiArgs &ma, int nt, size_t ldsVec, hipStream_t st)
{
  const size_t sl = ldsVec + 2 * sizeof(SolveScalM<NS>);
  CHIP(blah2hip_ensure_lds_((const void *)clutter_solve_multi_kernel<KI, NS>, 160 * 1024 - 2048));
  hipLaunchKernelGGL((clutter_solve_multi_kernel<KI, NS>), dim3(ma.nCpi, (ma.nSurv + NS - 1) / NS), dim3(nt), sl, st, ma);
  return BLAH2HIP_OK;
}

} // namespace

// Mailboxes of the look-ahead Toeplitz solve (solve_la.hpp): sized for the largest launch each plan can be chosen for
// (create, and again when BLAH2HIP_CLUTTER_OPT_SOLVE_E changes).  Zeroed once: tags are launch epochs >= 1.
int solve_la_alloc(blah2hip_clutter_s *h)
{
  // the mailbox layout depends on the slice width only; the largest batch a width can be chosen for is the handle's
  int64_t need = 0;
  for (int E : sla::kE) {
    if (h->solveE && E != h->solveE) continue;
    const sla::Plan p4 = sla::make_plan(h->nBins, E, 4), p8 = sla::make_plan(h->nBins, E, 8);
    int64_t batch = h->maxBatch;
    if (!h->solveE && E != 12 && !(h->blockChild && p8.G == 1)) batch = std::min<int64_t>(batch, 8 * (h->numCU / (8 * std::min(p4.G, p8.G))));
    need = std::max(need, p4.stride * batch);
  }
  if (need > h->mailWords) {
    if (h->d_mail) CHIP(hipFree(h->d_mail));
    h->d_mail = nullptr; h->mailWords = 0;
    CHIP(hipMalloc(&h->d_mail, (size_t)need * sizeof(sla::u64)));
    CHIP(hipMemset(h->d_mail, 0, (size_t)need * sizeof(sla::u64)));
    h->mailWords = need;
  }
  if (!h->d_epoch) {
    CHIP(hipMalloc(&h->d_epoch, 4 * sizeof(uint32_t)));
    CHIP(hipMemset(h->d_epoch, 0, 4 * sizeof(uint32_t)));
  }
  if (!h->laCap[0][0]) CHIP(solve_la_capacity(h));
  return BLAH2HIP_OK;
}

void launch_solve_epoch(uint32_t *epoch, hipStream_t st)
{
  hipLaunchKernelGGL(solve_epoch_kernel, dim3(1), dim3(1), 0, st, epoch);
}

// The Toeplitz solve of nCpi systems whose r, b sit in sa.rb (the epoch of the look-ahead form's mailboxes has been
// bumped by the launch in front: clutter_reduce_kernel, or solve_epoch_kernel)
int launch_solve(blah2hip_clutter_s *h, const SolveArgs &sa, uint32_t nCpi, hipStream_t st)
{
  int32_t *ok = sa.ok;
  CHIP(blah2hip_ensure_lds_((const void *)clutter_solve_kernel<1>, 160 * 1024 - 2048));
  CHIP(blah2hip_ensure_lds_((const void *)clutter_solve_kernel<2>, 160 * 1024 - 2048));
  CHIP(blah2hip_ensure_lds_((const void *)clutter_solve_kernel<4>, 160 * 1024 - 2048));
  CHIP(h->timer.tic(BLAH2HIP_CK_SOLVE, st));
  if (h->solveForm != BLAH2HIP_CLUTTER_SOLVE_STEPWISE && h->d_mail) {
    // blocks of 32 orders on several workgroups per CPI (solve_la.hpp): as many CUs per CPI as the launch leaves free
    sla::Plan p = sla::choose_plan(h->nBins, (int)nCpi, h->numCU, h->solveE, [h](int E, int NW) { return solve_la_cap(h, E, NW); });
    // A block child beyond one system per CU (n_cpi n_blocks small systems: 4096 at configs[1] with 16 blocks): the planner's
    // fallback is its widest slices, built for a lone CPI's "nothing to wait for".  The narrowest slices that still make ONE
    // workgroup per system wait for nothing either, and ran the 1024 ... 4096 systems of 410 taps 2.8 x faster (measured,
    // DESIGN.md section 7 item 13).  Handles without blocks keep the planner's choice: their taps' bits are a contract.
    if (h->blockChild && !h->solveE && p.E == 12 && (int64_t)((nCpi + 7) / 8 * 8) > h->numCU)
      for (int E : sla::kE) {
        const sla::Plan q = sla::make_plan(h->nBins, E, 8);
        if (q.G == 1) { p = q; break; }
      }
    sla::Args la;
    la.rb = sa.rb; la.w = sa.w; la.ok = ok; la.mail = h->d_mail; la.epoch = h->d_epoch; la.fault = h->d_epoch + 1;
    la.spinLimit = h->spinLimit ? h->spinLimit : sla::SPIN_LIMIT;
    la.n = h->nBins; la.NB = p.NB; la.nbulk = p.nbulk; la.G = p.G; la.nCpi = (int)nCpi; la.mailStride = p.stride;
    la.offHalo = p.offHalo; la.offFeed = p.offFeed; la.offHaloFlag = p.offHaloFlag; la.offFeedFlag = p.offFeedFlag;
    la.offStatus = p.offStatus;
    if (p.stride * (int64_t)nCpi > h->mailWords) CFAIL(BLAH2HIP_ERR_INVALID, "internal: solve mailbox too small for this launch");
    const int grid = ((int)nCpi + 7) / 8 * 8 * p.G;
    switch (p.E) {
    case 2: launch_solve_la<2>(la, grid, p.NW, st); break;
    case 3: launch_solve_la<3>(la, grid, p.NW, st); break;
    case 6: launch_solve_la<6>(la, grid, p.NW, st); break;
    default: launch_solve_la<12>(la, grid, p.NW, st); break;
    }
    h->lastForm = BLAH2HIP_CLUTTER_SOLVE_LOOKAHEAD; h->lastE = p.E; h->lastG = p.G;
    CHIP(hipGetLastError());
    // ... and behind it the one-workgroup kernel, gated per CPI on the fault word of this launch: workgroups that a busy
    // chip (another handle's kernels, a chip-filling launch on a second stream) dispatched so late that a bounded wait ran
    // out leave their CPI to it.  No CPI faulted: every workgroup reads one word and leaves (2 us for the launch).
    SolveArgs ga = sa;
    ga.gate = h->d_mail + p.offStatus + 1; ga.gateStride = p.stride; ga.retries = h->d_epoch + 2; ga.epoch = h->d_epoch;
    launch_solve_stepwise(h, ga, nCpi, st);
  } else {
    launch_solve_stepwise(h, sa, nCpi, st);
    h->lastForm = BLAH2HIP_CLUTTER_SOLVE_STEPWISE; h->lastE = 0; h->lastG = 1;
  }
  CHIP(hipGetLastError());
  CHIP(h->timer.toc(BLAH2HIP_CK_SOLVE, st));
  return BLAH2HIP_OK;
}

// the smallest tile that holds the channels, up to the register budget of KI indices per thread
int launch_solve_multi(blah2hip_clutter_s *h, const SolveMultiArgs &ma, hipStream_t st)
{
  const size_t ldsVec = ((size_t)2 * (h->nBins + 1)) * sizeof(dcx);
  int kper, nt;
  solve_threads(h, &kper, &nt);
  const int K = ma.nSurv;
  if (K == 1) {
    if (kper == 1) return launch_solve_multi_ns<1, 1>(ma, nt, ldsVec, st);
    if (kper == 2) return launch_solve_multi_ns<2, 1>(ma, nt, ldsVec, st);
    return launch_solve_multi_ns<4, 1>(ma, nt, ldsVec, st);
  }
  if (kper == 4) return launch_solve_multi_ns<4, 2>(ma, nt, ldsVec, st);
  if (kper == 2) return K <= 2 ? launch_solve_multi_ns<2, 2>(ma, nt, ldsVec, st) : launch_solve_multi_ns<2, 4>(ma, nt, ldsVec, st);
  if (K <= 2) return launch_solve_multi_ns<1, 2>(ma, nt, ldsVec, st);
  if (K <= 4) return launch_solve_multi_ns<1, 4>(ma, nt, ldsVec, st);
  return launch_solve_multi_ns<1, 8>(ma, nt, ldsVec, st);
}

} // namespace clutter
} // namespace blah2

using namespace blah2::clutter;

extern "C" {

int blah2hip_clutter_solve(blah2hip_clutter_t h, const double *rb, uint32_t n_cpi, float *w, int32_t *ok)
{
  if (!h || !rb || !w || !ok) CFAIL(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (h->blk) return blah2hip_clutter_solve(h->blk, rb, n_cpi, w, ok); // n_cpi counts virtual CPIs
  if (n_cpi == 0 || n_cpi > h->maxBatch) CFAIL(BLAH2HIP_ERR_INVALID, "n_cpi outside [1, max_batch]");
  CHIP(hipSetDevice(h->device));
  const size_t n = (size_t)h->nBins;
  CHIP(hipMemcpyAsync(h->d_rb, rb, (size_t)n_cpi * 2 * n * sizeof(dcx), hipMemcpyHostToDevice, h->stream));
  launch_solve_epoch(h->d_epoch, h->stream);
  { const int rc_ = launch_solve(h, solve_args(h, h->d_rb, h->d_w, h->d_ok), n_cpi, h->stream); if (rc_) return rc_; }
  note_last(h, h->d_ok, h->stream);
  CHIP(hipMemcpyAsync(w, h->d_w, (size_t)n_cpi * n * sizeof(blah2::cf), hipMemcpyDeviceToHost, h->stream));
  CHIP(hipMemcpyAsync(ok, h->d_ok, (size_t)n_cpi * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  CHIP(hipStreamSynchronize(h->stream));
  return BLAH2HIP_OK;
}

int blah2hip_clutter_solve_dev(blah2hip_clutter_t h, const double *d_rb, uint32_t n_cpi, float *d_w, int32_t *d_ok, void *stream)
{
  if (!h || !d_rb || !d_w || !d_ok) CFAIL(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (h->blk) return blah2hip_clutter_solve_dev(h->blk, d_rb, n_cpi, d_w, d_ok, stream);
  if (n_cpi == 0 || n_cpi > h->maxBatch) CFAIL(BLAH2HIP_ERR_INVALID, "n_cpi outside [1, max_batch]");
  CHIP(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  launch_solve_epoch(h->d_epoch, st);
  note_last(h, d_ok, st);
  return launch_solve(h, solve_args(h, (dcx *)d_rb, (blah2::cf *)d_w, d_ok), n_cpi, st);
}

} // extern "C"
