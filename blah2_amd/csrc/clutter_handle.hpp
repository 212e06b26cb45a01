// Internal to the library: what the two units of the clutter filter share.  clutter.hip holds the planner, the
// correlation and FIR launches and most of the C API; clutter_solve.hip holds every Toeplitz-solve kernel, their launch
// paths and the two entry points that are only a solve.  Here: the handle, whose fields both units read directly, the
// error helpers, the argument structs that cross the unit boundary and the few functions one unit calls in the other.
// Host code only.  A unit defines B2_SPLIT_BUTTERFLIES ahead of this header (range_core.hpp brings fft_wg.hpp in).
#pragma once

#include <hip/hip_runtime.h>

#include "blah2hip.h"
#include "range_core.hpp"
#include "timing.hpp"

#include <stdint.h>

#include <string>

// context.hip: the thread's error string (blah2hip_last_error) and the once-per-(device, kernel) LDS attribute
extern "C" void blah2hip_set_error_(const char *msg);
extern "C" hipError_t blah2hip_ensure_lds_(const void *kern, int bytes);

#define CHIP(expr)                                                                        \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) {                                                               \
      blah2hip_set_error_((std::string(#expr) + ": " + hipGetErrorString(e_)).c_str());   \
      return BLAH2HIP_ERR_HIP;                                                            \
    }                                                                                     \
  } while (0)
#define CFAIL(code, msg)            \
  do {                              \
    blah2hip_set_error_(msg);       \
    return code;                    \
  } while (0)

namespace blah2 {
namespace clutter {

struct dcx {
  double x, y;
};

// ---- reduction of the partials (fp64), then the Toeplitz solve -----------------
struct SolveArgs {
  const cf *partial; // [nCpi][2][nJobs][nBins]
  dcx *rb;           // [nCpi][2][nBins]: r then b, fp64
  cf *w;             // [nCpi][nBins]
  int32_t *ok;       // [nCpi]
  int32_t nBins, nJobs;
  uint32_t *epoch;   // launch epoch of the look-ahead solve's mailboxes (solve_la.hpp), bumped here
  // clutter_solve_kernel as the launch BEHIND the look-ahead solve: a workgroup runs only if its CPI's fault word carries
  // this launch's epoch (a bounded wait of the look-ahead form ran out), and counts itself in *retries
  const unsigned long long *gate = nullptr; // the CPI's fault word: gate[cpi * gateStride]
  int64_t gateStride = 0;
  uint32_t *retries = nullptr;
};

struct SolveMultiArgs {
  const dcx *rb; // [nCpi][rows][nBins]: r, then b_0 .. b_{nSurv-1}
  cf *w;         // [nSurv][nCpi][nBins]
  int32_t *ok;   // [nSurv][nCpi]
  int32_t nBins, rows, nSurv, nCpi;
};

} // namespace clutter
} // namespace blah2

struct blah2hip_clutter_s {
  typedef blah2::cf cf;
  typedef blah2::clutter::dcx dcx;
  int device = 0;
  int32_t delayMin = 0, delayMax = 0;
  uint32_t N = 0, maxBatch = 1;
  int32_t nBins = 0;
  int r3 = 8;
  int F = 2048, segLen = 0, nSeg = 0, nJobs = 0, firGrid = 0, numCU = 256;
  bool firCarry = false;     // blocks of F/2 samples, the window overlap carried in registers (plan)
  bool firNoCarry = false;   // BLAH2HIP_CLUTTER_OPT_FIR_CARRY = 0
  hipStream_t stream = nullptr;
  cf *d_tw = nullptr;
  cf *d_partial = nullptr;
  dcx *d_rb = nullptr;
  cf *d_w = nullptr;
  int32_t *d_ok = nullptr;
  cf *d_stage = nullptr; // host entry points: x, y, y_out planes
  size_t stageElems = 0;
  int solveK = 0;            // indices per thread of the one-workgroup Toeplitz solve (0 = by size)
  int solveForm = 0;         // BLAH2HIP_CLUTTER_OPT_SOLVE_FORM
  int solveE = 0;            // BLAH2HIP_CLUTTER_OPT_SOLVE_E (0 = by launch size)
  unsigned long long *d_mail = nullptr; // mailboxes of the look-ahead solve (solve_la.hpp), sized for max_batch
  int64_t mailWords = 0;
  uint32_t *d_epoch = nullptr; // [0] launch epoch, [1] sticky fault word (a bounded spin ran out), [2] CPIs solved again by the gated launch
  uint32_t spinLimit = 0;      // BLAH2HIP_CLUTTER_OPT_SOLVE_SPIN_LIMIT (0 = sla::SPIN_LIMIT)
  int laCap[4][2] = {};        // workgroups of clutter_solve_la_kernel<kE[i], 4 | 8> the chip holds at once
  int lastForm = 0, lastE = 0, lastG = 0; // what the last launch ran
  bool corrHalf = false;     // half-window correlation (2 transforms per F/2 samples) instead of the windowed one
  int fftLenForce = 0;       // BLAH2HIP_CLUTTER_OPT_FFT_LEN (0 = planner)
  int corrForce = 0;         // BLAH2HIP_CLUTTER_OPT_CORR
  int corrGrid = 0;          // BLAH2HIP_CLUTTER_OPT_CORR_GRID (0 = clutter_grids' own; a re-plan returns to 0)
  int lastCorrGrid = 0;      // BLAH2HIP_CLUTTER_INFO_CORR_GRID
  // the last call, as note_last() recorded it
  int32_t *lastOk = nullptr; // where it wrote its flags
  hipStream_t lastStream = nullptr; // ... and the stream it was enqueued on (blah2hip_clutter_get_info waits for that one only)
  uint32_t lastSurv = 0, lastNCpi = 0; // a multi call: its channels and CPIs per channel (0: a single call)
  blah2::KernelTimer<BLAH2HIP_CK_COUNT> timer;
  // LONG filters (more than F - 15 = 4081 taps; see long_process): two children of LONG_C taps run the
  // correlations (first lag = this filter's) and the FIR (first lag 0, on pre-shifted planes) chunk by chunk
  blah2hip_clutter_s *subCorr = nullptr, *subFir = nullptr;
  int nChunks = 0;
  cf *d_long = nullptr;      // [3][maxBatch][N]: private copies of x and y (the output is built in the y copy) + one work plane
  dcx *d_solveWs = nullptr;  // [maxBatch][4 nBins + 2]: clutter_solve_big_kernel's vectors
  // several surveillance channels on one reference (blah2hip_clutter_process_multi_dev_fmt): built by the first such call
  // for the channels it asks for, kept apart from d_w / d_rb (an ambiguity handle may hold d_w, blah2hip_amb_set_fir)
  uint32_t multiK = 0;         // channels the buffers below hold
  size_t multiJobs = 0;        // n_cpi x (workgroups per CPI) that d_partialM holds
  cf *d_partialM = nullptr;    // [n_cpi][rows][nJobs][nBins], rows = 1 + K rounded up to even: r, b_0 .. b_{K-1}
  dcx *d_rbM = nullptr;        // [n_cpi][rows][nBins]
  cf *d_wM = nullptr;          // [K][n_cpi][nBins]: virtual CPI k n_cpi + c
  int32_t *d_okM = nullptr;    // [K][n_cpi]
  // taps per BLOCK of the CPI (blah2hip_clutter_create_ex with n_blocks > 1, see launch_clutter_blocks): this handle keeps the
  // CPI's geometry (N, delayMin: the FIR's XsMap) and the FIR's timer; `blk` is a handle for CPIs of N / nBlocks samples and a
  // batch of maxBatch nBlocks -- the plan, the estimation kernels' buffers, taps, flags and solve state of the virtual CPIs
  uint32_t nBlocks = 1;
  blah2hip_clutter_s *blk = nullptr;
  bool blockChild = false; // this handle IS such a child: its launches have n_cpi n_blocks systems (launch_solve)
};

namespace blah2 {
namespace clutter {

// What blah2hip_clutter_read_last, _taps_dev and _get_info go by: every entry point ends with one of these.  surv > 0: a
// multi call of surv channels and nCpi CPIs per channel (the taps and flags are the multi buffers', virtual CPI k nCpi + c).
inline void note_last(blah2hip_clutter_s *h, int32_t *ok, hipStream_t st, uint32_t surv = 0, uint32_t nCpi = 0)
{
  h->lastSurv = surv; h->lastNCpi = nCpi; // (lastNCpi is read behind a multi call only)
  h->lastOk = ok;
  h->lastStream = st;
}

// a solve alone, of systems that sit in `rb` already: no partials, nothing to reduce
inline SolveArgs solve_args(const blah2hip_clutter_s *h, dcx *rb, cf *w, int32_t *ok)
{
  SolveArgs sa;
  sa.partial = nullptr; sa.rb = rb; sa.w = w; sa.ok = ok; sa.nBins = h->nBins; sa.nJobs = 0; sa.epoch = h->d_epoch;
  return sa;
}

// clutter_solve.hip, called from clutter.hip.  Not exported from the library.
#define B2_CLUTTER_LOCAL __attribute__((visibility("hidden")))
// mailboxes of the look-ahead solve for the handle's plans (create, and again when BLAH2HIP_CLUTTER_OPT_SOLVE_E changes)
B2_CLUTTER_LOCAL int solve_la_alloc(blah2hip_clutter_s *h);
// the launch that bumps the look-ahead solve's epoch where no reduction runs in front of the solve
B2_CLUTTER_LOCAL void launch_solve_epoch(uint32_t *epoch, hipStream_t st);
// nCpi systems (r, b in sa.rb) inside the handle's BLAH2HIP_CK_SOLVE bracket; records the form that ran
B2_CLUTTER_LOCAL int launch_solve(blah2hip_clutter_s *h, const SolveArgs &sa, uint32_t nCpi, hipStream_t st);
// one recursion per CPI with ma.nSurv right-hand sides; the caller brackets it
B2_CLUTTER_LOCAL int launch_solve_multi(blah2hip_clutter_s *h, const SolveMultiArgs &ma, hipStream_t st);

} // namespace clutter
} // namespace blah2
