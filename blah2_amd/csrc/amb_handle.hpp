// Internal to the library: what the units behind include/blah2hip.h share.  The ambiguity handle, whose fields every
// unit reads directly (no accessors), the error and launch-check helpers, and the few engine functions (capi.hip)
// that another unit calls.  Host code only: capi.hip, array.hip, detect.hip, integrate.hip, taper.hip, walk.hip,
// carriers.hip and context.hip all include it.
#pragma once

#include <hip/hip_runtime.h>

#include "blah2hip.h"
#include "range_core.hpp"
#include "table_cache.hpp"
#include "timing.hpp"

#include <algorithm>
#include <map>
#include <string>
#include <vector>

// context.hip: the thread's error string (blah2hip_last_error) and the once-per-(device, kernel) LDS attribute
extern "C" void blah2hip_set_error_(const char *msg);
extern "C" hipError_t blah2hip_ensure_lds_(const void *kern, int bytes);

struct blah2hip_amb_s {
  typedef blah2::cf cf;
  // ---- geometry and plan: written by create and blah2hip_amb_set_option (capi.hip), read by every unit
  int device = 0;
  blah2hip_amb_dims_t dims{};
  int32_t delayMin = 0, delayMax = 0, dopplerMin = 0, dopplerMax = 0;
  uint32_t fs = 0;
  int r3 = 8;
  blah2::RangePlan plan{};          // segmentation (of the longest chunk) + the first chunk's lag window
  struct LagChunk { int32_t lag0, count, col0; }; // linear lags lag0 .. lag0 + count - 1 -> map columns col0 ..
  std::vector<LagChunk> chunks;     // the delay axis as runs of consecutive LINEAR lags (one chunk in the usual case)
  int32_t maxChunk = 0;
  std::vector<int32_t> delayAxis;
  std::vector<double> dopplerAxis;
  hipStream_t stream = nullptr;
  int numCU = 256;
  int dopTilesX = 0, dopTilesY = 0; // direct-DFT fallback grid
  int dopR3 = 0;                    // 0 = direct fallback, else Bluestein on WgFft<dopR3>
  int dopGridX = 0;
  int nParts = 0;                   // metrics partials per CPI
  int nTiles = 0;                   // 16-column tiles of the range map

  // ---- execution plan: per handle, fixed at create or through blah2hip_amb_set_option (capi.hip); detect.hip reads cfar2d*
  int rangeGridForce = 0;           // BLAH2HIP_OPT_RANGE_GRID (0 = the launched kernel's residency)
  int rangeWalk = 0;                // BLAH2HIP_OPT_RANGE_WALK (0 = the engine's choice)
  int dopForce = BLAH2HIP_DOP_AUTO; // BLAH2HIP_OPT_DOPPLER_KERNEL
  int rangeKernel = 0;              // BLAH2HIP_OPT_RANGE_KERNEL (0 = by transform length)
  int fftLenForce = 0;              // BLAH2HIP_OPT_FFT_LEN (0 = planner)
  int multiMode = BLAH2HIP_MULTI_AUTO; // BLAH2HIP_OPT_MULTI_SURV_RANGE
  int cfar2dForce = 0;              // BLAH2HIP_OPT_CFAR2D_KERNEL
  int dopGridForce = 0;             // BLAH2HIP_OPT_DOPPLER_GRID (0 = residency of the persistent kernel)
  int cfar2dSegRows = 0;            // BLAH2HIP_OPT_CFAR2D_SEG_ROWS (0 = cost model of cfar2d_stream_launch)
  int cfar2dGridForce = 0;          // BLAH2HIP_OPT_CFAR2D_GRID (0 = one workgroup per CU)
  int leakMode = 1;                 // BLAH2HIP_OPT_LEAK_COMPENSATION: 0 off, 1 auto (applied where it can reach 3e-5 of the mean level), 2 always
  int hotMode = 1;                  // BLAH2HIP_OPT_HOT_COLUMNS: 0 off, 1 auto (CPIs long enough for a peak HOT_RATIO above the mean level), 2 always
  uint32_t cfarLooks = 1;           // BLAH2HIP_OPT_CFAR_LOOKS: looks per cell the detectors' threshold factors are made for (detect.hip)
  int taperSegRows = 0;             // BLAH2HIP_OPT_TAPER_SEG_ROWS (0 = the launch's own choice, taper.hip)

  // ---- device buffers allocated by create (capi.hip) and freed by destroy, which frees every buffer of the handle
  cf *d_tw = nullptr;
  cf *d_dopW = nullptr;
  double2 *d_dopW64 = nullptr;   // hot_columns_kernel: exp(-2 pi i k / nD) in fp64
  uint32_t *d_hotCount = nullptr; // [2][max_batch]: columns the last call's hot_columns_kernel rewrote, columns it left out
  cf *d_R = nullptr;
  cf *d_map = nullptr;
  double *d_partSum = nullptr;   // (array.hip's kernels leave their per-workgroup partials here too)
  float *d_partMax = nullptr;
  uint32_t *d_tickets = nullptr; // arrival counters of the fused Map::set_metrics finish (doppler_sub1k_kernel), zero between launches
  uint32_t *d_rangeWalk = nullptr;  // rangew1k_kernel's ticket heads and exit counter (range_walk.hpp), zero between launches
  double *d_metrics = nullptr;
  double *d_doppler = nullptr;
  uint32_t *d_count = nullptr;
  uint32_t *d_detWords = nullptr;   // detect_finish_kernel, tiled form: [2][max_batch] records appended, tickets taken; zero between launches
  cf *d_dtw = nullptr;              // exp(-2 pi i k/M)
  cf *d_chirp = nullptr;            // exp(-i pi n^2/nD)
  cf *d_bf = nullptr;               // chirp-kernel spectrum / M in register layout
  cf *d_bfn = nullptr;              // the same in natural order (M = 2048 only: doppler_tilew_kernel)

  // ---- written by capi.hip while it runs: lazily allocated staging, what the last launch ran, FIR, leak, hot columns
  void *h_pin = nullptr;            // pinned host staging of the c64 entry point
  size_t h_pin_bytes = 0;
  void *d_in = nullptr; // staging for the host entry points
  size_t d_in_bytes = 0;
  cf *d_rot = nullptr; // rotated reference / converted planes for asymmetric Doppler limits
  int rangeGridLast = 0;            // BLAH2HIP_INFO_RANGE_GRID: workgroup cap of the last launch
  int lastDoppler = 0;              // BLAH2HIP_INFO_LAST_DOPPLER_KERNEL
  int lastRange = 0;                // BLAH2HIP_INFO_LAST_RANGE_KERNEL
  int dopGridLast = 0, dopTilesLast = 0; // BLAH2HIP_INFO_DOPPLER_GRID / _TILES

  // the clutter filter's FIR fused into the range correlation (blah2hip_amb_set_fir): the filter handle's taps
  const cf *firW = nullptr; // [max_batch][firBins]; nullptr: the plain range kernels
  int firBins = 0, firDmin = 0;
  cf *d_H = nullptr;        // [max_batch][16][256]: the taps' spectrum in the transform's register layout (taps_spectrum_kernel)
  int32_t *d_firK0 = nullptr; // [max_batch]: the largest tap's index (left out of d_H, applied in the time domain)

  // Fixed-pattern leak compensation (see leak_calibrate): per (range kernel, Doppler kernel) the lags of the zero-Doppler row
  // into which the fp32 transform chain leaks a fixed fraction g of the lag-0 cell, measured once on a synthetic CPI
  struct LeakCal { int nLags = 0; double maxAbs = 0.0; bool active = false; int32_t *d_lag = nullptr; cf *d_g = nullptr; };
  std::map<int, LeakCal> leak;      // key = range kernel id * 64 + Doppler kernel id
  bool inLeakCal = false;
  bool lastHot = false;             // the last process call launched hot_columns_kernel
  hipStream_t lastHotStream = nullptr; // ... on this stream (BLAH2HIP_INFO_HOT_COLUMNS waits for that one only)
  uint32_t lastHotCpis = 0;         // ... over this many CPIs
  uint32_t lastMaps = 0;            // maps (virtual CPIs) of the last process call: what d_R holds (0 = no call yet; walk.hip)
  int lastLeakLags = 0;             // BLAH2HIP_INFO_LEAK_LAGS: lags corrected by the last process call (0 = not applied)
  double lastLeakMax = 0.0;         // BLAH2HIP_INFO_LEAK_MAX_E12: the largest |g| of the calibration the last call ran under

  // ---- written by detect.hip; bearingGridLast by array.hip, taperGridLast by taper.hip, the migration and rate fields by walk.hip,
  // the carrier fields by carriers.hip
  // The detectors' threshold tables on the device: three lists under the one policy of table_cache.hpp (eight unpinned
  // tables each, what *_prepare handed out is pinned and never evicted), filled by detect.hip, freed by destroy (capi.hip).
  // An averaging or ordered-statistic table is alpha[n + 1], then with a rank (permille) rank[n + 1] words; a greatest-of /
  // smallest-of table is (2 hR + 1)(nT + 1)^2 factors for this handle's maps.
  struct CfarKey { double pfa; uint32_t looks, rank; size_t n; };
  struct GoKey { double pfa; uint32_t kind; int32_t nG, nT, hR; };
  blah2::TableCache<CfarKey> alphaTables; // cell averaging (rank 0): one per (pfa, looks, size) seen
  blah2::TableCache<CfarKey> osTables;    // ordered statistic: one per (pfa, looks, rank_permille, size) seen
  blah2::TableCache<GoKey> goTables;      // one per (pfa, kind, nGuard, nTrain, hR) seen
  double *d_sat = nullptr;          // 2-D CFAR summed-area table [max_batch][nD+1][nDelay+1], allocated at its first use
  blah2hip_hit_t *d_hits = nullptr; // the *_process calls' hit list, grown to the map's cell count
  uint32_t hitCap = 0;
  int cfar2dSegRowsLast = 0, cfar2dGridLast = 0; // BLAH2HIP_INFO_CFAR2D_SEG_ROWS / _GRID
  int detGridLast = 0, detTiledLast = 0; // BLAH2HIP_INFO_DETECT_GRID / _TILED
  int bearingGridLast = 0;          // BLAH2HIP_INFO_BEARING_GRID
  int taperGridLast = 0;            // BLAH2HIP_INFO_TAPER_GRID
  double *d_migrate = nullptr;      // [nD] half walks (blah2hip_amb_set_migration), allocated at its first use, freed by destroy
  bool migrateSet = false;          // ... and whether a table is set
  int migrateGridLast = 0;          // BLAH2HIP_INFO_MIGRATE_GRID
  cf *d_rates = nullptr;            // [BLAH2HIP_MAX_RATES][nD] chirps c_k[i] (blah2hip_amb_set_rates, walk.hip), allocated at its first use, freed by destroy
  uint32_t nRates = 0, zeroRates = 0; // ... hypotheses of the bank that is set (0 = none), and bit k: q[k] == 0
  int rateGridLast = 0;             // BLAH2HIP_INFO_RATE_GRID
  void *d_carriers = nullptr;       // [BLAH2HIP_MAX_CARRIERS][nD] CarrierEntry (blah2hip_amb_set_carriers, carriers.hip), allocated at its first use, freed by destroy
  uint32_t nCarriers = 0;           // ... carriers of the table that is set (0 = none)
  int carrierGridLast = 0;          // BLAH2HIP_INFO_CARRIER_GRID
  int trackGridLast = 0, trackShiftLast = 0; // BLAH2HIP_INFO_TRACK_GRID / _TRACK_MAX_SHIFT (integrate.hip)

  // ---- every unit brackets its launches (tic / toc below)
  blah2::KernelTimer<BLAH2HIP_K_COUNT> timer;

};

namespace blah2 {

static inline int fail(int code, const std::string &msg)
{
  blah2hip_set_error_(msg.c_str());
  return code;
}

#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return fail(BLAH2HIP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));      \
  } while (0)

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (device, kernel): the
// attribute belongs to the function object of the CURRENT device, and a process
// may hold handles on several devices.
#define LDSCFG(kern, bytes)                                                                   \
  do {                                                                                       \
    hipError_t e_ = blah2hip_ensure_lds_((const void *)(kern), (int)(bytes));                 \
    if (e_ != hipSuccess)                                                                    \
      return fail(BLAH2HIP_ERR_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e_)); \
  } while (0)

static inline int tic(blah2hip_amb_s *h, int k, hipStream_t st)
{
  HIPCHK(h->timer.tic(k, st));
  return BLAH2HIP_OK;
}

static inline int toc(blah2hip_amb_s *h, int k, hipStream_t st)
{
  HIPCHK(h->timer.toc(k, st));
  return BLAH2HIP_OK;
}

// table_cache.hpp's device: HIP on the current device
struct HipTableDevice {
  static const char *text(hipError_t e) { return e == hipSuccess ? nullptr : hipGetErrorString(e); }
  const char *alloc(size_t bytes, double **d) { return text(hipMalloc(d, bytes)); }
  const char *upload(double *d, const double *host, size_t bytes) { return text(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice)); }
  bool free(double *d) { return hipFree(d) == hipSuccess; }
  const char *synchronize() { return text(hipDeviceSynchronize()); }
  bool capturing(void *stream)
  {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing((hipStream_t)stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
  }
};

// whether the byte ranges [a, a + na) and [b, b + nb) share a byte: what the calls with caller-owned outputs refuse
static inline bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb)
{
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

// Workgroups per CPI of a launch that strides over `units` accesses a CPI: eight a CU over the launch of n_cpi CPIs, each
// with at least one pass of 256 units, and no more than `cap` (what the handle has partials for, where the kernel
// leaves one per workgroup)
static inline uint32_t groups_per_cpi(const blah2hip_amb_s *h, size_t units, uint32_t n_cpi, size_t cap = SIZE_MAX)
{
  const size_t passes = (units + 255) / 256, spread = (8 * (size_t)h->numCU + n_cpi - 1) / n_cpi;
  return (uint32_t)std::max<size_t>(1, std::min({cap, passes, spread}));
}

// capi.hip: Map::set_metrics of n_maps maps of `cells` cells from the n_parts partials a map in h->d_partSum / d_partMax
// (metrics_kernel, inside its BLAH2HIP_K_METRICS bracket).  Not exported from the library.
__attribute__((visibility("hidden"))) int amb_metrics_enqueue(blah2hip_amb_s *h, uint32_t n_maps, int n_parts, double cells, double *d_metrics, hipStream_t st);

} // namespace blah2
