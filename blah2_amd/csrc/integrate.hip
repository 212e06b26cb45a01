// Non-coherent integration behind include/blah2hip.h: the sum of |M|^2 over the surveillance channels and over a sliding
// window of consecutive CPIs.  Host code of the blah2hip_nci_* entry points; the kernel is integrate_kernels.hpp's.  With
// tracks set (blah2hip_nci_set_tracks) the window sums follow an echo's walk in delay and Doppler: track_kernels.hpp's kernels.
#include "amb_handle.hpp"
#include "integrate_kernels.hpp"
#include "track_kernels.hpp"

#include <cmath>

using namespace blah2;

// The integrator: a window over the maps of ONE ambiguity handle (its geometry, partials, timer), the CPI counter and
// the history planes
struct blah2hip_nci_s {
  blah2hip_amb_s *amb = nullptr;
  uint32_t nSurv = 0, window = 0, hop = 0;
  uint64_t g = 0;          // CPIs since the creation or the last reset
  float *d_hist = nullptr; // [window - 1][cells]: p of the last window - 1 CPIs
  // tracks (blah2hip_nci_set_tracks): the ring takes the history's place
  bool tracks = false;
  uint32_t nRates = 0, maxCpi = 0, ringLen = 0;
  float *d_ring = nullptr; // [ringLen][cells]: p of CPI g in plane g mod ringLen
  int2 *d_tab = nullptr;   // [nRates][window][n_doppler]: (jr, s)
  KernelTimer<BLAH2HIP_NK_COUNT> timer; // the kernel's launches are bracketed here, not in the ambiguity handle's slots
};

namespace {

// The windows that end inside the next n_cpi CPIs: a window ends at every g >= W - 1 with (g - (W - 1)) % H == 0.
// first: the g of the first of them at or behind the counter, whether it lies inside the n_cpi CPIs or not.
void windows_in(const blah2hip_nci_s *n, uint32_t n_cpi, uint32_t *n_out, uint64_t *first)
{
  const uint64_t w1 = n->window - 1, H = n->hop;
  const uint64_t f = n->g <= w1 ? w1 : w1 + (n->g - w1 + H - 1) / H * H;
  const uint64_t end = n->g + n_cpi; // one past the last CPI
  *first = f;
  *n_out = f < end ? (uint32_t)((end - 1 - f) / H + 1) : 0;
}

} // namespace

extern "C" {

int blah2hip_nci_create(blah2hip_amb_t amb, uint32_t n_surv, uint32_t window, uint32_t hop, blah2hip_nci_t *out)
{
  if (!amb || !out) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (n_surv == 0 || n_surv > BLAH2HIP_MAX_SURV) return fail(BLAH2HIP_ERR_INVALID, "n_surv outside [1, BLAH2HIP_MAX_SURV]");
  if (window == 0 || window > BLAH2HIP_MAX_NCI_WINDOW) return fail(BLAH2HIP_ERR_INVALID, "window outside [1, BLAH2HIP_MAX_NCI_WINDOW]");
  if (hop == 0) return fail(BLAH2HIP_ERR_INVALID, "hop is 0");
  static_assert(BLAH2HIP_MAX_NCI_WINDOW == NCI_MAX_WINDOW, "launch_nci covers the header's windows");
  const size_t cells = (size_t)amb->dims.n_doppler_bins * amb->dims.n_delay_bins;
  // one workgroup per 256 units of two cells, each with a metrics partial per output map in the handle's buffers (nParts
  // a map: the Doppler kernels' largest grid, which is a workgroup per 8 x 64 cells at the least -- so this holds)
  if (((cells + 1) / 2 + 255) / 256 > (size_t)amb->nParts)
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "integrate: the handle holds fewer metrics partials per map than the kernel has workgroups");
  HIPCHK(hipSetDevice(amb->device));
  blah2hip_nci_s *n = new blah2hip_nci_s;
  n->amb = amb;
  n->nSurv = n_surv; n->window = window; n->hop = hop;
  if (window > 1) {
    hipError_t e = hipMalloc(&n->d_hist, (size_t)(window - 1) * cells * sizeof(float));
    if (e != hipSuccess) { delete n; return fail(BLAH2HIP_ERR_HIP, std::string("hipMalloc(history): ") + hipGetErrorString(e)); }
  }
  *out = n;
  return BLAH2HIP_OK;
}

int blah2hip_nci_destroy(blah2hip_nci_t n)
{
  if (!n) return BLAH2HIP_OK;
  int rc = BLAH2HIP_OK;
  (void)hipSetDevice(n->amb->device);
  (void)hipDeviceSynchronize(); // enqueued calls may still read and write the history, and record the timer's events
  if (n->d_hist && hipFree(n->d_hist) != hipSuccess) rc = fail(BLAH2HIP_ERR_HIP, "hipFree(history)");
  if (n->d_ring && hipFree(n->d_ring) != hipSuccess) rc = fail(BLAH2HIP_ERR_HIP, "hipFree(ring)");
  if (n->d_tab && hipFree(n->d_tab) != hipSuccess) rc = fail(BLAH2HIP_ERR_HIP, "hipFree(track tables)");
  n->timer.destroy();
  delete n;
  return rc;
}

int blah2hip_nci_reset(blah2hip_nci_t n)
{
  if (!n) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  n->g = 0; // the planes keep their bytes: no window of the new count reaches them
  return BLAH2HIP_OK;
}

int blah2hip_nci_count(blah2hip_nci_t n, uint32_t n_cpi, uint32_t *n_out, uint64_t *first_end)
{
  if (!n) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  uint32_t no;
  uint64_t fe;
  windows_in(n, n_cpi, &no, &fe);
  if (n_out) *n_out = no;
  if (first_end) *first_end = fe;
  return BLAH2HIP_OK;
}

int blah2hip_nci_process_dev(blah2hip_nci_t n, const void *d_map, uint32_t n_cpi, const float *w, void *d_out_map,
                             double *d_out_metrics, uint32_t out_cap, uint32_t *n_out, uint64_t *first_end, void *stream)
{
  if (!n) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (n->tracks) return fail(BLAH2HIP_ERR_INVALID, "integrate: tracks are set, the history lives in the ring (blah2hip_nci_process_tracks_dev)");
  blah2hip_amb_s *h = n->amb;
  if (n_cpi == 0) return fail(BLAH2HIP_ERR_INVALID, "n_cpi is 0");
  if ((uint64_t)n->nSurv * n_cpi > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "n_surv * n_cpi above max_batch");
  uint32_t nOut;
  uint64_t first;
  windows_in(n, n_cpi, &nOut, &first);
  if (nOut > out_cap) return fail(BLAH2HIP_ERR_INVALID, "more output maps than out_cap");
  if (nOut > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "more output maps than max_batch");
  double wsum = 0.0;
  for (uint32_t k = 0; k < n->nSurv; k++) {
    const float wk = w ? w[k] : 1.f;
    if (!(wk >= 0.f) || !std::isfinite(wk)) return fail(BLAH2HIP_ERR_INVALID, "a channel weight is negative or not finite");
    wsum += (double)wk;
  }
  if (!(wsum > 0.0)) return fail(BLAH2HIP_ERR_INVALID, "the channel weights add up to 0");
  if (nOut > 0 && (!d_out_map || !d_out_metrics)) return fail(BLAH2HIP_ERR_INVALID, "NULL output");
  const size_t cells = (size_t)h->dims.n_doppler_bins * h->dims.n_delay_bins;
  const cf *in = d_map ? (const cf *)d_map : h->d_map;
  if ((uintptr_t)in & 7 || (nOut > 0 && ((uintptr_t)d_out_map & 7))) return fail(BLAH2HIP_ERR_INVALID, "a map is not 8-byte aligned");
  const size_t inBytes = (size_t)n->nSurv * n_cpi * cells * sizeof(cf);
  if (nOut > 0 && (ranges_overlap(in, inBytes, d_out_map, (size_t)nOut * cells * sizeof(cf)) ||
                   ranges_overlap(in, inBytes, d_out_metrics, (size_t)nOut * 2 * sizeof(double))))
    return fail(BLAH2HIP_ERR_INVALID, "integrate: an output overlaps the input maps");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;

  NciArgs a;
  a.in = in;
  a.out = (cf *)d_out_map;
  a.hist = n->d_hist;
  a.partSum = h->d_partSum;
  a.partMax = h->d_partMax;
  for (uint32_t k = 0; k < BLAH2HIP_MAX_SURV; k++) a.w[k] = k < n->nSurv ? (w ? w[k] : 1.f) : 0.f;
  a.scale = (float)(1.0 / ((double)n->window * wsum));
  a.cells = (uint32_t)cells;
  a.nCpi = n_cpi;
  a.K = n->nSurv;
  a.firstOut = nOut ? (uint32_t)(first - n->g) : n_cpi;
  a.hop = (uint32_t)std::min<uint64_t>(n->hop, n_cpi);
  a.histValid = (uint32_t)std::min<uint64_t>(n->g, n->window - 1);
  // Workgroups: one per 256 units of two cells (create has checked the handle's partials: nOut <= max_batch maps of nParts
  // each).  The grid depends on the map alone -- not on n_cpi, the counter or the outputs -- so a window's partials are the
  // same sums however the CPIs were cut into calls.
  const uint32_t G = (uint32_t)(((cells + 1) / 2 + 255) / 256);
  HIPCHK(n->timer.tic(BLAH2HIP_NK_NCI, st));
  launch_nci(n->window, dim3(G), st, a);
  HIPCHK(hipGetLastError());
  HIPCHK(n->timer.toc(BLAH2HIP_NK_NCI, st));
  n->g += n_cpi;
  if (n_out) *n_out = nOut;
  if (first_end) *first_end = first;
  if (nOut == 0) return BLAH2HIP_OK;
  return amb_metrics_enqueue(h, nOut, (int)G, (double)cells, d_out_metrics, st);
}

int blah2hip_nci_walk_table(blah2hip_amb_t amb, double fc, double cpi_spacing, double *walk)
{
  if (!amb || !walk) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (!std::isfinite(fc) || !(fc > 0.0)) return fail(BLAH2HIP_ERR_INVALID, "walk table: the carrier frequency must be finite and positive");
  if (!std::isfinite(cpi_spacing) || !(cpi_spacing > 0.0)) return fail(BLAH2HIP_ERR_INVALID, "walk table: the CPI spacing must be finite and positive");
  const double nCorr = (double)amb->dims.n_corr, nD = (double)amb->dims.n_doppler_bins;
  for (uint32_t j = 0; j < amb->dims.n_doppler_bins; j++) walk[j] = -amb->dopplerAxis[j] * nCorr * nD * cpi_spacing / fc;
  return BLAH2HIP_OK;
}

int blah2hip_nci_set_tracks(blah2hip_nci_t n, const double *walk, const double *q, uint32_t n_rates, uint32_t max_cpi)
{
  if (!n) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  blah2hip_amb_s *h = n->amb;
  const uint32_t nD = h->dims.n_doppler_bins, nDelay = h->dims.n_delay_bins, W = n->window;
  static const double zeroRate = 0.0;
  if (!q || n_rates == 0) { q = &zeroRate; n_rates = 1; }
  if (n_rates > BLAH2HIP_MAX_RATES) return fail(BLAH2HIP_ERR_INVALID, "tracks: more than BLAH2HIP_MAX_RATES hypotheses");
  if (max_cpi == 0) return fail(BLAH2HIP_ERR_INVALID, "tracks: max_cpi is 0");
  if ((uint64_t)n->nSurv * max_cpi > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "tracks: n_surv * max_cpi above max_batch");
  if ((uint64_t)nDelay >= (1ull << 31) - BLAH2HIP_MAX_TRACK_SHIFT) return fail(BLAH2HIP_ERR_INVALID, "tracks: n_delay too large for int32 columns");
  for (uint32_t k = 0; k < n_rates; k++) {
    if (!std::isfinite(q[k])) return fail(BLAH2HIP_ERR_INVALID, "tracks: a rate is not finite");
    if (!(std::fabs(q[k]) * (double)(W - 1) < (double)nD)) return fail(BLAH2HIP_ERR_INVALID, "tracks: a rate drifts n_doppler rows or more over the window");
  }
  if (walk)
    for (uint32_t j = 0; j < nD; j++)
      if (!std::isfinite(walk[j])) return fail(BLAH2HIP_ERR_INVALID, "tracks: a walk is not finite");
  // the tables, in fp64: r = rint(q a), jr = j - r, s = rint(-0.5 a (walk[j] + walk[jr])); (-1, 0) where jr leaves the map
  std::vector<int2> tab((size_t)n_rates * W * nD);
  int64_t maxShift = 0;
  for (uint32_t k = 0; k < n_rates; k++)
    for (uint32_t a = 0; a < W; a++) {
      const int64_t r = (int64_t)std::rint(q[k] * (double)a); // |q| (W - 1) < nD: fits
      for (uint32_t j = 0; j < nD; j++) {
        const int64_t jr = (int64_t)j - r;
        int2 e = make_int2(-1, 0);
        if (jr >= 0 && jr < (int64_t)nD) {
          const double s = walk ? std::rint(-0.5 * (double)a * (walk[j] + walk[jr])) : 0.0;
          if (!(std::fabs(s) <= (double)BLAH2HIP_MAX_TRACK_SHIFT))
            return fail(BLAH2HIP_ERR_INVALID, "tracks: a shift above BLAH2HIP_MAX_TRACK_SHIFT cells");
          e = make_int2((int)jr, (int)s);
          maxShift = std::max<int64_t>(maxShift, std::llabs((long long)s));
        }
        tab[((size_t)k * W + a) * nD + j] = e;
      }
    }
  // one metrics partial per workgroup of track_sum_kernel and output map in the handle's buffers: the Doppler kernels' tile
  const uint32_t strips = (nDelay + TRK_COLS - 1) / TRK_COLS, groups = (nD + TRK_ROWS - 1) / TRK_ROWS;
  if ((uint64_t)strips * groups > (uint64_t)h->nParts)
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "tracks: the handle holds fewer metrics partials per map than the kernel has workgroups");
  const size_t cells = (size_t)nD * nDelay;
  const uint32_t ringLen = W - 1 + max_cpi;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize()); // a launch in flight may still read the table and the ring
  float *ring = nullptr;
  int2 *dtab = nullptr;
  hipError_t e = hipMalloc(&ring, (size_t)ringLen * cells * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&dtab, tab.size() * sizeof(int2));
  if (e == hipSuccess) e = hipMemcpy(dtab, tab.data(), tab.size() * sizeof(int2), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(ring);
    (void)hipFree(dtab);
    return fail(BLAH2HIP_ERR_HIP, std::string("tracks: ") + hipGetErrorString(e));
  }
  (void)hipFree(n->d_ring);
  (void)hipFree(n->d_tab);
  n->d_ring = ring;
  n->d_tab = dtab;
  n->tracks = true;
  n->nRates = n_rates;
  n->maxCpi = max_cpi;
  n->ringLen = ringLen;
  n->g = 0;
  h->trackShiftLast = (int)maxShift;
  return BLAH2HIP_OK;
}

int blah2hip_nci_process_tracks_dev(blah2hip_nci_t n, const void *d_map, uint32_t n_cpi, const float *w, void *d_out_map,
                                    uint8_t *d_out_index, double *d_out_metrics, uint32_t out_cap, uint32_t *n_out,
                                    uint64_t *first_end, void *stream)
{
  if (!n) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (!n->tracks) return fail(BLAH2HIP_ERR_INVALID, "tracks: none set (blah2hip_nci_set_tracks)");
  blah2hip_amb_s *h = n->amb;
  if (n_cpi == 0) return fail(BLAH2HIP_ERR_INVALID, "n_cpi is 0");
  if (n_cpi > n->maxCpi) return fail(BLAH2HIP_ERR_INVALID, "tracks: n_cpi above the max_cpi of blah2hip_nci_set_tracks");
  if ((uint64_t)n->nSurv * n_cpi > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "n_surv * n_cpi above max_batch");
  uint32_t nOut;
  uint64_t first;
  windows_in(n, n_cpi, &nOut, &first);
  if (nOut > out_cap) return fail(BLAH2HIP_ERR_INVALID, "more output maps than out_cap");
  if (nOut > h->dims.max_batch || nOut > 65535) return fail(BLAH2HIP_ERR_INVALID, "more output maps than max_batch");
  double wsum = 0.0;
  for (uint32_t k = 0; k < n->nSurv; k++) {
    const float wk = w ? w[k] : 1.f;
    if (!(wk >= 0.f) || !std::isfinite(wk)) return fail(BLAH2HIP_ERR_INVALID, "a channel weight is negative or not finite");
    wsum += (double)wk;
  }
  if (!(wsum > 0.0)) return fail(BLAH2HIP_ERR_INVALID, "the channel weights add up to 0");
  if (nOut > 0 && (!d_out_map || !d_out_metrics)) return fail(BLAH2HIP_ERR_INVALID, "NULL output");
  const uint32_t nD = h->dims.n_doppler_bins, nDelay = h->dims.n_delay_bins;
  const size_t cells = (size_t)nD * nDelay;
  const cf *in = d_map ? (const cf *)d_map : h->d_map;
  if ((uintptr_t)in & 7 || (nOut > 0 && ((uintptr_t)d_out_map & 7))) return fail(BLAH2HIP_ERR_INVALID, "a map is not 8-byte aligned");
  const size_t inBytes = (size_t)n->nSurv * n_cpi * cells * sizeof(cf), outBytes = (size_t)nOut * cells * sizeof(cf);
  const size_t metBytes = (size_t)nOut * 2 * sizeof(double), idxBytes = (size_t)nOut * cells;
  if (nOut > 0 && (ranges_overlap(in, inBytes, d_out_map, outBytes) || ranges_overlap(in, inBytes, d_out_metrics, metBytes)))
    return fail(BLAH2HIP_ERR_INVALID, "integrate: an output overlaps the input maps");
  if (nOut > 0 && d_out_index && (ranges_overlap(in, inBytes, d_out_index, idxBytes) || ranges_overlap(d_out_map, outBytes, d_out_index, idxBytes) ||
                                  ranges_overlap(d_out_metrics, metBytes, d_out_index, idxBytes)))
    return fail(BLAH2HIP_ERR_INVALID, "tracks: the index plane overlaps a map or the metrics");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;

  // p of the call's CPIs into the ring.  Workgroups per group of NCI_GROUP CPIs: one per 256 units of two cells, from the
  // map alone, so p has the same bits however the CPIs are cut into calls.
  TrackPowerArgs pa;
  pa.n = NciArgs{};
  pa.n.in = in;
  for (uint32_t k = 0; k < BLAH2HIP_MAX_SURV; k++) pa.n.w[k] = k < n->nSurv ? (w ? w[k] : 1.f) : 0.f;
  pa.n.cells = (uint32_t)cells;
  pa.n.nCpi = n_cpi;
  pa.n.K = n->nSurv;
  pa.ring = n->d_ring;
  pa.ringLen = n->ringLen;
  pa.slot0 = (uint32_t)(n->g % n->ringLen);
  const uint32_t GP = (uint32_t)(((cells + 1) / 2 + 255) / 256);
  HIPCHK(n->timer.tic(BLAH2HIP_NK_TRACK_POWER, st));
  hipLaunchKernelGGL(track_power_kernel, dim3(GP, (n_cpi + NCI_GROUP - 1) / NCI_GROUP), dim3(256), 0, st, pa);
  HIPCHK(hipGetLastError());
  HIPCHK(n->timer.toc(BLAH2HIP_NK_TRACK_POWER, st));
  n->g += n_cpi;
  if (n_out) *n_out = nOut;
  if (first_end) *first_end = first;
  if (nOut == 0) return BLAH2HIP_OK;

  // The window sums: ceil(nDelay / 64) ceil(nD / 8) workgroups per output map (set_tracks has checked the handle's
  // partials), from the geometry alone; the outputs go along the grid's second axis.
  TrackSumArgs sa;
  sa.ring = n->d_ring;
  sa.tab = n->d_tab;
  sa.out = (cf *)d_out_map;
  sa.index = d_out_index;
  sa.partSum = h->d_partSum;
  sa.partMax = h->d_partMax;
  sa.scale = (float)(1.0 / ((double)n->window * wsum));
  sa.nD = (int32_t)nD;
  sa.nDelay = (int32_t)nDelay;
  sa.W = n->window;
  sa.K = n->nRates;
  sa.ringLen = n->ringLen;
  sa.slotFirst = (uint32_t)(first % n->ringLen);
  sa.hopMod = (uint32_t)(n->hop % n->ringLen);
  sa.strips = (nDelay + TRK_COLS - 1) / TRK_COLS;
  const uint32_t G = sa.strips * ((nD + TRK_ROWS - 1) / TRK_ROWS);
  HIPCHK(n->timer.tic(BLAH2HIP_NK_TRACK_SUM, st));
  hipLaunchKernelGGL(track_sum_kernel, dim3(G, nOut), dim3(256), 0, st, sa);
  HIPCHK(hipGetLastError());
  HIPCHK(n->timer.toc(BLAH2HIP_NK_TRACK_SUM, st));
  h->trackGridLast = (int)G;
  return amb_metrics_enqueue(h, nOut, (int)G, (double)cells, d_out_metrics, st);
}

int blah2hip_nci_set_timing(blah2hip_nci_t n, int enable)
{
  if (!n) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  n->timer.enabled = enable != 0;
  return BLAH2HIP_OK;
}

int blah2hip_nci_get_timing(blah2hip_nci_t n, double *ms_total, uint32_t *launches)
{
  if (!n || !ms_total || !launches) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(n->amb->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(n->timer.collect(ms_total, launches));
  return BLAH2HIP_OK;
}

} // extern "C"
