// Non-coherent integration behind include/blah2hip.h: the sum of |M|^2 over the surveillance channels and over a sliding
// window of consecutive CPIs.  Host code of the blah2hip_nci_* entry points; the kernel is integrate_kernels.hpp's.
#include "amb_handle.hpp"
#include "integrate_kernels.hpp"

#include <cmath>

using namespace blah2;

// The integrator: a window over the maps of ONE ambiguity handle (its geometry, partials, timer), the CPI counter and
// the history planes
struct blah2hip_nci_s {
  blah2hip_amb_s *amb = nullptr;
  uint32_t nSurv = 0, window = 0, hop = 0;
  uint64_t g = 0;          // CPIs since the creation or the last reset
  float *d_hist = nullptr; // [window - 1][cells]: p of the last window - 1 CPIs
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
