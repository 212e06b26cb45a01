// The receiver array behind include/blah2hip.h: beams and covariance of the channel maps and of the channels' samples,
// MVDR weights, per-detection snapshots and bearings.  Host code of the entry points; the kernels are beam_kernels.hpp's.
#include "amb_handle.hpp"
#include "beam_kernels.hpp"

#include <cmath>
#include <cstring>

using namespace blah2;

namespace {

// The counts the array calls share, in the order each of them checks them: channels, beams (NO_BEAMS: the call has none),
// CPIs and, with `batch`, the channel maps against the handle's max_batch
constexpr uint32_t NO_BEAMS = ~0u;
int counts_check(const blah2hip_amb_s *h, uint32_t n_surv, uint32_t n_beams, uint32_t n_cpi, bool batch)
{
  if (n_surv == 0 || n_surv > BLAH2HIP_MAX_SURV) return fail(BLAH2HIP_ERR_INVALID, "n_surv outside [1, BLAH2HIP_MAX_SURV]");
  if (n_beams != NO_BEAMS && (n_beams == 0 || n_beams > BLAH2HIP_MAX_BEAMS))
    return fail(BLAH2HIP_ERR_INVALID, "n_beams outside [1, BLAH2HIP_MAX_BEAMS]");
  if (n_cpi == 0) return fail(BLAH2HIP_ERR_INVALID, "n_cpi is 0");
  if (batch && (uint64_t)n_surv * n_cpi > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "n_surv * n_cpi above max_batch");
  return BLAH2HIP_OK;
}

// the host's w[b][k] (re, im) into the table of the launch arguments, whose other entries are zero; w == nullptr (the
// weights are on the device): all of them
void unpack_weights(cf (&dst)[BLAH2HIP_MAX_BEAMS][BLAH2HIP_MAX_SURV], const float *w, uint32_t n_beams, uint32_t n_surv)
{
  memset(dst, 0, sizeof(dst));
  if (!w) return;
  for (uint32_t b = 0; b < n_beams; b++)
    for (uint32_t k = 0; k < n_surv; k++) dst[b][k] = cmake(w[2 * (b * n_surv + k)], w[2 * (b * n_surv + k) + 1]);
}

// sample_cov_kernel for a plane format Ch: accesses of Ch::COVW samples (wide) or of one
template <class Ch> void sample_cov_launch(bool wide, uint32_t n_surv, dim3 grid, hipStream_t st, const SampCovArgs &a)
{
  if (wide) launch_sample_cov<Ch, Ch::COVW>(n_surv, grid, st, a);
  else launch_sample_cov<Ch, 1>(n_surv, grid, st, a);
}

// beam_samples_kernel (wdev == nullptr) or beam_samples_wdev_kernel for a plane format Ch: pairs of samples (wide) or single ones
template <class Ch>
void beam_samples_launch(bool wide, uint32_t n_surv, dim3 grid, hipStream_t st, const BeamSampArgs &a, const cf *wdev)
{
  if (wdev) { if (wide) launch_beam_samples<Ch, 2, true>(n_surv, grid, st, a, wdev); else launch_beam_samples<Ch, 1, true>(n_surv, grid, st, a, wdev); }
  else { if (wide) launch_beam_samples<Ch, 2, false>(n_surv, grid, st, a, wdev); else launch_beam_samples<Ch, 1, false>(n_surv, grid, st, a, wdev); }
}

} // namespace

extern "C" {

// ------------------------------------------------ beams in the map domain --
// blah2hip_amb_beamform_dev (w: the host's one set of weights) and blah2hip_amb_beamform_wdev (d_w: a set per CPI on the device)
static int beamform_enqueue(blah2hip_amb_t h, const void *d_map, uint32_t n_surv, uint32_t n_cpi, const float *w, const float *d_w,
                            uint32_t n_beams, void *d_beam_map, double *d_beam_metrics, void *stream)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  int rc;
  if ((rc = counts_check(h, n_surv, n_beams, n_cpi, true))) return rc;
  if ((uint64_t)n_beams * n_cpi > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "n_beams * n_cpi above max_batch");
  if ((!w && !d_w) || !d_beam_map || !d_beam_metrics) return fail(BLAH2HIP_ERR_INVALID, "NULL weights or output");
  const size_t cells = (size_t)h->dims.n_doppler_bins * h->dims.n_delay_bins;
  const cf *in = d_map ? (const cf *)d_map : h->d_map;
  const size_t inBytes = (size_t)n_surv * n_cpi * cells * sizeof(cf);
  if (ranges_overlap(in, inBytes, d_beam_map, (size_t)n_beams * n_cpi * cells * sizeof(cf)) ||
      ranges_overlap(in, inBytes, d_beam_metrics, (size_t)n_beams * n_cpi * 2 * sizeof(double)))
    return fail(BLAH2HIP_ERR_INVALID, "beamform: an output overlaps the input maps");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;

  BeamArgs a;
  a.in = in;
  a.out = (cf *)d_beam_map;
  a.partSum = h->d_partSum;
  a.partMax = h->d_partMax;
  a.cells = (uint32_t)cells;
  a.nCpi = n_cpi;
  a.nBeams = n_beams;
  unpack_weights(a.w, d_w ? nullptr : w, n_beams, n_surv);
  // 16-byte accesses where CPI c starts at the same offset modulo 16 bytes in every channel's and every beam's block: the
  // blocks are n_cpi * cells cells apart, so an odd product (odd cell count, odd n_cpi) with more than one block does not
  const bool oddBlock = ((size_t)n_cpi * cells) & 1;
  const bool wide = !(((uintptr_t)in ^ (uintptr_t)d_beam_map) & 15) && !((uintptr_t)in & 7) &&
                    !(oddBlock && (n_surv > 1 || n_beams > 1));
  // workgroups per CPI: no more than the handle has partials for (nParts per CPI of max_batch >= n_beams * n_cpi)
  const uint32_t G = groups_per_cpi(h, wide ? (cells + 1) / 2 : cells, n_cpi, (size_t)h->nParts);
  if ((rc = tic(h, BLAH2HIP_K_BEAM, st))) return rc;
  if (d_w) {
    if (wide) launch_beamform<2, true>(n_surv, dim3(G, n_cpi), st, a, (const cf *)d_w);
    else launch_beamform<1, true>(n_surv, dim3(G, n_cpi), st, a, (const cf *)d_w);
  } else {
    if (wide) launch_beamform<2, false>(n_surv, dim3(G, n_cpi), st, a, nullptr);
    else launch_beamform<1, false>(n_surv, dim3(G, n_cpi), st, a, nullptr);
  }
  HIPCHK(hipGetLastError());
  if ((rc = toc(h, BLAH2HIP_K_BEAM, st))) return rc;
  return amb_metrics_enqueue(h, n_beams * n_cpi, (int)G, (double)cells, d_beam_metrics, st);
}

int blah2hip_amb_beamform_dev(blah2hip_amb_t h, const void *d_map, uint32_t n_surv, uint32_t n_cpi, const float *w,
                              uint32_t n_beams, void *d_beam_map, double *d_beam_metrics, void *stream)
{
  return beamform_enqueue(h, d_map, n_surv, n_cpi, w, nullptr, n_beams, d_beam_map, d_beam_metrics, stream);
}

int blah2hip_amb_beamform_wdev(blah2hip_amb_t h, const void *d_map, uint32_t n_surv, uint32_t n_cpi, const float *d_w,
                               uint32_t n_beams, void *d_beam_map, double *d_beam_metrics, void *stream)
{
  return beamform_enqueue(h, d_map, n_surv, n_cpi, nullptr, d_w, n_beams, d_beam_map, d_beam_metrics, stream);
}

// ------------------------------------------------------- adaptive beams --
int blah2hip_amb_covariance_dev(blah2hip_amb_t h, const void *d_map, uint32_t n_surv, uint32_t n_cpi, uint32_t row0, uint32_t row1,
                                uint32_t col0, uint32_t col1, double *d_cov, void *stream)
{
  if (!h || !d_cov) return fail(BLAH2HIP_ERR_INVALID, "NULL handle or output");
  int rc;
  if ((rc = counts_check(h, n_surv, NO_BEAMS, n_cpi, true))) return rc;
  const uint32_t nD = h->dims.n_doppler_bins, nDelay = h->dims.n_delay_bins;
  if (row0 >= row1 || row1 > nD || col0 >= col1 || col1 > nDelay)
    return fail(BLAH2HIP_ERR_INVALID, "covariance: the training rectangle is empty or leaves the map");
  const size_t cells = (size_t)nD * nDelay;
  const cf *in = d_map ? (const cf *)d_map : h->d_map;
  const size_t KK = (size_t)n_surv * n_surv;
  if (ranges_overlap(in, (size_t)n_surv * n_cpi * cells * sizeof(cf), d_cov, (size_t)n_cpi * KK * 2 * sizeof(double)))
    return fail(BLAH2HIP_ERR_INVALID, "covariance: the output overlaps the input maps");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;

  CovArgs a;
  a.in = in;
  a.part = h->d_partSum;
  a.chStride = (size_t)n_cpi * cells;
  a.cells = (uint32_t)cells;
  a.nDelay = nDelay;
  a.row0 = row0; a.col0 = col0; a.nRows = row1 - row0; a.width = col1 - col0;
  // workgroups per CPI: no more than the handle's partials hold, n_cpi * G * K^2 doubles in max_batch * nParts
  // (n_surv * n_cpi <= max_batch and nParts >= 128, so there is room for 16 at the least)
  const size_t gCap = ((size_t)h->dims.max_batch * h->nParts) / ((size_t)n_cpi * KK);
  if (gCap == 0) return fail(BLAH2HIP_ERR_INVALID, "covariance: the handle's partials are too small");
  const uint32_t G = groups_per_cpi(h, (size_t)a.nRows * a.width, n_cpi, gCap);
  if ((rc = tic(h, BLAH2HIP_K_COV, st))) return rc;
  launch_array_cov(n_surv, dim3(G, n_cpi), st, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(cov_fold_kernel, dim3(n_cpi), dim3(64), 0, st, h->d_partSum, G, n_surv, d_cov);
  HIPCHK(hipGetLastError());
  return toc(h, BLAH2HIP_K_COV, st);
}

int blah2hip_amb_mvdr_weights_dev(blah2hip_amb_t h, const double *d_cov, uint32_t n_surv, uint32_t n_cpi, const float *steer,
                                  uint32_t n_beams, double loading, float *d_w, int32_t *d_ok, void *stream)
{
  if (!h || !d_cov || !steer || !d_w) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  int rc;
  if ((rc = counts_check(h, n_surv, n_beams, n_cpi, false))) return rc;
  if (!(loading >= 0.0) || !std::isfinite(loading)) return fail(BLAH2HIP_ERR_INVALID, "mvdr: loading is negative or not finite");
  MvdrArgs a;
  unpack_weights(a.steer, steer, n_beams, n_surv);
  for (uint32_t b = 0; b < n_beams; b++) {
    bool any = false;
    for (uint32_t k = 0; k < n_surv; k++) any = any || a.steer[b][k].x != 0.f || a.steer[b][k].y != 0.f;
    if (!any) return fail(BLAH2HIP_ERR_INVALID, "mvdr: a steering vector is all zero");
  }
  HIPCHK(hipSetDevice(h->device));
  a.cov = d_cov;
  a.w = (cf *)d_w;
  a.ok = d_ok;
  a.loading = loading;
  a.nBeams = n_beams;
  launch_mvdr_weights(n_surv, n_cpi, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return BLAH2HIP_OK;
}

// ------------------------------------------- the array in the sample domain --
// what the sample-domain calls share: format, counts, planes and their alignment, stride.  bytes: one sample of a plane.
static int sample_planes_check(blah2hip_amb_t h, int fmt, const void *const *d_y, uint32_t n_surv, uint32_t n_cpi, uint64_t cpi_stride,
                               size_t *bytes)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (fmt != BLAH2HIP_FMT_C32 && fmt != BLAH2HIP_FMT_I8)
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "sample-domain beams: BLAH2HIP_FMT_C32 or BLAH2HIP_FMT_I8 planes");
  int rc;
  if ((rc = counts_check(h, n_surv, NO_BEAMS, n_cpi, false))) return rc;
  if (!d_y) return fail(BLAH2HIP_ERR_INVALID, "NULL plane array");
  *bytes = fmt == BLAH2HIP_FMT_I8 ? 2 : 8;
  for (uint32_t k = 0; k < n_surv; k++) {
    if (!d_y[k]) return fail(BLAH2HIP_ERR_INVALID, "NULL plane");
    if ((uintptr_t)d_y[k] & (*bytes - 1))
      return fail(BLAH2HIP_ERR_INVALID, "a plane is not aligned to its sample (int8 pairs: 2 bytes, fp32 pairs: 8 bytes)");
  }
  if (n_cpi > 1 && cpi_stride < h->dims.n_samples) return fail(BLAH2HIP_ERR_INVALID, "cpi_stride < n_samples");
  return BLAH2HIP_OK;
}

// true where, CPI by CPI, sample `first` of every plane sits at the same offset modulo an access of V samples: the
// number of single samples in front of the first aligned access is then one number per CPI (it may differ between CPIs)
static bool sample_planes_agree(const void *const *planes, uint32_t n_planes, size_t bytes, uint64_t stride, uint32_t n_cpi,
                                uint32_t first, uint32_t V, const void *const *more = nullptr, uint32_t n_more = 0, size_t more_bytes = 0,
                                uint64_t more_stride = 0)
{
  for (uint32_t c = 0; c < n_cpi; c++) {
    const uint64_t at0 = ((uintptr_t)planes[0] / bytes + c * stride + first) % V;
    for (uint32_t k = 1; k < n_planes; k++)
      if (((uintptr_t)planes[k] / bytes + c * stride + first) % V != at0) return false;
    for (uint32_t b = 0; b < n_more; b++)
      if (((uintptr_t)more[b] / more_bytes + c * more_stride + first) % V != at0) return false;
  }
  return true;
}

int blah2hip_amb_sample_covariance_dev(blah2hip_amb_t h, int fmt, const void *const *d_y, uint32_t n_surv, uint32_t n_cpi,
                                       uint64_t cpi_stride, uint32_t s0, uint32_t s1, double *d_cov, void *stream)
{
  size_t bytes = 0;
  int rc;
  if ((rc = sample_planes_check(h, fmt, d_y, n_surv, n_cpi, cpi_stride, &bytes))) return rc;
  if (!d_cov) return fail(BLAH2HIP_ERR_INVALID, "NULL output");
  if ((uint64_t)n_surv * n_cpi > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "n_surv * n_cpi above max_batch");
  const uint32_t nS = h->dims.n_samples;
  if (s0 >= s1 || s1 > nS) return fail(BLAH2HIP_ERR_INVALID, "sample covariance: the window is empty or leaves the CPI");
  const size_t KK = (size_t)n_surv * n_surv;
  const size_t planeBytes = ((size_t)(n_cpi - 1) * cpi_stride + nS) * bytes;
  for (uint32_t k = 0; k < n_surv; k++)
    if (ranges_overlap(d_y[k], planeBytes, d_cov, (size_t)n_cpi * KK * 2 * sizeof(double)))
      return fail(BLAH2HIP_ERR_INVALID, "sample covariance: the output overlaps an input plane");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;

  SampCovArgs a;
  memset(a.y, 0, sizeof(a.y));
  for (uint32_t k = 0; k < n_surv; k++) a.y[k] = d_y[k];
  a.part = h->d_partSum;
  a.cpiStride = cpi_stride;
  a.s0 = s0;
  a.n = s1 - s0;
  const uint32_t V = fmt == BLAH2HIP_FMT_I8 ? SampI8::COVW : SampC32::COVW;
  const bool wide = sample_planes_agree(d_y, n_surv, bytes, cpi_stride, n_cpi, s0, V);
  // workgroups per CPI: blah2hip_amb_covariance_dev's rule, over accesses instead of cells
  const size_t gCap = ((size_t)h->dims.max_batch * h->nParts) / ((size_t)n_cpi * KK);
  if (gCap == 0) return fail(BLAH2HIP_ERR_INVALID, "sample covariance: the handle's partials are too small");
  const uint32_t G = groups_per_cpi(h, wide ? (a.n + V - 1) / V : a.n, n_cpi, gCap);
  if ((rc = tic(h, BLAH2HIP_K_COV, st))) return rc;
  if (fmt == BLAH2HIP_FMT_I8) sample_cov_launch<SampI8>(wide, n_surv, dim3(G, n_cpi), st, a);
  else sample_cov_launch<SampC32>(wide, n_surv, dim3(G, n_cpi), st, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(cov_fold_kernel, dim3(n_cpi), dim3(64), 0, st, h->d_partSum, G, n_surv, d_cov);
  HIPCHK(hipGetLastError());
  return toc(h, BLAH2HIP_K_COV, st);
}

// blah2hip_amb_beam_samples_dev (w: the host's one set of weights) and blah2hip_amb_beam_samples_wdev (d_w: a set per CPI on the device)
static int beam_samples_enqueue(blah2hip_amb_t h, int fmt, const void *const *d_y, uint32_t n_surv, uint32_t n_cpi, uint64_t cpi_stride,
                                const float *w, const float *d_w, uint32_t n_beams, void *const *d_beam, uint64_t beam_stride,
                                void *stream)
{
  size_t bytes = 0;
  int rc;
  if ((rc = sample_planes_check(h, fmt, d_y, n_surv, n_cpi, cpi_stride, &bytes))) return rc;
  if (n_beams == 0 || n_beams > BLAH2HIP_MAX_BEAMS) return fail(BLAH2HIP_ERR_INVALID, "n_beams outside [1, BLAH2HIP_MAX_BEAMS]");
  if ((!w && !d_w) || !d_beam) return fail(BLAH2HIP_ERR_INVALID, "NULL weights or output");
  const uint32_t nS = h->dims.n_samples;
  if (n_cpi > 1 && beam_stride < nS) return fail(BLAH2HIP_ERR_INVALID, "beam_stride < n_samples");
  const size_t inBytes = ((size_t)(n_cpi - 1) * cpi_stride + nS) * bytes;
  const size_t outBytes = ((size_t)(n_cpi - 1) * beam_stride + nS) * sizeof(cf);
  for (uint32_t b = 0; b < n_beams; b++) {
    if (!d_beam[b]) return fail(BLAH2HIP_ERR_INVALID, "NULL beam plane");
    if ((uintptr_t)d_beam[b] & 7) return fail(BLAH2HIP_ERR_INVALID, "a beam plane is not 8-byte aligned");
    for (uint32_t k = 0; k < n_surv; k++)
      if (ranges_overlap(d_y[k], inBytes, d_beam[b], outBytes)) return fail(BLAH2HIP_ERR_INVALID, "beam samples: a beam plane overlaps an input plane");
    for (uint32_t o = 0; o < b; o++)
      if (ranges_overlap(d_beam[o], outBytes, d_beam[b], outBytes)) return fail(BLAH2HIP_ERR_INVALID, "beam samples: two beam planes overlap");
  }
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;

  BeamSampArgs a;
  memset(a.y, 0, sizeof(a.y));
  memset(a.out, 0, sizeof(a.out));
  for (uint32_t k = 0; k < n_surv; k++) a.y[k] = d_y[k];
  for (uint32_t b = 0; b < n_beams; b++) a.out[b] = (cf *)d_beam[b];
  a.cpiStride = cpi_stride;
  a.beamStride = beam_stride;
  a.nSamples = nS;
  a.nBeams = n_beams;
  unpack_weights(a.w, d_w ? nullptr : w, n_beams, n_surv);
  // pairs of samples where every input plane's and every beam plane's copy of a CPI starts at the same parity of sample
  const bool wide = sample_planes_agree(d_y, n_surv, bytes, cpi_stride, n_cpi, 0, 2, (const void *const *)d_beam, n_beams, sizeof(cf), beam_stride);
  // workgroups per CPI: nothing caps them, the kernel leaves no partials
  const uint32_t G = groups_per_cpi(h, wide ? ((size_t)nS + 1) / 2 : nS, n_cpi);
  if ((rc = tic(h, BLAH2HIP_K_BEAM, st))) return rc;
  if (fmt == BLAH2HIP_FMT_I8) beam_samples_launch<SampI8>(wide, n_surv, dim3(G, n_cpi), st, a, (const cf *)d_w);
  else beam_samples_launch<SampC32>(wide, n_surv, dim3(G, n_cpi), st, a, (const cf *)d_w);
  HIPCHK(hipGetLastError());
  return toc(h, BLAH2HIP_K_BEAM, st);
}

int blah2hip_amb_beam_samples_dev(blah2hip_amb_t h, int fmt, const void *const *d_y, uint32_t n_surv, uint32_t n_cpi, uint64_t cpi_stride,
                                  const float *w, uint32_t n_beams, void *const *d_beam, uint64_t beam_stride, void *stream)
{
  return beam_samples_enqueue(h, fmt, d_y, n_surv, n_cpi, cpi_stride, w, nullptr, n_beams, d_beam, beam_stride, stream);
}

int blah2hip_amb_beam_samples_wdev(blah2hip_amb_t h, int fmt, const void *const *d_y, uint32_t n_surv, uint32_t n_cpi, uint64_t cpi_stride,
                                   const float *d_w, uint32_t n_beams, void *const *d_beam, uint64_t beam_stride, void *stream)
{
  return beam_samples_enqueue(h, fmt, d_y, n_surv, n_cpi, cpi_stride, nullptr, d_w, n_beams, d_beam, beam_stride, stream);
}

int blah2hip_amb_snapshot_dev(blah2hip_amb_t h, const void *d_map, uint32_t n_surv, uint32_t n_cpi,
                              const blah2hip_det_t *d_dets, uint32_t cap, const uint32_t *d_count, uint32_t n_lists,
                              float *d_snap, void *stream)
{
  if (!h || !d_dets || !d_count || !d_snap) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (n_surv == 0 || n_surv > BLAH2HIP_MAX_SURV) return fail(BLAH2HIP_ERR_INVALID, "n_surv outside [1, BLAH2HIP_MAX_SURV]");
  if (n_cpi == 0 || (uint64_t)n_surv * n_cpi > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "n_cpi is 0 or n_surv * n_cpi above max_batch");
  if (cap == 0) return fail(BLAH2HIP_ERR_INVALID, "cap is 0");
  if (n_lists == 0 || n_lists % n_cpi != 0) return fail(BLAH2HIP_ERR_INVALID, "n_lists is 0 or not a multiple of n_cpi");
  HIPCHK(hipSetDevice(h->device));
  SnapArgs a;
  a.map = d_map ? (const cf *)d_map : h->d_map;
  a.dets = d_dets;
  a.count = d_count;
  a.snap = (cf *)d_snap;
  a.nSurv = n_surv; a.nCpi = n_cpi; a.cap = cap; a.nLists = n_lists;
  a.nD = (int32_t)h->dims.n_doppler_bins;
  a.nDelay = (int32_t)h->dims.n_delay_bins;
  const size_t blocks = ((size_t)n_lists * cap + 255) / 256;
  hipLaunchKernelGGL(snapshot_kernel, dim3((uint32_t)std::min<size_t>(blocks, 8u * (size_t)h->numCU)), dim3(256), 0,
                     (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return BLAH2HIP_OK;
}

int blah2hip_amb_bearing_dev(blah2hip_amb_t h, const void *d_map, uint32_t n_surv, uint32_t n_cpi,
                             const blah2hip_det_t *d_dets, uint32_t cap, const uint32_t *d_count, uint32_t n_lists,
                             const double *d_cov, double loading, const float *d_steer, uint32_t n_grid, uint32_t flags,
                             blah2hip_bearing_t *d_out, void *stream)
{
  if (!h || !d_dets || !d_count || !d_steer || !d_out) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (n_surv < 2 || n_surv > BLAH2HIP_MAX_SURV) return fail(BLAH2HIP_ERR_INVALID, "n_surv outside [2, BLAH2HIP_MAX_SURV]");
  if (n_cpi == 0 || (uint64_t)n_surv * n_cpi > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "n_cpi is 0 or n_surv * n_cpi above max_batch");
  if (cap == 0) return fail(BLAH2HIP_ERR_INVALID, "cap is 0");
  if (n_lists == 0 || n_lists % n_cpi != 0 || n_lists > 65535)
    return fail(BLAH2HIP_ERR_INVALID, "n_lists is 0, not a multiple of n_cpi or above 65535");
  if (n_grid < 3 || n_grid > BLAH2HIP_MAX_BEARING_GRID) return fail(BLAH2HIP_ERR_INVALID, "n_grid outside [3, BLAH2HIP_MAX_BEARING_GRID]");
  if (flags & ~BLAH2HIP_BEARING_WRAP) return fail(BLAH2HIP_ERR_INVALID, "bearing: unknown flag bits");
  if (d_cov && (!(loading >= 0.0) || !std::isfinite(loading))) return fail(BLAH2HIP_ERR_INVALID, "bearing: loading is negative or not finite");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  BearingArgs a;
  a.map = d_map ? (const cf *)d_map : h->d_map;
  a.dets = d_dets;
  a.count = d_count;
  a.cov = d_cov;
  a.steer = (const cf *)d_steer;
  a.out = d_out;
  a.loading = d_cov ? loading : 0.0;
  a.nCpi = n_cpi; a.cap = cap; a.nGrid = n_grid;
  a.wrap = flags & BLAH2HIP_BEARING_WRAP;
  a.nD = (int32_t)h->dims.n_doppler_bins;
  a.nDelay = (int32_t)h->dims.n_delay_bins;
  // workgroups per list: the count lives on the device, so one per BEARING_CHUNK slots of cap (those behind the count return
  // before they build the table), and no more than eight a CU over the launch: a workgroup strides over the chunks
  const uint32_t X = std::max(1u, std::min(cap / BEARING_CHUNK + (cap % BEARING_CHUNK ? 1u : 0u), 8u * (uint32_t)h->numCU / n_lists));
  int rc;
  if ((rc = tic(h, BLAH2HIP_K_BEARING, st))) return rc;
  launch_bearing(n_surv, dim3(X, n_lists), st, a);
  HIPCHK(hipGetLastError());
  h->bearingGridLast = (int)X;
  return toc(h, BLAH2HIP_K_BEARING, st);
}

} // extern "C"
