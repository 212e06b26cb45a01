// Doppler taper behind include/blah2hip.h: the taps of the named cosine-sum windows and the stencil over finished maps.
// Host code of blah2hip_doppler_taper and blah2hip_amb_taper_dev; the kernel is taper_kernels.hpp's.
#include "amb_handle.hpp"
#include "taper_kernels.hpp"

#include <cmath>

using namespace blah2;

namespace {

// a_0 .. a_P of w[i] = sum_p (-1)^p a_p cos(2 pi p i / n)
struct Window { int kind; uint32_t P; double a[BLAH2HIP_MAX_TAPER_SIDE + 1]; };
const Window WINDOWS[] = {
    {BLAH2HIP_TAPER_NONE, 0, {1.0}},
    {BLAH2HIP_TAPER_HANN, 1, {0.5, 0.5}},
    {BLAH2HIP_TAPER_HAMMING, 1, {0.54, 0.46}},
    {BLAH2HIP_TAPER_BLACKMAN, 2, {0.42, 0.5, 0.08}},
    {BLAH2HIP_TAPER_BLACKMAN_HARRIS, 3, {0.35875, 0.48829, 0.14128, 0.01168}},
    {BLAH2HIP_TAPER_NUTTALL, 3, {0.3635819, 0.4891775, 0.1365995, 0.0106411}},
    {BLAH2HIP_TAPER_FLATTOP, 4, {0.21557895, 0.41663158, 0.277263158, 0.083578947, 0.006947368}},
};

} // namespace

extern "C" {

int blah2hip_doppler_taper(int kind, int normalise, float *taps, uint32_t *n_side)
{
  if (!taps || !n_side) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  for (const Window &w : WINDOWS) {
    if (w.kind != kind) continue;
    const double norm = normalise ? w.a[0] : 1.0;
    for (uint32_t m = 0; m <= BLAH2HIP_MAX_TAPER_SIDE; m++) {
      const double t = m == 0 ? w.a[0] : m <= w.P ? ((m & 1) ? -0.5 : 0.5) * w.a[m] : 0.0;
      taps[m] = (float)(t / norm);
    }
    *n_side = w.P;
    return BLAH2HIP_OK;
  }
  return fail(BLAH2HIP_ERR_INVALID, "unknown window");
}

int blah2hip_amb_taper_dev(blah2hip_amb_t h, const void *d_map, uint32_t n_maps, const float *taps, uint32_t n_side,
                           void *d_out_map, double *d_out_metrics, void *stream)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  static_assert(BLAH2HIP_MAX_TAPER_SIDE == 4, "launch_taper covers the header's half widths");
  if (n_side > BLAH2HIP_MAX_TAPER_SIDE) return fail(BLAH2HIP_ERR_INVALID, "n_side above BLAH2HIP_MAX_TAPER_SIDE");
  const uint32_t nD = h->dims.n_doppler_bins, nDelay = h->dims.n_delay_bins;
  if (nD < 2 * n_side + 1) return fail(BLAH2HIP_ERR_INVALID, "taper: fewer Doppler bins than the stencil has taps");
  if (n_maps == 0 || n_maps > h->dims.max_batch || n_maps > 65535) return fail(BLAH2HIP_ERR_INVALID, "n_maps outside [1, max_batch]");
  if (!taps || !d_out_map || !d_out_metrics) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  for (uint32_t m = 0; m <= n_side; m++)
    if (!std::isfinite(taps[m])) return fail(BLAH2HIP_ERR_INVALID, "a tap is not finite");
  const size_t cells = (size_t)nD * nDelay;
  const cf *in = d_map ? (const cf *)d_map : h->d_map;
  if ((uintptr_t)in & 7 || (uintptr_t)d_out_map & 7) return fail(BLAH2HIP_ERR_INVALID, "a map is not 8-byte aligned");
  const size_t bytes = (size_t)n_maps * cells * sizeof(cf);
  if (ranges_overlap(in, bytes, d_out_map, bytes) || ranges_overlap(in, bytes, d_out_metrics, (size_t)n_maps * 2 * sizeof(double)))
    return fail(BLAH2HIP_ERR_INVALID, "taper: an output overlaps the input maps (the stencil cannot run in place)");

  // Grid (strips, segments, maps), from the map's geometry and BLAH2HIP_OPT_TAPER_SEG_ROWS alone -- never from n_maps: a
  // map's partials are then the same sums however the maps are cut into calls.  The launch's own choice: segments of 32
  // rows (the halo rows, 2 n_side a segment, are read twice: a quarter more at n_side 4), which gives a lone map of 513
  // rows 17 workgroups a strip.  A map's workgroups each leave a metrics partial in the handle's buffers (nParts a map):
  // longer segments where there would be more.
  const uint32_t strips = (nDelay + TAPER_COLS - 1) / TAPER_COLS;
  if (strips > (uint32_t)h->nParts) return fail(BLAH2HIP_ERR_UNSUPPORTED, "taper: the handle holds fewer metrics partials per map than the map has column strips");
  uint32_t seg = h->taperSegRows > 0 ? (uint32_t)h->taperSegRows : 32;
  seg = std::min(seg, nD);
  const uint32_t maxSegs = (uint32_t)h->nParts / strips;
  seg = std::max(seg, (nD + maxSegs - 1) / maxSegs);
  const uint32_t segs = (nD + seg - 1) / seg;
  if (segs > 65535) return fail(BLAH2HIP_ERR_UNSUPPORTED, "taper: more segments than a grid dimension holds");

  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  TaperArgs a;
  a.in = in;
  a.out = (cf *)d_out_map;
  a.partSum = h->d_partSum;
  a.partMax = h->d_partMax;
  for (uint32_t m = 0; m <= BLAH2HIP_MAX_TAPER_SIDE; m++) a.t[m] = m <= n_side ? taps[m] : 0.f;
  a.nD = nD;
  a.nDelay = nDelay;
  a.segRows = seg;
  int rc;
  if ((rc = tic(h, BLAH2HIP_K_BEAM, st))) return rc;
  launch_taper(n_side, dim3(strips, segs, n_maps), st, a);
  HIPCHK(hipGetLastError());
  if ((rc = toc(h, BLAH2HIP_K_BEAM, st))) return rc;
  h->taperGridLast = (int)(strips * segs);
  return amb_metrics_enqueue(h, n_maps, (int)(strips * segs), (double)cells, d_out_metrics, st);
}

} // extern "C"
