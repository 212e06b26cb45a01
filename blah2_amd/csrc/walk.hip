// Walk sums behind include/blah2hip.h: the table of half walks, the chirp table of a bank of Doppler rates, and the shifted
// (and chirped) Doppler sum over the range map that the last process call left on the handle.  Host code of
// blah2hip_migration_table, blah2hip_amb_set_migration, blah2hip_amb_migrate_dev, blah2hip_doppler_rate,
// blah2hip_amb_set_rates and blah2hip_amb_rate_bank_dev; the kernel is walk_kernels.hpp's, in its two shapes.
#include "amb_handle.hpp"
#include "walk_kernels.hpp"

#include <cmath>

using namespace blah2;

// The launch of both _dev entry points, behind their own precondition.  `what` opens the error texts, `rows` is the kernel's
// rows per workgroup, `gridLast` the handle's BLAH2HIP_INFO_*_GRID word of the entry point.
static int walk_launch(blah2hip_amb_t h, const std::string &what, const void *d_map, uint32_t n_maps, void *d_out_map, uint8_t *d_out_index,
                       double *d_out_metrics, void *stream, uint32_t rows, void (*kernel)(WalkArgs), int *gridLast)
{
  if (h->lastMaps == 0) return fail(BLAH2HIP_ERR_INVALID, what + ": no process call has left a range map on the handle");
  if (n_maps == 0 || n_maps > h->lastMaps || n_maps > 65535) return fail(BLAH2HIP_ERR_INVALID, what + ": n_maps outside [1, maps of the last process call]");
  if (!d_out_map || !d_out_metrics) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  const uint32_t nD = h->dims.n_doppler_bins, nDelay = h->dims.n_delay_bins;
  const size_t cells = (size_t)nD * nDelay;
  const cf *in = d_map ? (const cf *)d_map : h->d_map;
  if ((uintptr_t)in & 7 || (uintptr_t)d_out_map & 7) return fail(BLAH2HIP_ERR_INVALID, "a map is not 8-byte aligned");
  const size_t bytes = (size_t)n_maps * cells * sizeof(cf), metBytes = (size_t)n_maps * 2 * sizeof(double), idxBytes = (size_t)n_maps * cells;
  // a thread reads the one input cell it writes (zero-shift rows): the same buffer is fine, a shifted one is not
  if ((const void *)in != d_out_map && ranges_overlap(in, bytes, d_out_map, bytes))
    return fail(BLAH2HIP_ERR_INVALID, what + ": the output maps overlap the input maps without being the same buffer");
  if (ranges_overlap(in, bytes, d_out_metrics, metBytes) || ranges_overlap(d_out_map, bytes, d_out_metrics, metBytes))
    return fail(BLAH2HIP_ERR_INVALID, what + ": the metrics buffer lies inside a map");
  if (d_out_index && (ranges_overlap(in, bytes, d_out_index, idxBytes) || ranges_overlap(d_out_map, bytes, d_out_index, idxBytes) ||
                      ranges_overlap(d_out_metrics, metBytes, d_out_index, idxBytes)))
    return fail(BLAH2HIP_ERR_INVALID, what + ": the index plane overlaps a map or the metrics");

  // Grid (column strips, row groups, maps), from the geometry alone -- never from n_maps, and a bank goes in passes inside
  // the workgroup.  A map's workgroups each leave a metrics partial in the handle's buffers: strips * groups =
  // ceil(nDelay / 64) ceil(nD / rows) of them, rows 32 or 16, never more than the ceil(nDelay / 64) ceil(nD / 8) that create
  // set aside for doppler_dft_kernel, so the row groups need no widening.
  const uint32_t strips = (nDelay + WALK_COLS - 1) / WALK_COLS, groups = (nD + rows - 1) / rows;
  if (strips * groups > (uint32_t)h->nParts) return fail(BLAH2HIP_ERR_UNSUPPORTED, what + ": the handle holds fewer metrics partials per map than the launch has workgroups");

  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  WalkArgs a;
  a.R = h->d_R;
  a.in = in;
  a.out = (cf *)d_out_map;
  a.index = d_out_index;
  a.W = h->d_dopW;
  a.half = h->migrateSet ? h->d_migrate : nullptr;
  a.chirp = h->d_rates;
  a.partSum = h->d_partSum;
  a.partMax = h->d_partMax;
  a.nD = (int32_t)nD;
  a.nDelay = (int32_t)nDelay;
  a.nTiles = h->nTiles;
  a.nRates = h->nRates;
  a.zeroRates = h->zeroRates;
  int rc;
  if ((rc = tic(h, BLAH2HIP_K_DOPPLER, st))) return rc;
  hipLaunchKernelGGL(kernel, dim3(strips, groups, n_maps), dim3(64 * WALK_WAVES), 0, st, a);
  HIPCHK(hipGetLastError());
  if ((rc = toc(h, BLAH2HIP_K_DOPPLER, st))) return rc;
  *gridLast = (int)(strips * groups);
  return amb_metrics_enqueue(h, n_maps, (int)(strips * groups), (double)cells, d_out_metrics, st);
}

extern "C" {

int blah2hip_migration_table(blah2hip_amb_t h, double fc, double *half_walk)
{
  if (!h || !half_walk) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (!std::isfinite(fc) || !(fc > 0.0)) return fail(BLAH2HIP_ERR_INVALID, "migration: the carrier frequency must be finite and positive");
  const double nCorr = (double)h->dims.n_corr;
  for (uint32_t j = 0; j < h->dims.n_doppler_bins; j++) half_walk[j] = -0.5 * h->dopplerAxis[j] * nCorr / fc;
  return BLAH2HIP_OK;
}

int blah2hip_amb_set_migration(blah2hip_amb_t h, const double *half_walk)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (!half_walk) {
    h->migrateSet = false;
    return BLAH2HIP_OK;
  }
  const uint32_t nD = h->dims.n_doppler_bins;
  for (uint32_t j = 0; j < nD; j++) {
    if (!std::isfinite(half_walk[j])) return fail(BLAH2HIP_ERR_INVALID, "migration: a half walk is not finite");
    if (!(std::fabs(std::rint(half_walk[j] * (double)(nD - 1))) <= (double)BLAH2HIP_MAX_MIGRATION))
      return fail(BLAH2HIP_ERR_INVALID, "migration: a row walks more than BLAH2HIP_MAX_MIGRATION cells from the middle of the CPI");
  }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize()); // a launch in flight may still read the table
  if (!h->d_migrate) HIPCHK(hipMalloc(&h->d_migrate, nD * sizeof(double)));
  HIPCHK(hipMemcpy(h->d_migrate, half_walk, nD * sizeof(double), hipMemcpyHostToDevice));
  h->migrateSet = true;
  return BLAH2HIP_OK;
}

int blah2hip_amb_migrate_dev(blah2hip_amb_t h, const void *d_map, uint32_t n_maps, void *d_out_map, double *d_out_metrics, void *stream)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (!h->migrateSet) return fail(BLAH2HIP_ERR_INVALID, "migrate: no table set (blah2hip_amb_set_migration)");
  return walk_launch(h, "migrate", d_map, n_maps, d_out_map, nullptr, d_out_metrics, stream, WALK_WAVES * 8, walk_sum_kernel<8, 1>, &h->migrateGridLast);
}

int blah2hip_doppler_rate(blah2hip_amb_t h, double fc, double accel, double *q)
{
  if (!h || !q) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (!std::isfinite(fc) || !(fc > 0.0)) return fail(BLAH2HIP_ERR_INVALID, "doppler rate: the carrier frequency must be finite and positive");
  if (!std::isfinite(accel)) return fail(BLAH2HIP_ERR_INVALID, "doppler rate: the acceleration must be finite");
  const double T = (double)h->dims.n_doppler_bins * (double)h->dims.n_corr / (double)h->fs;
  *q = -accel * fc / 299792458.0 * T * T;
  return BLAH2HIP_OK;
}

int blah2hip_amb_set_rates(blah2hip_amb_t h, const double *q, uint32_t n_rates)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (!q || n_rates == 0) {
    h->nRates = 0;
    return BLAH2HIP_OK;
  }
  if (n_rates > BLAH2HIP_MAX_RATES) return fail(BLAH2HIP_ERR_INVALID, "rates: more than BLAH2HIP_MAX_RATES hypotheses");
  const uint32_t nD = h->dims.n_doppler_bins;
  uint32_t zero = 0;
  for (uint32_t k = 0; k < n_rates; k++) {
    if (!std::isfinite(q[k])) return fail(BLAH2HIP_ERR_INVALID, "rates: a rate is not finite");
    if (!(std::fabs(q[k]) <= (double)nD)) return fail(BLAH2HIP_ERR_INVALID, "rates: a rate drifts more than n_doppler bins over the CPI");
    if (q[k] == 0.0) zero |= 1u << k;
  }
  // c_k[i] = exp(-i theta_k(i)), theta_k(i) = pi q[k] t(i)^2 / (4 nD^2) in fp64, rounded to fp32
  std::vector<cf> table((size_t)n_rates * nD);
  const double den = 4.0 * (double)nD * (double)nD;
  for (uint32_t k = 0; k < n_rates; k++)
    for (uint32_t i = 0; i < nD; i++) {
      const int64_t t = 2 * (int64_t)i - ((int64_t)nD - 1);
      const double th = M_PI * q[k] * (double)(t * t) / den;
      table[(size_t)k * nD + i] = cmake((float)std::cos(th), (float)(-std::sin(th)));
    }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize()); // a launch in flight may still read the table
  if (!h->d_rates) HIPCHK(hipMalloc(&h->d_rates, (size_t)BLAH2HIP_MAX_RATES * nD * sizeof(cf)));
  HIPCHK(hipMemcpy(h->d_rates, table.data(), table.size() * sizeof(cf), hipMemcpyHostToDevice));
  h->nRates = n_rates;
  h->zeroRates = zero;
  return BLAH2HIP_OK;
}

int blah2hip_amb_rate_bank_dev(blah2hip_amb_t h, const void *d_map, uint32_t n_maps, void *d_out_map, uint8_t *d_out_index,
                               double *d_out_metrics, void *stream)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (h->nRates == 0) return fail(BLAH2HIP_ERR_INVALID, "rate bank: no bank set (blah2hip_amb_set_rates)");
  return walk_launch(h, "rate bank", d_map, n_maps, d_out_map, d_out_index, d_out_metrics, stream, WALK_WAVES * 4, walk_sum_kernel<4, 2>, &h->rateGridLast);
}

} // extern "C"
