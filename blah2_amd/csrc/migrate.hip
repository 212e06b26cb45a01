// Range-migration compensation behind include/blah2hip.h: the table of half walks and the shifted Doppler sum over the
// range map that the last process call left on the handle.  Host code of blah2hip_migration_table,
// blah2hip_amb_set_migration and blah2hip_amb_migrate_dev; the kernel is migrate_kernels.hpp's.
#include "amb_handle.hpp"
#include "migrate_kernels.hpp"

#include <cmath>

using namespace blah2;

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
  if (h->lastMaps == 0) return fail(BLAH2HIP_ERR_INVALID, "migrate: no process call has left a range map on the handle");
  if (n_maps == 0 || n_maps > h->lastMaps || n_maps > 65535) return fail(BLAH2HIP_ERR_INVALID, "migrate: n_maps outside [1, maps of the last process call]");
  if (!d_out_map || !d_out_metrics) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  const uint32_t nD = h->dims.n_doppler_bins, nDelay = h->dims.n_delay_bins;
  const size_t cells = (size_t)nD * nDelay;
  const cf *in = d_map ? (const cf *)d_map : h->d_map;
  if ((uintptr_t)in & 7 || (uintptr_t)d_out_map & 7) return fail(BLAH2HIP_ERR_INVALID, "a map is not 8-byte aligned");
  const size_t bytes = (size_t)n_maps * cells * sizeof(cf), metBytes = (size_t)n_maps * 2 * sizeof(double);
  // a thread reads the one input cell it writes (zero-shift rows): the same buffer is fine, a shifted one is not
  if ((const void *)in != d_out_map && ranges_overlap(in, bytes, d_out_map, bytes))
    return fail(BLAH2HIP_ERR_INVALID, "migrate: the output maps overlap the input maps without being the same buffer");
  if (ranges_overlap(in, bytes, d_out_metrics, metBytes) || ranges_overlap(d_out_map, bytes, d_out_metrics, metBytes))
    return fail(BLAH2HIP_ERR_INVALID, "migrate: the metrics buffer lies inside a map");

  // Grid (column strips, row groups, maps), from the geometry alone -- never from n_maps.  A map's workgroups each leave a
  // metrics partial in the handle's buffers: strips * groups = ceil(nDelay / 64) ceil(nD / 32) of them, never more than the
  // ceil(nDelay / 64) ceil(nD / 8) that create set aside for doppler_dft_kernel, so the row groups need no widening.
  const uint32_t strips = (nDelay + MIG_COLS - 1) / MIG_COLS, groups = (nD + MIG_ROWS - 1) / MIG_ROWS;
  if (strips * groups > (uint32_t)h->nParts) return fail(BLAH2HIP_ERR_UNSUPPORTED, "migrate: the handle holds fewer metrics partials per map than the launch has workgroups");

  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  MigrateArgs a;
  a.R = h->d_R;
  a.in = in;
  a.out = (cf *)d_out_map;
  a.W = h->d_dopW;
  a.half = h->d_migrate;
  a.partSum = h->d_partSum;
  a.partMax = h->d_partMax;
  a.nD = (int32_t)nD;
  a.nDelay = (int32_t)nDelay;
  a.nTiles = h->nTiles;
  int rc;
  if ((rc = tic(h, BLAH2HIP_K_DOPPLER, st))) return rc;
  hipLaunchKernelGGL(migrate_kernel, dim3(strips, groups, n_maps), dim3(64 * MIG_WAVES), 0, st, a);
  HIPCHK(hipGetLastError());
  if ((rc = toc(h, BLAH2HIP_K_DOPPLER, st))) return rc;
  h->migrateGridLast = (int)(strips * groups);
  return amb_metrics_enqueue(h, n_maps, (int)(strips * groups), (double)cells, d_out_metrics, st);
}

} // extern "C"
