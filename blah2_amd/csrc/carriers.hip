// Multi-carrier integration behind include/blah2hip.h: the table that aligns every carrier's Doppler rows with the
// handle's axis, and the gather-and-sum over the carriers' maps.  Host code of blah2hip_carrier_table,
// blah2hip_amb_set_carriers and blah2hip_amb_fuse_carriers_dev; the kernel is carrier_kernels.hpp's.
#include "amb_handle.hpp"
#include "carrier_kernels.hpp"

#include <cmath>

using namespace blah2;

static_assert(BLAH2HIP_MAX_CARRIERS == 8, "launch_carrier_sum covers the header's carrier counts");
static_assert(BLAH2HIP_MAX_CARRIERS >= BLAH2HIP_MAX_DDC_CARRIERS, "every carrier the down-converter produces can be summed");
static_assert(sizeof(CarrierEntry) == 16, "one scalar load of four words per entry");

// The header's table in fp64, entry [c * nD + j], and the rows' cover counts; the one builder behind the host-only
// function and the upload, so the device never sums along another table than the one a caller can read.
static int carrier_table_build(blah2hip_amb_t h, const double *ratio, uint32_t n, int interp, std::vector<CarrierEntry> &tab,
                               std::vector<uint32_t> &covered)
{
  if (!ratio) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (n == 0 || n > BLAH2HIP_MAX_CARRIERS) return fail(BLAH2HIP_ERR_INVALID, "carriers: n_carriers outside [1, BLAH2HIP_MAX_CARRIERS]");
  if (interp != BLAH2HIP_CARRIER_NEAREST && interp != BLAH2HIP_CARRIER_LINEAR) return fail(BLAH2HIP_ERR_INVALID, "carriers: unknown interpolation");
  for (uint32_t c = 0; c < n; c++)
    if (!std::isfinite(ratio[c]) || !(ratio[c] >= 0.5 && ratio[c] <= 2.0))
      return fail(BLAH2HIP_ERR_INVALID, "carriers: a ratio is not finite or lies outside [0.5, 2]");
  const uint32_t nD = h->dims.n_doppler_bins;
  if (nD < 2) return fail(BLAH2HIP_ERR_INVALID, "carriers: fewer than two Doppler bins");
  const std::vector<double> &dop = h->dopplerAxis;
  const double top = (double)(nD - 1);
  const double span = dop[nD - 1] - dop[0];
  const double delta = span / top;
  tab.assign((size_t)n * nD, CarrierEntry{0, 1.f, 0.f, 0u});
  covered.assign(nD, 0u);
  for (uint32_t c = 0; c < n; c++)
    for (uint32_t j = 0; j < nD; j++) {
      // one operation a statement: no contraction into a fused multiply-add, the restatement's bits
      const double scaled = ratio[c] * dop[j];
      const double off = scaled - dop[0];
      double u = off / delta;
      const double r = std::rint(u);
      if (std::fabs(u - r) <= 1e-9) u = r;
      if (u >= 0.0 && u <= top) covered[j]++;
      u = std::min(std::max(u, 0.0), top); // the edge row stands in
      CarrierEntry &e = tab[(size_t)c * nD + j];
      if (interp == BLAH2HIP_CARRIER_NEAREST) {
        e.row = (int32_t)std::floor(u + 0.5);
      } else {
        const double lo = std::floor(u);
        const double t = u - lo;
        e.row = (int32_t)lo;
        e.aHi = (float)t;
        e.aLo = (float)(1.0 - t);
      }
    }
  return BLAH2HIP_OK;
}

extern "C" {

int blah2hip_carrier_table(blah2hip_amb_t h, const double *ratio, uint32_t n_carriers, int interp, int32_t *row, float *a_lo,
                           float *a_hi, uint32_t *covered)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  std::vector<CarrierEntry> tab;
  std::vector<uint32_t> cov;
  const int rc = carrier_table_build(h, ratio, n_carriers, interp, tab, cov);
  if (rc) return rc;
  for (size_t i = 0; i < tab.size(); i++) {
    if (row) row[i] = tab[i].row;
    if (a_lo) a_lo[i] = tab[i].aLo;
    if (a_hi) a_hi[i] = tab[i].aHi;
  }
  if (covered) std::copy(cov.begin(), cov.end(), covered);
  return BLAH2HIP_OK;
}

int blah2hip_amb_set_carriers(blah2hip_amb_t h, const double *ratio, uint32_t n_carriers, int interp)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (n_carriers == 0) {
    h->nCarriers = 0;
    return BLAH2HIP_OK;
  }
  std::vector<CarrierEntry> tab;
  std::vector<uint32_t> cov;
  const int rc = carrier_table_build(h, ratio, n_carriers, interp, tab, cov);
  if (rc) return rc;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize()); // a launch in flight may still read the table
  if (!h->d_carriers) HIPCHK(hipMalloc(&h->d_carriers, (size_t)BLAH2HIP_MAX_CARRIERS * h->dims.n_doppler_bins * sizeof(CarrierEntry)));
  HIPCHK(hipMemcpy(h->d_carriers, tab.data(), tab.size() * sizeof(CarrierEntry), hipMemcpyHostToDevice));
  h->nCarriers = n_carriers;
  return BLAH2HIP_OK;
}

int blah2hip_amb_fuse_carriers_dev(blah2hip_amb_t h, const void *d_map, uint32_t n_cpi, const float *w, void *d_out_map,
                                   double *d_out_metrics, void *stream)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  const uint32_t C = h->nCarriers;
  if (C == 0) return fail(BLAH2HIP_ERR_INVALID, "fuse carriers: no table set (blah2hip_amb_set_carriers)");
  if (n_cpi == 0 || n_cpi > 65535 || (uint64_t)C * n_cpi > h->dims.max_batch)
    return fail(BLAH2HIP_ERR_INVALID, "fuse carriers: n_cpi is 0 or n_carriers * n_cpi above max_batch");
  if (!d_out_map || !d_out_metrics) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  double wsum = 0.0;
  for (uint32_t c = 0; c < C; c++) {
    const float wc = w ? w[c] : 1.f;
    if (!(wc >= 0.f) || !std::isfinite(wc)) return fail(BLAH2HIP_ERR_INVALID, "a carrier weight is negative or not finite");
    wsum += (double)wc;
  }
  if (!(wsum > 0.0)) return fail(BLAH2HIP_ERR_INVALID, "the carrier weights add up to 0");
  const uint32_t nD = h->dims.n_doppler_bins, nDelay = h->dims.n_delay_bins;
  const size_t cells = (size_t)nD * nDelay;
  const cf *in = d_map ? (const cf *)d_map : h->d_map;
  if ((uintptr_t)in & 7 || (uintptr_t)d_out_map & 7) return fail(BLAH2HIP_ERR_INVALID, "a map is not 8-byte aligned");
  const size_t inBytes = (size_t)C * n_cpi * cells * sizeof(cf), outBytes = (size_t)n_cpi * cells * sizeof(cf);
  const size_t metBytes = (size_t)n_cpi * 2 * sizeof(double);
  if (ranges_overlap(in, inBytes, d_out_map, outBytes) || ranges_overlap(in, inBytes, d_out_metrics, metBytes))
    return fail(BLAH2HIP_ERR_INVALID, "fuse carriers: an output overlaps the input maps (the gather cannot run in place)");
  if (ranges_overlap(d_out_map, outBytes, d_out_metrics, metBytes))
    return fail(BLAH2HIP_ERR_INVALID, "fuse carriers: the metrics buffer lies inside the output maps");

  // Grid (strips * row groups, CPIs), from the map's geometry alone -- never from n_cpi: a map's bits and partials are the
  // same however the CPIs are cut into calls.  strips * groups = ceil(nDelay / 64) ceil(nD / 8): what create set aside for
  // doppler_dft_kernel.
  const uint32_t strips = (nDelay + CAR_COLS - 1) / CAR_COLS, groups = (nD + CAR_ROWS - 1) / CAR_ROWS;
  if ((uint64_t)strips * groups > (uint64_t)h->nParts)
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "fuse carriers: the handle holds fewer metrics partials per map than the launch has workgroups");

  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  CarrierArgs a;
  a.in = in;
  a.tab = (const CarrierEntry *)h->d_carriers;
  a.out = (cf *)d_out_map;
  a.partSum = h->d_partSum;
  a.partMax = h->d_partMax;
  for (uint32_t c = 0; c < BLAH2HIP_MAX_CARRIERS; c++) a.w[c] = c < C ? (w ? w[c] : 1.f) : 0.f;
  a.scale = (float)(1.0 / wsum);
  a.nD = (int32_t)nD;
  a.nDelay = (int32_t)nDelay;
  a.nCpi = n_cpi;
  a.strips = strips;
  int rc;
  if ((rc = tic(h, BLAH2HIP_K_BEAM, st))) return rc;
  launch_carrier_sum(C, dim3(strips * groups, n_cpi), st, a);
  HIPCHK(hipGetLastError());
  if ((rc = toc(h, BLAH2HIP_K_BEAM, st))) return rc;
  h->carrierGridLast = (int)(strips * groups);
  return amb_metrics_enqueue(h, n_cpi, (int)(strips * groups), (double)cells, d_out_metrics, st);
}

} // extern "C"
