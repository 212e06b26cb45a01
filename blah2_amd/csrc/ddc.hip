// Digital down-converter behind include/blah2hip.h: mix, low-pass and decimate up to eight carriers of a two-channel
// stream.  Host code of the blah2hip_ddc_* entry points; the kernels are ddc_kernels.hpp's.  Everything is allocated by
// create: reset and the dev entry point only enqueue.
#include "amb_handle.hpp"
#include "ddc_kernels.hpp"

#include <cmath>

using namespace blah2;

struct blah2hip_ddc_s {
  int device = 0;
  double fs = 0.0;
  uint32_t D = 0, T = 0, C = 0, CB = 1, Cpad = 0;
  uint32_t maxIn = 0, maxRows = 0;
  DdcPlan plan{};
  cf *d_taps = nullptr;        // [Cpad][T], entry s = g_c[T - 1 - s]; zeros behind the carriers
  double *d_r = nullptr;       // [Cpad] f_c D / fs
  cf *d_hist = nullptr;        // [2][T - 1]
  uint64_t *d_pos = nullptr;   // absolute index of the next output
  uint64_t nextSample = 0;     // ... of the next input sample, as the calls made so far leave it
  KernelTimer<BLAH2HIP_DK_COUNT> timer;
};

namespace {

bool sizes_ok(uint32_t decim, uint32_t n_taps)
{
  return decim >= 1 && decim <= BLAH2HIP_MAX_DDC_DECIM && n_taps >= 1 && n_taps <= BLAH2HIP_MAX_DDC_TAPS;
}

// I0 by its series sum_k ((x / 2)^k / k!)^2
double bessel_i0(double x)
{
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 1000; k++) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

size_t in_bytes(int fmt) { return fmt == BLAH2HIP_FMT_I8 ? 2 : 8; }

template <int R> void launch_r(uint32_t CB, dim3 grid, dim3 block, size_t lds, hipStream_t st, const DdcArgs &a)
{
  if (CB == 1) hipLaunchKernelGGL((ddc_kernel<R, 1>), grid, block, lds, st, a);
  else if (CB == 2) hipLaunchKernelGGL((ddc_kernel<R, 2>), grid, block, lds, st, a);
  else hipLaunchKernelGGL((ddc_kernel<R, 4>), grid, block, lds, st, a);
}

template <int R> hipError_t ensure_r(int bytes)
{
  hipError_t e = blah2hip_ensure_lds_((const void *)ddc_kernel<R, 1>, bytes);
  if (e == hipSuccess) e = blah2hip_ensure_lds_((const void *)ddc_kernel<R, 2>, bytes);
  if (e == hipSuccess) e = blah2hip_ensure_lds_((const void *)ddc_kernel<R, 4>, bytes);
  return e;
}

} // namespace

extern "C" {

int blah2hip_ddc_design(uint32_t decim, uint32_t n_taps, double cutoff, double beta, double *h)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "ddc design: NULL table");
  if (!sizes_ok(decim, n_taps)) return fail(BLAH2HIP_ERR_INVALID, "ddc design: decim outside [1, 64] or n_taps outside [1, 1024]");
  if (!(cutoff > 0.0 && cutoff <= 1.0)) return fail(BLAH2HIP_ERR_INVALID, "ddc design: cutoff outside (0, 1]");
  if (!std::isfinite(beta) || beta < 0.0) return fail(BLAH2HIP_ERR_INVALID, "ddc design: beta negative or not finite");
  const uint32_t T = n_taps;
  const double nu = cutoff / (2.0 * decim);
  // the first half, mirrored: h[t] == h[T - 1 - t] bit for bit
  for (uint32_t t = 0; t < (T + 1) / 2; t++) {
    const double k = 2.0 * t - (double)(T - 1); // 2 (t - (T - 1) / 2), an integer
    const double a = M_PI * nu * k;             // pi 2 nu (t - (T - 1) / 2)
    const double sinc = a == 0.0 ? 1.0 : std::sin(a) / a;
    const double rel = T > 1 ? k / (double)(T - 1) : 0.0;
    const double v = sinc * bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - rel * rel)));
    h[t] = v;
    h[T - 1 - t] = v;
  }
  long double s = 0.0L;
  for (uint32_t t = 0; t < T; t++) s += h[t];
  const double sd = (double)s;
  if (!(std::fabs(sd) > 0.0) || !std::isfinite(sd)) return fail(BLAH2HIP_ERR_INVALID, "ddc design: the taps sum to zero");
  for (uint32_t t = 0; t < T; t++) h[t] /= sd;
  return BLAH2HIP_OK;
}

int blah2hip_ddc_create(double fs, uint32_t decim, const double *h, uint32_t n_taps, const double *offset_hz, uint32_t n_carriers,
                        uint32_t max_in, uint32_t max_rows, int device, blah2hip_ddc_t *out)
{
  if (!out) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (!h || !offset_hz) return fail(BLAH2HIP_ERR_INVALID, "ddc: NULL taps or offsets");
  if (!std::isfinite(fs) || !(fs > 0.0)) return fail(BLAH2HIP_ERR_INVALID, "ddc: fs must be finite and positive");
  if (!sizes_ok(decim, n_taps)) return fail(BLAH2HIP_ERR_INVALID, "ddc: decim outside [1, 64] or n_taps outside [1, 1024]");
  if (n_carriers == 0 || n_carriers > BLAH2HIP_MAX_DDC_CARRIERS) return fail(BLAH2HIP_ERR_INVALID, "ddc: n_carriers outside [1, 8]");
  for (uint32_t t = 0; t < n_taps; t++)
    if (!std::isfinite(h[t])) return fail(BLAH2HIP_ERR_INVALID, "ddc: a tap is not finite");
  for (uint32_t c = 0; c < n_carriers; c++)
    if (!std::isfinite(offset_hz[c]) || std::fabs(offset_hz[c]) > 0.5 * fs) return fail(BLAH2HIP_ERR_INVALID, "ddc: an offset is not finite or beyond fs / 2");
  if (max_in == 0 || max_in > (1u << 30) || max_in % decim) return fail(BLAH2HIP_ERR_INVALID, "ddc: max_in zero, above 2^30 or no multiple of decim");
  if (max_rows == 0 || max_rows > 65535) return fail(BLAH2HIP_ERR_INVALID, "ddc: max_rows outside [1, 65535]");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(BLAH2HIP_ERR_NO_DEVICE, "no HIP device visible (the HIP path is the only path)");
  if (device < 0 || device >= ndev) return fail(BLAH2HIP_ERR_INVALID, "device index out of range");
  HIPCHK(hipSetDevice(device));

  blah2hip_ddc_s *d = new blah2hip_ddc_s;
  d->device = device;
  d->fs = fs; d->D = decim; d->T = n_taps; d->C = n_carriers;
  d->CB = n_carriers == 1 ? 1 : n_carriers == 2 ? 2 : 4;
  d->Cpad = (n_carriers + d->CB - 1) / d->CB * d->CB;
  d->maxIn = max_in; d->maxRows = max_rows;
  d->plan = ddc_plan(decim, n_taps);
  const uint32_t T = n_taps;
  std::vector<float> rev((size_t)d->Cpad * T * 2, 0.f);
  std::vector<double> r(d->Cpad, 0.0);
  for (uint32_t c = 0; c < n_carriers; c++) {
    const double a = offset_hz[c] / fs;
    r[c] = offset_hz[c] * (double)decim / fs;
    for (uint32_t t = 0; t < T; t++) {
      // frac(a t) from the product and its exact residual, then one rounding to fp32
      const double dt = (double)t, p = a * dt, e = std::fma(a, dt, -p);
      const double ang = 2.0 * M_PI * ((p - std::rint(p)) + e);
      const float re = (float)(h[t] * std::cos(ang)), im = (float)(h[t] * std::sin(ang));
      rev[((size_t)c * T + (T - 1 - t)) * 2] = re;
      rev[((size_t)c * T + (T - 1 - t)) * 2 + 1] = im;
    }
  }
  const size_t histBytes = std::max<size_t>(16, (size_t)2 * (T - 1) * sizeof(cf));
  hipError_t e = hipMalloc(&d->d_taps, rev.size() * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&d->d_r, r.size() * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&d->d_hist, histBytes);
  if (e == hipSuccess) e = hipMalloc(&d->d_pos, sizeof(uint64_t));
  if (e == hipSuccess) e = hipMemcpy(d->d_taps, rev.data(), rev.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d->d_r, r.data(), r.size() * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d->d_hist, 0, histBytes);
  if (e == hipSuccess) e = hipMemset(d->d_pos, 0, sizeof(uint64_t));
  // the largest image any handle asks for (the attribute is set once per device and kernel), set here so that the dev
  // call only enqueues
  const int ldsMax = DDC_LDS_SAMPLES * 16;
  if (e == hipSuccess) e = ensure_r<1>(ldsMax);
  if (e == hipSuccess) e = ensure_r<2>(ldsMax);
  if (e == hipSuccess) e = ensure_r<4>(ldsMax);
  if (e != hipSuccess) {
    (void)blah2hip_ddc_destroy(d);
    return fail(BLAH2HIP_ERR_HIP, std::string("ddc create: ") + hipGetErrorString(e));
  }
  *out = d;
  return BLAH2HIP_OK;
}

int blah2hip_ddc_destroy(blah2hip_ddc_t d)
{
  if (!d) return BLAH2HIP_OK;
  (void)hipSetDevice(d->device);
  (void)hipDeviceSynchronize(); // enqueued calls may still use the buffers and record the timer's events
  int rc = BLAH2HIP_OK;
  void *bufs[] = {d->d_taps, d->d_r, d->d_hist, d->d_pos};
  for (void *p : bufs)
    if (p && hipFree(p) != hipSuccess) rc = fail(BLAH2HIP_ERR_HIP, "hipFree(ddc)");
  d->timer.destroy();
  delete d;
  return rc;
}

int blah2hip_ddc_reset(blah2hip_ddc_t d, uint64_t first_sample, void *stream)
{
  if (!d) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (first_sample % d->D) return fail(BLAH2HIP_ERR_INVALID, "ddc reset: first_sample is no multiple of decim");
  HIPCHK(hipSetDevice(d->device));
  hipLaunchKernelGGL(ddc_reset_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, d->d_hist, 2 * (d->T - 1), d->d_pos, first_sample / d->D);
  HIPCHK(hipGetLastError());
  d->nextSample = first_sample;
  return BLAH2HIP_OK;
}

int blah2hip_ddc_process_dev(blah2hip_ddc_t d, int fmt, const void *d_x, const void *d_y, uint32_t n_in, uint32_t n_rows, uint64_t in_stride,
                             void *d_out_x, void *d_out_y, uint64_t out_stride, uint64_t carrier_stride, void *stream)
{
  if (!d) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (fmt != BLAH2HIP_FMT_C32 && fmt != BLAH2HIP_FMT_I16 && fmt != BLAH2HIP_FMT_I8)
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "ddc: the input is FMT_C32 planes, FMT_I16 words or FMT_I8 planes");
  const bool twoPlanes = fmt != BLAH2HIP_FMT_I16;
  if (!d_x || (twoPlanes && !d_y) || !d_out_x || !d_out_y) return fail(BLAH2HIP_ERR_INVALID, "ddc: NULL pointer");
  if (n_in == 0 || n_in > d->maxIn || n_in % d->D) return fail(BLAH2HIP_ERR_INVALID, "ddc: n_in zero, above max_in or no multiple of decim");
  if (n_rows == 0 || n_rows > d->maxRows) return fail(BLAH2HIP_ERR_INVALID, "ddc: n_rows outside [1, max_rows]");
  const uint32_t n_out = n_in / d->D;
  if (n_rows > 1 && (in_stride < n_in || out_stride < n_out)) return fail(BLAH2HIP_ERR_INVALID, "ddc: a stride overlaps rows");
  const uint64_t carrierSpan = (uint64_t)(n_rows - 1) * out_stride + n_out;
  if (d->C > 1 && carrier_stride < carrierSpan) return fail(BLAH2HIP_ERR_INVALID, "ddc: carrier_stride overlaps carriers");
  const size_t ib = in_bytes(fmt);
  if ((uintptr_t)d_x % ib || (twoPlanes && (uintptr_t)d_y % ib) || (uintptr_t)d_out_x % 8 || (uintptr_t)d_out_y % 8)
    return fail(BLAH2HIP_ERR_INVALID, "ddc: a buffer is off its alignment");
  const size_t inSpan = (size_t)((uint64_t)(n_rows - 1) * in_stride + n_in) * ib;
  const size_t outSpan = (size_t)((uint64_t)(d->C - 1) * carrier_stride + carrierSpan) * sizeof(cf);
  if (ranges_overlap(d_out_x, outSpan, d_out_y, outSpan)) return fail(BLAH2HIP_ERR_INVALID, "ddc: the outputs overlap each other");
  const void *outs[] = {d_out_x, d_out_y};
  for (const void *o : outs)
    if (ranges_overlap(o, outSpan, d_x, inSpan) || (twoPlanes && ranges_overlap(o, outSpan, d_y, inSpan)))
      return fail(BLAH2HIP_ERR_INVALID, "ddc: an output overlaps an input");
  HIPCHK(hipSetDevice(d->device));
  hipStream_t st = (hipStream_t)stream;

  DdcArgs a{};
  a.x = d_x; a.y = d_y; a.inStride = in_stride; a.nIn = n_in; a.nOut = n_out; a.fmt = fmt;
  a.hist = d->d_hist; a.taps = d->d_taps; a.r = d->d_r; a.pos = d->d_pos;
  a.outX = (cf *)d_out_x; a.outY = (cf *)d_out_y; a.outStride = out_stride; a.carrierStride = carrier_stride;
  a.D = d->D; a.T = d->T; a.C = d->C; a.tile = d->plan.tile; a.Lp = d->plan.Lp; a.TR = d->plan.TR;
  const dim3 grid((n_out + d->plan.tile - 1) / d->plan.tile, n_rows), block(d->plan.threads);
  const size_t lds = ddc_lds_bytes(d->D, d->plan);
  HIPCHK(d->timer.tic(BLAH2HIP_DK_DDC, st));
  if (d->plan.R == 1) launch_r<1>(d->CB, grid, block, lds, st, a);
  else if (d->plan.R == 2) launch_r<2>(d->CB, grid, block, lds, st, a);
  else launch_r<4>(d->CB, grid, block, lds, st, a);
  HIPCHK(hipGetLastError());
  HIPCHK(d->timer.toc(BLAH2HIP_DK_DDC, st));
  // behind it on the same stream: the main kernel's workgroups have all read the history by then
  DdcTailArgs t{};
  t.x = d_x; t.y = d_y; t.inStride = in_stride; t.nIn = n_in; t.nRows = n_rows; t.nOut = n_out; t.fmt = fmt;
  t.hist = d->d_hist; t.pos = d->d_pos; t.T = d->T;
  HIPCHK(d->timer.tic(BLAH2HIP_DK_TAIL, st));
  hipLaunchKernelGGL(ddc_tail_kernel, dim3(1), dim3(256), 0, st, t);
  HIPCHK(hipGetLastError());
  HIPCHK(d->timer.toc(BLAH2HIP_DK_TAIL, st));
  d->nextSample += (uint64_t)n_rows * n_in;
  return BLAH2HIP_OK;
}

int blah2hip_ddc_read_taps(blah2hip_ddc_t d, uint32_t carrier, float *g)
{
  if (!d || !g) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (carrier >= d->C) return fail(BLAH2HIP_ERR_INVALID, "ddc: carrier outside the handle's");
  // from the device: what the kernel multiplies with
  std::vector<float> rev((size_t)d->T * 2);
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(hipMemcpy(rev.data(), d->d_taps + (size_t)carrier * d->T, rev.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (uint32_t t = 0; t < d->T; t++) {
    g[2 * t] = rev[2 * (size_t)(d->T - 1 - t)];
    g[2 * t + 1] = rev[2 * (size_t)(d->T - 1 - t) + 1];
  }
  return BLAH2HIP_OK;
}

int blah2hip_ddc_get_info(blah2hip_ddc_t d, int what, int64_t *value)
{
  if (!d || !value) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (what == BLAH2HIP_DDC_INFO_TILE) *value = d->plan.tile;
  else if (what == BLAH2HIP_DDC_INFO_NEXT_SAMPLE) *value = (int64_t)d->nextSample;
  else return fail(BLAH2HIP_ERR_INVALID, "ddc: unknown info");
  return BLAH2HIP_OK;
}

int blah2hip_ddc_set_timing(blah2hip_ddc_t d, int enable)
{
  if (!d) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  d->timer.enabled = enable != 0;
  return BLAH2HIP_OK;
}

int blah2hip_ddc_get_timing(blah2hip_ddc_t d, double *ms_total, uint32_t *launches)
{
  if (!d || !ms_total || !launches) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(d->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(d->timer.collect(ms_total, launches));
  return BLAH2HIP_OK;
}

} // extern "C"
