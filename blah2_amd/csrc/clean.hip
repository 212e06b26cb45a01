// Strong-echo cancellation behind include/blah2hip.h: least-squares CLEAN on the samples.  Host code of the
// blah2hip_clean_* entry points; the kernels are clean_kernels.hpp's.  Everything is allocated by create: the dev entry
// points only enqueue.
#include "amb_handle.hpp"
#include "clean_kernels.hpp"

#include <cmath>

using namespace blah2;

struct blah2hip_clean_s {
  int device = 0;
  uint32_t n = 0, maxBatch = 0;
  double fs = 0.0;
  int32_t dlo = 0, dhi = 0;
  int numCU = 256;
  uint32_t partCap = 0;       // partials in d_part, over all CPIs of a call
  double *d_part = nullptr;   // [partCap][CLN_PART]
  double *d_G = nullptr;      // [maxBatch][cap][cap] (re, im) of the last fit, cap = its cap_atoms
  double *d_b = nullptr;      // [maxBatch][cap] (re, im)
  double *d_amp = nullptr;    // [maxBatch][cap] (re, im): the last fit's amplitudes, beside the caller's copy
  int32_t *d_ok = nullptr;    // [maxBatch]
  uint32_t lastCap = 0, lastCpis = 0; // 0: no fit yet
  int gridForce = 0;          // BLAH2HIP_CLEAN_OPT_GRAM_GRID
  int gramGridLast = 0, subGridLast = 0;
  KernelTimer<BLAH2HIP_CLK_COUNT> timer;
};

namespace {

bool clean_fmt_ok(int fmt) { return fmt == BLAH2HIP_FMT_C32 || fmt == BLAH2HIP_FMT_I16X_C32Y || fmt == BLAH2HIP_FMT_I8X_C32Y; }
size_t x_bytes(int fmt) { return fmt == BLAH2HIP_FMT_C32 ? 8 : fmt == BLAH2HIP_FMT_I16X_C32Y ? 8 : 2; }
size_t x_align(int fmt) { return fmt == BLAH2HIP_FMT_C32 ? 8 : fmt == BLAH2HIP_FMT_I16X_C32Y ? 4 : 2; }

// what fit and subtract share: the arguments that describe the planes and the atoms.  0, or the code with the message set.
int check_planes(const blah2hip_clean_s *h, int fmt, const void *d_x, const void *d_y, uint32_t n_cpi, uint64_t cpi_stride,
                 const blah2hip_atom_t *d_atoms, uint32_t cap_atoms, const uint32_t *d_atom_count)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (!d_x || !d_y || !d_atoms || !d_atom_count) return fail(BLAH2HIP_ERR_INVALID, "clean: NULL pointer");
  if (n_cpi == 0 || n_cpi > h->maxBatch) return fail(BLAH2HIP_ERR_INVALID, "clean: n_cpi outside [1, max_batch]");
  if (cap_atoms == 0 || cap_atoms > BLAH2HIP_MAX_ATOMS) return fail(BLAH2HIP_ERR_INVALID, "clean: cap_atoms outside [1, BLAH2HIP_MAX_ATOMS]");
  if (!clean_fmt_ok(fmt)) return fail(BLAH2HIP_ERR_UNSUPPORTED, "clean: the surveillance channel must be an fp32 plane (FMT_C32, FMT_I16X_C32Y, FMT_I8X_C32Y)");
  if (n_cpi > 1 && cpi_stride < h->n) return fail(BLAH2HIP_ERR_INVALID, "clean: cpi_stride < n_samples");
  if ((uintptr_t)d_x % x_align(fmt) || (uintptr_t)d_y % 8) return fail(BLAH2HIP_ERR_INVALID, "clean: a sample plane is off its alignment");
  if ((uintptr_t)d_atoms % 8 || (uintptr_t)d_atom_count % 4) return fail(BLAH2HIP_ERR_INVALID, "clean: the atom list is off its alignment");
  return BLAH2HIP_OK;
}

struct Span { const void *p; size_t bytes; };

bool any_overlap(const Span *outs, int nOut, const Span *ins, int nIn)
{
  for (int i = 0; i < nOut; i++) {
    for (int j = 0; j < nIn; j++)
      if (ranges_overlap(outs[i].p, outs[i].bytes, ins[j].p, ins[j].bytes)) return true;
    for (int j = i + 1; j < nOut; j++)
      if (ranges_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes)) return true;
  }
  return false;
}

size_t plane_bytes(uint32_t n, uint32_t n_cpi, uint64_t stride, size_t each) { return ((size_t)(n_cpi - 1) * stride + n) * each; }

CleanIn make_in(const blah2hip_clean_s *h, int fmt, const void *d_x, const void *d_y, uint64_t cpi_stride, const blah2hip_atom_t *d_atoms,
                uint32_t cap_atoms, const uint32_t *d_atom_count)
{
  CleanIn in;
  in.x = d_x;
  in.y = (const cf *)d_y;
  in.cpiStride = cpi_stride;
  in.n = h->n;
  in.fmt = fmt;
  in.dlo = h->dlo;
  in.dhi = h->dhi;
  in.invFs = 1.0 / h->fs;
  in.atoms = d_atoms;
  in.count = d_atom_count;
  in.capAtoms = cap_atoms;
  return in;
}

} // namespace

extern "C" {

int blah2hip_clean_create(uint32_t n_samples, double fs, int32_t delay_lo, int32_t delay_hi, int device, uint32_t max_batch,
                          blah2hip_clean_t *out)
{
  if (!out) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (n_samples == 0 || n_samples > (1u << 26)) return fail(BLAH2HIP_ERR_INVALID, "clean: n_samples outside [1, 2^26]");
  if (!std::isfinite(fs) || !(fs > 0.0)) return fail(BLAH2HIP_ERR_INVALID, "clean: fs must be finite and positive");
  if (delay_hi < delay_lo) return fail(BLAH2HIP_ERR_INVALID, "clean: delay_hi < delay_lo");
  if (delay_lo <= -(1 << 26) || delay_hi >= (1 << 26)) return fail(BLAH2HIP_ERR_INVALID, "clean: a delay limit beyond 2^26 samples");
  if ((int64_t)delay_hi - delay_lo > CLN_MAX_SPAN)
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "clean: delay_hi - delay_lo above 4095 (the reference window plus halo is kept in LDS)");
  if (max_batch == 0) max_batch = 1;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(BLAH2HIP_ERR_NO_DEVICE, "no HIP device visible (the HIP path is the only path)");
  if (device < 0 || device >= ndev) return fail(BLAH2HIP_ERR_INVALID, "device index out of range");
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  blah2hip_clean_s *h = new blah2hip_clean_s;
  h->device = device;
  h->n = n_samples; h->fs = fs; h->dlo = delay_lo; h->dhi = delay_hi; h->maxBatch = max_batch;
  h->numCU = prop.multiProcessorCount;
  h->partCap = std::max<uint32_t>(max_batch, 8u * (uint32_t)h->numCU);
  const size_t A = BLAH2HIP_MAX_ATOMS;
  hipError_t e = hipMalloc(&h->d_part, (size_t)h->partCap * CLN_PART * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&h->d_G, (size_t)max_batch * A * A * 2 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&h->d_b, (size_t)max_batch * A * 2 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&h->d_amp, (size_t)max_batch * A * 2 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&h->d_ok, (size_t)max_batch * sizeof(int32_t));
  // the largest dynamic LDS either kernel can ask for on any handle (the attribute is set once per device and kernel),
  // set here so that the dev calls only enqueue
  const size_t ldsMax = clean_lds_window(CLN_MAX_SPAN) + clean_lds_tab(A) + clean_lds_base() + clean_lds_tile(A);
  if (e == hipSuccess) e = blah2hip_ensure_lds_((const void *)clean_gram_kernel, (int)ldsMax);
  if (e == hipSuccess) e = blah2hip_ensure_lds_((const void *)clean_subtract_kernel, (int)ldsMax);
  if (e != hipSuccess) {
    (void)blah2hip_clean_destroy(h);
    return fail(BLAH2HIP_ERR_HIP, std::string("clean create: ") + hipGetErrorString(e));
  }
  *out = h;
  return BLAH2HIP_OK;
}

int blah2hip_clean_destroy(blah2hip_clean_t h)
{
  if (!h) return BLAH2HIP_OK;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize(); // enqueued calls may still use the buffers and record the timer's events
  int rc = BLAH2HIP_OK;
  void *bufs[] = {h->d_part, h->d_G, h->d_b, h->d_amp, h->d_ok};
  for (void *p : bufs)
    if (p && hipFree(p) != hipSuccess) rc = fail(BLAH2HIP_ERR_HIP, "hipFree(clean)");
  h->timer.destroy();
  delete h;
  return rc;
}

int blah2hip_clean_set_option(blah2hip_clean_t h, int option, int64_t value)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (option != BLAH2HIP_CLEAN_OPT_GRAM_GRID) return fail(BLAH2HIP_ERR_INVALID, "clean: unknown option");
  if (value < 0 || value > (1 << 20)) return fail(BLAH2HIP_ERR_INVALID, "clean: grid outside [0, 2^20]");
  h->gridForce = (int)value;
  return BLAH2HIP_OK;
}

int blah2hip_clean_get_info(blah2hip_clean_t h, int what, int64_t *value)
{
  if (!h || !value) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (what == BLAH2HIP_CLEAN_INFO_GRAM_GRID) *value = h->gramGridLast;
  else if (what == BLAH2HIP_CLEAN_INFO_SUBTRACT_GRID) *value = h->subGridLast;
  else return fail(BLAH2HIP_ERR_INVALID, "clean: unknown info");
  return BLAH2HIP_OK;
}

int blah2hip_clean_atoms_dev(blah2hip_clean_t h, blah2hip_amb_t amb, const blah2hip_det_t *d_dets, uint32_t cap, const uint32_t *d_count,
                             uint32_t n_cpi, double snr_min_db, uint32_t max_echoes, int32_t side_delay, int32_t side_doppler,
                             blah2hip_atom_t *d_atoms, uint32_t cap_atoms, uint32_t *d_atom_count, int32_t *d_used, void *stream)
{
  if (!h || !amb) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (!d_dets || !d_count || !d_atoms || !d_atom_count || !d_used) return fail(BLAH2HIP_ERR_INVALID, "clean atoms: NULL pointer");
  if (n_cpi == 0 || n_cpi > h->maxBatch) return fail(BLAH2HIP_ERR_INVALID, "clean atoms: n_cpi outside [1, max_batch]");
  if (cap == 0) return fail(BLAH2HIP_ERR_INVALID, "clean atoms: cap is 0");
  if (cap_atoms == 0 || cap_atoms > BLAH2HIP_MAX_ATOMS) return fail(BLAH2HIP_ERR_INVALID, "clean atoms: cap_atoms outside [1, BLAH2HIP_MAX_ATOMS]");
  if (max_echoes > BLAH2HIP_MAX_ATOMS) return fail(BLAH2HIP_ERR_INVALID, "clean atoms: max_echoes above BLAH2HIP_MAX_ATOMS");
  if (side_delay < 0 || side_delay > 2 || side_doppler < 0 || side_doppler > 1)
    return fail(BLAH2HIP_ERR_INVALID, "clean atoms: side_delay outside [0, 2] or side_doppler outside [0, 1]");
  if (std::isnan(snr_min_db)) return fail(BLAH2HIP_ERR_INVALID, "clean atoms: snr_min_db is not a number");
  if ((uintptr_t)d_dets % 8 || (uintptr_t)d_atoms % 8 || (uintptr_t)d_count % 4 || (uintptr_t)d_atom_count % 4 || (uintptr_t)d_used % 4)
    return fail(BLAH2HIP_ERR_INVALID, "clean atoms: a buffer is off its alignment");
  const Span outs[] = {{d_atoms, (size_t)n_cpi * cap_atoms * sizeof(blah2hip_atom_t)}, {d_atom_count, (size_t)n_cpi * 4},
                       {d_used, (size_t)n_cpi * cap_atoms * 4}};
  const Span ins[] = {{d_dets, (size_t)n_cpi * cap * sizeof(blah2hip_det_t)}, {d_count, (size_t)n_cpi * 4}};
  if (any_overlap(outs, 3, ins, 2)) return fail(BLAH2HIP_ERR_INVALID, "clean atoms: an output overlaps an input or another output");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  CleanAtomsArgs a;
  a.dets = d_dets; a.count = d_count; a.atoms = d_atoms; a.atomCount = d_atom_count; a.used = d_used;
  a.cap = cap; a.capAtoms = cap_atoms; a.maxEchoes = max_echoes;
  a.sideDelay = side_delay; a.sideDoppler = side_doppler; a.dlo = h->dlo; a.dhi = h->dhi;
  a.snrMin = snr_min_db;
  a.halfBin = 0.5 / amb->dims.cpi;
  HIPCHK(h->timer.tic(BLAH2HIP_CLK_ATOMS, st));
  hipLaunchKernelGGL(clean_atoms_kernel, dim3(n_cpi), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  HIPCHK(h->timer.toc(BLAH2HIP_CLK_ATOMS, st));
  return BLAH2HIP_OK;
}

int blah2hip_clean_fit_dev(blah2hip_clean_t h, int fmt, const void *d_x, const void *d_y, uint32_t n_cpi, uint64_t cpi_stride,
                           const blah2hip_atom_t *d_atoms, uint32_t cap_atoms, const uint32_t *d_atom_count, double loading,
                           double *d_amp, int32_t *d_ok, void *stream)
{
  int rc;
  if ((rc = check_planes(h, fmt, d_x, d_y, n_cpi, cpi_stride, d_atoms, cap_atoms, d_atom_count))) return rc;
  if (!d_amp || !d_ok) return fail(BLAH2HIP_ERR_INVALID, "clean fit: NULL output");
  if ((uintptr_t)d_amp % 8 || (uintptr_t)d_ok % 4) return fail(BLAH2HIP_ERR_INVALID, "clean fit: an output is off its alignment");
  if (!std::isfinite(loading) || loading < 0.0) return fail(BLAH2HIP_ERR_INVALID, "clean fit: loading must be finite and not negative");
  const Span outs[] = {{d_amp, (size_t)n_cpi * cap_atoms * 16}, {d_ok, (size_t)n_cpi * 4}};
  const Span ins[] = {{d_x, plane_bytes(h->n, n_cpi, cpi_stride, x_bytes(fmt))}, {d_y, plane_bytes(h->n, n_cpi, cpi_stride, 8)},
                      {d_atoms, (size_t)n_cpi * cap_atoms * sizeof(blah2hip_atom_t)}, {d_atom_count, (size_t)n_cpi * 4}};
  if (any_overlap(outs, 2, ins, 4)) return fail(BLAH2HIP_ERR_INVALID, "clean fit: an output overlaps an input or another output");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;

  // Workgroups per CPI of the partials kernel: eight a CU over the call (as many as are resident with few atoms: the kernel
  // is a stream of loads then), one per chunk at the most, and no more than the handle has partials for; the option
  // overrides the first of the three.
  const uint32_t nChunks = (h->n + CLN_CH - 1) / CLN_CH;
  uint32_t G = h->gridForce ? (uint32_t)h->gridForce : (8u * (uint32_t)h->numCU + n_cpi - 1) / n_cpi;
  G = std::max<uint32_t>(1, std::min({G, nChunks, h->partCap / n_cpi}));
  CleanGramArgs ga;
  ga.in = make_in(h, fmt, d_x, d_y, cpi_stride, d_atoms, cap_atoms, d_atom_count);
  ga.part = h->d_part;
  const size_t lds = clean_lds_window(h->dhi - h->dlo) + clean_lds_tab(cap_atoms) + clean_lds_base() + clean_lds_tile(cap_atoms);
  HIPCHK(h->timer.tic(BLAH2HIP_CLK_GRAM, st));
  hipLaunchKernelGGL(clean_gram_kernel, dim3(G, n_cpi), dim3(256), lds, st, ga);
  HIPCHK(hipGetLastError());
  HIPCHK(h->timer.toc(BLAH2HIP_CLK_GRAM, st));
  HIPCHK(h->timer.tic(BLAH2HIP_CLK_FOLD, st));
  hipLaunchKernelGGL(clean_fold_kernel, dim3((cap_atoms * (cap_atoms + 1) + 3) / 4, n_cpi), dim3(256), 0, st, (const double *)h->d_part, G, d_atom_count, cap_atoms, h->d_G, h->d_b);
  HIPCHK(hipGetLastError());
  HIPCHK(h->timer.toc(BLAH2HIP_CLK_FOLD, st));
  HIPCHK(h->timer.tic(BLAH2HIP_CLK_SOLVE, st));
  hipLaunchKernelGGL(clean_solve_kernel, dim3(n_cpi), dim3(64), 0, st, (const double *)h->d_G, (const double *)h->d_b, d_atoms, d_atom_count,
                     cap_atoms, h->dlo, h->dhi, loading, d_amp, d_ok, h->d_amp, h->d_ok);
  HIPCHK(hipGetLastError());
  HIPCHK(h->timer.toc(BLAH2HIP_CLK_SOLVE, st));
  h->gramGridLast = (int)G;
  h->lastCap = cap_atoms;
  h->lastCpis = n_cpi;
  return BLAH2HIP_OK;
}

int blah2hip_clean_subtract_dev(blah2hip_clean_t h, int fmt, const void *d_x, const void *d_y, uint32_t n_cpi, uint64_t cpi_stride,
                                const blah2hip_atom_t *d_atoms, uint32_t cap_atoms, const uint32_t *d_atom_count, const double *d_amp,
                                const int32_t *d_ok, void *d_y_out, uint64_t out_stride, void *stream)
{
  int rc;
  if ((rc = check_planes(h, fmt, d_x, d_y, n_cpi, cpi_stride, d_atoms, cap_atoms, d_atom_count))) return rc;
  if (!d_amp || !d_ok || !d_y_out) return fail(BLAH2HIP_ERR_INVALID, "clean subtract: NULL pointer");
  if ((uintptr_t)d_amp % 8 || (uintptr_t)d_ok % 4 || (uintptr_t)d_y_out % 8) return fail(BLAH2HIP_ERR_INVALID, "clean subtract: a buffer is off its alignment");
  if (n_cpi > 1 && out_stride < h->n) return fail(BLAH2HIP_ERR_INVALID, "clean subtract: out_stride < n_samples");
  const bool inPlace = d_y_out == d_y && (n_cpi == 1 || out_stride == cpi_stride);
  const Span out = {d_y_out, plane_bytes(h->n, n_cpi, out_stride, 8)};
  const Span ins[] = {{d_x, plane_bytes(h->n, n_cpi, cpi_stride, x_bytes(fmt))}, {d_atoms, (size_t)n_cpi * cap_atoms * sizeof(blah2hip_atom_t)},
                      {d_atom_count, (size_t)n_cpi * 4}, {d_amp, (size_t)n_cpi * cap_atoms * 16}, {d_ok, (size_t)n_cpi * 4},
                      {d_y, plane_bytes(h->n, n_cpi, cpi_stride, 8)}};
  if (any_overlap(&out, 1, ins, inPlace ? 5 : 6))
    return fail(BLAH2HIP_ERR_INVALID, "clean subtract: the output overlaps an input (only d_y_out == d_y with equal strides may alias)");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const uint32_t nChunks = (h->n + CLN_CH - 1) / CLN_CH;
  const uint32_t G = std::max<uint32_t>(1, std::min<uint32_t>(nChunks, (4u * (uint32_t)h->numCU + n_cpi - 1) / n_cpi));
  CleanSubArgs sa;
  sa.in = make_in(h, fmt, d_x, d_y, cpi_stride, d_atoms, cap_atoms, d_atom_count);
  sa.amp = d_amp;
  sa.ok = d_ok;
  sa.out = (cf *)d_y_out;
  sa.outStride = out_stride;
  const size_t lds = clean_lds_window(h->dhi - h->dlo) + clean_lds_tab(cap_atoms) + clean_lds_base();
  HIPCHK(h->timer.tic(BLAH2HIP_CLK_SUBTRACT, st));
  hipLaunchKernelGGL(clean_subtract_kernel, dim3(G, n_cpi), dim3(256), lds, st, sa);
  HIPCHK(hipGetLastError());
  HIPCHK(h->timer.toc(BLAH2HIP_CLK_SUBTRACT, st));
  h->subGridLast = (int)G;
  return BLAH2HIP_OK;
}

int blah2hip_clean_process_dev(blah2hip_clean_t h, int fmt, const void *d_x, const void *d_y, uint32_t n_cpi, uint64_t cpi_stride,
                               const blah2hip_atom_t *d_atoms, uint32_t cap_atoms, const uint32_t *d_atom_count, double loading,
                               double *d_amp, int32_t *d_ok, void *d_y_out, uint64_t out_stride, void *stream)
{
  // the subtraction's own refusals first, so that a refused call has enqueued nothing
  int rc;
  if ((rc = check_planes(h, fmt, d_x, d_y, n_cpi, cpi_stride, d_atoms, cap_atoms, d_atom_count))) return rc;
  if (!d_amp || !d_ok || !d_y_out) return fail(BLAH2HIP_ERR_INVALID, "clean: NULL pointer");
  if ((uintptr_t)d_y_out % 8) return fail(BLAH2HIP_ERR_INVALID, "clean: the output plane is off its alignment");
  if (n_cpi > 1 && out_stride < h->n) return fail(BLAH2HIP_ERR_INVALID, "clean: out_stride < n_samples");
  const bool inPlace = d_y_out == d_y && (n_cpi == 1 || out_stride == cpi_stride);
  const Span out = {d_y_out, plane_bytes(h->n, n_cpi, out_stride, 8)};
  const Span ins[] = {{d_x, plane_bytes(h->n, n_cpi, cpi_stride, x_bytes(fmt))}, {d_atoms, (size_t)n_cpi * cap_atoms * sizeof(blah2hip_atom_t)},
                      {d_atom_count, (size_t)n_cpi * 4}, {d_amp, (size_t)n_cpi * cap_atoms * 16}, {d_ok, (size_t)n_cpi * 4},
                      {d_y, plane_bytes(h->n, n_cpi, cpi_stride, 8)}};
  if (any_overlap(&out, 1, ins, inPlace ? 5 : 6))
    return fail(BLAH2HIP_ERR_INVALID, "clean: the output overlaps an input (only d_y_out == d_y with equal strides may alias)");
  if ((rc = blah2hip_clean_fit_dev(h, fmt, d_x, d_y, n_cpi, cpi_stride, d_atoms, cap_atoms, d_atom_count, loading, d_amp, d_ok, stream))) return rc;
  return blah2hip_clean_subtract_dev(h, fmt, d_x, d_y, n_cpi, cpi_stride, d_atoms, cap_atoms, d_atom_count, d_amp, d_ok, d_y_out, out_stride, stream);
}

int blah2hip_clean_read_last(blah2hip_clean_t h, uint32_t cpi, double *G, double *b, double *amp, int32_t *ok)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (h->lastCpis == 0) return fail(BLAH2HIP_ERR_INVALID, "clean: no fit yet");
  if (cpi >= h->lastCpis) return fail(BLAH2HIP_ERR_INVALID, "clean: cpi outside the last fit's batch");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());
  const size_t cap = h->lastCap;
  if (G) HIPCHK(hipMemcpy(G, h->d_G + (size_t)cpi * cap * cap * 2, cap * cap * 16, hipMemcpyDeviceToHost));
  if (b) HIPCHK(hipMemcpy(b, h->d_b + (size_t)cpi * cap * 2, cap * 16, hipMemcpyDeviceToHost));
  if (amp) HIPCHK(hipMemcpy(amp, h->d_amp + (size_t)cpi * cap * 2, cap * 16, hipMemcpyDeviceToHost));
  if (ok) HIPCHK(hipMemcpy(ok, h->d_ok + cpi, 4, hipMemcpyDeviceToHost));
  return BLAH2HIP_OK;
}

int blah2hip_clean_set_timing(blah2hip_clean_t h, int enable)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  h->timer.enabled = enable != 0;
  return BLAH2HIP_OK;
}

int blah2hip_clean_get_timing(blah2hip_clean_t h, double *ms_total, uint32_t *launches)
{
  if (!h || !ms_total || !launches) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(h->timer.collect(ms_total, launches));
  return BLAH2HIP_OK;
}

} // extern "C"
