// Detection behind include/blah2hip.h: 1-D and 2-D CFAR (cell-averaging, ordered-statistic, greatest-of / smallest-of) with
// their threshold-table caches and summed-area table, the clutter map and its gate, Centroid and Interpolate on the host and
// on the device.  Host code; the kernels are cfar_kernels.hpp's, oscfar_kernels.hpp's, gocfar_kernels.hpp's,
// cmap_kernels.hpp's and detect_kernels.hpp's.
#include "amb_handle.hpp"
#include "cfar_kernels.hpp"
#include "cmap_kernels.hpp"
#include "detect_kernels.hpp"
#include "gocfar_kernels.hpp"
#include "oscfar_kernels.hpp"

#include <map>

#include "cfar_alpha.hpp"

using namespace blah2;

// The clutter map of ONE ambiguity handle (its geometry, buffers and timer): the memory, the age, the plane b and the
// threshold tables of the pfa values it has seen
struct blah2hip_cmap_s {
  blah2hip_amb_s *amb = nullptr;
  uint32_t memory = 0, flags = 0;
  uint64_t age = 0;      // CPIs absorbed since the creation or the last reset
  float *d_bg = nullptr; // [cells]: b
  TableCache<double> tables; // alpha[0 .. 16 T] per pfa
};

namespace {

// The detectors' threshold tables on the device.  Four lists -- cell averaging, ordered statistic, greatest-of / smallest-of
// on the ambiguity handle, the clutter map's on its own handle -- under the one policy of table_cache.hpp: a hit only hands
// out the pointer; a miss builds, allocates and uploads (blocking), which is refused while `st` is being captured into a
// graph -- *_prepare is the call for that, and what it hands out (`pin`) lives as long as the handle; eight unpinned tables
// a list, and a call never touches another list.  What differs is below: the key, when an entry serves a request, the
// builder and the two texts.
//
// Cell averaging (permille 0, h->alphaTables, `rank` unused): blah2hip_cfar_alpha's alpha[0 .. maxN], keyed by (pfa, looks,
// size); a larger table serves a smaller request.  Ordered statistic (h->osTables): blah2hip_oscfar_alpha's alpha[maxN + 1]
// doubles, then rank[maxN + 1] words, in one allocation, keyed by (pfa, looks, rank, size); the size must match, because
// the rank words sit behind alpha[maxN].  The looks are the handle's BLAH2HIP_OPT_CFAR_LOOKS at the time of the call.
int cfar_table(blah2hip_amb_s *h, double pfa, uint32_t permille, size_t maxN, const double **alpha, const uint32_t **rank,
               hipStream_t st = nullptr, bool pin = false)
{
  typedef blah2hip_amb_s::CfarKey Key;
  const bool os = permille != 0;
  const Key key{pfa, h->cfarLooks, permille, maxN};
  HipTableDevice dev;
  const int rc = (os ? h->osTables : h->alphaTables).get(
      dev, key,
      [&](const Key &e) { return e.pfa == pfa && e.looks == key.looks && e.rank == permille && (os ? e.n == maxN : e.n >= maxN); },
      [&](std::vector<double> &host) {
        host.resize(((maxN + 1) * (sizeof(double) + (os ? sizeof(uint32_t) : 0)) + sizeof(double) - 1) / sizeof(double));
        return os ? blah2hip_oscfar_alpha(pfa, key.looks, permille, (uint32_t)maxN, host.data(), reinterpret_cast<uint32_t *>(host.data() + (maxN + 1)))
                  : blah2hip_cfar_alpha(pfa, key.looks, (uint32_t)maxN, host.data());
      },
      os ? "ordered-statistic table of this (pfa, rank, window) is not resident: call "
           "blah2hip_oscfar1d_prepare / blah2hip_oscfar2d_prepare before capturing the stream"
         : "threshold table of this (pfa, window) is not resident: call blah2hip_cfar1d_prepare / "
           "blah2hip_cfar2d_prepare before capturing the stream",
      os ? "ordered-statistic table upload: " : "alpha table upload: ", st, pin, alpha);
  if (rc == BLAH2HIP_OK && os) *rank = reinterpret_cast<const uint32_t *>(*alpha + (maxN + 1));
  return rc;
}

// ---- the checks the entry points share, in the order each entry point makes them ----
int check_dev(const blah2hip_amb_s *h, const blah2hip_hit_t *d_hits, const uint32_t *d_count, uint32_t n_cpi)
{
  if (!h || !d_hits || !d_count) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (n_cpi == 0 || n_cpi > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "n_cpi outside [1, max_batch]");
  return BLAH2HIP_OK;
}

// CfarDetector1D's ctor parameters are int8_t (CfarDetector1D.h:46)
int check_1d(int32_t n_guard, int32_t n_train, int32_t min_delay)
{
  if (n_guard < 0 || n_guard > 127 || n_train < 0 || n_train > 127 || min_delay < -128 || min_delay > 127)
    return fail(BLAH2HIP_ERR_INVALID, "nGuard/nTrain/minDelay outside int8 range");
  return BLAH2HIP_OK;
}

// the four sizes of a 2-D window, and minDelay for the calls that have one: oscfar2d_dev looks at minDelay first
int check_2d(int32_t ngd, int32_t ntd, int32_t ngf, int32_t ntf, int32_t min_delay = 0, bool delay_first = false)
{
  const bool delayBad = min_delay < -128 || min_delay > 127;
  if (delay_first && delayBad) return fail(BLAH2HIP_ERR_INVALID, "minDelay outside int8 range");
  for (int32_t v : {ngd, ntd, ngf, ntf})
    if (v < 0 || v > 127) return fail(BLAH2HIP_ERR_INVALID, "guard/train sizes outside [0, 127]");
  if (delayBad) return fail(BLAH2HIP_ERR_INVALID, "minDelay outside int8 range");
  return BLAH2HIP_OK;
}

// training cells of a full 2-D window, plus the cell under test: the size of its table
size_t window_cells(int32_t ngd, int32_t ntd, int32_t ngf, int32_t ntf)
{
  return (size_t)(2 * (ngd + ntd) + 1) * (2 * (ngf + ntf) + 1);
}

int os_check_rank(uint32_t permille)
{
  if (permille < 1 || permille > 1000) return fail(BLAH2HIP_ERR_INVALID, "rank_permille outside [1, 1000]");
  return BLAH2HIP_OK;
}

// the one-pass tile kernel covers windows whose halo fits its LDS budget; larger ones take the summed-area table
bool cfar2d_use_tile(const blah2hip_amb_s *h, int ngd, int ntd, int ngf, int ntf)
{
  if (h->cfar2dForce == BLAH2HIP_CFAR2D_SAT) return false;
  return ngf + ntf <= C2T_MAX_HR && ngd + ntd <= C2T_MAX_HC;
}

// the stream kernel exists for the window shapes of C2S_SHAPES (cfar_kernels.hpp)
bool cfar2d_stream_shape(int ngd, int ntd, int ngf, int ntf)
{
#define B2_X(TD, GD, TF, GF) if (ntd == TD && ngd == GD && ntf == TF && ngf == GF) return true;
  C2S_SHAPES(B2_X)
#undef B2_X
  return false;
}
// The rows the detector skips (|doppler| < minDoppler, CfarDetector1D.cpp:40) as ONE interval [lo, hi) of the handle's Doppler axis
// (monotonic: Ambiguity.cpp:60-66), which the stream kernel tests with scalar compares; false if they are not one interval.
bool cfar2d_dead_rows(const blah2hip_amb_s *h, double min_doppler, int *lo, int *hi)
{
  const int nD = (int)h->dims.n_doppler_bins;
  int first = nD, last = -1, count = 0;
  for (int i = 0; i < nD; i++)
    if (std::fabs(h->dopplerAxis[i]) < min_doppler) { first = std::min(first, i); last = i; count++; }
  if (count == 0) { *lo = *hi = 0; return true; }
  *lo = first; *hi = last + 1;
  return count == last + 1 - first;
}
bool cfar2d_use_stream(const blah2hip_amb_s *h, int ngd, int ntd, int ngf, int ntf, double min_doppler)
{
  if (h->cfar2dForce == BLAH2HIP_CFAR2D_SAT || h->cfar2dForce == BLAH2HIP_CFAR2D_TILE) return false;
  int lo, hi;
  return cfar2d_stream_shape(ngd, ntd, ngf, ntf) && cfar2d_dead_rows(h, min_doppler, &lo, &hi);
}

// rows per segment: the fewest rounds of (segment + its 2 hR halo rows) over the wave slots of the chip
void cfar2d_stream_launch(blah2hip_amb_s *h, const Cfar2dArgs &a, uint32_t n_cpi, hipStream_t st)
{
  Cfar2dStreamArgs ta;
  ta.d = a;
  ta.nCpi = (int32_t)n_cpi;
  const int hC = a.ngD + a.ntD, hR = a.ngF + a.ntF;
  ta.strips = (a.nDelay + (64 - 2 * hC) - 1) / (64 - 2 * hC);
  const int64_t slots = (int64_t)h->numCU * 4 * 5; // about five waves per SIMD at ~ 100 VGPRs
  int64_t best = INT64_MAX;
  for (int R : {8, 16, 32, 64, 128, 256, 512, 1024, (int)a.nD}) { // a lone CPI: short segments, every SIMD a wave
    if (R > a.nD) continue;
    const int64_t segs = (a.nD + R - 1) / R, tasks = segs * ta.strips * n_cpi;
    const int64_t cost = ((tasks + slots - 1) / slots) * (std::min(R, (int)a.nD) + 2 * hR + 16); // 16: start-up of a wave, in rows
    if (cost < best) { best = cost; ta.rowsPerSeg = std::min(R, (int)a.nD); ta.segs = (int32_t)segs; }
  }
  if (h->cfar2dSegRows > 0) { // BLAH2HIP_OPT_CFAR2D_SEG_ROWS
    ta.rowsPerSeg = std::min(h->cfar2dSegRows, (int)a.nD);
    ta.segs = (a.nD + ta.rowsPerSeg - 1) / ta.rowsPerSeg;
  }
  h->cfar2dSegRowsLast = ta.rowsPerSeg;
  h->cfar2dGridLast = 0;
  ta.nTasks = ta.nCpi * ta.segs * ta.strips;
  cfar2d_dead_rows(h, a.minDoppler, &ta.deadLo, &ta.deadHi);
  const int grid = (((ta.nTasks + 3) / 4) + 7) & ~7;
#define B2_X(TD, GD, TF, GF) \
  if (a.ntD == TD && a.ngD == GD && a.ntF == TF && a.ngF == GF) { \
    hipLaunchKernelGGL((cfar2d_stream_kernel<TD, GD, TF, GF>), dim3(grid), dim3(256), 0, st, ta); \
    return; \
  }
  C2S_SHAPES(B2_X)
#undef B2_X
}

int ensure_sat(blah2hip_amb_s *h)
{
  if (h->d_sat) return BLAH2HIP_OK;
  const size_t satElems = (size_t)(h->dims.n_doppler_bins + 1) * (h->dims.n_delay_bins + 1);
  HIPCHK(hipMalloc(&h->d_sat, satElems * h->dims.max_batch * sizeof(double)));
  HIPCHK(hipMemset(h->d_sat, 0, satElems * h->dims.max_batch * sizeof(double))); // zero borders
  return BLAH2HIP_OK;
}

// Which kernel a cell-averaging 2-D window runs on under the handle's BLAH2HIP_OPT_CFAR2D_KERNEL: the stream kernel, else the
// tile kernel, else the summed-area table, which is allocated here (a no-op once it is).  A forced kernel never runs another
// one: what it cannot do is refused.  blah2hip_cfar2d_prepare asks with min_doppler 0, which skips no rows.
int cfar2d_choose(blah2hip_amb_s *h, int ngd, int ntd, int ngf, int ntf, double min_doppler, bool *stream, bool *tile)
{
  *stream = cfar2d_use_stream(h, ngd, ntd, ngf, ntf, min_doppler);
  *tile = cfar2d_use_tile(h, ngd, ntd, ngf, ntf);
  if (h->cfar2dForce == BLAH2HIP_CFAR2D_TILE && !*tile)
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "2-D window beyond the tile kernel's halo (nGf + nTf <= 24, nGd + nTd <= 40)");
  if (h->cfar2dForce == BLAH2HIP_CFAR2D_STREAM && !cfar2d_stream_shape(ngd, ntd, ngf, ntf))
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "the stream kernel is not instantiated for this 2-D window (C2S_SHAPES in cfar_kernels.hpp)");
  // the handle's Doppler axis is monotonic (Ambiguity.cpp:60-66), so this cannot fail today
  if (h->cfar2dForce == BLAH2HIP_CFAR2D_STREAM && !*stream)
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "the stream kernel needs the rows below minDoppler to be one interval of the Doppler axis");
  return *stream || *tile ? BLAH2HIP_OK : ensure_sat(h);
}

// What CfarArgs and Cfar2dArgs have in common (d_map, d_metrics NULL: the handle's own), behind the zeroing of the counts
template <class Args>
int start_args(Args &a, const blah2hip_amb_s *h, const void *d_map, const double *d_metrics, uint32_t n_cpi, int32_t min_delay,
               double min_doppler, blah2hip_hit_t *d_hits, uint32_t cap, uint32_t *d_count, hipStream_t st)
{
  HIPCHK(hipMemsetAsync(d_count, 0, n_cpi * sizeof(uint32_t), st));
  a.map = d_map ? (const cf *)d_map : h->d_map;
  a.metrics = d_metrics ? d_metrics : h->d_metrics;
  a.doppler = h->d_doppler;
  a.hits = d_hits;
  a.count = d_count;
  a.nD = (int32_t)h->dims.n_doppler_bins;
  a.nDelay = (int32_t)h->dims.n_delay_bins;
  a.delayMin = h->delayMin;
  a.minDelay = min_delay;
  a.minDoppler = min_doppler;
  a.cap = cap;
  return BLAH2HIP_OK;
}

// A 1-D detector's launch, one workgroup per Doppler row: the row as fp64 |z|^2 in LDS while it fits (150 KB: 19 200 delay
// bins), straight from L2 beyond.  The attribute is set once per (device, kernel), to its largest use.
template <class Args>
int launch_rows(void (*staged)(Args), void (*unstaged)(Args), const Args &a, int nD, int nDelay, uint32_t n_cpi, hipStream_t st)
{
  const size_t rowBytes = (size_t)nDelay * sizeof(double);
  if (rowBytes <= 150 * 1024) {
    if (rowBytes > 48 * 1024) LDSCFG(staged, 150 * 1024);
    hipLaunchKernelGGL(staged, dim3(nD, n_cpi), dim3(256), rowBytes, st, a);
  } else {
    hipLaunchKernelGGL(unstaged, dim3(nD, n_cpi), dim3(256), 0, st, a);
  }
  HIPCHK(hipGetLastError());
  return BLAH2HIP_OK;
}

// the *_process calls' hit list on the device: worst case every cell fires; sized for that once
int ensure_hits(blah2hip_amb_s *h, size_t cells)
{
  if (h->hitCap >= cells) return BLAH2HIP_OK;
  if (h->d_hits) HIPCHK(hipFree(h->d_hits));
  h->d_hits = nullptr;
  HIPCHK(hipMalloc(&h->d_hits, cells * sizeof(blah2hip_hit_t)));
  h->hitCap = (uint32_t)cells;
  return BLAH2HIP_OK;
}

// A detector's hits into the caller's arrays, in the reference's order: it emits row by row, then by delay
// (CfarDetector1D.cpp:36-92).  delay0, doppler_axis: the map's axes.
int emit_hits(std::vector<blah2hip_hit_t> &hits, int32_t delay0, const double *doppler_axis, double *delay, double *doppler,
              double *snr, uint32_t cap, uint32_t *count)
{
  std::sort(hits.begin(), hits.end(), [](const blah2hip_hit_t &a, const blah2hip_hit_t &b) {
    return a.row != b.row ? a.row < b.row : a.col < b.col;
  });
  const uint32_t n = (uint32_t)hits.size();
  *count = n;
  if (n > cap) return fail(BLAH2HIP_ERR_CAPACITY, "detection capacity too small");
  for (uint32_t i = 0; i < n; i++) {
    if (delay) delay[i] = (double)(hits[i].col + delay0); // CfarDetector1D.cpp:88  j + x->delay[0]
    if (doppler) doppler[i] = doppler_axis[hits[i].row];  // :89
    if (snr) snr[i] = hits[i].snr;                        // :90
  }
  return BLAH2HIP_OK;
}

// ... of the detector call just enqueued on the handle's stream into h->d_hits / h->d_count
int hits_to_host(blah2hip_amb_s *h, double *delay, double *doppler, double *snr, uint32_t cap, uint32_t *count)
{
  uint32_t n = 0;
  HIPCHK(hipMemcpyAsync(&n, h->d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  n = std::min(n, h->hitCap);
  std::vector<blah2hip_hit_t> hits(n);
  if (n) HIPCHK(hipMemcpy(hits.data(), h->d_hits, n * sizeof(blah2hip_hit_t), hipMemcpyDeviceToHost));
  return emit_hits(hits, h->delayAxis[0], h->dopplerAxis.data(), delay, doppler, snr, cap, count);
}

// A *_process call: enqueue(map, metrics) runs the detector's *_dev call on a one-CPI view of the handle's buffers, into
// h->d_hits / h->d_count on the handle's stream
template <class Enqueue>
int process_one(blah2hip_amb_s *h, uint32_t cpi, double *delay, double *doppler, double *snr, uint32_t cap, uint32_t *count,
                Enqueue enqueue)
{
  if (!h || !count) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (cpi >= h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "cpi index out of range");
  HIPCHK(hipSetDevice(h->device));
  const size_t cells = (size_t)h->dims.n_doppler_bins * h->dims.n_delay_bins;
  int rc;
  if ((rc = ensure_hits(h, cells))) return rc;
  if ((rc = enqueue(h->d_map + cells * cpi, h->d_metrics + 2 * cpi))) return rc;
  return hits_to_host(h, delay, doppler, snr, cap, count);
}

// blah2hip_cfar1d_dev and, with `os`, blah2hip_oscfar1d_dev: one call but for the rank, its table and the kernel
int cfar1d_enqueue(bool os, blah2hip_amb_s *h, const void *d_map, const double *d_metrics, uint32_t n_cpi, double pfa,
                   uint32_t permille, int32_t n_guard, int32_t n_train, int32_t min_delay, double min_doppler,
                   blah2hip_hit_t *d_hits, uint32_t cap, uint32_t *d_count, void *stream)
{
  int rc;
  if ((rc = check_dev(h, d_hits, d_count, n_cpi)) || (rc = check_1d(n_guard, n_train, min_delay))) return rc;
  if (os && (rc = os_check_rank(permille))) return rc;
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  OsCfarArgs oa;
  CfarArgs &a = oa.c;
  oa.rank = nullptr; // cell averaging (permille 0) has no ranks: cfar_table leaves this alone and cfar1d_kernel takes oa.c only
  if ((rc = cfar_table(h, pfa, permille, (size_t)(2 * n_train), &a.alpha, &oa.rank, st))) return rc;
  if ((rc = start_args(a, h, d_map, d_metrics, n_cpi, min_delay, min_doppler, d_hits, cap, d_count, st))) return rc;
  a.delayAxis = nullptr; // the engine's own axis: delayMin + j
  a.nGuard = n_guard; a.nTrain = n_train;
  if ((rc = tic(h, BLAH2HIP_K_CFAR, st))) return rc;
  rc = os ? launch_rows(oscfar1d_kernel<true>, oscfar1d_kernel<false>, oa, a.nD, a.nDelay, n_cpi, st)
          : launch_rows(cfar1d_kernel<true>, cfar1d_kernel<false>, a, a.nD, a.nDelay, n_cpi, st);
  return rc ? rc : toc(h, BLAH2HIP_K_CFAR, st);
}

// ... and blah2hip_cfar1d_prepare / blah2hip_oscfar1d_prepare
int cfar1d_pin(bool os, blah2hip_amb_s *h, double pfa, uint32_t permille, int32_t n_train)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (n_train < 0 || n_train > 127) return fail(BLAH2HIP_ERR_INVALID, "nTrain outside int8 range");
  int rc;
  if (os && (rc = os_check_rank(permille))) return rc;
  HIPCHK(hipSetDevice(h->device));
  const double *d = nullptr;
  const uint32_t *r = nullptr;
  return cfar_table(h, pfa, permille, (size_t)(2 * n_train), &d, &r, nullptr, true);
}

// The clutter map's table of this pfa on the device, in the map's own list
int cmap_table(blah2hip_cmap_s *cm, double pfa, const double **alpha, hipStream_t st = nullptr, bool pin = false)
{
  HipTableDevice dev;
  return cm->tables.get(
      dev, pfa, [&](double e) { return e == pfa; },
      [&](std::vector<double> &host) {
        const uint32_t last = CMAP_AGES * cm->memory;
        host.resize(last + 1);
        cmap_alpha_fill(pfa, cm->memory, last, host.data());
        return BLAH2HIP_OK;
      },
      "clutter-map table of this pfa is not resident: call blah2hip_cmap_prepare before capturing the stream",
      "clutter-map table upload: ", st, pin, alpha);
}

int check_pfa(double pfa)
{
  if (!(pfa > 0.0 && pfa < 1.0)) return fail(BLAH2HIP_ERR_INVALID, "pfa outside (0, 1)");
  return BLAH2HIP_OK;
}

// ---- greatest-of / smallest-of ----
// The in-bounds training columns of the two halves of delay column j (gocfar_kernels.hpp: the same expressions)
void gocfar_cols(int j, int nC, int nG, int nT, int *cL, int *cR)
{
  *cL = std::max(std::min(j - nG, nC) - std::max(j - nG - nT, 1), 0);
  *cR = std::min(j + nG + nT + 1, nC) - std::min(j + nG + 1, nC);
}

// The table of gocfar_kernels.hpp for this handle's maps: alpha[((rows - 1)(nT + 1) + cL)(nT + 1) + cR] for every (rows, cL,
// cR) a cell of the map has under the window (hR 0: the 1-D detector, rows = 1), NaN elsewhere.  Distinct triples with one
// (a, b) = (rows cL, rows cR) share one solve.
void gocfar_host_table(const blah2hip_amb_s *h, double pfa, uint32_t kind, int nG, int nT, int hR, std::vector<double> &tab)
{
  const int nD = (int)h->dims.n_doppler_bins, nC = (int)h->dims.n_delay_bins, W = nT + 1;
  tab.assign((size_t)(2 * hR + 1) * W * W, std::nan(""));
  std::vector<char> rowsSeen(2 * hR + 2, 0), colsSeen((size_t)W * W, 0);
  for (int i = 0; i < nD; i++) rowsSeen[std::min(i + hR, nD - 1) - std::max(i - hR, 0) + 1] = 1;
  for (int j = 0; j < nC; j++) {
    int cL, cR;
    gocfar_cols(j, nC, nG, nT, &cL, &cR);
    colsSeen[(size_t)cL * W + cR] = 1;
  }
  std::map<std::pair<uint32_t, uint32_t>, uint32_t> index;
  std::vector<uint32_t> a, b;
  for (int rows = 1; rows <= 2 * hR + 1; rows++)
    for (int c = 0; rowsSeen[rows] && c < W * W; c++)
      if (colsSeen[c] && c != 0 && index.emplace(std::make_pair((uint32_t)(rows * (c / W)), (uint32_t)(rows * (c % W))), (uint32_t)a.size()).second) {
        a.push_back((uint32_t)(rows * (c / W)));
        b.push_back((uint32_t)(rows * (c % W)));
      }
  std::vector<double> alpha(a.size());
  goso_alpha_fill(pfa, kind, (uint32_t)a.size(), a.data(), b.data(), alpha.data());
  for (int rows = 1; rows <= 2 * hR + 1; rows++)
    for (int c = 0; rowsSeen[rows] && c < W * W; c++)
      if (colsSeen[c] && c != 0)
        tab[(size_t)(rows - 1) * W * W + c] = alpha[index.at(std::make_pair((uint32_t)(rows * (c / W)), (uint32_t)(rows * (c % W))))];
}

// ... on the device, in h->goTables, keyed by (pfa, kind, nGuard, nTrain, hR) -- the map's geometry is the handle's
int gocfar_table(blah2hip_amb_s *h, double pfa, uint32_t kind, int nG, int nT, int hR, const double **alpha,
                 hipStream_t st = nullptr, bool pin = false)
{
  typedef blah2hip_amb_s::GoKey Key;
  HipTableDevice dev;
  return h->goTables.get(
      dev, Key{pfa, kind, nG, nT, hR},
      [&](const Key &e) { return e.pfa == pfa && e.kind == kind && e.nG == nG && e.nT == nT && e.hR == hR; },
      [&](std::vector<double> &host) {
        gocfar_host_table(h, pfa, kind, nG, nT, hR, host);
        return BLAH2HIP_OK;
      },
      "greatest-of / smallest-of table of this (pfa, kind, window) is not resident: call "
      "blah2hip_gocfar1d_prepare / blah2hip_gocfar2d_prepare before capturing the stream",
      "greatest-of / smallest-of table upload: ", st, pin, alpha);
}

// what the greatest-of / smallest-of calls check after the window's sizes: the kind, pfa, the handle's looks
int gocfar_check(const blah2hip_amb_s *h, double pfa, uint32_t kind)
{
  if (kind != BLAH2HIP_CFAR_GO && kind != BLAH2HIP_CFAR_SO) return fail(BLAH2HIP_ERR_INVALID, "kind: BLAH2HIP_CFAR_GO or BLAH2HIP_CFAR_SO");
  if (int rc = check_pfa(pfa)) return rc;
  if (h->cfarLooks > 1)
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "greatest-of / smallest-of: the thresholds are made for one look per cell (BLAH2HIP_OPT_CFAR_LOOKS is above 1)");
  return BLAH2HIP_OK;
}

int gocfar2d_check(int32_t ngd, int32_t ntd, int32_t hr, int32_t min_delay = 0)
{
  if (int rc = check_2d(ngd, ntd, 0, hr, min_delay)) return rc;
  if (hr > C2T_MAX_HR || ngd + ntd > C2T_MAX_HC)
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "greatest-of / smallest-of 2-D window beyond the tile's halo (n_rows_doppler <= 24, nGd + nTd <= 40)");
  return BLAH2HIP_OK;
}

} // namespace

extern "C" {

// ------------------------------------------------------------ clutter map --
// Host arithmetic only (cfar_alpha.hpp)
int blah2hip_cmap_alpha(double pfa, uint32_t memory, uint32_t max_age, double *alpha)
{
  if (!alpha) return fail(BLAH2HIP_ERR_INVALID, "NULL table");
  if (memory == 0 || memory > BLAH2HIP_MAX_CMAP_MEMORY) return fail(BLAH2HIP_ERR_INVALID, "memory outside [1, BLAH2HIP_MAX_CMAP_MEMORY]");
  if (int rc = check_pfa(pfa)) return rc;
  cmap_alpha_fill(pfa, memory, max_age, alpha);
  return BLAH2HIP_OK;
}

int blah2hip_cmap_create(blah2hip_amb_t amb, uint32_t memory, uint32_t flags, blah2hip_cmap_t *out)
{
  if (!amb || !out) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (memory == 0 || memory > BLAH2HIP_MAX_CMAP_MEMORY) return fail(BLAH2HIP_ERR_INVALID, "memory outside [1, BLAH2HIP_MAX_CMAP_MEMORY]");
  if (flags & ~(uint32_t)BLAH2HIP_CMAP_NORMALISE) return fail(BLAH2HIP_ERR_INVALID, "unknown flag bits");
  const size_t cells = (size_t)amb->dims.n_doppler_bins * amb->dims.n_delay_bins;
  if (cells >= (1ull << 32)) return fail(BLAH2HIP_ERR_UNSUPPORTED, "clutter map: more than 2^32 - 1 cells");
  HIPCHK(hipSetDevice(amb->device));
  blah2hip_cmap_s *cm = new blah2hip_cmap_s;
  cm->amb = amb;
  cm->memory = memory;
  cm->flags = flags;
  hipError_t e = hipMalloc(&cm->d_bg, cells * sizeof(float));
  if (e == hipSuccess) e = hipMemset(cm->d_bg, 0, cells * sizeof(float)); // what blah2hip_cmap_read_background shows before the first CPI
  if (e != hipSuccess) {
    (void)hipFree(cm->d_bg);
    delete cm;
    return fail(BLAH2HIP_ERR_HIP, std::string("hipMalloc(clutter map): ") + hipGetErrorString(e));
  }
  *out = cm;
  return BLAH2HIP_OK;
}

int blah2hip_cmap_destroy(blah2hip_cmap_t cm)
{
  if (!cm) return BLAH2HIP_OK;
  int rc = BLAH2HIP_OK;
  (void)hipSetDevice(cm->amb->device);
  (void)hipDeviceSynchronize(); // enqueued calls may still use the plane and the tables
  if (hipFree(cm->d_bg) != hipSuccess) rc = fail(BLAH2HIP_ERR_HIP, "hipFree(clutter map)");
  HipTableDevice dev;
  if (!cm->tables.free_all(dev)) rc = fail(BLAH2HIP_ERR_HIP, "hipFree(clutter-map table)");
  delete cm;
  return rc;
}

int blah2hip_cmap_reset(blah2hip_cmap_t cm)
{
  if (!cm) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  cm->age = 0; // the plane keeps its bytes: the first CPI of the new count overwrites them unread
  return BLAH2HIP_OK;
}

int blah2hip_cmap_age(blah2hip_cmap_t cm, uint64_t *age)
{
  if (!cm || !age) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  *age = cm->age;
  return BLAH2HIP_OK;
}

int blah2hip_cmap_prepare(blah2hip_cmap_t cm, double pfa)
{
  if (!cm) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (int rc = check_pfa(pfa)) return rc;
  HIPCHK(hipSetDevice(cm->amb->device));
  const double *d = nullptr;
  return cmap_table(cm, pfa, &d, nullptr, true);
}

int blah2hip_cmap_process_dev(blah2hip_cmap_t cm, const void *d_map, const double *d_metrics, uint32_t n_cpi, double pfa,
                              int32_t min_delay, double min_doppler, blah2hip_hit_t *d_hits, uint32_t cap, uint32_t *d_count,
                              uint8_t *d_out_exceed, float *d_out_level, void *stream)
{
  if (!cm) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  blah2hip_amb_s *h = cm->amb;
  if (n_cpi == 0 || n_cpi > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "n_cpi outside [1, max_batch]");
  int rc;
  if ((rc = check_pfa(pfa))) return rc;
  if ((d_hits == nullptr) != (d_count == nullptr)) return fail(BLAH2HIP_ERR_INVALID, "d_hits and d_count: both or neither");
  if (d_hits && cap == 0) return fail(BLAH2HIP_ERR_INVALID, "cap is 0");
  const cf *map = d_map ? (const cf *)d_map : h->d_map;
  if ((uintptr_t)map & 7) return fail(BLAH2HIP_ERR_INVALID, "a map is not 8-byte aligned");
  if (h->cfarLooks > 1)
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "clutter map: the thresholds are made for one look per cell (BLAH2HIP_OPT_CFAR_LOOKS is above 1)");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  CmapArgs a;
  if ((rc = cmap_table(cm, pfa, &a.alpha, st))) return rc;
  if (d_count) HIPCHK(hipMemsetAsync(d_count, 0, n_cpi * sizeof(uint32_t), st));
  const size_t cells = (size_t)h->dims.n_doppler_bins * h->dims.n_delay_bins;
  a.map = map;
  a.metrics = d_metrics ? d_metrics : h->d_metrics;
  a.doppler = h->d_doppler;
  a.bg = cm->d_bg;
  a.hits = d_hits;
  a.count = d_count;
  a.exceed = d_out_exceed;
  a.level = d_out_level;
  a.cells = (uint32_t)cells;
  a.nCpi = n_cpi;
  a.nDelay = (int32_t)h->dims.n_delay_bins;
  a.delayMin = h->delayMin;
  a.minDelay = min_delay;
  a.minDoppler = min_doppler;
  a.cap = cap;
  // The age travels in the launch arguments: a captured graph repeats the launch, not the count.  Nothing looks beyond
  // age 16 T (the table's last entry, k = T), so the argument stops there.
  a.age0 = (uint32_t)std::min<uint64_t>(cm->age, (uint64_t)CMAP_AGES * cm->memory);
  a.memory = cm->memory;
  a.normalise = (cm->flags & BLAH2HIP_CMAP_NORMALISE) ? 1u : 0u;
  const uint32_t G = (uint32_t)(((cells + 1) / 2 + 255) / 256);
  if ((rc = tic(h, BLAH2HIP_K_CFAR, st))) return rc;
  hipLaunchKernelGGL(cmap_kernel, dim3(G), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  if ((rc = toc(h, BLAH2HIP_K_CFAR, st))) return rc;
  cm->age += n_cpi;
  return BLAH2HIP_OK;
}

int blah2hip_cmap_gate_dev(blah2hip_cmap_t cm, const uint8_t *d_exceed, uint32_t n_cpi, const blah2hip_hit_t *d_hits, uint32_t cap,
                           const uint32_t *d_count, blah2hip_hit_t *d_hits_out, uint32_t *d_count_out, void *stream)
{
  if (!cm || !d_exceed || !d_hits || !d_count || !d_hits_out || !d_count_out) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  blah2hip_amb_s *h = cm->amb;
  if (n_cpi == 0 || n_cpi > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "n_cpi outside [1, max_batch]");
  if (cap == 0) return fail(BLAH2HIP_ERR_INVALID, "cap is 0");
  const size_t listBytes = (size_t)n_cpi * cap * sizeof(blah2hip_hit_t), countBytes = n_cpi * sizeof(uint32_t);
  if (ranges_overlap(d_hits, listBytes, d_hits_out, listBytes) || ranges_overlap(d_count, countBytes, d_count_out, countBytes))
    return fail(BLAH2HIP_ERR_INVALID, "gate: the output list overlaps the input list (the compaction cannot run in place)");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  GateArgs a;
  a.exceed = d_exceed;
  a.hits = d_hits;
  a.count = d_count;
  a.out = d_hits_out;
  a.countOut = d_count_out;
  a.nD = (int32_t)h->dims.n_doppler_bins;
  a.nDelay = (int32_t)h->dims.n_delay_bins;
  a.cap = cap;
  int rc;
  if ((rc = tic(h, BLAH2HIP_K_CFAR, st))) return rc;
  hipLaunchKernelGGL(hits_gate_kernel, dim3(n_cpi), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  return toc(h, BLAH2HIP_K_CFAR, st);
}

int blah2hip_cmap_read_background(blah2hip_cmap_t cm, float *b)
{
  if (!cm || !b) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  blah2hip_amb_s *h = cm->amb;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(b, cm->d_bg, (size_t)h->dims.n_doppler_bins * h->dims.n_delay_bins * sizeof(float), hipMemcpyDeviceToHost));
  return BLAH2HIP_OK;
}

// ------------------------------------------------------------------- CFAR --
// Host arithmetic only (cfar_alpha.hpp)
int blah2hip_cfar_alpha(double pfa, uint32_t looks, uint32_t max_n, double *alpha)
{
  if (!alpha) return fail(BLAH2HIP_ERR_INVALID, "NULL table");
  if (looks == 0 || looks > BLAH2HIP_MAX_CFAR_LOOKS) return fail(BLAH2HIP_ERR_INVALID, "looks outside [1, BLAH2HIP_MAX_CFAR_LOOKS]");
  if (looks > 1 && !(pfa > 0.0 && pfa < 1.0)) return fail(BLAH2HIP_ERR_INVALID, "pfa outside (0, 1) with more than one look");
  cfar_alpha_fill(pfa, looks, max_n, alpha);
  return BLAH2HIP_OK;
}

int blah2hip_cfar1d_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics,
                        uint32_t n_cpi, double pfa, int32_t n_guard, int32_t n_train,
                        int32_t min_delay, double min_doppler, blah2hip_hit_t *d_hits, uint32_t cap,
                        uint32_t *d_count, void *stream)
{
  return cfar1d_enqueue(false, h, d_map, d_metrics, n_cpi, pfa, 0, n_guard, n_train, min_delay, min_doppler, d_hits, cap, d_count, stream);
}

int blah2hip_cfar1d_process(blah2hip_amb_t h, uint32_t cpi, double pfa, int32_t n_guard,
                            int32_t n_train, int32_t min_delay, double min_doppler, double *delay,
                            double *doppler, double *snr, uint32_t cap, uint32_t *count)
{
  return process_one(h, cpi, delay, doppler, snr, cap, count, [&](const cf *m, const double *met) {
    return blah2hip_cfar1d_dev(h, m, met, 1, pfa, n_guard, n_train, min_delay, min_doppler, h->d_hits, h->hitCap, h->d_count,
                               h->stream);
  });
}

// CfarDetector1D::process on a map that lives on the HOST (any Map<complex<double>>, not only one
// the engine produced): uploads it, runs cfar1d_kernel, frees.  noise_power is Map::noisePower.
int blah2hip_cfar1d_map(const float *map, uint32_t n_doppler, uint32_t n_delay, const int32_t *delay_axis,
                        const double *doppler_axis, double noise_power, double pfa, int32_t n_guard,
                        int32_t n_train, int32_t min_delay, double min_doppler, int device, double *delay,
                        double *doppler, double *snr, uint32_t cap, uint32_t *count)
{
  if (!map || !delay_axis || !doppler_axis || !count) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (n_doppler == 0 || n_delay == 0) return fail(BLAH2HIP_ERR_INVALID, "empty map");
  int rc;
  if ((rc = check_1d(n_guard, n_train, min_delay))) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(BLAH2HIP_ERR_NO_DEVICE, "no HIP device visible (the HIP path is the only path)");
  if (device < 0 || device >= ndev) return fail(BLAH2HIP_ERR_INVALID, "device index out of range");
  HIPCHK(hipSetDevice(device));
  const size_t cells = (size_t)n_doppler * n_delay;
  std::vector<double> alpha(2 * n_train + 1);
  if ((rc = blah2hip_cfar_alpha(pfa, 1, (uint32_t)(2 * n_train), alpha.data()))) return rc; // one look: any pfa
  const double met[2] = {noise_power, 0.0};
  char *pool = nullptr; // one allocation: map | hits | doppler | alpha | metrics | delay axis | count
  const size_t oMap = 0, oHits = oMap + cells * sizeof(cf), oDop = oHits + cells * sizeof(blah2hip_hit_t),
               oAlpha = oDop + n_doppler * sizeof(double), oMet = oAlpha + alpha.size() * sizeof(double),
               oAxis = oMet + 2 * sizeof(double), oCnt = oAxis + n_delay * sizeof(int32_t), total = oCnt + sizeof(uint32_t);
  HIPCHK(hipMalloc(&pool, total));
  std::vector<blah2hip_hit_t> hits;
  uint32_t n = 0;
  auto run = [&]() -> int {
    HIPCHK(hipMemcpy(pool + oMap, map, cells * sizeof(cf), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(pool + oDop, doppler_axis, n_doppler * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(pool + oAlpha, alpha.data(), alpha.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(pool + oMet, met, sizeof met, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(pool + oAxis, delay_axis, n_delay * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(pool + oCnt, 0, sizeof(uint32_t)));
    CfarArgs a;
    a.map = (const cf *)(pool + oMap);
    a.metrics = (const double *)(pool + oMet);
    a.doppler = (const double *)(pool + oDop);
    a.alpha = (const double *)(pool + oAlpha);
    a.hits = (blah2hip_hit_t *)(pool + oHits);
    a.count = (uint32_t *)(pool + oCnt);
    a.nD = (int32_t)n_doppler; a.nDelay = (int32_t)n_delay; a.delayMin = delay_axis[0];
    a.delayAxis = (const int32_t *)(pool + oAxis); // x->delay[j] of a caller-built map need not be delay[0] + j (CfarDetector1D.cpp:53)
    a.nGuard = n_guard; a.nTrain = n_train; a.minDelay = min_delay; a.minDoppler = min_doppler;
    a.cap = (uint32_t)cells;
    if (int lrc = launch_rows(cfar1d_kernel<true>, cfar1d_kernel<false>, a, a.nD, a.nDelay, 1, nullptr)) return lrc;
    HIPCHK(hipMemcpy(&n, pool + oCnt, sizeof(uint32_t), hipMemcpyDeviceToHost)); // synchronises with the null stream
    hits.resize(n);
    if (n) HIPCHK(hipMemcpy(hits.data(), pool + oHits, n * sizeof(blah2hip_hit_t), hipMemcpyDeviceToHost));
    return BLAH2HIP_OK;
  };
  rc = run();
  (void)hipFree(pool);
  if (rc) return rc;
  return emit_hits(hits, delay_axis[0], doppler_axis, delay, doppler, snr, cap, count);
}

// ---------------------------------------------------------------- 2-D CFAR --
int blah2hip_cfar2d_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics, uint32_t n_cpi,
                        double pfa, int32_t ngd, int32_t ntd, int32_t ngf, int32_t ntf, int32_t min_delay,
                        double min_doppler, blah2hip_hit_t *d_hits, uint32_t cap, uint32_t *d_count,
                        void *stream)
{
  int rc;
  if ((rc = check_dev(h, d_hits, d_count, n_cpi)) || (rc = check_2d(ngd, ntd, ngf, ntf, min_delay))) return rc;
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  bool useStream, useTile;
  if ((rc = cfar2d_choose(h, ngd, ntd, ngf, ntf, min_doppler, &useStream, &useTile))) return rc;
  Cfar2dArgs a;
  if ((rc = cfar_table(h, pfa, 0, window_cells(ngd, ntd, ngf, ntf), &a.alpha, nullptr, st))) return rc;
  if ((rc = start_args(a, h, d_map, d_metrics, n_cpi, min_delay, min_doppler, d_hits, cap, d_count, st))) return rc;
  a.sat = h->d_sat;
  a.ngD = ngd; a.ntD = ntd; a.ngF = ngf; a.ntF = ntf;
  const int nD = a.nD, nC = a.nDelay;
  if (useStream) {
    if ((rc = tic(h, BLAH2HIP_K_CFAR, st))) return rc;
    cfar2d_stream_launch(h, a, n_cpi, st);
    HIPCHK(hipGetLastError());
    return toc(h, BLAH2HIP_K_CFAR, st);
  }
  if (useTile) {
    Cfar2dTileArgs ta;
    ta.d = a;
    ta.nCpi = (int32_t)n_cpi;
    ta.rowsOut = C2T_ROWS - 2 * (ngf + ntf);
    ta.tilesX = (nC + C2T_COLS - 1) / C2T_COLS;
    ta.tilesY = (nD + ta.rowsOut - 1) / ta.rowsOut;
    const int hC = ngd + ntd;
    // the whole threshold table in LDS when it fits beside the tile (the default 17 x 9 window: 154 entries)
    const int64_t tableN = (int64_t)window_cells(ngd, ntd, ngf, ntf) + 1;
    ta.alphaLds = (tableN <= 2048 && c2t_lds_bytes(hC, (int)tableN) <= 160 * 1024) ? (int32_t)tableN : 0;
    const size_t lds = c2t_lds_bytes(hC, ta.alphaLds);
    const int64_t nAll = (int64_t)ta.tilesX * ta.tilesY * n_cpi;
    const int64_t wgCap = h->cfar2dGridForce > 0 ? h->cfar2dGridForce : h->numCU; // BLAH2HIP_OPT_CFAR2D_GRID
    const int grid = (int)std::max<int64_t>(8, (std::min<int64_t>(nAll, wgCap) + 7) & ~7); // one persistent workgroup per CU (LDS)
    h->cfar2dGridLast = grid;
    h->cfar2dSegRowsLast = 0;
    if ((rc = tic(h, BLAH2HIP_K_CFAR, st))) return rc;
    auto launch = [&](auto kern) -> int {
      LDSCFG(kern, lds);
      hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * C2T_WAVES), lds, st, ta);
      return BLAH2HIP_OK;
    };
    const bool two = C2T_COLS + 2 * hC <= 128;
    if (two) rc = ta.alphaLds ? launch(cfar2d_tile_kernel<2, true>) : launch(cfar2d_tile_kernel<2, false>);
    else rc = ta.alphaLds ? launch(cfar2d_tile_kernel<3, true>) : launch(cfar2d_tile_kernel<3, false>);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return toc(h, BLAH2HIP_K_CFAR, st);
  }
  h->cfar2dGridLast = h->cfar2dSegRowsLast = 0;
  if ((rc = tic(h, BLAH2HIP_K_SAT_ROWS, st))) return rc;
  hipLaunchKernelGGL(sat_rows_kernel, dim3(nD, n_cpi), dim3(256), 0, st, a);
  if ((rc = toc(h, BLAH2HIP_K_SAT_ROWS, st))) return rc;
  if ((rc = tic(h, BLAH2HIP_K_SAT_COLS, st))) return rc;
  hipLaunchKernelGGL(sat_cols_kernel, dim3((nC + 63) / 64, n_cpi), dim3(64), 0, st, a);
  if ((rc = toc(h, BLAH2HIP_K_SAT_COLS, st))) return rc;
  if ((rc = tic(h, BLAH2HIP_K_CFAR, st))) return rc;
  hipLaunchKernelGGL(cfar2d_kernel, dim3((nC + 255) / 256, nD, n_cpi), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  return toc(h, BLAH2HIP_K_CFAR, st);
}

int blah2hip_cfar1d_prepare(blah2hip_amb_t h, double pfa, int32_t n_train)
{
  return cfar1d_pin(false, h, pfa, 0, n_train);
}

int blah2hip_cfar2d_prepare(blah2hip_amb_t h, double pfa, int32_t ngd, int32_t ntd, int32_t ngf, int32_t ntf)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  int rc;
  if ((rc = check_2d(ngd, ntd, ngf, ntf))) return rc;
  HIPCHK(hipSetDevice(h->device));
  bool useStream, useTile;
  if ((rc = cfar2d_choose(h, ngd, ntd, ngf, ntf, 0.0, &useStream, &useTile))) return rc;
  const double *d = nullptr;
  return cfar_table(h, pfa, 0, window_cells(ngd, ntd, ngf, ntf), &d, nullptr, nullptr, true);
}

int blah2hip_cfar2d_process(blah2hip_amb_t h, uint32_t cpi, double pfa, int32_t ngd, int32_t ntd,
                            int32_t ngf, int32_t ntf, int32_t min_delay, double min_doppler, double *delay,
                            double *doppler, double *snr, uint32_t cap, uint32_t *count)
{
  return process_one(h, cpi, delay, doppler, snr, cap, count, [&](const cf *m, const double *met) {
    return blah2hip_cfar2d_dev(h, m, met, 1, pfa, ngd, ntd, ngf, ntf, min_delay, min_doppler, h->d_hits, h->hitCap, h->d_count,
                               h->stream);
  });
}

// ------------------------------------------------------ ordered statistic --
// Host arithmetic only (cfar_alpha.hpp)
int blah2hip_oscfar_alpha(double pfa, uint32_t looks, uint32_t rank_permille, uint32_t max_n, double *alpha, uint32_t *rank)
{
  if (!alpha) return fail(BLAH2HIP_ERR_INVALID, "NULL table");
  if (looks == 0 || looks > BLAH2HIP_MAX_CFAR_LOOKS) return fail(BLAH2HIP_ERR_INVALID, "looks outside [1, BLAH2HIP_MAX_CFAR_LOOKS]");
  if (int rc = os_check_rank(rank_permille)) return rc;
  if (int rc = check_pfa(pfa)) return rc;
  oscfar_alpha_fill(pfa, looks, rank_permille, max_n, alpha, rank);
  return BLAH2HIP_OK;
}

int blah2hip_oscfar1d_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics, uint32_t n_cpi, double pfa,
                          uint32_t rank_permille, int32_t n_guard, int32_t n_train, int32_t min_delay, double min_doppler,
                          blah2hip_hit_t *d_hits, uint32_t cap, uint32_t *d_count, void *stream)
{
  return cfar1d_enqueue(true, h, d_map, d_metrics, n_cpi, pfa, rank_permille, n_guard, n_train, min_delay, min_doppler, d_hits, cap,
                        d_count, stream);
}

int blah2hip_oscfar1d_prepare(blah2hip_amb_t h, double pfa, uint32_t rank_permille, int32_t n_train)
{
  return cfar1d_pin(true, h, pfa, rank_permille, n_train);
}

int blah2hip_oscfar1d_process(blah2hip_amb_t h, uint32_t cpi, double pfa, uint32_t rank_permille, int32_t n_guard,
                              int32_t n_train, int32_t min_delay, double min_doppler, double *delay, double *doppler,
                              double *snr, uint32_t cap, uint32_t *count)
{
  return process_one(h, cpi, delay, doppler, snr, cap, count, [&](const cf *m, const double *met) {
    return blah2hip_oscfar1d_dev(h, m, met, 1, pfa, rank_permille, n_guard, n_train, min_delay, min_doppler, h->d_hits,
                                 h->hitCap, h->d_count, h->stream);
  });
}

// what the 2-D ordered-statistic calls check after the handle: the window's sizes (min_delay: see check_2d), the rank, the halo
static int os2d_check(uint32_t rank_permille, int32_t ngd, int32_t ntd, int32_t ngf, int32_t ntf, int32_t min_delay = 0)
{
  int rc;
  if ((rc = check_2d(ngd, ntd, ngf, ntf, min_delay, true)) || (rc = os_check_rank(rank_permille))) return rc;
  if (ngf + ntf > C2T_MAX_HR || ngd + ntd > C2T_MAX_HC)
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "ordered-statistic 2-D window beyond the tile's halo (nGf + nTf <= 24, nGd + nTd <= 40): "
                                          "a rank has no summed-area form");
  return BLAH2HIP_OK;
}

int blah2hip_oscfar2d_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics, uint32_t n_cpi, double pfa,
                          uint32_t rank_permille, int32_t ngd, int32_t ntd, int32_t ngf, int32_t ntf, int32_t min_delay,
                          double min_doppler, blah2hip_hit_t *d_hits, uint32_t cap, uint32_t *d_count, void *stream)
{
  int rc;
  if ((rc = check_dev(h, d_hits, d_count, n_cpi)) || (rc = os2d_check(rank_permille, ngd, ntd, ngf, ntf, min_delay))) return rc;
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  OsCfar2dArgs oa;
  Cfar2dArgs &a = oa.d;
  if ((rc = cfar_table(h, pfa, rank_permille, window_cells(ngd, ntd, ngf, ntf), &a.alpha, &oa.rank, st))) return rc;
  if ((rc = start_args(a, h, d_map, d_metrics, n_cpi, min_delay, min_doppler, d_hits, cap, d_count, st))) return rc;
  a.sat = nullptr;
  a.ngD = ngd; a.ntD = ntd; a.ngF = ngf; a.ntF = ntf;
  const size_t lds = o2_lds_bytes(ngd + ntd, ngf + ntf);
  if (lds > 48 * 1024) LDSCFG(oscfar2d_kernel, o2_lds_bytes(C2T_MAX_HC, C2T_MAX_HR)); // once per (device, kernel): its largest use
  if ((rc = tic(h, BLAH2HIP_K_CFAR, st))) return rc;
  hipLaunchKernelGGL(oscfar2d_kernel, dim3((a.nDelay + O2_COLS - 1) / O2_COLS, (a.nD + O2_ROWS - 1) / O2_ROWS, n_cpi), dim3(256),
                     lds, st, oa);
  HIPCHK(hipGetLastError());
  return toc(h, BLAH2HIP_K_CFAR, st);
}

int blah2hip_oscfar2d_prepare(blah2hip_amb_t h, double pfa, uint32_t rank_permille, int32_t ngd, int32_t ntd, int32_t ngf,
                              int32_t ntf)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  int rc;
  if ((rc = os2d_check(rank_permille, ngd, ntd, ngf, ntf))) return rc;
  HIPCHK(hipSetDevice(h->device));
  const double *d = nullptr;
  const uint32_t *r = nullptr;
  return cfar_table(h, pfa, rank_permille, window_cells(ngd, ntd, ngf, ntf), &d, &r, nullptr, true);
}

int blah2hip_oscfar2d_process(blah2hip_amb_t h, uint32_t cpi, double pfa, uint32_t rank_permille, int32_t ngd, int32_t ntd,
                              int32_t ngf, int32_t ntf, int32_t min_delay, double min_doppler, double *delay,
                              double *doppler, double *snr, uint32_t cap, uint32_t *count)
{
  return process_one(h, cpi, delay, doppler, snr, cap, count, [&](const cf *m, const double *met) {
    return blah2hip_oscfar2d_dev(h, m, met, 1, pfa, rank_permille, ngd, ntd, ngf, ntf, min_delay, min_doppler, h->d_hits,
                                 h->hitCap, h->d_count, h->stream);
  });
}

// ------------------------------------------------- greatest-of / smallest-of --
// Host arithmetic only (cfar_alpha.hpp)
int blah2hip_gocfar_alpha(double pfa, uint32_t kind, uint32_t n_pairs, const uint32_t *a, const uint32_t *b, double *alpha)
{
  if (!a || !b || !alpha) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (kind != BLAH2HIP_CFAR_GO && kind != BLAH2HIP_CFAR_SO) return fail(BLAH2HIP_ERR_INVALID, "kind: BLAH2HIP_CFAR_GO or BLAH2HIP_CFAR_SO");
  if (int rc = check_pfa(pfa)) return rc;
  goso_alpha_fill(pfa, kind, n_pairs, a, b, alpha);
  return BLAH2HIP_OK;
}

int blah2hip_gocfar1d_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics, uint32_t n_cpi, double pfa, uint32_t kind,
                          int32_t n_guard, int32_t n_train, int32_t min_delay, double min_doppler, blah2hip_hit_t *d_hits,
                          uint32_t cap, uint32_t *d_count, void *stream)
{
  int rc;
  if ((rc = check_dev(h, d_hits, d_count, n_cpi)) || (rc = check_1d(n_guard, n_train, min_delay)) || (rc = gocfar_check(h, pfa, kind)))
    return rc;
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  GoCfarArgs ga;
  CfarArgs &a = ga.c;
  ga.kind = kind;
  if ((rc = gocfar_table(h, pfa, kind, n_guard, n_train, 0, &a.alpha, st))) return rc;
  if ((rc = start_args(a, h, d_map, d_metrics, n_cpi, min_delay, min_doppler, d_hits, cap, d_count, st))) return rc;
  a.delayAxis = nullptr; // the engine's own axis: delayMin + j
  a.nGuard = n_guard; a.nTrain = n_train;
  if ((rc = tic(h, BLAH2HIP_K_CFAR, st))) return rc;
  rc = launch_rows(gocfar1d_kernel<true>, gocfar1d_kernel<false>, ga, a.nD, a.nDelay, n_cpi, st);
  return rc ? rc : toc(h, BLAH2HIP_K_CFAR, st);
}

int blah2hip_gocfar1d_prepare(blah2hip_amb_t h, double pfa, uint32_t kind, int32_t n_guard, int32_t n_train)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  int rc;
  if ((rc = check_1d(n_guard, n_train, 0)) || (rc = gocfar_check(h, pfa, kind))) return rc;
  HIPCHK(hipSetDevice(h->device));
  const double *d = nullptr;
  return gocfar_table(h, pfa, kind, n_guard, n_train, 0, &d, nullptr, true);
}

int blah2hip_gocfar1d_process(blah2hip_amb_t h, uint32_t cpi, double pfa, uint32_t kind, int32_t n_guard, int32_t n_train,
                              int32_t min_delay, double min_doppler, double *delay, double *doppler, double *snr, uint32_t cap,
                              uint32_t *count)
{
  return process_one(h, cpi, delay, doppler, snr, cap, count, [&](const cf *m, const double *met) {
    return blah2hip_gocfar1d_dev(h, m, met, 1, pfa, kind, n_guard, n_train, min_delay, min_doppler, h->d_hits, h->hitCap,
                                 h->d_count, h->stream);
  });
}

int blah2hip_gocfar2d_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics, uint32_t n_cpi, double pfa, uint32_t kind,
                          int32_t ngd, int32_t ntd, int32_t n_rows_doppler, int32_t min_delay, double min_doppler,
                          blah2hip_hit_t *d_hits, uint32_t cap, uint32_t *d_count, void *stream)
{
  int rc;
  if ((rc = check_dev(h, d_hits, d_count, n_cpi)) || (rc = gocfar2d_check(ngd, ntd, n_rows_doppler, min_delay)) ||
      (rc = gocfar_check(h, pfa, kind)))
    return rc;
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  GoCfar2dArgs ga;
  Cfar2dArgs &a = ga.d;
  ga.kind = kind;
  if ((rc = gocfar_table(h, pfa, kind, ngd, ntd, n_rows_doppler, &a.alpha, st))) return rc;
  if ((rc = start_args(a, h, d_map, d_metrics, n_cpi, min_delay, min_doppler, d_hits, cap, d_count, st))) return rc;
  a.sat = nullptr;
  a.ngD = ngd; a.ntD = ntd; a.ngF = 0; a.ntF = n_rows_doppler;
  const size_t lds = g2_lds_bytes(ngd + ntd, n_rows_doppler);
  if (lds > 48 * 1024) LDSCFG(gocfar2d_kernel, g2_lds_bytes(C2T_MAX_HC, C2T_MAX_HR)); // once per (device, kernel): its largest use
  if ((rc = tic(h, BLAH2HIP_K_CFAR, st))) return rc;
  hipLaunchKernelGGL(gocfar2d_kernel, dim3((a.nDelay + G2_COLS - 1) / G2_COLS, (a.nD + G2_ROWS - 1) / G2_ROWS, n_cpi), dim3(256),
                     lds, st, ga);
  HIPCHK(hipGetLastError());
  return toc(h, BLAH2HIP_K_CFAR, st);
}

int blah2hip_gocfar2d_prepare(blah2hip_amb_t h, double pfa, uint32_t kind, int32_t ngd, int32_t ntd, int32_t n_rows_doppler)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  int rc;
  if ((rc = gocfar2d_check(ngd, ntd, n_rows_doppler)) || (rc = gocfar_check(h, pfa, kind))) return rc;
  HIPCHK(hipSetDevice(h->device));
  const double *d = nullptr;
  return gocfar_table(h, pfa, kind, ngd, ntd, n_rows_doppler, &d, nullptr, true);
}

int blah2hip_gocfar2d_process(blah2hip_amb_t h, uint32_t cpi, double pfa, uint32_t kind, int32_t ngd, int32_t ntd,
                              int32_t n_rows_doppler, int32_t min_delay, double min_doppler, double *delay, double *doppler,
                              double *snr, uint32_t cap, uint32_t *count)
{
  return process_one(h, cpi, delay, doppler, snr, cap, count, [&](const cf *m, const double *met) {
    return blah2hip_gocfar2d_dev(h, m, met, 1, pfa, kind, ngd, ntd, n_rows_doppler, min_delay, min_doppler, h->d_hits,
                                 h->hitCap, h->d_count, h->stream);
  });
}

// ------------------------------------------------- centroid / interpolate --
// Host arithmetic on a handful of detections (O(n^2) over tens of items).
int blah2hip_centroid(const double *delay, const double *doppler, const double *snr, uint32_t count,
                      uint16_t n_delay, uint16_t n_doppler, double resolution_doppler,
                      double *delay_out, double *doppler_out, double *snr_out, uint32_t *count_out)
{
  if (!count_out || (count && (!delay || !doppler || !snr || !delay_out || !doppler_out || !snr_out)))
    return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  uint32_t kept = 0;
  for (uint32_t i = 0; i < count; i++) {
    // Centroid.cpp:36-39: uint16_t limits -> (int)delay - n_delay wraps when negative
    const uint16_t lo = (uint16_t)((int)delay[i] - (int)n_delay);
    const uint16_t hi = (uint16_t)((int)delay[i] + (int)n_delay);
    const double flo = doppler[i] - (n_doppler * resolution_doppler);
    const double fhi = doppler[i] + (n_doppler * resolution_doppler);
    bool keep = true;
    for (uint32_t j = 0; j < count && keep; j++) {
      if (j == i) continue;
      if (delay[j] > lo && delay[j] < hi && doppler[j] > flo && doppler[j] < fhi && snr[i] < snr[j]) keep = false;
    }
    if (keep) {
      delay_out[kept] = delay[i];
      doppler_out[kept] = doppler[i];
      snr_out[kept] = snr[i];
      kept++;
    }
  }
  *count_out = kept;
  return BLAH2HIP_OK;
}

int blah2hip_interpolate(const double *delay, const double *doppler, const double *snr, uint32_t count,
                         const float *map, uint32_t n_doppler, uint32_t n_delay, const int32_t *delay_axis,
                         const double *doppler_axis, double noise_power, int do_delay, int do_doppler,
                         double *delay_out, double *doppler_out, double *snr_out, uint32_t *count_out)
{
  if (!count_out || !map || !delay_axis || !doppler_axis) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (count && (!delay || !doppler || !snr || !delay_out || !doppler_out || !snr_out))
    return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  // 10*log10|z| - noisePower of one map cell (Interpolate.cpp:50-52)
  auto cell = [&](int64_t row, int64_t col) -> double {
    if (row < 0 || row >= (int64_t)n_doppler || col < 0 || col >= (int64_t)n_delay)
      return std::nan(""); // the reference would index out of bounds here
    const float *z = map + 2 * ((size_t)row * n_delay + (size_t)col);
    return 10.0 * std::log10(std::hypot((double)z[0], (double)z[1])) - noise_power;
  };
  // Map::doppler_hz_to_bin: exact match, 0 on a miss (Map.cpp:102-113)
  auto row_of = [&](double hz) -> int64_t {
    for (uint32_t r = 0; r < n_doppler; r++)
      if (doppler_axis[r] == hz) return r;
    return 0;
  };
  uint32_t kept = 0;
  for (uint32_t i = 0; i < count; i++) {
    double intDelay = delay[i], intDoppler = doppler[i], intSnrDelay = snr[i];
    const double intSnrDoppler = snr[i]; // never updated in the reference (:80 writes intSnrDelay)
    const int64_t row = row_of(doppler[i]);
    const int64_t col = (int64_t)(delay[i] - delay_axis[0]);
    if (do_delay) {
      if (delay[i] == delay_axis[0] || delay[i] == delay_axis[n_delay - 1]) continue; // :46-49
      const double s0 = cell(row, col - 1), s1 = cell(row, col), s2 = cell(row, col + 1);
      if (s1 < s0 || s1 < s2) continue; // :54-58 dropped (peak lower than a neighbour)
      double off = (s0 - s2) / (2 * (s0 - (2 * s1) + s2));
      intSnrDelay = s1 - (((s0 - s2) * off) / 4);
      intDelay = delay[i] + off;
    }
    if (do_doppler) {
      if (doppler[i] == doppler_axis[0] || doppler[i] == doppler_axis[n_doppler - 1]) continue; // :67-70
      const double s0 = cell(row - 1, col), s1 = cell(row, col), s2 = cell(row + 1, col);
      if (s1 < s0 || s1 < s2) continue;
      double off = (s0 - s2) / (2 * (s0 - (2 * s1) + s2));
      intSnrDelay = s1 - (((s0 - s2) * off) / 4); // sic, :80
      intDoppler = doppler[i] + ((doppler_axis[1] - doppler_axis[0]) * off);
    }
    delay_out[kept] = intDelay;
    doppler_out[kept] = intDoppler;
    snr_out[kept] = std::max(std::max(intSnrDelay, intSnrDoppler), snr[i]); // :88
    kept++;
  }
  *count_out = kept;
  return BLAH2HIP_OK;
}

// ------------------------------------------- centroid / interpolate, device --
// Centroid::process and Interpolate::process on device-resident hit lists and maps (blah2.cpp:285-287 without the host):
// one launch of detect_finish_kernel, nothing in front of it.
int blah2hip_detect_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics, uint32_t n_cpi,
                        const blah2hip_hit_t *d_hits, uint32_t cap, const uint32_t *d_count,
                        uint16_t n_centroid_delay, uint16_t n_centroid_doppler, double resolution_doppler,
                        int do_centroid, int do_delay, int do_doppler,
                        blah2hip_det_t *d_out, uint32_t cap_out, uint32_t *d_count_out, void *stream)
{
  if (!h || !d_hits || !d_count || !d_out || !d_count_out) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (n_cpi == 0 || n_cpi > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "n_cpi outside [1, max_batch]");
  if (cap == 0) return fail(BLAH2HIP_ERR_INVALID, "cap is 0");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  DetectArgs a;
  a.map = d_map ? (const cf *)d_map : h->d_map;
  a.metrics = d_metrics ? d_metrics : h->d_metrics;
  a.doppler = h->d_doppler;
  a.hits = d_hits;
  a.count = d_count;
  a.out = d_out;
  a.countOut = d_count_out;
  a.appended = h->d_detWords;
  a.tickets = h->d_detWords + h->dims.max_batch;
  a.nD = (int32_t)h->dims.n_doppler_bins;
  a.nDelay = (int32_t)h->dims.n_delay_bins;
  a.delayMin = h->delayAxis[0];
  a.nCentroidDelay = (int32_t)n_centroid_delay;
  a.boxDoppler = n_centroid_doppler * resolution_doppler; // the expression of blah2hip_centroid (Centroid.cpp:38-39)
  a.cap = cap;
  a.capOut = cap_out;
  a.doCentroid = do_centroid != 0; a.doDelay = do_delay != 0; a.doDoppler = do_doppler != 0;
  // A list that fits one LDS tile: one workgroup per CPI, counter in LDS.  Longer lists: blocks of DET_BLOCK hits over G
  // workgroups per CPI, enough of them to fill the device with a lone CPI at its cap and no more than eight a CPI once
  // the batch alone fills it (a workgroup without a block of its CPI's list leaves after one load).
  const uint32_t blocks = (cap + DET_BLOCK - 1) / DET_BLOCK;
  const bool tiled = cap > (uint32_t)DET_TILE;
  const uint32_t G = tiled ? std::min(blocks, std::max(8u, (uint32_t)(4 * h->numCU) / n_cpi)) : 1u;
  if (tiled)
    hipLaunchKernelGGL(detect_finish_kernel<true>, dim3(G, n_cpi), dim3(DET_BLOCK), 0, st, a);
  else
    hipLaunchKernelGGL(detect_finish_kernel<false>, dim3(1, n_cpi), dim3(DET_BLOCK), 0, st, a);
  HIPCHK(hipGetLastError());
  h->detGridLast = (int)G;
  h->detTiledLast = tiled ? 1 : 0;
  return BLAH2HIP_OK;
}

} // extern "C"
