// Detection behind include/blah2hip.h: 1-D and 2-D CFAR (cell-averaging and ordered-statistic) with their threshold-table
// caches and summed-area table, Centroid and Interpolate on the host and on the device.  Host code; the kernels are
// cfar_kernels.hpp's, oscfar_kernels.hpp's and detect_kernels.hpp's.
#include "amb_handle.hpp"
#include "cfar_kernels.hpp"
#include "detect_kernels.hpp"
#include "oscfar_kernels.hpp"

#include <cmath>
#include <thread>

using namespace blah2;

namespace {

// CFAR threshold factors alpha[n] = n*(pfa^(-1/n) - 1), n = 1..maxN, evaluated with the
// same libm pow the reference calls (CfarDetector1D.cpp:76).  A small per-handle cache keyed by
// (pfa, maxN), least recently used first out (a caller that adapts pfa per CPI does not grow device
// memory): a hit only hands out the pointer; a miss allocates and uploads (blocking), which is
// refused while `st` is being captured into a graph -- *_prepare is the call for that.  A table *_prepare has handed out
// lives as long as the handle (`pin`): a graph captured afterwards has its address baked in, and no synchronisation
// at eviction time protects a later replay.  Only unpinned tables are evicted.
// The looks per cell are the handle's BLAH2HIP_OPT_CFAR_LOOKS at the time of the call and part of the key; one look is the
// expression above, more go through blah2hip_cfar_alpha's bisection (below).
constexpr size_t ALPHA_TABLES_MAX = 8;

// Pfa(t) of a cell that is the sum of L looks against the mean of n training cells of L looks each, threshold factor
// alpha = n t, m = n L: sum_{k < L} C(m + k - 1, k) t^k / (1 + t)^(m + k), term by term in the log domain (the first term
// alone underflows for large m, and lgamma's absolute error at m ~ 1e5 would show in the result)
double pfa_of_looks(double t, double m, uint32_t L)
{
  const double lt = std::log(t), l1 = std::log1p(t);
  double lg = -m * l1, s = std::exp(lg);
  for (uint32_t k = 1; k < L; k++) {
    lg += std::log((m + (double)k - 1.0) / (double)k) + lt - l1;
    s += std::exp(lg);
  }
  return s;
}

// alpha[n] for L > 1 looks: Pfa(t) = pfa by bisection in fp64 until the interval no longer splits; the upper end is returned
double alpha_of_looks(double pfa, uint32_t n, uint32_t L)
{
  const double m = (double)n * (double)L;
  double lo = 0.0, hi = 1.0;
  while (pfa_of_looks(hi, m, L) > pfa) hi *= 2.0;
  for (;;) {
    const double mid = 0.5 * (lo + hi);
    if (mid == lo || mid == hi) break;
    if (pfa_of_looks(mid, m, L) > pfa) lo = mid;
    else hi = mid;
  }
  return (double)n * hi;
}

int alpha_table(blah2hip_amb_s *h, double pfa, size_t maxN, const double **out, hipStream_t st = nullptr, bool pin = false)
{
  auto &T = h->alphaTables;
  const uint32_t looks = h->cfarLooks;
  for (size_t i = 0; i < T.size(); i++)
    if (T[i].pfa == pfa && T[i].looks == looks && T[i].n >= maxN) {
      blah2hip_amb_s::AlphaTable t = T[i];
      t.pinned = t.pinned || pin;
      T.erase(T.begin() + (long)i);
      T.push_back(t); // most recently used last
      *out = t.d;
      return BLAH2HIP_OK;
    }
  if (st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
      return fail(BLAH2HIP_ERR_INVALID, "threshold table of this (pfa, window) is not resident: call blah2hip_cfar1d_prepare / "
                                        "blah2hip_cfar2d_prepare before capturing the stream");
  }
  std::vector<double> alpha(maxN + 1);
  int rc;
  if ((rc = blah2hip_cfar_alpha(pfa, looks, (uint32_t)maxN, alpha.data()))) return rc;
  size_t unpinned = 0;
  for (const auto &e : T) unpinned += e.pinned ? 0 : 1;
  if (unpinned >= ALPHA_TABLES_MAX) {
    HIPCHK(hipDeviceSynchronize()); // the oldest unpinned table may still be read by enqueued work
    for (size_t i = 0; i < T.size(); i++)
      if (!T[i].pinned) {
        (void)hipFree(T[i].d);
        T.erase(T.begin() + (long)i);
        break;
      }
  }
  blah2hip_amb_s::AlphaTable t{pfa, looks, maxN, nullptr, pin};
  HIPCHK(hipMalloc(&t.d, (maxN + 1) * sizeof(double)));
  hipError_t e = hipMemcpy(t.d, alpha.data(), (maxN + 1) * sizeof(double), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(t.d); return fail(BLAH2HIP_ERR_HIP, std::string("alpha table upload: ") + hipGetErrorString(e)); }
  T.push_back(t);
  *out = t.d;
  return BLAH2HIP_OK;
}

// ---- ordered-statistic factors (blah2hip_oscfar_alpha; the formulas are in include/blah2hip.h) ----
uint32_t os_rank(uint64_t n, uint32_t permille)
{
  return (uint32_t)std::max<uint64_t>(1, (n * permille + 999) / 1000);
}

// one look: log Pfa(alpha; n, k) = -sum_{i<k} log1p(alpha / (n - i))
double os_logpfa1(double alpha, uint32_t n, uint32_t k)
{
  double s = 0.0;
  for (uint32_t i = 0; i < k; i++) s -= std::log1p(alpha / (double)(n - i));
  return s;
}

double os_alpha1(double pfa, uint32_t n, uint32_t k)
{
  const double lp = std::log(pfa);
  double lo = 0.0, hi = 1.0;
  while (os_logpfa1(hi, n, k) > lp) hi *= 2.0;
  for (;;) {
    const double mid = 0.5 * (lo + hi);
    if (mid == lo || mid == hi) break;
    if (os_logpfa1(mid, n, k) > lp) lo = mid;
    else hi = mid;
  }
  return hi;
}

// Q_L(t) = e^-t sum_{j<L} t^j / j!, summed outwards from its largest term (no overflow for any t and L); lf[j] = log j!
double os_q(double t, uint32_t L, const double *lf)
{
  if (!(t > 0.0)) return 1.0;
  const uint32_t js = (uint32_t)std::min<double>((double)(L - 1), std::floor(t));
  double s = 1.0, r = 1.0;
  for (uint32_t j = js; j + 1 < L; j++) { r *= t / (double)(j + 1); s += r; }
  r = 1.0;
  for (uint32_t j = js; j > 0; j--) { r *= (double)j / t; s += r; }
  return std::exp(-t + (double)js * std::log(t) - lf[js]) * s;
}

// P_L(x) = 1 - Q_L(x) from its own series e^-x x^L / L! (1 + x/(L+1) + x^2/((L+1)(L+2)) + ...), for x < L (no cancellation)
double os_p_series(double x, uint32_t L, const double *lf)
{
  if (!(x > 0.0)) return 0.0;
  double s = 1.0, r = 1.0;
  for (uint32_t m = 1; m < 100000; m++) {
    r *= x / (double)(L + m);
    s += r;
    if (r < 1e-17 * s) break;
  }
  return std::exp(-x + (double)L * std::log(x) - lf[L]) * s;
}

// log of the density of the k-th smallest of n Gamma(L) variables at x, without its constant n! / ((k-1)! (n-k)!)
double os_logdens(double x, uint32_t n, uint32_t k, uint32_t L, const double *lf)
{
  double P, Q;
  if (x < (double)L) { P = os_p_series(x, L, lf); Q = 1.0 - P; }
  else { Q = os_q(x, L, lf); P = 1.0 - Q; }
  double g = -x - lf[L - 1];
  if (L > 1) g += (double)(L - 1) * std::log(x);
  if (k > 1) g += (double)(k - 1) * std::log(P);
  if (n > k) g += (double)(n - k) * std::log(Q);
  return g;
}

constexpr int OS_COARSE = 4096, OS_FINE = 16384; // grid points of a scan for the integrand's support; Simpson intervals over it
constexpr double OS_CUT = 60.0;                  // the support: within e^-60 of the largest value

// Simpson nodes x and weights times density w for int f_(k)(x) Q_L(alpha x) dx at alpha >= alpha0: the interval on which
// f_(k)(x) Q_L(alpha0 x) is within e^-60 of its largest value (Q_L(alpha x) falls as alpha rises, so the interval holds
// the integrand of every larger alpha), found by two scans of OS_COARSE points, the second inside the first one's result
struct OsNodes { std::vector<double> x, w; };

void os_nodes(OsNodes &N, double alpha0, double logc, uint32_t n, uint32_t k, uint32_t L, const double *lf)
{
  auto G = [&](double x) {
    double g = os_logdens(x, n, k, L, lf);
    if (alpha0 > 0.0) g += std::log(os_q(alpha0 * x, L, lf));
    return g;
  };
  double a = 0.0, b = (double)L + 40.0 * std::sqrt((double)L) + 100.0;
  std::vector<double> g(OS_COARSE + 1);
  for (int pass = 0; pass < 2; pass++) {
    const double hc = (b - a) / OS_COARSE;
    int imax = 0;
    for (int i = 0; i <= OS_COARSE; i++) {
      g[i] = G(a + hc * i);
      if (g[i] > g[imax]) imax = i;
    }
    int ilo = imax, ihi = imax;
    while (ilo > 0 && !(g[ilo] < g[imax] - OS_CUT)) ilo--;
    while (ihi < OS_COARSE && !(g[ihi] < g[imax] - OS_CUT)) ihi++;
    b = a + hc * ihi;
    a = a + hc * ilo;
  }
  const double h = (b - a) / OS_FINE;
  N.x.resize(OS_FINE + 1);
  N.w.resize(OS_FINE + 1);
  for (int i = 0; i <= OS_FINE; i++) {
    N.x[i] = a + h * i;
    const double simpson = (i == 0 || i == OS_FINE) ? 1.0 : ((i & 1) ? 4.0 : 2.0);
    N.w[i] = simpson * (h / 3.0) * std::exp(logc + os_logdens(N.x[i], n, k, L, lf));
  }
}

double os_pfa_nodes(const OsNodes &N, double alpha, uint32_t L, const double *lf)
{
  double s = 0.0;
  for (int i = 0; i <= OS_FINE; i++) s += N.w[i] * os_q(alpha * N.x[i], L, lf);
  return s;
}

// alpha[n] for L > 1 looks: Pfa(alpha) = int f_(k)(x) Q_L(alpha x) dx = pfa.  The bracket [hi / 2, hi] by doubling, each
// trial on nodes of its own; then a bisection on the nodes of the bracket's lower end until the interval no longer
// splits.  The upper end is returned.
double os_alpha_looks(double pfa, uint32_t n, uint32_t k, uint32_t L, const double *lf)
{
  double logc = 0.0; // log( n! / ((k-1)! (n-k)!) ) = sum_{i<k} log(n - i) - log (k-1)!
  for (uint32_t i = 0; i < k; i++) logc += std::log((double)(n - i));
  for (uint32_t i = 2; i < k; i++) logc -= std::log((double)i);
  OsNodes N;
  double lo = 0.0, hi = 1.0;
  for (;;) {
    os_nodes(N, hi, logc, n, k, L, lf);
    if (!(os_pfa_nodes(N, hi, L, lf) > pfa) || hi > 1e300) break;
    lo = hi;
    hi *= 2.0;
  }
  os_nodes(N, lo, logc, n, k, L, lf);
  for (;;) {
    const double mid = 0.5 * (lo + hi);
    if (mid == lo || mid == hi) break;
    if (os_pfa_nodes(N, mid, L, lf) > pfa) lo = mid;
    else hi = mid;
  }
  return hi;
}

// The ordered-statistic detectors' tables: alpha[maxN + 1] doubles, then rank[maxN + 1] words, in one device allocation; a
// cache of their own keyed by (pfa, looks, rank, size) with the rules of alpha_table above (eight unpinned entries, least
// recently used first out, *_prepare pins), which it never touches.
constexpr size_t OS_TABLES_MAX = 8;

int os_table(blah2hip_amb_s *h, double pfa, uint32_t permille, size_t maxN, const double **alpha, const uint32_t **rank,
             hipStream_t st = nullptr, bool pin = false)
{
  auto &T = h->osTables;
  const uint32_t looks = h->cfarLooks;
  for (size_t i = 0; i < T.size(); i++)
    if (T[i].pfa == pfa && T[i].looks == looks && T[i].rank == permille && T[i].n == maxN) {
      blah2hip_amb_s::OsTable t = T[i];
      t.pinned = t.pinned || pin;
      T.erase(T.begin() + (long)i);
      T.push_back(t); // most recently used last
      *alpha = t.d;
      *rank = reinterpret_cast<const uint32_t *>(t.d + (maxN + 1));
      return BLAH2HIP_OK;
    }
  if (st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
      return fail(BLAH2HIP_ERR_INVALID, "ordered-statistic table of this (pfa, rank, window) is not resident: call "
                                        "blah2hip_oscfar1d_prepare / blah2hip_oscfar2d_prepare before capturing the stream");
  }
  const size_t bytes = (maxN + 1) * (sizeof(double) + sizeof(uint32_t));
  std::vector<double> host((bytes + sizeof(double) - 1) / sizeof(double));
  int rc;
  if ((rc = blah2hip_oscfar_alpha(pfa, looks, permille, (uint32_t)maxN, host.data(),
                                  reinterpret_cast<uint32_t *>(host.data() + (maxN + 1)))))
    return rc;
  size_t unpinned = 0;
  for (const auto &e : T) unpinned += e.pinned ? 0 : 1;
  if (unpinned >= OS_TABLES_MAX) {
    HIPCHK(hipDeviceSynchronize()); // the oldest unpinned table may still be read by enqueued work
    for (size_t i = 0; i < T.size(); i++)
      if (!T[i].pinned) {
        (void)hipFree(T[i].d);
        T.erase(T.begin() + (long)i);
        break;
      }
  }
  blah2hip_amb_s::OsTable t{pfa, looks, permille, maxN, nullptr, pin};
  HIPCHK(hipMalloc(&t.d, host.size() * sizeof(double)));
  hipError_t e = hipMemcpy(t.d, host.data(), bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(t.d); return fail(BLAH2HIP_ERR_HIP, std::string("ordered-statistic table upload: ") + hipGetErrorString(e)); }
  T.push_back(t);
  *alpha = t.d;
  *rank = reinterpret_cast<const uint32_t *>(t.d + (maxN + 1));
  return BLAH2HIP_OK;
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

} // namespace

extern "C" {

// ------------------------------------------------------------------- CFAR --
// Host arithmetic only.  One look: the reference's expression with the same libm pow, whatever pfa is.  More looks: a
// bisection per n of about 55 evaluations of `looks` terms each; long tables (a 2-D window at hundreds of looks) are cut
// into interleaved slices for up to eight threads -- every entry is computed on its own, so the slices do not change it.
int blah2hip_cfar_alpha(double pfa, uint32_t looks, uint32_t max_n, double *alpha)
{
  if (!alpha) return fail(BLAH2HIP_ERR_INVALID, "NULL table");
  if (looks == 0 || looks > BLAH2HIP_MAX_CFAR_LOOKS) return fail(BLAH2HIP_ERR_INVALID, "looks outside [1, BLAH2HIP_MAX_CFAR_LOOKS]");
  if (looks > 1 && !(pfa > 0.0 && pfa < 1.0)) return fail(BLAH2HIP_ERR_INVALID, "pfa outside (0, 1) with more than one look");
  alpha[0] = std::nan("");
  if (looks == 1) {
    for (size_t n = 1; n <= max_n; n++) alpha[n] = (double)n * (pow(pfa, -1.0 / (double)n) - 1);
    return BLAH2HIP_OK;
  }
  const uint64_t terms = (uint64_t)max_n * looks;
  const uint32_t nThreads = terms < 50000 ? 1u : std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
  auto slice = [=](uint32_t first) {
    for (uint64_t n = 1 + first; n <= max_n; n += nThreads) alpha[n] = alpha_of_looks(pfa, (uint32_t)n, looks);
  };
  std::vector<std::thread> pool;
  uint32_t started = 1;
  try {
    for (; started < nThreads; started++) pool.emplace_back(slice, started);
  } catch (const std::exception &) { // no thread to be had: the slices that are left run here
  }
  slice(0);
  for (uint32_t t = started; t < nThreads; t++) slice(t);
  for (auto &t : pool) t.join();
  return BLAH2HIP_OK;
}

int blah2hip_cfar1d_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics,
                        uint32_t n_cpi, double pfa, int32_t n_guard, int32_t n_train,
                        int32_t min_delay, double min_doppler, blah2hip_hit_t *d_hits, uint32_t cap,
                        uint32_t *d_count, void *stream)
{
  if (!h || !d_hits || !d_count) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (n_cpi == 0 || n_cpi > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "n_cpi outside [1, max_batch]");
  // CfarDetector1D's ctor parameters are int8_t (CfarDetector1D.h:46)
  if (n_guard < 0 || n_guard > 127 || n_train < 0 || n_train > 127 || min_delay < -128 || min_delay > 127)
    return fail(BLAH2HIP_ERR_INVALID, "nGuard/nTrain/minDelay outside int8 range");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const double *d_alpha = nullptr;
  int rc;
  if ((rc = alpha_table(h, pfa, (size_t)(2 * n_train), &d_alpha, st))) return rc;
  HIPCHK(hipMemsetAsync(d_count, 0, n_cpi * sizeof(uint32_t), st));
  CfarArgs a;
  a.map = d_map ? (const cf *)d_map : h->d_map;
  a.metrics = d_metrics ? d_metrics : h->d_metrics;
  a.doppler = h->d_doppler;
  a.alpha = d_alpha;
  a.hits = d_hits;
  a.count = d_count;
  a.nD = (int32_t)h->dims.n_doppler_bins;
  a.nDelay = (int32_t)h->dims.n_delay_bins;
  a.delayMin = h->delayMin;
  a.delayAxis = nullptr; // the engine's own axis: delayMin + j
  a.nGuard = n_guard; a.nTrain = n_train; a.minDelay = min_delay;
  a.minDoppler = min_doppler;
  a.cap = cap;
  if ((rc = tic(h, BLAH2HIP_K_CFAR, st))) return rc;
  {
    // the row as fp64 |z|^2 in LDS while it fits (150 KB: 19 200 delay bins), straight from L2 beyond
    const size_t rowBytes = (size_t)a.nDelay * sizeof(double);
    if (rowBytes <= 150 * 1024) {
      if (rowBytes > 48 * 1024) LDSCFG(cfar1d_kernel<true>, 150 * 1024); // the attribute is set once per (device, kernel): its largest use
      hipLaunchKernelGGL(cfar1d_kernel<true>, dim3(a.nD, n_cpi), dim3(256), rowBytes, st, a);
    } else {
      hipLaunchKernelGGL(cfar1d_kernel<false>, dim3(a.nD, n_cpi), dim3(256), 0, st, a);
    }
  }
  HIPCHK(hipGetLastError());
  if ((rc = toc(h, BLAH2HIP_K_CFAR, st))) return rc;
  return BLAH2HIP_OK;
}

int blah2hip_cfar1d_process(blah2hip_amb_t h, uint32_t cpi, double pfa, int32_t n_guard,
                            int32_t n_train, int32_t min_delay, double min_doppler, double *delay,
                            double *doppler, double *snr, uint32_t cap, uint32_t *count)
{
  if (!h || !count) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (cpi >= h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "cpi index out of range");
  HIPCHK(hipSetDevice(h->device));
  const size_t cells = (size_t)h->dims.n_doppler_bins * h->dims.n_delay_bins;
  int rc;
  if ((rc = ensure_hits(h, cells))) return rc;
  // run on a one-CPI view of the internal buffers
  const cf *m = h->d_map + cells * cpi;
  const double *met = h->d_metrics + 2 * cpi;
  rc = blah2hip_cfar1d_dev(h, m, met, 1, pfa, n_guard, n_train, min_delay, min_doppler, h->d_hits,
                           h->hitCap, h->d_count, h->stream);
  if (rc) return rc;
  return hits_to_host(h, delay, doppler, snr, cap, count);
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
  if (n_guard < 0 || n_guard > 127 || n_train < 0 || n_train > 127 || min_delay < -128 || min_delay > 127)
    return fail(BLAH2HIP_ERR_INVALID, "nGuard/nTrain/minDelay outside int8 range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(BLAH2HIP_ERR_NO_DEVICE, "no HIP device visible (the HIP path is the only path)");
  if (device < 0 || device >= ndev) return fail(BLAH2HIP_ERR_INVALID, "device index out of range");
  HIPCHK(hipSetDevice(device));
  const size_t cells = (size_t)n_doppler * n_delay;
  std::vector<double> alpha(2 * n_train + 1);
  alpha[0] = std::nan("");
  for (int n = 1; n <= 2 * n_train; n++) alpha[n] = n * (pow(pfa, -1.0 / n) - 1);
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
    const size_t rowBytes = (size_t)a.nDelay * sizeof(double);
    if (rowBytes <= 150 * 1024) {
      if (rowBytes > 48 * 1024) HIPCHK(blah2hip_ensure_lds_((const void *)cfar1d_kernel<true>, 150 * 1024));
      hipLaunchKernelGGL(cfar1d_kernel<true>, dim3(a.nD, 1), dim3(256), rowBytes, 0, a);
    } else {
      hipLaunchKernelGGL(cfar1d_kernel<false>, dim3(a.nD, 1), dim3(256), 0, 0, a);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(&n, pool + oCnt, sizeof(uint32_t), hipMemcpyDeviceToHost)); // synchronises with the null stream
    hits.resize(n);
    if (n) HIPCHK(hipMemcpy(hits.data(), pool + oHits, n * sizeof(blah2hip_hit_t), hipMemcpyDeviceToHost));
    return BLAH2HIP_OK;
  };
  const int rc = run();
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
  if (!h || !d_hits || !d_count) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (n_cpi == 0 || n_cpi > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "n_cpi outside [1, max_batch]");
  for (int32_t v : {ngd, ntd, ngf, ntf})
    if (v < 0 || v > 127) return fail(BLAH2HIP_ERR_INVALID, "guard/train sizes outside [0, 127]");
  if (min_delay < -128 || min_delay > 127) return fail(BLAH2HIP_ERR_INVALID, "minDelay outside int8 range");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  const int nD = (int)h->dims.n_doppler_bins, nC = (int)h->dims.n_delay_bins;
  int rc;
  if (h->cfar2dForce == BLAH2HIP_CFAR2D_TILE && !cfar2d_use_tile(h, ngd, ntd, ngf, ntf))
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "2-D window beyond the tile kernel's halo (nGf + nTf <= 24, nGd + nTd <= 40)");
  if (h->cfar2dForce == BLAH2HIP_CFAR2D_STREAM && !cfar2d_stream_shape(ngd, ntd, ngf, ntf))
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "the stream kernel is not instantiated for this 2-D window (C2S_SHAPES in cfar_kernels.hpp)");
  {
    int lo, hi; // the handle's Doppler axis is monotonic (Ambiguity.cpp:60-66), so this cannot fail today; a forced kernel never runs another one
    if (h->cfar2dForce == BLAH2HIP_CFAR2D_STREAM && !cfar2d_dead_rows(h, min_doppler, &lo, &hi))
      return fail(BLAH2HIP_ERR_UNSUPPORTED, "the stream kernel needs the rows below minDoppler to be one interval of the Doppler axis");
  }
  if (!cfar2d_use_stream(h, ngd, ntd, ngf, ntf, min_doppler) && !cfar2d_use_tile(h, ngd, ntd, ngf, ntf) && (rc = ensure_sat(h))) return rc; // no-op once allocated
  const double *d_alpha = nullptr;
  if ((rc = alpha_table(h, pfa, (size_t)(2 * (ngd + ntd) + 1) * (2 * (ngf + ntf) + 1), &d_alpha, st))) return rc;
  HIPCHK(hipMemsetAsync(d_count, 0, n_cpi * sizeof(uint32_t), st));
  Cfar2dArgs a;
  a.map = d_map ? (const cf *)d_map : h->d_map;
  a.metrics = d_metrics ? d_metrics : h->d_metrics;
  a.doppler = h->d_doppler;
  a.alpha = d_alpha;
  a.sat = h->d_sat;
  a.hits = d_hits;
  a.count = d_count;
  a.nD = nD; a.nDelay = nC; a.delayMin = h->delayMin;
  a.ngD = ngd; a.ntD = ntd; a.ngF = ngf; a.ntF = ntf; a.minDelay = min_delay;
  a.minDoppler = min_doppler;
  a.cap = cap;
  if (cfar2d_use_stream(h, ngd, ntd, ngf, ntf, min_doppler)) {
    if ((rc = tic(h, BLAH2HIP_K_CFAR, st))) return rc;
    cfar2d_stream_launch(h, a, n_cpi, st);
    HIPCHK(hipGetLastError());
    if ((rc = toc(h, BLAH2HIP_K_CFAR, st))) return rc;
    return BLAH2HIP_OK;
  }
  if (cfar2d_use_tile(h, ngd, ntd, ngf, ntf)) {
    Cfar2dTileArgs ta;
    ta.d = a;
    ta.nCpi = (int32_t)n_cpi;
    ta.rowsOut = C2T_ROWS - 2 * (ngf + ntf);
    ta.tilesX = (nC + C2T_COLS - 1) / C2T_COLS;
    ta.tilesY = (nD + ta.rowsOut - 1) / ta.rowsOut;
    const int hC = ngd + ntd;
    // the whole threshold table in LDS when it fits beside the tile (the default 17 x 9 window: 154 entries)
    const int64_t tableN = (int64_t)(2 * (ngd + ntd) + 1) * (2 * (ngf + ntf) + 1) + 1;
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
    if ((rc = toc(h, BLAH2HIP_K_CFAR, st))) return rc;
    return BLAH2HIP_OK;
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
  if ((rc = toc(h, BLAH2HIP_K_CFAR, st))) return rc;
  return BLAH2HIP_OK;
}

int blah2hip_cfar1d_prepare(blah2hip_amb_t h, double pfa, int32_t n_train)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (n_train < 0 || n_train > 127) return fail(BLAH2HIP_ERR_INVALID, "nTrain outside int8 range");
  HIPCHK(hipSetDevice(h->device));
  const double *d = nullptr;
  return alpha_table(h, pfa, (size_t)(2 * n_train), &d, nullptr, true);
}

int blah2hip_cfar2d_prepare(blah2hip_amb_t h, double pfa, int32_t ngd, int32_t ntd, int32_t ngf, int32_t ntf)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  for (int32_t v : {ngd, ntd, ngf, ntf})
    if (v < 0 || v > 127) return fail(BLAH2HIP_ERR_INVALID, "guard/train sizes outside [0, 127]");
  HIPCHK(hipSetDevice(h->device));
  int rc;
  if (h->cfar2dForce == BLAH2HIP_CFAR2D_TILE && !cfar2d_use_tile(h, ngd, ntd, ngf, ntf))
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "2-D window beyond the tile kernel's halo (nGf + nTf <= 24, nGd + nTd <= 40)");
  if (h->cfar2dForce == BLAH2HIP_CFAR2D_STREAM && !cfar2d_stream_shape(ngd, ntd, ngf, ntf))
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "the stream kernel is not instantiated for this 2-D window (C2S_SHAPES in cfar_kernels.hpp)");
  if (!cfar2d_use_stream(h, ngd, ntd, ngf, ntf, 0.0) && !cfar2d_use_tile(h, ngd, ntd, ngf, ntf) && (rc = ensure_sat(h))) return rc;
  const double *d = nullptr;
  return alpha_table(h, pfa, (size_t)(2 * (ngd + ntd) + 1) * (2 * (ngf + ntf) + 1), &d, nullptr, true);
}

int blah2hip_cfar2d_process(blah2hip_amb_t h, uint32_t cpi, double pfa, int32_t ngd, int32_t ntd,
                            int32_t ngf, int32_t ntf, int32_t min_delay, double min_doppler, double *delay,
                            double *doppler, double *snr, uint32_t cap, uint32_t *count)
{
  if (!h || !count) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (cpi >= h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "cpi index out of range");
  HIPCHK(hipSetDevice(h->device));
  const size_t cells = (size_t)h->dims.n_doppler_bins * h->dims.n_delay_bins;
  int rc;
  if ((rc = ensure_hits(h, cells))) return rc;
  rc = blah2hip_cfar2d_dev(h, h->d_map + cells * cpi, h->d_metrics + 2 * cpi, 1, pfa, ngd, ntd, ngf, ntf,
                           min_delay, min_doppler, h->d_hits, h->hitCap, h->d_count, h->stream);
  if (rc) return rc;
  return hits_to_host(h, delay, doppler, snr, cap, count);
}

// ------------------------------------------------------ ordered statistic --
// Host arithmetic only.  One look: a bisection per n on the logarithm of the product formula.  More looks: per n the nodes
// and weights of the quadrature once, then a bisection of about 60 sums over them; the entries are computed on their own,
// in interleaved slices for up to eight threads when the table is long.
int blah2hip_oscfar_alpha(double pfa, uint32_t looks, uint32_t rank_permille, uint32_t max_n, double *alpha, uint32_t *rank)
{
  if (!alpha) return fail(BLAH2HIP_ERR_INVALID, "NULL table");
  if (looks == 0 || looks > BLAH2HIP_MAX_CFAR_LOOKS) return fail(BLAH2HIP_ERR_INVALID, "looks outside [1, BLAH2HIP_MAX_CFAR_LOOKS]");
  if (rank_permille < 1 || rank_permille > 1000) return fail(BLAH2HIP_ERR_INVALID, "rank_permille outside [1, 1000]");
  if (!(pfa > 0.0 && pfa < 1.0)) return fail(BLAH2HIP_ERR_INVALID, "pfa outside (0, 1)");
  alpha[0] = std::nan("");
  if (rank) rank[0] = 0;
  for (uint64_t n = 1; n <= max_n; n++)
    if (rank) rank[n] = os_rank(n, rank_permille);
  std::vector<double> lf(looks + 1, 0.0); // log j!
  for (uint32_t j = 2; j <= looks; j++) lf[j] = lf[j - 1] + std::log((double)j);
  // (one look costs about 60 k log1p per entry: only a long 2-D table is worth the threads)
  const bool threads = looks == 1 ? max_n >= 512 : max_n >= 16;
  const uint32_t nThreads = !threads ? 1u : std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
  auto slice = [=, &lf](uint32_t first) {
    for (uint64_t n = 1 + first; n <= max_n; n += nThreads) {
      const uint32_t k = os_rank(n, rank_permille);
      alpha[n] = looks == 1 ? os_alpha1(pfa, (uint32_t)n, k) : os_alpha_looks(pfa, (uint32_t)n, k, looks, lf.data());
    }
  };
  std::vector<std::thread> pool;
  uint32_t started = 1;
  try {
    for (; started < nThreads; started++) pool.emplace_back(slice, started);
  } catch (const std::exception &) { // no thread to be had: the slices that are left run here
  }
  slice(0);
  for (uint32_t t = started; t < nThreads; t++) slice(t);
  for (auto &t : pool) t.join();
  return BLAH2HIP_OK;
}

int blah2hip_oscfar1d_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics, uint32_t n_cpi, double pfa,
                          uint32_t rank_permille, int32_t n_guard, int32_t n_train, int32_t min_delay, double min_doppler,
                          blah2hip_hit_t *d_hits, uint32_t cap, uint32_t *d_count, void *stream)
{
  if (!h || !d_hits || !d_count) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (n_cpi == 0 || n_cpi > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "n_cpi outside [1, max_batch]");
  if (n_guard < 0 || n_guard > 127 || n_train < 0 || n_train > 127 || min_delay < -128 || min_delay > 127)
    return fail(BLAH2HIP_ERR_INVALID, "nGuard/nTrain/minDelay outside int8 range");
  int rc;
  if ((rc = os_check_rank(rank_permille))) return rc;
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  OsCfarArgs oa;
  CfarArgs &a = oa.c;
  if ((rc = os_table(h, pfa, rank_permille, (size_t)(2 * n_train), &a.alpha, &oa.rank, st))) return rc;
  HIPCHK(hipMemsetAsync(d_count, 0, n_cpi * sizeof(uint32_t), st));
  a.map = d_map ? (const cf *)d_map : h->d_map;
  a.metrics = d_metrics ? d_metrics : h->d_metrics;
  a.doppler = h->d_doppler;
  a.hits = d_hits;
  a.count = d_count;
  a.nD = (int32_t)h->dims.n_doppler_bins;
  a.nDelay = (int32_t)h->dims.n_delay_bins;
  a.delayMin = h->delayMin;
  a.delayAxis = nullptr; // the engine's own axis: delayMin + j
  a.nGuard = n_guard; a.nTrain = n_train; a.minDelay = min_delay;
  a.minDoppler = min_doppler;
  a.cap = cap;
  if ((rc = tic(h, BLAH2HIP_K_CFAR, st))) return rc;
  {
    // the row as fp64 |z|^2 in LDS while it fits (150 KB: 19 200 delay bins), straight from L2 beyond: cfar1d_kernel's limit
    const size_t rowBytes = (size_t)a.nDelay * sizeof(double);
    if (rowBytes <= 150 * 1024) {
      if (rowBytes > 48 * 1024) LDSCFG(oscfar1d_kernel<true>, 150 * 1024);
      hipLaunchKernelGGL(oscfar1d_kernel<true>, dim3(a.nD, n_cpi), dim3(256), rowBytes, st, oa);
    } else {
      hipLaunchKernelGGL(oscfar1d_kernel<false>, dim3(a.nD, n_cpi), dim3(256), 0, st, oa);
    }
  }
  HIPCHK(hipGetLastError());
  if ((rc = toc(h, BLAH2HIP_K_CFAR, st))) return rc;
  return BLAH2HIP_OK;
}

int blah2hip_oscfar1d_prepare(blah2hip_amb_t h, double pfa, uint32_t rank_permille, int32_t n_train)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  if (n_train < 0 || n_train > 127) return fail(BLAH2HIP_ERR_INVALID, "nTrain outside int8 range");
  int rc;
  if ((rc = os_check_rank(rank_permille))) return rc;
  HIPCHK(hipSetDevice(h->device));
  const double *d = nullptr;
  const uint32_t *r = nullptr;
  return os_table(h, pfa, rank_permille, (size_t)(2 * n_train), &d, &r, nullptr, true);
}

int blah2hip_oscfar1d_process(blah2hip_amb_t h, uint32_t cpi, double pfa, uint32_t rank_permille, int32_t n_guard,
                              int32_t n_train, int32_t min_delay, double min_doppler, double *delay, double *doppler,
                              double *snr, uint32_t cap, uint32_t *count)
{
  if (!h || !count) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (cpi >= h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "cpi index out of range");
  HIPCHK(hipSetDevice(h->device));
  const size_t cells = (size_t)h->dims.n_doppler_bins * h->dims.n_delay_bins;
  int rc;
  if ((rc = ensure_hits(h, cells))) return rc;
  rc = blah2hip_oscfar1d_dev(h, h->d_map + cells * cpi, h->d_metrics + 2 * cpi, 1, pfa, rank_permille, n_guard, n_train,
                             min_delay, min_doppler, h->d_hits, h->hitCap, h->d_count, h->stream);
  if (rc) return rc;
  return hits_to_host(h, delay, doppler, snr, cap, count);
}

static int os2d_check(blah2hip_amb_t h, uint32_t rank_permille, int32_t ngd, int32_t ntd, int32_t ngf, int32_t ntf)
{
  if (!h) return fail(BLAH2HIP_ERR_INVALID, "NULL handle");
  for (int32_t v : {ngd, ntd, ngf, ntf})
    if (v < 0 || v > 127) return fail(BLAH2HIP_ERR_INVALID, "guard/train sizes outside [0, 127]");
  int rc;
  if ((rc = os_check_rank(rank_permille))) return rc;
  if (ngf + ntf > C2T_MAX_HR || ngd + ntd > C2T_MAX_HC)
    return fail(BLAH2HIP_ERR_UNSUPPORTED, "ordered-statistic 2-D window beyond the tile's halo (nGf + nTf <= 24, nGd + nTd <= 40): "
                                          "a rank has no summed-area form");
  return BLAH2HIP_OK;
}

int blah2hip_oscfar2d_dev(blah2hip_amb_t h, const void *d_map, const double *d_metrics, uint32_t n_cpi, double pfa,
                          uint32_t rank_permille, int32_t ngd, int32_t ntd, int32_t ngf, int32_t ntf, int32_t min_delay,
                          double min_doppler, blah2hip_hit_t *d_hits, uint32_t cap, uint32_t *d_count, void *stream)
{
  if (!h || !d_hits || !d_count) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (n_cpi == 0 || n_cpi > h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "n_cpi outside [1, max_batch]");
  if (min_delay < -128 || min_delay > 127) return fail(BLAH2HIP_ERR_INVALID, "minDelay outside int8 range");
  int rc;
  if ((rc = os2d_check(h, rank_permille, ngd, ntd, ngf, ntf))) return rc;
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  OsCfar2dArgs oa;
  Cfar2dArgs &a = oa.d;
  if ((rc = os_table(h, pfa, rank_permille, (size_t)(2 * (ngd + ntd) + 1) * (2 * (ngf + ntf) + 1), &a.alpha, &oa.rank, st))) return rc;
  HIPCHK(hipMemsetAsync(d_count, 0, n_cpi * sizeof(uint32_t), st));
  a.map = d_map ? (const cf *)d_map : h->d_map;
  a.metrics = d_metrics ? d_metrics : h->d_metrics;
  a.doppler = h->d_doppler;
  a.sat = nullptr;
  a.hits = d_hits;
  a.count = d_count;
  a.nD = (int32_t)h->dims.n_doppler_bins; a.nDelay = (int32_t)h->dims.n_delay_bins; a.delayMin = h->delayMin;
  a.ngD = ngd; a.ntD = ntd; a.ngF = ngf; a.ntF = ntf; a.minDelay = min_delay;
  a.minDoppler = min_doppler;
  a.cap = cap;
  const size_t lds = o2_lds_bytes(ngd + ntd, ngf + ntf);
  if (lds > 48 * 1024) LDSCFG(oscfar2d_kernel, o2_lds_bytes(C2T_MAX_HC, C2T_MAX_HR)); // once per (device, kernel): its largest use
  if ((rc = tic(h, BLAH2HIP_K_CFAR, st))) return rc;
  hipLaunchKernelGGL(oscfar2d_kernel, dim3((a.nDelay + O2_COLS - 1) / O2_COLS, (a.nD + O2_ROWS - 1) / O2_ROWS, n_cpi), dim3(256),
                     lds, st, oa);
  HIPCHK(hipGetLastError());
  if ((rc = toc(h, BLAH2HIP_K_CFAR, st))) return rc;
  return BLAH2HIP_OK;
}

int blah2hip_oscfar2d_prepare(blah2hip_amb_t h, double pfa, uint32_t rank_permille, int32_t ngd, int32_t ntd, int32_t ngf,
                              int32_t ntf)
{
  int rc;
  if ((rc = os2d_check(h, rank_permille, ngd, ntd, ngf, ntf))) return rc;
  HIPCHK(hipSetDevice(h->device));
  const double *d = nullptr;
  const uint32_t *r = nullptr;
  return os_table(h, pfa, rank_permille, (size_t)(2 * (ngd + ntd) + 1) * (2 * (ngf + ntf) + 1), &d, &r, nullptr, true);
}

int blah2hip_oscfar2d_process(blah2hip_amb_t h, uint32_t cpi, double pfa, uint32_t rank_permille, int32_t ngd, int32_t ntd,
                              int32_t ngf, int32_t ntf, int32_t min_delay, double min_doppler, double *delay,
                              double *doppler, double *snr, uint32_t cap, uint32_t *count)
{
  if (!h || !count) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  if (cpi >= h->dims.max_batch) return fail(BLAH2HIP_ERR_INVALID, "cpi index out of range");
  HIPCHK(hipSetDevice(h->device));
  const size_t cells = (size_t)h->dims.n_doppler_bins * h->dims.n_delay_bins;
  int rc;
  if ((rc = ensure_hits(h, cells))) return rc;
  rc = blah2hip_oscfar2d_dev(h, h->d_map + cells * cpi, h->d_metrics + 2 * cpi, 1, pfa, rank_permille, ngd, ntd, ngf, ntf,
                             min_delay, min_doppler, h->d_hits, h->hitCap, h->d_count, h->stream);
  if (rc) return rc;
  return hits_to_host(h, delay, doppler, snr, cap, count);
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
