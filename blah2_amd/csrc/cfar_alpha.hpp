// The detectors' threshold arithmetic behind blah2hip_cfar_alpha, blah2hip_oscfar_alpha, blah2hip_cmap_alpha and
// blah2hip_gocfar_alpha (detect.hip validates and calls cfar_alpha_fill / oscfar_alpha_fill / cmap_alpha_fill /
// goso_alpha_fill).  Host only, C++17 and libm, no HIP: tests/host/emulate_cfar_alpha.cpp compiles it
// on its own.  The formulas are in include/blah2hip.h.  Everything here has internal linkage (the unnamed namespace): the
// library exports none of it, and nothing the compiler emits out of line -- the thread objects of run_slices included --
// can be interposed.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <exception>
#include <thread>
#include <vector>

namespace blah2 {
namespace {

// The upper end of [lo, hi] once it no longer splits in fp64; above(mid): the function is still above its target at mid
// (it falls as its argument rises).  The callers bracket first.
template <class Above>
inline double bisect_upper(double lo, double hi, Above above)
{
  for (;;) {
    const double mid = 0.5 * (lo + hi);
    if (mid == lo || mid == hi) return hi;
    if (above(mid)) lo = mid;
    else hi = mid;
  }
}

// slice(0) .. slice(nThreads - 1), all but the first on threads of their own; the ones no thread could be started for run
// on the caller.  The slices are interleaved (entry n belongs to slice (n - 1) % nThreads) and every entry is computed on
// its own, so the cut does not change a table.
inline uint32_t table_threads() { return std::min(8u, std::max(1u, std::thread::hardware_concurrency())); }

template <class Slice>
inline void run_slices(uint32_t nThreads, Slice slice)
{
  std::vector<std::thread> pool;
  uint32_t started = 1;
  try {
    for (; started < nThreads; started++) pool.emplace_back(slice, started);
  } catch (const std::exception &) { // no thread to be had: the slices that are left run here
  }
  slice(0);
  for (uint32_t t = started; t < nThreads; t++) slice(t);
  for (auto &t : pool) t.join();
}

// ---- cell averaging ----
// Pfa(t) of a cell that is the sum of L looks against the mean of n training cells of L looks each, threshold factor
// alpha = n t, m = n L: sum_{k < L} C(m + k - 1, k) t^k / (1 + t)^(m + k), term by term in the log domain (the first term
// alone underflows for large m, and lgamma's absolute error at m ~ 1e5 would show in the result)
inline double pfa_of_looks(double t, double m, uint32_t L)
{
  const double lt = std::log(t), l1 = std::log1p(t);
  double lg = -m * l1, s = std::exp(lg);
  for (uint32_t k = 1; k < L; k++) {
    lg += std::log((m + (double)k - 1.0) / (double)k) + lt - l1;
    s += std::exp(lg);
  }
  return s;
}

// alpha[n] for L > 1 looks: Pfa(t) = pfa by bisection in fp64
inline double alpha_of_looks(double pfa, uint32_t n, uint32_t L)
{
  const double m = (double)n * (double)L;
  double hi = 1.0;
  while (pfa_of_looks(hi, m, L) > pfa) hi *= 2.0;
  return (double)n * bisect_upper(0.0, hi, [&](double t) { return pfa_of_looks(t, m, L) > pfa; });
}

// blah2hip_cfar_alpha past its checks.  One look: alpha[n] = n (pfa^(-1/n) - 1), the reference's expression with the same
// libm pow (CfarDetector1D.cpp:76), whatever pfa is.  More looks: a bisection per n of about 55 evaluations of `looks` terms
// each; long tables (a 2-D window at hundreds of looks) are cut into slices for up to eight threads.
inline void cfar_alpha_fill(double pfa, uint32_t looks, uint32_t max_n, double *alpha)
{
  alpha[0] = std::nan("");
  if (looks == 1) {
    for (size_t n = 1; n <= max_n; n++) alpha[n] = (double)n * (pow(pfa, -1.0 / (double)n) - 1);
    return;
  }
  const uint64_t terms = (uint64_t)max_n * looks;
  const uint32_t nThreads = terms < 50000 ? 1u : table_threads();
  run_slices(nThreads, [=](uint32_t first) {
    for (uint64_t n = 1 + first; n <= max_n; n += nThreads) alpha[n] = alpha_of_looks(pfa, (uint32_t)n, looks);
  });
}

// ---- ordered statistic ----
inline uint32_t os_rank(uint64_t n, uint32_t permille)
{
  return (uint32_t)std::max<uint64_t>(1, (n * permille + 999) / 1000);
}

// one look: log Pfa(alpha; n, k) = -sum_{i<k} log1p(alpha / (n - i))
inline double os_logpfa1(double alpha, uint32_t n, uint32_t k)
{
  double s = 0.0;
  for (uint32_t i = 0; i < k; i++) s -= std::log1p(alpha / (double)(n - i));
  return s;
}

inline double os_alpha1(double pfa, uint32_t n, uint32_t k)
{
  const double lp = std::log(pfa);
  double hi = 1.0;
  while (os_logpfa1(hi, n, k) > lp) hi *= 2.0;
  return bisect_upper(0.0, hi, [&](double alpha) { return os_logpfa1(alpha, n, k) > lp; });
}

// Q_L(t) = e^-t sum_{j<L} t^j / j!, summed outwards from its largest term (no overflow for any t and L); lf[j] = log j!
inline double os_q(double t, uint32_t L, const double *lf)
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
inline double os_p_series(double x, uint32_t L, const double *lf)
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
inline double os_logdens(double x, uint32_t n, uint32_t k, uint32_t L, const double *lf)
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

inline void os_nodes(OsNodes &N, double alpha0, double logc, uint32_t n, uint32_t k, uint32_t L, const double *lf)
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

inline double os_pfa_nodes(const OsNodes &N, double alpha, uint32_t L, const double *lf)
{
  double s = 0.0;
  for (int i = 0; i <= OS_FINE; i++) s += N.w[i] * os_q(alpha * N.x[i], L, lf);
  return s;
}

// alpha[n] for L > 1 looks: Pfa(alpha) = int f_(k)(x) Q_L(alpha x) dx = pfa.  The bracket [hi / 2, hi] by doubling, each
// trial on nodes of its own; then a bisection on the nodes of the bracket's lower end.
inline double os_alpha_looks(double pfa, uint32_t n, uint32_t k, uint32_t L, const double *lf)
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
  return bisect_upper(lo, hi, [&](double alpha) { return os_pfa_nodes(N, alpha, L, lf) > pfa; });
}

// blah2hip_oscfar_alpha past its checks (rank may be NULL).  One look: a bisection per n on the logarithm of the product
// formula, about 60 k log1p per entry, so only a long 2-D table is worth the threads.  More looks: per n the nodes and
// weights of the quadrature once, then a bisection of about 60 sums over them.
inline void oscfar_alpha_fill(double pfa, uint32_t looks, uint32_t rank_permille, uint32_t max_n, double *alpha, uint32_t *rank)
{
  alpha[0] = std::nan("");
  if (rank) rank[0] = 0;
  for (uint64_t n = 1; n <= max_n; n++)
    if (rank) rank[n] = os_rank(n, rank_permille);
  std::vector<double> lf(looks + 1, 0.0); // log j!
  for (uint32_t j = 2; j <= looks; j++) lf[j] = lf[j - 1] + std::log((double)j);
  const bool threads = looks == 1 ? max_n >= 512 : max_n >= 16;
  const uint32_t nThreads = !threads ? 1u : table_threads();
  run_slices(nThreads, [=, &lf](uint32_t first) {
    for (uint64_t n = 1 + first; n <= max_n; n += nThreads) {
      const uint32_t k = os_rank(n, rank_permille);
      alpha[n] = looks == 1 ? os_alpha1(pfa, (uint32_t)n, k) : os_alpha_looks(pfa, (uint32_t)n, k, looks, lf.data());
    }
  });
}

// ---- clutter map ----
// log Pfa(alpha) of a cell against alpha b at age a > T, b the map's average of memory T (include/blah2hip.h):
// -sum_i log1p(alpha c_i) over the weights w (1 - w)^m, m = 0 .. a - T - 1, newest first, then T times (1 - w)^(a - T) / T,
// w = 1 / T; the powers by repeated multiplication, the sum in this order (process.py: clutter_map_alpha does the same
// operations)
inline double cmap_logpfa(double alpha, uint32_t a, uint32_t T)
{
  const double w = 1.0 / (double)T, q = 1.0 - w;
  double g = 1.0, s = 0.0;
  for (uint32_t m = 0; m < a - T; m++) {
    s -= std::log1p(alpha * (w * g));
    g *= q;
  }
  return s - (double)T * std::log1p(alpha * (g / (double)T));
}

// blah2hip_cmap_alpha past its checks.  a <= T: the mean of a values, a (pfa^(-1/a) - 1) as cfar_alpha_fill has it.
// T < a <= 16 T: a bisection of about 60 evaluations of a - T + 1 terms each; entries beyond 16 T repeat that one.
inline void cmap_alpha_fill(double pfa, uint32_t T, uint32_t max_age, double *alpha)
{
  alpha[0] = std::nan("");
  const double lp = std::log(pfa);
  const uint32_t last = std::min<uint64_t>(max_age, 16ull * T);
  for (uint32_t a = 1; a <= std::min(last, T); a++) alpha[a] = (double)a * (pow(pfa, -1.0 / (double)a) - 1);
  const uint64_t terms = last > T ? (uint64_t)(last - T) * (last - T) / 2 : 0;
  const uint32_t nThreads = terms < 50000 ? 1u : table_threads();
  run_slices(nThreads, [=](uint32_t first) {
    for (uint64_t a = (uint64_t)T + 1 + first; a <= last; a += nThreads) {
      double hi = 1.0;
      while (cmap_logpfa(hi, (uint32_t)a, T) > lp) hi *= 2.0;
      alpha[a] = bisect_upper(0.0, hi, [&](double x) { return cmap_logpfa(x, (uint32_t)a, T) > lp; });
    }
  });
  for (uint64_t a = (uint64_t)last + 1; a <= max_age; a++) alpha[a] = alpha[last];
}

// ---- greatest-of / smallest-of ----
// One look, halves of a and b training cells (include/blah2hip.h).  T(alpha; a, b) = E[e^(-alpha U); U < V] for the half
// means U = Gamma(a) / a, V = Gamma(b) / b:  sum_{j<b} C(a-1+j, j) (b/a)^j s^-(a+j),  s = 1 + (alpha + b) / a, term by term in
// the log domain like pfa_of_looks (at the halo limits the first terms underflow and the sum has 1960 of them).
inline double goso_t(double alpha, uint32_t a, uint32_t b)
{
  const double da = (double)a, db = (double)b;
  const double ls = std::log(1.0 + (alpha + db) / da), lr = std::log(db / da) - ls;
  double lg = -da * ls, s = std::exp(lg);
  for (uint32_t j = 1; j < b; j++) {
    lg += std::log((da - 1.0 + (double)j) / (double)j) + lr;
    s += std::exp(lg);
  }
  return s;
}

// E[e^(-alpha U); U > V]: the same series from j = b on.  The whole series sums to (1 + alpha/a)^-a, and that minus goso_t is
// the textbook form of this quantity; with uneven halves and a small pfa the two are equal to eight digits and more (a = 1,
// b = 3, pfa 1e-8: 3e-3 each), so the tail is summed instead: positive terms that fall from the first one on (the ratio is
// below (a + b - 1) / (a + b + alpha)), until what is left is below 1e-17 of the sum.
inline double goso_tail(double alpha, uint32_t a, uint32_t b)
{
  const double da = (double)a, db = (double)b, sv = 1.0 + (alpha + db) / da;
  const double ls = std::log(sv), lr = std::log(db / da) - ls, q = (db / da) / sv;
  double lg = -da * ls;
  for (uint32_t j = 1; j <= b; j++) lg += std::log((da - 1.0 + (double)j) / (double)j) + lr;
  double s = std::exp(lg);
  for (uint32_t j = b + 1; j < b + 100000000u; j++) {
    const double f = (da - 1.0 + (double)j) / (double)j;
    lg += std::log(f) + lr;
    const double t = std::exp(lg), r = f * q; // r: no later ratio is larger
    s += t;
    if (!(t * r > (1.0 - r) * 1e-17 * s)) break;
  }
  return s;
}

constexpr uint32_t GOSO_GO = 1, GOSO_SO = 2; // BLAH2HIP_CFAR_GO, BLAH2HIP_CFAR_SO

// Pfa(alpha) of the pair of thresholds alpha mu_A, alpha mu_B: smallest-of  T(a, b) + T(b, a);  greatest-of the two tails,
// which is (1 + alpha/a)^-a + (1 + alpha/b)^-b minus the former.  The halves in ascending size, so that (a, b) and (b, a)
// give the same bits.
inline double goso_pfa(double alpha, uint32_t kind, uint32_t a, uint32_t b)
{
  if (a > b) std::swap(a, b);
  if (kind == GOSO_SO) return goso_t(alpha, a, b) + goso_t(alpha, b, a);
  return goso_tail(alpha, a, b) + goso_tail(alpha, b, a);
}

inline double goso_alpha(double pfa, uint32_t kind, uint32_t a, uint32_t b)
{
  if (a == 0 && b == 0) return std::nan("");
  if (a == 0 || b == 0) { // one half: the cell-averaging factor over the other (cfar_alpha_fill's expression)
    const double n = (double)(a + b);
    return n * (pow(pfa, -1.0 / n) - 1);
  }
  double hi = 1.0;
  while (goso_pfa(hi, kind, a, b) > pfa) hi *= 2.0;
  return bisect_upper(0.0, hi, [&](double x) { return goso_pfa(x, kind, a, b) > pfa; });
}

// blah2hip_gocfar_alpha past its checks: alpha[i] for the pair (a[i], b[i]).  A bisection of about 60 evaluations of a + b
// terms each per pair (greatest-of: a + b logarithms and the tails' few dozen terms); long lists (a 2-D window's pairs at the map's corners) are cut into slices.
inline void goso_alpha_fill(double pfa, uint32_t kind, uint32_t n_pairs, const uint32_t *a, const uint32_t *b, double *alpha)
{
  uint64_t terms = 0;
  for (uint32_t i = 0; i < n_pairs; i++) terms += (uint64_t)a[i] + b[i];
  const uint32_t nThreads = terms < 20000 ? 1u : table_threads();
  run_slices(nThreads, [=](uint32_t first) {
    for (uint64_t i = first; i < n_pairs; i += nThreads) alpha[i] = goso_alpha(pfa, kind, a[i], b[i]);
  });
}

} // namespace
} // namespace blah2
