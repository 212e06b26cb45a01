// Device code of the clutter filter's Toeplitz solve (clutter_solve.hip): the one-workgroup recursion for one and for
// several right-hand sides, its form on vectors in global memory for the long filters, and the look-ahead form on several
// workgroups per CPI (solve_la.hpp).  Included by clutter_solve.hip alone: every instantiation of these kernels is that unit's.
#pragma once

#include <hip/hip_runtime.h>

#include "clutter_handle.hpp"

#include <stdint.h>

namespace blah2 {
namespace clutter {

// Hermitian Toeplitz solve A w = b, A[i][j] = r[i-j], by the Levinson recursion with its inner
// products replaced by Schur-type residual recursions, so that one order is a purely ELEMENT-WISE
// update of length n with a few scalars broadcast -- no reduction, one workgroup barrier per order.
//
// Levinson (the round-1 kernel): forward vector f (T_m f = e_1), backward vector conj(rev f), solution
// x; per order m it needs ef = sum_i r[m-i] f[i] and ex = sum_i r[m-i] x[i]: two dot products, i.e. a
// wave reduction, an LDS exchange of partials and a second barrier per order (3.1 ms for 2047 orders).
// Apply T to the (zero-extended) vectors instead and carry the results along:
//     a_m[j] = (T f_m)[j],  c_m[j] = (T conj(rev f_m))[j],  g_m[j] = b[j] - (T x_m)[j]        (j >= m)
// then ef = a_m[m] and d = b[m] - ex = g_m[m] are simply the LEADING ELEMENTS, and with D = 1 - |ef|^2
//     a_{m+1}[j] = (a_m[j]   - ef       c_m[j-1]) / D        f_{m+1}[i]        = (f_m[i]         - ef       conj f_m[m-i]) / D
//     c_{m+1}[j] = (c_m[j-1] - conj(ef) a_m[j]  ) / D        conj f_{m+1}[m-i] = (conj f_m[m-i] - conj(ef) f_m[i]      ) / D
//     g_{m+1}[j] = g_m[j] - d c_{m+1}[j]                     x_{m+1}[i]        = x_m[i] + d conj f_{m+1}[m-i]
// Both columns are carried UNNORMALISED -- A = s a, C = s c, F = s f with s_{m+1} = s_m D, the
// prediction-error power relative to r[0] -- which removes every per-element division and makes the two
// columns literally the same update,
//     (u, v) -> (u - ef v, v - conj(ef) u),      acc += dt v',      ef = A_m[m] / s_m,  dt = d / s_{m+1},
// on different operands: index j > m carries (A[j], C[j-1], -g[j]), index j <= m carries
// (F[j], conj F[m-j], x[j]).  An index changes role once, at m = j, where A[m] and g[m] have been
// consumed as the scalars and F[m] = x[m] = 0 start.  Thread t owns the indices t + NT k (u and acc in
// registers); v comes from a neighbour (C[j-1]) or the mirror index (F[m-j]) through an LDS array that
// holds C[j] for j > m and F[j] for j <= m, double-buffered so that one barrier per order suffices.
// The critical path of an order is short: the owner of index m+1 forms ef' = A'[m+1] / s_{m+1} as soon
// as its own update is done -- 1/s_{m+1} = (1/s_m)(1/D) needs only THIS order's ef, so every thread
// computes it (one reciprocal) while the LDS operands are in flight -- and publishes (ef', 1/s_{m+1},
// d') for the next order.
// The matrix is positive definite iff r[0] > 0 and every D > 0 -- the condition under which the
// reference's chol() succeeds (WienerHopf.cpp:111) -- else ok = 0.  fp64 throughout.
__device__ __forceinline__ dcx dsub_mul(dcx u, dcx e, dcx v) // u - e*v, two dependent fmas per component
{
  return {__builtin_fma(e.y, v.y, __builtin_fma(-e.x, v.x, u.x)), __builtin_fma(-e.y, v.x, __builtin_fma(-e.x, v.y, u.y))};
}
__device__ __forceinline__ dcx dadd_mul(dcx u, dcx e, dcx v) // u + e*v
{
  return {__builtin_fma(-e.y, v.y, __builtin_fma(e.x, v.x, u.x)), __builtin_fma(e.y, v.x, __builtin_fma(e.x, v.y, u.y))};
}
// 1/d for d in (0, 1]: hardware estimate + two Newton steps (5 dependent instructions instead of the
// ~10 of the IEEE-exact division sequence; this reciprocal sits on the critical path of every order)
__device__ __forceinline__ double fast_rcp(double d)
{
  double r = __builtin_amdgcn_rcp(d);
  double e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-d, r, 1.0);
  return __builtin_fma(r, e, r);
}

// scalars of one order, published through LDS by the owner of index m at the end of order m-1
struct SolveScal {
  dcx ef;    // reflection coefficient a_m[m] = A_m[m] / s_m
  dcx d;     // g_m[m]
  double rs; // 1 / s_m
  double pad;
};

template <int K>
__global__ __launch_bounds__(1024) void clutter_solve_kernel(SolveArgs a)
{
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int n = a.nBins;
  // two buffers of n + 1 entries (entry n stays zero: "F[m]" as seen by index 0), then the scalars
  dcx *cur = reinterpret_cast<dcx *>(smem);
  dcx *nxt = cur + (n + 1);
  SolveScal *scal = reinterpret_cast<SolveScal *>(nxt + (n + 1)); // [parity]
  const int cpi = blockIdx.x;
  const int t = threadIdx.x, NT = blockDim.x;
  if (a.gate) { // behind the look-ahead solve: only the CPIs it gave up on
    const unsigned long long g = __hip_atomic_load(a.gate + (size_t)cpi * a.gateStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((uint32_t)g != *a.epoch) return;
    if (t == 0) atomicAdd(a.retries, 1u);
  }
  const dcx *rg = a.rb + (size_t)cpi * 2 * n;
  const double r0 = rg[0].x;
  bool ok = (r0 > 0.0) && isfinite(r0);
  const double inv0 = ok ? 1.0 / r0 : 0.0;
  const dcx x0 = {rg[n].x * inv0, rg[n].y * inv0}; // x_1[0] = b[0] / r[0]
  dcx U[K], Acc[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int j = t + NT * k;
    U[k] = {0.0, 0.0};
    Acc[k] = {0.0, 0.0};
    if (j < n) {
      const dcx rj = rg[j], bj = rg[n + j];
      if (j == 0) {
        U[k] = {inv0, 0.0}; // F_1[0] = f_1[0] (s_1 = 1)
        Acc[k] = x0;
      } else {
        U[k] = {rj.x * inv0, rj.y * inv0};  // A_1[j] = r[j] / r[0]  (= C_1[j])
        const dcx g = dsub_mul(bj, rj, x0); // g_1[j] = b[j] - r[j] x_1[0]
        Acc[k] = {-g.x, -g.y};
      }
      cur[j] = U[k];
      if (j == 1) {
        scal[1] = SolveScal{U[k], {-Acc[k].x, -Acc[k].y}, 1.0, 0.0};
        U[k] = {0.0, 0.0};   // becomes F[1] = 0, x[1] = 0 at order 1
        Acc[k] = {0.0, 0.0};
      }
    }
  }
  if (t == 0) { cur[n] = {0.0, 0.0}; nxt[n] = {0.0, 0.0}; }
  __syncthreads();
  for (int m = 1; m < n && ok; m++) {
    const SolveScal q = scal[m & 1];
    // operands first: they are in flight while the scalars below are formed
    dcx v[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int j = t + NT * k;
      const int src = (j > m) ? j - 1 : (j == 0 ? n : m - j); // C[j-1], or F[m-j] (F[m] = 0 lives in entry n)
      const dcx s = cur[min(src, n)];
      v[k] = {s.x, (j > m) ? s.y : -s.y};
    }
    const double D = __builtin_fma(-q.ef.y, q.ef.y, __builtin_fma(-q.ef.x, q.ef.x, 1.0));
    if (!(D > 0.0) || !isfinite(D)) { ok = false; break; } // uniform: every thread reads the same scalars
    const double rsn = q.rs * fast_rcp(D); // 1 / s_{m+1}
    const dcx dt = {q.d.x * rsn, q.d.y * rsn};
    const dcx efc = {q.ef.x, -q.ef.y};
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int j = t + NT * k;
      if (j < n) {
        const dcx un = dsub_mul(U[k], q.ef, v[k]);
        const dcx vn = dsub_mul(v[k], efc, U[k]);
        const dcx an = dadd_mul(Acc[k], dt, vn);
        const bool hi = j > m;
        nxt[j] = {hi ? vn.x : un.x, hi ? vn.y : un.y};
        const bool owner = (j == m + 1); // this index turns into F[m+1] = 0, x[m+1] = 0 for the next order
        if (owner) scal[(m + 1) & 1] = SolveScal{{un.x * rsn, un.y * rsn}, {-an.x, -an.y}, rsn, 0.0};
        U[k] = {owner ? 0.0 : un.x, owner ? 0.0 : un.y};
        Acc[k] = {owner ? 0.0 : an.x, owner ? 0.0 : an.y};
      }
    }
    __syncthreads();
    dcx *tmp = cur; cur = nxt; nxt = tmp;
  }
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int j = t + NT * k;
    if (j < n) a.w[(size_t)cpi * n + j] = ok ? cmake((float)Acc[k].x, (float)Acc[k].y) : cmake(0.f, 0.f);
  }
  if (t == 0) a.ok[cpi] = ok ? 1 : 0;
}

// clutter_solve_kernel for several right-hand sides on ONE matrix (blah2hip_clutter_process_multi_dev_fmt): the columns
// (U, v), ef, D and 1 / s_{m+1} belong to toeplitz(r) and are formed once per order; a channel adds one Acc, one d and one
// dt = d / s_{m+1}.  Per channel the arithmetic is clutter_solve_kernel's in its order, so the taps are its bits.  A
// workgroup carries a tile of NS channels (blockIdx.y = the tile; NS = 8, 4, 2 at 1, 2, 4 indices per thread: 32 registers
// of Acc); channels of the tile beyond nSurv run on zeros and are not written.  LDS: cur / nxt as there, and the scalars
// with NS values of d.
template <int NS> struct SolveScalM {
  dcx ef;
  double rs, pad;
  dcx d[NS];
};

template <int K, int NS>
__global__ __launch_bounds__(1024) void clutter_solve_multi_kernel(SolveMultiArgs a)
{
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int n = a.nBins;
  dcx *cur = reinterpret_cast<dcx *>(smem);
  dcx *nxt = cur + (n + 1);
  SolveScalM<NS> *scal = reinterpret_cast<SolveScalM<NS> *>(nxt + (n + 1)); // [parity]
  const int cpi = blockIdx.x, k0 = blockIdx.y * NS;
  const int ns = min(NS, a.nSurv - k0);
  const int t = threadIdx.x, NT = blockDim.x;
  const dcx *rg = a.rb + (size_t)cpi * a.rows * n;
  const dcx *bg = rg + (size_t)(1 + k0) * n; // b of channel k0 + c: bg + c n
  const double r0 = rg[0].x;
  bool ok = (r0 > 0.0) && isfinite(r0);
  const double inv0 = ok ? 1.0 / r0 : 0.0;
  dcx x0[NS];
#pragma unroll
  for (int c = 0; c < NS; c++) {
    x0[c] = {0.0, 0.0};
    if (c < ns) x0[c] = {bg[(size_t)c * n].x * inv0, bg[(size_t)c * n].y * inv0}; // x_1[0] = b[0] / r[0]
  }
  dcx U[K], Acc[NS][K];
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int j = t + NT * k;
    U[k] = {0.0, 0.0};
#pragma unroll
    for (int c = 0; c < NS; c++) Acc[c][k] = {0.0, 0.0};
    if (j < n) {
      const dcx rj = rg[j];
      if (j == 0) {
        U[k] = {inv0, 0.0};
#pragma unroll
        for (int c = 0; c < NS; c++) Acc[c][k] = x0[c];
      } else {
        U[k] = {rj.x * inv0, rj.y * inv0};
#pragma unroll
        for (int c = 0; c < NS; c++)
          if (c < ns) {
            const dcx g = dsub_mul(bg[(size_t)c * n + j], rj, x0[c]); // g_1[j] = b[j] - r[j] x_1[0]
            Acc[c][k] = {-g.x, -g.y};
          }
      }
      cur[j] = U[k];
      if (j == 1) {
        SolveScalM<NS> s;
        s.ef = U[k]; s.rs = 1.0; s.pad = 0.0;
#pragma unroll
        for (int c = 0; c < NS; c++) { s.d[c] = {-Acc[c][k].x, -Acc[c][k].y}; Acc[c][k] = {0.0, 0.0}; }
        scal[1] = s;
        U[k] = {0.0, 0.0};
      }
    }
  }
  if (t == 0) { cur[n] = {0.0, 0.0}; nxt[n] = {0.0, 0.0}; }
  __syncthreads();
  for (int m = 1; m < n && ok; m++) {
    const SolveScalM<NS> q = scal[m & 1];
    dcx v[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int j = t + NT * k;
      const int src = (j > m) ? j - 1 : (j == 0 ? n : m - j);
      const dcx s = cur[min(src, n)];
      v[k] = {s.x, (j > m) ? s.y : -s.y};
    }
    const double D = __builtin_fma(-q.ef.y, q.ef.y, __builtin_fma(-q.ef.x, q.ef.x, 1.0));
    if (!(D > 0.0) || !isfinite(D)) { ok = false; break; }
    const double rsn = q.rs * fast_rcp(D);
    dcx dt[NS];
#pragma unroll
    for (int c = 0; c < NS; c++) dt[c] = {q.d[c].x * rsn, q.d[c].y * rsn};
    const dcx efc = {q.ef.x, -q.ef.y};
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int j = t + NT * k;
      if (j < n) {
        const dcx un = dsub_mul(U[k], q.ef, v[k]);
        const dcx vn = dsub_mul(v[k], efc, U[k]);
        const bool hi = j > m;
        nxt[j] = {hi ? vn.x : un.x, hi ? vn.y : un.y};
        const bool owner = (j == m + 1);
        SolveScalM<NS> s;
        s.ef = {un.x * rsn, un.y * rsn}; s.rs = rsn; s.pad = 0.0;
#pragma unroll
        for (int c = 0; c < NS; c++) {
          const dcx an = dadd_mul(Acc[c][k], dt[c], vn);
          s.d[c] = {-an.x, -an.y};
          Acc[c][k] = {owner ? 0.0 : an.x, owner ? 0.0 : an.y};
        }
        if (owner) scal[(m + 1) & 1] = s;
        U[k] = {owner ? 0.0 : un.x, owner ? 0.0 : un.y};
      }
    }
    __syncthreads();
    dcx *tmp = cur; cur = nxt; nxt = tmp;
  }
#pragma unroll
  for (int c = 0; c < NS; c++)
    if (c < ns) {
      cf *wc = a.w + ((size_t)(k0 + c) * a.nCpi + cpi) * n;
#pragma unroll
      for (int k = 0; k < K; k++) {
        const int j = t + NT * k;
        if (j < n) wc[j] = ok ? cmake((float)Acc[c][k].x, (float)Acc[c][k].y) : cmake(0.f, 0.f);
      }
      if (t == 0) a.ok[(size_t)(k0 + c) * a.nCpi + cpi] = ok ? 1 : 0;
    }
}

// The same recursion for ANY n (the long filters, blah2hip_clutter_create): every vector in global memory -- per CPI cur / nxt
// (n + 1 entries each, shared between the threads: written and read through L2, sc1, with the workgroup barrier between), U and
// Acc (n each, touched by their owner only) -- and a loop over the indices a thread owns instead of register arrays.  A few
// microseconds an order: built for coverage (the reference runs a dense nBins x nBins Cholesky there), not for speed.
__device__ __forceinline__ dcx ld_l2(const dcx *p)
{
  return {__hip_atomic_load(&p->x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __hip_atomic_load(&p->y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)};
}
__device__ __forceinline__ void st_l2(dcx *p, dcx v)
{
  __hip_atomic_store(&p->x, v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&p->y, v.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ __launch_bounds__(1024) void clutter_solve_big_kernel(SolveArgs a, dcx *ws)
{
  __shared__ SolveScal scal[2];
  const int n = a.nBins, cpi = blockIdx.x, t = threadIdx.x, NT = blockDim.x;
  dcx *cur = ws + (size_t)cpi * (4 * (size_t)n + 2);
  dcx *nxt = cur + (n + 1), *U = nxt + (n + 1), *Acc = U + n;
  const dcx *rg = a.rb + (size_t)cpi * 2 * n;
  const double r0 = rg[0].x;
  bool ok = (r0 > 0.0) && isfinite(r0);
  const double inv0 = ok ? 1.0 / r0 : 0.0;
  const dcx x0 = {rg[n].x * inv0, rg[n].y * inv0};
  for (int j = t; j < n; j += NT) { // the first order, as clutter_solve_kernel sets it up
    const dcx rj = rg[j], bj = rg[n + j];
    dcx u, acc;
    if (j == 0) {
      u = {inv0, 0.0};
      acc = x0;
    } else {
      u = {rj.x * inv0, rj.y * inv0};
      const dcx g = dsub_mul(bj, rj, x0);
      acc = {-g.x, -g.y};
    }
    st_l2(cur + j, u);
    if (j == 1) {
      scal[1] = SolveScal{u, {-acc.x, -acc.y}, 1.0, 0.0};
      u = {0.0, 0.0};
      acc = {0.0, 0.0};
    }
    U[j] = u;
    Acc[j] = acc;
  }
  if (t == 0) { st_l2(cur + n, {0.0, 0.0}); st_l2(nxt + n, {0.0, 0.0}); }
  __syncthreads();
  for (int m = 1; m < n && ok; m++) {
    const SolveScal q = scal[m & 1];
    const double D = __builtin_fma(-q.ef.y, q.ef.y, __builtin_fma(-q.ef.x, q.ef.x, 1.0));
    if (!(D > 0.0) || !isfinite(D)) { ok = false; break; } // uniform: every thread reads the same scalars
    const double rsn = q.rs * fast_rcp(D);
    const dcx dt = {q.d.x * rsn, q.d.y * rsn};
    const dcx efc = {q.ef.x, -q.ef.y};
    for (int j = t; j < n; j += NT) {
      const int src = (j > m) ? j - 1 : (j == 0 ? n : m - j);
      const dcx s = ld_l2(cur + min(src, n));
      const dcx v = {s.x, (j > m) ? s.y : -s.y};
      const dcx u = U[j], acc = Acc[j];
      const dcx un = dsub_mul(u, q.ef, v);
      const dcx vn = dsub_mul(v, efc, u);
      const dcx an = dadd_mul(acc, dt, vn);
      const bool hi = j > m;
      st_l2(nxt + j, {hi ? vn.x : un.x, hi ? vn.y : un.y});
      const bool owner = (j == m + 1);
      if (owner) scal[(m + 1) & 1] = SolveScal{{un.x * rsn, un.y * rsn}, {-an.x, -an.y}, rsn, 0.0};
      U[j] = {owner ? 0.0 : un.x, owner ? 0.0 : un.y};
      Acc[j] = {owner ? 0.0 : an.x, owner ? 0.0 : an.y};
    }
    __syncthreads();
    dcx *tmp = cur; cur = nxt; nxt = tmp;
  }
  for (int j = t; j < n; j += NT) {
    const dcx acc = Acc[j];
    a.w[(size_t)cpi * n + j] = ok ? cmake((float)acc.x, (float)acc.y) : cmake(0.f, 0.f);
  }
  if (t == 0) a.ok[cpi] = ok ? 1 : 0;
}

#include "solve_la.hpp"

__global__ void solve_epoch_kernel(uint32_t *epoch)
{
  const uint32_t e = *epoch + 1u;
  *epoch = e ? e : 1u;
}

} // namespace clutter
} // namespace blah2
