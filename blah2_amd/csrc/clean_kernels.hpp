// Kernels of clean.hip: strong-echo cancellation on the samples (least-squares CLEAN, blah2hip_clean_*).
//   clean_atoms_kernel     the strongest detections of a CPI expanded into clusters of atoms (delay, Doppler)
//   clean_gram_kernel      lower triangle of G = S^H S and b = S^H y of the atoms' replicas, one fp64 partial per workgroup
//   clean_fold_kernel      ... the partials added in a fixed order (blocks in index order) into the Hermitian G and b
//   clean_solve_kernel     (G + loading (tr G / P) I) a = b through an fp64 Cholesky factor, per CPI
//   clean_subtract_kernel  y_out = y - S a
// The replica of atom p is s_p[n] = x[n - d_p] exp(+2 pi i f_p n / fs), x taken as 0 outside the CPI (nothing wraps).
//
// Phase.  With r = f / fs in fp64 the phase of sample n = m + t (m a multiple of CLN_T, t < CLN_T) is the product of two
// fp32 phasors, each the rounding of an fp64 sincospi: base(m) = exp(2 pi i frac(r m)), where r m is taken with its exact
// fused-multiply-add residual so that only r's own rounding remains (|r| m 2^-53 <= 2^-28 turns at m < 2^26, |f| <= fs / 2),
// and tab(t) = exp(2 pi i frac(r t)).  No fp32 product f n is ever formed.  Error budget per sample, in units of
// u = 2^-24 times |x|: the two rounded phasors 0.71 each, their fp32 complex product 2, the product with x 2, the fp64
// phase 2 pi 2^-28 = 0.4: 5.8 u <= the contract's 8 u.
//
// Choice of form for the Gram products (P = 32: 560 complex pair products a sample).  A vector-ALU form that reads both
// replicas of a pair from LDS moves 16 bytes for 4 fused multiply-adds: at 128 multiply-add lanes and 256 LDS bytes a clock
// per CU that is LDS-bound at half the ALU rate.  A 4 x 4 register block per thread reads 8 replica values (64 bytes) for 16
// complex products (64 multiply-adds): 1 byte a multiply-add, half of what the LDS delivers at the ALU's full rate -- the
// kernel below, bound by vector-ALU issue.  The exact-fp32 MFMA (16x16x4) runs at the same 64 FLOP/clk/SIMD as the vector
// ALU, so it cannot be faster than an ALU-bound vector form by more than the issue slots the loads and address arithmetic
// take; it is not built.
#pragma once

#include "range_core.hpp"

namespace blah2 {

constexpr int CLN_MAX = BLAH2HIP_MAX_ATOMS; // atoms per CPI
constexpr int CLN_T = 128;                  // samples per tile: the replicas of a tile sit in LDS side by side
constexpr int CLN_CH = 1024;                // samples per chunk: the x window of a chunk plus the halo is staged once
constexpr int CLN_TILES = CLN_CH / CLN_T;
constexpr int CLN_MAX_SPAN = 4095;          // delay_hi - delay_lo
constexpr int CLN_ROW = CLN_MAX + 1;        // entries per row of a partial: G[p][0 .. 31], then b[p]
constexpr int CLN_PART = CLN_MAX * CLN_ROW * 2; // doubles per partial
constexpr int CLN_MAX_STRIDE = CLN_T + 16;  // the largest padded row of the replica tile

struct CleanIn {
  const void *x;      // the reference plane in its format
  const cf *y;        // the surveillance plane (fp32)
  uint64_t cpiStride; // samples from CPI to CPI, both planes
  uint32_t n;         // samples per CPI
  int fmt;
  int32_t dlo, dhi;
  double invFs;
  const blah2hip_atom_t *atoms; // [nCpi][capAtoms]
  const uint32_t *count;        // [nCpi]
  uint32_t capAtoms;
};

// LDS bytes of the gram and subtract kernels for a handle's span and a call's atom capacity
__host__ __device__ static inline size_t clean_lds_window(int32_t span) { return (((size_t)CLN_CH + span) * sizeof(cf) + 15) & ~(size_t)15; }
__host__ __device__ static inline size_t clean_lds_tab(uint32_t cap) { return (size_t)cap * CLN_T * sizeof(cf); }
__host__ __device__ static inline size_t clean_lds_base() { return (size_t)CLN_TILES * CLN_MAX * sizeof(cf); }
// thread groups per 4 x 4 block (SL) and the padded row of the replica tile for PB blocks of four atoms: clean_gram_kernel's plan
__host__ __device__ static inline uint32_t clean_slices(uint32_t PB)
{
  const uint32_t NT = PB * (PB + 1) / 2 + PB;
  uint32_t SL = 64;
  while (NT * SL > 256) SL >>= 1;
  return SL;
}
__host__ __device__ static inline uint32_t clean_stride(uint32_t PB) { const uint32_t SL = clean_slices(PB); return CLN_T + (SL / 4 > 1 ? SL / 4 : 1); }
// the largest tile any atom count up to cap needs (fewer atoms: fewer rows, but wider padding)
__host__ __device__ static inline size_t clean_lds_tile(uint32_t cap)
{
  size_t m = 0;
  for (uint32_t PB = 1; PB <= (cap + 3) / 4; PB++) {
    const size_t b = (size_t)(4 * PB + 4) * clean_stride(PB) * sizeof(cf);
    m = b > m ? b : m;
  }
  return m;
}

__device__ __forceinline__ cf cln_mul(cf a, cf b) { return cmake(fmaf(-a.y, b.y, a.x * b.x), fmaf(a.y, b.x, a.x * b.y)); }

// exp(2 pi i frac(r n)) rounded once to fp32 (see "Phase" above)
__device__ __forceinline__ cf cln_phasor(double r, uint32_t n)
{
  const double dn = (double)n, p = r * dn, e = fma(r, dn, -p);
  const double fr = (p - rint(p)) + e;
  double s, c;
  sincospi(2.0 * fr, &s, &c);
  return cmake((float)c, (float)s);
}

__device__ __forceinline__ cf cln_load_x(const void *x, int fmt, uint64_t i)
{
  if (fmt == BLAH2HIP_FMT_C32) return ((const cf *)x)[i];
  if (fmt == BLAH2HIP_FMT_I16X_C32Y) { // I1 Q1 I2 Q2: tuner 1 is the reference
    const int16_t *p = (const int16_t *)x + 4 * i;
    return cmake((float)p[0], (float)p[1]);
  }
  const int8_t *p = (const int8_t *)x + 2 * i;
  return cmake((float)p[0], (float)p[1]);
}

__device__ __forceinline__ bool cln_atom_ok(const blah2hip_atom_t &a, int32_t dlo, int32_t dhi)
{
  return a.delay >= dlo && a.delay <= dhi && fabs(a.doppler) < __builtin_huge_val(); // (a NaN fails the comparison)
}

// The atoms of the CPI into LDS (delays, r = f / fs) and the phasor table tab[p][t]; returns whether every atom is valid.
// All 256 threads call it; it ends in a barrier.
__device__ __forceinline__ bool cln_setup(const CleanIn &a, uint32_t cpi, uint32_t P, int32_t *sDelay, double *sR, cf *tab)
{
  const uint32_t t = threadIdx.x;
  int bad = 0;
  if (t < P) {
    const blah2hip_atom_t at = a.atoms[(size_t)cpi * a.capAtoms + t];
    bad = !cln_atom_ok(at, a.dlo, a.dhi);
    sDelay[t] = at.delay;
    sR[t] = at.doppler * a.invFs;
  }
  if (__syncthreads_or(bad)) return false;
  for (uint32_t e = t; e < P * CLN_T; e += 256) tab[e] = cln_phasor(sR[e / CLN_T], e % CLN_T);
  __syncthreads();
  return true;
}

// The x window of the chunk at n0 into LDS: xw[w] = x[n0 - dhi + w], 0 outside the CPI; and the tiles' base phasors.
// Replica p at sample n0 + s reads xw[s + dhi - d_p].  The caller puts a barrier in front (the window's last readers) and
// behind.
__device__ __forceinline__ void cln_stage(const CleanIn &a, uint32_t cpi, uint32_t P, uint32_t n0, const double *sR, cf *xw, cf *base)
{
  const uint32_t t = threadIdx.x, W = CLN_CH + (uint32_t)(a.dhi - a.dlo);
  const int64_t m0 = (int64_t)n0 - a.dhi;
  const uint64_t off = (uint64_t)cpi * a.cpiStride;
  for (uint32_t w = t; w < W; w += 256) {
    const int64_t m = m0 + w;
    xw[w] = (m >= 0 && m < (int64_t)a.n) ? cln_load_x(a.x, a.fmt, off + (uint64_t)m) : cmake(0.f, 0.f);
  }
  const uint32_t tile = t / CLN_MAX, p = t % CLN_MAX; // 8 tiles x 32 atoms: one phasor a thread
  if (p < P) base[t] = cln_phasor(sR[p], n0 + tile * CLN_T);
}

struct CleanGramArgs {
  CleanIn in;
  double *part; // [nCpi][CLN_PART / 2 entries][gridDim.x] (re, im)
};

// grid (G, nCpi), 256 threads, dynamic LDS: window | tab | base | tile.  A workgroup walks the chunks blockIdx.x, + G, ...
// of its CPI.  Per tile of CLN_T samples the P replicas and y are formed in LDS (rows 0 .. P-1, zero rows up to a multiple
// of 4, then y and three zero rows); the products are cut into 4 x 4 blocks (i, j <= i) of the lower triangle plus the blocks
// (i, y), one block a thread group of SL threads, thread `slice` of a group taking the samples slice, slice + SL, ...  of
// the tile: CLN_T / SL <= 32 fp32 fused multiply-adds per sum (the documented run length), then the sums are added into the
// thread's fp64 accumulators, which live through all chunks.  At the end a butterfly over the SL lanes of a group (a fixed
// tree) leaves the workgroup's partial.  No floating-point atomics.  A CPI with an invalid atom leaves zeros.
__global__ __launch_bounds__(256) void clean_gram_kernel(CleanGramArgs g)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char cln_lds[];
  __shared__ int32_t sDelay[CLN_MAX];
  __shared__ double sR[CLN_MAX];
  const CleanIn &a = g.in;
  const uint32_t cpi = blockIdx.y, t = threadIdx.x;
  const uint32_t P = min(a.count[cpi], a.capAtoms);
  // entry e of this workgroup's partial: (re, im) at part[2 * e * gridDim.x]: a CPI's partials of one entry lie side by side
  double *part = g.part + 2 * ((size_t)cpi * gridDim.x * (CLN_PART / 2) + blockIdx.x);
  const size_t ps = 2 * (size_t)gridDim.x;
  if (P == 0) return; // (nothing of the partial is read)
  cf *xw = (cf *)cln_lds;
  cf *tab = (cf *)(cln_lds + clean_lds_window(a.dhi - a.dlo));
  cf *base = tab + (size_t)a.capAtoms * CLN_T;
  cf *tile = base + CLN_TILES * CLN_MAX;
  if (!cln_setup(a, cpi, P, sDelay, sR, tab)) {
    for (uint32_t e = t; e < CLN_PART / 2; e += 256) { part[e * ps] = 0.0; part[e * ps + 1] = 0.0; }
    return;
  }
  const uint32_t PB = (P + 3) / 4, tri = PB * (PB + 1) / 2, NT = tri + PB;
  const uint32_t SL = clean_slices(PB);
  const uint32_t stride = clean_stride(PB); // rows 4 apart land SL samples apart in the banks
  const uint32_t task = t / SL, slice = t % SL;
  const bool active = task < NT;
  uint32_t ti = 0, tj = PB; // block row, block column (PB: the y block)
  if (task < tri) {
    while ((ti + 1) * (ti + 2) / 2 <= task) ti++;
    tj = task - ti * (ti + 1) / 2;
  } else if (active) ti = task - tri;
  const uint32_t rows = 4 * PB + 4, yRow = 4 * PB;

  double accR[4][4], accI[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) accR[i][j] = accI[i][j] = 0.0;

  const uint32_t nChunks = (a.n + CLN_CH - 1) / CLN_CH;
  const cf *y = a.y + (size_t)cpi * a.cpiStride;
  for (uint32_t c = blockIdx.x; c < nChunks; c += gridDim.x) {
    const uint32_t n0 = c * CLN_CH;
    __syncthreads();
    cln_stage(a, cpi, P, n0, sR, xw, base);
    __syncthreads();
    for (uint32_t k = 0; k < CLN_TILES; k++) {
      const uint32_t t0 = n0 + k * CLN_T;
      if (t0 >= a.n) break;
      for (uint32_t e = t; e < rows * CLN_T; e += 256) {
        const uint32_t row = e / CLN_T, ts = e % CLN_T, n = t0 + ts;
        cf s = cmake(0.f, 0.f);
        if (n < a.n) {
          if (row < P) s = cln_mul(xw[k * CLN_T + ts + (uint32_t)(a.dhi - sDelay[row])], cln_mul(base[k * CLN_MAX + row], tab[row * CLN_T + ts]));
          else if (row == yRow) s = y[n];
        }
        tile[row * stride + ts] = s;
      }
      __syncthreads();
      if (active) {
        float fr[4][4], fi[4][4];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int j = 0; j < 4; j++) fr[i][j] = fi[i][j] = 0.f;
        const cf *A = tile + (4 * ti) * stride + slice, *B = tile + (4 * tj) * stride + slice;
        for (uint32_t s = 0; s < CLN_T; s += SL) {
          cf va[4], vb[4];
#pragma unroll
          for (int i = 0; i < 4; i++) { va[i] = A[i * stride + s]; vb[i] = B[i * stride + s]; }
#pragma unroll
          for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) { // conj(a) b
              fr[i][j] = fmaf(va[i].y, vb[j].y, fmaf(va[i].x, vb[j].x, fr[i][j]));
              fi[i][j] = fmaf(-va[i].y, vb[j].x, fmaf(va[i].x, vb[j].y, fi[i][j]));
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int j = 0; j < 4; j++) { accR[i][j] += (double)fr[i][j]; accI[i][j] += (double)fi[i][j]; }
      }
      __syncthreads();
    }
  }
  // the SL lanes of a group are neighbours inside one wave (SL divides 64): a butterfly, the same tree every call
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      double vr = accR[i][j], vi = accI[i][j];
      for (uint32_t off = SL >> 1; off > 0; off >>= 1) { vr += __shfl_xor(vr, off); vi += __shfl_xor(vi, off); }
      const uint32_t p = 4 * ti + i, q = 4 * tj + j;
      if (active && slice == 0 && p < P) {
        if (tj < PB) {
          if (q <= p) { part[(p * CLN_ROW + q) * ps] = vr; part[(p * CLN_ROW + q) * ps + 1] = vi; }
        } else if (j == 0) { part[(p * CLN_ROW + CLN_MAX) * ps] = vr; part[(p * CLN_ROW + CLN_MAX) * ps + 1] = vi; }
      }
    }
}

// grid (ceil(cap (cap + 1) / 4), nCpi), 256 threads: a wave per entry (p, q <= p) or b[p].  The entry's nParts partials are added
// in index order in 64 contiguous blocks, lane l taking block l, and the block sums then in block order by lane 0: a fixed
// order, so two calls give the same bits.  Then G[c][p][q] (re, im) with both triangles, G[q][p] the exact conjugate of
// G[p][q], the diagonal's imaginary part 0, zeros from the CPI's atom count on; b[c][p] likewise.  G: [nCpi][cap][cap],
// b: [nCpi][cap].
__global__ __launch_bounds__(256) void clean_fold_kernel(const double *part, uint32_t nParts, const uint32_t *count, uint32_t cap,
                                                         double *G, double *b)
{
  __shared__ double sr[4][64], si[4][64];
  const uint32_t cpi = blockIdx.y, P = min(count[cpi], cap), wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t e = blockIdx.x * 4 + wave;
  const bool live = e < cap * (cap + 1);
  const uint32_t p = live ? e / (cap + 1) : 0, q = live ? e % (cap + 1) : 0;
  const bool isB = q == cap, wanted = live && (isB || q <= p);
  double vr = 0.0, vi = 0.0;
  if (wanted && p < P) {
    const double *pe = part + 2 * ((size_t)cpi * (CLN_PART / 2) + (p * CLN_ROW + (isB ? CLN_MAX : q))) * nParts;
    const uint32_t k = (nParts + 63) / 64, w0 = lane * k, w1 = min(nParts, w0 + k);
    for (uint32_t w = w0; w < w1; w++) { vr += pe[2 * w]; vi += pe[2 * w + 1]; }
  }
  sr[wave][lane] = vr;
  si[wave][lane] = vi;
  __syncthreads();
  if (!wanted || lane != 0) return;
  vr = vi = 0.0;
  for (uint32_t l = 0; l < 64; l++) { vr += sr[wave][l]; vi += si[wave][l]; }
  if (isB) {
    b[2 * ((size_t)cpi * cap + p)] = vr;
    b[2 * ((size_t)cpi * cap + p) + 1] = vi;
  } else {
    double *lo = G + 2 * (((size_t)cpi * cap + p) * cap + q), *up = G + 2 * (((size_t)cpi * cap + q) * cap + p);
    if (p == q) { lo[0] = vr; lo[1] = 0.0; }
    else { lo[0] = vr; lo[1] = vi; up[0] = vr; up[1] = -vi; }
  }
}

// grid (nCpi), 64 threads.  G_l = G + loading (tr G / P) I = L L^H column by column in cholesky_loaded's arithmetic (the
// pivot's sum and each entry's sum run over p = 0 .. j-1 in order; the column is scaled by 1 / pivot), thread i taking row i;
// L v = b and L^H a = v column-oriented, each unknown's terms subtracted in the order the columns are solved.  ok = 1
// when every atom is valid, every pivot is finite and above 2^-46 of its loaded diagonal entry (positive beyond the
// rounding of its sum: exactly dependent atoms fail without loading whatever the last bits do) and a is finite; otherwise ok = 0 and a = 0.  P = 0: ok = 1.
// amp and ampKeep: [nCpi][cap] (re, im), zeros from P on.
__global__ __launch_bounds__(64) void clean_solve_kernel(const double *G, const double *b, const blah2hip_atom_t *atoms, const uint32_t *count,
                                                         uint32_t cap, int32_t dlo, int32_t dhi, double loading, double *amp,
                                                         int32_t *ok, double *ampKeep, int32_t *okKeep)
{
  __shared__ double lr[CLN_MAX][CLN_MAX + 1], li[CLN_MAX][CLN_MAX + 1], vr[CLN_MAX], vi[CLN_MAX], xr[CLN_MAX], xi[CLN_MAX];
  __shared__ double sInv, sDelta;
  __shared__ int sGood;
  const uint32_t cpi = blockIdx.x, t = threadIdx.x, P = min(count[cpi], cap);
  const double *Gc = G + 2 * (size_t)cpi * cap * cap, *bc = b + 2 * (size_t)cpi * cap;
  int bad = 0;
  if (t < P) bad = !cln_atom_ok(atoms[(size_t)cpi * cap + t], dlo, dhi);
  if (t == 0) {
    double tr = 0.0;
    for (uint32_t i = 0; i < P; i++) tr += Gc[2 * (i * cap + i)];
    sDelta = P ? loading * (tr / (double)P) : 0.0;
    sGood = 1;
  }
  if (t < P) {
    for (uint32_t q = 0; q <= t; q++) { lr[t][q] = Gc[2 * (t * cap + q)]; li[t][q] = Gc[2 * (t * cap + q) + 1]; }
    vr[t] = bc[2 * t];
    vi[t] = bc[2 * t + 1];
  }
  bad = __syncthreads_or(bad);
  for (uint32_t j = 0; j < P; j++) {
    if (t == j) {
      const double diag = lr[j][j] + sDelta;
      double d = diag;
      for (uint32_t p = 0; p < j; p++) d -= lr[j][p] * lr[j][p] + li[j][p] * li[j][p];
      if (!(d > 0x1p-46 * diag) || !(d < __builtin_huge_val())) sGood = 0; // (positive beyond the rounding of its own sum)
      const double piv = sqrt(d);
      lr[j][j] = piv;
      sInv = 1.0 / piv;
    }
    __syncthreads();
    if (t > j && t < P) {
      double sr = lr[t][j], si = li[t][j];
      for (uint32_t p = 0; p < j; p++) { // - L[i][p] conj(L[j][p])
        sr -= lr[t][p] * lr[j][p] + li[t][p] * li[j][p];
        si -= li[t][p] * lr[j][p] - lr[t][p] * li[j][p];
      }
      lr[t][j] = sr * sInv;
      li[t][j] = si * sInv;
    }
    __syncthreads();
  }
  for (uint32_t j = 0; j < P; j++) { // L v = b
    if (t == j) { xr[j] = vr[j] / lr[j][j]; xi[j] = vi[j] / lr[j][j]; }
    __syncthreads();
    if (t > j && t < P) {
      vr[t] -= lr[t][j] * xr[j] - li[t][j] * xi[j];
      vi[t] -= lr[t][j] * xi[j] + li[t][j] * xr[j];
    }
    __syncthreads();
  }
  if (t < P) { vr[t] = xr[t]; vi[t] = xi[t]; }
  __syncthreads();
  for (int j = (int)P - 1; j >= 0; j--) { // L^H a = v
    if ((int)t == j) { xr[j] = vr[j] / lr[j][j]; xi[j] = vi[j] / lr[j][j]; }
    __syncthreads();
    if ((int)t < j) { // - conj(L[j][t]) a[j]
      vr[t] -= lr[j][t] * xr[j] + li[j][t] * xi[j];
      vi[t] -= lr[j][t] * xi[j] - li[j][t] * xr[j];
    }
    __syncthreads();
  }
  int nf = 0;
  if (t < P) nf = !(fabs(xr[t]) < __builtin_huge_val()) || !(fabs(xi[t]) < __builtin_huge_val());
  nf = __syncthreads_or(nf);
  const int good = !bad && (P == 0 || (sGood && !nf));
  if (t < cap) {
    const double ar = (good && t < P) ? xr[t] : 0.0, ai = (good && t < P) ? xi[t] : 0.0;
    amp[2 * ((size_t)cpi * cap + t)] = ar;
    amp[2 * ((size_t)cpi * cap + t) + 1] = ai;
    ampKeep[2 * ((size_t)cpi * cap + t)] = ar;
    ampKeep[2 * ((size_t)cpi * cap + t) + 1] = ai;
  }
  if (t == 0) { ok[cpi] = good; okKeep[cpi] = good; }
}

struct CleanSubArgs {
  CleanIn in;
  const double *amp; // [nCpi][capAtoms] (re, im)
  const int32_t *ok; // [nCpi]
  cf *out;
  uint64_t outStride;
};

// one sample: y - sum_p a_p s_p as an fp32 fused chain in atom order
__device__ __forceinline__ cf cln_cancel(cf v, uint32_t s, uint32_t P, int32_t dhi, const int32_t *sDelay, const cf *sAmp, const cf *xw,
                                         const cf *base, const cf *tab)
{
  const uint32_t k = s / CLN_T, ts = s % CLN_T;
  for (uint32_t p = 0; p < P; p++) {
    const cf r = cln_mul(xw[s + (uint32_t)(dhi - sDelay[p])], cln_mul(base[k * CLN_MAX + p], tab[p * CLN_T + ts]));
    const cf am = sAmp[p];
    v.x = fmaf(am.y, r.y, fmaf(-am.x, r.x, v.x));
    v.y = fmaf(-am.y, r.x, fmaf(-am.x, r.y, v.y));
  }
  return v;
}

// grid (G, nCpi), 256 threads, dynamic LDS: window | tab | base.  The same staging and the same replicas as
// clean_gram_kernel; the amplitudes are rounded once to fp32.  16-byte accesses (two samples) where the CPI's y and output
// rows both start on 16 bytes, single samples otherwise.  A CPI with ok = 0 or no atoms is copied (skipped when in place).
// Samples from n on -- the stride gap -- are not written.  Each sample is read and written by the same thread: out may be y.
__global__ __launch_bounds__(256) void clean_subtract_kernel(CleanSubArgs g)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char cln_lds[];
  __shared__ int32_t sDelay[CLN_MAX];
  __shared__ double sR[CLN_MAX];
  __shared__ cf sAmp[CLN_MAX];
  typedef float f4 __attribute__((ext_vector_type(4)));
  const CleanIn &a = g.in;
  const uint32_t cpi = blockIdx.y, t = threadIdx.x;
  const uint32_t P = min(a.count[cpi], a.capAtoms);
  const cf *y = a.y + (size_t)cpi * a.cpiStride;
  cf *out = g.out + (size_t)cpi * g.outStride;
  const bool wide = ((((uintptr_t)y) | ((uintptr_t)out)) & 15) == 0;
  const uint32_t nChunks = (a.n + CLN_CH - 1) / CLN_CH;
  cf *xw = (cf *)cln_lds;
  cf *tab = (cf *)(cln_lds + clean_lds_window(a.dhi - a.dlo));
  cf *base = tab + (size_t)a.capAtoms * CLN_T;
  bool cancel = P > 0 && g.ok[cpi] != 0;
  if (cancel) cancel = cln_setup(a, cpi, P, sDelay, sR, tab); // (ok = 1 implies valid atoms; never index on trust)
  if (!cancel) {
    if (out == y) return;
    for (uint32_t c = blockIdx.x; c < nChunks; c += gridDim.x) {
      const uint32_t n0 = c * CLN_CH;
      for (uint32_t s = t; s < CLN_CH && n0 + s < a.n; s += 256) out[n0 + s] = y[n0 + s];
    }
    return;
  }
  if (t < P) sAmp[t] = cmake((float)g.amp[2 * ((size_t)cpi * a.capAtoms + t)], (float)g.amp[2 * ((size_t)cpi * a.capAtoms + t) + 1]);
  for (uint32_t c = blockIdx.x; c < nChunks; c += gridDim.x) {
    const uint32_t n0 = c * CLN_CH;
    __syncthreads();
    cln_stage(a, cpi, P, n0, sR, xw, base);
    __syncthreads();
    if (wide) {
      for (uint32_t u = t; u < CLN_CH / 2; u += 256) {
        const uint32_t s = 2 * u, n = n0 + s;
        if (n + 1 < a.n) {
          const f4 v = *reinterpret_cast<const f4 *>(y + n);
          const cf r0 = cln_cancel(cmake(v[0], v[1]), s, P, a.dhi, sDelay, sAmp, xw, base, tab);
          const cf r1 = cln_cancel(cmake(v[2], v[3]), s + 1, P, a.dhi, sDelay, sAmp, xw, base, tab);
          f4 o;
          o[0] = r0.x; o[1] = r0.y; o[2] = r1.x; o[3] = r1.y;
          *reinterpret_cast<f4 *>(out + n) = o;
        } else if (n < a.n) out[n] = cln_cancel(y[n], s, P, a.dhi, sDelay, sAmp, xw, base, tab);
      }
    } else {
      for (uint32_t s = t; s < CLN_CH && n0 + s < a.n; s += 256)
        out[n0 + s] = cln_cancel(y[n0 + s], s, P, a.dhi, sDelay, sAmp, xw, base, tab);
    }
  }
}

struct CleanAtomsArgs {
  const blah2hip_det_t *dets; // [nCpi][cap]
  const uint32_t *count;      // [nCpi]
  blah2hip_atom_t *atoms;     // [nCpi][capAtoms]
  uint32_t *atomCount;        // [nCpi]
  int32_t *used;              // [nCpi][capAtoms]: indices of the detections that gave atoms, in their order; -1 behind
  uint32_t cap, capAtoms, maxEchoes;
  int32_t sideDelay, sideDoppler, dlo, dhi;
  double snrMin, halfBin; // 0.5 / cpi
};

// whether detection (s1, r1, c1, i1) goes in front of (s0, r0, c0, i0): stronger, then lower row, lower column (index last, for
// duplicates)
__device__ __forceinline__ bool cln_before(double s1, int32_t r1, int32_t c1, uint32_t i1, double s0, int32_t r0, int32_t c0, uint32_t i0)
{
  if (s1 != s0) return s1 > s0;
  if (r1 != r0) return r1 < r0;
  if (c1 != c0) return c1 < c0;
  return i1 < i0;
}

// grid (nCpi), 256 threads.  maxEchoes rounds of selection: every thread scans its share of the list for the best record
// with snr >= snrMin that no earlier round took, a tree over LDS picks the round's winner; thread 0 expands it (echo, then
// i, then j), drops members outside [dlo, dhi], and drops the whole echo where its members do not fit into capAtoms.
__global__ __launch_bounds__(256) void clean_atoms_kernel(CleanAtomsArgs a)
{
  __shared__ double bs[256];
  __shared__ int32_t br[256], bc[256];
  __shared__ uint32_t bi[256];
  __shared__ uint32_t taken[CLN_MAX];
  __shared__ uint32_t nTaken, nAtoms, nUsed;
  const uint32_t cpi = blockIdx.x, t = threadIdx.x;
  const uint32_t n = min(a.count[cpi], a.cap);
  const blah2hip_det_t *d = a.dets + (size_t)cpi * a.cap;
  blah2hip_atom_t *at = a.atoms + (size_t)cpi * a.capAtoms;
  int32_t *used = a.used + (size_t)cpi * a.capAtoms;
  if (t == 0) nTaken = nAtoms = nUsed = 0;
  if (t < a.capAtoms) used[t] = -1;
  __syncthreads();
  for (uint32_t e = 0; e < a.maxEchoes; e++) {
    double s0 = 0.0;
    int32_t r0 = 0, c0 = 0;
    uint32_t i0 = 0xffffffffu;
    for (uint32_t i = t; i < n; i += 256) {
      const double s = d[i].snr;
      if (!(s >= a.snrMin)) continue;
      bool seen = false;
      for (uint32_t k = 0; k < nTaken; k++) seen |= taken[k] == i;
      if (seen) continue;
      if (i0 == 0xffffffffu || cln_before(s, d[i].row, d[i].col, i, s0, r0, c0, i0)) { s0 = s; r0 = d[i].row; c0 = d[i].col; i0 = i; }
    }
    bs[t] = s0; br[t] = r0; bc[t] = c0; bi[t] = i0;
    __syncthreads();
    for (uint32_t off = 128; off > 0; off >>= 1) {
      if (t < off && bi[t + off] != 0xffffffffu &&
          (bi[t] == 0xffffffffu || cln_before(bs[t + off], br[t + off], bc[t + off], bi[t + off], bs[t], br[t], bc[t], bi[t]))) {
        bs[t] = bs[t + off]; br[t] = br[t + off]; bc[t] = bc[t + off]; bi[t] = bi[t + off];
      }
      __syncthreads();
    }
    const uint32_t win = bi[0];
    if (win == 0xffffffffu) break; // (uniform: every thread reads the same word)
    if (t == 0) {
      taken[nTaken++] = win;
      const double dc = rint(d[win].delay), f = d[win].doppler;
      uint32_t m = 0;
      for (int32_t i = -a.sideDelay; i <= a.sideDelay; i++) {
        const double dd = dc + (double)i;
        if (dd >= (double)a.dlo && dd <= (double)a.dhi) m += 2 * a.sideDoppler + 1;
      }
      if (m > 0 && nAtoms + m <= a.capAtoms) {
        for (int32_t i = -a.sideDelay; i <= a.sideDelay; i++) {
          const double dd = dc + (double)i;
          if (!(dd >= (double)a.dlo && dd <= (double)a.dhi)) continue;
          for (int32_t j = -a.sideDoppler; j <= a.sideDoppler; j++) {
            blah2hip_atom_t o;
            o.delay = (int32_t)dd;
            o.reserved = 0;
            o.doppler = f + (double)j * a.halfBin;
            at[nAtoms++] = o;
          }
        }
        used[nUsed++] = (int32_t)win;
      }
    }
    __syncthreads();
  }
  __syncthreads();
  if (t == 0) a.atomCount[cpi] = nAtoms;
}

} // namespace blah2
