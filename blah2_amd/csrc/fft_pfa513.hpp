// 513-point complex DFT (forward) as a Good-Thomas prime-factor transform, 513 = 27 * 19, gcd(27, 19) = 1: no twiddles
// between the two factors, no zero padding, no chirp.  The Doppler stage at nD = 513 (BASELINE configs[1]) runs it in
// place of the chirp-z transform on 1024 points (doppler_pfa513_kernel, kernels.hpp).
//
// Input map  n = (19 n1 + 27 n2) mod 513,          n1 in [0, 27), n2 in [0, 19)
// Output map k = (190 k1 + 324 k2) mod 513,        k1 in [0, 27), k2 in [0, 19)   (CRT: 190 = 1 mod 27, 0 mod 19;
//                                                                                  324 = 0 mod 27, 1 mod 19)
// so that W_513^(n k) = W_27^(n1 k1) W_19^(n2 k2) and X[k1, k2] = sum_n1 W_27^(n1 k1) sum_n2 W_19^(n2 k2) x[n1, n2].
//
// Lane use (one column per 32-lane half of a wave; two columns per wave):
//   step 1  lane n1 < 27 : load1 -- x[n1, n2] - r0 for n2 = 0..18 from the column (19 registers), then dft19_store --
//                          the 19-point DFT over n2, Y[k2][n1] written to the exchange region at k2 * 27 + n1
//                          (lanes 27..31 idle)
//   step 2  lane k2 < 19 : load2 -- Y[k2][n1] for n1 = 0..26, then dft27 -- the 27-point DFT over n1, X[k1, k2] left in
//                          register k1, bound for output k = out_index(k1, k2) (lanes 19..31 idle)
// The exchange region (19 x 27 = 513 values) may be the column's own region: every lane of a wave has issued all of its
// loads of a step before any lane stores (a wave's LDS operations execute in order), which the host emulation
// (tests/host/emulate_pfa513.cpp) reproduces by running each step's loads for all lanes before the stores.
// Step-1 writes are 27 consecutive values per k2, step-2 reads 19 rows at a pitch of 27 (odd): no bank conflicts.
//
// 19-point DFT in the symmetric form: a_j = x_j + x_(19-j), b_j = x_j - x_(19-j) (j = 1..9), then for k = 1..9
//   A_k = x_0 + sum_j cos(2 pi jk/19) a_j,  B_k = sum_j sin(2 pi jk/19) b_j,  X_k = A_k - i B_k,  X_(19-k) = A_k + i B_k
// -- a complex times a real constant is one v_pk_fma_f32 with the constant pair (cos, sin) in SGPRs and op_sel picking
// the half; each k's A and B chains are one asm statement each (a statement boundary between dependent packed
// instructions costs an s_nop, fft_wg.hpp).  27-point DFT as 3 x 9, the 9-point one as 3 x 3: 27 3-point DFTs (six
// packed instructions each, one asm statement) and 28 constant twiddles.  Constants are fp64 values rounded once.
// Forward transform only (the Doppler map's sign).
#pragma once

#include "fft_wg.hpp"

namespace blah2 {

// (cos, sin)(2 pi m / 19)
constexpr float PFA_C19[19] = {
  (float)1.0, (float)0.94581724170063464, (float)0.78914050939639357, (float)0.54694815812242692, (float)0.24548548714079924,
  (float)-0.082579345472332269, (float)-0.40169542465296942, (float)-0.67728157162574087, (float)-0.87947375120648896,
  (float)-0.98636130340272232, (float)-0.98636130340272243, (float)-0.8794737512064893, (float)-0.6772815716257411,
  (float)-0.40169542465296904, (float)-0.082579345472332741, (float)0.24548548714079879, (float)0.54694815812242659,
  (float)0.78914050939639391, (float)0.94581724170063464};
constexpr float PFA_S19[19] = {
  (float)0.0, (float)0.32469946920468346, (float)0.61421271268966782, (float)0.83716647826252855, (float)0.96940026593933037,
  (float)0.99658449300666985, (float)0.9157733266550574, (float)0.73572391067313181, (float)0.47594739303707367,
  (float)0.16459459028073403, (float)-0.16459459028073378, (float)-0.47594739303707312, (float)-0.73572391067313159,
  (float)-0.91577332665505762, (float)-0.99658449300666985, (float)-0.96940026593933049, (float)-0.83716647826252877,
  (float)-0.61421271268966737, (float)-0.32469946920468373};
// W_27^e = (cos, -sin)(2 pi e / 27), e = 0..16
constexpr float PFA_WC27[17] = {
  (float)1.0, (float)0.97304487057982381, (float)0.89363264032341228, (float)0.76604444311897801, (float)0.59715859170278618,
  (float)0.3960797660391569, (float)0.17364817766693041, (float)-0.058144828910475774, (float)-0.28680323271109021,
  (float)-0.49999999999999978, (float)-0.68624163786873349, (float)-0.83548781141293627, (float)-0.93969262078590832,
  (float)-0.99323835774194302, (float)-0.99323835774194302, (float)-0.93969262078590854, (float)-0.83548781141293649};
constexpr float PFA_WS27[17] = {
  (float)0.0, (float)-0.23061587074244017, (float)-0.44879918020046217, (float)-0.64278760968653925, (float)-0.80212319275504373,
  (float)-0.918216106880274, (float)-0.98480775301220802, (float)-0.99830815827126818, (float)-0.9579895123154889,
  (float)-0.86602540378443871, (float)-0.72737364157304885, (float)-0.54950897807080623, (float)-0.34202014332566888,
  (float)-0.11609291412522993, (float)0.11609291412523012, (float)0.34202014332566821, (float)0.54950897807080601};
constexpr float PFA_SIN3 = (float)0.86602540378443865; // sin(2 pi / 3)

// forward 3-point DFT in place: t = b + c, d = b - c, (a + t, m - i s d, m + i s d) with m = a - t/2, s = sin(2 pi/3)
#if defined(B2_PACKED_COMPLEX)
__device__ __forceinline__ void pfa_dft3(cf &a, cf &b, cf &c)
{
  const b2_pk k = {-0.5f, PFA_SIN3};
  b2_pk y0, y1, y2, m;
  asm("v_pk_add_f32 %2, %5, %6\n\t"                                                   // t = b + c
      "v_pk_add_f32 %3, %5, %6 neg_lo:[0,1] neg_hi:[0,1]\n\t"                         // d = b - c
      "v_pk_add_f32 %0, %4, %2\n\t"                                                   // a + t
      "v_pk_fma_f32 %2, %2, %7, %4 op_sel_hi:[1,0,1]\n\t"                             // m = a - t/2
      "v_pk_fma_f32 %1, %3, %7, %2 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_hi:[1,0,0]\n\t" // m + (s d.y, -s d.x)
      "v_pk_fma_f32 %3, %3, %7, %2 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]"     // m + (-s d.y, s d.x)
      : "=&v"(y0), "=v"(y1), "=&v"(m), "=&v"(y2)
      : "v"(B2_V(a)), "v"(B2_V(b)), "v"(B2_V(c)), "s"(k));
  a = B2_C(y0);
  b = B2_C(y1);
  c = B2_C(y2);
}
#else
B2_HD void pfa_dft3(cf &a, cf &b, cf &c)
{
  const cf t = cadd(b, c), d = csub(b, c);
  const cf m = cmake(a.x - 0.5f * t.x, a.y - 0.5f * t.y);
  const float s = PFA_SIN3;
  a = cadd(a, t);
  b = cmake(m.x + s * d.y, m.y - s * d.x);
  c = cmake(m.x - s * d.y, m.y + s * d.x);
}
#endif

template <int E> B2_HD cf pfa_w27(cf a) { return E == 0 ? a : twid_k<-1>(a, PFA_WC27[E], PFA_WS27[E]); }

// forward 9-point DFT in place, natural order: i = j1 + 3 j2, p = p2 + 3 p1
B2_HD void pfa_dft9(cf *u)
{
  pfa_dft3(u[0], u[3], u[6]);
  pfa_dft3(u[1], u[4], u[7]);
  pfa_dft3(u[2], u[5], u[8]); // u[j1 + 3 p2]
  u[4] = pfa_w27<3>(u[4]);    // W_9^(j1 p2)
  u[7] = pfa_w27<6>(u[7]);
  u[5] = pfa_w27<6>(u[5]);
  u[8] = pfa_w27<12>(u[8]);
  pfa_dft3(u[0], u[1], u[2]);
  pfa_dft3(u[3], u[4], u[5]);
  pfa_dft3(u[6], u[7], u[8]); // u[3 p2 + p1] = out[p2 + 3 p1]
  cf o[9];
#pragma unroll
  for (int p2 = 0; p2 < 3; p2++)
#pragma unroll
    for (int p1 = 0; p1 < 3; p1++) o[p2 + 3 * p1] = u[3 * p2 + p1];
#pragma unroll
  for (int i = 0; i < 9; i++) u[i] = o[i];
}

template <int Q2> B2_HD void pfa_dft27_col(cf (*y)[9])
{
  y[1][Q2] = pfa_w27<Q2>(y[1][Q2]);
  y[2][Q2] = pfa_w27<2 * Q2>(y[2][Q2]);
  pfa_dft3(y[0][Q2], y[1][Q2], y[2][Q2]);
}

// forward 27-point DFT in place, natural order: i = i1 + 3 i2, q = q2 + 9 q1
B2_HD void pfa_dft27(cf *v)
{
  cf y[3][9];
#pragma unroll
  for (int i1 = 0; i1 < 3; i1++) {
#pragma unroll
    for (int i2 = 0; i2 < 9; i2++) y[i1][i2] = v[i1 + 3 * i2];
    pfa_dft9(y[i1]);
  }
  pfa_dft27_col<0>(y);
  pfa_dft27_col<1>(y);
  pfa_dft27_col<2>(y);
  pfa_dft27_col<3>(y);
  pfa_dft27_col<4>(y);
  pfa_dft27_col<5>(y);
  pfa_dft27_col<6>(y);
  pfa_dft27_col<7>(y);
  pfa_dft27_col<8>(y);
#pragma unroll
  for (int q2 = 0; q2 < 9; q2++)
#pragma unroll
    for (int q1 = 0; q1 < 3; q1++) v[q2 + 9 * q1] = y[q1][q2];
}

// X_K and X_(19-K) of the 19-point DFT from x_0, a_j, b_j (j = 1..9, in a[j - 1], b[j - 1])
#if defined(B2_PACKED_COMPLEX)
template <int K> __device__ __forceinline__ void pfa_dft19_pair(cf x0, const cf *a, const cf *b, cf &xk, cf &xm)
{
#define PFA_W(j) const b2_pk w##j = {PFA_C19[(j * K) % 19], PFA_S19[(j * K) % 19]};
  PFA_W(1) PFA_W(2) PFA_W(3) PFA_W(4) PFA_W(5) PFA_W(6) PFA_W(7) PFA_W(8) PFA_W(9)
#undef PFA_W
  b2_pk A, B, rk, rm;
  // A = x0 + sum_j cos * a_j: the low half of each constant pair
#define PFA_FA(i, o) "v_pk_fma_f32 %0, %" #i ", %" #o ", %0 op_sel_hi:[1,0,1]\n\t"
  asm("v_pk_fma_f32 %0, %1, %10, %19 op_sel_hi:[1,0,1]\n\t" PFA_FA(2, 11) PFA_FA(3, 12) PFA_FA(4, 13) PFA_FA(5, 14)
        PFA_FA(6, 15) PFA_FA(7, 16) PFA_FA(8, 17) "v_pk_fma_f32 %0, %9, %18, %0 op_sel_hi:[1,0,1]"
      : "=&v"(A)
      : "v"(B2_V(a[0])), "v"(B2_V(a[1])), "v"(B2_V(a[2])), "v"(B2_V(a[3])), "v"(B2_V(a[4])), "v"(B2_V(a[5])),
        "v"(B2_V(a[6])), "v"(B2_V(a[7])), "v"(B2_V(a[8])), "s"(w1), "s"(w2), "s"(w3), "s"(w4), "s"(w5), "s"(w6), "s"(w7),
        "s"(w8), "s"(w9), "v"(B2_V(x0)));
#undef PFA_FA
  // B = sum_j sin * b_j: the high half; then A - i B and A + i B
#define PFA_FB(i, o) "v_pk_fma_f32 %0, %" #i ", %" #o ", %0 op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
  asm("v_pk_mul_f32 %0, %3, %12 op_sel:[0,1] op_sel_hi:[1,1]\n\t" PFA_FB(4, 13) PFA_FB(5, 14) PFA_FB(6, 15)
        PFA_FB(7, 16) PFA_FB(8, 17) PFA_FB(9, 18) PFA_FB(10, 19) PFA_FB(11, 20)
      "v_pk_add_f32 %1, %21, %0 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]\n\t"
      "v_pk_add_f32 %2, %21, %0 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]"
      : "=&v"(B), "=&v"(rk), "=&v"(rm)
      : "v"(B2_V(b[0])), "v"(B2_V(b[1])), "v"(B2_V(b[2])), "v"(B2_V(b[3])), "v"(B2_V(b[4])), "v"(B2_V(b[5])),
        "v"(B2_V(b[6])), "v"(B2_V(b[7])), "v"(B2_V(b[8])), "s"(w1), "s"(w2), "s"(w3), "s"(w4), "s"(w5), "s"(w6), "s"(w7),
        "s"(w8), "s"(w9), "v"(A));
#undef PFA_FB
  xk = B2_C(rk);
  xm = B2_C(rm);
}
#else
template <int K> B2_HD void pfa_dft19_pair(cf x0, const cf *a, const cf *b, cf &xk, cf &xm)
{
  cf A = x0, B = cmake(0.f, 0.f);
  for (int j = 1; j <= 9; j++) {
    const float c = PFA_C19[(j * K) % 19], s = PFA_S19[(j * K) % 19];
    A = cmake(A.x + c * a[j - 1].x, A.y + c * a[j - 1].y);
    B = cmake(B.x + s * b[j - 1].x, B.y + s * b[j - 1].y);
  }
  xk = cmake(A.x + B.y, A.y - B.x);
  xm = cmake(A.x - B.y, A.y + B.x);
}
#endif

struct Pfa513 {
  static constexpr int N = 513, N1 = 27, N2 = 19;
  static constexpr int XP = 27; // exchange region: Y[k2][n1] at k2 * XP + n1

  // output index of register k1 on step-2 lane k2
  B2_HD static constexpr int out_index(int k1, int k2) { return (190 * k1 + 324 * k2) % N; }

  // step-1 lane n1: v[n2] = col[(19 n1 + 27 n2) mod 513] - r0
  B2_HD static void load1(int n1, const cf *col, cf r0, cf *v)
  {
    const unsigned base = 19u * (unsigned)n1;
#pragma unroll
    for (int n2 = 0; n2 < N2; n2++) {
      const unsigned i = base + 27u * n2;
      v[n2] = csub(col[i < (unsigned)N ? i : i - N], r0);
    }
  }
  // step-1 lane n1: 19-point DFT of v (clobbered), Y[k2] written to out[k2 * XP] (out = the exchange region + n1)
  B2_HD static void dft19_store(cf *v, cf *out)
  {
    cf a[9], b[9];
#pragma unroll
    for (int j = 1; j <= 9; j++) {
      a[j - 1] = cadd(v[j], v[N2 - j]);
      b[j - 1] = csub(v[j], v[N2 - j]);
    }
    out[0] = cadd(cadd(cadd(cadd(v[0], a[0]), cadd(a[1], a[2])), cadd(cadd(a[3], a[4]), cadd(a[5], a[6]))), cadd(a[7], a[8]));
    cf xk, xm;
#define PFA_PAIR(K) pfa_dft19_pair<K>(v[0], a, b, xk, xm); out[K * XP] = xk; out[(N2 - K) * XP] = xm;
    PFA_PAIR(1) PFA_PAIR(2) PFA_PAIR(3) PFA_PAIR(4) PFA_PAIR(5) PFA_PAIR(6) PFA_PAIR(7) PFA_PAIR(8) PFA_PAIR(9)
#undef PFA_PAIR
  }
  // step-2 lane k2: v[n1] = Y[k2][n1]
  B2_HD static void load2(int k2, const cf *X, cf *v)
  {
#pragma unroll
    for (int n1 = 0; n1 < N1; n1++) v[n1] = X[k2 * XP + n1];
  }
  // step-2 lane: 27-point DFT, X[k1, k2] in v[k1]
  B2_HD static void dft27(cf *v) { pfa_dft27(v); }
};

} // namespace blah2
