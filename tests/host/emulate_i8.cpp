// Host check of the int8 sample formats' index algebra: InI8 / InI8C32 (blah2_amd/csrc/range_core.hpp) through
// load_seg_x / mask_seg_x / load_seg_y / mask_seg_y -- the portable DEFINITION of the segment windows that the GPU
// loads must reproduce -- against plain indexing of the planes.  Used by tests/test_i8_capture.py (not gpu).
//
//   emulate_i8 R3 nCorr nPulses delayMin nDelay nSeg segLen seed
//       -> "mismatches=<count> checked=<values>"; exit status 1 on any mismatch
// The planes start ONE SAMPLE into their allocations (2-byte aligned only) and are surrounded by a poison value, so a
// window that reads outside its pulse without masking it shows.
#include "../../blah2_amd/csrc/range_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace blah2;

static const int8_t POISON = 99;

template <int R3> int run(int nCorr, int nPulses, int delayMin, int nDelay, int nSeg, int segLen, unsigned seed)
{
  constexpr int T = 16 * R3, F = 256 * R3;
  if (segLen + nDelay - 1 > F || nSeg * segLen < nCorr) { std::printf("geometry does not fit F = %d\n", F); return 2; }
  const int64_t n = (int64_t)nCorr * nPulses, pad = 4096;
  std::vector<int8_t> xb(2 * (n + 2 * pad) + 2, POISON), yb(2 * (n + 2 * pad) + 2, POISON);
  std::vector<cf> yc(n + 2 * pad, cmake(POISON, POISON));
  int8_t *x = xb.data() + 2 * pad + 2, *y = yb.data() + 2 * pad + 2; // sample 0, one sample past an aligned start
  std::mt19937 rng(seed);
  std::uniform_int_distribution<int> d(-128, 127);
  for (int64_t i = 0; i < 2 * n; i++) { x[i] = (int8_t)d(rng); y[i] = (int8_t)d(rng); }
  for (int64_t i = 0; i < n; i++) yc[pad + i] = cmake((float)y[2 * i] + 0.5f, (float)y[2 * i + 1] - 0.25f); // not the int8 values: a swapped channel shows
  const InI8 in{x, y};
  const InI8C32 inc{x, yc.data() + pad};
  RangePlan p{};
  p.nCorr = nCorr; p.nDoppler = nPulses; p.nDelay = nDelay; p.delayMin = delayMin; p.nSeg = nSeg; p.segLen = segLen;
  long bad = 0, checked = 0;
  auto same = [&](cf a, float re, float im) { checked++; if (a.x != re || a.y != im) bad++; };
  for (int pulse = 0; pulse < nPulses; pulse++) {
    const int64_t base = (int64_t)pulse * nCorr;
    const InI8 at = in.at(base); // the same channels, sample `base` first
    for (int s = 0; s < nSeg; s++)
      for (int t = 0; t < T; t++) {
        cf vx[16], vy[16], wx[16], wy[16], ax[16], ay[16];
        load_seg_x<R3>(in, p, base, s, t, vx); mask_seg_x<R3>(p, s, t, vx);
        load_seg_y<R3>(in, p, base, s, t, vy); mask_seg_y<R3>(p, s, t, vy);
        load_seg_x<R3>(inc, p, base, s, t, wx); mask_seg_x<R3>(p, s, t, wx);
        load_seg_y<R3>(inc, p, base, s, t, wy); mask_seg_y<R3>(p, s, t, wy);
        load_seg_x<R3>(at, p, 0, s, t, ax); mask_seg_x<R3>(p, s, t, ax);
        load_seg_y<R3>(at, p, 0, s, t, ay); mask_seg_y<R3>(p, s, t, ay);
        for (int k = 0; k < 16; k++) {
          const int m = t + T * k; // position in the F-point window
          // x'[m] = x[s*segLen + m] for m < segLen inside the pulse, else 0
          const int ix = s * segLen + m;
          const bool okx = m < segLen && ix < nCorr;
          const float xr = okx ? (float)x[2 * (base + ix)] : 0.f, xi = okx ? (float)x[2 * (base + ix) + 1] : 0.f;
          same(vx[k], xr, xi); same(wx[k], xr, xi); same(ax[k], xr, xi);
          // y'[m] = y[s*segLen + delayMin + m] inside the pulse, else 0
          const int iy = s * segLen + delayMin + m;
          const bool oky = iy >= 0 && iy < nCorr;
          const float yr = oky ? (float)y[2 * (base + iy)] : 0.f, yi = oky ? (float)y[2 * (base + iy) + 1] : 0.f;
          same(vy[k], yr, yi); same(ay[k], yr, yi);
          same(wy[k], oky ? yr + 0.5f : 0.f, oky ? yi - 0.25f : 0.f);
        }
      }
  }
  // lx / ly on their own: every sample, both signs' extremes included
  for (int64_t i = 0; i < n; i++) {
    same(in.lx(i), (float)x[2 * i], (float)x[2 * i + 1]);
    same(in.ly(i), (float)y[2 * i], (float)y[2 * i + 1]);
    same(inc.lx(i), (float)x[2 * i], (float)x[2 * i + 1]);
  }
  const int8_t ext[4] = {-128, 127, -1, 0};
  const InI8 e{ext, ext};
  same(e.lx(0), -128.f, 127.f); same(e.ly(1), -1.f, 0.f);
  std::printf("mismatches=%ld checked=%ld\n", bad, checked);
  return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
  if (argc != 9) { std::fprintf(stderr, "usage: emulate_i8 R3 nCorr nPulses delayMin nDelay nSeg segLen seed\n"); return 2; }
  const int R3 = std::atoi(argv[1]), nCorr = std::atoi(argv[2]), nP = std::atoi(argv[3]), dmin = std::atoi(argv[4]),
            nDelay = std::atoi(argv[5]), nSeg = std::atoi(argv[6]), segLen = std::atoi(argv[7]);
  const unsigned seed = (unsigned)std::atoi(argv[8]);
  switch (R3) {
  case 4: return run<4>(nCorr, nP, dmin, nDelay, nSeg, segLen, seed);
  case 8: return run<8>(nCorr, nP, dmin, nDelay, nSeg, segLen, seed);
  case 16: return run<16>(nCorr, nP, dmin, nDelay, nSeg, segLen, seed);
  }
  return 2;
}
