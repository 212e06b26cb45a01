// Host emulation of the 513-point prime-factor transform (blah2_amd/csrc/fft_pfa513.hpp) as
// doppler_pfa513_kernel runs it on one column: the lanes of each step one after another, every
// lane's loads of a step before any lane's stores (what a wave's in-order LDS operations give),
// the exchange region aliased to the column, DC removal (r0 subtracted, 513 r0 added to bin 0).
// Used by tests/test_pfa513_host.py (not gpu).
//
//   emulate_pfa513 IN   IN: 513 lines "re im"; prints 513 lines "re im", the DFT in natural order
#include "../../blah2_amd/csrc/fft_pfa513.hpp"

#include <cstdio>
#include <vector>

using namespace blah2;

int main(int argc, char **argv)
{
  if (argc != 2) { std::fprintf(stderr, "usage: emulate_pfa513 IN\n"); return 2; }
  std::FILE *f = std::fopen(argv[1], "r");
  if (!f) { std::perror(argv[1]); return 2; }
  constexpr int N = Pfa513::N;
  std::vector<cf> region(N);
  for (int i = 0; i < N; i++)
    if (std::fscanf(f, "%f %f", &region[i].x, &region[i].y) != 2) { std::fprintf(stderr, "short input\n"); return 2; }
  std::fclose(f);

  const cf r0 = region[0];
  std::vector<cf> reg(32 * 27);
  for (int l = 0; l < Pfa513::N1; l++) Pfa513::load1(l, region.data(), r0, &reg[l * 27]);
  for (int l = 0; l < Pfa513::N1; l++) Pfa513::dft19_store(&reg[l * 27], region.data() + l);
  for (int l = 0; l < Pfa513::N2; l++) Pfa513::load2(l, region.data(), &reg[l * 27]);
  std::vector<cf> out(N);
  for (int l = 0; l < Pfa513::N2; l++) {
    cf *v = &reg[l * 27];
    Pfa513::dft27(v);
    for (int k1 = 0; k1 < Pfa513::N1; k1++) {
      cf d = v[k1];
      if (l == 0 && k1 == 0) d = cmake(d.x + (float)N * r0.x, d.y + (float)N * r0.y);
      out[Pfa513::out_index(k1, l)] = d;
    }
  }
  for (int k = 0; k < N; k++) std::printf("%.9g %.9g\n", out[k].x, out[k].y);
  return 0;
}
