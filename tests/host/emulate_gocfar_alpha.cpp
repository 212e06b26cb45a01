// Host build of the greatest-of / smallest-of threshold arithmetic (blah2_amd/csrc/cfar_alpha.hpp) on its own, without the
// library: the filler behind blah2hip_gocfar_alpha, printed so that no bit is lost.
//   emulate_gocfar_alpha SPEC...
//     KIND:PFA:A,B[:A,B...]   KIND 1 (greatest-of) or 2 (smallest-of); prints "go N" and a line of N hex doubles, one per pair,
//                             NaN as "nan"
// PFA in any form strtod reads (the test passes hex).  The guard word behind the table must be untouched.  Exit status 1 on
// a bad SPEC or a failed check.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../blah2_amd/csrc/cfar_alpha.hpp"

using namespace blah2;

int main(int argc, char **argv)
{
  for (int i = 1; i < argc; i++) {
    std::vector<std::string> f;
    for (char *tok = std::strtok(argv[i], ":"); tok; tok = std::strtok(nullptr, ":")) f.push_back(tok);
    if (f.size() < 3) { std::fprintf(stderr, "bad spec %d\n", i); return 1; }
    const uint32_t kind = (uint32_t)std::strtoul(f[0].c_str(), nullptr, 10);
    const double pfa = std::strtod(f[1].c_str(), nullptr);
    if (kind != GOSO_GO && kind != GOSO_SO) { std::fprintf(stderr, "bad kind in spec %d\n", i); return 1; }
    std::vector<uint32_t> a, b;
    for (size_t k = 2; k < f.size(); k++) {
      unsigned x, y;
      if (std::sscanf(f[k].c_str(), "%u,%u", &x, &y) != 2) { std::fprintf(stderr, "bad pair in spec %d\n", i); return 1; }
      a.push_back(x);
      b.push_back(y);
    }
    const uint32_t n = (uint32_t)a.size();
    const double guard = -12345.0;
    std::vector<double> alpha(n + 1, guard); // the table and one guard word behind it; a longer write is the sanitizer's
    goso_alpha_fill(pfa, kind, n, a.data(), b.data(), alpha.data());
    if (alpha[n] != guard) { std::fprintf(stderr, "spec %d: the guard word is wrong\n", i); return 1; }
    std::printf("go %u\n", n);
    for (uint32_t k = 0; k < n; k++) {
      if (std::isnan(alpha[k])) std::printf("nan%c", k + 1 == n ? '\n' : ' ');
      else std::printf("%a%c", alpha[k], k + 1 == n ? '\n' : ' ');
    }
  }
  return 0;
}
