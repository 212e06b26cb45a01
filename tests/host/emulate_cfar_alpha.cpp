// Host build of the detectors' threshold arithmetic (blah2_amd/csrc/cfar_alpha.hpp) on its own, without the library: the
// table fillers behind blah2hip_cfar_alpha and blah2hip_oscfar_alpha, printed so that no bit is lost.
//   emulate_cfar_alpha SPEC...
//     ca:PFA:LOOKS:MAXN        cell averaging       prints "ca MAXN" and a line of MAXN hex doubles alpha[1 .. MAXN]
//     os:PFA:LOOKS:RANK:MAXN   ordered statistic    prints "os MAXN", that line, and a line of the ranks k(1 .. MAXN)
// PFA in any form strtod reads (the test passes hex).  alpha[0] must be NaN and rank[0] zero; the guard words behind the
// tables must be untouched.  Exit status 1 on a bad SPEC or a failed check.
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
    const bool os = !f.empty() && f[0] == "os";
    if (f.size() != (os ? 5u : 4u) || (!os && f[0] != "ca")) { std::fprintf(stderr, "bad spec %d\n", i); return 1; }
    const double pfa = std::strtod(f[1].c_str(), nullptr);
    const uint32_t looks = (uint32_t)std::strtoul(f[2].c_str(), nullptr, 10);
    const uint32_t permille = os ? (uint32_t)std::strtoul(f[3].c_str(), nullptr, 10) : 0;
    const uint32_t maxN = (uint32_t)std::strtoul(f.back().c_str(), nullptr, 10);
    const double guard = -12345.0;
    std::vector<double> alpha(maxN + 2, guard); // the table and one guard word behind it; a longer write is the sanitizer's
    std::vector<uint32_t> rank(maxN + 2, 0xdeadbeefu);
    if (os) oscfar_alpha_fill(pfa, looks, permille, maxN, alpha.data(), rank.data());
    else cfar_alpha_fill(pfa, looks, maxN, alpha.data());
    if (!std::isnan(alpha[0]) || alpha[maxN + 1] != guard || (os && (rank[0] != 0 || rank[maxN + 1] != 0xdeadbeefu))) {
      std::fprintf(stderr, "spec %d: alpha[0], rank[0] or a guard word is wrong\n", i);
      return 1;
    }
    std::printf("%s %u\n", os ? "os" : "ca", maxN);
    for (uint32_t n = 1; n <= maxN; n++) std::printf("%a%c", alpha[n], n == maxN ? '\n' : ' ');
    if (os)
      for (uint32_t n = 1; n <= maxN; n++) std::printf("%u%c", rank[n], n == maxN ? '\n' : ' ');
  }
  return 0;
}
