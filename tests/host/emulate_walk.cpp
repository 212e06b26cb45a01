// Host build of the Doppler kernels' tile walk (blah2_amd/csrc/doppler_walk.hpp), walked the way the kernels walk it:
// workgroup b takes doppler_walk_tile(b, G, k, T) for k = 0, 1, ... until it gets -1.
//   emulate_walk            every grid 1 ... 64 and 8 k <= 512 against every tile count below; prints "ok <cases>"
//   emulate_walk G T        prints "b k tile" for every tile taken, in the order of the walk
// Checks: every tile exactly once; a workgroup's tiles increase; after -1 a workgroup gets -1 for ever (the kernels stop
// at the first); G % 8 == 0: the tiles of the workgroups with equal b & 7 in one iteration are consecutive integers, in
// the order of b; other grids: tile = b + k G.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../blah2_amd/csrc/doppler_walk.hpp"

using blah2::doppler_walk_tile;

static int fails = 0;
#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      if (fails++ < 20) { std::printf("FAIL G=%d T=%d: ", G, T); std::printf(__VA_ARGS__); std::printf("\n"); }        \
    }                                                                                                                  \
  } while (0)

static void check(int G, int T)
{
  std::vector<int> seen(T, 0);
  int maxIter = 0;
  for (int b = 0; b < G; b++) {
    int last = -1, k = 0;
    for (;; k++) {
      const int it = doppler_walk_tile(b, G, k, T);
      if (it < 0) break;
      CHECK(it < T, "b=%d k=%d tile %d out of range", b, k, it);
      if (it >= T) break;
      CHECK(it > last, "b=%d k=%d tile %d after %d", b, k, it, last);
      if (G & 7) CHECK(it == b + k * G, "b=%d k=%d tile %d, old walk gives %d", b, k, it, b + k * G);
      seen[it]++;
      last = it;
      CHECK(k <= T, "b=%d does not stop", b);
      if (k > T) break;
    }
    if (k > maxIter) maxIter = k;
    for (int kk = k; kk < k + 3; kk++) CHECK(doppler_walk_tile(b, G, kk, T) < 0, "b=%d k=%d a tile after none", b, kk);
  }
  for (int t = 0; t < T; t++) CHECK(seen[t] == 1, "tile %d taken %d times", t, seen[t]);
  if ((G & 7) == 0)
    for (int k = 0; k < maxIter; k++)
      for (int x = 0; x < 8; x++) {
        int prev = -1;
        bool ended = false;
        for (int b = x; b < G; b += 8) {
          const int it = doppler_walk_tile(b, G, k, T);
          if (it < 0) { ended = true; continue; }
          CHECK(!ended, "label %d iteration %d: b=%d has a tile after a workgroup without one", x, k, b);
          CHECK(prev < 0 || it == prev + 1, "label %d iteration %d: b=%d tile %d after %d", x, k, b, it, prev);
          prev = it;
        }
      }
}

int main(int argc, char **argv)
{
  if (argc == 3) {
    const int G = std::atoi(argv[1]), T = std::atoi(argv[2]);
    if (G < 1 || T < 1) return 2;
    for (int b = 0; b < G; b++)
      for (int k = 0;; k++) {
        const int it = doppler_walk_tile(b, G, k, T);
        if (it < 0) break;
        std::printf("%d %d %d\n", b, k, it);
      }
    return 0;
  }
  const int tiles[] = {1, 7, 19, 56, 57, 511, 512, 513, 6656};
  int cases = 0;
  for (int T : tiles) {
    for (int G = 1; G <= 64; G++, cases++) check(G, T);
    for (int G = 72; G <= 512; G += 8, cases++) check(G, T);
  }
  if (fails) { std::printf("%d failures\n", fails); return 1; }
  std::printf("ok %d\n", cases);
  return 0;
}
