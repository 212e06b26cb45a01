// Host build of rangew1k_kernel's ticketed pulse walk (blah2_amd/csrc/range_walk.hpp), pulled the way the kernel pulls it:
// the 12 waves of workgroup b start at head b & 7, take their first pulse with range_walk_next(), request the ticket
// for every further pulse AHEAD of its use (one fetch-and-add on the current head, the kernel's range_walk_request) and
// hand it to range_walk_next() later; a wave that gets -1 counts itself out on the exit word and the last one zeroes the
// nine words.
//   emulate_range_walk              every nPulses below x every grid below x every order of pulls; prints "ok <cases>"
//   emulate_range_walk G N ORDER    prints "workgroup wave pulse" for every pulse handed out, in the order of the pulls
// Orders of the pulls (the waves are independent: any interleaving of their atomics can happen on the chip):
//   0  in step: every wave takes a pulse, in the order of (workgroup, wave), then every wave requests its next ticket,
//      round after round -- no skew
//   1  in step, in the reverse order
//   2  pseudo-random wave at every step, a request and its use any number of steps apart, and pseudo-random other waves
//      running in the middle of a wave's head search
//   3  wave 0 runs until it has nothing left, then wave 1, ... (one wave empties all eight heads)
//   4  the same from the last wave down
// Checks: every pulse in [0, nPulses) exactly once, never one outside; every wave ends after at most nPulses + 1 calls,
// each of at most 8 pulls; a wave that got -1 gets -1 again; no head is pulled more often than its pulses + the
// launch's waves (a 32-bit word cannot wrap); the exit word reaches the number of waves once and the reset leaves nine
// zeros; order 0: the first min(G, blocks) blocks of 12 pulses go to the workgroups the static walk gives them to, wave w
// of workgroup b to pulse 12 b + w.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../blah2_amd/csrc/range_walk.hpp"

using namespace blah2;

static int fails = 0;
#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      if (fails++ < 20) { std::printf("FAIL G=%d N=%d order=%d: ", G, N, order); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                                                                                  \
  } while (0)

struct Wave {
  int head = 0;
  bool started = false, done = false, have = false, busy = false;
  uint32_t ticket = 0;
  int calls = 0;
};

struct Launch {
  int G, N, order;
  bool print;
  std::vector<uint32_t> words;
  std::vector<Wave> waves;
  std::vector<int> seen, owner;
  uint64_t rng = 0x2545F4914F6CDD1Dull;
  int depth = 0;
  int resets = 0;

  Launch(int G_, int N_, int order_, bool print_)
      : G(G_), N(N_), order(order_), print(print_), words(RWALK_WORDS, 0u), waves((size_t)G_ * RWALK_BLOCK), seen(N_, 0), owner(N_, -1)
  {
    for (size_t w = 0; w < waves.size(); w++) waves[w].head = (int)(w / RWALK_BLOCK) & (RWALK_HEADS - 1);
  }
  uint32_t rnd() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)(rng >> 32); }
  uint32_t fetch_add(int word) { return words[word]++; }

  // one step of wave w: its next pulse (the kernel: at the start, then once per pulse)
  void step(int w)
  {
    Wave &v = waves[w];
    if (v.done || v.busy) return; // (busy: order 2 came back to a wave in the middle of its own search)
    if (v.started && !v.have) { // the ticket for this pulse has not been requested yet: that is this step
      v.ticket = fetch_add(range_walk_head_word(v.head));
      v.have = true;
      if (order == 2) return; // on its own in the random order; the others request and use back to back
    }
    v.busy = true;
    auto pull = [&](int x) {
      // order 2: other waves run between two pulls of this wave's search
      if (order == 2 && depth < 3 && (rnd() & 3) == 0) {
        depth++;
        step((int)(rnd() % waves.size()));
        depth--;
      }
      return fetch_add(range_walk_head_word(x));
    };
    const int pulse = v.started ? range_walk_next(v.head, N, pull, v.have, v.ticket) : range_walk_next(v.head, N, pull);
    v.busy = false;
    v.started = true;
    v.have = false;
    v.calls++;
    CHECK(v.calls <= N + 1, "wave %d does not stop", w);
    CHECK(v.head >= 0 && v.head < RWALK_HEADS, "wave %d at head %d", w, v.head);
    if (pulse < 0 || v.calls > N + 1) {
      v.done = true;
      // nothing left for this wave: a further search finds nothing either
      int h2 = v.head;
      auto pull2 = [&](int x) { return fetch_add(range_walk_head_word(x)); };
      CHECK(range_walk_next(h2, N, pull2) < 0, "wave %d: a pulse after none", w);
      if (fetch_add(RWALK_EXIT_WORD) + 1u == (uint32_t)waves.size()) { // the kernel's range_walk_leave
        check_heads();
        for (int x = 0; x <= RWALK_HEADS; x++) words[x * RWALK_LINE_WORDS] = 0u;
        resets++;
      }
      return;
    }
    CHECK(pulse < N, "wave %d got pulse %d", w, pulse);
    if (pulse >= N) return;
    seen[pulse]++;
    owner[pulse] = w;
    if (print) std::printf("%d %d %d\n", w / RWALK_BLOCK, w % RWALK_BLOCK, pulse);
  }
  // orders 0 and 1: all waves request the ticket for their next pulse, as far ahead of its use as a whole round
  void request(int w)
  {
    Wave &v = waves[w];
    if (v.done || !v.started || v.have) return;
    v.ticket = fetch_add(range_walk_head_word(v.head));
    v.have = true;
  }
  void check_heads()
  {
    const int64_t blocks = ((int64_t)N + RWALK_BLOCK - 1) / RWALK_BLOCK;
    for (int x = 0; x < RWALK_HEADS; x++) {
      const int64_t mine = ((blocks - x + RWALK_HEADS - 1) / RWALK_HEADS) * RWALK_BLOCK; // an upper bound of head x's pulses
      // every wave pulls an exhausted head at most twice (its search, and the check above), plus one ticket ahead
      CHECK((int64_t)words[range_walk_head_word(x)] <= mine + 3 * (int64_t)waves.size(), "head %d pulled %u times", x, words[range_walk_head_word(x)]);
    }
  }
  bool live() const
  {
    for (const Wave &v : waves)
      if (!v.done) return true;
    return false;
  }
  void run()
  {
    const int W = (int)waves.size();
    if (order == 0 || order == 1) {
      while (live()) {
        for (int j = 0; j < W; j++) step(order == 0 ? j : W - 1 - j);
        for (int j = 0; j < W; j++) request(order == 0 ? j : W - 1 - j);
      }
    } else if (order == 2) {
      int guard = 0;
      while (live()) {
        step((int)(rnd() % W));
        if (++guard > 64 * (N + W)) { // the random pick has left few waves alive: finish them in order
          for (int j = 0; j < W; j++)
            while (!waves[j].done) step(j);
        }
      }
    } else {
      for (int j = 0; j < W; j++) {
        const int w = order == 3 ? j : W - 1 - j;
        while (!waves[w].done) step(w);
      }
    }
    for (int p = 0; p < N; p++) CHECK(seen[p] == 1, "pulse %d handed out %d times", p, seen[p]);
    CHECK(resets == 1, "%d resets", resets);
    for (int x = 0; x <= RWALK_HEADS; x++) CHECK(words[x * RWALK_LINE_WORDS] == 0u, "word %d not zero after the launch", x);
    for (size_t k = 0; k < words.size(); k++)
      if (k % RWALK_LINE_WORDS) CHECK(words[k] == 0u, "word %zu between the lines written", k);
    if (order == 0) {
      const int blocks = (N + RWALK_BLOCK - 1) / RWALK_BLOCK;
      for (int b = 0; b < G && b < blocks; b++)
        for (int w = 0; w < RWALK_BLOCK && b * RWALK_BLOCK + w < N; w++)
          CHECK(owner[b * RWALK_BLOCK + w] == b * RWALK_BLOCK + w, "pulse %d went to wave %d, not to its static owner", b * RWALK_BLOCK + w,
                owner[b * RWALK_BLOCK + w]);
    }
  }
};

int main(int argc, char **argv)
{
  if (argc == 4) {
    const int G = std::atoi(argv[1]), N = std::atoi(argv[2]), order = std::atoi(argv[3]);
    if (G < 1 || N < 1 || order < 0 || order > 4) return 2;
    Launch l(G, N, order, true);
    l.run();
    return fails ? 1 : 0;
  }
  const int pulses[] = {1, 5, 11, 12, 13, 95, 96, 97, 603, 1026, 131328};
  const int grids[] = {1, 2, 3, 7, 8, 9, 16, 24, 256};
  int cases = 0;
  for (int N : pulses)
    for (int G : grids)
      for (int order = 0; order < 5; order++, cases++) {
        Launch l(G, N, order, false);
        l.run();
      }
  // the formula on its own: ticket -> pulse is a bijection of (head, ticket) onto the integers, block by block
  {
    const int G = 0, N = 0, order = -1;
    for (uint32_t k = 0; k < 100; k++)
      for (int x = 0; x < RWALK_HEADS; x++) {
        const int64_t p = range_walk_pulse(x, k);
        CHECK(p / RWALK_BLOCK % RWALK_HEADS == x && p % RWALK_BLOCK == k % RWALK_BLOCK && p / (RWALK_BLOCK * RWALK_HEADS) == k / RWALK_BLOCK,
              "head %d ticket %u -> %lld", x, k, (long long)p);
      }
    CHECK(range_walk_pulse(7, 0xffffffffu) > (int64_t)0x7fffffff, "the largest ticket wraps");
  }
  if (fails) { std::printf("%d failures\n", fails); return 1; }
  std::printf("ok %d\n", cases);
  return 0;
}
