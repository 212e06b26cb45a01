// The ticketed pulse walk of rangew1k_kernel: which pulse a ticket stands for, and where a wave pulls next.  Host and
// device code; index arithmetic and nothing more -- the atomics that hand the tickets out are the caller's.
//
// Why.  The static walk gives wave w of workgroup b the pulses b*12 + w + k*G*12: every wave has its share fixed at launch,
// and the launch ends with the slowest wave and a last round that is only partly full.  Here a wave takes its next pulse
// from a counter when it needs one, so the launch ends within a pulse of the moment the work runs out.
//
// The pulses are cut into blocks of RWALK_BLOCK = 12 consecutive ones (a workgroup's waves); head x of RWALK_HEADS = 8
// hands out the blocks whose index is = x mod 8, in order:
//   ticket k of head x  ->  pulse ((k / 12) * 8 + x) * 12 + k % 12.
// A workgroup starts at head blockIdx.x & 7 (the XCD it is observed to run on: a label for speed, never for
// correctness), so the first G*12 tickets cover the pulses the static walk's first round covers and the chip keeps
// working on one contiguous window of the input.  Eight heads because one word saturates near 88 returning atomics
// per microsecond and the headline pulls 67.
// A ticket whose pulse is >= nPulses says the head is exhausted (it stays exhausted: tickets only grow); the wave moves to
// head (x + 1) & 7, and after RWALK_HEADS exhausted heads in a row it has no pulse left.  Heads no workgroup starts at
// (grids below 8) are emptied this way.  Every pulse comes up exactly once, whatever the order of the pulls
// (tests/host/emulate_range_walk.cpp).
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#define B2_RW_HD __host__ __device__ __forceinline__
#else
#define B2_RW_HD inline
#endif

namespace blah2 {

constexpr int RWALK_HEADS = 8;
constexpr int RWALK_BLOCK = 12;      // = RANGEW1K_WAVES
constexpr int RWALK_LINE_WORDS = 32; // each counter on a 128-byte line of its own
constexpr int RWALK_EXIT_WORD = RWALK_HEADS * RWALK_LINE_WORDS;
constexpr int RWALK_WORDS = (RWALK_HEADS + 1) * RWALK_LINE_WORDS; // the per-handle buffer: eight heads, one exit counter

// word of head x inside the buffer
B2_RW_HD int range_walk_head_word(int x) { return x * RWALK_LINE_WORDS; }

// pulse of ticket k of head x (64-bit: tickets past the end of a long launch must not wrap)
B2_RW_HD int64_t range_walk_pulse(int x, uint32_t k)
{
  return ((int64_t)(k / RWALK_BLOCK) * RWALK_HEADS + x) * RWALK_BLOCK + k % RWALK_BLOCK;
}

// The next pulse of a wave whose current head is `head`, or -1 when all heads are exhausted.  pull(x) takes one ticket
// of head x (a returning fetch-and-add of 1).  `head` moves on to the head the pulse came from.
// `first`: a ticket of `head` the caller has already taken (requested ahead of its use), tried before any pull.
template <class Pull> B2_RW_HD int range_walk_next(int &head, int nPulses, Pull &&pull, bool haveFirst = false, uint32_t first = 0)
{
  // (a loop, not eight copies: the search runs once per wave at the end of a launch and must not shape the kernel around it)
#if defined(__clang__)
#pragma nounroll
#endif
  for (int tries = 0; tries < RWALK_HEADS; tries++) {
    const uint32_t k = (haveFirst && tries == 0) ? first : pull(head);
    const int64_t pulse = range_walk_pulse(head, k);
    if (pulse < nPulses) return (int)pulse;
    head = (head + 1) & (RWALK_HEADS - 1);
  }
  return -1;
}

} // namespace blah2
