// The tile walk of the persistent Doppler kernels at nD <= 513 (doppler_pfa513_kernel, doppler_tile1k_kernel,
// doppler_tile_kernel): which tile workgroup b of a grid of G takes in its k-th iteration.  Host and device code; an
// index map and nothing more -- no workgroup ever waits for another.
//
// Why it is not b + k G: rows of the final map are nDelay * 8 bytes (3288 at configs[1]), no multiple of 128, so a
// tile's 128-byte row piece straddles two lines and every line is shared by the tiles s and s + 1.  Workgroups are dealt
// round-robin over the eight XCDs (b & 7: observed, a label for speed and never for correctness), so with b + k G the
// two halves of each line are written through two different L2s and leave as two partial lines.  Here the workgroups of
// one label take CONSECUTIVE tiles in the same iteration, and a label keeps one contiguous range of tiles over its
// iterations: the neighbours of a line sit in one L2 at about the same time and the pieces can merge before they leave.
//   label x = b & 7, slot s = b >> 3, S = G / 8 slots per label, C = ceil(T / 8) tiles per label:
//   tile = x C + k S + s   while k S + s < C and tile < T.
// (The interleaved form, tile = k G + x S + s, merged no better and ran 3 % slower: DESIGN.md section 7 item 5b.)
// Grids that are no multiple of 8 (forced ones; launches with fewer tiles than resident workgroups) keep b + k G.
// Every tile comes up exactly once, a workgroup's tiles increase with k, and once a workgroup has no tile it has none
// for any later k (tests/host/emulate_walk.cpp).
#pragma once

#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#define B2_HD __host__ __device__ __forceinline__
#else
#define B2_HD inline
#endif

namespace blah2 {

// tile of workgroup b (of G) in iteration k, of T tiles; -1: none
B2_HD int doppler_walk_tile(int b, int G, int k, int T)
{
  if (G & 7) {
    const long long it = (long long)b + (long long)k * G;
    return it < T ? (int)it : -1;
  }
  const int x = b & 7, s = b >> 3, S = G >> 3;
  const int C = (T + 7) >> 3;
  const long long j = (long long)k * S + s; // position inside the label's range
  if (j >= C) return -1;
  const long long it = (long long)x * C + j;
  return it < T ? (int)it : -1;
}

} // namespace blah2
