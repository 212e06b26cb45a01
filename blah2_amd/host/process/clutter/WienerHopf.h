// WienerHopf: least-squares FIR clutter canceller (reference surface:
// src/process/clutter/WienerHopf.h:68-78).  process() reads x, replaces the
// contents of y with the filtered surveillance channel and returns true; when
// the normal equations are not positive definite it returns false and leaves
// y alone (the caller then skips the CPI, blah2.cpp:270-273).
#ifndef BLAH2HIP_HOST_WIENERHOPF_H
#define BLAH2HIP_HOST_WIENERHOPF_H

#include "data/IqData.h"

#include <stdint.h>
#include <vector>

struct blah2hip_clutter_s;

class WienerHopf
{
public:
  // nBlocks > 1: taps per block of nSamples / nBlocks samples, the filter's history carried across the block edges
  // (blah2hip_clutter_create_ex); process() returns false when any block's normal equations are not positive definite
  WienerHopf(int32_t delayMin, int32_t delayMax, uint32_t nSamples, uint32_t nBlocks = 1);
  ~WienerHopf();
  WienerHopf(const WienerHopf &) = delete;
  WienerHopf &operator=(const WienerHopf &) = delete;

  bool process(IqData *x, IqData *y);

private:
  blah2hip_clutter_s *engine = nullptr;
  uint32_t nSamples, nBlocks;
  int32_t *dOk = nullptr, *hOk = nullptr; // device flags (one per block) and their pinned host copy
};

#endif
