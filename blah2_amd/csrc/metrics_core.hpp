// The pieces of Map::set_metrics (Map.cpp:187-206) that every kernel with a fused metrics epilogue shares: the Doppler
// kernels of kernels.hpp and the beam former of beam_kernels.hpp.  Inline device functions only, no kernels: any unit may
// include it.
#pragma once

#include <hip/hip_runtime.h>

#include "fft_wg.hpp"

namespace blah2 {

// 10*log10|z| = 5*log10(re^2+im^2) = 5*log10(2) * log2(re^2+im^2)
__device__ __forceinline__ float db_of(cf z) { return 1.50514997831990597607f * log2f(z.x * z.x + z.y * z.y); }

// Map::set_metrics partial of one wave: the lanes' (sum of dB values, largest dB value) folded by a butterfly over the
// lane index, every lane ending with the wave's result.  One definition for every kernel that fuses the metrics, so
// the order of the additions -- and with it the bits of noisePower -- is the same whichever Doppler kernel ran.
__device__ __forceinline__ void wave_sum_max(double &lsum, float &lmax)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lsum += __shfl_xor(lsum, off);
    lmax = fmaxf(lmax, __shfl_xor(lmax, off));
  }
}

// sum / max over the 256 threads of a workgroup -> one partial per workgroup
__device__ __forceinline__ void block_metrics_partial(double lsum, float lmax, double *dst_sum, float *dst_max)
{
  __shared__ double wsum[4];
  __shared__ float wmax[4];
  wave_sum_max(lsum, lmax);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { wsum[wave] = lsum; wmax[wave] = lmax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    float m = 0.f; // Map.cpp:193: the running max starts at 0
    for (int w = 0; w < (int)(blockDim.x >> 6); w++) { s += wsum[w]; m = fmaxf(m, wmax[w]); }
    *dst_sum = s;
    *dst_max = m;
  }
}

} // namespace blah2
