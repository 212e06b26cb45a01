// De-blocking of USRP captures on gfx950 (include/blah2hip.h, blah2hip_deblock_c32_dev).
//
// Reference: blah2's src/capture/usrp/Usrp.cpp:29-104.  The driver receives a two-channel fc32 stream and,
// with save.iq on, writes per recv() call samps_per_buff complex<float> of channel 0 (x, the reference channel) and
// then samps_per_buff of channel 1 (y, the surveillance channel):
//
//   file = [ x block 0 | y block 0 | x block 1 | y block 1 | ... ]      a block: B complex<float>
//   sample s of channel c is complex value (s / B) * 2B + c * B + s % B of the file
//
// blah2.cpp:250-258 cuts CPI k as samples [k n, (k+1) n) of each channel, so a CPI starts and ends mid-block.  The
// kernel writes the two complex-fp32 planes of BLAH2HIP_FMT_C32 for a batch of CPIs out of the batch's raw bytes: a
// streaming copy, 8 bytes read and 8 written per sample and channel.  Values are copied bit for bit.
//
// Work split: a workgroup of 256 lanes owns DB_CHUNK consecutive items of one CPI's row, an item being one sample
// (8-byte path) or two (16-byte path; B, first, n and the stride even, so a pair never straddles a block and stays
// 16-byte aligned on both sides).  Each lane loads all of its items of both channels before it stores any.
#include <hip/hip_runtime.h>

#include "blah2hip.h"

#include <cstdint>
#include <string>

namespace {

typedef float v2f_t __attribute__((ext_vector_type(2)));
typedef float v4f_t __attribute__((ext_vector_type(4)));

constexpr int DB_THREADS = 256;
constexpr int DB_ITEMS = 4;  // items per lane and channel: 8 loads in flight before the first store
constexpr uint32_t DB_CHUNK = DB_THREADS * DB_ITEMS;

struct DeblockArgs {
  uint64_t first;      // sample offset of CPI 0 within the buffer
  uint64_t n;          // samples per CPI
  uint64_t stride;     // plane elements between CPIs
  uint64_t block;      // B
  uint32_t items;      // items per row (n, or n / 2 on the 16-byte path)
  uint32_t chunks;     // workgroups per row
};

// (s / B, s % B) with a 32-bit division whenever s fits, which is every realistic capture offset
__device__ __forceinline__ void divmod(uint64_t s, uint64_t b, uint64_t &q, uint64_t &r)
{
  if ((s >> 32) == 0 && (b >> 32) == 0) {
    const uint32_t s32 = (uint32_t)s, b32 = (uint32_t)b;
    const uint32_t q32 = s32 / b32;
    q = q32;
    r = s32 - q32 * b32;
  } else {
    q = s / b;
    r = s - q * b;
  }
}

// T = v2f_t (one sample per item) or v4f_t (two); W = samples per item
template <class T, int W>
__global__ __launch_bounds__(DB_THREADS) void deblock_kernel(const T *__restrict__ raw, T *__restrict__ x,
                                                             T *__restrict__ y, DeblockArgs a)
{
  const uint32_t row = blockIdx.x / a.chunks;
  const uint32_t chunk = blockIdx.x - row * a.chunks;
  // the row's first sample, split once per lane: s = (row start) + W * item = base + W * item, base = q0 * B + r0
  uint64_t q0, r0;
  divmod(a.first + (uint64_t)row * a.n, a.block, q0, r0);
  const uint64_t bw = a.block / W;  // block length in items (W divides B on the 16-byte path)
  T vx[DB_ITEMS], vy[DB_ITEMS];
  uint64_t it[DB_ITEMS];
#pragma unroll
  for (int k = 0; k < DB_ITEMS; k++) {
    it[k] = (uint64_t)chunk * DB_CHUNK + k * DB_THREADS + threadIdx.x;
    if (it[k] < a.items) {
      uint64_t q, r;
      divmod(r0 / W + it[k], bw, q, r);  // r0 is a multiple of W on the 16-byte path
      const uint64_t e = (q0 + q) * 2 * bw + r;  // x item of the sample in units of T; y is bw further
      vx[k] = __builtin_nontemporal_load(raw + e);
      vy[k] = __builtin_nontemporal_load(raw + e + bw);
    }
  }
  const uint64_t o = (uint64_t)row * (a.stride / W);
#pragma unroll
  for (int k = 0; k < DB_ITEMS; k++) {
    if (it[k] < a.items) {
      x[o + it[k]] = vx[k];
      y[o + it[k]] = vy[k];
    }
  }
}

} // namespace

extern "C" void blah2hip_set_error_(const char *msg);

extern "C" int blah2hip_deblock_c32_dev(const void *d_raw, uint32_t block, uint64_t first, uint32_t n_samples,
                                        uint32_t n_cpi, void *d_x, void *d_y, uint64_t cpi_stride, void *stream)
{
  if (!d_raw || !d_x || !d_y) {
    blah2hip_set_error_("deblock_c32_dev: NULL pointer");
    return BLAH2HIP_ERR_INVALID;
  }
  if (block == 0 || n_samples == 0) {
    blah2hip_set_error_("deblock_c32_dev: block and n_samples must be positive");
    return BLAH2HIP_ERR_INVALID;
  }
  if (n_cpi > 1 && cpi_stride < n_samples) {
    blah2hip_set_error_("deblock_c32_dev: cpi_stride < n_samples would overlap the CPIs' rows");
    return BLAH2HIP_ERR_INVALID;
  }
  if (n_cpi == 0) return BLAH2HIP_OK;
  const bool aligned = (((uintptr_t)d_raw | (uintptr_t)d_x | (uintptr_t)d_y) & 15) == 0;
  const bool wide = aligned && block % 2 == 0 && first % 2 == 0 && n_samples % 2 == 0 && (n_cpi == 1 || cpi_stride % 2 == 0);
  DeblockArgs a{};
  a.first = first;
  a.n = n_samples;
  a.stride = n_cpi > 1 ? cpi_stride : 0;
  a.block = block;
  a.items = wide ? n_samples / 2 : n_samples;
  a.chunks = (uint32_t)(((uint64_t)a.items + DB_CHUNK - 1) / DB_CHUNK);
  const uint64_t blocks = (uint64_t)a.chunks * n_cpi;
  if (blocks > 0x7fffffffull) {
    blah2hip_set_error_("deblock_c32_dev: batch too large for one launch");
    return BLAH2HIP_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)stream;
  if (wide)
    deblock_kernel<v4f_t, 2><<<dim3((uint32_t)blocks), dim3(DB_THREADS), 0, st>>>((const v4f_t *)d_raw, (v4f_t *)d_x,
                                                                                  (v4f_t *)d_y, a);
  else
    deblock_kernel<v2f_t, 1><<<dim3((uint32_t)blocks), dim3(DB_THREADS), 0, st>>>((const v2f_t *)d_raw, (v2f_t *)d_x,
                                                                                  (v2f_t *)d_y, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    blah2hip_set_error_((std::string("deblock_kernel launch: ") + hipGetErrorString(e)).c_str());
    return BLAH2HIP_ERR_HIP;
  }
  return BLAH2HIP_OK;
}
