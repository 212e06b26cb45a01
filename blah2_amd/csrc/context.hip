// What every unit of the library leans on: the device context of the host classes, the thread's error string and the
// once-per-(device, kernel) LDS attribute.
#include "amb_handle.hpp"

#include <mutex>
#include <set>

using namespace blah2;

static thread_local std::string g_err;

extern "C" {

const char *blah2hip_last_error(void) { return g_err.c_str(); }

int blah2hip_device_count(int *count)
{
  if (!count) return fail(BLAH2HIP_ERR_INVALID, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *count = 0; return fail(BLAH2HIP_ERR_NO_DEVICE, hipGetErrorString(e)); }
  *count = n;
  return BLAH2HIP_OK;
}

// ---------------------------------------------------------- device context --
struct blah2hip_ctx_s {
  int device = 0;
  hipStream_t stream = nullptr;
};

int blah2hip_ctx_create(int device, blah2hip_ctx_t *out)
{
  if (!out) return fail(BLAH2HIP_ERR_INVALID, "out is NULL");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(BLAH2HIP_ERR_NO_DEVICE, "no HIP device visible (the HIP path is the only path)");
  if (device < 0 || device >= ndev) return fail(BLAH2HIP_ERR_INVALID, "device index out of range");
  HIPCHK(hipSetDevice(device));
  auto *c = new blah2hip_ctx_s;
  c->device = device;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) { delete c; return fail(BLAH2HIP_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e)); }
  *out = c;
  return BLAH2HIP_OK;
}

int blah2hip_ctx_destroy(blah2hip_ctx_t c)
{
  if (!c) return BLAH2HIP_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
  delete c;
  return BLAH2HIP_OK;
}

void *blah2hip_ctx_stream(blah2hip_ctx_t c) { return c ? (void *)c->stream : nullptr; }

int blah2hip_ctx_sync(blah2hip_ctx_t c)
{
  if (!c) return fail(BLAH2HIP_ERR_INVALID, "NULL context");
  HIPCHK(hipStreamSynchronize(c->stream));
  return BLAH2HIP_OK;
}

int blah2hip_ctx_malloc(blah2hip_ctx_t c, size_t bytes, void **dptr)
{
  if (!c || !dptr) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMalloc(dptr, bytes));
  return BLAH2HIP_OK;
}

int blah2hip_ctx_free(blah2hip_ctx_t c, void *dptr)
{
  if (!c) return fail(BLAH2HIP_ERR_INVALID, "NULL context");
  if (dptr) { HIPCHK(hipSetDevice(c->device)); HIPCHK(hipFree(dptr)); }
  return BLAH2HIP_OK;
}

int blah2hip_ctx_malloc_host(blah2hip_ctx_t c, size_t bytes, void **hptr)
{
  if (!c || !hptr) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipHostMalloc(hptr, bytes, hipHostMallocDefault));
  return BLAH2HIP_OK;
}

int blah2hip_ctx_free_host(blah2hip_ctx_t c, void *hptr)
{
  if (!c) return fail(BLAH2HIP_ERR_INVALID, "NULL context");
  if (hptr) HIPCHK(hipHostFree(hptr));
  return BLAH2HIP_OK;
}

int blah2hip_ctx_h2d(blah2hip_ctx_t c, void *dptr, const void *hptr, size_t bytes)
{
  if (!c || !dptr || !hptr) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(dptr, hptr, bytes, hipMemcpyHostToDevice, c->stream));
  return BLAH2HIP_OK;
}

int blah2hip_ctx_d2d(blah2hip_ctx_t c, void *dst, const void *src, size_t bytes)
{
  if (!c || !dst || !src) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
  return BLAH2HIP_OK;
}

int blah2hip_ctx_d2h(blah2hip_ctx_t c, void *hptr, const void *dptr, size_t bytes)
{
  if (!c || !dptr || !hptr) return fail(BLAH2HIP_ERR_INVALID, "NULL argument");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(hptr, dptr, bytes, hipMemcpyDeviceToHost, c->stream));
  return BLAH2HIP_OK;
}

// A streaming read of `bytes` of device memory and nothing else (16-byte loads, four in flight per lane, the sum kept
// behind a condition that never holds): what the memory system delivers to a kernel that only reads, the ceiling the
// range kernel's loads are priced against beside the copy (bench.py `roofline.read_ceiling`).
typedef float v4f_t __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void stream_read_kernel(const v4f_t *__restrict__ src, size_t n16, float *sink)
{
  // a workgroup takes contiguous 64 KB chunks (16 loads of 16 bytes per lane, all requested before the first is used:
  // the shape tools/membench measured at 6.3 TB/s), chunk c + k * gridDim.x
  constexpr size_t CH = 16 * 256;
  float acc = 0.f;
  const size_t nch = n16 / CH;
  for (size_t c = blockIdx.x; c < nch; c += gridDim.x) {
    const v4f_t *p = src + c * CH + threadIdx.x;
    v4f_t v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) v[k] = __builtin_nontemporal_load(p + 256 * k);
#pragma unroll
    for (int k = 0; k < 16; k++) acc += (v[k].x + v[k].y) + (v[k].z + v[k].w);
  }
  for (size_t i = nch * CH + (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) {
    const v4f_t a = src[i];
    acc += a.x + a.y + a.z + a.w;
  }
  if (acc == 1.2345678e-30f && sink) *sink = acc;
}

int blah2hip_stream_read_dev(const void *d_src, size_t bytes, void *d_sink, void *stream)
{
  if (!d_src || ((uintptr_t)d_src & 15)) return fail(BLAH2HIP_ERR_INVALID, "stream_read_dev: source NULL or not 16-byte aligned");
  int dev = 0, cus = 256;
  HIPCHK(hipGetDevice(&dev));
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  stream_read_kernel<<<dim3(cus * 6), dim3(256), 0, (hipStream_t)stream>>>((const v4f_t *)d_src, bytes / 16, (float *)d_sink);
  HIPCHK(hipGetLastError());
  return BLAH2HIP_OK;
}

// ------------------------------------------------------- internal hooks --
// every unit reports errors here (fail() in amb_handle.hpp, CFAIL / CHIP in clutter_handle.hpp; spectrum.hip and capture.hip call it directly)
void blah2hip_set_error_(const char *msg) { g_err = msg ? msg : ""; }

hipError_t blah2hip_ensure_lds_(const void *kern, int bytes)
{
  static std::mutex mu;
  static std::set<std::pair<int, const void *>> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(mu);
  if (done.count({dev, kern})) return hipSuccess;
  e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.insert({dev, kern});
  return e;
}

} // extern "C"
