// Trace builds only (-DRANGEW_TRACE / -DDOPW_TRACE / -DC2T_TRACE, tools/build_trace.sh): the per-phase s_memtime ticks a
// kernel's waves collect are added into a device global and printed by the kernel itself (every 8th launch: the totals so
// far, as fractions).  Nothing of it appears in a kernel signature or an argument struct; without the macros this header
// is empty.
// -DRANGEW_TRACE also keeps, for the last RW_EXIT_RING launches of rangew1k_kernel, every wave's start and exit time
// (wall_clock64, one clock for the whole device) and the number of pulses it ran: how far behind the first exit the launch
// ends is what a dynamic pulse walk could win.  The one piece of host code: trace_rw_dump(), called when a handle is
// destroyed, writes the ring to the file BLAH2HIP_TRACE_EXITS names (tools/range_walk_spread.py reads it).
#pragma once
#if defined(RANGEW_TRACE) || defined(DOPW_TRACE) || defined(C2T_TRACE)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
namespace blah2 {
// (internal linkage: more than one unit includes this header, and the kernels of one trace macro sit in one unit)
static __device__ unsigned long long trace_buckets[16];
static __device__ unsigned int trace_launches;
// one lane per wave: its buckets; the first wave of the launch also counts the launch and prints every 8th
template <int N> __device__ __forceinline__ void trace_finish(const char *tag, const uint64_t (&tr)[N], bool first_wave_of_grid)
{
  for (int k = 0; k < N; k++) atomicAdd(&trace_buckets[k], (unsigned long long)tr[k]);
  if (first_wave_of_grid && (atomicAdd(&trace_launches, 1u) & 7u) == 7u) {
    double tot = 0;
    for (int k = 0; k < N; k++) tot += (double)trace_buckets[k];
    printf("[%s trace] buckets:", tag);
    for (int k = 0; k < N; k++) printf(" %.3f", (double)trace_buckets[k] / tot);
    printf(" of %.3e ticks (waves that have finished so far, %u launches)\n", tot, trace_launches);
  }
}
#ifdef RANGEW_TRACE
constexpr int RW_EXIT_RING = 8, RW_EXIT_WAVES = 4096;
struct RwExit { unsigned long long start, exit; unsigned pulses, xcd; };
static __device__ RwExit trace_rw_exit[RW_EXIT_RING][RW_EXIT_WAVES];
static __device__ unsigned trace_rw_waves[RW_EXIT_RING]; // waves of the launch in that slot
static __device__ unsigned trace_rw_exited, trace_rw_launch;
// one lane per wave, every wave of the launch (also those without a pulse): the last one closes the launch's slot
__device__ __forceinline__ void trace_rw_leave(unsigned wave, unsigned waves, unsigned long long start, unsigned pulses)
{
  const unsigned slot = __hip_atomic_load(&trace_rw_launch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) % RW_EXIT_RING;
  if (wave < (unsigned)RW_EXIT_WAVES) {
    RwExit &r = trace_rw_exit[slot][wave];
    r.start = start;
    r.pulses = pulses;
    r.xcd = blockIdx.x & 7;
    r.exit = wall_clock64();
  }
  if (__hip_atomic_fetch_add(&trace_rw_exited, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == waves) {
    trace_rw_waves[slot] = waves;
    __hip_atomic_store(&trace_rw_exited, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&trace_rw_launch, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
// host: "slot waves wave xcd pulses start exit" per line (ticks of the device's wall clock, kHz in the header line)
inline void trace_rw_dump()
{
  const char *path = getenv("BLAH2HIP_TRACE_EXITS");
  if (!path || !*path) return;
  static RwExit rec[RW_EXIT_RING][RW_EXIT_WAVES];
  unsigned waves[RW_EXIT_RING], launches = 0;
  int dev = 0, khz = 0;
  if (hipDeviceSynchronize() != hipSuccess || hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess ||
      hipMemcpyFromSymbol(rec, HIP_SYMBOL(trace_rw_exit), sizeof(rec)) != hipSuccess ||
      hipMemcpyFromSymbol(waves, HIP_SYMBOL(trace_rw_waves), sizeof(waves)) != hipSuccess ||
      hipMemcpyFromSymbol(&launches, HIP_SYMBOL(trace_rw_launch), sizeof(launches)) != hipSuccess)
    return;
  if (!launches) return; // a handle that never ran the kernel keeps an earlier handle's file
  FILE *f = fopen(path, "w");
  if (!f) return;
  fprintf(f, "# wall_clock_khz %d launches %u\n", khz, launches);
  for (int s = 0; s < RW_EXIT_RING; s++) {
    if (launches < (unsigned)RW_EXIT_RING && (unsigned)s >= launches) continue;
    for (unsigned w = 0; w < waves[s] && w < (unsigned)RW_EXIT_WAVES; w++)
      fprintf(f, "%d %u %u %u %u %llu %llu\n", s, waves[s], w, rec[s][w].xcd, rec[s][w].pulses, rec[s][w].start, rec[s][w].exit);
  }
  fclose(f);
}
#endif
} // namespace blah2
#endif
