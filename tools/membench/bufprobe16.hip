// bufprobe.hip for 2-BYTE accesses: what does buffer_load_ushort through a raw descriptor return on gfx950 for
// offsets around num_records, for "negative" (wrapped) voffsets, with the offset split between voffset / soffset /
// the immediate, and with a descriptor base that is only 2-byte aligned?  (The int8 sample format, csrc/bufload.hpp
// ChanI8, relies on the answers for its zero padding.)  Prints one line per case and a verdict per rule; exit
// status 0 only if every rule the kernels rely on holds.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

typedef int v4i __attribute__((ext_vector_type(4)));

// through the builtin (RawBuiltin<ChanI8>)
__global__ void probe(const unsigned short *buf, int base_half, unsigned *out, int nrec_bytes, const int *voffs, const int *soffs, int ncase)
{
  // base points 2048 halfwords (+ base_half) into the allocation so that small negative offsets stay inside it
  __amdgpu_buffer_rsrc_t d = __builtin_amdgcn_make_buffer_rsrc((void *)(buf + 2048 + base_half), (short)0, nrec_bytes, 0x00020000);
  for (int c = 0; c < ncase; c++) {
    const int vo = voffs[c], so = __builtin_amdgcn_readfirstlane(soffs[c]);
    out[c] = __builtin_amdgcn_raw_buffer_load_b16(d, vo, so, 0);
  }
}

// through the inline-asm form (ChanI8::ld), 1000 of the offset in the instruction's immediate
__global__ void probe_imm(const unsigned short *buf, int base_half, unsigned *out, int nrec_bytes, const int *voffs, const int *soffs, int ncase)
{
  const unsigned long long a = (unsigned long long)(buf + 2048 + base_half);
  v4i d;
  d.x = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
  d.y = __builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32)) & 0xffff;
  d.z = __builtin_amdgcn_readfirstlane(nrec_bytes);
  d.w = 0x00020000;
  for (int c = 0; c < ncase; c++) {
    const int vo = voffs[c] - 1000, so = __builtin_amdgcn_readfirstlane(soffs[c]);
    unsigned r = 0xdeadbeefu; // the upper half must come back zero
    asm volatile("buffer_load_ushort %0, %1, %2, %3 offen offset:1000\n\ts_waitcnt vmcnt(0)" : "+v"(r) : "v"(vo), "s"(d), "s"(so) : "memory");
    out[c] = r;
  }
}

// a whole wave as the kernels load a y window: lane t, load k reads sample dmin + t + 64 k (voffset (dmin + t) * 2, the
// 128 k in the immediate), through the builtin (form 0) and inline asm (form 1)
template <int K> __device__ void wave_asm(unsigned *out, v4i d, int vo)
{
  if constexpr (K < 16) {
    unsigned r = 0xdeadbeefu;
    asm volatile("buffer_load_ushort %0, %1, %2, 0 offen offset:%3\n\ts_waitcnt vmcnt(0)" : "+v"(r) : "v"(vo), "s"(d), "n"(K * 128) : "memory");
    out[K * 64 + threadIdx.x] = r;
    wave_asm<K + 1>(out, d, vo);
  }
}
__global__ void probe_wave(const unsigned short *buf, unsigned *out, int nrec_bytes, int dmin, int form)
{
  const unsigned long long a = (unsigned long long)(buf + 2048);
  int vo = (dmin + (int)threadIdx.x) * 2;
  asm volatile("" : "+v"(vo));
  if (form == 2) {
    __amdgpu_buffer_rsrc_t d = __builtin_amdgcn_make_buffer_rsrc((void *)(buf + 2048), (short)0, nrec_bytes, 0x00020000);
#pragma unroll
    for (int k = 0; k < 16; k++) {
      int o = vo + k * 128;
      asm volatile("" : "+v"(o));
      out[k * 64 + threadIdx.x] = __builtin_amdgcn_raw_buffer_load_b16(d, o, 0, 0);
    }
  } else if (form == 0) {
    __amdgpu_buffer_rsrc_t d = __builtin_amdgcn_make_buffer_rsrc((void *)(buf + 2048), (short)0, nrec_bytes, 0x00020000);
#pragma unroll
    for (int k = 0; k < 16; k++) out[k * 64 + threadIdx.x] = __builtin_amdgcn_raw_buffer_load_b16(d, vo + k * 128, 0, 0);
  } else {
    v4i d;
    d.x = __builtin_amdgcn_readfirstlane((int)(unsigned)a);
    d.y = __builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32)) & 0xffff;
    d.z = __builtin_amdgcn_readfirstlane(nrec_bytes);
    d.w = 0x00020000;
    wave_asm<0>(out, d, vo);
  }
}

int main()
{
  const int N = 1 << 16; // halfwords
  std::vector<unsigned short> h(N);
  for (int i = 0; i < N; i++) h[i] = (unsigned short)(0x8000u + i); // never 0: a zero is always the range check
  unsigned short *d;
  unsigned *o;
  int *dv, *ds;
  if (hipMalloc(&d, N * 2) != hipSuccess) { std::printf("no device\n"); return 2; }
  hipMalloc(&o, 256 * 4); hipMalloc(&dv, 256 * 4); hipMalloc(&ds, 256 * 4);
  hipMemcpy(d, h.data(), N * 2, hipMemcpyHostToDevice);
  // 2002 bytes: 1001 samples, the view ends MID-dword whatever the base alignment
  const int nrec = 2002;
  struct C { int vo, so; bool in; const char *what; bool rely = true; }; // rely false: reported, no kernel depends on it (y keeps its whole offset in voffset)
  const std::vector<C> cs = {
    {0, 0, true, "first"}, {2, 0, true, "second (odd halfword)"}, {1998, 0, true, "last whole dword's first half"},
    {2000, 0, true, "LAST sample, offset = num_records - 2"}, {2002, 0, false, "offset = num_records"},
    {2004, 0, false, "num_records + 2"}, {4096, 0, false, "far beyond"},
    {-2, 0, false, "voffset -2"}, {-4, 0, false, "voffset -4"}, {-82, 0, false, "voffset -82"},
    {-2, 2, false, "voffset -2 + soffset 2 (true offset 0)", false}, {-82, 1024, false, "voffset -82 + soffset 1024 (true offset 942)", false},
    {0, 2000, true, "soffset only, last sample"}, {0, 2002, false, "soffset only, = num_records"},
    {1000, 1000, true, "split, sum 2000 (last sample)"}, {1002, 1000, false, "split, sum 2002"}, {2, 8192, false, "soffset > num_records"},
  };
  std::vector<int> vo, so;
  for (auto &c : cs) { vo.push_back(c.vo); so.push_back(c.so); }
  hipMemcpy(dv, vo.data(), vo.size() * 4, hipMemcpyHostToDevice);
  hipMemcpy(ds, so.data(), so.size() * 4, hipMemcpyHostToDevice);
  std::vector<unsigned> r(256);
  int bad = 0;
  for (int base_half = 0; base_half < 2; base_half++) {
    for (int form = 0; form < 2; form++) {
      hipMemset(o, 0xFF, 256 * 4);
      if (form == 0) probe<<<1, 1>>>(d, base_half, o, nrec, dv, ds, (int)cs.size());
      else probe_imm<<<1, 1>>>(d, base_half, o, nrec, dv, ds, (int)cs.size());
      if (hipDeviceSynchronize() != hipSuccess) { std::printf("kernel failed: %s\n", hipGetErrorString(hipGetLastError())); return 2; }
      hipMemcpy(r.data(), o, 256 * 4, hipMemcpyDeviceToHost);
      std::printf("-- base %s-aligned, %s; num_records = %d bytes\n", base_half ? "2-byte" : "4-byte", form ? "inline asm, 1000 in the immediate" : "builtin", nrec);
      for (size_t c = 0; c < cs.size(); c++) {
        const unsigned want = cs[c].in ? (unsigned)h[2048 + base_half + (cs[c].vo + cs[c].so) / 2] : 0u;
        const bool ok = r[c] == want;
        bad += !ok && cs[c].rely;
        std::printf("voffset %6d soffset %6d : %08x (expected %08x) %s  %s\n", cs[c].vo, cs[c].so, r[c], want, ok ? "ok " : (cs[c].rely ? "BAD" : "differs (not relied on)"), cs[c].what);
      }
    }
  }
  unsigned *ow;
  hipMalloc(&ow, 1024 * 4);
  std::vector<unsigned> rw(1024);
  const int nrecw = 2 * 700; // 700 samples: the windows below run past both ends
  int split_bad = 0; // forms 0 and 1 are reported only: no kernel splits a possibly negative 2-byte offset
  for (int dmin : {-299, -256, -43, -10, 1})
    for (int form = 0; form < 3; form++) {
      hipMemset(ow, 0xFF, 1024 * 4);
      probe_wave<<<1, 64>>>(d, ow, nrecw, dmin, form);
      if (hipDeviceSynchronize() != hipSuccess) { std::printf("kernel failed: %s\n", hipGetErrorString(hipGetLastError())); return 2; }
      hipMemcpy(rw.data(), ow, 1024 * 4, hipMemcpyDeviceToHost);
      int wbad = 0, first = -1;
      for (int k = 0; k < 16; k++)
        for (int t = 0; t < 64; t++) {
          const int i = dmin + t + 64 * k;
          const unsigned want = (i >= 0 && i < 700) ? (unsigned)h[2048 + i] : 0u;
          if (rw[k * 64 + t] != want) { if (first < 0) first = k * 64 + t; wbad++; }
        }
      std::printf("wave window from sample %4d, %s: %d of 1024 differ", dmin, form == 2 ? "whole offset in voffset" : form ? "inline asm, 128 k in the immediate" : "builtin, 128 k in the immediate", wbad);
      if (first >= 0) std::printf(" (first: load %d lane %d sample %d got %08x)", first / 64, first % 64, dmin + first % 64 + 64 * (first / 64), rw[first]);
      std::printf("\n");
      if (form == 2) bad += wbad;
      else split_bad += wbad;
    }
  std::printf("negative voffset + immediate (not used by ChanI8): %d values differ\n", split_bad);
  std::printf(bad ? "%d cases differ from what csrc/bufload.hpp ChanI8 relies on\n"
                  : "all cases as ChanI8 relies on them: 2-byte granular range check, negative voffset out of range, upper half zero (%d)\n", bad);
  return bad ? 1 : 0;
}
