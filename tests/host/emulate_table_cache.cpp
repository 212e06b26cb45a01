// Host build of the detectors' table-cache policy (blah2_amd/csrc/table_cache.hpp) on its own, without the library and
// without a GPU: the cache drives a fake device that records every call and keeps its "device" tables on the heap, so a
// leak, a double free or a read of an evicted table is the sanitizers' to report.
//   emulate_table_cache OP...     one list with integer keys; after every OP one line
//       OP rc=RC out=VALUE|- events=E,E,... list=KEY[p],... live=N built=N err=TEXT
//     gK  get key K                 GK  get key K, served by any entry with a key >= K (the averaging tables' rule)
//     pK  get key K and pin it      cK  get key K on a stream that is being captured
//     bK  get key K, the builder fails with rc -7
//     aK / uK / sK  get key K; the allocation / the upload / the synchronisation fails
//     f   free_all
// VALUE is the first word of the table handed out (the builder writes 1000 + K), `events` the device calls the OP made,
// `list` the entries least recently used first (p: pinned), `live` the device allocations that are not freed, `built` the
// builder's calls so far.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../blah2_amd/csrc/table_cache.hpp"

static std::string last_error;
extern "C" void blah2hip_set_error_(const char *msg) { last_error = msg; }

struct FakeDevice {
  std::vector<std::string> events;
  std::set<double *> live;
  bool failAlloc = false, failUpload = false, failSync = false, isCapturing = false;
  const char *alloc(size_t bytes, double **d)
  {
    events.push_back("alloc" + std::to_string(bytes));
    if (failAlloc) return "out of memory";
    *d = new double[bytes / sizeof(double)];
    live.insert(*d);
    return nullptr;
  }
  const char *upload(double *d, const double *host, size_t bytes)
  {
    events.push_back("upload");
    if (!live.count(d)) std::abort();
    if (failUpload) return "upload refused";
    std::memcpy(d, host, bytes);
    return nullptr;
  }
  bool free(double *d)
  {
    events.push_back("free");
    if (!live.erase(d)) std::abort(); // not allocated, or freed twice
    delete[] d;
    return true;
  }
  const char *synchronize()
  {
    events.push_back("sync");
    return failSync ? "device lost" : nullptr;
  }
  bool capturing(void *)
  {
    events.push_back("capturing");
    return isCapturing;
  }
};

int main(int argc, char **argv)
{
  blah2::TableCache<int> cache;
  FakeDevice dev;
  int built = 0, stream = 0;
  for (int i = 1; i < argc; i++) {
    const char op = argv[i][0];
    const int key = std::atoi(argv[i] + 1);
    dev.events.clear();
    last_error.clear();
    int rc = 0;
    const double *out = nullptr;
    if (op == 'f') {
      rc = cache.free_all(dev) ? 0 : 1;
    } else if (std::strchr("gGpcbaus", op)) {
      dev.isCapturing = op == 'c';
      dev.failAlloc = op == 'a';
      dev.failUpload = op == 'u';
      dev.failSync = op == 's';
      rc = cache.get(
          dev, key, [&](int e) { return op == 'G' ? e >= key : e == key; },
          [&](std::vector<double> &host) {
            built++;
            if (op == 'b') return -7;
            host.assign(3, 1000.0 + key);
            return 0;
          },
          "not resident: call x_prepare before capturing the stream", "table upload: ", &stream, op == 'p', &out);
    } else {
      std::fprintf(stderr, "bad op %s\n", argv[i]);
      return 1;
    }
    if (rc == 0 && op != 'f' && (!out || !dev.live.count(const_cast<double *>(out)))) {
      std::fprintf(stderr, "%s: the table handed out is not a live allocation\n", argv[i]);
      return 1;
    }
    std::printf("%s rc=%d out=", argv[i], rc);
    if (out) std::printf("%g", out[0]);
    else std::printf("-");
    std::printf(" events=");
    for (size_t k = 0; k < dev.events.size(); k++) std::printf("%s%s", k ? "," : "", dev.events[k].c_str());
    std::printf(" list=");
    for (size_t k = 0; k < cache.entries.size(); k++)
      std::printf("%s%d%s", k ? "," : "", cache.entries[k].key, cache.entries[k].pinned ? "p" : "");
    std::printf(" live=%zu built=%d err=%s\n", dev.live.size(), built, last_error.c_str());
  }
  return 0; // (tables still in the list at exit are the leak sanitizer's: the test ends its runs with f)
}
