// The detectors' device-table cache: the policy, stated once.  Host code without a HIP include -- the device reaches it
// through the `Dev` parameter of its two functions, so tests/host/emulate_table_cache.cpp drives it with a fake.
//
// A list holds tables least recently used first, eight unpinned ones at most (a caller that adapts pfa per CPI does not grow
// device memory).  A hit moves the entry to the back and hands out its pointer; a pin, once set, stays.  A miss builds the
// table on the host, uploads it (blocking) and evicts the oldest unpinned entry if there are now too many: the device is
// synchronised first, because enqueued work may still read that table.  A miss is refused while the stream is being
// captured into a graph, before anything is built -- *_prepare is the call for that.  A table *_prepare has handed out is
// pinned and lives as long as the list: a graph captured afterwards has its address baked in, and no synchronisation at
// eviction time protects a later replay.  Only unpinned tables are evicted.  A builder, allocation or upload failure leaves
// the list as it was and nothing allocated.
//
// Dev:  const char *alloc(size_t bytes, double **d)                        nullptr, or the error's text
//       const char *upload(double *d, const double *host, size_t bytes)    (blocking)
//       bool free(double *d)                                               false: the free failed
//       const char *synchronize()                                          the whole device
//       bool capturing(void *stream)
#pragma once

#include "blah2hip.h"

#include <cstddef>
#include <string>
#include <vector>

extern "C" void blah2hip_set_error_(const char *msg); // context.hip: the thread's error string (blah2hip_last_error)

namespace blah2 {

template <class Key>
struct TableCache {
  static constexpr size_t MAX_UNPINNED = 8;
  struct Entry { Key key; double *d; bool pinned; };
  std::vector<Entry> entries; // least recently used first

  // The table `match(entry key)` accepts, else the one `build(host)` fills (an rc other than 0 is handed on), stored under
  // `key`.  `missing`: the refusal's text while `stream` is being captured; `upload`: what stands in front of a HIP error's.
  template <class Dev, class Match, class Build>
  int get(Dev &dev, const Key &key, Match match, Build build, const char *missing, const char *upload, void *stream, bool pin,
          const double **out)
  {
    auto fail = [](int code, const std::string &msg) { blah2hip_set_error_(msg.c_str()); return code; };
    for (size_t i = 0; i < entries.size(); i++)
      if (match(entries[i].key)) {
        Entry e = entries[i];
        e.pinned = e.pinned || pin;
        entries.erase(entries.begin() + (long)i);
        entries.push_back(e); // most recently used last
        *out = e.d;
        return BLAH2HIP_OK;
      }
    if (stream && dev.capturing(stream)) return fail(BLAH2HIP_ERR_INVALID, missing);
    std::vector<double> host;
    if (int rc = build(host)) return rc;
    Entry e{key, nullptr, pin};
    const size_t bytes = host.size() * sizeof(double);
    if (const char *err = dev.alloc(bytes, &e.d)) return fail(BLAH2HIP_ERR_HIP, std::string(upload) + err);
    if (const char *err = dev.upload(e.d, host.data(), bytes)) {
      dev.free(e.d);
      return fail(BLAH2HIP_ERR_HIP, std::string(upload) + err);
    }
    size_t unpinned = pin ? 0 : 1;
    for (const Entry &o : entries) unpinned += o.pinned ? 0 : 1;
    if (unpinned > MAX_UNPINNED) {
      if (const char *err = dev.synchronize()) { // the oldest unpinned table may still be read by enqueued work
        dev.free(e.d);
        return fail(BLAH2HIP_ERR_HIP, std::string("hipDeviceSynchronize(): ") + err);
      }
      for (size_t i = 0; i < entries.size(); i++)
        if (!entries[i].pinned) {
          dev.free(entries[i].d);
          entries.erase(entries.begin() + (long)i);
          break;
        }
    }
    entries.push_back(e);
    *out = e.d;
    return BLAH2HIP_OK;
  }

  // every table of the list (destroy); true if every free succeeded
  template <class Dev>
  bool free_all(Dev &dev)
  {
    bool ok = true;
    for (Entry &e : entries) ok = dev.free(e.d) && ok;
    entries.clear();
    return ok;
  }
};

} // namespace blah2
