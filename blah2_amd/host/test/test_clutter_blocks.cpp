// The drop-in WienerHopf with taps per block -- WienerHopf(delayMin, delayMax, nSamples, nBlocks)::process(IqData*, IqData*)
// -- against the fp64 restatement's filtered channel (tests/clutter_blocks_ref.py), written by
// tests/test_clutter_blocks_host_gpu.py the way tests/test_host_cpp_gpu.py writes test_golden's records.
//
//     test_clutter_blocks record.bin [record.bin ...]
//
// A record (little-endian): "B2CLBK01", int64 n, delayMin, delayMax, nBlocks, ok, then x, y and the expected y (each an
// int64 count and that many complex fp64).  ok = 0: a block's normal equations are not positive definite -- process()
// returns false and y keeps its samples.  Every record runs twice on one pair of FIFOs (the second CPI through the eager
// pinned-shadow path).  Exit code 0 = all checks passed.
#include "data/IqData.h"
#include "process/clutter/WienerHopf.h"

#include <complex>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

typedef std::complex<double> cd;

static int failures = 0;
static std::string ctx;
#define CHECK(cond)                                                                                              \
  do {                                                                                                           \
    if (!(cond)) { std::printf("CHECK FAILED [%s] %s:%d: %s\n", ctx.c_str(), __FILE__, __LINE__, #cond); failures++; } \
  } while (0)
#define CHECK_LE(val, lim)                                                                                       \
  do {                                                                                                           \
    const double v_ = (val), l_ = (lim);                                                                         \
    if (!(v_ <= l_)) { std::printf("CHECK FAILED [%s] %s:%d: %s = %.3e > %.3e\n", ctx.c_str(), __FILE__, __LINE__, #val, v_, l_); failures++; } \
  } while (0)

static const double Y_TOL = 1e-4; // tests/test_clutter_gpu.py

struct Record {
  int64_t n, dmin, dmax, nBlocks, ok;
  std::vector<cd> x, y, yref;
};

static bool load(const char *path, Record &g)
{
  FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  bool ok = true;
  auto get = [&](void *p, size_t bytes) { if (std::fread(p, 1, bytes, f) != bytes) ok = false; };
  auto vec = [&](std::vector<cd> &v) {
    int64_t c = 0;
    get(&c, sizeof c);
    if (!ok || c < 0 || c > (int64_t)1 << 28) { ok = false; return; }
    v.resize((size_t)c);
    get(v.data(), (size_t)c * sizeof(cd));
  };
  char magic[8];
  get(magic, 8);
  if (!ok || std::memcmp(magic, "B2CLBK01", 8) != 0) { std::fclose(f); return false; }
  int64_t head[5];
  get(head, sizeof head);
  g.n = head[0]; g.dmin = head[1]; g.dmax = head[2]; g.nBlocks = head[3]; g.ok = head[4];
  vec(g.x); vec(g.y); vec(g.yref);
  std::fclose(f);
  return ok && (int64_t)g.x.size() == g.n && (int64_t)g.y.size() == g.n && (int64_t)g.yref.size() == g.n;
}

static void run_record(const Record &g, const std::string &name)
{
  const uint32_t n = (uint32_t)g.n;
  IqData x{n}, y{n};
  WienerHopf filter((int32_t)g.dmin, (int32_t)g.dmax, n, (uint32_t)g.nBlocks);
  for (int c = 0; c < 2; c++) {
    ctx = name + " cpi " + std::to_string(c);
    for (int64_t i = 0; i < g.n; i++) { x.push_back(g.x[(size_t)i]); y.push_back(g.y[(size_t)i]); } // evicts the previous CPI
    const bool ok = filter.process(&x, &y);
    CHECK(ok == (g.ok != 0));
    CHECK((int64_t)y.get_length() == g.n && (int64_t)x.get_length() == g.n);
    const auto yd = y.get_data(), xd = x.get_data();
    CHECK((int64_t)yd.size() == g.n && (int64_t)xd.size() == g.n);
    if ((int64_t)yd.size() != g.n || (int64_t)xd.size() != g.n) return;
    double ymax = 0, emax = 0;
    bool xsame = true;
    for (int64_t i = 0; i < g.n; i++) {
      ymax = std::max(ymax, std::abs(g.yref[(size_t)i]));
      emax = std::max(emax, std::abs(yd[(size_t)i] - g.yref[(size_t)i]));
      xsame = xsame && xd[(size_t)i] == g.x[(size_t)i];
    }
    CHECK(xsame); // the reference channel is read only
    if (g.ok) CHECK_LE(emax / ymax, Y_TOL);
    else CHECK(emax == 0.0); // skipped: y keeps its samples (the record's expected y is its y)
    std::printf("[%s] ok %d, max|dy| / max|y_ref| = %.3e\n", ctx.c_str(), (int)ok, emax / ymax);
  }
}

int main(int argc, char **argv)
{
  if (argc < 2) { std::printf("usage: test_clutter_blocks record.bin [...]\n"); return 2; }
  for (int a = 1; a < argc; a++) {
    Record g;
    if (!load(argv[a], g)) { std::printf("cannot read %s\n", argv[a]); return 2; }
    const std::string p(argv[a]);
    const size_t s = p.find_last_of('/');
    const std::string name = p.substr(s == std::string::npos ? 0 : s + 1);
    const int before = failures;
    run_record(g, name);
    std::printf("%s: %s\n", name.c_str(), failures == before ? "ok" : "FAILED");
  }
  std::printf(failures ? "FAILED (%d)\n" : "OK\n", failures);
  return failures ? 1 : 0;
}
