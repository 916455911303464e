// ABI version, error strings, the tuning options and the event-based kernel timing hooks.
#include <ctype.h>
#include <errno.h>
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
#include <mutex>
#include <vector>
#include "common.h"
#include "options.h"
#include "prof.h"

namespace {
struct Pair { hipEvent_t a, b; int cls; };
bool g_on = false;
std::mutex g_mu;
std::vector<Pair> g_used;
std::vector<Pair> g_free;
Pair g_cur[kProfClasses];
bool g_open[kProfClasses] = {};
double g_ms[kProfClasses] = {};
int64_t g_n[kProfClasses] = {};
double g_flops[kProfClasses] = {};
double g_bytes[kProfClasses] = {};
}  // namespace

void passl_prof_retag(int from, int to) {
  if (!g_on) return;
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g_open[from]) return;
  g_cur[to] = g_cur[from];
  g_cur[to].cls = to;
  g_open[to] = true;
  g_open[from] = false;
}

void passl_prof_work(int cls, double flops, double bytes) {
  if (!g_on) return;
  std::lock_guard<std::mutex> lk(g_mu);
  g_flops[cls] += flops;
  g_bytes[cls] += bytes;
}

void passl_prof_begin(int cls, hipStream_t st) {
  if (!g_on) return;
  std::lock_guard<std::mutex> lk(g_mu);
  Pair p;
  if (!g_free.empty()) { p = g_free.back(); g_free.pop_back(); }
  else { (void)hipEventCreate(&p.a); (void)hipEventCreate(&p.b); }
  p.cls = cls;
  (void)hipEventRecord(p.a, st);
  g_cur[cls] = p;
  g_open[cls] = true;
}

void passl_prof_end(int cls, hipStream_t st) {
  if (!g_on) return;
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g_open[cls]) return;
  (void)hipEventRecord(g_cur[cls].b, st);
  g_used.push_back(g_cur[cls]);
  g_open[cls] = false;
}

extern "C" int passl_hip_prof_enable(int on) {
  std::lock_guard<std::mutex> lk(g_mu);
  g_on = on != 0;
  return PASSL_OK;
}

extern "C" int passl_hip_prof_collect(int cls, double* total_ms, int64_t* launches) {
  if (cls < 0 || cls >= kProfClasses || !total_ms || !launches) return PASSL_EINVAL;
  std::lock_guard<std::mutex> lk(g_mu);
  for (auto& p : g_used) {
    (void)hipEventSynchronize(p.b);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { g_ms[p.cls] += ms; g_n[p.cls] += 1; }
    g_free.push_back(p);
  }
  g_used.clear();
  *total_ms = g_ms[cls];
  *launches = g_n[cls];
  g_ms[cls] = 0; g_n[cls] = 0;
  return PASSL_OK;
}

// algorithmic FLOPs / HBM bytes of the launches timed since the last collect_work of this class
extern "C" int passl_hip_prof_collect_work(int cls, double* flops, double* bytes) {
  if (cls < 0 || cls >= kProfClasses || !flops || !bytes) return PASSL_EINVAL;
  std::lock_guard<std::mutex> lk(g_mu);
  *flops = g_flops[cls];
  *bytes = g_bytes[cls];
  g_flops[cls] = 0; g_bytes[cls] = 0;
  return PASSL_OK;
}

// What an (event, kernel, event) bracket reads ON TOP of the kernel's own duration: the same bracket around nothing,
// averaged over n pairs on `stream` (synchronises).  bench.py reports it next to the event-timed averages: rocprofv3's
// kernel durations are begin/end timestamps of the dispatch itself, an event pair also sees the two event packets
// and the gap before the dispatch starts.
extern "C" int passl_hip_prof_event_overhead(int n, passl_stream_t stream, double* avg_us) {
  if (n <= 0 || n > 4096 || !avg_us) return PASSL_EINVAL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  std::vector<hipEvent_t> ev(2 * (size_t)n);
  for (auto& e : ev)
    if (hipEventCreate(&e) != hipSuccess) return PASSL_ELAUNCH;
  for (int i = 0; i < n; ++i) {
    (void)hipEventRecord(ev[2 * i], st);
    (void)hipEventRecord(ev[2 * i + 1], st);
  }
  (void)hipStreamSynchronize(st);
  double sum = 0.0;
  int cnt = 0;
  for (int i = 0; i < n; ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]) == hipSuccess) { sum += ms; cnt += 1; }
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  if (cnt == 0) return PASSL_ELAUNCH;
  *avg_us = 1000.0 * sum / cnt;
  return PASSL_OK;
}

// ---- tuning options: the table of options.h, defaults overridden by PASSL_<NAME> on the first access
namespace {
struct OptRow {
  const char* name;
  int def, lo, hi;
  int n;          // > 0: the value must also be one of vals[0, n)
  int vals[4];
};
constexpr int count(std::initializer_list<int> v) { return (int)v.size(); }
#define ANY RANGE(INT_MIN, INT_MAX)
#define RANGE(lo, hi) lo, hi, 0, {}
#define ONE_OF(...) INT_MIN, INT_MAX, count({__VA_ARGS__}), {__VA_ARGS__}
#define PASSL_OPT_ROW(name, def, values) {#name, def, values},
constexpr OptRow kOpts[] = {PASSL_OPTION_LIST(PASSL_OPT_ROW)};
#undef PASSL_OPT_ROW
#undef ONE_OF
#undef RANGE
#undef ANY
constexpr int kNumOpts = (int)Opt::kCount;
static_assert(sizeof(kOpts) / sizeof(kOpts[0]) == kNumOpts, "options.h: one row per option");

constexpr bool accepts(const OptRow& r, int v) {
  if (v < r.lo || v > r.hi) return false;
  for (int i = 0; i < r.n; ++i)
    if (r.vals[i] == v) return true;
  return r.n == 0;
}
constexpr bool defaults_accepted() {
  for (const OptRow& r : kOpts)
    if (!accepts(r, r.def)) return false;
  return true;
}
static_assert(defaults_accepted(), "options.h: a default outside its option's accepted values");

int g_opt[kNumOpts];

bool init_options() {
  for (int i = 0; i < kNumOpts; ++i) {
    const OptRow& r = kOpts[i];
    g_opt[i] = r.def;
    char var[64] = "PASSL_";
    for (int k = 0; r.name[k]; ++k) var[6 + k] = (char)toupper((unsigned char)r.name[k]);
    const char* e = getenv(var);
    if (!e) continue;
    char* end = nullptr;
    errno = 0;
    const long v = strtol(e, &end, 10);
    if (!*e || *end || errno || v < INT_MIN || v > INT_MAX || !accepts(r, (int)v))
      fprintf(stderr, "libpassl_hip: %s=%s is not a value of option %s: it keeps its default %d\n", var, e, r.name,
              r.def);
    else
      g_opt[i] = (int)v;
  }
  return true;
}

int* opt_values() {
  static const bool ready = init_options();
  (void)ready;
  return g_opt;
}

int opt_index(const char* name) {
  for (int i = 0; name && i < kNumOpts; ++i)
    if (!strcmp(name, kOpts[i].name)) return i;
  return -1;
}
}  // namespace

int passl_opt(Opt o) { return opt_values()[(int)o]; }

extern "C" int passl_hip_set_option(const char* name, int value) {
  const int i = opt_index(name);
  if (i < 0 || !accepts(kOpts[i], value)) return PASSL_EINVAL;
  opt_values()[i] = value;
  return PASSL_OK;
}

extern "C" int passl_hip_get_option(const char* name, int* value) {
  const int i = opt_index(name);
  if (i < 0 || !value) return PASSL_EINVAL;
  *value = opt_values()[i];
  return PASSL_OK;
}

extern "C" int passl_hip_abi_version(void) { return PASSL_HIP_ABI_VERSION; }

extern "C" const char* passl_hip_strerror(int status) {
  switch (status) {
    case PASSL_OK: return "ok";
    case PASSL_EINVAL: return "invalid argument (null/misaligned pointer or unsupported shape)";
    case PASSL_ELAUNCH: return "kernel launch failed";
    case PASSL_EUNSUPPORTED: return "dtype/shape combination not built";
    default: return "unknown status";
  }
}
