// Library identity, thread-local error reporting, device queries and the
// path options.
#include <atomic>
#include <cstring>
#include <mutex>

#include "grl_internal.h"

namespace grl {
namespace {
thread_local char g_err[1024] = "";
}

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int device_cu_count() {
  // One process drives one GPU (torch.distributed one-rank-per-device), so the
  // current device's CU count is fixed for the life of the process.
  static int cached = 0;
  static std::once_flag once;
  std::call_once(once, [] {
    int dev = 0;
    int cus = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
      cached = cus;
    else
      cached = 256;  // MI355X
  });
  return cached;
}

namespace {
struct OptDef {
  const char* name;
  int64_t def, lo, hi;
};
#define GRL_OPT_DEF(id, name, def, lo, hi) {name, def, lo, hi},
#define GRL_OPT_INIT(id, name, def, lo, hi) {def},
constexpr OptDef kOpts[OPT_COUNT] = {GRL_OPTIONS(GRL_OPT_DEF)};
std::atomic<int64_t> g_opt[OPT_COUNT] = {GRL_OPTIONS(GRL_OPT_INIT)};
#undef GRL_OPT_DEF
#undef GRL_OPT_INIT

int find_opt(const char* name) {
  for (int i = 0; name && i < OPT_COUNT; ++i)
    if (strcmp(name, kOpts[i].name) == 0) return i;
  return -1;
}
}  // namespace

int64_t opt(GrlOpt o) { return g_opt[o].load(std::memory_order_relaxed); }

}  // namespace grl

extern "C" int grl_set_option(const char* name, int64_t value) {
  using namespace grl;
  const int i = find_opt(name);
  GRL_CHECK_ARG(i >= 0, "grl_set_option: unknown option '%s'", name ? name : "(null)");
  GRL_CHECK_ARG(value >= kOpts[i].lo && value <= kOpts[i].hi, "grl_set_option: %s = %lld outside [%lld, %lld]",
                name, (long long)value, (long long)kOpts[i].lo, (long long)kOpts[i].hi);
  g_opt[i].store(value, std::memory_order_relaxed);
  return GRL_OK;
}

extern "C" int grl_get_option(const char* name, int64_t* value) {
  using namespace grl;
  const int i = find_opt(name);
  GRL_CHECK_ARG(i >= 0, "grl_get_option: unknown option '%s'", name ? name : "(null)");
  GRL_CHECK_ARG(value != nullptr, "grl_get_option: null value pointer");
  *value = g_opt[i].load(std::memory_order_relaxed);
  return GRL_OK;
}

extern "C" const char* grl_version(void) { return "grl-mi355x 0.1.0 (gfx950)"; }

extern "C" const char* grl_last_error(void) { return grl::g_err; }
