// The library's host-side state: the error message behind gh_last_error (set_error), the optional per-kernel event profiler
// (prof_begin / prof_end, gh_profile_*), the per-device counters of clamped inputs (clamp_counter, gh_clamp_events), the one
// opt-in to more than 64 KB of dynamic LDS (lds_opt_in) and gh_abi_version.  Host code only: this file holds no kernel.
#include "../../include/get_hip.h"
#include "common.h"
#include <map>
#include <mutex>
#include <stdarg.h>
#include <unordered_map>
#include <vector>

namespace gh {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---------------------------------------------------------------------------- event profiler
struct ProfRec { hipEvent_t a, b; int tag; double work; };
static bool g_prof_on = false;
static unsigned g_prof_mask = 0xFFFFFFFFu;     // bit t set: kernels with tag t are instrumented (gh_profile_select)
static std::vector<ProfRec> g_prof_recs;
static std::vector<hipEvent_t> g_prof_pool;
static hipEvent_t g_prof_cur = nullptr;

static hipEvent_t prof_event() {
  if (!g_prof_pool.empty()) { hipEvent_t e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}
bool prof_enabled() { return g_prof_on; }
void prof_begin(hipStream_t s, int tag) {
  g_prof_cur = nullptr;
  if (!g_prof_on || !((g_prof_mask >> tag) & 1u)) return;
  g_prof_cur = prof_event();
  if (g_prof_cur) (void)hipEventRecord(g_prof_cur, s);
}
void prof_end(int tag, double work, hipStream_t s) {
  if (!g_prof_on || !g_prof_cur) return;
  hipEvent_t b = prof_event();
  if (!b) return;
  (void)hipEventRecord(b, s);
  g_prof_recs.push_back(ProfRec{g_prof_cur, b, tag, work});
  g_prof_cur = nullptr;
}

// Device counters of clamped out-of-range inputs (include/get_hip.h gh_clamp_events, gh_clamp_events_n): GH_CLAMP_SLOTS unsigned
// ints per device, allocated on first use, handed to the kernels that clamp (cross_entropy: [0], left_assemble: [1],
// evd_assemble: [2], embed_bwd: [3], softmax_xent_fwd: [4]).
static std::mutex g_clamp_mu;
static std::unordered_map<int, unsigned int*> g_clamp_buf;
unsigned int* clamp_counter() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(g_clamp_mu);
  auto it = g_clamp_buf.find(dev);
  if (it != g_clamp_buf.end()) return it->second;
  unsigned int* p = nullptr;
  if (hipMalloc((void**)&p, GH_CLAMP_SLOTS * sizeof(unsigned int)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  if (hipMemset(p, 0, GH_CLAMP_SLOTS * sizeof(unsigned int)) != hipSuccess) { (void)hipGetLastError(); (void)hipFree(p); return nullptr; }
  g_clamp_buf.emplace(dev, p);
  return p;
}

// ---------------------------------------------------------------------------- LDS opt-in (common.h)
// The only place that raises hipFuncAttributeMaxDynamicSharedMemorySize.  A kernel's static LDS counts against the 160 KB of a CU
// as well, so the limit asked for is 160 KB minus that (a flat 160 KB is refused for any kernel with a static word).  The table
// holds the static LDS of every (kernel, device) that has been raised: the attribute is set once, later calls are a look-up.
// (Keyed by the function pointer, not the kernel's type: the instantiations of one template share a type.)
static std::mutex g_lds_mu;
static std::map<std::pair<const void*, int>, size_t> g_lds_static;
int lds_opt_in(const void* kernel, size_t dynamic_lds, const char* who) {
  constexpr size_t kDefault = 64 * 1024, kCu = 160 * 1024;
  if (dynamic_lds <= kDefault) return 0;
  int dev = 0;
  GH_CHECK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_lds_mu);
  const auto key = std::make_pair(kernel, dev);
  auto it = g_lds_static.find(key);
  const bool raised = it != g_lds_static.end();
  size_t static_lds = 0;
  if (raised) {
    static_lds = it->second;
  } else {
    hipFuncAttributes fa;
    const hipError_t e = hipFuncGetAttributes(&fa, kernel);
    GH_REQUIRE(e == hipSuccess, "%s: cannot read the kernel's attributes: %s", who, hipGetErrorString(e));
    static_lds = fa.sharedSizeBytes;
  }
  GH_REQUIRE(static_lds + dynamic_lds <= kCu, "%s: needs %zu bytes of dynamic LDS beside %zu static ones (a CU has %zu)", who,
             dynamic_lds, static_lds, kCu);
  if (!raised) {
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kCu - static_lds));
    GH_REQUIRE(e == hipSuccess, "%s: raising the dynamic LDS limit to %zu bytes (%zu static) was refused: %s", who, kCu - static_lds,
               static_lds, hipGetErrorString(e));
    g_lds_static.emplace(key, static_lds);
  }
  return 0;
}

}  // namespace gh

using namespace gh;

extern "C" int gh_clamp_events_n(int64_t* out, int n, int reset) {
  GH_REQUIRE(out, "clamp_events: NULL output");
  GH_REQUIRE(n >= 1 && n <= GH_CLAMP_SLOTS, "clamp_events: %d slots asked for (1 .. %d)", n, GH_CLAMP_SLOTS);
  unsigned int* p = clamp_counter();
  GH_REQUIRE(p, "clamp_events: cannot allocate the counter");
  unsigned int h[GH_CLAMP_SLOTS] = {};
  GH_CHECK_HIP(hipDeviceSynchronize());
  GH_CHECK_HIP(hipMemcpy(h, p, sizeof(h), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i) out[i] = (int64_t)h[i];
  if (reset) GH_CHECK_HIP(hipMemset(p, 0, sizeof(h)));
  return 0;
}
extern "C" int gh_clamp_events(int64_t* out, int reset) { return gh_clamp_events_n(out, 4, reset); }

extern "C" int gh_abi_version(void) { return GH_ABI_VERSION; }
extern "C" const char* gh_last_error(void) { return g_err; }

extern "C" int gh_profile_enable(int on) {
  g_prof_on = on != 0;
  return 0;
}
// out[PROF_NTAGS][3] = {total ms, total work, launches}; waits for the recorded events, then resets.
extern "C" int gh_profile_select(uint32_t tag_mask) {
  g_prof_mask = tag_mask;
  return 0;
}

extern "C" int gh_profile_collect(double* out, int rows) {
  GH_REQUIRE(rows >= PROF_NTAGS, "profile_collect: need %d rows", (int)PROF_NTAGS);
  for (int i = 0; i < rows * 3; ++i) out[i] = 0.0;
  for (auto& r : g_prof_recs) {
    float ms = 0.f;
    GH_CHECK_HIP(hipEventSynchronize(r.b));
    GH_CHECK_HIP(hipEventElapsedTime(&ms, r.a, r.b));
    out[r.tag * 3 + 0] += ms;
    out[r.tag * 3 + 1] += r.work;
    out[r.tag * 3 + 2] += 1.0;
    g_prof_pool.push_back(r.a);
    g_prof_pool.push_back(r.b);
  }
  g_prof_recs.clear();
  return 0;
}
