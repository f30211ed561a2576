// The runtime services of libfinrom_hip.so's C ABI (include/finrom.h): error text, stream-capture registry and deferred
// frees, CallGuard, Scratch, the per-kernel profiler, the finrom_malloc pool, and the copy / sync / profile / version entry points.
// An extern "C" region is open only around entry points; every helper stands outside one.
#include "api_private.h"

#include <algorithm>
#include <mutex>

namespace finrom {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int hip_fail(hipError_t e, const char* what) {
  g_err = std::string(what) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")";
  return FINROM_ERR_HIP;
}

// ---- stream capture registry, deferred frees (finrom_core.h) --------------------------------------------------------------
static std::mutex g_cap_mu;
static std::vector<hipStream_t> g_cap_streams;          // streams last seen under capture
struct DeferredCall { void (*fn)(void*); void* arg; };
static std::vector<DeferredCall> g_deferred;            // capture-unsafe cleanups waiting for the capture to end
static thread_local bool tl_call_captures = false;

static bool query_capturing(hipStream_t st) {
  if (st == nullptr) return false;                      // the legacy default stream cannot be captured (and must not be queried
                                                        //  while another stream captures: that is itself an "implicit" violation)
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  const hipError_t e = hipStreamIsCapturing(st, &cs);
  if (e != hipSuccess) { (void)hipGetLastError(); return false; }      // a stream that no longer exists is not capturing
  return cs != hipStreamCaptureStatusNone;              // (an invalidated capture is still open until EndCapture)
}
bool note_stream(hipStream_t st) {
  const bool cap = query_capturing(st);
  if (st == nullptr) return false;
  std::lock_guard<std::mutex> lk(g_cap_mu);
  auto it = std::find(g_cap_streams.begin(), g_cap_streams.end(), st);
  if (cap && it == g_cap_streams.end()) g_cap_streams.push_back(st);
  if (!cap && it != g_cap_streams.end()) g_cap_streams.erase(it);
  return cap;
}
static bool any_capture_locked() {
  for (size_t i = 0; i < g_cap_streams.size();) {
    if (query_capturing(g_cap_streams[i])) ++i;
    else g_cap_streams.erase(g_cap_streams.begin() + i);
  }
  return !g_cap_streams.empty();
}
bool any_capture() { std::lock_guard<std::mutex> lk(g_cap_mu); return any_capture_locked(); }
bool call_captures() { return tl_call_captures; }
static void hip_free_cb(void* p) { (void)hipFree(p); }
void defer_or_run(void (*fn)(void*), void* arg) {
  {
    std::lock_guard<std::mutex> lk(g_cap_mu);
    if (any_capture_locked()) { g_deferred.push_back({fn, arg}); return; }
  }
  fn(arg);
}
void dev_free(void* p) { if (p) defer_or_run(hip_free_cb, p); }
void flush_deferred() {
  std::vector<DeferredCall> run;
  {
    std::lock_guard<std::mutex> lk(g_cap_mu);
    if (g_deferred.empty() || any_capture_locked()) return;
    run.swap(g_deferred);
  }
  for (auto& d : run) d.fn(d.arg);
}
int deferred_count() { std::lock_guard<std::mutex> lk(g_cap_mu); return (int)g_deferred.size(); }
CallGuard::CallGuard(hipStream_t st) : prev(tl_call_captures) {
  const bool cap = note_stream(st);
  tl_call_captures = prev || cap;
  if (!tl_call_captures) flush_deferred();
}
CallGuard::~CallGuard() { tl_call_captures = prev; }

int Scratch::reserve(size_t bytes) {
  if (bytes <= cap) { captured = captured || tl_call_captures; return 0; }
  if (tl_call_captures || any_capture()) {
    set_error("a workspace of " + std::to_string(bytes) + " bytes is needed while a stream capture is open: run the same call once "
              "(same handle, same batch size) before the capture begins");
    return FINROM_ERR_UNSUPPORTED;
  }
  if (p) {
    if (captured) retired.push_back(p);        // a graph captured earlier still points at it: keep it until the handle goes
    else (void)hipFree(p);
    p = nullptr; cap = 0; captured = false;
  }
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) { p = nullptr; set_error("hipMalloc of " + std::to_string(bytes) + " scratch bytes failed"); return FINROM_ERR_NOMEM; }
  cap = bytes;
  return 0;
}
void Scratch::release() {
  dev_free(p);
  for (void* q : retired) dev_free(q);
  retired.clear();
  p = nullptr; cap = 0; captured = false;
}

// ---- profiling -------------------------------------------------------------------------
static const char* kSlotNames[K_NUM] = {"pack", "fom_assemble", "fom_chol_solve", "unpack_w", "rom_proj_mfma",
                                        "rom_reduced_solve", "subfin_avg", "sampler_gemm_exp", "misc",
                                        "fom_path_small", "fom_path_interpreter", "fom_path_band_registers", "fom_path_band_lds_4wave"};
struct Pending { int slot; hipEvent_t e0, e1; };
static std::mutex g_prof_mu;
static bool g_prof_on = false;
static std::vector<Pending> g_pending;
static std::vector<hipEvent_t> g_pool;
static bool g_overlap = true;
static double g_ms[K_NUM];
static int64_t g_cnt[K_NUM];

static hipEvent_t get_event() {
  if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}
ScopedKernelTimer::ScopedKernelTimer(int slot_, hipStream_t s_) : slot(slot_), s(s_) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (!g_prof_on) return;
  // a stream that is being captured into a HIP graph records nothing now: an event recorded there becomes a graph node and can
  // never be waited for or timed from the host (hmc.run_chains_device captures the one-sample call sequence)
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return;
  e0 = get_event(); e1 = get_event();
  if (e0 && e1) (void)hipEventRecord(e0, s);
}
ScopedKernelTimer::~ScopedKernelTimer() {
  if (!e0 || !e1) return;
  (void)hipEventRecord(e1, s);
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_pending.push_back({slot, e0, e1});
}
static void drain_pending() {
  for (auto& p : g_pending) {
    float ms = 0.f;
    if (hipEventSynchronize(p.e1) == hipSuccess && hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) {
      g_ms[p.slot] += ms; g_cnt[p.slot] += 1;
      if (p.slot >= K_FOM_PATH_SMALL && p.slot <= K_FOM_PATH_BAND_LDSW) { g_ms[K_FOM] += ms; g_cnt[K_FOM] += 1; }
    }
    g_pool.push_back(p.e0); g_pool.push_back(p.e1);
  }
  g_pending.clear();
}
bool overlap_enabled() { return g_overlap; }

// finrom_malloc / finrom_free recycle small buffers (<= 16 MiB, size classes = powers of two, at most 256 MiB parked): the scalar
// call surface allocates a handful of small buffers per call, and hipMalloc / hipFree cost more than its kernels.  A parked
// buffer carries the event finrom_free_async recorded behind its last user; the next owner waits for it.
namespace {
constexpr size_t kPoolMaxEach = (size_t)16 << 20, kPoolMaxTotal = (size_t)256 << 20;
struct Parked { void* p; hipEvent_t ev; int dev; };       // (dev: a parked buffer is only handed out on the device it lives on)
std::mutex g_pool_mu;
std::vector<std::pair<void*, size_t>> g_pool_live;          // pooled allocations handed out: (pointer, size class)
std::vector<std::pair<size_t, Parked>> g_pool_free;         // parked: (size class, buffer)
size_t g_pool_free_bytes = 0;
std::vector<hipEvent_t> g_pool_events;
size_t size_class(size_t bytes) { size_t c = 256; while (c < bytes) c <<= 1; return c; }
void event_destroy_cb(void* e) { (void)hipEventDestroy((hipEvent_t)e); }
}  // namespace

}  // namespace finrom

using namespace finrom;

extern "C" {

int finrom_version(void) { return FINROM_ABI_VERSION; }
const char* finrom_last_error(void) { return g_err.c_str(); }

int finrom_device_count(int* count) { if (!count) return FINROM_ERR_ARG; FR_HIP(hipGetDeviceCount(count)); return 0; }
int finrom_set_device(int ordinal) { FR_HIP(hipSetDevice(ordinal)); return 0; }
int finrom_malloc(void** dptr, size_t bytes) {
  if (!dptr) return FINROM_ERR_ARG;
  *dptr = nullptr;
  if (bytes == 0) return 0;
  const bool capture = any_capture();
  if (!capture) flush_deferred();
  size_t cap = bytes;
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (bytes <= kPoolMaxEach) {
    cap = size_class(bytes);
    std::unique_lock<std::mutex> lk(g_pool_mu);
    for (size_t i = g_pool_free.size(); i-- > 0;) {          // (the most recently parked first)
      if (g_pool_free[i].first != cap || g_pool_free[i].second.dev != dev) continue;
      Parked b = g_pool_free[i].second;
      bool done = b.ev == nullptr;
      if (!done) { done = hipEventQuery(b.ev) == hipSuccess; if (!done) (void)hipGetLastError(); }
      if (!done && capture) continue;                          // (no host wait while a capture is open)
      g_pool_free.erase(g_pool_free.begin() + i);
      g_pool_free_bytes -= cap;
      g_pool_live.emplace_back(b.p, cap);
      lk.unlock();
      if (b.ev != nullptr) {
        // the last user (a launch on some non-blocking stream) must have finished before the new owner writes
        const hipError_t e = done ? hipSuccess : hipEventSynchronize(b.ev);
        std::lock_guard<std::mutex> lk2(g_pool_mu);
        g_pool_events.push_back(b.ev);
        if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize(pooled buffer)");
      }
      *dptr = b.p;
      return 0;
    }
  }
  if (capture) { set_error("finrom_malloc: refused while a stream capture is open (allocate before the capture begins)"); return FINROM_ERR_UNSUPPORTED; }
  hipError_t e = hipMalloc(dptr, cap);
  if (e != hipSuccess) { set_error("hipMalloc of " + std::to_string(cap) + " bytes failed: " + hipGetErrorName(e)); return FINROM_ERR_NOMEM; }
  if (bytes <= kPoolMaxEach) { std::lock_guard<std::mutex> lk(g_pool_mu); g_pool_live.emplace_back(*dptr, cap); }
  return 0;
}
}  // extern "C"
// stream: the stream of the buffer's last user, or NULL when that user is known to have finished / ran on the default stream
static int pool_free(void* dptr, hipStream_t stream, bool have_stream) {
  if (!dptr) return 0;
  size_t cap = 0;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (size_t i = 0; i < g_pool_live.size(); ++i)
      if (g_pool_live[i].first == dptr) { cap = g_pool_live[i].second; g_pool_live.erase(g_pool_live.begin() + i); break; }
  }
  const bool st_captures = have_stream && note_stream(stream);
  if (cap != 0 && !st_captures) {
    hipEvent_t ev = nullptr;
    if (have_stream && stream != nullptr) {
      {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        if (!g_pool_events.empty()) { ev = g_pool_events.back(); g_pool_events.pop_back(); }
      }
      if (ev == nullptr && !any_capture() && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
      if (ev != nullptr && hipEventRecord(ev, stream) != hipSuccess) { (void)hipGetLastError(); defer_or_run(event_destroy_cb, ev); ev = nullptr; cap = 0; }
      if (ev == nullptr) cap = 0;                              // no event to be had: do not park, free (deferred under capture)
    }
    if (cap != 0) {
      int dev = 0;
      hipPointerAttribute_t at{};
      if (hipPointerGetAttributes(&at, dptr) == hipSuccess) dev = at.device; else { (void)hipGetLastError(); (void)hipGetDevice(&dev); }
      std::lock_guard<std::mutex> lk(g_pool_mu);
      if (g_pool_free_bytes + cap <= kPoolMaxTotal) {
        g_pool_free.push_back({cap, Parked{dptr, ev, dev}});
        g_pool_free_bytes += cap;
        return 0;
      }
      if (ev != nullptr) g_pool_events.push_back(ev);
    }
  }
  // not pooled, pool full, or last used inside a capture (the graph may replay it: never recycled, freed once no capture is open)
  dev_free(dptr);
  return 0;
}
extern "C" {
int finrom_free(void* dptr) { return pool_free(dptr, nullptr, false); }
int finrom_free_async(void* dptr, void* stream) { return pool_free(dptr, (hipStream_t)stream, true); }
int finrom_note_stream(void* stream) {
  const bool cap = note_stream((hipStream_t)stream);
  if (!cap) flush_deferred();
  return cap ? 1 : 0;
}
int finrom_deferred_count(void) { return deferred_count(); }
int finrom_flush_deferred(void) { flush_deferred(); return deferred_count(); }
int finrom_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) {
  if (bytes == 0) return 0;
  CallGuard cg((hipStream_t)stream);
  if (call_captures() || any_capture()) { set_error("finrom_memcpy_h2d synchronises: not while a stream capture is open"); return FINROM_ERR_UNSUPPORTED; }
  FR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  FR_HIP(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}
int finrom_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) {
  if (bytes == 0) return 0;
  CallGuard cg((hipStream_t)stream);
  if (call_captures() || any_capture()) { set_error("finrom_memcpy_d2h synchronises: not while a stream capture is open"); return FINROM_ERR_UNSUPPORTED; }
  FR_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  FR_HIP(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}
int finrom_memset(void* dst, int value, size_t bytes, void* stream) {
  if (bytes == 0) return 0;
  CallGuard cg((hipStream_t)stream);
  if (stream == nullptr && any_capture()) { set_error("finrom_memset on the default stream: not while a stream capture is open"); return FINROM_ERR_UNSUPPORTED; }
  FR_HIP(hipMemsetAsync(dst, value, bytes, (hipStream_t)stream));
  return 0;
}
int finrom_stream_sync(void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (call_captures()) { set_error("finrom_stream_sync on a capturing stream"); return FINROM_ERR_UNSUPPORTED; }
  FR_HIP(hipStreamSynchronize((hipStream_t)stream));
  return 0;
}

int finrom_set_overlap(int on) { g_overlap = on != 0; return 0; }
int finrom_profile_enable(int on) { std::lock_guard<std::mutex> lk(g_prof_mu); g_prof_on = on != 0; return 0; }
int finrom_profile_reset(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  drain_pending();
  for (int i = 0; i < K_NUM; ++i) { g_ms[i] = 0; g_cnt[i] = 0; }
  return 0;
}
int finrom_profile_slots(void) { return K_NUM; }
int finrom_profile_read(int slot, const char** name, int64_t* launches, double* total_ms) {
  if (slot < 0 || slot >= K_NUM) return FINROM_ERR_ARG;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  drain_pending();
  if (name) *name = kSlotNames[slot];
  if (launches) *launches = g_cnt[slot];
  if (total_ms) *total_ms = g_ms[slot];
  return 0;
}

}  // extern "C"
