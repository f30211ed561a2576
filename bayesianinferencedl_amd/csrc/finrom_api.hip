// extern "C" surface of libfinrom_hip.so (see include/finrom.h for the contract), in four parts: the runtime services, the FOM
// handle, the ROM handle with finrom_solve_pairs, inference (sampler, mlp, hmc, metric, lbfgs).  The host-only table builders and
// validators are rom_tables.hip's and fom_band_tables.hip's.  An extern "C" region is open only around entry
// points; every helper stands outside one.
#include "api_private.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>

namespace finrom {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int hip_fail(hipError_t e, const char* what) {
  g_err = std::string(what) + ": " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")";
  return FINROM_ERR_HIP;
}

// ---- stream capture registry, deferred frees (finrom_internal.h) ----------------------------------------------------------
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

extern "C" {

// ---------------------------------------------------------------------------------------
// FOM
// ---------------------------------------------------------------------------------------
int finrom_fom_create(const finrom_fom_desc* a, finrom_fom_t* out) {
  if (!a || !out) { set_error("fom_create: null argument"); return FINROM_ERR_ARG; }
  *out = nullptr;
  const int n = a->n, nnzL = a->nnzL;
  if (n <= 0 || nnzL < n || a->xdim <= 0 || a->n_obs < 0 || a->nasm < 0 || a->n_alist < 0 || a->cache_slots < 1 ||
      a->cache_slots > 126 || (a->fwd_chunk != 8 && a->fwd_chunk != 16) || a->nops_fwd < 2 * a->fwd_chunk ||
      a->nops_bwd < 2 * VM_CHUNK || a->nops_fwd % (2 * a->fwd_chunk) || a->nops_bwd % (2 * VM_CHUNK)) {
    set_error("fom_create: inconsistent sizes"); return FINROM_ERR_ARG;
  }
  // validate every index the kernels will dereference (a bad index would fault the GPU) and
  // the prefetch rule of the op streams
  auto bad = [&](const char* what) { set_error(std::string("fom_create: invalid ") + what); return FINROM_ERR_ARG; };
  const int gsize = nnzL + 2 * n;
  if ((int64_t)(nnzL + 3 * (int64_t)n) * 512 >= (int64_t)1 << 31) { set_error("fom_create: value vector too long for 32-bit buffer offsets"); return FINROM_ERR_UNSUPPORTED; }
  for (int t = 0; t < a->n_alist; ++t) if (a->a_list[t] < 0 || a->a_list[t] >= nnzL) return bad("a_list");
  if (a->asm_ptr[0] != 0 || a->asm_ptr[nnzL] != a->nasm) return bad("asm_ptr");
  for (int e = 0; e < nnzL; ++e) if (a->asm_ptr[e + 1] < a->asm_ptr[e]) return bad("asm_ptr");
  for (int t = 0; t < a->nasm; ++t) if (a->asm_idx[t] < 0 || a->asm_idx[t] >= a->xdim) return bad("asm_idx");
  int fused = 0;
  if (a->n_imm < 0 || (a->n_imm > 0 && !a->imm)) return bad("imm");
  {
    std::vector<int> stored(gsize, -10);
    std::vector<char> slot_set(std::max(a->cache_slots, 1), 0);      // row-cache slots that have been written (FINOFF)
    auto need = [&](int g, int c) { return g >= 0 && g < gsize && stored[g] + 2 <= c; };
    for (int t = 0; t < a->nops_fwd; ++t) {
      const int k = a->fwd_kind[t], A = a->fwd_a[t], B = a->fwd_b[t], D = a->fwd_d[t], c = t / a->fwd_chunk;
      if (A < -1 || A >= gsize) return bad("forward op operand index");     // fetched for every op, used or not
      switch (k) {
        case 0: if ((A >= 0 && !need(A, c)) || A < -1 || B < 0 || B >= a->cache_slots + 2) return bad("forward FMA op"); break;
        case 3: case 4: if (!need(A, c)) return bad("forward LDX/FMAX op"); break;
        case 5: if (!need(A, c) || D < 0 || D >= nnzL || B < -1 || B >= a->cache_slots) return bad("forward FINOFF op"); stored[D] = c;
                if (B >= 0) slot_set[B] = 1;
                break;
        case 11: if (B < 0 || B >= a->cache_slots || D < 0 || D >= a->cache_slots || !slot_set[B] || !slot_set[D]) return bad("forward FMALL op"); break;
        case 6: if (D < 0 || D >= nnzL || B < 0 || B >= n) return bad("forward FINDIAG op"); stored[D] = c; stored[nnzL + B] = c; break;
        case 7: if (D < 0 || D >= n) return bad("forward YSET op"); break;
        case 9: if (a->xdim > FOM_MAX_FUSED_X || B < 0 || B >= a->xdim || D < 0 || D >= a->n_imm) return bad("forward XFMA op"); fused = 1; break;
        case 10: if (a->xdim > FOM_MAX_FUSED_X || D < 0 || D >= a->n_imm) return bad("forward CADD op"); fused = 1; break;
        case 8: if (D < nnzL + n || D >= gsize) return bad("forward FINY op"); stored[D] = c; break;
        default: return bad("forward op kind");
      }
      if (t >= a->nops_fwd - 2 * a->fwd_chunk && (k != 0 || B != a->cache_slots + 1)) return bad("forward stream tail (must be padding)");
    }
    std::fill(stored.begin(), stored.end(), -10);
    auto need1 = [&](int g, int c) { return g >= 0 && g < gsize && stored[g] + 2 <= c; };   // backward: same look-ahead as forward
    for (int t = 0; t < a->nops_bwd; ++t) {
      const int k = a->bwd_kind[t], A = a->bwd_a[t], B = a->bwd_b[t], D = a->bwd_d[t], c = t / VM_CHUNK;
      if (A < -1 || A >= gsize || B < -1 || B >= gsize) return bad("backward op operand index");
      switch (k) {
        case 0: break;
        case 1: if (!need1(A, c) || !need1(B, c)) return bad("backward WFMA op"); break;
        case 3: if (!need1(A, c)) return bad("backward WSET op"); break;
        case 5: if (!need1(A, c) || D < nnzL + n || D >= gsize) return bad("backward WFIN op"); stored[D] = c; break;
        default: return bad("backward op kind");
      }
      if (t >= a->nops_bwd - 2 * VM_CHUNK && k != 0) return bad("backward stream tail (must be NOP padding)");
    }
  }
  if (a->n_obs > 0) {
    if (a->obs_ptr[0] != 0) return bad("obs_ptr");
    for (int o = 0; o < a->n_obs; ++o) if (a->obs_ptr[o + 1] < a->obs_ptr[o]) return bad("obs_ptr");
    for (int t = 0; t < a->obs_ptr[a->n_obs]; ++t) if (a->obs_idx[t] < 0 || a->obs_idx[t] >= n) return bad("obs_idx");
  }
  {
    std::vector<char> seen(n, 0);
    for (int i = 0; i < n; ++i) { int v = a->perm[i]; if (v < 0 || v >= n || seen[v]) return bad("perm"); seen[v] = 1; }
  }

  auto* h = new finrom_fom_s();
  FomDev& d = h->d;
  d.n = n; d.nnzL = nnzL; d.xdim = a->xdim; d.n_obs = a->n_obs; d.n_alist = a->n_alist; d.cache_slots = a->cache_slots;
  d.gsize = gsize;
  d.fwd_chunk = a->fwd_chunk;
  d.nchunks_fwd = a->nops_fwd / a->fwd_chunk - 2; d.nchunks_bwd = a->nops_bwd / VM_CHUNK - 2;
  d.trace = nullptr;
  d.has_grad = 0; d.nchunks_res = 0;
  std::vector<int> fkb(a->nops_fwd), bkb(a->nops_bwd);
  // device encoding of the forward stream: load offsets in bytes, the common multiply-adds (FMA, FMALL) carry the LDS
  // byte offsets of their row-cache slots in kb and d, every other op kind | (b+1) << 8, and one bit mask per chunk flags
  // the slots that are NOT plain multiply-adds (bits 0..15) and the multiply-adds whose second operand is in LDS (bits 16..31)
  std::vector<int> fa2(a->nops_fwd), fd2(a->nops_fwd), fmask(a->nops_fwd / a->fwd_chunk, 0);
  for (int t = 0; t < a->nops_fwd; ++t) {
    // ops without a global operand (padding, fused-assembly ops) fetch from beyond the buffer's range: the hardware
    // bounds check returns 0 without touching memory (a real element could be uninitialised: 0 * NaN)
    fa2[t] = a->fwd_a[t] < 0 ? 0x7FFFFFF0 : a->fwd_a[t] * 512;
    fd2[t] = a->fwd_d[t];
    // the common multiply-add is acc -= rc[b] * (G[a] + rc[d']): FMA reads the ZERO slot as d', FMALL an out-of-range G[a]
    // the common multiply-add is acc -= rc[b] * (G[a] + rc[d']): FMA reads the ZERO slot as d', FMALL an out-of-range G[a]
    if (a->fwd_kind[t] == 0) { fkb[t] = a->fwd_b[t] * 512; fd2[t] = (a->cache_slots + 1) * 512; }
    else if (a->fwd_kind[t] == 11) { fkb[t] = a->fwd_b[t] * 512; fd2[t] = a->fwd_d[t] * 512;
                                       fmask[t / a->fwd_chunk] |= 1 << (16 + t % a->fwd_chunk); }     // second operand in LDS
    else { fkb[t] = a->fwd_kind[t] | ((a->fwd_b[t] + 1) << 8); fmask[t / a->fwd_chunk] |= 1 << (t % a->fwd_chunk); }
  }
  // backward stream on the device: byte offsets of both operands (out of range = no operand: the fetch returns 0 without
  // touching memory) and kind | d << 8
  std::vector<int> ba2(a->nops_bwd), bb2(a->nops_bwd);
  for (int t = 0; t < a->nops_bwd; ++t) {
    const int k = a->bwd_kind[t];
    ba2[t] = (k == 0 || a->bwd_a[t] < 0) ? 0x7FFFFFF0 : a->bwd_a[t] * 512;
    bb2[t] = (k != 1 || a->bwd_b[t] < 0) ? 0x7FFFFFF0 : a->bwd_b[t] * 512;
    bkb[t] = k | ((k == 5 ? a->bwd_d[t] : 0) << 8);
  }
  int rc = 0;
  const int nobsnz = a->n_obs > 0 ? a->obs_ptr[a->n_obs] : 0;
  // assembly records: {entry, idx0..3, first/last of the remaining terms, 0} and {c0, w0..3}; unused slots
  // multiply parameter 0 by a zero weight
  std::vector<int> reci((size_t)a->n_alist * 8, 0);
  std::vector<double> recd((size_t)a->n_alist * 5, 0.0);
  for (int t = 0; t < a->n_alist; ++t) {
    const int e = a->a_list[t], t0 = a->asm_ptr[e], t1 = a->asm_ptr[e + 1];
    reci[t * 8 + 0] = e; recd[t * 5 + 0] = a->asm_c0[e];
    for (int k = 0; k < 4 && t0 + k < t1; ++k) { reci[t * 8 + 1 + k] = a->asm_idx[t0 + k]; recd[t * 5 + 1 + k] = a->asm_w[t0 + k]; }
    reci[t * 8 + 5] = std::min(t0 + 4, t1); reci[t * 8 + 6] = t1;
  }
  if (!rc) rc = up(h->owned, &d.asm_rec_i, reci.data(), reci.size());
  if (!rc) rc = up(h->owned, &d.asm_rec_d, recd.data(), recd.size());
  if (!rc) rc = up(h->owned, &d.asm_idx, a->asm_idx, a->nasm);
  if (!rc) rc = up(h->owned, &d.asm_w, a->asm_w, a->nasm);
  if (!rc) rc = up(h->owned, &d.rhs, a->rhs, n);
  if (!rc) rc = up(h->owned, &d.f_a, fa2.data(), fa2.size());
  if (!rc) rc = up(h->owned, &d.f_mask, fmask.data(), fmask.size());
  d.fused = fused;
  if (fused && a->n_alist != 0) { finrom_fom_destroy(h); set_error("fom_create: a fused stream must come with n_alist = 0"); return FINROM_ERR_ARG; }
  if (!rc) rc = up(h->owned, &d.f_imm, a->imm, (size_t)a->n_imm);
  if (!rc) rc = up(h->owned, &d.f_kb, fkb.data(), fkb.size());
  if (!rc) rc = up(h->owned, &d.f_d, fd2.data(), fd2.size());
  if (!rc) rc = up(h->owned, &d.b_a, ba2.data(), ba2.size());
  if (!rc) rc = up(h->owned, &d.b_b, bb2.data(), bb2.size());
  if (!rc) rc = up(h->owned, &d.b_kd, bkb.data(), bkb.size());
  if (!rc) rc = up(h->owned, &d.obs_ptr, a->obs_ptr, a->n_obs + 1);
  if (!rc) rc = up(h->owned, &d.obs_idx, a->obs_idx, nobsnz);
  if (!rc) rc = up(h->owned, &d.obs_w, a->obs_w, nobsnz);
  if (!rc) rc = up(h->owned, &d.perm, a->perm, n);
  if (rc) { finrom_fom_destroy(h); return rc; }
  *out = h;
  return 0;
}

void finrom_fom_destroy(finrom_fom_t h) {
  if (!h) return;
  for (void* p : h->owned) dev_free(p);                 // (queued while a stream capture is open: finrom_internal.h)
  h->xT.release(); h->Gw.release(); h->gradT.release(); h->qtmp.release(); h->hgrad.release();
  delete h;
}

}  // extern "C"
namespace finrom {
// FINROM_NO_BAND (A/B: the interpreter although the mesh has a band plan): read once per process, by whichever of
// fom_solve_stages, finrom_fom_gradient and finrom_solve_pairs is called first; all three see that value
bool env_no_band() { static const bool v = getenv("FINROM_NO_BAND") != nullptr; return v; }
// equal pieces when the batch exceeds the workspace bound `limit` (a short last piece would leave the GPU mostly idle)
static int64_t fom_equal_chunk(int64_t S, int64_t limit) {
  const int64_t npieces = (S + limit - 1) / limit;
  return npieces <= 1 ? limit : ((S + npieces - 1) / npieces + 63) / 64 * 64;
}
// stages: 1 = pack + assembly, 2 = interpreter (+ unpack of w), 3 = both.  finrom_solve_pairs runs stage 1, then
// launches the ROM half, then stage 2 (only possible when the batch fits one workspace chunk).
int64_t fom_chunk_samples(const FomDev& d, const BandDev* band) {
  // bound the per-call workspace (L values dominate: nnzL * 8 B per sample)
  const size_t per_sample = ((size_t)(band && band->on ? band->gsize : d.gsize) + d.xdim) * sizeof(double);
  // (FINROM_FOM_WORKSPACE_BYTES=<n>, read per call: another bound, so that a test can make a small batch run in pieces)
  const char* env_ws = getenv("FINROM_FOM_WORKSPACE_BYTES");
  const int64_t bound = env_ws != nullptr && atoll(env_ws) > 0 ? (int64_t)atoll(env_ws) : (int64_t)((size_t)48 << 30);
  const int64_t chunk = bound / (int64_t)per_sample;
  return std::max<int64_t>(64, chunk / 64 * 64);
}
int fom_solve_stages(finrom_fom_t h, const double* x, int64_t S, double* qoi, double* w, int32_t* info, hipStream_t st, int stages,
                     bool records) {
  const FomDev& d = h->d;
  const bool no_band = env_no_band();
  // Small batches: where the mesh has a band plan the band sweep serves them too -- ONE wave walking its 1597 pivots takes 1.7 ms
  // (QoI only) / 2.3 ms (with w) at m = 12 and 4.2 / 4.4 ms at m = 20, the level-scheduled small-batch kernel 2.7 and 17.9 ms
  // (tools/fom_small_vs_band.py) -- so the latency-oriented schedule (one workgroup per sample) is the forward path only of
  // meshes without window sizes (m >= 32); finrom_fom_gradient keeps it for small batches (its adjoint stage beats a lone wave
  // of the band adjoint kernel: 3.1 against 10 ms).
  if (h->small.small_max > 0 && S <= h->small.small_max && !(h->band.on && !no_band)) {
    int rc;
    if (!h->small.in_lds && (rc = h->Gw.reserve((size_t)S * d.gsize * sizeof(double)))) return rc;
    if (!(stages & 2)) return 0;
    h->last_path = h->small.in_lds ? FINROM_FOM_PATH_SMALL_LDS : FINROM_FOM_PATH_SMALL_GLOBAL;
    return launch_fom_small(d, h->small, x, S, (double*)h->Gw.p, qoi, w, info, st);
  }
  if (h->band.on && !no_band) {
    const BandDev& b = h->band_for(w != nullptr);        // (the half plan of a mirror-symmetric operator when nobody wants w)
    const FomDev& basm = &b == &h->band_m ? h->band_m_asm : h->band_asm;
    h->last_path = band_path(b, w == nullptr);
    const int64_t chunk = fom_equal_chunk(S, fom_chunk_samples(d, &b));
    for (int64_t s0 = 0; s0 < S; s0 += chunk) {
      const int64_t Sc = std::min(chunk, S - s0), nblk = (Sc + 63) / 64;
      int rc;
      if (stages & (1 | 4)) {                            // (4: reserve the workspace only -- finrom_solve_pairs, before its fork)
        if ((rc = h->xT.reserve((size_t)nblk * d.xdim * 64 * sizeof(double)))) return rc;
        if ((rc = h->Gw.reserve((size_t)nblk * b.gsize * 64 * sizeof(double)))) return rc;
      }
      if (stages & 1) {
        if ((rc = launch_pack(x + s0 * d.xdim, Sc, d.xdim, (double*)h->xT.p, st))) return rc;
        if ((rc = launch_fom_assemble(basm, (const double*)h->xT.p, nblk, (double*)h->Gw.p, st))) return rc;
      }
      if (stages & 2) {
        BandFnDev fnl = h->band_m_fn;
        if (!records) fnl.fin_rec = nullptr, fnl.post_rec = nullptr;      // (the sweep reads the tables themselves)
        const BandFnDev* fn = &b == &h->band_m && fnl.cw != nullptr ? &fnl : nullptr;
        if ((rc = launch_fom_band(b, (double*)h->Gw.p, nblk, Sc, qoi ? qoi + s0 * d.n_obs : nullptr, info ? info + s0 : nullptr, st, w == nullptr, fn))) return rc;
        if (w && (rc = launch_unpack((const double*)h->Gw.p, Sc, d.n, b.gsize, b.offY, b.perm, w + s0 * d.n, st))) return rc;
      }
    }
    return 0;
  }
  h->last_path = FINROM_FOM_PATH_INTERPRETER;
  const int64_t chunk = fom_equal_chunk(S, fom_chunk_samples(d));
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t Sc = std::min(chunk, S - s0);
    const int64_t nblk = (Sc + 63) / 64;
    int rc;
    if (stages & (1 | 4)) {
      if ((rc = h->xT.reserve((size_t)nblk * d.xdim * 64 * sizeof(double)))) return rc;
      if ((rc = h->Gw.reserve((size_t)nblk * d.gsize * 64 * sizeof(double)))) return rc;
    }
    if (stages & 1) {
      if ((rc = launch_pack(x + s0 * d.xdim, Sc, d.xdim, (double*)h->xT.p, st))) return rc;
      if (!d.fused && (rc = launch_fom_assemble(d, (const double*)h->xT.p, nblk, (double*)h->Gw.p, st))) return rc;
    }
    if (stages & 2) {
      if ((rc = launch_fom(d, (const double*)h->xT.p, nblk, Sc, (double*)h->Gw.p, qoi ? qoi + s0 * d.n_obs : nullptr, info ? info + s0 : nullptr, st))) return rc;
      if (w && (rc = launch_unpack_w(d, (const double*)h->Gw.p, Sc, w + s0 * d.n, st))) return rc;
    }
  }
  return 0;
}
}  // namespace finrom
extern "C" {

int finrom_fom_solve(finrom_fom_t h, const double* x, int64_t S, double* qoi, double* w, int32_t* info, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!x || (!qoi && h->d.n_obs > 0)))) { set_error("fom_solve: bad argument"); return FINROM_ERR_ARG; }
  return fom_solve_stages(h, x, S, qoi, w, info, (hipStream_t)stream, 3);
}

int finrom_fom_last_path(finrom_fom_t h) {
  if (!h) { set_error("fom_last_path: null handle"); return FINROM_ERR_ARG; }
  return h->last_path;
}

int finrom_fom_set_small_max(finrom_fom_t h, int32_t small_max) {
  if (!h || small_max < 0) { set_error("fom_set_small_max: bad argument"); return FINROM_ERR_ARG; }
  if (small_max > 0 && h->small.rec == nullptr) { set_error("fom_set_small_max: finrom_fom_set_small has not been called"); return FINROM_ERR_ARG; }
  h->small.small_max = small_max;
  return 0;
}

int finrom_fom_set_small(finrom_fom_t h, const finrom_fom_small_desc* a) {
  if (!h || !a || a->small_max < 0 || a->npairs < 0 || a->nasm < 0 || a->nlev_f <= 0 || a->nlev_b <= 0) { set_error("fom_set_small: bad argument"); return FINROM_ERR_ARG; }
  const FomDev& d = h->d;
  const int n = d.n, nnzL = d.nnzL;
  auto bad = [&](const char* what) { set_error(std::string("fom_set_small: invalid ") + what); return FINROM_ERR_ARG; };
  // every index the kernel dereferences, and the level property (a row only reads rows of lower levels)
  if (a->row_ptr[0] != 0 || a->row_ptr[n] != nnzL) return bad("row_ptr");
  std::vector<int> ent_row(nnzL);
  for (int i = 0; i < n; ++i) {
    if (a->row_ptr[i + 1] <= a->row_ptr[i]) return bad("row_ptr");
    for (int e = a->row_ptr[i]; e < a->row_ptr[i + 1]; ++e) {
      ent_row[e] = i;
      const int j = a->ent_col[e];
      if (j < 0 || j > i || (e == a->row_ptr[i + 1] - 1) != (j == i)) return bad("ent_col (diagonal must close its row)");
    }
  }
  if (a->pair_ptr[0] != 0 || a->pair_ptr[nnzL] != a->npairs) return bad("pair_ptr");
  if (a->asm_ptr[0] != 0 || a->asm_ptr[nnzL] != a->nasm) return bad("asm_ptr");
  for (int e = 0; e < nnzL; ++e) {
    if (a->pair_ptr[e + 1] < a->pair_ptr[e] || a->asm_ptr[e + 1] < a->asm_ptr[e]) return bad("pair_ptr / asm_ptr");
    for (int k = a->pair_ptr[e]; k < a->pair_ptr[e + 1]; ++k) {
      const int pa = a->pair_a[k], pb = a->pair_b[k];
      if (pa < a->row_ptr[ent_row[e]] || pa >= e || pb < 0 || pb >= nnzL || ent_row[pb] != a->ent_col[e]) return bad("pair");
    }
  }
  for (int t = 0; t < a->nasm; ++t) if (a->asm_idx[t] < 0 || a->asm_idx[t] >= d.xdim) return bad("asm_idx");
  if (a->col_ptr[0] != 0 || a->col_ptr[n] != nnzL - n) return bad("col_ptr");
  for (int j = 0; j < n; ++j) {
    if (a->col_ptr[j + 1] < a->col_ptr[j]) return bad("col_ptr");
    for (int c = a->col_ptr[j]; c < a->col_ptr[j + 1]; ++c) {
      const int e = a->col_ent[c];
      if (e < 0 || e >= nnzL || a->ent_col[e] != j || ent_row[e] != a->col_row[c] || a->col_row[c] <= j) return bad("column view");
    }
  }
  auto levels_ok = [&](const int* ptr, const int* rows, int nlev, bool forward) {
    if (ptr[0] != 0 || ptr[nlev] != n) return false;
    std::vector<int> lev(n, -1);
    for (int l = 0; l < nlev; ++l) {
      if (ptr[l + 1] < ptr[l]) return false;
      for (int t = ptr[l]; t < ptr[l + 1]; ++t) { const int i = rows[t]; if (i < 0 || i >= n || lev[i] >= 0) return false; lev[i] = l; }
    }
    for (int i = 0; i < n; ++i) {
      if (lev[i] < 0) return false;
      if (forward) { for (int e = a->row_ptr[i]; e < a->row_ptr[i + 1] - 1; ++e) if (lev[a->ent_col[e]] >= lev[i]) return false; }
      else { for (int c = a->col_ptr[i]; c < a->col_ptr[i + 1]; ++c) if (lev[a->col_row[c]] >= lev[i]) return false; }
    }
    return true;
  };
  if (!levels_ok(a->lev_ptr_f, a->lev_rows_f, a->nlev_f, true)) return bad("forward levels");
  if (!levels_ok(a->lev_ptr_b, a->lev_rows_b, a->nlev_b, false)) return bad("backward levels");
  FomSmallDev q;
  int rc = 0;
  // device layout for latency: a stream of fixed-size records (see FomSmallRec), (entry, row) column items as 8-B items
  std::vector<FomSmallRec> rec;
  std::vector<int> rec_ptr(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    for (int e = a->row_ptr[i]; e < a->row_ptr[i + 1]; ++e) {
      const int k0 = a->pair_ptr[e], np = a->pair_ptr[e + 1] - k0, t0 = a->asm_ptr[e], nt = a->asm_ptr[e + 1] - t0;
      const int nrec = std::max(1, std::max((np + 15) / 16, (nt + 7) / 8));
      for (int c = 0; c < nrec; ++c) {
        FomSmallRec r{};
        r.e = e; r.col = a->ent_col[e];
        r.npair = std::max(0, std::min(16, np - 16 * c));
        for (int u = 0; u < r.npair; ++u) r.first[u] = int2{a->pair_a[k0 + 16 * c + u], a->pair_b[k0 + 16 * c + u]};
        const int ntc = std::max(0, std::min(8, nt - 8 * c));
        for (int u = 0; u < ntc; ++u) { r.aidx[u] = a->asm_idx[t0 + 8 * c + u]; r.aw[u] = a->asm_w[t0 + 8 * c + u]; }
        r.c0 = c == 0 ? a->asm_c0[e] : 0.0;
        r.flags = (c == nrec - 1 ? 1 : 0) | (r.col == i ? 2 : 0) | ((ntc > 0 || r.c0 != 0.0) ? 4 : 0);
        rec.push_back(r);
      }
    }
    rec_ptr[i + 1] = (int)rec.size();
  }
  rec.resize(rec.size() + 6, FomSmallRec{});
  std::vector<int2> colv((size_t)(nnzL - n) + 8, int2{0, 0});
  for (int c = 0; c < nnzL - n; ++c) colv[c] = int2{a->col_ent[c], a->col_row[c]};
  if (!rc) rc = up(h->owned, &q.row_ptr, a->row_ptr, n + 1);
  if (!rc) rc = up(h->owned, &q.ent_col, a->ent_col, nnzL);
  if (!rc) rc = up(h->owned, &q.rec_ptr, rec_ptr.data(), rec_ptr.size());
  if (!rc) rc = up(h->owned, &q.rec, rec.data(), rec.size());
  if (!rc) rc = up(h->owned, &q.col_ptr, a->col_ptr, n + 1);
  if (!rc) rc = up(h->owned, &q.colv, colv.data(), colv.size());
  if (!rc) rc = up(h->owned, &q.lev_ptr_f, a->lev_ptr_f, a->nlev_f + 1);
  if (!rc) rc = up(h->owned, &q.lev_rows_f, a->lev_rows_f, n);
  if (!rc) rc = up(h->owned, &q.lev_ptr_b, a->lev_ptr_b, a->nlev_b + 1);
  if (!rc) rc = up(h->owned, &q.lev_rows_b, a->lev_rows_b, n);
  if (rc) return rc;
  q.small_max = a->small_max; q.nlev_f = a->nlev_f; q.nlev_b = a->nlev_b;
  q.in_lds = (size_t)(nnzL + 3 * n + d.xdim) * sizeof(double) <= (size_t)156 * 1024;      // value vector (+ adjoint region) + x
  h->small = q;
  return 0;
}

}  // extern "C"
// Device tables of a validated band descriptor for a problem of n dofs and n_obs computed observation rows (the handle's own
// sizes for finrom_fom_set_band, the half problem's for finrom_fom_set_band_mirror): the sweep's BandDev and the parameters of
// its assembly pre-pass.  The handle owns the uploads.
static int build_band(finrom_fom_t h, const finrom_fom_band_desc* a, int n, int n_obs, int64_t gsize, int64_t nL, BandDev* b_out, FomDev* asm_out) {
  struct { int n, xdim, n_obs; } d{n, h->d.xdim, n_obs};
  const int G = a->nfins * (a->npf + a->nif) + a->npost, nift = a->nif * (a->nif + 1) / 2;
  BandDev b{};
  b.n = n; b.n_obs = d.n_obs; b.xdim = d.xdim; b.gsize = (int)gsize; b.nAB = a->nAB; b.nL = (int)nL; b.nLx = a->nLx;
  b.NSF = a->NSF; b.NSP = a->NSP; b.NX = a->NX; b.nfins = a->nfins; b.npf = a->npf; b.nif = a->nif; b.npost = a->npost;
  b.post_g0 = a->nfins * (a->npf + a->nif); b.post_e0 = a->nfins * a->npf; b.post_L0 = a->nfins * a->npf * a->NSF;
  b.offL = a->nAB; b.offLx = a->nAB + (int)nL; b.offY = a->nAB + (int)nL + a->nLx; b.offX = b.offY + n;
  b.offV = b.offX + band_xsize(a->NSP);
  // records of the assembly pre-pass (fom_assemble_kernel): every value slot, so that special slots start at zero
  std::vector<int> reci((size_t)a->nAB * 8, 0);
  std::vector<double> recd((size_t)a->nAB * 5, 0.0);
  for (int e = 0; e < a->nAB; ++e) {
    const int t0 = a->ab_ptr[e], t1 = a->ab_ptr[e + 1];
    reci[e * 8 + 0] = e; recd[e * 5 + 0] = a->ab_c0[e];
    for (int k = 0; k < 4 && t0 + k < t1; ++k) { reci[e * 8 + 1 + k] = a->ab_idx[t0 + k]; recd[e * 5 + 1 + k] = a->ab_w[t0 + k]; }
    reci[e * 8 + 5] = std::min(t0 + 4, t1); reci[e * 8 + 6] = t1;
  }
  FomDev& q = *asm_out;
  q = FomDev{};
  q.xdim = d.xdim; q.gsize = (int)gsize; q.n_alist = a->nAB;
  int rc = 0;
  const int necp = a->ecp_ptr[a->npost], nobsnz = d.n_obs > 0 ? a->obs_ptr[d.n_obs] : 0;
  if (!rc) rc = up(h->owned, &q.asm_rec_i, reci.data(), reci.size());
  if (!rc) rc = up(h->owned, &q.asm_rec_d, recd.data(), recd.size());
  if (!rc) rc = up(h->owned, &q.asm_idx, a->ab_idx, a->nterms);
  if (!rc) rc = up(h->owned, &q.asm_w, a->ab_w, a->nterms);
  if (!rc) rc = up(h->owned, &b.abmap, a->abmap, (size_t)3 * G);
  if (!rc) rc = up(h->owned, &b.Fg, a->Fg, G);
  if (!rc) rc = up(h->owned, &b.act, a->act, a->npost);
  if (!rc) rc = up(h->owned, &b.lx_ptr, a->lx_ptr, a->npost + 1);
  if (!rc) rc = up(h->owned, &b.ent_extra, a->ent_extra, a->npost);
  if (!rc) rc = up(h->owned, &b.ecp_ptr, a->ecp_ptr, a->npost + 1);
  if (!rc) rc = up(h->owned, &b.ecp_slot, a->ecp_slot, necp);
  if (!rc) rc = up(h->owned, &b.ecp_off, a->ecp_off, necp);
  if (!rc) rc = up(h->owned, &b.schur_off, a->schur_off, (size_t)a->nfins * nift);
  if (!rc) rc = up(h->owned, &b.iface_elim, a->iface_elim, (size_t)a->nfins * a->nif);
  if (!rc) rc = up(h->owned, &b.perm, a->perm, n);
  if (!rc) rc = up(h->owned, &b.obs_ptr, a->obs_ptr, d.n_obs + 1);
  if (!rc) rc = up(h->owned, &b.obs_idx, a->obs_idx, nobsnz);
  if (!rc) rc = up(h->owned, &b.obs_w, a->obs_w, nobsnz);
  if (a->qoi_FgQ != nullptr) {
    const int nqz = a->qoi_obs_ptr[d.n_obs];
    if (!rc) rc = up(h->owned, &b.FgQ, a->qoi_FgQ, G);
    if (!rc) rc = up(h->owned, &b.row_fin, a->qoi_row_fin, d.n_obs);
    if (!rc) rc = up(h->owned, &b.qobs_ptr, a->qoi_obs_ptr, d.n_obs + 1);
    if (!rc) rc = up(h->owned, &b.qobs_idx, a->qoi_obs_idx, nqz);
    if (!rc) rc = up(h->owned, &b.qobs_w, a->qoi_obs_w, nqz);
    b.qo = 1;
  }
  if (rc) return rc;
  b.on = getenv("FINROM_BAND_TIMING") != nullptr ? 2 : 1;      // 2: block 0 reports its phase clocks in sample 0's QoI (diagnostic)
  *b_out = b;
  return 0;
}
extern "C" {

int finrom_fom_set_band(finrom_fom_t h, const finrom_fom_band_desc* a) {
  if (!h || !a) { set_error("fom_set_band: null argument"); return FINROM_ERR_ARG; }
  const FomDev& d = h->d;
  int64_t gsize = 0, nL = 0;
  if (int rc = validate_band(a, d.n, d.xdim, d.n_obs, &gsize, &nL)) return rc;
  BandDev b{};
  if (int rc = build_band(h, a, d.n, d.n_obs, gsize, nL, &b, &h->band_asm)) return rc;
  h->band = b;
  h->band_m = BandDev{}; h->band_m_fn = BandFnDev{};      // (a half plan belongs to the plan it was installed beside)
  return 0;
}

int finrom_fom_set_band_mirror(finrom_fom_t h, const finrom_fom_band_desc* a, int32_t n_half, int32_t n_rows, const int32_t* out_ptr,
                               const int32_t* out_col) {
  if (!h || !a) { set_error("fom_set_band_mirror: null argument"); return FINROM_ERR_ARG; }
  if (!h->band.on) { set_error("fom_set_band_mirror: finrom_fom_set_band has not been called"); return FINROM_ERR_ARG; }
  const FomDev& d = h->d;
  if (n_half <= 0 || n_half > d.n) { set_error("fom_set_band_mirror: invalid n_half"); return FINROM_ERR_ARG; }
  int64_t gsize = 0, nL = 0;
  if (int rc = validate_band_mirror(a, n_half, d.xdim, n_rows, d.n_obs, out_ptr, out_col, &gsize, &nL)) return rc;
  BandDev b{};
  FomDev q{};
  if (int rc = build_band(h, a, n_half, n_rows, gsize, nL, &b, &q)) return rc;
  int rc = up(h->owned, &b.out_ptr, out_ptr, n_rows + 1);
  if (!rc) rc = up(h->owned, &b.out_col, out_col, d.n_obs);
  if (rc) return rc;
  b.n_out = d.n_obs;
  // The post as functionals, where the descriptor fits (FINROM_FOM_POST_STORED=1: the stored-factor form, the A/B switch).  The
  // workspace of that form is the value slots and the fins' g: the plan's sizes -- chunking, the pair path's reservation, the
  // assembly pre-pass's stride -- all follow gsize.
  BandFnDev fn{};
  if (getenv("FINROM_FOM_POST_STORED") == nullptr) {
    std::vector<double> cw; std::vector<int> piv_row, piv_off;
    const int fits = derive_post_functionals(a, n_half, n_rows, cw, piv_row, piv_off);
    if (fits < 0) return fits;
    if (fits) {
      rc = up(h->owned, &fn.cw, cw.data(), cw.size());
      if (!rc) rc = up(h->owned, &fn.piv_row, piv_row.data(), piv_row.size());
      if (!rc) rc = up(h->owned, &fn.piv_off, piv_off.data(), piv_off.size());
      if (!rc && getenv("FINROM_FOM_NO_PIVOT_RECORDS") == nullptr) {      // (the A/B switch: the sweep reads the tables themselves)
        std::vector<BandFinRec> fr; std::vector<BandPostRec> qr;
        derive_pivot_records(a, cw, piv_row, piv_off, fr, qr);
        if ((rc = check_pivot_records(a, cw, piv_row, piv_off, fr.data(), qr.data()))) return rc;
        fr.resize(fr.size() + band_rec_pad(a->NSF), BandFinRec{}); qr.resize(qr.size() + band_rec_pad(a->NSP), BandPostRec{});
        rc = up(h->owned, &fn.fin_rec, fr.data(), fr.size());
        if (!rc) rc = up(h->owned, &fn.post_rec, qr.data(), qr.size());
      }
      if (rc) return rc;
      b.offL = b.offLx = b.offX = b.offV = 0;             // (regions this form does not have)
      b.offY = a->nAB;
      b.gsize = q.gsize = a->nAB + a->nfins * a->nif;
    }
  }
  h->band_m = b; h->band_m_asm = q; h->band_m_fn = fn;
  return 0;
}

int finrom_fom_band_mirror_form(finrom_fom_t h) {
  if (!h || !h->band_m.on) return 0;
  return h->band_m_fn.cw != nullptr ? 2 : 1;
}

int finrom_fom_band_mirror_records_on(finrom_fom_t h) {
  return h && h->band_m.on && h->band_m_fn.post_rec != nullptr ? 1 : 0;
}

int finrom_fom_set_band_gradient(finrom_fom_t h, const finrom_fom_band_grad_desc* a) {
  if (!h || !a || !a->bt_ptr || !a->g_ptr) { set_error("fom_set_band_gradient: null argument"); return FINROM_ERR_ARG; }
  if (!h->band.on) { set_error("fom_set_band_gradient: finrom_fom_set_band has not been called"); return FINROM_ERR_ARG; }
  const FomDev& d = h->d;
  const int n = d.n;
  auto bad = [&](const char* what) { set_error(std::string("fom_set_band_gradient: invalid ") + what); return FINROM_ERR_ARG; };
  if (a->bt_ptr[0] != 0) return bad("bt_ptr");
  for (int i = 0; i < n; ++i) if (a->bt_ptr[i + 1] < a->bt_ptr[i]) return bad("bt_ptr");
  const int nbt = a->bt_ptr[n];
  if (nbt > 0 && (!a->bt_obs || !a->bt_w)) return bad("table pointer (null)");
  for (int t = 0; t < nbt; ++t) if (a->bt_obs[t] < 0 || a->bt_obs[t] >= d.n_obs) return bad("bt_obs");
  if (a->g_ptr[0] != 0) return bad("g_ptr");
  for (int j = 0; j < d.xdim; ++j) if (a->g_ptr[j + 1] < a->g_ptr[j]) return bad("g_ptr");
  const int ng = a->g_ptr[d.xdim];
  if (ng > 0 && (!a->g_a || !a->g_b || !a->g_w)) return bad("table pointer (null)");
  for (int t = 0; t < ng; ++t) if (a->g_a[t] < 0 || a->g_a[t] >= n || a->g_b[t] < 0 || a->g_b[t] >= n) return bad("g_a / g_b");
  BandGradDev g;
  int rc = 0;
  if (!rc) rc = up(h->owned, &g.bt_ptr, a->bt_ptr, n + 1);
  if (!rc) rc = up(h->owned, &g.bt_obs, a->bt_obs, nbt);
  if (!rc) rc = up(h->owned, &g.bt_w, a->bt_w, nbt);
  if (!rc) rc = up(h->owned, &g.g_ptr, a->g_ptr, d.xdim + 1);
  if (!rc) rc = up(h->owned, &g.g_a, a->g_a, ng);
  if (!rc) rc = up(h->owned, &g.g_b, a->g_b, ng);
  if (!rc) rc = up(h->owned, &g.g_w, a->g_w, ng);
  if (rc) return rc;
  g.on = 1;
  h->band_grad = g;
  return 0;
}

int finrom_fom_solve_rhs(finrom_fom_t h, const double* x, int64_t S, const double* rhs, int32_t nrhs, double* out, int32_t* info,
                         void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || nrhs < 0 || (S > 0 && nrhs > 0 && (!x || !rhs || !out))) { set_error("fom_solve_rhs: bad argument"); return FINROM_ERR_ARG; }
  if (!h->band.on) { set_error("fom_solve_rhs: needs the band sweep (finrom_fom_set_band)"); return FINROM_ERR_UNSUPPORTED; }
  if (S == 0 || nrhs == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const FomDev& d = h->d;
  const BandDev& b = h->band;
  h->last_path = band_path(b, false);
  const int64_t dr = (int64_t)nrhs * d.n;
  const size_t per_sample = ((size_t)b.gsize + d.xdim + 2 * (size_t)dr) * sizeof(double);
  const int64_t limit = std::max<int64_t>(64, (int64_t)((size_t)48 << 30) / (int64_t)per_sample / 64 * 64);
  for (int64_t s0 = 0; s0 < S; s0 += limit) {
    const int64_t Sc = std::min(limit, S - s0), nblk = (Sc + 63) / 64;
    int rc;
    if ((rc = h->xT.reserve((size_t)nblk * d.xdim * 64 * sizeof(double)))) return rc;
    if ((rc = h->Gw.reserve((size_t)nblk * b.gsize * 64 * sizeof(double)))) return rc;
    if ((rc = h->gradT.reserve((size_t)nblk * 2 * dr * 64 * sizeof(double)))) return rc;      // rhsT | outT
    if ((rc = h->qtmp.reserve((size_t)Sc * std::max(d.n_obs, 1) * sizeof(double)))) return rc;
    double* rhsT = (double*)h->gradT.p;
    double* outT = rhsT + (size_t)nblk * dr * 64;
    if ((rc = launch_pack(x + s0 * d.xdim, Sc, d.xdim, (double*)h->xT.p, st))) return rc;
    if ((rc = launch_fom_assemble(h->band_asm, (const double*)h->xT.p, nblk, (double*)h->Gw.p, st))) return rc;
    if ((rc = launch_fom_band(b, (double*)h->Gw.p, nblk, Sc, (double*)h->qtmp.p, info ? info + s0 : nullptr, st, false))) return rc;
    if ((rc = launch_pack(rhs + s0 * dr, Sc, (int)dr, rhsT, st))) return rc;
    if ((rc = launch_fom_band_resolve(b, (double*)h->Gw.p, nblk, nrhs, rhsT, outT, st))) return rc;
    if ((rc = launch_unpack(outT, Sc, (int)dr, dr, 0, nullptr, out + s0 * dr, st))) return rc;
  }
  return 0;
}

int finrom_fom_set_gradient(finrom_fom_t h, const finrom_fom_grad_desc* a) {
  if (!h || !a || a->nops_res < VM_CHUNK || a->nops_res % VM_CHUNK) { set_error("fom_set_gradient: bad argument"); return FINROM_ERR_ARG; }
  FomDev& d = h->d;
  const int n = d.n, nnzL = d.nnzL, gsize = nnzL + 3 * n;
  auto bad = [&](const char* what) { set_error(std::string("fom_set_gradient: invalid ") + what); return FINROM_ERR_ARG; };
  {
    std::vector<int> stored(gsize, -10);
    auto need1 = [&](int g, int c) { return g >= 0 && g < gsize && stored[g] + 1 <= c; };
    for (int t = 0; t < a->nops_res; ++t) {
      const int k = a->res_kind[t], A = a->res_a[t], B = a->res_b[t], D = a->res_d[t], c = t / VM_CHUNK;
      if (A < -1 || A >= gsize || B < -1 || B >= gsize) return bad("resolve op operand index");
      switch (k) {
        case 0: break;
        case 1: if (!need1(A, c) || !need1(B, c)) return bad("WFMA op"); break;
        case 3: if (!need1(A, c)) return bad("WSET op"); break;
        case 5: if (!need1(A, c) || D < nnzL + 2 * n || D >= gsize) return bad("WFIN op"); stored[D] = c; break;
        default: return bad("op kind");
      }
    }
  }
  if (a->bt_ptr[0] != 0) return bad("bt_ptr");
  for (int i = 0; i < n; ++i) if (a->bt_ptr[i + 1] < a->bt_ptr[i]) return bad("bt_ptr");
  for (int t = 0; t < a->bt_ptr[n]; ++t) if (a->bt_obs[t] < 0 || a->bt_obs[t] >= d.n_obs) return bad("bt_obs");
  if (a->g_ptr[0] != 0) return bad("g_ptr");
  for (int j = 0; j < d.xdim; ++j) if (a->g_ptr[j + 1] < a->g_ptr[j]) return bad("g_ptr");
  for (int t = 0; t < a->g_ptr[d.xdim]; ++t) if (a->g_a[t] < 0 || a->g_a[t] >= n || a->g_b[t] < 0 || a->g_b[t] >= n) return bad("g_a/g_b");
  std::vector<int> rkb(a->nops_res);
  for (int t = 0; t < a->nops_res; ++t) rkb[t] = a->res_kind[t] | ((a->res_b[t] + 1) << 8);
  int rc = 0;
  if (!rc) rc = up(h->owned, &d.r_a, a->res_a, a->nops_res);
  if (!rc) rc = up(h->owned, &d.r_kb, rkb.data(), rkb.size());
  if (!rc) rc = up(h->owned, &d.r_d, a->res_d, a->nops_res);
  if (!rc) rc = up(h->owned, &d.bt_ptr, a->bt_ptr, n + 1);
  if (!rc) rc = up(h->owned, &d.bt_obs, a->bt_obs, a->bt_ptr[n]);
  if (!rc) rc = up(h->owned, &d.bt_w, a->bt_w, a->bt_ptr[n]);
  if (!rc) rc = up(h->owned, &d.g_ptr, a->g_ptr, d.xdim + 1);
  if (!rc) rc = up(h->owned, &d.g_a, a->g_a, a->g_ptr[d.xdim]);
  if (!rc) rc = up(h->owned, &d.g_b, a->g_b, a->g_ptr[d.xdim]);
  if (!rc) rc = up(h->owned, &d.g_w, a->g_w, a->g_ptr[d.xdim]);
  if (rc) return rc;
  d.nchunks_res = a->nops_res / VM_CHUNK;
  d.has_grad = 1;
  d.gsize = gsize;                       // value vector grows by the adjoint region
  return 0;
}

int finrom_fom_gradient(finrom_fom_t h, const double* x, const double* data, int32_t data_per_sample, int64_t S,
                        double* grad, double* J, double* qoi, int32_t* info, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!x || !data || !grad || !J))) { set_error("fom_gradient: bad argument"); return FINROM_ERR_ARG; }
  if (!h->d.has_grad && !h->band_grad.on) { set_error("fom_gradient: finrom_fom_set_gradient has not been called"); return FINROM_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const FomDev& d = h->d;
  const bool no_band = env_no_band();
  const bool small = h->small.small_max > 0 && S <= h->small.small_max && d.n_obs <= 64 && d.has_grad;
  if (!small && h->band.on && h->band_grad.on && !no_band) {
    // the full band sweep (the factor and w stay in the workspace), then the adjoint solve and the contraction on the same layout
    const BandDev& b = h->band;
    h->last_path = band_path(b, false);
    const size_t per_sample = ((size_t)b.gsize + 2 * d.xdim) * sizeof(double);
    const int64_t limit = std::max<int64_t>(64, (int64_t)((size_t)48 << 30) / (int64_t)per_sample / 64 * 64);
    const int64_t chunk = fom_equal_chunk(S, limit);
    for (int64_t s0 = 0; s0 < S; s0 += chunk) {
      const int64_t Sc = std::min(chunk, S - s0), nblk = (Sc + 63) / 64;
      int rc;
      if ((rc = h->xT.reserve((size_t)nblk * d.xdim * 64 * sizeof(double)))) return rc;
      if ((rc = h->Gw.reserve((size_t)nblk * b.gsize * 64 * sizeof(double)))) return rc;
      if ((rc = h->gradT.reserve((size_t)nblk * d.xdim * 64 * sizeof(double)))) return rc;
      double* q = qoi ? qoi + s0 * d.n_obs : nullptr;
      if (!q) { if ((rc = h->qtmp.reserve((size_t)Sc * d.n_obs * sizeof(double)))) return rc; q = (double*)h->qtmp.p; }
      if ((rc = launch_pack(x + s0 * d.xdim, Sc, d.xdim, (double*)h->xT.p, st))) return rc;
      if ((rc = launch_fom_assemble(h->band_asm, (const double*)h->xT.p, nblk, (double*)h->Gw.p, st))) return rc;
      if ((rc = launch_fom_band(b, (double*)h->Gw.p, nblk, Sc, q, info ? info + s0 : nullptr, st, false))) return rc;
      if ((rc = launch_fom_band_adjoint(b, h->band_grad, (double*)h->Gw.p, nblk, Sc, q, data + (data_per_sample ? s0 * d.n_obs : 0),
                                        data_per_sample ? d.n_obs : 0, (double*)h->gradT.p, J + s0, st))) return rc;
      if ((rc = launch_unpack((const double*)h->gradT.p, Sc, d.xdim, d.xdim, 0, nullptr, grad + s0 * d.xdim, st))) return rc;
    }
    return 0;
  }
  if (!d.has_grad) { set_error("fom_gradient: finrom_fom_set_gradient has not been called (the band tables serve large batches only)"); return FINROM_ERR_ARG; }
  if (h->small.small_max > 0 && S <= h->small.small_max && d.n_obs <= 64) {      // small batch: value and gradient in one workgroup per sample
    int rc;
    if (!h->small.in_lds && (rc = h->Gw.reserve((size_t)S * d.gsize * sizeof(double)))) return rc;
    double* q = qoi;
    if (!q) { if ((rc = h->qtmp.reserve((size_t)S * d.n_obs * sizeof(double)))) return rc; q = (double*)h->qtmp.p; }
    FomSmallGrad g;
    g.data = data; g.data_stride = data_per_sample ? d.n_obs : 0; g.grad = grad; g.J = J;
    h->last_path = h->small.in_lds ? FINROM_FOM_PATH_SMALL_LDS : FINROM_FOM_PATH_SMALL_GLOBAL;
    return launch_fom_small(d, h->small, x, S, (double*)h->Gw.p, q, nullptr, info, st, g);
  }
  h->last_path = FINROM_FOM_PATH_INTERPRETER;
  const size_t per_sample = ((size_t)d.gsize + 2 * d.xdim) * sizeof(double);
  int64_t chunk = (int64_t)((size_t)48 << 30) / (int64_t)per_sample;
  chunk = std::max<int64_t>(64, chunk / 64 * 64);
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t Sc = std::min(chunk, S - s0);
    const int64_t nblk = (Sc + 63) / 64;
    int rc;
    if ((rc = h->xT.reserve((size_t)nblk * d.xdim * 64 * sizeof(double)))) return rc;
    if ((rc = h->Gw.reserve((size_t)nblk * d.gsize * 64 * sizeof(double)))) return rc;
    if ((rc = h->gradT.reserve((size_t)nblk * d.xdim * 64 * sizeof(double)))) return rc;
    double* q = qoi ? qoi + s0 * d.n_obs : nullptr;
    if (!q) { if ((rc = h->qtmp.reserve((size_t)Sc * d.n_obs * sizeof(double)))) return rc; q = (double*)h->qtmp.p; }
    if ((rc = launch_pack(x + s0 * d.xdim, Sc, d.xdim, (double*)h->xT.p, st))) return rc;
    if (!d.fused && (rc = launch_fom_assemble(d, (const double*)h->xT.p, nblk, (double*)h->Gw.p, st))) return rc;
    if ((rc = launch_fom(d, (const double*)h->xT.p, nblk, Sc, (double*)h->Gw.p, q, info ? info + s0 : nullptr, st))) return rc;
    if ((rc = launch_fom_adjoint(d, nblk, Sc, (double*)h->Gw.p, q, data + (data_per_sample ? s0 * d.n_obs : 0),
                                 data_per_sample ? d.n_obs : 0, (double*)h->gradT.p, J + s0, st))) return rc;
    if ((rc = launch_unpack((const double*)h->gradT.p, Sc, d.xdim, d.xdim, 0, nullptr, grad + s0 * d.xdim, st))) return rc;
  }
  return 0;
}

}  // extern "C"

extern "C" {

// ---------------------------------------------------------------------------------------
// ROM
// ---------------------------------------------------------------------------------------
int finrom_rom_create(const finrom_rom_desc* a, finrom_rom_t* out) {
  if (!a || !out) { set_error("rom_create: null argument"); return FINROM_ERR_ARG; }
  *out = nullptr;
  if (int rc = validate_rom_desc(a)) return rc;
  const int r = a->r, NB = (r + 15) / 16, rp = 16 * NB;
  if (NB > 13) { set_error("rom_create: basis size > 208 not supported"); return FINROM_ERR_UNSUPPORTED; }

  auto cnt = [&](int row) { return a->row_ptr[row + 1] - a->row_ptr[row]; };
  const std::vector<int> order = rows_by_term_count(a);
  auto* h = new finrom_rom_s();
  RomDev& d = h->d;
  d.n = a->n; d.r = r; d.rp = rp; d.NB = NB; d.P = a->P; d.n_obs = a->n_obs;
  d.solve_in_lds = rp <= 176 ? 1 : 0;
  d.trace = nullptr;
  auto push_slot = [&](std::vector<double>& T, std::vector<int>& Pi, const std::vector<int>& rows4, int t) {
    for (int q = 0; q < 4; ++q) {
      const size_t base = T.size();
      T.resize(base + rp, 0.0);
      int pi = 0;
      if (q < (int)rows4.size() && rows4[q] >= 0) {
        const int row = rows4[q], tt = a->row_ptr[row] + t;
        if (tt < a->row_ptr[row + 1]) { std::memcpy(&T[base], a->term_val + (size_t)tt * r, r * sizeof(double)); pi = a->term_p[tt]; }
      }
      Pi.push_back(pi);
    }
  };
  // ---- pattern-uniform k-steps for the single-wave kernels (see RomDev::tvu) ----------------------------------------------
  std::vector<double> tvu; std::vector<int> kmeta;
  {
    std::vector<KStep> ksteps = uniform_ksteps(a, order);
    // every term-count group gets an even number of k-steps (a k-step of zero rows pads it): the multi-wave main loop is
    // unrolled twice and specialised by term count, so that its phases start at even k-steps
    for (size_t k = 0; k < ksteps.size();) {
      size_t k1 = k;
      while (k1 < ksteps.size() && ksteps[k1].pat.size() == ksteps[k].pat.size()) ++k1;
      if ((k1 - k) % 2) { ksteps.insert(ksteps.begin() + k1, KStep{ksteps[k].pat, {-1, -1, -1, -1}}); ++k1; }
      k = k1;
    }
    for (int t = 0; t < 4; ++t) {
      d.uend[t] = 0;
      for (const KStep& ks : ksteps) if ((int)ks.pat.size() > t) ++d.uend[t];
    }
    int uslots = 0;
    for (size_t k = 0; k < ksteps.size(); ++k) {
      const int nt = (int)ksteps[k].pat.size();
      if (nt > 4) { delete h; set_error("rom_create: a row of psi has more than 4 terms"); return FINROM_ERR_UNSUPPORTED; }
      for (int t = 0; t < nt; ++t) {
        const int pp = ksteps[k].pat[t];
        for (int q = 0; q < 4; ++q) {
          const size_t base = tvu.size();
          tvu.resize(base + rp, 0.0);
          const int row = ksteps[k].rows[q];
          if (row < 0) continue;
          for (int tt = a->row_ptr[row]; tt < a->row_ptr[row + 1]; ++tt)
            if (a->term_p[tt] == pp) for (int col = 0; col < r; ++col) tvu[base + col] += a->term_val[(size_t)tt * r + col];
        }
      }
      uslots += nt;
    }
    // per-k-step records for the interleaved main loop: {first slot, term count, -, -, theta index of slots 0..3}; eight padding
    // k-steps point at the zero slots behind the table
    d.nku = (int)ksteps.size();
    {
      int sl = 0;
      for (size_t k = 0; k < ksteps.size(); ++k) {
        const int nt = (int)ksteps[k].pat.size();
        int rec[8] = {sl, nt, 0, 0, 0, 0, 0, 0};
        for (int t = 0; t < nt; ++t) rec[4 + t] = ksteps[k].pat[t];
        kmeta.insert(kmeta.end(), rec, rec + 8);
        sl += nt;
      }
      for (int k = 0; k < 8; ++k) { int rec[8] = {uslots, 1, 0, 0, 0, 0, 0, 0}; kmeta.insert(kmeta.end(), rec, rec + 8); }
    }
    tvu.resize(tvu.size() + (size_t)4 * 4 * rp, 0.0);       // one k-step of padding for the prefetch
    d.tvu_bytes = (int)std::min<size_t>(tvu.size() * sizeof(double), (size_t)0x7FFFFFF0);

    // ---- the same k-steps grouped by their leading parameter (build_grouped_tables above; proj_main_grouped, NB <= 5) ------
    d.n_ext = 0; d.nkg = 0; d.ext_final = 0; d.ext = nullptr;
    d.nkg_m = 0; d.kmg_m = 0; d.ext_final_m = 0; d.twin = nullptr;
    d.nkg_s = 0; d.kmg_s = 0; d.ext_final_s = 0; d.short_lo = 0.0; d.short_hi = 0.0;
    if (NB <= 5 && getenv("FINROM_PROJ_UNGROUPED") == nullptr) {
      GroupedTables gt;
      if (build_grouped_tables(a, ksteps, rp, gt)) {
        d.nkg = gt.nkg; d.n_ext = gt.n_ext; d.ext_final = gt.ext_final;
        h->tvg_host = gt.tvg; h->kmg_host = gt.kmg; h->def_host = gt.def;      // (finrom_rom_set_mirror appends the half list)
        d.tvg_bytes = (int)std::min<size_t>(gt.tvg.size() * sizeof(double), (size_t)0x7FFFFFF0);
        int grc = up(h->owned, &d.tvg, gt.tvg.data(), gt.tvg.size());
        if (!grc) grc = up(h->owned, &d.kmg, gt.kmg.data(), gt.kmg.size());
        if (!grc) grc = up(h->owned, &d.ext_def, gt.def.data(), gt.def.size());
        if (grc) { finrom_rom_destroy(h); return grc; }
      }
    }
  }
  // root rows (F != 0) for B_r = psi^T F
  std::vector<int> frows;
  for (int i = 0; i < a->n; ++i) if (a->rhs[i] != 0.0 && cnt(i) > 0) frows.push_back(i);
  d.rhs_nk = ((int)frows.size() + 3) / 4;
  d.rhs_nt = 0;
  for (int row : frows) d.rhs_nt = std::max(d.rhs_nt, cnt(row));
  std::vector<double> rtv, rf; std::vector<int> rpi;
  for (int ks = 0; ks < d.rhs_nk; ++ks) {
    std::vector<int> rows4;
    for (int q = 0; q < 4; ++q) {
      const int idx = ks * 4 + q;
      rows4.push_back(idx < (int)frows.size() ? frows[idx] : -1);
      rf.push_back(idx < (int)frows.size() ? a->rhs[frows[idx]] : 0.0);
    }
    for (int t = 0; t < d.rhs_nt; ++t) push_slot(rtv, rpi, rows4, t);
  }
  if (rtv.empty()) { rtv.assign(4 * rp, 0.0); rpi.assign(4, 0); rf.assign(4, 0.0); }

  // h_p = Psi_p^T F for the offline/online form of B_r
  std::vector<double> hp((size_t)(a->P + 1) * rp, 0.0);
  for (int i = 0; i < a->n; ++i) {
    if (a->rhs[i] == 0.0) continue;
    for (int t = a->row_ptr[i]; t < a->row_ptr[i + 1]; ++t)
      for (int col = 0; col < r; ++col) hp[(size_t)a->term_p[t] * rp + col] += a->rhs[i] * a->term_val[(size_t)t * r + col];
  }

  int rc = 0;
  if (!rc) rc = up(h->owned, &h->gram.h, hp.data(), hp.size());
  if (!rc) rc = up(h->owned, &d.tvu, tvu.data(), tvu.size());
  if (!rc) rc = up(h->owned, &d.kmeta, kmeta.data(), kmeta.size());
  if (!rc) rc = up(h->owned, &d.rhs_tv, rtv.data(), rtv.size());
  if (!rc) rc = up(h->owned, &d.rhs_pidx, rpi.data(), rpi.size());
  if (!rc) rc = up(h->owned, &d.rhs_f, rf.data(), rf.size());
  if (!rc) rc = up(h->owned, &d.obs_phi, a->obs_phi, (size_t)a->n_obs * r);
  if (rc) { finrom_rom_destroy(h); return rc; }
  *out = h;
  return 0;
}

}  // extern "C"
// a half list (finrom_rom_set_mirror / _short) appended behind the handle's grouped tables: records, rows and factors go behind
// what is there, everything is uploaded again; nd gets the new arrays and n_ext, kmg0 = where the list's records start
struct HostTables { std::vector<double> tvg; std::vector<int> kmg, def; };
static int append_half_list(finrom_rom_t h, const finrom_rom_desc* a, const double* row_weight, RomDev& nd, GroupedTables& g, int& kmg0,
                            HostTables& next, const char* who) {
  std::vector<int> kclass;
  const std::vector<KStep> ksteps = mirror_ksteps(a, row_weight, kclass);
  const int slot0 = (int)(h->tvg_host.size() / ((size_t)4 * nd.rp));
  if (!build_grouped_tables(a, ksteps, nd.rp, g, &kclass, slot0, nd.n_ext, short_scale_free(a, h->short_grouped))) { set_error(std::string(who) + ": the half descriptor has no grouped form"); return FINROM_ERR_UNSUPPORTED; }
  std::vector<double> tvg(h->tvg_host); tvg.insert(tvg.end(), g.tvg.begin(), g.tvg.end());
  std::vector<int> kmg(h->kmg_host); kmg.insert(kmg.end(), g.kmg.begin(), g.kmg.end());
  std::vector<int> def(h->def_host); def.insert(def.end(), g.def.begin(), g.def.end());
  if (tvg.size() * sizeof(double) > (size_t)0x7FFFFFF0) { set_error(std::string(who) + ": tables too large"); return FINROM_ERR_UNSUPPORTED; }
  int rc = up(h->owned, &nd.tvg, tvg.data(), tvg.size());
  if (!rc) rc = up(h->owned, &nd.kmg, kmg.data(), kmg.size());
  if (!rc) rc = up(h->owned, &nd.ext_def, def.data(), def.size());
  if (rc) return rc;
  kmg0 = (int)h->kmg_host.size();
  nd.tvg_bytes = (int)(tvg.size() * sizeof(double)); nd.n_ext = g.n_ext;
  next.tvg.swap(tvg); next.kmg.swap(kmg); next.def.swap(def);      // (the caller commits them with nd once nothing can fail any more)
  return 0;
}
extern "C" {

int finrom_rom_set_mirror(finrom_rom_t h, const finrom_rom_desc* a, const int32_t* row_node, const double* row_weight,
                          const int32_t* theta_twin) {
  if (!h || !a) { set_error("rom_set_mirror: null argument"); return FINROM_ERR_ARG; }
  RomDev& d = h->d;
  if (int rc = validate_rom_mirror(a, d.n, row_node, row_weight, theta_twin)) return rc;
  if (a->r != d.r || a->P != d.P) { set_error("rom_set_mirror: basis size / parameter count differ from the handle's"); return FINROM_ERR_ARG; }
  if (d.nkg_m > 0) { set_error("rom_set_mirror: already installed"); return FINROM_ERR_ARG; }
  // the one-wave grouped kernel is the only form that walks the half list
  if (d.NB > 5 || d.nkg == 0) { set_error("rom_set_mirror: the handle has no grouped form (r > 80, FINROM_PROJ_UNGROUPED, nothing to group)"); return FINROM_ERR_UNSUPPORTED; }
  GroupedTables g;
  int kmg0 = 0;
  RomDev nd = d;
  HostTables next;
  if (int rc = append_half_list(h, a, row_weight, nd, g, kmg0, next, "rom_set_mirror")) return rc;
  if (int rc = up(h->owned, &nd.twin, theta_twin, (size_t)d.P)) return rc;      // (the handle keeps its tables; what was uploaded is freed with it)
  nd.kmg_m = kmg0; nd.nkg_m = g.nkg; nd.ext_final_m = g.ext_final;
  d = nd;
  h->tvg_host.swap(next.tvg); h->kmg_host.swap(next.kmg); h->def_host.swap(next.def);
  h->mirror_n = a->n;
  h->mirror_counts[0][0] = (int)rows_by_term_count(a).size(); h->mirror_counts[0][1] = g.live; h->mirror_counts[0][2] = g.fma_ksteps;
  return 0;
}

int finrom_rom_set_mirror_short(finrom_rom_t h, const finrom_rom_desc* a, const double* row_weight, double theta_lo, double theta_hi) {
  if (!h || !a || !row_weight) { set_error("rom_set_mirror_short: null argument"); return FINROM_ERR_ARG; }
  RomDev& d = h->d;
  if (d.nkg_m == 0) { set_error("rom_set_mirror_short: finrom_rom_set_mirror comes first"); return FINROM_ERR_ARG; }
  if (d.nkg_s > 0) { set_error("rom_set_mirror_short: already installed"); return FINROM_ERR_ARG; }
  if (int rc = validate_rom_desc(a)) return rc;
  if (a->r != d.r || a->P != d.P || a->n != h->mirror_n) { set_error("rom_set_mirror_short: sizes differ from the half descriptor's"); return FINROM_ERR_ARG; }
  if (!(theta_lo > 0.0 && theta_lo <= theta_hi)) { set_error("rom_set_mirror_short: need 0 < theta_lo <= theta_hi"); return FINROM_ERR_ARG; }
  if (int rc = validate_row_weights(a, row_weight)) return rc;
  GroupedTables g;
  int kmg0 = 0;
  RomDev nd = d;
  HostTables next;
  if (int rc = append_half_list(h, a, row_weight, nd, g, kmg0, next, "rom_set_mirror_short")) return rc;
  nd.kmg_s = kmg0; nd.nkg_s = g.nkg; nd.ext_final_s = g.ext_final; nd.short_lo = theta_lo; nd.short_hi = theta_hi;
  d = nd;
  h->tvg_host.swap(next.tvg); h->kmg_host.swap(next.kmg); h->def_host.swap(next.def);
  h->mirror_counts[1][0] = (int)rows_by_term_count(a).size(); h->mirror_counts[1][1] = g.live; h->mirror_counts[1][2] = g.fma_ksteps;
  return 0;
}

int finrom_rom_mirror_info(finrom_rom_t h, int32_t which, int32_t* live_rows, int32_t* ksteps, int32_t* fma_ksteps) {
  if (!h || !live_rows || !ksteps || !fma_ksteps || which < 0 || which > 1) { set_error("rom_mirror_info: bad argument"); return FINROM_ERR_ARG; }
  *live_rows = h->mirror_counts[which][0]; *ksteps = h->mirror_counts[which][1]; *fma_ksteps = h->mirror_counts[which][2];      // (zeros: not installed)
  return 0;
}

int finrom_rom_last_form(finrom_rom_t h) {
  if (!h) { set_error("rom_last_form: null handle"); return FINROM_ERR_ARG; }
  return h->last_form;
}

int finrom_rom_last_epilogue(finrom_rom_t h) {
  if (!h) { set_error("rom_last_epilogue: null handle"); return FINROM_ERR_ARG; }
  return h->last_epilogue;
}

void finrom_rom_destroy(finrom_rom_t h) {
  if (!h) return;
  for (void* p : h->owned) dev_free(p);
  h->Ar.release(); h->Br.release(); h->theta.release(); h->qtmp.release(); h->vw.release(); h->grad_ticket.release();
  h->part.release(); h->ext.release();
  if (h->side) defer_or_run([](void* s) { (void)hipStreamDestroy((hipStream_t)s); }, h->side);
  if (h->fom_side) defer_or_run([](void* s) { (void)hipStreamDestroy((hipStream_t)s); }, h->fom_side);
  if (h->ev_join_fom) defer_or_run([](void* e) { (void)hipEventDestroy((hipEvent_t)e); }, h->ev_join_fom);
  if (h->ev_fork) defer_or_run([](void* e) { (void)hipEventDestroy((hipEvent_t)e); }, h->ev_fork);
  if (h->ev_join) defer_or_run([](void* e) { (void)hipEventDestroy((hipEvent_t)e); }, h->ev_join);
  delete h;
}

int finrom_rom_set_gram(finrom_rom_t h, int32_t npairs, const int32_t* pair_p, const int32_t* pair_q, const double* G) {
  if (!h || npairs <= 0 || !pair_p || !pair_q || !G) { set_error("rom_set_gram: bad argument"); return FINROM_ERR_ARG; }
  if (npairs > ROM_GRAM_MAX_PAIRS) { set_error("rom_set_gram: more than 64 pairs"); return FINROM_ERR_UNSUPPORTED; }
  const RomDev& d = h->d;
  const int r = d.r, R = d.rp, NB = d.NB;
  for (int t = 0; t < npairs; ++t)
    if (pair_p[t] < 0 || pair_q[t] > d.P || pair_p[t] > pair_q[t]) { set_error("rom_set_gram: invalid pair (need 0 <= p <= q <= P)"); return FINROM_ERR_ARG; }
  for (int t = 0; t < npairs; ++t)
    for (int u = 0; u < t; ++u)
      if (pair_p[t] == pair_p[u] && pair_q[t] == pair_q[u]) { set_error("rom_set_gram: duplicate pair"); return FINROM_ERR_ARG; }
  auto at = [&](int t, int i, int j) { return (i < r && j < r) ? G[((size_t)t * r + i) * r + j] : 0.0; };
  for (int t = 0; t < npairs; ++t)
    for (int i = 0; i < r; ++i)
      for (int j = 0; j < i; ++j) {
        const double x = at(t, i, j), y = at(t, j, i);
        if (!(std::fabs(x - y) <= 1e-12 * (std::fabs(x) + std::fabs(y)) + 1e-300)) { set_error("rom_set_gram: block is not symmetric"); return FINROM_ERR_ARG; }
      }
  int rc = 0;
  RomGramDev gm = h->gram;
  if (!rc) rc = up(h->owned, &gm.pair_p, pair_p, npairs);
  if (!rc) rc = up(h->owned, &gm.pair_q, pair_q, npairs);
  if (NB <= 6) {       // tile images: lane (q, c), register g of tile (ti <= tj) holds entry (16 ti + q + 4 g, 16 tj + c)
    const int NT = NB * (NB + 1) / 2;
    std::vector<double> Gt((size_t)npairs * NT * 256, 0.0);
    for (int t = 0; t < npairs; ++t) {
      int tile = 0;
      for (int ti = 0; ti < NB; ++ti)
        for (int tj = ti; tj < NB; ++tj, ++tile)
          for (int lane = 0; lane < 64; ++lane)
            for (int g = 0; g < 4; ++g)
              Gt[(((size_t)t * NT + tile) * 64 + lane) * 4 + g] = at(t, 16 * ti + (lane >> 4) + 4 * g, 16 * tj + (lane & 15));
    }
    if (!rc) rc = up(h->owned, &gm.Gt, Gt.data(), Gt.size());
  } else {             // packed upper triangle, row by row (= the lower triangle by columns the Cholesky kernels read)
    const size_t np = (size_t)R * (R + 1) / 2;
    std::vector<double> Gp((size_t)npairs * np, 0.0);
    for (int t = 0; t < npairs; ++t)
      for (int row = 0; row < r; ++row)
        for (int col = row; col < r; ++col) Gp[t * np + (size_t)row * R - ((size_t)row * (row - 1)) / 2 + col - row] = at(t, row, col);
    if (!rc) rc = up(h->owned, &gm.Gp, Gp.data(), Gp.size());
  }
  if (rc) return rc;
  gm.npairs = npairs;
  h->gram = gm;
  return 0;
}

int finrom_rom_set_projection(finrom_rom_t h, int32_t mode) {
  if (!h || (mode != FINROM_PROJECTION_DIRECT && mode != FINROM_PROJECTION_GRAM)) { set_error("rom_set_projection: bad argument"); return FINROM_ERR_ARG; }
  if (mode == FINROM_PROJECTION_GRAM && h->gram.npairs == 0) { set_error("rom_set_projection: finrom_rom_set_gram has not been called"); return FINROM_ERR_ARG; }
  h->projection = mode;
  return 0;
}

}  // extern "C"
// A_r, B_r (or, with factor > 0, the factor / the solution) by the form of the reduced operator the handle is set to
// (mirror: the call may offer the half list of finrom_rom_set_mirror to its samples -- finrom_rom_solve only)
static int rom_project(finrom_rom_t h, const double* theta, int64_t S, int factor, int* info, hipStream_t st,
                       double* w_r = nullptr, double* qoi_r = nullptr, bool mirror = false, bool roomy = false, bool short_waits = false) {
  h->last_form = FINROM_ROM_FORM_FULL;
  roomy = roomy && h->projection == FINROM_PROJECTION_DIRECT && rom_roomy_applies(h->d, factor, w_r, qoi_r);
  short_waits = roomy && short_waits;
  h->last_epilogue = !roomy ? FINROM_ROM_EPILOGUE_STANDARD : short_waits ? FINROM_ROM_EPILOGUE_ROOMY_SHORT_WAITS : FINROM_ROM_EPILOGUE_ROOMY;
  if (h->projection == FINROM_PROJECTION_GRAM)
    return launch_rom_gram(h->d, h->gram, theta, S, (double*)h->Ar.p, (double*)h->Br.p, factor, info, st, w_r, qoi_r);
  RomDev d = h->d;
  d.ext = nullptr;
  if (!mirror) d.nkg_m = d.nkg_s = 0;
  if (d.nkg > 0 && S > 0 && (roomy || !rom_splitk_applies(d, S))) {      // the grouped main loop: room for the samples' scalars
    if (int rc = h->ext.reserve((size_t)S * d.n_ext * sizeof(double))) return rc;
    d.ext = (double*)h->ext.p;
    if (d.nkg_m > 0) h->last_form = FINROM_ROM_FORM_HALF;
  }
  return launch_rom_proj(d, theta, S, (double*)h->Ar.p, (double*)h->Br.p, factor, info, st, w_r, qoi_r, roomy, short_waits);
}

// roomy: finrom_solve_pairs beside the FOM's half sweep -- QoI-only calls at r <= 80 then take the 256-register one-wave kernel at
// every batch size (rom_roomy_applies); finrom_rom_solve itself never does.  short_waits: that kernel's form without the fixed waits
// between accumulate-chained MFMAs (finrom_rom_s::short_waits says where)
static int rom_solve_impl(finrom_rom_t h, const double* theta, int64_t S, double* w_r, double* qoi_r, double* A_r,
                          double* B_r, int32_t* info, void* stream, bool roomy, bool short_waits = false) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!theta || (!qoi_r && h->d.n_obs > 0)))) { set_error("rom_solve: bad argument"); return FINROM_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const RomDev& d = h->d;
  const size_t per_sample = ((size_t)d.rp * (d.rp + 1) / 2 + d.rp) * sizeof(double);
  int64_t chunk = std::max<int64_t>(4, (int64_t)(((size_t)16 << 30) / per_sample) / 4 * 4);
  if (S > chunk) { const int64_t np = (S + chunk - 1) / chunk; chunk = ((S + np - 1) / np + 3) / 4 * 4; }      // equal pieces
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t Sc = std::min(chunk, S - s0);
    int rc;
    // one-sample call patterns (MAP / HMC: a handful of samples, latency): contraction over several workgroups per sample, then
    // the MFMA-form factorisation + substitutions (rom_onesample.hip)
    const bool rm = roomy && A_r == nullptr && B_r == nullptr && h->projection == FINROM_PROJECTION_DIRECT && rom_roomy_applies(d, 2, w_r, qoi_r);
    if (!rm && A_r == nullptr && B_r == nullptr && h->projection == FINROM_PROJECTION_DIRECT && rom_onesample_applies(d, Sc)) {
      h->last_epilogue = FINROM_ROM_EPILOGUE_STANDARD;
      if ((rc = h->part.reserve(rom_onesample_scratch_bytes(d, Sc)))) return rc;
      h->last_form = FINROM_ROM_FORM_FULL;
      if ((rc = launch_rom_onesample(d, theta + s0 * d.P, Sc, (double*)h->part.p, 0, RomGradArgs(), w_r ? w_r + s0 * d.r : nullptr,
                                     qoi_r ? qoi_r + s0 * d.n_obs : nullptr, info ? info + s0 : nullptr, st))) return rc;
      continue;
    }
    if ((rc = h->Ar.reserve((size_t)Sc * (d.rp * (d.rp + 1) / 2) * sizeof(double)))) return rc;
    if ((rc = h->Br.reserve((size_t)Sc * d.rp * sizeof(double)))) return rc;
    // A_r is factored inside the projection kernel (in registers, MFMA trailing updates) unless the caller
    // wants A_r itself back (the state the reference's gradients use) or the basis needs more than one wave
    const bool want_factor = A_r == nullptr;
    int factor = (want_factor && d.NB <= 6) ? 1 : 0;                  // in-register, inside the projection kernel
    // ... and when neither A_r nor B_r is wanted back (r <= 80), the two substitutions and the reduced QoI happen there
    // as well: no packed factor in memory, no second kernel
    if (factor && (d.NB <= 5 || (d.NB == 6 && h->projection == FINROM_PROJECTION_DIRECT && rom_splitk_applies(d, Sc))) && A_r == nullptr && B_r == nullptr)
      factor = 2;
    // wider bases, only the reduced QoI wanted (the sample-pair path): factorisation and QoI stay in the registers of the
    // projection kernel's waves (fused_solve_mw); A_r never reaches memory
    if (d.NB > 6 && want_factor && h->projection == FINROM_PROJECTION_DIRECT && A_r == nullptr && B_r == nullptr && w_r == nullptr &&
        qoi_r != nullptr && d.n_obs + 1 <= 16 * 3) factor = 3;
    if ((rc = rom_project(h, theta + s0 * d.P, Sc, factor, info ? info + s0 : nullptr, st,
                          w_r ? w_r + s0 * d.r : nullptr, qoi_r ? qoi_r + s0 * d.n_obs : nullptr, true, rm, short_waits))) return rc;
    if (factor >= 2) continue;
    int factored = factor;
    if (want_factor && d.NB > 6) {                                     // wider bases: blocked MFMA Cholesky kernel
      if ((rc = launch_rom_chol_blocked(d, (double*)h->Ar.p, Sc, info ? info + s0 : nullptr, st))) return rc;
      factored = 1;
    }
    if ((rc = launch_rom_solve(d, (const double*)h->Ar.p, (const double*)h->Br.p, Sc, w_r ? w_r + s0 * d.r : nullptr,
                               qoi_r ? qoi_r + s0 * d.n_obs : nullptr, A_r ? A_r + s0 * (int64_t)d.r * d.r : nullptr,
                               B_r ? B_r + s0 * d.r : nullptr, info ? info + s0 : nullptr, factored, st))) return rc;
  }
  return 0;
}
extern "C" {

int finrom_rom_solve(finrom_rom_t h, const double* theta, int64_t S, double* w_r, double* qoi_r, double* A_r,
                     double* B_r, int32_t* info, void* stream) {
  return rom_solve_impl(h, theta, S, w_r, qoi_r, A_r, B_r, info, stream, false);
}

int finrom_rom_set_gradient(finrom_rom_t h, int32_t npairs, const int32_t* pair_p, const int32_t* pair_i, const double* G) {
  if (!h || npairs < 0 || (npairs > 0 && (!pair_p || !pair_i || !G))) { set_error("rom_set_gradient: bad argument"); return FINROM_ERR_ARG; }
  for (int t = 0; t < npairs; ++t)
    if (pair_p[t] < 0 || pair_p[t] > h->d.P || pair_i[t] < 0 || pair_i[t] >= h->d.P) { set_error("rom_set_gradient: invalid pair"); return FINROM_ERR_ARG; }
  int rc = 0;
  if (!rc) rc = up(h->owned, &h->g_pair_p, pair_p, npairs);
  if (!rc) rc = up(h->owned, &h->g_pair_i, pair_i, npairs);
  if (!rc) rc = up(h->owned, &h->g_Gt, G, (size_t)npairs * h->d.r * h->d.r);
  if (rc) return rc;
  h->g_npairs = npairs;
  return 0;
}

int finrom_rom_grad(finrom_rom_t h, const double* theta, const double* data, int32_t data_per_sample, int64_t S,
                    double* J, double* g, double* w_r, double* qoi_r, int32_t* info, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!theta || !data || !J || !g))) { set_error("rom_grad: bad argument"); return FINROM_ERR_ARG; }
  if (h->g_npairs == 0) { set_error("rom_grad: finrom_rom_set_gradient has not been called"); return FINROM_ERR_ARG; }
  const RomDev& d = h->d;
  hipStream_t st = (hipStream_t)stream;
  const size_t per_sample = ((size_t)d.rp * (d.rp + 1) / 2 + d.rp) * sizeof(double);
  int64_t chunk = std::max<int64_t>(4, (int64_t)(((size_t)16 << 30) / per_sample) / 4 * 4);
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t Sc = std::min(chunk, S - s0);
    int rc;
    if ((rc = h->Ar.reserve((size_t)Sc * (d.rp * (d.rp + 1) / 2) * sizeof(double)))) return rc;
    if ((rc = h->Br.reserve((size_t)Sc * d.rp * sizeof(double)))) return rc;
    double* q = qoi_r ? qoi_r + s0 * d.n_obs : nullptr;
    if (!q) { if ((rc = h->qtmp.reserve((size_t)Sc * d.n_obs * sizeof(double)))) return rc; q = (double*)h->qtmp.p; }
    // one-sample call patterns (MAP / HMC), 48 < r <= 96, the per-sample contraction: projection split over four waves, both
    // solves in registers, the gradient contraction dealt over the same waves -- one kernel, nothing but the outputs written
    if (h->projection == FINROM_PROJECTION_DIRECT && rom_onesample_applies(d, Sc)) {
      // contraction over several workgroups per sample, MFMA-form factorisation + forward / adjoint solves (rom_onesample.hip),
      // then the gradient contraction dealt over 36 workgroups per sample
      RomGradArgs ga;
      ga.data = data + (data_per_sample ? s0 * d.n_obs : 0); ga.data_stride = data_per_sample ? d.n_obs : 0;
      ga.theta = theta + s0 * d.P; ga.J = J + s0; ga.g = g + s0 * d.P;
      ga.npairs = h->g_npairs; ga.pair_p = h->g_pair_p; ga.pair_i = h->g_pair_i; ga.Gt = h->g_Gt;
      const size_t vw_bytes = (size_t)Sc * 2 * d.rp * sizeof(double), gp_bytes = (size_t)Sc * ROM_GRAD_SMALL_NG * 32 * sizeof(double);
      if ((rc = h->vw.reserve(vw_bytes + gp_bytes))) return rc;
      if ((rc = h->part.reserve(rom_onesample_scratch_bytes(d, Sc)))) return rc;
      if (!h->grad_ticket.p) {                          // arrival counters: zero once, the kernel leaves them zero
        if ((rc = h->grad_ticket.reserve(ROM_SPLITK_MAX_S * sizeof(int)))) return rc;
        FR_HIP(hipMemset(h->grad_ticket.p, 0, ROM_SPLITK_MAX_S * sizeof(int)));
      }
      ga.vw = (double*)h->vw.p; ga.gpart = (double*)((char*)h->vw.p + vw_bytes); ga.ticket = (int*)h->grad_ticket.p;
      ga.defer_sum = h->defer_gsum && s0 == 0 && Sc == S;
      ga.info_store = ga.defer_sum && h->info_store;
      h->last_gpart = ga.defer_sum ? ga.gpart : nullptr;
      if ((rc = launch_rom_onesample(d, theta + s0 * d.P, Sc, (double*)h->part.p, 1, ga, w_r ? w_r + s0 * d.r : nullptr, q,
                                     info ? info + s0 : nullptr, st, ga.defer_sum ? h->fuse : nullptr))) return rc;
      if ((rc = launch_rom_grad_contract_small(d, Sc, ga, st, ga.defer_sum ? h->back : nullptr))) return rc;
      continue;
    }
    if (h->projection == FINROM_PROJECTION_DIRECT && rom_splitk_applies(d, Sc) && d.n_obs <= 64) {
      RomGradArgs ga;
      ga.data = data + (data_per_sample ? s0 * d.n_obs : 0); ga.data_stride = data_per_sample ? d.n_obs : 0;
      ga.theta = theta + s0 * d.P; ga.J = J + s0; ga.g = g + s0 * d.P;
      ga.npairs = h->g_npairs; ga.pair_p = h->g_pair_p; ga.pair_i = h->g_pair_i; ga.Gt = h->g_Gt;
      const size_t vw_bytes = (size_t)Sc * 2 * d.rp * sizeof(double), gp_bytes = (size_t)Sc * ROM_GRAD_SMALL_NG * 32 * sizeof(double);
      if ((rc = h->vw.reserve(vw_bytes + gp_bytes))) return rc;
      if (!h->grad_ticket.p) {                          // arrival counters: zero once, the kernel leaves them zero
        if ((rc = h->grad_ticket.reserve(ROM_SPLITK_MAX_S * sizeof(int)))) return rc;
        FR_HIP(hipMemset(h->grad_ticket.p, 0, ROM_SPLITK_MAX_S * sizeof(int)));      // synchronous: ordered before ANY stream's first use
      }
      ga.vw = (double*)h->vw.p; ga.gpart = (double*)((char*)h->vw.p + vw_bytes); ga.ticket = (int*)h->grad_ticket.p;
      {
        ScopedKernelTimer t(K_ROM_PROJ, st);
        if ((rc = launch_rom_proj_splitk(d, theta + s0 * d.P, Sc, (double*)h->Ar.p, (double*)h->Br.p, 4, info ? info + s0 : nullptr, st,
                                         w_r ? w_r + s0 * d.r : nullptr, q, ga))) return rc;
      }
      if ((rc = launch_rom_grad_contract_small(d, Sc, ga, st))) return rc;
      continue;
    }
    // the factor of A_r: inside the projection kernel for r <= 96, by the blocked MFMA Cholesky kernel for wider bases
    if ((rc = rom_project(h, theta + s0 * d.P, Sc, d.NB <= 6 ? 1 : 0, info ? info + s0 : nullptr, st))) return rc;
    if (d.NB > 6 && (rc = launch_rom_chol_blocked(d, (double*)h->Ar.p, Sc, info ? info + s0 : nullptr, st))) return rc;
    RomGradArgs ga;
    ga.data = data + (data_per_sample ? s0 * d.n_obs : 0); ga.data_stride = data_per_sample ? d.n_obs : 0;
    ga.theta = theta + s0 * d.P; ga.J = J + s0; ga.g = g + s0 * d.P;
    ga.npairs = h->g_npairs; ga.pair_p = h->g_pair_p; ga.pair_i = h->g_pair_i; ga.Gt = h->g_Gt;
    // batches: the contraction with the blocks G_pi runs on the matrix cores for 16 samples at a time; a handful of samples
    // (the one-sample call pattern) keep it inside the substitution kernel (one launch less)
    const bool batched = Sc >= 64 && d.n_obs <= 64;
    if (batched) {
      if ((rc = h->vw.reserve((size_t)Sc * 2 * d.rp * sizeof(double)))) return rc;
      ga.vw = (double*)h->vw.p;
    }
    if ((rc = launch_rom_grad(d, (const double*)h->Ar.p, (const double*)h->Br.p, Sc, w_r ? w_r + s0 * d.r : nullptr, q,
                              info ? info + s0 : nullptr, ga, st))) return rc;
    if (batched && (rc = launch_rom_grad_contract(d, Sc, ga, st))) return rc;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------
int finrom_subfin_avg(const double* Sop, int32_t P, int32_t n, const double* k, int64_t S, double* theta, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!Sop || P <= 0 || n <= 0 || S < 0 || (S > 0 && (!k || !theta))) { set_error("subfin_avg: bad argument"); return FINROM_ERR_ARG; }
  return launch_subfin_avg(Sop, P, n, k, S, theta, (hipStream_t)stream);
}

}  // extern "C"
// FINROM_TRACE=<prefix>: every finrom_solve_pairs call records, per workgroup of the FOM interpreter and of the
// projection kernel, {start, end, HW_ID, XCC_ID} and rewrites <prefix>.fom.bin / <prefix>.proj.bin (int64 x 6 per
// workgroup) after a device synchronisation.  Diagnostic for the co-residency of the two halves.
static long long* g_trace_buf[2] = {nullptr, nullptr};
static constexpr size_t kTraceWg = 1u << 18;
static const char* trace_prefix() { static const char* p = getenv("FINROM_TRACE"); return p; }
static int trace_dump(const char* kind, long long* dbuf, size_t nwg) {
  std::vector<long long> h(nwg * 6);
  FR_HIP(hipDeviceSynchronize());
  FR_HIP(hipMemcpy(h.data(), dbuf, nwg * 6 * sizeof(long long), hipMemcpyDeviceToHost));
  const std::string path = std::string(trace_prefix()) + "." + kind + ".bin";
  if (FILE* f = fopen(path.c_str(), "wb")) { fwrite(h.data(), sizeof(long long), h.size(), f); fclose(f); }
  return 0;
}
extern "C" {

int finrom_solve_pairs(finrom_fom_t fom, finrom_rom_t rom, const double* Sop, const double* x, int64_t S,
                       double* qoi, double* qoi_r, double* err, double* w, double* w_r, double* theta,
                       int32_t* info, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!fom || !rom || !Sop || S < 0 || (S > 0 && (!x || !qoi || !qoi_r))) { set_error("solve_pairs: bad argument"); return FINROM_ERR_ARG; }
  if (fom->d.n_obs != rom->d.n_obs) { set_error("solve_pairs: FOM and ROM observation operators differ in size"); return FINROM_ERR_ARG; }
  if (S == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if ((rc = rom->ensure_side())) return rc;
  if (!theta) {
    if ((rc = rom->theta.reserve((size_t)S * rom->d.P * sizeof(double)))) return rc;
    theta = (double*)rom->theta.p;
  }
  // The two halves run on two streams (FINROM_NO_OVERLAP / finrom_set_overlap(0): in turn, for per-kernel profiling).  With the
  // band sweep as the FOM half (HBM-bound, one 300-register wave per SIMD, vector units 80 % idle) a projection wave fits beside
  // every sweep wave, and since the projection hides its non-MFMA work behind its own MFMAs a lone wave per SIMD is efficient:
  // measured 26.3 ms side by side against 29.1 ms in turn per 100k samples (r = 80).
  static const bool env_no_overlap = getenv("FINROM_NO_OVERLAP") != nullptr;      // (read once, not per call)
  // (The four-wave band sweep of m = 16, 20 takes a whole CU's LDS -- 157 KB per workgroup -- and the wide-basis projection 43 KB
  // per workgroup: the two kernels cannot share a CU, side by side they take turns CU by CU at the dispatcher's discretion.  That
  // still beats running them in turn by 1-5 % (r = 200: 68.6 against 72.0 ms per 20k samples, 420 against 425 ms per 125k), so
  // those sizes fork too; their event-timed kernel durations then include waiting for CUs -- FINROM_NO_OVERLAP=1 gives clean ones.)
  const bool overlap = overlap_enabled() && !env_no_overlap;
  hipStream_t side = overlap ? rom->side : st;
  const bool tracing = trace_prefix() != nullptr;
  if (tracing) {
    for (int i = 0; i < 2; ++i)
      if (!g_trace_buf[i]) FR_HIP(hipMalloc((void**)&g_trace_buf[i], kTraceWg * 6 * sizeof(long long)));
    FR_HIP(hipMemset(g_trace_buf[0], 0, kTraceWg * 6 * sizeof(long long)));
    FR_HIP(hipMemset(g_trace_buf[1], 0, kTraceWg * 6 * sizeof(long long)));
    FR_HIP(hipDeviceSynchronize());
    fom->d.trace = (size_t)((S + 63) / 64) <= kTraceWg ? g_trace_buf[0] : nullptr;
    rom->d.trace = (size_t)S <= kTraceWg ? g_trace_buf[1] : nullptr;
  }
  // (the fork below: everything already queued on the caller's stream -- inputs, zeroed info -- precedes both halves)
  // ROM half first, on a high-priority stream: its 4-wave, 160-VGPR workgroups need large contiguous
  // register ranges, so they claim their slots before the small FOM waves fill the remaining ones
  // The FOM's short bandwidth-bound pre-pass (pack + assembly) used to run first, alone: beside the projection kernel it crawls and
  // the interpreter of round 1, whose waves then started late, WAS the critical path.  Since the band sweep the FOM half ends
  // long before the ROM half (6.8 against 21.8 ms side by side at the headline), so the pre-pass now runs after the fork, on the
  // FOM side, and only the sub-fin averages -- the head of the ROM half -- precede it.
  // Every workspace the two halves need is reserved BEFORE the fork: an allocation failure after it would return while the
  // side stream still writes the caller's outputs.  Any other failure after the fork joins the side stream first.
  const BandDev& fband = fom->band_for(w != nullptr);
  const bool split = S <= fom_chunk_samples(fom->d, &fband);
  // Round 4: beside the ONE-WAVE projection kernel (r <= 80, two 200-register waves per SIMD) the register band sweep (m <= 12, one
  // 312-register wave per SIMD) runs on a stream masked to THREE CUs of every shader engine (96 of 256): what the projection loses is
  // proportional to the CU-time it shares with sweep waves, and confined to fewer CUs the sweep's waves -- fewer at a time, less
  // contention for HBM -- need less of it in total (256 CUs x 6.9 ms -> 96 x 15.3 ms; the sweep still ends long before the projection).
  // Measured, headline: step 21.54 -> 20.92 ms; two CUs per engine make the sweep the longer half (22.4), four give 21.06.  NOT for the
  // multi-wave projection kernels (r = 120: 49.7 -> 56.7 ms, their workgroups leave the confined sweep too few slots), the four-wave
  // sweep (LDS-exclusive: no change) or the offline/online form (FOM-bound: 9.1 -> 14.3).  FINROM_FOM_CUS=<n> forces n CUs (0: off).
  static const int env_fom_cus = getenv("FINROM_FOM_CUS") != nullptr ? atoi(getenv("FINROM_FOM_CUS")) : -1;
  const bool no_band = env_no_band();
  int fom_cus = env_fom_cus;
  // The half plan of a mirror-symmetric operator (finrom_fom_set_band_mirror: a 154-register wave, 60 KB per sample, 1.3 ms alone)
  // is confined to ONE CU of every shader engine: it then lives 6.1 ms on 32 CUs instead of 3.1 ms on 96, still a third of the
  // projection's time, and the projection loses least.  Headline, step in ms: unmasked 19.48, one CU per engine 19.06, two 19.20,
  // three 19.32 (the full plan with three: 20.11-20.15).
  const bool half_plan = &fband == &fom->band_m;
  if (fom_cus < 0)
    fom_cus = (rom->projection == FINROM_PROJECTION_DIRECT && rom->d.NB <= 5 && fom->band.on && fom->band.NSP <= 14 && !no_band &&
               w == nullptr && S >= 16384) ? (half_plan ? -1 : -3) : 0;
  hipStream_t fst = st;
  if (overlap && fom_cus != 0) {
    if ((rc = rom->ensure_fom_side(fom_cus))) return rc;
    if (rom->fom_side) fst = rom->fom_side;
  }
  // With the sweep on its masked stream and its pre-pass off it (below), the ROM half can stay on the CALLER's stream: sub-fin
  // averages, per-sample scalars, projection and the difference kernel then follow each other in stream order, and the library's
  // unmasked side stream carries the pre-pass instead -- no cross-stream wait on the step's critical path (each costs 40-80 us:
  // between two steps of the headline the GPU waited 0.33 ms).  FINROM_ROM_ON_SIDE=1: the ROM half on the side stream, as for
  // every other caller's stream.
  static const bool env_rom_on_side = getenv("FINROM_ROM_ON_SIDE") != nullptr;
  static const bool env_pre_masked = getenv("FINROM_FOM_PREPASS_MASKED") != nullptr;
  const bool pre_unmasked = fst != st && split && !env_pre_masked;
  // Only when the caller's stream is a non-blocking one: hipExtStreamCreateWithCUMask has no flags argument, the masked stream is a
  // BLOCKING stream, and the null stream (torch's default) serialises with it -- measured: the sweep then starts when the
  // projection ends (29.0 instead of 20.2 ms per step).
  unsigned st_flags = 0;
  const bool st_nonblocking = st != nullptr && hipStreamGetFlags(st, &st_flags) == hipSuccess && (st_flags & hipStreamNonBlocking);
  const bool rom_on_caller = pre_unmasked && !env_rom_on_side && st_nonblocking;
  const hipStream_t rst = rom_on_caller ? st : side;      // the ROM half
  const hipStream_t pst = rom_on_caller ? side : st;      // the FOM half's unmasked pre-pass
  auto join = [&]() {
    if (overlap && !rom_on_caller && hipEventRecord(rom->ev_join, side) == hipSuccess) (void)hipStreamWaitEvent(st, rom->ev_join, 0);
    if (fst != st && hipEventRecord(rom->ev_join_fom, fst) == hipSuccess) (void)hipStreamWaitEvent(st, rom->ev_join_fom, 0);      // (the sweep waited for the pre-pass)
  };
  auto fail = [&](int code) { if (overlap) (void)hipStreamSynchronize(side); if (fst != st) (void)hipStreamSynchronize(fst); return code; };
  if (split && (rc = fom_solve_stages(fom, x, S, qoi, w, info, st, 4))) return rc;          // (reserves the FOM workspace)
  // the sub-fin averages (bandwidth-bound, short) run BEFORE the fork, alone: beside the sweep they were starved (0.19 -> 0.39 ms
  // at the headline, 0.6 -> 5.8 ms at m = 20) and they head the ROM half's critical path
  if ((rc = launch_subfin_avg(Sop, rom->d.P, fom->d.xdim, x, S, theta, st))) return fail(rc);
  if (overlap) {                          // the ROM half starts after the averages
    FR_HIP(hipEventRecord(rom->ev_fork, st));
    FR_HIP(hipStreamWaitEvent(side, rom->ev_fork, 0));
    if (fst != st) FR_HIP(hipStreamWaitEvent(fst, rom->ev_fork, 0));
  }
  // Beside the HALF sweep (154 registers, 11.8 KB of LDS per wave) a QoI-only projection at r <= 80 takes the roomy one-wave kernel:
  // 256 + 154 registers still share a SIMD.  Whether the roomy kernel runs depends on the two handles and on what the caller wants
  // back, never on batch size, stream or mask.  FINROM_PROJ_NO_ROOMY=1 at handle creation: the 200-register kernel, as everywhere else.
  // WHICH of its two forms runs does depend on the mask: the epilogue drops the fixed waits between accumulate-chained MFMAs (same
  // bits) only beside a sweep on its masked stream, for the reason the pivot records below have: a batch too small for
  // the mask is bounded from BELOW by the benchmark's contract (0.662 ms at 4096 samples; with the short waits the step measured
  // 0.660 and 0.678 ms there, with the fixed ones 0.69).
  if ((rc = rom_solve_impl(rom, theta, S, w_r, qoi_r, nullptr, nullptr, info, rst, half_plan && !rom->no_roomy, rom->short_waits(fst != st))))
    return fail(rc);
  // With a masked FOM stream only the SWEEP runs on it: pack + assembly go to an unmasked stream (they take 0.1 ms there against
  // 2.0 ms on 96 CUs beside the projection's start, and since the grouped projection loop the FOM half is the one that ends
  // last: step 20.46 -> 20.26 ms).  FINROM_FOM_PREPASS_MASKED=1: the whole FOM half on the masked stream, as before.
  // Pivot records (DESIGN 4c') are for the sweep CONFINED to its masked stream: there every millisecond it lives shorter returns
  // CU-time to the projection.  A batch too small for the mask keeps the table-reading kernel on this path: its step is a chain of
  // launch latencies, which the benchmark's contract bounds from BELOW by the reference's flop count over the matrix peak
  // (tests/test_gpu_bench_contract.py: 0.662 ms at 4096 samples; on records the step is 0.62 ms, on tables 0.71).  Same bits either way.
  const bool records = fst != st;
  if (pre_unmasked) {
    if ((rc = fom_solve_stages(fom, x, S, qoi, w, info, pst, 1))) return fail(rc);
    if (hipEventRecord(rom->ev_join_fom, pst) != hipSuccess || hipStreamWaitEvent(fst, rom->ev_join_fom, 0) != hipSuccess) return fail(FINROM_ERR_HIP);
    if ((rc = fom_solve_stages(fom, x, S, qoi, w, info, fst, 2, records))) return fail(rc);
  } else if ((rc = fom_solve_stages(fom, x, S, qoi, w, info, fst, 3, records))) return fail(rc);
  join();
  // a roomy call returns a sample that either half flagged as NaN in qoi_r and err (launch_sub_flagged); every other call keeps
  // what its kernels wrote
  if ((rom->last_epilogue == FINROM_ROM_EPILOGUE_ROOMY || rom->last_epilogue == FINROM_ROM_EPILOGUE_ROOMY_SHORT_WAITS) && info != nullptr) {
    if ((rc = launch_sub_flagged(qoi, qoi_r, info, fom->d.n_obs, S * (int64_t)fom->d.n_obs, err, st))) return rc;
  } else if (err && (rc = launch_sub(qoi, qoi_r, S * (int64_t)fom->d.n_obs, err, st))) return rc;
  if (tracing) {
    if (fom->d.trace) trace_dump("fom", g_trace_buf[0], (size_t)((S + 63) / 64));
    if (rom->d.trace) trace_dump("proj", g_trace_buf[1], (size_t)S);
    fom->d.trace = nullptr; rom->d.trace = nullptr;
  }
  return 0;
}

}  // extern "C"

extern "C" {

int finrom_sampler_create(const double* U, int32_t n, finrom_sampler_t* out) {
  if (!U || n <= 0 || !out) { set_error("sampler_create: bad argument"); return FINROM_ERR_ARG; }
  // the kernel only visits the K-range of an UPPER factor (scipy.linalg.cholesky's default, gaussian_field.py:30): a lower
  // factor such as np.linalg.cholesky(C) would silently give wrong fields
  for (int i = 1; i < n; ++i)
    for (int j = 0; j < i; ++j)
      if (U[(size_t)i * n + j] != 0.0) { set_error("sampler_create: U must be upper triangular (pass the transpose of a lower factor)"); return FINROM_ERR_ARG; }
  auto* h = new finrom_sampler_s();
  h->n = n;
  int rc = upload(&h->U, U, (size_t)n * n);
  if (rc) { delete h; return rc; }
  *out = h;
  return 0;
}
void finrom_sampler_destroy(finrom_sampler_t h) { if (!h) return; dev_free(h->U); h->xi.release(); h->fpart.release(); h->ftick.release(); delete h; }
int finrom_sampler_draw(finrom_sampler_t h, const double* xi, int64_t S, double* k, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!xi || !k))) { set_error("sampler_draw: bad argument"); return FINROM_ERR_ARG; }
  return launch_sampler(h->U, h->n, xi, S, k, (hipStream_t)stream);
}

int finrom_sampler_draw_seeded(finrom_sampler_t h, uint64_t seed, int64_t first_global_sample, int64_t S, double* k, double* xi_out,
                               void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || first_global_sample < 0 || (S > 0 && !k)) { set_error("sampler_draw_seeded: bad argument"); return FINROM_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  // pieces of <= 32k samples bound the xi scratch (1 GiB at n = 4101) when the caller does not want xi back
  const int64_t piece = xi_out ? S : std::min<int64_t>(S, 32768);
  for (int64_t s0 = 0; s0 < S; s0 += piece) {
    const int64_t Sc = std::min(piece, S - s0);
    double* xi = xi_out ? xi_out + s0 * h->n : nullptr;
    if (!xi) { int rc = h->xi.reserve((size_t)Sc * h->n * sizeof(double)); if (rc) return rc; xi = (double*)h->xi.p; }
    int rc = launch_philox_normal(seed, first_global_sample + s0, Sc, h->n, xi, st);
    if (!rc) rc = launch_sampler(h->U, h->n, xi, Sc, k + s0 * h->n, st);
    if (rc) return rc;
  }
  return 0;
}

}  // extern "C"
// the two triangular products' workspace on the handle (field_prior.hip): grown outside a capture only (Scratch::reserve refuses
// it inside one, with a message); the arrival counters are zeroed once, the kernels leave them zero
static int field_prior_ws(finrom_sampler_t h, int64_t S) {
  const bool fresh = h->ftick.p == nullptr;
  if (int rc = h->ftick.reserve(field_prior_tick_bytes(h->n))) return rc;
  if (fresh) FR_HIP(hipMemset(h->ftick.p, 0, field_prior_tick_bytes(h->n)));
  return h->fpart.reserve(field_prior_part_bytes(h->n, S));
}
extern "C" {
int finrom_sampler_field(finrom_sampler_t h, const double* mean, const double* v, int64_t S, double* k, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!v || !k))) { set_error("sampler_field: bad argument (null handle, v or k, or S < 0)"); return FINROM_ERR_ARG; }
  if (S == 0) return 0;
  if (int rc = field_prior_ws(h, S)) return rc;
  return launch_field_prior(h->U, h->n, 0, v, nullptr, 0.0, mean, k, nullptr, nullptr, S, (double*)h->fpart.p, (int*)h->ftick.p,
                            (hipStream_t)stream);
}
int finrom_sampler_pullback(finrom_sampler_t h, const double* g, int64_t S, double* out, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!g || !out))) { set_error("sampler_pullback: bad argument (null handle, g or out, or S < 0)"); return FINROM_ERR_ARG; }
  if (S == 0) return 0;
  if (int rc = field_prior_ws(h, S)) return rc;
  return launch_field_prior(h->U, h->n, 1, g, nullptr, 0.0, nullptr, out, nullptr, nullptr, S, (double*)h->fpart.p, (int*)h->ftick.p,
                            (hipStream_t)stream);
}

int finrom_mlp_create(const finrom_mlp_desc* a, finrom_mlp_t* out) {
  if (!a || !out) { set_error("mlp_create: null argument"); return FINROM_ERR_ARG; }
  *out = nullptr;
  if (a->n_in <= 0 || a->n_w <= 0 || a->n_w > 64 || a->n_layers < 0 || a->n_layers > 64 || a->n_out <= 0 || a->n_out > 64 ||
      !a->W0 || !a->b0 || !a->scale || !a->shift || !a->Wh || !a->bh || (a->n_layers > 0 && (!a->W || !a->b))) {
    set_error("mlp_create: inconsistent sizes (n_w, n_out <= 64)"); return FINROM_ERR_ARG;
  }
  auto* h = new finrom_mlp_s();
  MlpDev& d = h->d;
  d.n_in = a->n_in; d.n_w = a->n_w; d.n_layers = a->n_layers; d.n_out = a->n_out;
  int rc = 0;
  const size_t nw = a->n_w, L = a->n_layers;
  if (!rc) rc = up(h->owned, &d.W0, a->W0, (size_t)a->n_in * nw);
  if (!rc) rc = up(h->owned, &d.b0, a->b0, nw);
  if (!rc) rc = up(h->owned, &d.scale, a->scale, (L + 1) * nw);
  if (!rc) rc = up(h->owned, &d.shift, a->shift, (L + 1) * nw);
  if (!rc) rc = up(h->owned, &d.W, a->W, L * nw * nw);
  if (!rc) rc = up(h->owned, &d.b, a->b, L * nw);
  if (!rc) rc = up(h->owned, &d.Wh, a->Wh, nw * a->n_out);
  if (!rc) rc = up(h->owned, &d.bh, a->bh, (size_t)a->n_out);
  if (rc) { finrom_mlp_destroy(h); return rc; }
  *out = h;
  return 0;
}
void finrom_mlp_destroy(finrom_mlp_t h) {
  if (!h) return;
  for (void* p : h->owned) dev_free(p);
  h->tape.release(); h->theta.release(); h->gth.release(); h->shift.release(); h->qtmp.release(); h->etmp.release(); h->g0.release(); h->y0p.release(); h->thp.release();
  h->sur_w.release(); h->sur_zero.release(); h->sur_bad.release(); h->hml_grad.release();
  delete h;
}
int finrom_mlp_predict(finrom_mlp_t h, const double* k, int64_t S, double* e, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!k || !e))) { set_error("mlp_predict: bad argument"); return FINROM_ERR_ARG; }
  if (int fits = mlp_forward_fits(h->d)) return fits;      // (before any device call)
  int rc = h->tape.reserve((size_t)S * (h->d.n_layers + 1) * h->d.n_w * sizeof(float));
  if (rc) return rc;
  return launch_mlp_forward(h->d, k, S, nullptr, 0, (float*)h->tape.p, e, nullptr, (hipStream_t)stream);
}
int32_t finrom_mlp_stage_reach(int32_t n_layers, int32_t n_w, int32_t n_out, int32_t* staged, int32_t* stage_floats) {
  if (n_layers < 0 || n_layers > 64 || n_w <= 0 || n_w > 64 || n_out <= 0 || n_out > 64) { set_error("mlp_stage_reach: sizes outside finrom_mlp_create's"); return FINROM_ERR_ARG; }
  if (staged) *staged = mlp_tail_staged(n_layers, n_w, n_out) ? 1 : 0;
  if (stage_floats) *stage_floats = MLP_STAGE_FLOATS;
  return mlp_stage_reach(n_layers, n_w, n_out);
}
int32_t finrom_mlp_forward_max_in(void) { return MLP_FORWARD_MAX_IN; }
int finrom_mlp_set_tile_min(finrom_mlp_t h, int64_t tile_min) {
  if (!h || tile_min < 1) { set_error("mlp_set_tile_min: null handle or tile_min < 1"); return FINROM_ERR_ARG; }
  h->tile_min = tile_min;
  return 0;
}
int finrom_mlp_last_form(finrom_mlp_t h) { return h ? h->last_form : 0; }
int finrom_mlp_misfit_grad(finrom_mlp_t h, const double* k, const double* data, int32_t data_per_sample, int64_t S, double* grad,
                           double* loss, double* out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  CallGuard cg(st);
  if (!h || S < 0 || (S > 0 && !k)) { set_error("mlp_misfit_grad: bad argument (null handle or k, or S < 0)"); return FINROM_ERR_ARG; }
  if ((data == nullptr) != (loss == nullptr)) { set_error("mlp_misfit_grad: data and loss are given or left out together"); return FINROM_ERR_ARG; }
  if (grad != nullptr && data == nullptr) { set_error("mlp_misfit_grad: the gradient needs data"); return FINROM_ERR_ARG; }
  if (!grad && !loss && !out) { set_error("mlp_misfit_grad: at least one of grad, loss, out is required"); return FINROM_ERR_ARG; }
  if (S == 0) return 0;
  const MlpDev& m = h->d;
  const bool tile = S >= h->tile_min;
  if (!tile) { if (int fits = mlp_forward_fits(m)) return fits; }      // (before any device call)
  const int no = m.n_out;
  const int64_t stride = data_per_sample ? no : 0;
  int rc;
  if (tile && !h->sur_ready) {
    if (call_captures() || any_capture()) {
      set_error("mlp_misfit_grad: the tile form's padded weights cannot be made while a stream capture is open: run the same call once "
                "before the capture begins");
      return FINROM_ERR_UNSUPPORTED;
    }
    if ((rc = h->sur_w.reserve(sur_pad_floats(m) * sizeof(float)))) return rc;
    if ((rc = launch_sur_pad(m, (float*)h->sur_w.p, &h->sur_pad, st))) return rc;
    FR_HIP(hipStreamSynchronize(st));                  // (a later call may come on another stream)
    h->sur_ready = true;
  }
  // the per-sample forward writes its tape whatever is asked for; the tile form only for a gradient
  if (!tile || grad) { if ((rc = h->tape.reserve((size_t)S * (m.n_layers + 1) * m.n_w * sizeof(float)))) return rc; }
  if (!out) { if ((rc = h->etmp.reserve((size_t)S * no * sizeof(double)))) return rc; out = (double*)h->etmp.p; }
  if (tile) {
    if ((rc = h->sur_bad.reserve((size_t)S * sizeof(int)))) return rc;
    if ((rc = launch_sur_tile_forward(m, h->sur_pad, k, S, data, stride, grad ? (float*)h->tape.p : nullptr, out, loss, (int*)h->sur_bad.p, st))) return rc;
    if (grad && (rc = launch_sur_tile_backward(m, h->sur_pad, S, (const float*)h->tape.p, data, stride, out, (const int*)h->sur_bad.p, grad, st))) return rc;
    h->last_form = 2;
    return 0;
  }
  if (grad) {                                          // the walk back's qoi_r operand: zeros (0 + e is exact)
    const size_t cap0 = h->sur_zero.cap;
    if ((rc = h->sur_zero.reserve((size_t)S * no * sizeof(double)))) return rc;
    if (h->sur_zero.cap != cap0) {                     // (grown: outside any capture)
      FR_HIP(hipMemsetAsync(h->sur_zero.p, 0, h->sur_zero.cap, st));
      FR_HIP(hipStreamSynchronize(st));
    }
  }
  if ((rc = launch_sur_forward(m, k, S, data, stride, (float*)h->tape.p, out, loss, st))) return rc;
  if (grad && (rc = launch_sur_backward(m, S, (const float*)h->tape.p, data, stride, (const double*)h->sur_zero.p, out, grad, st))) return rc;
  h->last_form = 1;
  return 0;
}
}  // extern "C"
// clears the caller's info for the forms of romml_grad_impl whose kernels only ever flag in (a kernel node, not a memset node: below)
__global__ __launch_bounds__(256) static void clear_info_kernel(int32_t* __restrict__ info, int64_t S) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < S) info[i] = 0;
}
// (hs: the call is a leapfrog step -- finrom_hmc_leapfrog: position update in front, momentum update behind; one-sample form only)
struct HmcStep { const double* mom; double eps; double* k_out; HmcTail tail; const double* theta_parts_in; };
static int romml_grad_impl(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, const double* k, const double* data,
                           int32_t data_per_sample, int64_t S, double* grad, double* loss, double* qoi_r, double* e_nn,
                           int32_t* info, void* stream, const HmcStep* hs) {
  if (!rom || !mlp || !Sop || S < 0 || (S > 0 && (!k || !data || (!grad && !hs) || !loss))) { set_error("romml_grad: bad argument"); return FINROM_ERR_ARG; }
  const MlpDev& m = mlp->d;
  if (m.n_out != rom->d.n_obs) { set_error("romml_grad: the error model's outputs are not the ROM's observables"); return FINROM_ERR_ARG; }
  if (S == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int P = rom->d.P, no = m.n_out;
  int rc;
  if ((rc = mlp->tape.reserve((size_t)S * (m.n_layers + 1) * m.n_w * sizeof(float)))) return rc;
  if ((rc = mlp->theta.reserve(((size_t)S * P + (size_t)S * 16 * 16) * sizeof(double)))) return rc;      // theta | the contraction workgroups' own copies (MlpFuse)
  if ((rc = mlp->gth.reserve((size_t)S * P * sizeof(double)))) return rc;
  if ((rc = mlp->shift.reserve((size_t)S * no * sizeof(double)))) return rc;
  if (!qoi_r) { if ((rc = mlp->qtmp.reserve((size_t)S * no * sizeof(double)))) return rc; qoi_r = (double*)mlp->qtmp.p; }
  if (!e_nn) { if ((rc = mlp->etmp.reserve((size_t)S * no * sizeof(double)))) return rc; e_nn = (double*)mlp->etmp.p; }
  const int64_t stride = data_per_sample ? no : 0;
  // (the sub-fin averages theta = S k are formed inside the network's forward kernel: it reads k anyway)
  // One-sample form (the ROM's contraction + solve kernels, S <= 64): the gradient contraction leaves its partial sums to the
  // error model's backward kernel instead of fencing and drawing tickets for a last workgroup (-7 us per call); the error
  // model's forward pass is one more workgroup per sample of the ROM's contraction kernel (MlpFuse), behind the sub-fin averages.
  // (Tried and removed: under stream capture, the error model's forward kernel on a side stream beside the ROM's contraction
  // kernel -- the solve kernel is the first to need its output.  One fork / join inside a replayed graph cost ~240 us per call
  // on this runtime: 113 -> 355 us, tools/graph_call_cost.py.)
  const bool one = rom->projection == FINROM_PROJECTION_DIRECT && rom_onesample_applies(rom->d, S) && rom->g_npairs > 0;
  if (hs != nullptr && !(one && P <= 16)) {
    set_error("hmc_leapfrog: needs the one-sample form of the reduced model (<= 64 chains, direct projection, r <= 96, <= 16 averages, finrom_rom_set_gradient)");
    return FINROM_ERR_UNSUPPORTED;
  }
  MlpFuse fm;
  if (hs != nullptr) { fm.mom = hs->mom; fm.eps = hs->eps; fm.k_out = hs->k_out; fm.theta_parts = hs->theta_parts_in; }
  if (one && P <= 16) {                                // the network's forward pass and theta = S k ride in the ROM's contraction kernel
    fm.on = 1; fm.m = m; fm.k = k; fm.data = data; fm.data_stride = stride; fm.tape = (float*)mlp->tape.p; fm.e_out = e_nn;
    fm.data_shift = (double*)mlp->shift.p;
    if ((rc = mlp->y0p.reserve((size_t)S * fm.nw0 * 64 * sizeof(float)))) return rc;
    fm.y0_part = (float*)mlp->y0p.p;
    fm.Sop = Sop; fm.P = P; fm.theta_out = (double*)mlp->theta.p; fm.theta_scr = (double*)mlp->theta.p + (size_t)S * P;
  } else if (P <= 16) {
    if ((rc = launch_mlp_forward(m, k, S, data, stride, (float*)mlp->tape.p, e_nn, (double*)mlp->shift.p, st, Sop, P, (double*)mlp->theta.p))) return rc;
  } else {
    if ((rc = launch_subfin_avg(Sop, P, m.n_in, k, S, (double*)mlp->theta.p, st))) return rc;
    if ((rc = launch_mlp_forward(m, k, S, data, stride, (float*)mlp->tape.p, e_nn, (double*)mlp->shift.p, st))) return rc;
  }
  MlpBackFuse bf;
  if (fm.on) {
    if ((rc = mlp->g0.reserve((size_t)S * 64 * sizeof(float)))) return rc;
    bf.on = 1; bf.m = m; bf.tape = (const float*)mlp->tape.p; bf.data = data; bf.data_stride = stride; bf.qoi_r = qoi_r; bf.e_nn = e_nn;
    bf.g0_out = (float*)mlp->g0.p;
  }
  // info is this call's alone: stored by the one-sample solve kernel, cleared here for the other forms (whose kernels or flags in)
  // (by a kernel, not hipMemsetAsync: inside a captured graph the memset node cleared info in the first replay only, and the
  // chains of every later replay kept the flags they came with -- tests/test_gpu_hmc_leapfrog_field.py starts them at 5)
  if (info != nullptr && !one) {
    hipLaunchKernelGGL(clear_info_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, info, S);
    FR_HIP(hipGetLastError());
  }
  rom->defer_gsum = one; rom->last_gpart = nullptr; rom->fuse = fm.on ? &fm : nullptr; rom->back = bf.on ? &bf : nullptr;
  rom->info_store = one;
  rc = finrom_rom_grad(rom, (const double*)mlp->theta.p, (const double*)mlp->shift.p, 1, S, loss, (double*)mlp->gth.p, nullptr,
                       qoi_r, info, st);
  const double* gparts = rom->last_gpart;
  rom->defer_gsum = false; rom->last_gpart = nullptr; rom->fuse = nullptr; rom->back = nullptr; rom->info_store = false;
  if (rc) return rc;
  if (fm.on && gparts == nullptr) {                    // (the predicate above and finrom_rom_grad's own must agree)
    set_error("romml_grad: internal: the one-sample form was announced but not taken");
    return FINROM_ERR_UNSUPPORTED;
  }
  return launch_mlp_backward(m, S, (const float*)mlp->tape.p, data, stride, qoi_r, e_nn, (const double*)mlp->gth.p, Sop, P, grad, st,
                             gparts, gparts ? ROM_GRAD_SMALL_NG : 0, bf.on && gparts ? (const float*)mlp->g0.p : nullptr,
                             hs != nullptr ? &hs->tail : nullptr);
}
extern "C" {

int finrom_romml_grad(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, const double* k, const double* data,
                      int32_t data_per_sample, int64_t S, double* grad, double* loss, double* qoi_r, double* e_nn,
                      int32_t* info, void* stream) {
  CallGuard cg((hipStream_t)stream);
  return romml_grad_impl(rom, mlp, Sop, k, data, data_per_sample, S, grad, loss, qoi_r, e_nn, info, stream, nullptr);
}

}  // extern "C"
static int hmc_dev(const finrom_hmc_state* a, HmcDev* h, const char* who) {
  if (!a || a->C < 0 || a->n <= 0 || !a->mean || !a->K || !a->U || !a->dU || !a->Kq[0] || !a->Kq[1] || !a->P || !a->dUq || !a->H0 ||
      !a->P_block || !a->lu_block || !a->jt || !a->pt || !a->accept || !a->loss || !a->info) {
    set_error(std::string(who) + ": null field in finrom_hmc_state"); return FINROM_ERR_ARG;
  }
  h->C = a->C; h->n = a->n; h->eps = a->eps; h->c_lik = a->c_lik; h->c_pri = a->c_pri;
  h->mean = a->mean; h->K = a->K; h->U = a->U; h->dU = a->dU; h->Kq0 = a->Kq[0]; h->P = a->P; h->dUq = a->dUq; h->H0 = a->H0;
  h->P_block = a->P_block; h->lu_block = a->lu_block; h->jt = (long long*)a->jt; h->pt = (long long*)a->pt;
  h->accept = (long long*)a->accept; h->trace = a->trace; h->loss = a->loss; h->info = a->info;
  return 0;
}
extern "C" {
int finrom_hmc_begin(const finrom_hmc_state* a, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_begin")) return rc;
  return launch_hmc_begin(h, (hipStream_t)stream);
}
int finrom_hmc_end(const finrom_hmc_state* a, int32_t n_steps, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_end")) return rc;
  if (n_steps < 0) { set_error("hmc_end: n_steps < 0"); return FINROM_ERR_ARG; }
  return launch_hmc_end(h, a->Kq[n_steps & 1], (hipStream_t)stream);       // (the position ping-pongs once per step)
}
int finrom_hmc_draw(const uint64_t* seeds, int64_t C, int32_t n, int64_t first_proposal, int64_t B, double* P_block, double* lu_block,
                    void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (C < 0) { set_error("hmc_draw: C < 0"); return FINROM_ERR_ARG; }
  if (B < 0) { set_error("hmc_draw: B < 0"); return FINROM_ERR_ARG; }
  if (first_proposal < 0) { set_error("hmc_draw: first_proposal < 0"); return FINROM_ERR_ARG; }
  if (n < 1) { set_error("hmc_draw: n < 1"); return FINROM_ERR_ARG; }
  if (B == 0 || C == 0) return 0;
  if (!seeds || !P_block || !lu_block) { set_error("hmc_draw: null seeds, P_block or lu_block"); return FINROM_ERR_ARG; }
  if (B > INT64_MAX / C || B * C > INT64_MAX / 8 / n || first_proposal > INT64_MAX - B) {
    set_error("hmc_draw: B x C x n or first_proposal + B does not fit 64 bits"); return FINROM_ERR_ARG;
  }
  return launch_hmc_draw((const unsigned long long*)seeds, C, n, first_proposal, B, P_block, lu_block, (hipStream_t)stream);
}
int finrom_hmc_end_stage1(const finrom_hmc_state* a, int32_t n_steps, int32_t* ok1, double* Uq, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_end_stage1")) return rc;
  if (n_steps < 0) { set_error("hmc_end_stage1: n_steps < 0"); return FINROM_ERR_ARG; }
  if (h.C == 0) return 0;
  if (!ok1 || !Uq) { set_error("hmc_end_stage1: null ok1 or Uq"); return FINROM_ERR_ARG; }
  return launch_hmc_end_stage1(h, a->Kq[n_steps & 1], ok1, Uq, (hipStream_t)stream);
}
int finrom_hmc_end_stage2(const finrom_hmc_state* a, int32_t n_steps, const finrom_hmc_da* da, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_end_stage2")) return rc;
  if (n_steps < 0) { set_error("hmc_end_stage2: n_steps < 0"); return FINROM_ERR_ARG; }
  if (!da) { set_error("hmc_end_stage2: null descriptor"); return FINROM_ERR_ARG; }
  if (da->n_obs < 1) { set_error("hmc_end_stage2: n_obs < 1"); return FINROM_ERR_ARG; }
  if (h.C == 0) return 0;
  if (!da->ok1 || !da->Uq || !da->qoi_f || !da->info_f || !da->data || !da->lu2_block || !da->D || !da->loss_f || !da->accept1 ||
      !da->cand_loss_f) {
    set_error("hmc_end_stage2: null pointer in finrom_hmc_da (only correction may be NULL)"); return FINROM_ERR_ARG;
  }
  return launch_hmc_end_stage2(h, a->Kq[n_steps & 1], *da, (hipStream_t)stream);
}
int finrom_hmc_draw_stage2(const uint64_t* seeds, int64_t C, int64_t first_proposal, int64_t B, double* lu2_block, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (C < 0) { set_error("hmc_draw_stage2: C < 0"); return FINROM_ERR_ARG; }
  if (B < 0) { set_error("hmc_draw_stage2: B < 0"); return FINROM_ERR_ARG; }
  if (first_proposal < 0) { set_error("hmc_draw_stage2: first_proposal < 0"); return FINROM_ERR_ARG; }
  if (B == 0 || C == 0) return 0;
  if (!seeds || !lu2_block) { set_error("hmc_draw_stage2: null seeds or lu2_block"); return FINROM_ERR_ARG; }
  if (B > INT64_MAX / 8 / C || first_proposal > INT64_MAX - B) {
    set_error("hmc_draw_stage2: B x C or first_proposal + B does not fit 64 bits"); return FINROM_ERR_ARG;
  }
  return launch_hmc_draw_stage2((const unsigned long long*)seeds, C, first_proposal, B, lu2_block, (hipStream_t)stream);
}
int finrom_hmc_stats_update(const finrom_hmc_stats* s, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!s) { set_error("hmc_stats_update: null descriptor"); return FINROM_ERR_ARG; }
  if (s->C < 0) { set_error("hmc_stats_update: C < 0"); return FINROM_ERR_ARG; }
  if (s->n < 1) { set_error("hmc_stats_update: n < 1"); return FINROM_ERR_ARG; }
  if (s->batch < 1) { set_error("hmc_stats_update: batch < 1"); return FINROM_ERR_ARG; }
  if (s->burn < 0) { set_error("hmc_stats_update: burn < 0"); return FINROM_ERR_ARG; }
  if (s->proposal0 < 0) { set_error("hmc_stats_update: proposal0 < 0"); return FINROM_ERR_ARG; }
  if (s->C == 0) return 0;
  if (s->C > 65535) { set_error("hmc_stats_update: C > 65535 (one grid row per chain)"); return FINROM_ERR_ARG; }
  if (!s->pt || !s->accept || !s->cand || !s->cand_loss || !s->cur || !s->cur_loss || !s->acc_prev || !s->mean || !s->m2 ||
      !s->bsum || !s->bm_mean || !s->bm_m2) {
    set_error("hmc_stats_update: null pointer in finrom_hmc_stats (only misfit and accepted may be NULL)"); return FINROM_ERR_ARG;
  }
  return launch_hmc_stats(*s, (hipStream_t)stream);
}
int finrom_hmc_leapfrog(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, const finrom_hmc_state* a, int32_t step,
                        const double* data, int32_t data_per_sample, double* grad_out, double* qoi_r, double* e_nn, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_leapfrog")) return rc;
  if (!rom || !mlp || a->n != mlp->d.n_in || step < 0) { set_error("hmc_leapfrog: bad argument"); return FINROM_ERR_ARG; }
  if (a->c_pri == 0.0) { set_error("hmc_leapfrog: c_pri = 0"); return FINROM_ERR_ARG; }
  HmcStep hs;
  hs.mom = a->P; hs.eps = a->eps; hs.k_out = a->Kq[(step + 1) & 1];
  // theta of THIS step's field from the previous step's momentum update, when this is that field's step (not the first step of a
  // trajectory: finrom_hmc_begin has no averaging operator at hand); and this step leaves the next one's
  if (int rc = mlp->thp.reserve((size_t)a->C * HMC_THETA_PARTS * 16 * sizeof(double))) return rc;
  const bool carried = step > 0 && mlp->carry_k == a->Kq[step & 1] && mlp->carry_mom == a->P && mlp->carry_eps == a->eps &&
                       mlp->carry_S == a->C;
  hs.theta_parts_in = carried ? (const double*)mlp->thp.p : nullptr;
  hs.tail.eps = a->eps; hs.tail.theta_parts = rom->d.P <= HMC_THETA_MAXP ? (double*)mlp->thp.p : nullptr;
  mlp->carry_k = nullptr;
  hs.tail.on = 1; hs.tail.kq = hs.k_out; hs.tail.mean = a->mean; hs.tail.mom = a->P; hs.tail.dU = a->dUq;
  hs.tail.coef = a->c_lik / a->c_pri; hs.tail.eps_cpri = a->eps * a->c_pri; hs.tail.info = a->info;
  const int rc = romml_grad_impl(rom, mlp, Sop, a->Kq[step & 1], data, data_per_sample, a->C, grad_out, a->loss, qoi_r, e_nn, a->info, stream, &hs);
  if (rc == 0 && hs.tail.theta_parts != nullptr) { mlp->carry_k = hs.k_out; mlp->carry_mom = a->P; mlp->carry_eps = a->eps; mlp->carry_S = a->C; }
  return rc;
}

}  // extern "C"
// the leapfrog step in whitened coordinates: field kernel (position update in front), the plain romml value and gradient at the
// field, pullback kernel (momentum update behind); no theta carry (the field is not the position)
// (metric: the position moves along vel = M^-1 p, formed first -- finrom_hmc_leapfrog_field_metric; nullptr: along p itself)
static int hmc_leapfrog_field_impl(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, finrom_sampler_t prior, const double* field_mean,
                                   double* field, double* grad_field, const finrom_hmc_state* a, int32_t step, const double* data,
                                   int32_t data_per_sample, double* qoi_r, double* e_nn, const MetricDev* metric, double* vel,
                                   void* stream) {
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_leapfrog_field")) return rc;
  if (a->c_pri != 1.0) { set_error("hmc_leapfrog_field: c_pri must be 1 (whitened coordinates: the prior of v is N(0, I))"); return FINROM_ERR_ARG; }
  if (step < 0) { set_error("hmc_leapfrog_field: step < 0"); return FINROM_ERR_ARG; }
  if (!rom || !mlp || !Sop || !prior) { set_error("hmc_leapfrog_field: null rom, mlp, Sop or prior handle"); return FINROM_ERR_ARG; }
  if (!field || !grad_field || !data) { set_error("hmc_leapfrog_field: null field, grad_field or data"); return FINROM_ERR_ARG; }
  if (a->n != prior->n || a->n != mlp->d.n_in) {
    set_error("hmc_leapfrog_field: n = " + std::to_string(a->n) + " is not the prior's (" + std::to_string(prior->n) +
              ") or the error model's input size (" + std::to_string(mlp->d.n_in) + ")");
    return FINROM_ERR_ARG;
  }
  mlp->carry_k = nullptr;                  // (a theta carry of finrom_hmc_leapfrog does not survive a step of this form)
  if (a->C == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = field_prior_ws(prior, a->C)) return rc;
  double* vq = a->Kq[(step + 1) & 1];
  int rc = metric ? launch_hmc_velocity(*metric, a->P, a->C, vel, st) : 0;
  if (!rc) rc = launch_field_prior(prior->U, prior->n, 0, a->Kq[step & 1], metric ? vel : a->P, a->eps, field_mean, field, vq, nullptr,
                                   a->C, (double*)prior->fpart.p, (int*)prior->ftick.p, st);
  if (!rc) rc = romml_grad_impl(rom, mlp, Sop, field, data, data_per_sample, a->C, grad_field, a->loss, qoi_r, e_nn, a->info, stream, nullptr);
  if (rc) return rc;
  FieldPriorTail tl;
  tl.vq = vq; tl.c_lik = a->c_lik; tl.info = a->info; tl.mom = a->P; tl.dU = a->dUq; tl.eps = a->eps;
  return launch_field_prior(prior->U, prior->n, 1, grad_field, nullptr, 0.0, nullptr, nullptr, nullptr, &tl, a->C,
                            (double*)prior->fpart.p, (int*)prior->ftick.p, st);
}
extern "C" {
int finrom_hmc_leapfrog_field(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, finrom_sampler_t prior, const double* field_mean,
                              double* field, double* grad_field, const finrom_hmc_state* a, int32_t step, const double* data,
                              int32_t data_per_sample, double* qoi_r, double* e_nn, void* stream) {
  CallGuard cg((hipStream_t)stream);
  return hmc_leapfrog_field_impl(rom, mlp, Sop, prior, field_mean, field, grad_field, a, step, data, data_per_sample, qoi_r, e_nn,
                                 nullptr, nullptr, stream);
}

}  // extern "C"
// ---- the chains under the full-order and the plain reduced model (hmc_model.hip; hmc.py model="fom" | "rom") ----------------------
static int hmc_model_map_check(const char* who, const double* A, int32_t P) {
  if (A != nullptr && (P < 1 || P > HMC_MODEL_MAXP)) {
    set_error(std::string(who) + ": P = " + std::to_string(P) + " is outside 1 .. " + std::to_string(HMC_MODEL_MAXP));
    return FINROM_ERR_ARG;
  }
  return 0;
}
static int hmc_drift_impl(const finrom_hmc_state* a, int32_t step, const double* A, const double* theta0, int32_t P, double* theta_out,
                          void* stream, const char* who) {
  HmcDev h;
  if (int rc = hmc_dev(a, &h, who)) return rc;
  if (step < 0) { set_error(std::string(who) + ": step < 0"); return FINROM_ERR_ARG; }
  if (int rc = hmc_model_map_check(who, A, P)) return rc;
  if (A != nullptr && !theta_out) { set_error(std::string(who) + ": A without theta_out"); return FINROM_ERR_ARG; }
  if (a->C > INT32_MAX) { set_error(std::string(who) + ": C > 2^31 - 1 (one workgroup per chain)"); return FINROM_ERR_ARG; }
  return launch_hmc_drift(h, a->Kq[step & 1], a->Kq[(step + 1) & 1], A, theta0, P, theta_out, (hipStream_t)stream);
}
static int hmc_kick_impl(const finrom_hmc_state* a, int32_t step, const double* grad, const double* g_theta, const double* A, int32_t P,
                         double* grad_out, void* stream, const char* who) {
  HmcDev h;
  if (int rc = hmc_dev(a, &h, who)) return rc;
  if (step < 0) { set_error(std::string(who) + ": step < 0"); return FINROM_ERR_ARG; }
  if ((grad != nullptr) == (g_theta != nullptr)) {
    set_error(std::string(who) + ": exactly one of grad and g_theta must be given"); return FINROM_ERR_ARG;
  }
  if (g_theta != nullptr && !A) { set_error(std::string(who) + ": g_theta without A"); return FINROM_ERR_ARG; }
  if (g_theta != nullptr) { if (int rc = hmc_model_map_check(who, A, P)) return rc; }
  if (a->c_pri == 0.0) { set_error(std::string(who) + ": c_pri = 0"); return FINROM_ERR_ARG; }
  if (a->C > 65535) { set_error(std::string(who) + ": C > 65535 (one grid row per chain)"); return FINROM_ERR_ARG; }
  return launch_hmc_kick(h, a->Kq[(step + 1) & 1], grad, g_theta, A, P, grad_out, (hipStream_t)stream);
}
extern "C" {
int finrom_hmc_drift(const finrom_hmc_state* a, int32_t step, const double* A, const double* theta0, int32_t P, double* theta_out,
                     void* stream) {
  CallGuard cg((hipStream_t)stream);
  return hmc_drift_impl(a, step, A, theta0, P, theta_out, stream, "hmc_drift");
}
int finrom_hmc_kick(const finrom_hmc_state* a, int32_t step, const double* grad, const double* g_theta, const double* A, int32_t P,
                    double* grad_out, void* stream) {
  CallGuard cg((hipStream_t)stream);
  return hmc_kick_impl(a, step, grad, g_theta, A, P, grad_out, stream, "hmc_kick");
}
}  // extern "C"
// info is this step's alone: finrom_fom_gradient's and finrom_rom_grad's kernels flag into it (a kernel node: see romml_grad_impl)
static int hmc_clear_info(int32_t* info, int64_t S, hipStream_t st) {
  hipLaunchKernelGGL(clear_info_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, info, S);
  FR_HIP(hipGetLastError());
  return 0;
}
static int hmc_fom_check(finrom_fom_t fom, const finrom_hmc_state* a, const double* data, const char* who) {
  if (!fom || !data) { set_error(std::string(who) + ": null fom handle or data"); return FINROM_ERR_ARG; }
  if (fom->d.xdim != a->n) {
    set_error(std::string(who) + ": n = " + std::to_string(a->n) + " is not the full-order model's parameter count (" +
              std::to_string(fom->d.xdim) + "): the chains move nodal fields");
    return FINROM_ERR_UNSUPPORTED;
  }
  if (a->C > 65535) { set_error(std::string(who) + ": C > 65535 (one grid row per chain)"); return FINROM_ERR_UNSUPPORTED; }
  return 0;
}
extern "C" {
int finrom_hmc_leapfrog_fom(finrom_fom_t fom, const finrom_hmc_state* a, int32_t step, const double* data, int32_t data_per_sample,
                            double* grad_out, double* qoi, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_leapfrog_fom")) return rc;
  if (step < 0) { set_error("hmc_leapfrog_fom: step < 0"); return FINROM_ERR_ARG; }
  if (a->c_pri == 0.0) { set_error("hmc_leapfrog_fom: c_pri = 0"); return FINROM_ERR_ARG; }
  if (int rc = hmc_fom_check(fom, a, data, "hmc_leapfrog_fom")) return rc;
  if (a->C == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  double* g = grad_out;
  if (!g) { if (int rc = fom->hgrad.reserve((size_t)a->C * a->n * sizeof(double))) return rc; g = (double*)fom->hgrad.p; }
  double* kq = a->Kq[(step + 1) & 1];
  int rc = hmc_drift_impl(a, step, nullptr, nullptr, 0, nullptr, stream, "hmc_leapfrog_fom");
  if (!rc) rc = hmc_clear_info(a->info, a->C, st);
  if (!rc) rc = finrom_fom_gradient(fom, kq, data, data_per_sample, a->C, g, a->loss, qoi, a->info, stream);
  if (!rc) rc = hmc_kick_impl(a, step, g, nullptr, nullptr, 0, nullptr, stream, "hmc_leapfrog_fom");
  return rc;
}
int finrom_hmc_leapfrog_field_fom(finrom_fom_t fom, finrom_sampler_t prior, const double* field_mean, double* field, double* grad_field,
                                  const finrom_hmc_state* a, int32_t step, const double* data, int32_t data_per_sample, double* qoi,
                                  void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_leapfrog_field_fom")) return rc;
  if (a->c_pri != 1.0) { set_error("hmc_leapfrog_field_fom: c_pri must be 1 (whitened coordinates: the prior of v is N(0, I))"); return FINROM_ERR_ARG; }
  if (step < 0) { set_error("hmc_leapfrog_field_fom: step < 0"); return FINROM_ERR_ARG; }
  if (!prior || !field || !grad_field) { set_error("hmc_leapfrog_field_fom: null prior handle, field or grad_field"); return FINROM_ERR_ARG; }
  if (int rc = hmc_fom_check(fom, a, data, "hmc_leapfrog_field_fom")) return rc;
  if (a->n != prior->n) {
    set_error("hmc_leapfrog_field_fom: n = " + std::to_string(a->n) + " is not the prior's (" + std::to_string(prior->n) + ")");
    return FINROM_ERR_ARG;
  }
  if (a->C == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = field_prior_ws(prior, a->C)) return rc;
  double* vq = a->Kq[(step + 1) & 1];
  int rc = launch_field_prior(prior->U, prior->n, 0, a->Kq[step & 1], a->P, a->eps, field_mean, field, vq, nullptr, a->C,
                              (double*)prior->fpart.p, (int*)prior->ftick.p, st);
  if (!rc) rc = hmc_clear_info(a->info, a->C, st);
  if (!rc) rc = finrom_fom_gradient(fom, field, data, data_per_sample, a->C, grad_field, a->loss, qoi, a->info, stream);
  if (rc) return rc;
  FieldPriorTail tl;
  tl.vq = vq; tl.c_lik = a->c_lik; tl.info = a->info; tl.mom = a->P; tl.dU = a->dUq; tl.eps = a->eps;
  return launch_field_prior(prior->U, prior->n, 1, grad_field, nullptr, 0.0, nullptr, nullptr, nullptr, &tl, a->C,
                            (double*)prior->fpart.p, (int*)prior->ftick.p, st);
}
int finrom_hmc_leapfrog_rom(finrom_rom_t rom, const double* A, const double* theta0, const finrom_hmc_state* a, int32_t step,
                            const double* data, int32_t data_per_sample, double* theta, double* g_theta, double* grad_out,
                            double* qoi_r, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_leapfrog_rom")) return rc;
  if (step < 0) { set_error("hmc_leapfrog_rom: step < 0"); return FINROM_ERR_ARG; }
  if (a->c_pri == 0.0) { set_error("hmc_leapfrog_rom: c_pri = 0"); return FINROM_ERR_ARG; }
  if (!rom || !A || !data || !theta || !g_theta) { set_error("hmc_leapfrog_rom: null rom handle, A, data, theta or g_theta"); return FINROM_ERR_ARG; }
  if (rom->g_npairs == 0) { set_error("hmc_leapfrog_rom: finrom_rom_set_gradient has not been called"); return FINROM_ERR_ARG; }
  if (rom->d.P < 1 || rom->d.P > HMC_MODEL_MAXP) {
    set_error("hmc_leapfrog_rom: the reduced model has " + std::to_string(rom->d.P) + " averages; the step serves 1 .. " +
              std::to_string(HMC_MODEL_MAXP));
    return FINROM_ERR_UNSUPPORTED;
  }
  if (a->C > 65535) { set_error("hmc_leapfrog_rom: C > 65535 (one grid row per chain)"); return FINROM_ERR_UNSUPPORTED; }
  if (a->C == 0) return 0;
  const int P = rom->d.P;
  int rc = hmc_drift_impl(a, step, A, theta0, P, theta, stream, "hmc_leapfrog_rom");
  if (!rc) rc = hmc_clear_info(a->info, a->C, (hipStream_t)stream);
  if (!rc) rc = finrom_rom_grad(rom, theta, data, data_per_sample, a->C, a->loss, g_theta, nullptr, qoi_r, a->info, stream);
  if (!rc) rc = hmc_kick_impl(a, step, nullptr, g_theta, A, P, grad_out, stream, "hmc_leapfrog_rom");
  return rc;
}

}  // extern "C"
// ---- the chains under the pure deep-learning surrogate (hmc_ml.hip; hmc.py model="ml", ml_form=) -----------------------------------
// everything both entry points refuse before any device call, then the workspaces on the handle: tape and out per chain, the walk
// back's zero operand (grown outside a capture only: Scratch::reserve refuses inside one, with a message)
static int hmc_ml_prepare(finrom_mlp_t mlp, const finrom_hmc_state* a, const double* data, double** out, const char* who) {
  if (!mlp || !data) { set_error(std::string(who) + ": null mlp handle or data"); return FINROM_ERR_ARG; }
  const MlpDev& m = mlp->d;
  if (a->n != m.n_in) {
    set_error(std::string(who) + ": n = " + std::to_string(a->n) + " is not the network's input size (" + std::to_string(m.n_in) + ")");
    return FINROM_ERR_ARG;
  }
  if (a->c_pri == 0.0) { set_error(std::string(who) + ": c_pri = 0"); return FINROM_ERR_ARG; }
  if (int fits = mlp_forward_fits(m)) return fits;
  if (a->C > 65535) { set_error(std::string(who) + ": C > 65535 (one grid row per chain)"); return FINROM_ERR_UNSUPPORTED; }
  if (a->C == 0) return 0;
  int rc;
  if ((rc = mlp->tape.reserve((size_t)a->C * (m.n_layers + 1) * m.n_w * sizeof(float)))) return rc;
  if (!*out) { if ((rc = mlp->etmp.reserve((size_t)a->C * m.n_out * sizeof(double)))) return rc; *out = (double*)mlp->etmp.p; }
  const size_t cap0 = mlp->sur_zero.cap;
  if ((rc = mlp->sur_zero.reserve((size_t)a->C * m.n_out * sizeof(double)))) return rc;
  if (mlp->sur_zero.cap != cap0) {                     // (grown: outside any capture)
    FR_HIP(hipMemset(mlp->sur_zero.p, 0, mlp->sur_zero.cap));
  }
  return 0;
}
extern "C" {
int finrom_hmc_leapfrog_ml(finrom_mlp_t mlp, const finrom_hmc_state* a, int32_t step, const double* data, int32_t data_per_sample,
                           double* grad_out, double* out, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_leapfrog_ml")) return rc;
  if (step < 0) { set_error("hmc_leapfrog_ml: step < 0"); return FINROM_ERR_ARG; }
  if (int rc = hmc_ml_prepare(mlp, a, data, &out, "hmc_leapfrog_ml")) return rc;
  if (a->C == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const MlpDev& m = mlp->d;
  double* g = grad_out;
  if (!g) { if (int rc = mlp->hml_grad.reserve((size_t)a->C * a->n * sizeof(double))) return rc; g = (double*)mlp->hml_grad.p; }
  const int64_t stride = data_per_sample ? m.n_out : 0;
  double* kq = a->Kq[(step + 1) & 1];
  int rc = launch_hmc_ml_forward(m, h, a->Kq[step & 1], kq, data, stride, (float*)mlp->tape.p, out, a->loss, a->info, st);
  if (!rc) rc = launch_sur_backward(m, a->C, (const float*)mlp->tape.p, data, stride, (const double*)mlp->sur_zero.p, out, g, st);
  if (!rc) rc = launch_hmc_kick(h, kq, g, nullptr, nullptr, 0, nullptr, st);
  return rc;
}
int finrom_hmc_trajectory_ml(finrom_mlp_t mlp, const finrom_hmc_state* a, int32_t n_steps, const double* data, int32_t data_per_sample,
                             void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_trajectory_ml")) return rc;
  if (n_steps < 0) { set_error("hmc_trajectory_ml: n_steps < 0"); return FINROM_ERR_ARG; }
  double* out = nullptr;
  if (int rc = hmc_ml_prepare(mlp, a, data, &out, "hmc_trajectory_ml")) return rc;
  if (a->C == 0) return 0;
  const MlpDev& m = mlp->d;
  return launch_hmc_ml_trajectory(m, h, n_steps, a->Kq[0], a->Kq[1], data, data_per_sample ? m.n_out : 0, (const double*)mlp->sur_zero.p,
                                  (float*)mlp->tape.p, out, a->loss, a->info, (hipStream_t)stream);
}

// ---- low-rank metric (hmc_metric.hip) --------------------------------------------------------------------------------------------
int finrom_metric_create(const double* Vt, const double* lam, int32_t n, int32_t rho, finrom_metric_t* out) {
  if (!out) { set_error("metric_create: null out"); return FINROM_ERR_ARG; }
  *out = nullptr;
  if (!Vt || !lam || n <= 0) { set_error("metric_create: null Vt or lam, or n <= 0"); return FINROM_ERR_ARG; }
  if (rho < 1 || rho > METRIC_MAX_RHO) {
    set_error("metric_create: rho = " + std::to_string(rho) + " (need 1 <= rho <= 64)"); return FINROM_ERR_ARG;
  }
  for (int j = 0; j < rho; ++j)
    if (!std::isfinite(lam[j]) || !(lam[j] > 0.0)) {
      set_error("metric_create: lambda[" + std::to_string(j) + "] = " + std::to_string(lam[j]) + " (need finite and > 0)"); return FINROM_ERR_ARG;
    }
  double worst = 0.0;
  for (int i = 0; i < rho; ++i)
    for (int j = 0; j <= i; ++j) {
      long double s = 0.0L;
      for (int q = 0; q < n; ++q) s += (long double)Vt[(size_t)i * n + q] * Vt[(size_t)j * n + q];
      const double e = std::fabs((double)(s - (i == j ? 1.0L : 0.0L)));
      if (!(e <= worst)) worst = e;                      // (a NaN sticks)
    }
  if (!(worst <= 1e-10)) {
    set_error("metric_create: the rows of Vt are not orthonormal (|Vt Vt^T - I|_max = " + std::to_string(worst) + " > 1e-10)"); return FINROM_ERR_ARG;
  }
  std::vector<double> coef((size_t)METRIC_NUM_COEF * METRIC_MAX_RHO, 0.0);
  for (int j = 0; j < rho; ++j) {                        // (forms without cancellation at small lambda)
    const double l = lam[j], s = std::sqrt(1.0 + l);
    coef[(size_t)METRIC_OP_M * METRIC_MAX_RHO + j] = l;
    coef[(size_t)METRIC_OP_INV * METRIC_MAX_RHO + j] = -l / (1.0 + l);
    coef[(size_t)METRIC_OP_SQRT * METRIC_MAX_RHO + j] = l / (s + 1.0);
    coef[(size_t)METRIC_OP_INVSQRT * METRIC_MAX_RHO + j] = -l / ((1.0 + l) + s);
    coef[(size_t)METRIC_OP_D * METRIC_MAX_RHO + j] = l / (1.0 + l);
  }
  auto* h = new finrom_metric_s();
  h->d.n = n; h->d.rho = rho;
  double* dv = nullptr; double* dc = nullptr;
  int rc = upload(&dv, Vt, (size_t)rho * n);
  if (!rc) rc = upload(&dc, coef.data(), coef.size());
  h->d.Vt = dv; h->d.coef = dc;
  if (rc) { finrom_metric_destroy(h); return rc; }
  *out = h;
  return 0;
}
void finrom_metric_destroy(finrom_metric_t h) { if (!h) return; dev_free((void*)h->d.Vt); dev_free((void*)h->d.coef); delete h; }
int finrom_metric_apply(finrom_metric_t h, int32_t op, const double* x, int64_t S, double* y, double* quad, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!h || S < 0 || (S > 0 && (!x || !y))) { set_error("metric_apply: bad argument (null handle, x or y, or S < 0)"); return FINROM_ERR_ARG; }
  if (op < FINROM_METRIC_M || op > FINROM_METRIC_INVSQRT) { set_error("metric_apply: op = " + std::to_string(op) + " (need 0 .. 3)"); return FINROM_ERR_ARG; }
  if (S > 0 && x == y) { set_error("metric_apply: y must not be x"); return FINROM_ERR_ARG; }
  if (S == 0) return 0;
  return launch_metric_apply(h->d, op, x, S, y, quad, (hipStream_t)stream);
}
}  // extern "C"
static int hmc_metric_check(const finrom_hmc_state* a, finrom_metric_t m, const char* who) {
  if (!m) { set_error(std::string(who) + ": null metric handle"); return FINROM_ERR_ARG; }
  if (a->n != m->d.n) {
    set_error(std::string(who) + ": n = " + std::to_string(a->n) + " is not the metric's (" + std::to_string(m->d.n) + ")"); return FINROM_ERR_ARG;
  }
  return 0;
}
extern "C" {
int finrom_hmc_begin_metric(const finrom_hmc_state* a, finrom_metric_t metric, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_begin_metric")) return rc;
  if (int rc = hmc_metric_check(a, metric, "hmc_begin_metric")) return rc;
  return launch_hmc_begin_metric(h, metric->d, (hipStream_t)stream);
}
int finrom_hmc_end_metric(const finrom_hmc_state* a, finrom_metric_t metric, int32_t n_steps, void* stream) {
  CallGuard cg((hipStream_t)stream);
  HmcDev h;
  if (int rc = hmc_dev(a, &h, "hmc_end_metric")) return rc;
  if (int rc = hmc_metric_check(a, metric, "hmc_end_metric")) return rc;
  if (n_steps < 0) { set_error("hmc_end_metric: n_steps < 0"); return FINROM_ERR_ARG; }
  return launch_hmc_end_metric(h, metric->d, a->Kq[n_steps & 1], (hipStream_t)stream);
}
int finrom_hmc_leapfrog_field_metric(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, finrom_sampler_t prior,
                                     const double* field_mean, double* field, double* grad_field, const finrom_hmc_state* a,
                                     int32_t step, const double* data, int32_t data_per_sample, double* qoi_r, double* e_nn,
                                     finrom_metric_t metric, double* vel, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (!a || !metric || !vel) { set_error("hmc_leapfrog_field_metric: null state, metric handle or vel"); return FINROM_ERR_ARG; }
  if (a->n != metric->d.n) {
    set_error("hmc_leapfrog_field_metric: n = " + std::to_string(a->n) + " is not the metric's (" + std::to_string(metric->d.n) + ")");
    return FINROM_ERR_ARG;
  }
  return hmc_leapfrog_field_impl(rom, mlp, Sop, prior, field_mean, field, grad_field, a, step, data, data_per_sample, qoi_r, e_nn,
                                 &metric->d, vel, stream);
}

}  // extern "C"
// multi-start L-BFGS (lbfgs_kernels.hip): every check on the host, before the stream is looked at
static int lbfgs_dev(const finrom_lbfgs_state* a, LbfgsDev* L, const char* who) {
  auto bad = [&](const std::string& what) { set_error(std::string(who) + ": " + what); return FINROM_ERR_ARG; };
  if (!a) return bad("null state");
  if (a->S < 1) return bad("S = " + std::to_string(a->S) + " (need S >= 1)");
  if (a->S > 0x7fffffff) return bad("S = " + std::to_string(a->S) + " (one workgroup per start: need S < 2^31)");
  if (a->d < 1) return bad("d = " + std::to_string(a->d) + " (need d >= 1)");
  if (a->m < 1 || a->m > LBFGS_MAX_M) return bad("m = " + std::to_string(a->m) + " (need 1 <= m <= 16)");
  if (a->maxls < 1) return bad("maxls = " + std::to_string(a->maxls) + " (need maxls >= 1)");
  if (a->G != nullptr && (a->gdim < 1 || a->gdim > LBFGS_MAX_GDIM)) return bad("gdim = " + std::to_string(a->gdim) + " (need 1 <= gdim <= 16 with G)");
  if (a->G == nullptr && a->gdim != 0) return bad("gdim = " + std::to_string(a->gdim) + " without G (need 0)");
  if (a->k1_ptr != nullptr && (!a->k1_idx || !a->k1_val)) return bad("null k1_idx or k1_val with k1_ptr");
  if (a->fhist != nullptr && a->fhist_rows < 1) return bad("fhist_rows = " + std::to_string(a->fhist_rows) + " with fhist (need >= 1)");
  const char* null_name = !a->x ? "x" : !a->f ? "f" : !a->g ? "g" : !a->xt ? "xt" : !a->work ? "work" : !a->status ? "status" :
                          !a->nit ? "nit" : !a->nfev ? "nfev" : nullptr;
  if (null_name) return bad(std::string("null ") + null_name);
  if ((int64_t)a->d > (int64_t)LBFGS_MAX_E * 256) {
    set_error(std::string(who) + ": d = " + std::to_string(a->d) + " > 4352 (the kernels hold a start's vectors in registers)");
    return FINROM_ERR_UNSUPPORTED;
  }
  L->S = a->S; L->d = a->d; L->m = a->m; L->maxls = a->maxls; L->gdim = a->G ? a->gdim : 0;
  L->ftol = a->ftol; L->gtol = a->gtol; L->gamma = a->gamma; L->maxiter = a->maxiter; L->maxfun = a->maxfun;
  L->lo = a->lo; L->hi = a->hi; L->x = a->x; L->f = a->f; L->g = a->g; L->xt = a->xt; L->work = a->work;
  L->status = a->status; L->nit = (long long*)a->nit; L->nfev = (long long*)a->nfev;
  L->fhist = a->fhist; L->fhist_rows = a->fhist ? a->fhist_rows : 0; L->G = a->G;
  L->k1_ptr = a->k1_ptr; L->k1_idx = a->k1_idx; L->k1_val = a->k1_val;
  return 0;
}
extern "C" {
int finrom_lbfgs_begin(const finrom_lbfgs_state* a, void* stream) {
  LbfgsDev L;
  if (int rc = lbfgs_dev(a, &L, "lbfgs_begin")) return rc;
  CallGuard cg((hipStream_t)stream);
  return launch_lbfgs_begin(L, (hipStream_t)stream);
}
int finrom_lbfgs_propose(const finrom_lbfgs_state* a, void* stream) {
  LbfgsDev L;
  if (int rc = lbfgs_dev(a, &L, "lbfgs_propose")) return rc;
  CallGuard cg((hipStream_t)stream);
  return launch_lbfgs_propose(L, (hipStream_t)stream);
}
int finrom_lbfgs_accept(const finrom_lbfgs_state* a, const double* f_in, const double* g_in, const int32_t* info, void* stream) {
  LbfgsDev L;
  if (int rc = lbfgs_dev(a, &L, "lbfgs_accept")) return rc;
  if (!f_in || !g_in) { set_error(std::string("lbfgs_accept: null ") + (!f_in ? "f_in" : "g_in")); return FINROM_ERR_ARG; }
  CallGuard cg((hipStream_t)stream);
  return launch_lbfgs_accept(L, f_in, g_in, info, (hipStream_t)stream);
}

int finrom_sub(const double* a, const double* b, int64_t count, double* out, void* stream) {
  CallGuard cg((hipStream_t)stream);
  if (count < 0 || (count > 0 && (!a || !b || !out))) { set_error("sub: bad argument"); return FINROM_ERR_ARG; }
  return launch_sub(a, b, count, out, (hipStream_t)stream);
}

}  // extern "C"
