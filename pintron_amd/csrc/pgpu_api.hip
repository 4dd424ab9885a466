// Host side of libpintron_gpu.so: contexts, batched DP plans, C-ABI entry points.
// (C++ inside, extern "C" at the boundary; see include/pintron_gpu.h for the contract.)
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <time.h>
#include <new>
#include <mutex>
#include <vector>

#include "pgpu_internal.h"
#include "pgpu_index.h"

// Device scratch that outlives a plan: the batched host program creates and destroys a plan per
// round, and hipMalloc/hipFree (the latter synchronises the device) would dominate.  A context
// keeps one grow-only set of buffers per plan type; a plan borrows the set when it is free.
struct BufPool {
  static constexpr int SLOTS = PLAN_SLOTS;      // pgpu_index.h
  void* ptr[SLOTS] = {nullptr};
  size_t cap[SLOTS] = {0};
  bool busy = false;
  int sharers = 0;                // > 0: held by plans that use it one after the other (pgpu_pairing_plan_create_resident)
  const void* owner = nullptr;    // whose results the buffers hold right now
};

struct pgpu_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  char err[512] = {0};
  BufPool pools[2];          // 0: DP plans, 1: pairing plans
  bool timing = false;       // HIP events around every kernel group (bench / profiling)
  // the kernel groups of one DP plan are independent of each other: the ones outside the batch launch are
  // spread over four auxiliary streams so that a batch costs max(group) instead of sum(group) in latency
  static constexpr int NAUX = 4;
  hipStream_t aux[NAUX] = {nullptr};
  hipEvent_t ev_upload = nullptr;
  hipEvent_t ev_aux[NAUX] = {nullptr};
  // waiting: the calling thread must not burn a host core that other EST fibres could use (the
  // default HIP wait spins).  It naps and polls the event: measured on C3, naps of 50-200 us beat
  // a blocking-sync event by 5-7 % whole-program (the interrupt path costs more host time than
  // the naps cost latency).  PGPU_WAIT=<us> sets the nap, 0 = blocking-sync event, -1 = spin.
  hipEvent_t ev_done = nullptr;
  hipEvent_t ev_wait = nullptr;      // pgpu_ctx_wait (pairing / MEG stages)
  long wait_poll_us = 20;
  int poison = -1;           // PGPU_POISON=<0..255>: fill strings + workspace of every DP plan with that byte first
  // pinned staging for the device->host result copies (pageable copies block and spin inside HIP)
  void* pin[2] = {nullptr, nullptr};
  size_t pin_cap[2] = {0, 0};
  // timing events are recycled (a plan with the DP pool borrows them; create/destroy per group
  // and batch is measurable at a few hundred batches per second)
  std::vector<hipEvent_t> ev_pool;
};

static int wait_stream(pgpu_ctx* ctx, hipStream_t st) {
  if (hipEventRecord(ctx->ev_done, st) != hipSuccess) return -1;
  if (ctx->wait_poll_us != 0) {
    for (;;) {
      const hipError_t q = hipEventQuery(ctx->ev_done);
      if (q == hipSuccess) return 0;
      if (q != hipErrorNotReady) return -1;
      if (ctx->wait_poll_us > 0) { struct timespec ts = {0, ctx->wait_poll_us * 1000L}; nanosleep(&ts, nullptr); }
    }
  }
  return hipEventSynchronize(ctx->ev_done) == hipSuccess ? 0 : -1;
}

static void* pinned(pgpu_ctx* ctx, int slot, size_t bytes) {
  if (ctx->pin_cap[slot] < bytes) {
    if (ctx->pin[slot]) (void)hipHostFree(ctx->pin[slot]);
    ctx->pin[slot] = nullptr; ctx->pin_cap[slot] = 0;
    // never less than 2 MB: the first batches of a run grow from a few hundred jobs to thousands, and every
    // regrowth is a free (which waits for the device) and an allocation
    const size_t want = std::max<size_t>(bytes + bytes / 2 + 4096, (size_t)2 << 20);
    if (hipHostMalloc(&ctx->pin[slot], want, hipHostMallocDefault) != hipSuccess) return nullptr;
    pgpu_trace_alloc(slot ? "ctx pinned down" : "ctx pinned up", ctx->pin[slot], want);
    ctx->pin_cap[slot] = want;
  }
  return ctx->pin[slot];
}

extern "C" int pgpu_host_alloc(pgpu_ctx* ctx, size_t bytes, void** out) {
  if (!ctx || !out) return PGPU_EINVAL;
  *out = nullptr;
  if (pgpu_ctx_bind(ctx) != PGPU_OK) return PGPU_EDEVICE;
  if (hipHostMalloc(out, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) return pgpu_ctx_fail(ctx, PGPU_ENOMEM, "out of page-locked host memory");
  pgpu_trace_alloc("pgpu_host_alloc", *out, bytes);
  return PGPU_OK;
}
extern "C" int pgpu_host_free(pgpu_ctx* ctx, void* q) {
  if (!ctx) return PGPU_EINVAL;
  if (q && hipHostFree(q) != hipSuccess) return pgpu_ctx_fail(ctx, PGPU_EDEVICE, "hipHostFree failed");
  return PGPU_OK;
}

bool pgpu_ctx_pool_acquire(pgpu_ctx* ctx, int pool) {
  if (ctx->pools[pool].busy) return false;
  ctx->pools[pool].busy = true;
  return true;
}
void pgpu_ctx_pool_release(pgpu_ctx* ctx, int pool) { ctx->pools[pool].busy = false; ctx->pools[pool].owner = nullptr; }
// several plans, used strictly one after the other, on the same buffers
bool pgpu_ctx_pool_share(pgpu_ctx* ctx, int pool) {
  BufPool& p = ctx->pools[pool];
  if (p.busy && p.sharers == 0) return false;       // a plan holds it for itself
  p.busy = true; ++p.sharers;
  return true;
}
void pgpu_ctx_pool_unshare(pgpu_ctx* ctx, int pool, const void* who) {
  BufPool& p = ctx->pools[pool];
  if (p.owner == who) p.owner = nullptr;
  if (p.sharers > 0 && --p.sharers == 0) p.busy = false;
}
void pgpu_ctx_pool_set_owner(pgpu_ctx* ctx, int pool, const void* who) { ctx->pools[pool].owner = who; }
const void* pgpu_ctx_pool_owner(const pgpu_ctx* ctx, int pool) { return ctx->pools[pool].owner; }
// returns a buffer of at least `bytes` from the (acquired) pool, growing it when needed
void* pgpu_ctx_pool_get(pgpu_ctx* ctx, int pool, int slot, size_t bytes) {
  BufPool& p = ctx->pools[pool];
  if (slot < 0 || slot >= BufPool::SLOTS) return nullptr;
  if (bytes == 0) bytes = 16;
  if (p.cap[slot] < bytes) {
    if (p.ptr[slot]) (void)hipFree(p.ptr[slot]);
    p.ptr[slot] = nullptr; p.cap[slot] = 0;
    const size_t want = std::max<size_t>(bytes + bytes / 2 + 4096, pool == 0 ? (size_t)64 << 20 : 0);
    if (hipMalloc(&p.ptr[slot], want) != hipSuccess) {
      if (hipMalloc(&p.ptr[slot], bytes) != hipSuccess) return nullptr;
      p.cap[slot] = bytes;
    } else p.cap[slot] = want;
    pgpu_trace_alloc(pool ? "device pool 1" : "device pool 0", p.ptr[slot], p.cap[slot]);
  }
  return p.ptr[slot];
}
bool pgpu_ctx_timing(const pgpu_ctx* ctx) { return ctx->timing; }

extern "C" int pgpu_device_numa_node(pgpu_ctx* ctx) {
  if (!ctx) return -1;
  char bdf[64] = {0};
  if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf - 1, ctx->device) != hipSuccess) return -1;
  for (char* c = bdf; *c; ++c) if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');   // sysfs spells it in lower case
  char path[160];
  snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
  FILE* f = fopen(path, "r");
  if (!f) return -1;
  int node = -1;
  if (fscanf(f, "%d", &node) != 1) node = -1;
  fclose(f);
  return node;
}

extern "C" int pgpu_set_timing(pgpu_ctx* ctx, int enabled) {
  if (!ctx) return PGPU_EINVAL;
  ctx->timing = enabled != 0;
  return PGPU_OK;
}

static int set_err(pgpu_ctx* ctx, int code, const char* fmt, ...) {
  if (ctx) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
    va_end(ap);
  }
  return code;
}

#define HIP_TRY(ctx, call)                                                                  \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return set_err(ctx, e_ == hipErrorOutOfMemory ? PGPU_ENOMEM : PGPU_EDEVICE,           \
                     "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

hipStream_t pgpu_ctx_stream(pgpu_ctx* ctx) { return ctx->stream; }
hipError_t pgpu_ctx_wait(pgpu_ctx* ctx) {
  if (ctx->wait_poll_us <= 0) return hipStreamSynchronize(ctx->stream);
  hipError_t e = hipEventRecord(ctx->ev_wait, ctx->stream);
  if (e != hipSuccess) return e;
  // the kernels behind these waits run for milliseconds: naps five times the DP plans' (100 us by default)
  const struct timespec ts = {0, ctx->wait_poll_us * 5000L};
  for (;;) {
    e = hipEventQuery(ctx->ev_wait);
    if (e != hipErrorNotReady) return e;
    nanosleep(&ts, nullptr);
  }
}
int pgpu_ctx_bind(pgpu_ctx* ctx) {
  const hipError_t e = hipSetDevice(ctx->device);
  return e == hipSuccess ? PGPU_OK : set_err(ctx, PGPU_EDEVICE, "hipSetDevice(%d) failed: %s", ctx->device, hipGetErrorString(e));
}
int pgpu_ctx_fail(pgpu_ctx* ctx, int code, const char* msg) { return set_err(ctx, code, "%s", msg); }

extern "C" int pgpu_abi_version(void) { return 1; }

// ---- profiler ranges --------------------------------------------------------------------------------
#include <dlfcn.h>
namespace {
struct Roctx { int state = 0; int (*push)(const char*) = nullptr; int (*pop)() = nullptr; };   // state: 0 untried, 1 on, -1 off
Roctx g_roctx;
bool roctx_ready() {
  if (g_roctx.state) return g_roctx.state > 0;
  bool want = false;
  { const char* m = getenv("PGPU_MARKERS"); if (m) want = m[0] != '0'; else {
      const char* t = getenv("ROCP_TOOL_LIBRARIES"); const char* pl = getenv("LD_PRELOAD");
      want = (t && t[0]) || (pl && strstr(pl, "rocprofiler")); } }
  if (want) {
    void* so = nullptr;
    for (const char* n : { "librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so" })
      if ((so = dlopen(n, RTLD_NOW | RTLD_GLOBAL)) != nullptr) break;
    if (so) {
      *(void**)(&g_roctx.push) = dlsym(so, "roctxRangePushA");
      *(void**)(&g_roctx.pop) = dlsym(so, "roctxRangePop");
    }
  }
  g_roctx.state = (g_roctx.push && g_roctx.pop) ? 1 : -1;
  return g_roctx.state > 0;
}
}  // namespace
extern "C" void pgpu_range_push(const char* name) { if (roctx_ready()) g_roctx.push(name ? name : ""); }
extern "C" void pgpu_range_pop(void) { if (roctx_ready()) g_roctx.pop(); }

extern "C" const char* pgpu_build_info(void) {
  static char info[256];
  if (!info[0]) {
    const char* stamp = __DATE__ " " __TIME__ " " __VERSION__;
    unsigned long long h = 1469598103934665603ull;
    for (const char* c = stamp; *c; ++c) { h ^= (unsigned char)*c; h *= 1099511628211ull; }
    snprintf(info, sizeof info, "libpintron_gpu abi %d, gfx950, built %s %s, hip %d.%d.%d, stamp %016llx", pgpu_abi_version(), __DATE__,
             __TIME__, HIP_VERSION_MAJOR, HIP_VERSION_MINOR, HIP_VERSION_PATCH, h);
  }
  return info;
}

static bool aux_stream(pgpu_ctx* ctx, int i) {
  if (!ctx->aux[i] && hipStreamCreateWithFlags(&ctx->aux[i], hipStreamNonBlocking) != hipSuccess) { ctx->aux[i] = nullptr; return false; }
  if (!ctx->ev_aux[i] && hipEventCreateWithFlags(&ctx->ev_aux[i], hipEventDisableTiming) != hipSuccess) { ctx->ev_aux[i] = nullptr; return false; }
  return true;
}

// One timing event per device, recorded once when the first context of the process comes up: the start of every
// kernel group is reported relative to it (pgpu_group_info.t0_ms), so that a caller with several contexts
// (the host program's service threads) can lay the launches of all of them on ONE time line and tell the time
// the device was busy from the sum of the launches' durations.
static hipEvent_t g_base_event[64];
static std::mutex g_base_mu;
static hipEvent_t base_event(int device, hipStream_t st) {
  if (device < 0 || device >= 64) return nullptr;
  std::lock_guard<std::mutex> lk(g_base_mu);
  if (!g_base_event[device]) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) == hipSuccess && hipEventRecord(e, st) == hipSuccess && hipEventSynchronize(e) == hipSuccess) g_base_event[device] = e;
    else if (e) hipEventDestroy(e);
  }
  return g_base_event[device];
}

extern "C" int pgpu_init(int device, pgpu_ctx** out) {
  if (!out) return PGPU_EINVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return PGPU_EDEVICE;
  if (device < 0 || device >= n) return PGPU_EINVAL;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return PGPU_EDEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return PGPU_EDEVICE;   // gfx950 code objects only
  if (hipSetDevice(device) != hipSuccess) return PGPU_EDEVICE;
  pgpu_ctx* ctx = new (std::nothrow) pgpu_ctx();
  if (!ctx) return PGPU_ENOMEM;
  ctx->device = device;
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return PGPU_EDEVICE;
  }
  // the auxiliary streams are made when a plan first forks onto them (aux_stream): a stream costs ~5 ms and
  // ~17 MB of host memory in the runtime, and the one-launch batch forks only for LCF jobs with an N
  if (hipEventCreateWithFlags(&ctx->ev_upload, hipEventDisableTiming) != hipSuccess) { delete ctx; return PGPU_EDEVICE; }
  if (hipEventCreateWithFlags(&ctx->ev_done, hipEventDisableTiming | hipEventBlockingSync) != hipSuccess) { delete ctx; return PGPU_EDEVICE; }
  if (hipEventCreateWithFlags(&ctx->ev_wait, hipEventDisableTiming) != hipSuccess) { delete ctx; return PGPU_EDEVICE; }
  { const char* f = getenv("PGPU_WAIT"); if (f) ctx->wait_poll_us = atol(f); }
  { const char* f = getenv("PGPU_POISON"); if (f && f[0]) ctx->poison = atoi(f) & 255; }
  base_event(device, ctx->stream);
  *out = ctx;
  return PGPU_OK;
}

extern "C" int pgpu_destroy(pgpu_ctx* ctx) {
  if (!ctx) return PGPU_EINVAL;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  for (auto& pl : ctx->pools) for (auto& q : pl.ptr) if (q) hipFree(q);
  for (auto& a : ctx->aux) if (a) { hipStreamSynchronize(a); hipStreamDestroy(a); }
  if (ctx->ev_upload) hipEventDestroy(ctx->ev_upload);
  if (ctx->ev_done) hipEventDestroy(ctx->ev_done);
  if (ctx->ev_wait) hipEventDestroy(ctx->ev_wait);
  for (auto& e : ctx->ev_aux) if (e) hipEventDestroy(e);
  for (auto& e : ctx->ev_pool) if (e) hipEventDestroy(e);
  for (auto& q : ctx->pin) if (q) hipHostFree(q);
  hipStreamDestroy(ctx->stream);
  delete ctx;
  return PGPU_OK;
}

extern "C" const char* pgpu_last_error(const pgpu_ctx* ctx) { return ctx ? ctx->err : "null context"; }

// ---------------------------------------------------------------------------------------------
// DP plans
// ---------------------------------------------------------------------------------------------
namespace {

uint32_t row_class(uint32_t rows) {         // smallest R in {1,2,4,...,64} with 64*R >= rows
  if (rows > 4096u) return ROW_CLASS_STRIPS;  // beyond that: strips of 4096 rows on the R = 64 kernels
  uint32_t R = 1;
  while (64u * R < rows) R <<= 1;
  return R;
}

// A route = the kernel that serves a job, as the statistics name it: a family, split by row class where different
// kernels take the classes.  The device job table is sorted by family and row class (descending), so the jobs of
// a route are one slice of it; the routes are listed in that order.
enum DpRoute : uint8_t {
  RT_ALIGN_STRIPS, RT_ALIGN_COOP, RT_ALIGN_WAVE, RT_GAP_SLOW, RT_GAP, RT_ED, RT_KBAND, RT_LCF,
  RT_BORDERS_SLOW, RT_BORDERS_COOP, RT_BORDERS_WAVE, RT_AFFIX_STRIPS, RT_AFFIX_COOP, RT_AFFIX_WAVE,
  RT_LCFSA, RT_LCFW, RT_ALIGNB,
  RT_BATCH,              // the batch launch itself (no job is classified to it)
  RT_COUNT
};

// place of a route's jobs in the batch launch
enum BatchPlace { OUTSIDE, SEGMENT, ROLE_BORDERS, ROLE_AFFIX, ROLE_ALIGN };

// traceback workspace of one job (la rows, lb columns, row class R) as the route's kernel lays it out
using WsBytes = size_t (*)(uint32_t la, uint32_t lb, uint32_t R);
size_t ws_align_wave(uint32_t, uint32_t lb, uint32_t) { return ((size_t)lb + 64) * 64; }               // [step][64 lanes], 1 B
size_t ws_align_coop(uint32_t, uint32_t lb, uint32_t R) { return ((size_t)lb + 256) * 256 * align_coop_entry_bytes(R); }   // [step][256 lanes] (the band's words fit in there)
size_t ws_align_strips(uint32_t la, uint32_t lb, uint32_t R) {      // two boundary rows, then the directions of every strip
  return 2 * strip_bnd_bytes(lb) + (size_t)((la + 4095u) / 4096u) * ((size_t)lb + 64) * 64 * align_entry_bytes(R);
}
size_t ws_gap(uint32_t, uint32_t lb, uint32_t R) { return ((size_t)lb + 64) * 64 * gap_entry_bytes(R); }
size_t ws_gap_slow(uint32_t la, uint32_t lb, uint32_t) { return (size_t)9 * ((size_t)la + 1) * 4 + ((size_t)la + 1) * ((size_t)lb + 1); }   // 9 rolling diagonals + 1 B per cell
size_t ws_borders_slow(uint32_t la, uint32_t, uint32_t) { return (size_t)7 * ((size_t)la + 1) * 4; }   // 3 diagonals + 4 row-minima arrays
size_t ws_affix_strips(uint32_t, uint32_t lb, uint32_t) { return 2 * strip_bnd_bytes(lb); }            // two boundary rows
size_t ws_ed_strips(uint32_t la, uint32_t lb, uint32_t R) { return R == ROW_CLASS_STRIPS ? 2 * strip_bnd_bytes(std::max(la, lb)) : 0; }   // (ED, KBAND: the longer string is on the columns)

// algorithmic HBM bytes of one job: operands once; 1 B/cell of directions for ALIGN, 3 B/cell
// for GAP, read back, and two strings; 8 B per row when row minima are produced
using AlgoBytes = uint64_t (*)(uint64_t la, uint64_t lb, uint64_t p2);
uint64_t bytes_operands(uint64_t la, uint64_t lb, uint64_t) { return la + lb; }
uint64_t bytes_align(uint64_t la, uint64_t lb, uint64_t) { return la + lb + la * lb + 3 * (la + lb); }
uint64_t bytes_gap(uint64_t la, uint64_t lb, uint64_t) { return la + lb + 3 * la * lb + 3 * (la + lb); }
// (BORDERS touches the first and the last t_win characters of t only)
uint64_t bytes_borders(uint64_t la, uint64_t lb, uint64_t p2) { return la + std::min(lb, 2 * std::min(la + p2, lb)) + 2 * 8 * la; }
// suffix-array search: s2, and per lane about eight table probes, a few suffix-array / sequence probes of the
// bisection and the range minima, and the characters of one direct comparison
uint64_t bytes_lcfsa(uint64_t, uint64_t lb, uint64_t) { return lb + 64u * 96u; }

struct RouteInfo {
  const char* name;        // in the statistics (bench.py maps these to kernel names)
  int kind;                // pgpu_dp_kind it accounts to
  int family;              // KernelFamily: sort key of the job table, body of a batch segment
  WsBytes ws_bytes;        // nullptr: no workspace
  bool strings;            // two alignment strings of la + lb + 1 bytes each
  // cells = what the kernels compute (the roofline's numerator): this many per cell of the reference's loop bounds.
  // The suffix-array search computes none of the 46 x |prefix| cells those bounds give: left out rather than credited
  uint32_t cell_factor;
  AlgoBytes algo_bytes;
  BatchPlace place;
  int seg_pos;             // SEGMENT: position among the batch launch's segments (long-running families first)
  uint32_t big_from;       // SEGMENT: jobs of this row class and above keep a launch of their own (0: none do)
  // what stays outside the batch launch: launch order (heaviest first; by_rows: + the longest pattern), auxiliary
  // stream (-1: the main stream), launcher.  launch == nullptr: nothing of the route is ever left outside
  long weight; bool by_rows; int lane; DpLauncher launch;
  bool keyed;              // LCF: the kernel leaves one 64-bit key per job; at most 65535 jobs per launch (grid.y)
};

// Streams: HIP spreads its streams over four hardware queues, and what shares a queue runs one after the other:
// four lanes (one per queue), the routes dealt out so that the four sums of typical durations come out even.
constexpr RouteInfo ROUTES[] = {
  // name                      kind             family     workspace        strs cells bytes           place        seg big  weight rows lane launcher            keyed
  {"lev_wave<ALIGN,strips>",  PGPU_DP_ALIGN,   KF_ALIGN,   ws_align_strips, true,  1, bytes_align,    OUTSIDE,      0,  0,  5000, false,  2, launch_align_big,    false},
  {"align_coop",              PGPU_DP_ALIGN,   KF_ALIGN,   ws_align_coop,   true,  1, bytes_align,    ROLE_ALIGN,   0,  0,     0, false,  0, nullptr,             false},
  {"lev_wave<ALIGN>",         PGPU_DP_ALIGN,   KF_ALIGN,   ws_align_wave,   true,  1, bytes_align,    SEGMENT,      1,  0,     0, false,  0, nullptr,             false},
  {"gap_slow",                PGPU_DP_GAP,     KF_GAP,     ws_gap_slow,     true,  3, bytes_gap,      OUTSIDE,      0,  0,  4000, false,  3, launch_gap_slow,     false},
  {"gap_wave",                PGPU_DP_GAP,     KF_GAP,     ws_gap,          true,  3, bytes_gap,      SEGMENT,      2,  8,  4000, false,  3, launch_gap_big,      false},
  {"lev_wave<ED>",            PGPU_DP_ED,      KF_ED,      ws_ed_strips,    false, 1, bytes_operands, SEGMENT,      8, 32,  1000, false,  1, launch_ed_big,       false},
  {"lev_wave<KBAND>",         PGPU_DP_KBAND,   KF_KBAND,   ws_ed_strips,    false, 1, bytes_operands, SEGMENT,      3, 32,  2000, false,  2, launch_kband_big,    false},
  {"lcf",                     PGPU_DP_LCF,     KF_LCF,     nullptr,         false, 1, bytes_operands, OUTSIDE,      0,  0,  3000, false,  3, launch_lcf,          true},
  {"borders_slow",            PGPU_DP_BORDERS, KF_BORDERS, ws_borders_slow, false, 2, bytes_borders,  OUTSIDE,      0,  0, 10000, true,   1, launch_borders_slow, false},
  {"borders_coop",            PGPU_DP_BORDERS, KF_BORDERS, nullptr,         false, 2, bytes_borders,  ROLE_BORDERS, 0,  0, 10000, true,   1, launch_borders_coop, false},   // outside when its row minima exceed the batch's LDS
  {"lev_wave<BORDERS,R=1>",   PGPU_DP_BORDERS, KF_BORDERS, nullptr,         false, 2, bytes_borders,  SEGMENT,      4,  0,     0, false,  0, nullptr,             false},
  {"lev_wave<AFFIX,strips>",  PGPU_DP_AFFIX,   KF_AFFIX,   ws_affix_strips, false, 1, bytes_operands, OUTSIDE,      0,  0, 10000, true,   0, launch_affix_strips, false},
  {"affix_coop",              PGPU_DP_AFFIX,   KF_AFFIX,   nullptr,         false, 1, bytes_operands, ROLE_AFFIX,   0,  0,     0, false,  0, nullptr,             false},
  {"lev_wave<AFFIX,R=1>",     PGPU_DP_AFFIX,   KF_AFFIX,   nullptr,         false, 1, bytes_operands, SEGMENT,      5,  0,     0, false,  0, nullptr,             false},
  {"lcf_sa",                  PGPU_DP_LCF,     KF_LCFSA,   nullptr,         false, 0, bytes_lcfsa,    SEGMENT,      6,  0,     0, false,  0, nullptr,             false},
  {"lcf_small",               PGPU_DP_LCF,     KF_LCFW,    nullptr,         false, 1, bytes_operands, SEGMENT,      7,  0,     0, false,  0, nullptr,             false},
  {"align_band",              PGPU_DP_ALIGN,   KF_ALIGNB,  ws_align_coop,   true,  1, bytes_align,    SEGMENT,      0,  0,     0, false,  0, nullptr,             false},
  // the batch launch: first of all, on the main stream, where the upload already is
  {"dp_batch",                PGPU_DP_ALIGN,   KF_COUNT,   nullptr,         false, 0, nullptr,        OUTSIDE,      0,  0, 20000, false, -1, nullptr,             false},
};
static_assert(sizeof ROUTES / sizeof ROUTES[0] == RT_COUNT, "one entry per route, in the enum's order");
constexpr bool routes_consistent() {
  unsigned seen = 0;
  for (const RouteInfo& ri : ROUTES) {
    if (ri.lane >= pgpu_ctx::NAUX) return false;
    if (ri.big_from && (ri.place != SEGMENT || !ri.launch)) return false;      // a big part is what a segment leaves outside
    if (ri.place != SEGMENT) continue;
    if (ri.seg_pos >= MAX_WAVE_SEGS || (seen & (1u << ri.seg_pos))) return false;   // one segment each
    seen |= 1u << ri.seg_pos;
  }
  return true;
}
static_assert(routes_consistent(), "routing table");

// a slice of the sorted device job table with its share of the accounting
struct Slice { size_t first = 0, count = 0; uint64_t cells = 0, algo_bytes = 0; };

// one entry of the statistics = one route's jobs of a plan (LCF: at most 65535 of them), or the batch launch
struct Group {
  DpRoute route;
  Slice own;                   // what has a launch of its own; count 0: everything of the route runs in the batch launch
  uint32_t max_chunks = 0, max_l2 = 0;    // LCF: most 256-diagonal chunks, longest s2
  uint32_t max_rows = 0;       // largest a_len of the route's jobs (LDS of the one-job-per-workgroup BORDERS kernel)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float ms = 0.f;
  float t0_ms = -1.f;          // start of the last launch on the device's time line (base_event), -1: unknown
};

// the batch launch of a plan
struct BatchPlan {
  BatchDesc desc;
  uint32_t bc_max_rows;        // longest pattern of its BORDERS role
  int ab_start, ab_count;      // its banded ALIGN jobs (the follow-up launch looks at them)
};

// a job between classification and the upload image; operands are addressed by OFFSET until the arena's place is known
struct Keyed { DevJob j; uint64_t a_off, b_off; bool ag, bg; DpRoute route; uint32_t R; uint64_t size; };

}  // namespace

struct pgpu_dp_plan {
  size_t n_jobs = 0;
  std::vector<Group> groups;
  std::vector<pgpu_dp_result> prefill;       // status for jobs that never reach the device
  DevJob* d_jobs = nullptr;
  DevResult* d_results = nullptr;
  uint8_t* d_arena = nullptr;
  uint8_t* d_ws = nullptr;
  uint8_t* d_strs = nullptr;
  unsigned long long* d_keys = nullptr;
  size_t n_dev_jobs = 0, ws_bytes = 0, strs_bytes = 0, n_keys = 0;
  uint64_t cells[PGPU_DP_NKINDS] = {0}, algo_bytes[PGPU_DP_NKINDS] = {0};
  double ms[PGPU_DP_NKINDS] = {0};
  uint64_t launches[PGPU_DP_NKINDS] = {0};
  bool launched = false, synced = false;
  bool pooled = false;                      // device + pinned buffers and events borrowed from the context
  pgpu_ctx* owner = nullptr;
  // One device allocation: [arena | job table | LCF keys | results | strings | traceback workspace].
  // The first four are filled by ONE host->device copy from the pinned image `h_up`; results and
  // strings come back in ONE device->host copy into `h_down`, enqueued by launch after the kernels.
  uint8_t* d_base = nullptr;
  uint8_t* h_up = nullptr; uint8_t* h_down = nullptr;
  size_t up_bytes = 0, off_results = 0, down_bytes = 0;
  BatchPlan batch{};           // (batch.desc.ix: the index view the suffix-array LCF jobs search, one index per plan)
  // LCF: the kernel leaves one 64-bit key per job directly in front of the results; they come back in the
  // same copy and sync turns them into results (lcf_out[k] = caller index of the job of key k)
  std::vector<uint32_t> lcf_out;
  size_t off_keys = 0;
  bool lcf_decoded = false;
};

static void plan_free(pgpu_dp_plan* p) {
  if (!p) return;
  if (p->pooled) pgpu_ctx_pool_release(p->owner, 0);
  else {
    for (auto& g : p->groups) {
      if (g.ev0) hipEventDestroy(g.ev0);
      if (g.ev1) hipEventDestroy(g.ev1);
    }
    if (p->d_base) hipFree(p->d_base);
    if (p->h_up) hipHostFree(p->h_up);
    if (p->h_down) hipHostFree(p->h_down);
  }
  delete p;
}

extern "C" int pgpu_dp_plan_create(pgpu_ctx* ctx, const pgpu_index* idx, const pgpu_dp_job* jobs,
                                   size_t n_jobs, const char* arena, size_t arena_len,
                                   pgpu_dp_plan** out) {
  const pgpu_dp_part one = { jobs, n_jobs, arena, arena_len };
  return pgpu_dp_plan_create_parts(ctx, idx, &one, 1, out);
}

// Route, row class and size of a job whose operands lie inside their spaces (k.j holds the caller's values).
// `arena`: the caller's (LCF looks at the characters of s2).  Not PGPU_OK: the status the job gets without reaching the device
static int classify(const pgpu_dp_job& in, const char* arena, bool ag, bool bg, const LcfIndexView& lcf, Keyed& k) {
  const uint32_t la = in.a_len, lb = in.b_len;
  k.size = (uint64_t)la * lb;
  switch (in.kind) {
    case PGPU_DP_ALIGN:
      if (la > PGPU_MAX_ROWS_LEV || lb > PGPU_MAX_COLS) return PGPU_ERANGE;
      k.R = row_class(la);
      // exon against its stretch of the genomic sequence: the alignment hugs the diagonal.  Above 64 rows, lengths
      // within the band's half-width: inside the band on ONE wave among the wave-per-job jobs (four to a workgroup
      // instead of a workgroup each); the rare job the band cannot settle is finished by the follow-up launch
      if (la > 64u && la <= 4096u && (la > lb ? la - lb : lb - la) <= ALIGN_BAND_HALF) k.route = RT_ALIGNB;
      else k.route = k.R == 1 ? RT_ALIGN_WAVE : (k.R == ROW_CLASS_STRIPS ? RT_ALIGN_STRIPS : RT_ALIGN_COOP);
      return PGPU_OK;
    case PGPU_DP_GAP:
      if (lb > PGPU_MAX_GAP_SIDE || la > PGPU_MAX_GAP_SIDE || ((uint64_t)la + 1) * ((uint64_t)lb + 1) > PGPU_MAX_GAP_CELLS) return PGPU_ERANGE;
      // beyond 2048 rows: the anti-diagonal kernel over HBM (slow, but the reference computes these too)
      k.R = la > PGPU_MAX_ROWS_GAP ? ROW_CLASS_STRIPS : row_class(la);
      k.route = k.R == ROW_CLASS_STRIPS ? RT_GAP_SLOW : RT_GAP;
      return PGPU_OK;
    case PGPU_DP_ED:
      if (std::min(la, lb) > PGPU_MAX_ROWS_LEV || std::max(la, lb) > PGPU_MAX_COLS) return PGPU_ERANGE;
      k.R = row_class(std::min(la, lb)); k.route = RT_ED;
      return PGPU_OK;
    case PGPU_DP_KBAND: {
      const uint32_t n = std::max(la, lb), m = std::min(la, lb), ub = in.p0;
      if (n > PGPU_MAX_COLS || m > PGPU_MAX_ROWS_LEV) return PGPU_ERANGE;
      k.R = row_class(m); k.route = RT_KBAND;
      if (2ull * ub + 1 < n) k.size = (uint64_t)m * (2ull * ub + 1);
      return PGPU_OK;
    }
    case PGPU_DP_LCF:
      if (lb > 65535u || la >= (1u << 28)) return PGPU_ERANGE;
      k.R = 0; k.route = RT_LCF;
      // the small-exon search's question -- a prefix of the genomic sequence against a few dozen EST
      // characters -- is answered from the suffix array when exact matching is all there is to it: both
      // strings upper-case ACGT (no N wildcard can fire) and s2 short enough for one lane per start
      // ... or with ONE N in s2 (an EST with a stray N): the four strings with A, C, G, T in its place are searched
      // by the same wave (lcfsa_wave_body; job.p0 = the N's place + 1).  More Ns, or anything else: the DP kernel
      if (lcf.focc && lcf.rmq && ag && !bg && in.a_off == 0 && la <= lcf.first_bad && lb <= 64u) {
        const unsigned char* b = (const unsigned char*)arena + in.b_off;
        bool acgt = true;
        uint32_t n_wild = 0, wild_at = 0;
        for (uint32_t q = 0; q < lb && acgt; ++q) {
          if (b[q] == 'N' || b[q] == 'n') { ++n_wild; wild_at = q; }
          else acgt = b[q] == 'A' || b[q] == 'C' || b[q] == 'G' || b[q] == 'T';
        }
        if (acgt && n_wild <= 1u) { k.route = RT_LCFSA; k.j.p0 = n_wild ? wild_at + 1u : 0u; }
      }
      // two short strings: one wave (a lane per diagonal) instead of a workgroup and an atomic per job
      if (k.route == RT_LCF && (uint64_t)la * lb <= 16384u && la + lb <= 4096u) k.route = RT_LCFW;
      return PGPU_OK;
    case PGPU_DP_BORDERS: {
      // only the first and the last t_win = min(len_p + max_errs, len_t) characters of t are swept
      // (src/refine.c:117-121): t may be a whole intron of any length the index can hold
      const uint64_t t_win = std::min<uint64_t>((uint64_t)la + in.p2, lb);
      if (la > PGPU_MAX_ROWS_LEV || t_win > PGPU_MAX_COLS) return PGPU_ERANGE;
      if (in.p0 > in.p1 || in.p1 > la) return PGPU_EINVAL;
      // cells as the reference bounds them: two matrices of len_p x t_win; the gap of check_gap_errors is a whole
      // intron, the window a few dozen columns
      k.R = row_class(la); k.size = (uint64_t)la * t_win;
      k.route = k.R == 1 ? RT_BORDERS_WAVE : (k.R == ROW_CLASS_STRIPS ? RT_BORDERS_SLOW : RT_BORDERS_COOP);
      return PGPU_OK;
    }
    case PGPU_DP_AFFIX:
      if (la > PGPU_MAX_ROWS_LEV || lb > PGPU_MAX_COLS) return PGPU_ERANGE;
      k.R = row_class(la);
      k.route = k.R == 1 ? RT_AFFIX_WAVE : (k.R == ROW_CLASS_STRIPS ? RT_AFFIX_STRIPS : RT_AFFIX_COOP);
      return PGPU_OK;
    default: return PGPU_EINVAL;
  }
}

// pass 1: validate and classify every job of every part; prefill[i] = the status of caller job i (PGPU_OK: it is in
// the returned table).  Jobs of part q address part q's arena; the arenas are laid out one after the other.
static std::vector<Keyed> classify_jobs(const pgpu_dp_part* parts, size_t n_parts, size_t n_jobs, const LcfIndexView& lcf,
                                        bool has_genomic, size_t gen_len, std::vector<pgpu_dp_result>& prefill) {
  std::vector<Keyed> v;
  v.reserve(n_jobs);
  prefill.assign(n_jobs, pgpu_dp_result{});
  size_t i = 0, part_base = 0;
  for (size_t q = 0; q < n_parts; part_base += parts[q].arena_len, ++q)
    for (size_t w = 0; w < parts[q].n_jobs; ++w, ++i) {
      const pgpu_dp_job& in = parts[q].jobs[w];
      const size_t own_arena = parts[q].arena_len;
      prefill[i].status = PGPU_EINVAL;
      if (in.kind >= PGPU_DP_NKINDS) continue;
      const bool ag = in.flags & PGPU_JOB_A_GENOMIC, bg = in.flags & PGPU_JOB_B_GENOMIC;
      if ((ag || bg) && !has_genomic) continue;
      const size_t a_space = ag ? gen_len : own_arena, b_space = bg ? gen_len : own_arena;
      if (in.a_off > a_space || in.a_len > a_space - in.a_off) continue;
      if (in.b_off > b_space || in.b_len > b_space - in.b_off) continue;
      Keyed k{};
      k.a_off = in.a_off + (ag ? 0 : part_base); k.b_off = in.b_off + (bg ? 0 : part_base); k.ag = ag; k.bg = bg;
      k.j.la = in.a_len; k.j.lb = in.b_len;
      k.j.p0 = in.p0; k.j.p1 = in.p1; k.j.p2 = in.p2; k.j.tail = in.tail;
      k.j.out_idx = (uint32_t)i;
      prefill[i].status = classify(in, parts[q].arena, ag, bg, lcf, k);
      if (prefill[i].status != PGPU_OK) continue;
      k.j.r_class = k.R;
      v.push_back(k);
    }
  return v;
}

// pass 2: the order of the device job table: family, row class, then largest first (long jobs start early; waves of
// a workgroup and threads of a traceback wave get similar sizes).  A counting sort does it in three passes: 13-bit
// key = family, row class (descending) and the size reduced to its binary order of magnitude (descending); jobs
// with the same key keep the caller's order.
static void sort_jobs(std::vector<Keyed>& v) {
  auto key_of = [](const Keyed& k) -> uint32_t {
    uint32_t rcls = 0;
    while ((1u << rcls) < k.R) ++rcls;                                  // R = 0,1,2,4,...,128 -> 0..7
    const uint32_t mag = 63u - (uint32_t)__builtin_clzll(k.size | 1ull);  // floor(log2(size)), 0..63
    return ((uint32_t)ROUTES[k.route].family << 10) | ((7u - rcls) << 6) | (63u - mag);   // long jobs first
  };
  constexpr uint32_t NKEYS = (uint32_t)KF_COUNT << 10;
  std::vector<uint32_t> start(NKEYS + 1, 0);
  std::vector<uint32_t> kk(v.size());
  for (size_t q = 0; q < v.size(); ++q) { kk[q] = key_of(v[q]); ++start[kk[q] + 1]; }
  for (uint32_t c = 0; c < NKEYS; ++c) start[c + 1] += start[c];
  std::vector<Keyed> sorted;
  sorted.resize(v.size());
  for (size_t q = 0; q < v.size(); ++q) sorted[start[kk[q]]++] = v[q];
  v.swap(sorted);
}

// pass 3: workspaces, string slots and LCF keys (lcf_out[k] = caller index of the job of key k) in table order
struct DpSpace { size_t ws = 0, strs = 0; };
static DpSpace assign_workspace(std::vector<Keyed>& v, std::vector<uint32_t>& lcf_out) {
  DpSpace sp;
  for (auto& k : v) {
    const RouteInfo& ri = ROUTES[k.route];
    const size_t wb = ri.ws_bytes ? ri.ws_bytes(k.j.la, k.j.lb, k.R) : 0;
    if (wb) { k.j.ws_off = sp.ws; sp.ws += wb; }
    if (ri.strings) { k.j.str_off = sp.strs; sp.strs += 2 * ((size_t)k.j.la + k.j.lb + 1); }
    if (ri.keyed) lcf_out.push_back(k.j.out_idx);
    sp.ws = (sp.ws + 15) & ~(size_t)15;
  }
  return sp;
}

// pass 4: one group per route present (the jobs of a route are adjacent).  batched[g] = what of group g runs inside
// the batch launch: of a SEGMENT route all but the leading jobs of the large row classes, of a role route everything
// -- unless the largest BORDERS pattern needs more LDS than the roles may share.  cells / algo_bytes: per pgpu_dp_kind
static void form_groups(const std::vector<Keyed>& v, std::vector<Group>& groups, std::vector<Slice>& batched,
                        uint64_t* cells, uint64_t* algo_bytes) {
  for (size_t i = 0, j; i < v.size(); i = j) {
    const RouteInfo& ri = ROUTES[v[i].route];
    Group g{};
    g.route = v[i].route;
    Slice big, rest;
    for (j = i; j < v.size() && v[j].route == g.route && !(ri.keyed && j - i == 65535); ++j) {
      const Keyed& k = v[j];
      Slice& s = ri.big_from && k.R >= ri.big_from ? big : rest;
      ++s.count; s.cells += ri.cell_factor * k.size; s.algo_bytes += ri.algo_bytes(k.j.la, k.j.lb, k.j.p2);
      g.max_rows = std::max(g.max_rows, k.j.la);
      if (ri.keyed) {
        g.max_chunks = std::max(g.max_chunks, (uint32_t)(((uint64_t)k.j.la + k.j.lb + 254) / 256));   // ceil((la+lb-1)/256) diagonals
        g.max_l2 = std::max(g.max_l2, k.j.lb);
      }
    }
    big.first = i; rest.first = i + big.count;
    cells[ri.kind] += big.cells + rest.cells; algo_bytes[ri.kind] += big.algo_bytes + rest.algo_bytes;
    const bool in_batch = ri.place == ROLE_BORDERS ? dp_batch_lds_bytes(true, 1, g.max_rows, 1, 1) <= DP_BATCH_MAX_LDS : ri.place != OUTSIDE;
    g.own = in_batch ? big : rest;      // (only SEGMENT routes have a big part, and they are always in the batch)
    groups.push_back(g);
    batched.push_back(in_batch ? rest : Slice{});
  }
}

// pass 5: the batch launch from what the groups hand it; when there is one, its group is appended (the entry of the
// statistics that carries its timing and accounting)
static void form_batch(std::vector<Group>& groups, const std::vector<Slice>& batched, BatchPlan& b) {
  Group m{};
  m.route = RT_BATCH;
  const Slice* seg[MAX_WAVE_SEGS] = {nullptr};
  int seg_family[MAX_WAVE_SEGS] = {0};
  BatchDesc& d = b.desc;
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    const Slice& s = batched[gi];
    if (!s.count) continue;
    const RouteInfo& ri = ROUTES[groups[gi].route];
    switch (ri.place) {
      case SEGMENT:      seg[ri.seg_pos] = &s; seg_family[ri.seg_pos] = ri.family; break;
      case ROLE_BORDERS: d.bc_start = (int)s.first; d.bc_count = (int)s.count; b.bc_max_rows = groups[gi].max_rows; break;
      case ROLE_AFFIX:   d.ac_start = (int)s.first; d.ac_count = (int)s.count; break;
      case ROLE_ALIGN:   d.lc_start = (int)s.first; d.lc_count = (int)s.count; break;
      case OUTSIDE:      break;
    }
    if (groups[gi].route == RT_ALIGNB) { b.ab_start = (int)s.first; b.ab_count = (int)s.count; }
    m.own.count += s.count; m.own.cells += s.cells; m.own.algo_bytes += s.algo_bytes;
  }
  int waves = 0;
  for (int q = 0; q < MAX_WAVE_SEGS; ++q) {
    if (!seg[q]) continue;
    d.segs.family[d.segs.n] = seg_family[q]; d.segs.start[d.segs.n] = (int)seg[q]->first; d.segs.count[d.segs.n] = (int)seg[q]->count;
    ++d.segs.n;
    waves += (int)seg[q]->count;
  }
  d.wave_blocks = (waves + 3) / 4;
  if (m.own.count) groups.push_back(m);
}

// events of the groups (timing only), the one device allocation, the pinned images and the upload: the only part of
// plan creation that touches the context and HIP.  On failure the caller frees the plan
static int plan_upload(pgpu_ctx* ctx, pgpu_dp_plan* p, const pgpu_dp_part* parts, size_t n_parts, size_t arena_len,
                       const std::vector<Keyed>& v, const uint8_t* d_gen) {
  if (ctx->timing) {
    const size_t need = 2 * p->groups.size();
    if (p->pooled) {
      while (ctx->ev_pool.size() < need) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return set_err(ctx, PGPU_EDEVICE, "hipEventCreate failed");
        ctx->ev_pool.push_back(e);
      }
      for (size_t g = 0; g < p->groups.size(); ++g) { p->groups[g].ev0 = ctx->ev_pool[2 * g]; p->groups[g].ev1 = ctx->ev_pool[2 * g + 1]; }
    } else {
      for (auto& g : p->groups)
        if (hipEventCreate(&g.ev0) != hipSuccess || hipEventCreate(&g.ev1) != hipSuccess) return set_err(ctx, PGPU_EDEVICE, "hipEventCreate failed");
    }
  }

  // one device allocation, one pinned upload image, one pinned download image
  auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t n_jobs = p->n_jobs, strs = p->strs_bytes;
  const size_t off_arena = 0;
  const size_t off_jobs = up256(arena_len + 16);
  const size_t off_keys = up256(off_jobs + std::max<size_t>(v.size(), 1) * sizeof(DevJob));
  const size_t off_results = up256(off_keys + (p->n_keys + 1) * sizeof(unsigned long long));
  const size_t off_strs = off_results + std::max<size_t>(n_jobs, 1) * sizeof(DevResult);   // directly behind the results
  const size_t off_ws = up256(off_strs + strs + 16);
  const size_t total = off_ws + p->ws_bytes + 16;
  p->up_bytes = off_strs;                      // arena .. results (prefilled)
  p->off_results = off_results;
  p->off_keys = off_keys;
  p->down_bytes = (off_strs - off_keys) + strs;           // keys (+ padding), results, strings
  if (p->pooled) {
    p->d_base = (uint8_t*)pgpu_ctx_pool_get(ctx, 0, 0, total);
    p->h_up = (uint8_t*)pinned(ctx, 0, p->up_bytes);
    p->h_down = (uint8_t*)pinned(ctx, 1, p->down_bytes + 16);
  } else {
    void* q = nullptr;
    if (hipMalloc(&q, total) == hipSuccess) p->d_base = (uint8_t*)q;
    if (hipHostMalloc(&q, p->up_bytes, hipHostMallocDefault) == hipSuccess) p->h_up = (uint8_t*)q;
    if (hipHostMalloc(&q, p->down_bytes + 16, hipHostMallocDefault) == hipSuccess) p->h_down = (uint8_t*)q;
  }
  if (!p->d_base || !p->h_up || !p->h_down)
    return set_err(ctx, PGPU_ENOMEM, "batch buffers (%zu B device, %zu B pinned) could not be allocated", total, p->up_bytes + p->down_bytes);
  p->d_arena = p->d_base + off_arena;
  p->d_jobs = (DevJob*)(p->d_base + off_jobs);
  p->d_keys = (unsigned long long*)(p->d_base + off_keys);
  p->d_results = (DevResult*)(p->d_base + off_results);
  p->d_strs = p->d_base + off_strs;
  p->d_ws = p->d_base + off_ws;

  // the upload image: operands, the sorted job table with device pointers, zeroed LCF keys,
  // prefilled results (status of the jobs that never reach the device)
  {
    size_t at = off_arena;
    for (size_t q = 0; q < n_parts; ++q) { if (parts[q].arena_len) memcpy(p->h_up + at, parts[q].arena, parts[q].arena_len); at += parts[q].arena_len; }
  }
  DevJob* hj = (DevJob*)(p->h_up + off_jobs);
  for (size_t q = 0; q < v.size(); ++q) {
    DevJob d = v[q].j;
    d.a = (v[q].ag ? d_gen : p->d_arena) + v[q].a_off;
    d.b = (v[q].bg ? d_gen : p->d_arena) + v[q].b_off;
    hj[q] = d;
  }
  memset(p->h_up + off_keys, 0, off_results - off_keys);
  if (n_jobs) memcpy(p->h_up + off_results, p->prefill.data(), n_jobs * sizeof(DevResult));
  const hipError_t e = hipMemcpyAsync(p->d_base, p->h_up, p->up_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) return set_err(ctx, PGPU_EDEVICE, "upload failed: %s", hipGetErrorString(e));
  if (ctx->poison >= 0) {
    // debugging aid (PGPU_POISON=<byte>): what the kernels are going to write -- strings, traceback workspace --
    // starts from a known pattern instead of whatever the previous batch left there; an answer that changes
    // with the pattern comes from a read of memory nothing wrote (tools/stress_parity.py --poison)
    if (hipMemsetAsync(p->d_base + off_strs, ctx->poison, total - off_strs, ctx->stream) != hipSuccess) return set_err(ctx, PGPU_EDEVICE, "poison fill failed");
  }
  return PGPU_OK;
}

extern "C" int pgpu_dp_plan_create_parts(pgpu_ctx* ctx, const pgpu_index* idx, const pgpu_dp_part* parts,
                                         size_t n_parts, pgpu_dp_plan** out) {
  if (!ctx || !out || (n_parts && !parts)) return set_err(ctx, PGPU_EINVAL, "bad argument");
  *out = nullptr;
  size_t n_jobs = 0, arena_len = 0;
  for (size_t q = 0; q < n_parts; ++q) {
    if ((parts[q].n_jobs && !parts[q].jobs) || (parts[q].arena_len && !parts[q].arena)) return set_err(ctx, PGPU_EINVAL, "bad argument");
    n_jobs += parts[q].n_jobs; arena_len += parts[q].arena_len;
  }
  if (n_jobs >= (size_t)1 << 30) return set_err(ctx, PGPU_EINVAL, "too many jobs");   // (the batch launch counts them in int)
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  pgpu_dp_plan* p = new (std::nothrow) pgpu_dp_plan();
  if (!p) return set_err(ctx, PGPU_ENOMEM, "out of host memory");
  p->n_jobs = n_jobs;
  p->owner = ctx;
  p->pooled = pgpu_ctx_pool_acquire(ctx, 0);
  p->batch.desc.ix = pgpu_index_lcf_view(idx);

  std::vector<Keyed> v = classify_jobs(parts, n_parts, n_jobs, p->batch.desc.ix, idx != nullptr, idx ? pgpu_index_length(idx) : 0, p->prefill);
  sort_jobs(v);
  const DpSpace sp = assign_workspace(v, p->lcf_out);
  p->ws_bytes = sp.ws; p->strs_bytes = sp.strs; p->n_keys = p->lcf_out.size(); p->n_dev_jobs = v.size();
  std::vector<Slice> batched;
  form_groups(v, p->groups, batched, p->cells, p->algo_bytes);
  form_batch(p->groups, batched, p->batch);

  const int rc = plan_upload(ctx, p, parts, n_parts, arena_len, v, idx ? pgpu_index_genomic(idx) : nullptr);
  if (rc != PGPU_OK) { plan_free(p); return rc; }
  *out = p;
  return PGPU_OK;
}

extern "C" int pgpu_dp_plan_launch(pgpu_ctx* ctx, pgpu_dp_plan* p) {
  if (!ctx || !p) return set_err(ctx, PGPU_EINVAL, "bad argument");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  p->synced = false; p->lcf_decoded = false;       // a relaunch downloads anew: the image holds raw keys again
  // Launch order: the groups are independent, and the host needs a few microseconds per launch, so
  // the long poles go first (RouteInfo.weight): the batch launch, the one-job-per-workgroup sweeps it does not
  // hold, the large alignments, ... and the large edit distances last.
  std::vector<size_t> order;
  std::vector<size_t> key_of(p->groups.size(), 0);
  auto weight = [&](size_t gi) -> long {
    const RouteInfo& ri = ROUTES[p->groups[gi].route];
    return ri.weight + (ri.by_rows ? (long)p->groups[gi].max_rows : 0);
  };
  {
    size_t kb = 0;
    for (size_t gi = 0; gi < p->groups.size(); ++gi) {
      const Group& g = p->groups[gi];
      if (ROUTES[g.route].keyed) { key_of[gi] = kb; kb += g.own.count; }
      if (g.own.count) order.push_back(gi);                // (0: nothing left outside the batch launch)
    }
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return weight(a) > weight(b); });
  }
  // only the auxiliary streams (RouteInfo.lane) a plan uses are forked and joined
  unsigned used_mask = 0;
  for (size_t gi : order) { const int l = ROUTES[p->groups[gi].route].lane; if (l >= 0) used_mask |= 1u << l; }
  if (used_mask) {            // fork: the upload (plan_create) is on the main stream
    HIP_TRY(ctx, hipEventRecord(ctx->ev_upload, ctx->stream));
    for (int i = 0; i < pgpu_ctx::NAUX; ++i)
      if (used_mask & (1u << i)) {
        if (!aux_stream(ctx, i)) return set_err(ctx, PGPU_EDEVICE, "auxiliary stream %d could not be created", i);
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux[i], ctx->ev_upload, 0));
      }
  }
  for (size_t gi : order) {
    Group& g = p->groups[gi];
    const RouteInfo& ri = ROUTES[g.route];
    hipStream_t st = ri.lane >= 0 ? ctx->aux[ri.lane] : ctx->stream;
    if (g.ev0) HIP_TRY(ctx, hipEventRecord(g.ev0, st));
    const ProfRange range(ri.name);
    if (g.route == RT_BATCH) {
      if (!launch_dp_batch(p->d_jobs, p->batch.desc, p->batch.bc_max_rows, p->d_results, p->d_ws, p->d_strs, st))
        return set_err(ctx, PGPU_EDEVICE, "batch launch: LDS budget exceeded");
    } else {
      if (!ri.launch) return set_err(ctx, PGPU_EDEVICE, "no kernel for %zu jobs of %s outside the batch launch", g.own.count, ri.name);
      ri.launch(DpLaunch{p->d_jobs + g.own.first, (int)g.own.count, g.max_rows, g.max_chunks, g.max_l2, p->d_results, p->d_ws,
                         p->d_strs, p->d_keys + key_of[gi], st});
    }
    if (g.ev1) HIP_TRY(ctx, hipEventRecord(g.ev1, st));
    // behind the batch launch (and outside its pair of events, which time the one kernel the profiler lists as
    // dp_batch_kernel): the whole-matrix sweep of the banded alignments it could not settle
    if (g.route == RT_BATCH) launch_align_fallback(p->d_jobs + p->batch.ab_start, p->batch.ab_count, p->d_results, p->d_ws, p->d_strs, st);
    HIP_TRY(ctx, hipGetLastError());
  }
  for (int i = 0; i < pgpu_ctx::NAUX; ++i) {      // join: the main stream continues after every stream that was used
    if (!(used_mask & (1u << i))) continue;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_aux[i], ctx->aux[i]));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_aux[i], 0));
  }
  // results and alignment strings come back in one copy as soon as every group is done
  if (p->down_bytes)
    HIP_TRY(ctx, hipMemcpyAsync(p->h_down, p->d_base + p->off_keys, p->down_bytes, hipMemcpyDeviceToHost, ctx->stream));
  p->launched = true;
  return PGPU_OK;
}

// find_longest_common_factor_dp's answer from the key the kernel left (lcf_key in pgpu_dp_kernels.hip)
static void decode_lcf_keys(pgpu_dp_plan* p) {
  if (p->lcf_decoded) return;
  p->lcf_decoded = true;
  const unsigned long long* keys = (const unsigned long long*)p->h_down;
  DevResult* res = (DevResult*)(p->h_down + (p->off_results - p->off_keys));
  for (size_t k = 0; k < p->lcf_out.size(); ++k) {
    DevResult& r = res[p->lcf_out[k]];
    const unsigned long long key = keys[k];
    r.status = PGPU_OK;
    r.v[0] = (int32_t)(key >> 44);
    r.v[1] = key ? (int32_t)(0x0FFFFFFFu - (uint32_t)((key >> 16) & 0x0FFFFFFFu)) : 0;
    r.v[2] = key ? (int32_t)(0xFFFFu - (uint32_t)(key & 0xFFFFu)) : 0;
  }
}

extern "C" int pgpu_dp_plan_sync(pgpu_ctx* ctx, pgpu_dp_plan* p) {
  if (!ctx || !p) return set_err(ctx, PGPU_EINVAL, "bad argument");
  if (wait_stream(ctx, ctx->stream) != 0) return set_err(ctx, PGPU_EDEVICE, "waiting for the batch failed");
  p->synced = p->launched;
  if (p->launched) {
    decode_lcf_keys(p);
    for (int k = 0; k < PGPU_DP_NKINDS; ++k) { p->ms[k] = 0; p->launches[k] = 0; }
    for (auto& g : p->groups) {
      float ms = 0.f;
      if (!g.own.count) continue;           // everything of this group ran inside the batch launch
      if (g.ev0 && g.ev1 && hipEventElapsedTime(&ms, g.ev0, g.ev1) == hipSuccess) g.ms = ms;
      if (g.ev0) { hipEvent_t b = base_event(ctx->device, ctx->stream); float t0 = 0.f; g.t0_ms = (b && hipEventElapsedTime(&t0, b, g.ev0) == hipSuccess) ? t0 : -1.f; }
      p->ms[ROUTES[g.route].kind] += g.ms;
      p->launches[ROUTES[g.route].kind] += 1;
    }
  }
  return PGPU_OK;
}

extern "C" size_t pgpu_dp_plan_string_bytes(const pgpu_dp_plan* p) { return p ? p->strs_bytes : 0; }

extern "C" int pgpu_dp_plan_fetch(pgpu_ctx* ctx, pgpu_dp_plan* p, pgpu_dp_result* results,
                                  char* strings, size_t cap) {
  if (!ctx || !p || (p->n_jobs && !results)) return set_err(ctx, PGPU_EINVAL, "bad argument");
  if (p->strs_bytes && strings && cap < p->strs_bytes) return set_err(ctx, PGPU_ENOSPC, "string buffer too small: need %zu", p->strs_bytes);
  if (!p->launched) return set_err(ctx, PGPU_EINVAL, "the plan has not been launched");
  // launch enqueued the download behind the kernels; after this wait the pinned image is complete
  if (!p->synced && wait_stream(ctx, ctx->stream) != 0) return set_err(ctx, PGPU_EDEVICE, "result download failed");
  p->synced = true;
  decode_lcf_keys(p);
  const size_t rb = p->n_jobs * sizeof(DevResult);
  if (rb) memcpy(results, p->h_down + (p->off_results - p->off_keys), rb);
  if (p->strs_bytes && strings) memcpy(strings, p->h_down + (p->down_bytes - p->strs_bytes), p->strs_bytes);
  return PGPU_OK;
}

extern "C" int pgpu_dp_plan_results_to_device(pgpu_ctx* ctx, pgpu_dp_plan* p, void* dst, size_t cap) {
  if (!ctx || !p || !dst) return set_err(ctx, PGPU_EINVAL, "bad argument");
  const size_t bytes = p->n_jobs * sizeof(DevResult);
  if (cap < bytes) return set_err(ctx, PGPU_ENOSPC, "device buffer too small: need %zu", bytes);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!p->launched) return set_err(ctx, PGPU_EINVAL, "the plan has not been launched");
  // the complete results are in the pinned image (the LCF answers are decoded there)
  if (!p->synced && wait_stream(ctx, ctx->stream) != 0) return set_err(ctx, PGPU_EDEVICE, "result download failed");
  p->synced = true;
  decode_lcf_keys(p);
  if (bytes) HIP_TRY(ctx, hipMemcpyAsync(dst, p->h_down + (p->off_results - p->off_keys), bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return PGPU_OK;
}

extern "C" int pgpu_dp_plan_destroy(pgpu_ctx* ctx, pgpu_dp_plan* p) {
  if (!ctx || !p) return PGPU_EINVAL;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  plan_free(p);
  return PGPU_OK;
}

extern "C" uint64_t pgpu_dp_plan_cells(const pgpu_dp_plan* p, int kind) {
  return (p && kind >= 0 && kind < PGPU_DP_NKINDS) ? p->cells[kind] : 0;
}
extern "C" uint64_t pgpu_dp_plan_algo_bytes(const pgpu_dp_plan* p, int kind) {
  return (p && kind >= 0 && kind < PGPU_DP_NKINDS) ? p->algo_bytes[kind] : 0;
}
extern "C" double pgpu_dp_plan_kernel_ms(const pgpu_dp_plan* p, int kind) {
  return (p && kind >= 0 && kind < PGPU_DP_NKINDS) ? p->ms[kind] : 0.0;
}
extern "C" uint64_t pgpu_dp_plan_launches(const pgpu_dp_plan* p, int kind) {
  return (p && kind >= 0 && kind < PGPU_DP_NKINDS) ? p->launches[kind] : 0;
}

extern "C" int pgpu_dp_plan_n_groups(const pgpu_dp_plan* p) { return p ? (int)p->groups.size() : 0; }

extern "C" int pgpu_dp_plan_group_info(const pgpu_dp_plan* p, int i, pgpu_group_info* out) {
  if (!p || !out || i < 0 || i >= (int)p->groups.size()) return PGPU_EINVAL;
  const Group& g = p->groups[i];
  memset(out, 0, sizeof(*out));
  snprintf(out->name, sizeof(out->name), "%s", ROUTES[g.route].name);
  out->kind = ROUTES[g.route].kind; out->jobs = g.own.count; out->cells = g.own.cells; out->algo_bytes = g.own.algo_bytes;
  out->ms = g.ms; out->t0_ms = g.t0_ms;
  return PGPU_OK;
}

extern "C" int pgpu_dp_batch(pgpu_ctx* ctx, const pgpu_index* idx, const pgpu_dp_job* jobs,
                             size_t n_jobs, const char* arena, size_t arena_len,
                             pgpu_dp_result* results, char* strings, size_t strings_cap,
                             size_t* strings_used) {
  pgpu_dp_plan* p = nullptr;
  int rc = pgpu_dp_plan_create(ctx, idx, jobs, n_jobs, arena, arena_len, &p);
  if (rc != PGPU_OK) return rc;
  if (strings_used) *strings_used = p->strs_bytes;
  rc = pgpu_dp_plan_launch(ctx, p);
  if (rc == PGPU_OK) rc = pgpu_dp_plan_sync(ctx, p);
  if (rc == PGPU_OK) rc = pgpu_dp_plan_fetch(ctx, p, results, strings, strings_cap);
  pgpu_dp_plan_destroy(ctx, p);
  return rc;
}
