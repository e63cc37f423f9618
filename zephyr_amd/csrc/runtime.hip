// What libhelm keeps per process rather than per handle: the kernel registry with helm_warm, the counters of runtime objects and host-side
// waits, the tuning options, the pools of device buffers, pinned host buffers, streams and events, the scratch slots of the direct path, the scratch of
// enqueued factorisations on its way back to the pool, and the staged copies between the caller's host arrays and the device.
#include "helm_internal.hpp"
#include <chrono>
#include <atomic>
#include <unistd.h>
#include <time.h>
#include <mutex>
#include <thread>
#include <map>
#include <cstring>
#include <algorithm>

// ---- kernel registry and runtime-object bookkeeping (helm_internal.hpp) ---------------------------------------------------------------------
// (function-local statics: kernels register during the static initialisation of whichever translation unit comes first)
namespace {
struct KernelRec { const void *fn; const char *pretty; std::atomic<bool> launched{false}; };
struct KernelRegistry {
    std::mutex mu;
    std::vector<KernelRec *> recs;                 // records are never moved or freed: slots stay valid without the lock
    std::atomic<KernelRec *> fast[2048];
    std::atomic<int> n{0};
};
KernelRegistry &kreg() { static KernelRegistry *r = new KernelRegistry(); return *r; }
struct RuntimeCounters {
    std::atomic<long long> dev_frees{0}, dev_free_us{0}, sync_calls{0}, sync_us{0}, slow_syncs{0}, worst_sync_us{0};
    std::atomic<long long> dev_allocs{0}, dev_alloc_bytes{0}, dev_alloc_us{0}, host_allocs{0}, host_alloc_bytes{0}, host_alloc_us{0},
                           events{0}, streams{0}, first_launches{0}, first_launch_us{0}, resolved{0}, warm_us{0};
};
RuntimeCounters &rtc() { static RuntimeCounters *c = new RuntimeCounters(); return *c; }
double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}
double HelmFirstLaunch::now_ms() { return wall_ms(); }
int helm_kernel_register(const void *fn, const char *pretty) {
    KernelRegistry &r = kreg();
    std::lock_guard<std::mutex> lk(r.mu);
    KernelRec *k = new KernelRec(); k->fn = fn; k->pretty = pretty;
    r.recs.push_back(k);
    const int slot = (int)r.recs.size() - 1;
    if (slot < 2048) r.fast[slot].store(k);
    r.n.store(slot + 1);
    return slot;
}
bool helm_kernel_first_launch(int slot) {
    if (slot < 0 || slot >= 2048) return false;
    KernelRec *k = kreg().fast[slot].load(std::memory_order_relaxed);
    if (!k || k->launched.load(std::memory_order_relaxed)) return false;
    return !k->launched.exchange(true);
}
void helm_kernel_first_launch_done(int slot, double host_ms) {
    (void)slot;
    rtc().first_launches += 1; rtc().first_launch_us += (long long)(host_ms * 1e3);
    static const bool tr = getenv("HELM_LAUNCH_TRACE") && atoi(getenv("HELM_LAUNCH_TRACE"));
    if (tr) { KernelRec *k = kreg().fast[slot].load(); fprintf(stderr, "[helm first launch] %8.3f ms  %s\n", host_ms, k ? k->pretty : "?"); }
}
hipError_t helm_counted_malloc(void **p, size_t bytes) {
    const double t0 = wall_ms();
    const hipError_t e = (hipMalloc)(p, bytes);
    static const int tr = getenv("HELM_ALLOC_TRACE") ? atoi(getenv("HELM_ALLOC_TRACE")) : 0;
    if (tr >= 2) fprintf(stderr, "[helm alloc] hipMalloc %12zu B  %8.3f ms\n", bytes, wall_ms() - t0);
    rtc().dev_allocs += 1; rtc().dev_alloc_bytes += (long long)bytes; rtc().dev_alloc_us += (long long)((wall_ms() - t0) * 1e3);
    return e;
}
namespace {
struct SyncTimer {
    const char *what, *file; int line; double t0;
    SyncTimer(const char *w, const char *f, int l) : what(w), file(f), line(l), t0(wall_ms()) {}
    ~SyncTimer() {
        const double ms = wall_ms() - t0;
        rtc().sync_calls += 1; rtc().sync_us += (long long)(ms * 1e3);
        if (ms >= 10.0) { rtc().slow_syncs += 1; long long us = (long long)(ms * 1e3), prev = rtc().worst_sync_us.load(); while (us > prev && !rtc().worst_sync_us.compare_exchange_weak(prev, us)) {} }
        static const double thr = getenv("HELM_SYNC_TRACE") ? atof(getenv("HELM_SYNC_TRACE")) : 0.0;
        if (thr > 0 && ms >= thr) { const char *b = strrchr(file, '/'); fprintf(stderr, "[helm sync] %-22s %9.3f ms  %s:%d\n", what, ms, b ? b + 1 : file, line); }
    }
};
}
// A wait may poll before it blocks (helm_tuning.sync_spin_ms, default 0 = block at once).  Round 6 built this while hunting 60-80 ms stalls of the config-4
// gradient step in the belief that threads asleep on the runtime's interrupt were woken late; the stalls were the container's CPU quota freezing the process
// (zephyr_amd/problem.py, _norm2), which a polling thread makes worse, not better: under a quota every spinning thread is budget the launching threads
// do not have.  Kept as an option for hosts without one (the poll saves the 20-50 us wake-up of each of the ~30 waits of a work item).
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
}
// helm_tuning.sync_sleep_us > 0: a wait polls with a sleep of that many microseconds between two looks instead of the runtime's own wait, which keeps a CPU busy
// for as long as it lasts -- 2.5 CPUs per process in the pipelined bench job (two threads that are nearly always waiting for the GPU).  For N processes on a node
// whose container grants fewer CPUs than 2.5 N (round 6: 16 for the one-GPU boxes): exhausting the quota freezes every thread of every process for the rest of
// the scheduler period (profiles/r06_cpu_quota_stall.txt).  Costs the sleep's granularity per wait (~50 us, ~30 waits per work item).
static bool sleep_wait(hipStream_t s, hipEvent_t e, int sleep_us) {
    struct timespec ts; ts.tv_sec = 0; ts.tv_nsec = (long)sleep_us * 1000L;
    for (;;) {
        const hipError_t q = e ? hipEventQuery(e) : hipStreamQuery(s);
        if (q == hipSuccess) return true;
        (void)hipGetLastError();
        if (q != hipErrorNotReady) return false;
        nanosleep(&ts, nullptr);
    }
}
// wait for the stream, or for the event when one is given: sleeping poll (sync_sleep_us), else a bounded spin (sync_spin_ms), then the runtime's own wait
static hipError_t timed_wait(hipStream_t s, hipEvent_t e) {
    { const int su = helm_tuning_now().sync_sleep_us; if (su > 0 && sleep_wait(s, e, su)) return hipSuccess; }
    const double budget = helm_tuning_now().sync_spin_ms;
    if (budget > 0) {
        const double t0 = wall_ms();
        for (;;) {
            const hipError_t q = e ? hipEventQuery(e) : hipStreamQuery(s);
            if (q == hipSuccess) return hipSuccess;
            if (q != hipErrorNotReady) { (void)hipGetLastError(); break; }
            (void)hipGetLastError();
            if (wall_ms() - t0 > budget) break;
            for (int i = 0; i < 64; ++i) cpu_relax();
        }
    }
    return e ? (hipEventSynchronize)(e) : (hipStreamSynchronize)(s);
}
hipError_t helm_timed_stream_sync(hipStream_t s, const char *file, int line) { SyncTimer t("hipStreamSynchronize", file, line); return timed_wait(s, nullptr); }
hipError_t helm_timed_event_sync(hipEvent_t e, const char *file, int line) { SyncTimer t("hipEventSynchronize", file, line); return timed_wait(nullptr, e); }
hipError_t helm_timed_device_sync(const char *file, int line) { SyncTimer t("hipDeviceSynchronize", file, line); return (hipDeviceSynchronize)(); }
hipError_t helm_timed_memcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, const char *file, int line) { SyncTimer t("hipMemcpy", file, line); return (hipMemcpy)(dst, src, bytes, kind); }
hipError_t helm_counted_free(void *p) {
    if (!p) return hipSuccess;
    const double t0 = wall_ms();
    const hipError_t e = (hipFree)(p);                 // (waits for every stream of the device)
    const double ms = wall_ms() - t0;
    rtc().dev_frees += 1; rtc().dev_free_us += (long long)(ms * 1e3);
    static const int tr = getenv("HELM_ALLOC_TRACE") ? atoi(getenv("HELM_ALLOC_TRACE")) : 0;
    if (tr >= 2) fprintf(stderr, "[helm alloc] hipFree   %p  %8.3f ms\n", p, ms);
    return e;
}
hipError_t helm_counted_host_malloc(void **p, size_t bytes, unsigned flags) {
    const double t0 = wall_ms();
    const hipError_t e = (hipHostMalloc)(p, bytes, flags);
    rtc().host_allocs += 1; rtc().host_alloc_bytes += (long long)bytes; rtc().host_alloc_us += (long long)((wall_ms() - t0) * 1e3);
    return e;
}
hipError_t helm_counted_event_create(hipEvent_t *e, unsigned flags) { rtc().events += 1; return flags ? (hipEventCreateWithFlags)(e, flags) : (hipEventCreate)(e); }
hipError_t helm_counted_stream_create(hipStream_t *s, unsigned flags, int prio, bool with_prio) {
    rtc().streams += 1;
    return with_prio ? (hipStreamCreateWithPriority)(s, flags, prio) : (hipStreamCreateWithFlags)(s, flags);
}
extern "C" int helm_debug_runtime_stats(int reset, helm_runtime_stats *out) {
    RuntimeCounters &c = rtc();
    if (out) {
        out->dev_allocs = c.dev_allocs.load(); out->dev_alloc_bytes = (double)c.dev_alloc_bytes.load(); out->dev_alloc_ms = c.dev_alloc_us.load() * 1e-3;
        out->host_allocs = c.host_allocs.load(); out->host_alloc_bytes = (double)c.host_alloc_bytes.load(); out->host_alloc_ms = c.host_alloc_us.load() * 1e-3;
        out->events_created = c.events.load(); out->streams_created = c.streams.load();
        out->first_launches = c.first_launches.load(); out->first_launch_ms = c.first_launch_us.load() * 1e-3;
        out->kernels_registered = kreg().n.load(); out->kernels_resolved = c.resolved.load(); out->warm_ms = c.warm_us.load() * 1e-3;
        out->dev_frees = c.dev_frees.load(); out->dev_free_ms = c.dev_free_us.load() * 1e-3;
        out->sync_calls = c.sync_calls.load(); out->sync_ms = c.sync_us.load() * 1e-3; out->slow_syncs = c.slow_syncs.load(); out->worst_sync_ms = c.worst_sync_us.load() * 1e-3;
    }
    if (reset) { c.dev_allocs = 0; c.dev_alloc_bytes = 0; c.dev_alloc_us = 0; c.host_allocs = 0; c.host_alloc_bytes = 0; c.host_alloc_us = 0;
                 c.events = 0; c.streams = 0; c.first_launches = 0; c.first_launch_us = 0; c.dev_frees = 0; c.dev_free_us = 0; c.sync_calls = 0; c.sync_us = 0; c.slow_syncs = 0; c.worst_sync_us = 0; }
    return HELM_OK;
}
// (diagnostic) a thread of the library that does nothing but read the clock: the longest interval between two readings while it ran.  Tells a stall of the
// PROCESS (every thread stops: the watcher sees it too) from a stall of the GPU or of the runtime (the watcher keeps running).
namespace { std::atomic<bool> g_watch_on{false}; std::atomic<long long> g_watch_worst_us{0}, g_watch_gaps{0}; std::thread *g_watch_thread = nullptr; }
extern "C" int helm_debug_stall_watch(int start, double *worst_gap_ms, long long *gaps_over_5ms) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (start) {
        if (g_watch_thread) return HELM_OK;
        g_watch_worst_us = 0; g_watch_gaps = 0; g_watch_on = true;
        g_watch_thread = new std::thread([] {
            double last = wall_ms();
            while (g_watch_on.load(std::memory_order_relaxed)) {
                const double now = wall_ms(), gap = now - last;
                last = now;
                if (gap > 5.0) g_watch_gaps += 1;
                long long us = (long long)(gap * 1e3), prev = g_watch_worst_us.load();
                while (us > prev && !g_watch_worst_us.compare_exchange_weak(prev, us)) {}
            }
        });
        return HELM_OK;
    }
    if (g_watch_thread) { g_watch_on = false; g_watch_thread->join(); delete g_watch_thread; g_watch_thread = nullptr; }
    if (worst_gap_ms) *worst_gap_ms = g_watch_worst_us.load() * 1e-3;
    if (gaps_over_5ms) *gaps_over_5ms = g_watch_gaps.load();
    return HELM_OK;
}
static void slab_reserve(int device);
// Resolve every kernel of the library on `device` (code objects loaded, dispatch records built) without launching anything.  Idempotent; runs by itself
// when the first operator of a device is created (HELM_WARM=0 leaves it to the caller).
extern "C" int helm_warm(int device) {
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); helm_set_error(nullptr, "helm_warm: hipSetDevice failed"); return HELM_ERR_DEVICE; }
    static std::mutex mu; static std::map<int, int> done;
    std::lock_guard<std::mutex> lk(mu);
    KernelRegistry &r = kreg();
    const int n = std::min(r.n.load(), 2048);
    int &upto = done[device];
    const double t0 = wall_ms();
    for (int i = upto; i < n; ++i) {
        hipFuncAttributes at;
        if (hipFuncGetAttributes(&at, r.fast[i].load()->fn) == hipSuccess) rtc().resolved += 1; else (void)hipGetLastError();
    }
    upto = n;
    slab_reserve(device);
    rtc().warm_us += (long long)((wall_ms() - t0) * 1e3);
    return n;
}

// ---- tuning (include/helm.h: helm_tuning) ------------------------------------------------------------------------------------------------
int helm_env_int(const char *name, int d) { const char *v = getenv(name); return v ? atoi(v) : d; }
namespace {
std::mutex g_tune_mu;
bool g_tune_set = false;
helm_tuning g_tune_user;
double tune_d(const char *name, double d) { const char *v = getenv(name); return v ? atof(v) : d; }
}
// the limits every source of the options goes through (environment, helm_set_tuning): values outside them would switch a path off by accident
// (nd_plans = 0, nd_ws_gb = 0: batch forced to 1) rather than by intent
static void tuning_clamp(helm_tuning &t) {
    t.nd_leaf = std::max(2, t.nd_leaf);
    if (!(t.nd_ws_gb > 0)) t.nd_ws_gb = 32.0;
    t.nd_stable_safety = std::max(1.0, t.nd_stable_safety);
    if (!(t.nd_stable_thr >= 0)) t.nd_stable_thr = 0.0;
    t.nd_fused_leaf_min = std::max(1, t.nd_fused_leaf_min);
    t.nd_gjstep_min = std::max(64, t.nd_gjstep_min);
    t.nd_plans = std::max(1, t.nd_plans);
    t.ws_slots = std::min(4, std::max(1, t.ws_slots));
    t.pf_prio = t.pf_prio > 0 ? 1 : (t.pf_prio < 0 ? -1 : 0);
    if (!(t.mg3_omega > 0) || t.mg3_omega > 2.0) t.mg3_omega = 0.9;
    t.mg3_coarse = std::min(2, std::max(0, t.mg3_coarse));
    t.mg3_nd_leaf = std::max(2, t.mg3_nd_leaf);
    if (!std::isfinite(t.mg3_beta) || t.mg3_beta < 0) t.mg3_beta = 0.0;
    if (!(t.sync_spin_ms >= 0)) t.sync_spin_ms = 0.0;
    t.sync_spin_ms = std::min(t.sync_spin_ms, 60000.0);
    t.sync_sleep_us = std::min(100000, std::max(0, t.sync_sleep_us));
    t.nd_fused_sep_min = std::max(1, t.nd_fused_sep_min);
}
static helm_tuning tuning_from_env() {
    helm_tuning t;
    t.nd_leaf = helm_env_int("HELM_ND_LEAF", 8);
    t.nd_ws_gb = tune_d("HELM_ND_WS_GB", 32.0);
    t.nd_sparse_rhs = helm_env_int("HELM_ND_SPARSE_RHS", 1);
    t.nd_stable = helm_env_int("HELM_ND_STABLE", 1);
    t.nd_stable_thr = tune_d("HELM_ND_STABLE_THR", 0.0);
    t.nd_stable_safety = tune_d("HELM_ND_STABLE_SAFETY", 8.0);
    t.nd_fused_leaf = helm_env_int("HELM_ND_FUSEDLEAF", 1);
    t.nd_fused_leaf_min = helm_env_int("HELM_ND_FUSEDLEAF_MIN", 2048);
    t.nd_gjstep = helm_env_int("HELM_ND_GJSTEP", 1);
    t.nd_gjstep_min = helm_env_int("HELM_ND_GJSTEP_MIN", 128);
    t.nd_overlap = helm_env_int("HELM_ND_OVERLAP_NM", 1);
    t.nd_xcd_map = helm_env_int("HELM_ND_XCDMAP", 2);
    t.nd_plans = helm_env_int("HELM_ND_PLANS", 6);
    t.nd_direct_out = helm_env_int("HELM_ND_DIRECT_OUT", 1);
    t.nd_leaf_idle = helm_env_int("HELM_ND_LEAF_IDLE", 1);
    t.nd_many = helm_env_int("HELM_ND_MANY", 1);
    t.auto_direct = helm_env_int("HELM_AUTO_DIRECT", 1);
    t.auto_mg3 = helm_env_int("HELM_AUTO_MG3", 1);
    t.prof_ext = helm_env_int("HELM_PROF_EXT", 1);
    t.ws_slots = helm_env_int("HELM_WS_SLOTS", 3);
    t.pf_prio = helm_env_int("HELM_PF_PRIO", 1);
    t.mg3_keep = helm_env_int("HELM_MG3_KEEP", 1);
    t.mg3_keep_levels = helm_env_int("HELM_MG3_KEEP_LEVELS", -1);
    t.mg3_galerkin = helm_env_int("HELM_MG3_GALERKIN", 1);
    t.mg3_depth_model = helm_env_int("HELM_MG3_DEPTH_MODEL", 1);
    t.mg3_bt_f32 = helm_env_int("HELM_MG3_BT_F32", 1);
    t.mg3_otf = helm_env_int("HELM_MG3_OTF", 1);
    t.mg3_f32 = helm_env_int("HELM_MG3_F32", 1);
    t.mg3_omega = tune_d("HELM_MG3_OMEGA", 0.9);
    { const char *cs = getenv("HELM_MG3_COARSE"); t.mg3_coarse = cs && !strcmp(cs, "nd") ? 1 : (cs && !strcmp(cs, "bt") ? 2 : 0); }
    t.mg3_nd_leaf = helm_env_int("HELM_MG3_ND_LEAF", 2);
    t.mg3_bt_twist = helm_env_int("HELM_MG3_BT_TWIST", 1);
    t.mg3_beta = tune_d("HELM_MG3_BETA", 0.0);
    t.sync_spin_ms = tune_d("HELM_SYNC_SPIN_MS", 0.0);
    t.sync_sleep_us = helm_env_int("HELM_SYNC_SLEEP_US", 0);
    t.nd_fused_sep = helm_env_int("HELM_ND_FUSEDSEP", 1);
    t.nd_fused_sep_min = helm_env_int("HELM_ND_FUSEDSEP_MIN", 512);
    tuning_clamp(t);
    return t;
}
// The options in force.  helm_set_tuning's structure wins; otherwise defaults + environment, re-read when the HELM_* entries of the environment have changed
// (a test may flip a variable between two calls): the passes ask once per tree level from worker threads, and 27 getenv calls each time raced against exactly
// that setenv.  The environment is compared by a fingerprint of its HELM_* entries, at API entry only (helm_tuning_refresh).
extern char **environ;
static unsigned long long env_fingerprint() {
    unsigned long long h = 1469598103934665603ull;
    for (char **e = environ; e && *e; ++e) {
        const char *s = *e;
        if (s[0] != 'H' || s[1] != 'E' || s[2] != 'L' || s[3] != 'M' || s[4] != '_') continue;
        for (; *s; ++s) { h ^= (unsigned char)*s; h *= 1099511628211ull; }
        h ^= 0xff; h *= 1099511628211ull;
    }
    return h;
}
static bool g_tune_have = false; static unsigned long long g_tune_fp = 0; static helm_tuning g_tune_cached;
// called at the entry of the API calls that start work (create, assemble, prefactor, solve, apply, get_tuning): the environment is looked at THERE, by the
// calling thread, and nowhere below -- a caller that changes a HELM_* variable does so between two calls, as the header says
void helm_tuning_refresh() {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    const unsigned long long now = env_fingerprint();
    if (!g_tune_have || now != g_tune_fp) { g_tune_cached = tuning_from_env(); g_tune_fp = now; g_tune_have = true; }
}
helm_tuning helm_tuning_now() {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    if (g_tune_set) return g_tune_user;
    if (!g_tune_have) { g_tune_cached = tuning_from_env(); g_tune_fp = env_fingerprint(); g_tune_have = true; }
    return g_tune_cached;
}
extern "C" int helm_get_tuning(helm_tuning *out) { if (!out) return HELM_ERR_ARG; helm_tuning_refresh(); *out = helm_tuning_now(); return HELM_OK; }
extern "C" int helm_set_tuning(const helm_tuning *t) {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    if (t) { g_tune_user = *t; tuning_clamp(g_tune_user); g_tune_set = true; } else g_tune_set = false;
    return HELM_OK;
}

// Scratch of the direct path (fronts while factoring, front vectors while solving) is tens of GB at the bench size and
// is only needed during a call, so all handles of a process share one buffer; a handle that finds it taken (another
// host thread is inside a solve) falls back to its own.
// r4: the table is PER DEVICE (HELM_WS_SLOTS slots each, default 3, at most 4).  Round 3 kept one table of 3-4 slots for the whole process,
// tagged with a device: under the in-process dispatcher on an 8-GPU node the first three or four GPUs to ask got them and every other GPU
// allocated its ~30 GB beside running kernels on every solve (the 0.7-1.5 s stalls helm_reserve exists to remove).  A lease is
// (device, slot) packed as device * WS_SLOTS_MAX + slot.
#define WS_SLOTS_MAX 4
struct WsSlot { void *ptr = nullptr; size_t bytes = 0; bool busy = false; };
struct WsDevice { WsSlot slot[WS_SLOTS_MAX]; };
struct SharedWs { std::mutex mu; std::map<int, WsDevice> dev; };
static SharedWs g_shared_ws;
static int shared_ws_slots() { const int n = helm_tuning_now().ws_slots; return n < 1 ? 1 : (n > WS_SLOTS_MAX ? WS_SLOTS_MAX : n); }

// idle device buffers by (device, size); `held` and the cap are per device (r4: one sum over all GPUs hit a single device's cap with the second GPU's buffers)
struct DevPool { std::mutex mu; std::multimap<std::pair<int, size_t>, void *> idle; std::map<int, size_t> held; };
static DevPool g_pool;
static std::map<int, std::vector<hipEvent_t>> g_idle_events;      // per device, guarded by g_pool.mu

int helm_events_grow(helm_op *op, int n) {
    std::lock_guard<std::mutex> lk(g_pool.mu);
    for (int i = 0; i < n; ++i) {
        hipEvent_t e;
        std::vector<hipEvent_t> &idle = g_idle_events[op->device];
        if (!idle.empty()) { e = idle.back(); idle.pop_back(); }
        else if (hipEventCreate(&e) != hipSuccess) return -1;
        op->ev_pool.push_back(e);
    }
    return 0;
}
void helm_events_release(helm_op *op) {
    std::lock_guard<std::mutex> lk(g_pool.mu);
    std::vector<hipEvent_t> &idle = g_idle_events[op->device];
    for (hipEvent_t e : op->ev_pool) { if (idle.size() < 65536) idle.push_back(e); else hipEventDestroy(e); }
    op->ev_pool.clear();
}
// idle buffers of exactly that size the pool holds on the device (helm_reserve books up to a count)
size_t helm_pool_idle_count(int device, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_pool.mu);
    return g_pool.idle.count(std::make_pair(device, bytes));
}
// (small buffers too: hipFree waits for every stream of the device, which would stall a host thread that prepares the next operator
// while another one is solving -- the per-operator scratch of a few KB goes through the pool like the GB-sized buffers)
static const size_t kPoolMinBytes = (size_t)64;
// What the pool may hold idle: half of the device's memory (HELM_POOL_GB overrides; buffers below 1 MB are always kept: their hipFree
// would be a device synchronisation for nothing).  A 16-frequency job at 1024^2 hands back ~70 GB of
// factors when its operators go; with a 64-GB cap the overflow went to hipFree and the next job's hipMalloc calls -- issued while other
// threads had kernels and copies in flight -- took 1.2-1.5 s EACH (HELM_ALLOC_TRACE=1 shows them).
static size_t pool_cap_bytes(int device) {          // (call with g_pool.mu held)
    static std::map<int, size_t> caps;
    auto it = caps.find(device);
    if (it != caps.end()) return it->second;
    size_t cap = (size_t)64 << 30;
    if (const char *e = getenv("HELM_POOL_GB")) cap = (size_t)(atof(e) * 1e9);
    else {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) cap = prop.totalGlobalMem / 2;     // (r6: half, not three quarters -- the caller's own allocator (torch) lives on the same device and cannot make this pool give anything back)
        else (void)hipGetLastError();
    }
    caps[device] = cap;
    return cap;
}

// pinned host buffers (per-handle scalar records) and HIP streams are recycled the same way: a job creates one operator per frequency
// r4: the idle pool is capped by BYTES (HELM_HOSTPOOL_GB, default a quarter of the host's memory, at most 96 GB) and helm_trim / helm_host_trim
// give it back: results of 1 MB or more go through it (4.3 GB per frequency of the 2-D job), and with only an entry-count cap a long-lived
// process that changed nsrc or the split sizes could accumulate hundreds of GB of locked memory in size classes it never used again
struct HostPool { std::mutex mu; std::multimap<size_t, void *> idle; size_t held = 0; };
static HostPool g_hostpool;
static size_t hostpool_cap_bytes() {
    static const size_t cap = [] {
        if (const char *e = getenv("HELM_HOSTPOOL_GB")) return (size_t)(atof(e) * 1e9);
        const long pages = sysconf(_SC_PHYS_PAGES), psz = sysconf(_SC_PAGE_SIZE);
        const size_t ram = pages > 0 && psz > 0 ? (size_t)pages * (size_t)psz : (size_t)64 << 30;
        return std::min(ram / 4, (size_t)96 << 30);
    }();
    return cap;
}
// AllocTrace (helm_internal.hpp)
static std::atomic<long long> g_alloc_slow{0};
static std::atomic<long long> g_alloc_worst_us{0};
AllocTrace::AllocTrace(const char *w, size_t b) : what(w), bytes(b), t0(wall_ms()) {}
AllocTrace::~AllocTrace() {
    const double ms = wall_ms() - t0;
    if (ms > 1.0) {
        g_alloc_slow += 1;
        long long us = (long long)(ms * 1e3), prev = g_alloc_worst_us.load();
        while (us > prev && !g_alloc_worst_us.compare_exchange_weak(prev, us)) {}
        static const bool on = getenv("HELM_ALLOC_TRACE") && atoi(getenv("HELM_ALLOC_TRACE"));
        if (on) fprintf(stderr, "[helm alloc] %-14s %8.3f GB %9.1f ms\n", what, bytes * 1e-9, ms);
    }
}
// allocator calls (hipMalloc / hipFree / hipHostMalloc / pool flushes) that reached the driver and took more than 1 ms since the last reset
extern "C" int helm_debug_alloc_stats(int reset, long long *slow_calls, double *worst_ms) {
    if (slow_calls) *slow_calls = g_alloc_slow.load();
    if (worst_ms) *worst_ms = g_alloc_worst_us.load() * 1e-3;
    if (reset) { g_alloc_slow = 0; g_alloc_worst_us = 0; }
    return HELM_OK;
}

void *helm_hostpool_alloc(size_t bytes) {
    {
        std::lock_guard<std::mutex> lk(g_hostpool.mu);
        auto it = g_hostpool.idle.find(bytes);
        if (it != g_hostpool.idle.end()) { void *p = it->second; g_hostpool.idle.erase(it); g_hostpool.held -= bytes; return p; }
    }
    void *p = nullptr;
    AllocTrace tr("hipHostMalloc", bytes);
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void helm_hostpool_free(void *p, size_t bytes) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_hostpool.mu);
        if (g_hostpool.idle.size() < 1024 && (g_hostpool.held + bytes <= hostpool_cap_bytes() || bytes < ((size_t)1 << 20))) {
            g_hostpool.idle.insert(std::make_pair(bytes, p)); g_hostpool.held += bytes;
            return;
        }
    }
    AllocTrace tr("hipHostFree", bytes);
    hipHostFree(p);
}
// pinned host memory the library holds idle goes back to the system
extern "C" int helm_host_trim(void) {
    helm_tuning_refresh();
    std::lock_guard<std::mutex> lk(g_hostpool.mu);
    for (auto &kv : g_hostpool.idle) hipHostFree(kv.second);
    g_hostpool.idle.clear(); g_hostpool.held = 0;
    return HELM_OK;
}
struct StreamPool { std::mutex mu; std::multimap<std::pair<int, int>, hipStream_t> idle; };     // (device, priority class) -> idle streams
static StreamPool g_streams;
// prio: 0 normal, 1 highest, -1 lowest priority the device offers; the stream comes back idle (synchronised by helm_stream_release)
hipStream_t helm_stream_acquire(int device, int prio) {
    {
        std::lock_guard<std::mutex> lk(g_streams.mu);
        auto it = g_streams.idle.find(std::make_pair(device, prio));
        if (it != g_streams.idle.end()) { hipStream_t s = it->second; g_streams.idle.erase(it); return s; }
    }
    hipStream_t s = nullptr;
    if (prio == 0) { if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr; return s; }
    int plo = 0, phi = 0;
    (void)hipDeviceGetStreamPriorityRange(&plo, &phi);
    if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio > 0 ? phi : plo) != hipSuccess) return nullptr;
    return s;
}
void helm_stream_release(int device, int prio, hipStream_t s) {
    if (!s) return;
    hipStreamSynchronize(s);
    std::lock_guard<std::mutex> lk(g_streams.mu);
    if (g_streams.idle.size() < 64) { g_streams.idle.insert(std::make_pair(std::make_pair(device, prio), s)); return; }
    hipStreamDestroy(s);
}

// idle bytes of one device (what hipMemGetInfo's "free" figure does not count although an allocation can have them: mg3_available_bytes of mg3d.hip adds it)
size_t helm_pool_idle_bytes(int device) {
    std::lock_guard<std::mutex> lk(g_pool.mu);
    auto it = g_pool.held.find(device);
    return it == g_pool.held.end() ? 0 : it->second;
}
static void pool_forget(void *p);       // (g_pool.mu held) the buffer has gone back to the driver
static std::map<void *, bool> g_carved;  // blocks that are pieces of a slab (see slab_carve; guarded by g_pool.mu)
struct PoolClassStat { int in_use = 0, high = 0, total = 0; };
static std::map<std::pair<int, size_t>, PoolClassStat> g_pool_stats;         // (device, capacity) of big buffers; guarded by g_pool.mu        // (see pool_top_up)
// give this device's idle buffers back to the driver (the current device must be `device`)
static void pool_flush_device(int device) {
    std::lock_guard<std::mutex> lk(g_pool.mu);
    AllocTrace trf("pool flush", g_pool.held[device]);
    size_t kept = 0;
    for (auto it = g_pool.idle.lower_bound(std::make_pair(device, (size_t)0)); it != g_pool.idle.end() && it->first.first == device; ) {
        if (g_carved.count(it->second)) { kept += it->first.second; ++it; continue; }       // (a piece of a slab: stays idle)
        hipFree(it->second);
        pool_forget(it->second);
        it = g_pool.idle.erase(it);
    }
    g_pool.held[device] = kept;
    for (auto is = g_pool_stats.begin(); is != g_pool_stats.end(); ) { if (is->first.first == device) { is->second.total = is->second.in_use; is->second.high = is->second.in_use; } ++is; }
}
// hipMalloc that, under memory pressure, empties the device's idle pool and tries once more -- for every allocation of the library that does
// not go through the size-keyed pool itself (scratch slots, temporaries of the host-buffer entry points, plans)
hipError_t helm_malloc_retry(int device, void **p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return e;
    (void)hipGetLastError();
    pool_flush_device(device);
    e = hipMalloc(p, bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); *p = nullptr; }
    return e;
}
// r6: a request is served by the smallest idle buffer of the device whose capacity is at least the request and at most twice it (+ 1 MB; from 64 MB up: at most
// one size class more, so that the GB-sized factor and wavefield buffers do not take each other's places): the pool used to be
// keyed by the exact size, and sizes that follow the operator -- how many ill-conditioned fronts a frequency has, how many right-hand sides take a
// refinement pass -- missed it at every new frequency: 12 hipMalloc calls inside the timed region of the bench job after a five-item warm-up.  New buffers are
// allocated in size classes (steps of 1/8 of the power of two below, at least 4 KB), and the pool remembers every buffer's capacity, so a buffer
// goes back under what it can hold, not under what it was asked for.
static std::map<void *, size_t> g_pool_capacity;        // every live buffer that came out of helm_pool_alloc: what it can hold (guarded by g_pool.mu)
// Spares beyond the high-water mark (big buffers, 64 MB .. 16 GB): the pool of a class holds what the busiest moment so far needed, and a pipelined job's busiest
// moment is a matter of thread timing -- a job that got by with three factor buffers in its first five items asked for a fourth in its next twenty (round 6: 3 to 5 GB
// of hipMalloc inside the bench's timed region in one run of three; 0.6 ms on one box, 122 ms on another = the stall that cost round 5's driver run a fifth of its
// headline; with pairs of operators factored together a five-item warm-up sees one or two sets of pair buffers alive and the job needs three).  When the last
// operator of a device is destroyed -- every buffer idle, nobody waiting -- each such class whose busiest moment used EVERY buffer it had is topped up to
// high-water + HELM_POOL_SPARE (default 2); a class that kept one unused has its headroom and is left alone (so a job's last destroy adds nothing once the
// pool has settled: a top-up is a hipMalloc too, and the end of one timed pass is the eve of the next).
static const size_t kSpareMin = (size_t)64 << 20, kSpareMax = (size_t)16 << 30;
static void pool_forget(void *p) {
    auto it = g_pool_capacity.find(p);
    if (it == g_pool_capacity.end()) return;
    g_pool_capacity.erase(it);
}
// Small buffers (size class up to 16 MB: per-operator flags, estimates, split-K partials, the pivoted-LU storage of ill-conditioned fronts ...) come out of
// slabs of 512 MB, one hipMalloc each, carved by a bump pointer and recycled through the idle table like every other buffer.  Their sizes follow the operator
// -- how many fronts a frequency has flagged, which products split their inner dimension -- so a job met half a dozen new ones per pass over its frequencies
// however long the warm-up (round 6: 6 hipMalloc calls, 16 MB, in the timed region of every bench run).  A carved block is never handed back to the driver by
// itself; slabs live as long as the process (helm_trim keeps them: 512 MB each, a handful at most).
static const size_t kSlabBytes = (size_t)512 << 20, kSlabMaxBlock = (size_t)16 << 20;
struct Slab { char *base = nullptr; size_t used = 0; };
static std::map<int, std::vector<Slab>> g_slabs;                   // guarded by g_pool.mu
static bool slab_add(int device) {                                 // (g_pool.mu NOT held: the driver call may take milliseconds)
    void *b = nullptr;
    AllocTrace tr("pool slab", kSlabBytes);
    if (helm_malloc_retry(device, &b, kSlabBytes) != hipSuccess) return false;
    std::lock_guard<std::mutex> lk(g_pool.mu);
    Slab sl; sl.base = (char *)b;
    g_slabs[device].push_back(sl);
    return true;
}
static void *slab_carve(int device, size_t cap) {
    for (int attempt = 0; attempt < 2; ++attempt) {
        {
            std::lock_guard<std::mutex> lk(g_pool.mu);
            std::vector<Slab> &v = g_slabs[device];
            if (!v.empty()) {
                Slab &sl = v.back();
                const size_t off = (sl.used + 255) & ~(size_t)255;
                if (off + cap <= kSlabBytes) { sl.used = off + cap; void *p = sl.base + off; g_pool_capacity[p] = cap; g_carved[p] = true; return p; }
            }
        }
        if (!slab_add(device)) return nullptr;
    }
    return nullptr;
}
// the first slab of a device, brought into being by helm_warm (i.e. when the first operator of the device is created), not by whichever solve first misses the pool
static void slab_reserve(int device) {
    { std::lock_guard<std::mutex> lk(g_pool.mu); if (!g_slabs[device].empty()) return; }
    (void)slab_add(device);
}
static size_t pool_size_class(size_t bytes) {
    if (bytes <= 4096) return 4096;
    int top = 63 - __builtin_clzll((unsigned long long)(bytes - 1));      // bytes - 1 in [2^top, 2^(top+1))
    const int sh = top - 3;
    return (((bytes - 1) >> sh) + 1) << sh;
}
void *helm_pool_alloc(int device, size_t bytes) {
    if (bytes == 0) bytes = 1;
    {
        std::lock_guard<std::mutex> lk(g_pool.mu);
        // from 64 MB up a buffer of the request's own size class is preferred (the GB-sized factor, scratch and wavefield buffers keep to their own kind);
        // failing that -- and for small requests from the start -- the smallest idle buffer that holds the request and is at most twice its size (+ 1 MB).
        // (Measured, round 6: with the own-class rule alone the bench job allocated 5.2 GB inside its timed region in every run -- 0.6 ms on one box, 122 ms
        // on another, which is the kind of stall that cost round 5's driver run a fifth of its headline; with the fall-back: nothing above 8 MB.)
        static const double slack = getenv("HELM_POOL_SLACK") ? std::max(1.0, atof(getenv("HELM_POOL_SLACK"))) : 2.0;      // (diagnostic: 1 = a request's own size class only)
        static const int ptrace = getenv("HELM_ALLOC_TRACE") ? atoi(getenv("HELM_ALLOC_TRACE")) : 0;
        auto it = g_pool.idle.end();
        if (bytes >= ((size_t)64 << 20)) it = g_pool.idle.find(std::make_pair(device, pool_size_class(bytes)));
        if (it == g_pool.idle.end()) {
            it = g_pool.idle.lower_bound(std::make_pair(device, bytes));
            if (it != g_pool.idle.end() && (it->first.first != device || (double)it->first.second > slack * (double)bytes + (double)((size_t)1 << 20))) it = g_pool.idle.end();
        }
        if (ptrace >= 3 && bytes >= ((size_t)64 << 20))
            fprintf(stderr, "[helm pool] request %9.1f MB (class %9.1f MB): %s %9.1f MB\n", bytes / 1e6, pool_size_class(bytes) / 1e6, it != g_pool.idle.end() ? "served by an idle buffer of" : "MISS, allocating",
                    (it != g_pool.idle.end() ? it->first.second : pool_size_class(bytes)) / 1e6);
        if (it != g_pool.idle.end()) {
            void *p = it->second; g_pool.held[device] -= it->first.second;
            if (it->first.second >= kSpareMin) { PoolClassStat &cs = g_pool_stats[std::make_pair(device, it->first.second)]; cs.in_use += 1; cs.high = std::max(cs.high, cs.in_use); }
            g_pool.idle.erase(it); return p;
        }
    }
    void *p = nullptr;
    const size_t cap = pool_size_class(bytes);
    if (cap <= kSlabMaxBlock) {                 // small buffers are carved out of a slab: no driver call however many new sizes a frequency brings
        p = slab_carve(device, cap);
        if (p) return p;
    }
    AllocTrace tr("pool hipMalloc", cap);
    if (helm_malloc_retry(device, &p, cap) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_pool.mu);
    g_pool_capacity[p] = cap;
    if (cap >= kSpareMin) { PoolClassStat &cs = g_pool_stats[std::make_pair(device, cap)]; cs.total += 1; cs.in_use += 1; cs.high = std::max(cs.high, cs.in_use); }
    return p;
}
// (see PoolClassStat) called with no operator of the device alive
void helm_pool_top_up(int device, int spare) {
    std::vector<size_t> want;
    {
        std::lock_guard<std::mutex> lk(g_pool.mu);
        const size_t cap = pool_cap_bytes(device);
        size_t held = g_pool.held[device];
        for (auto &kv : g_pool_stats) {
            if (kv.first.first != device || kv.first.second > kSpareMax) continue;
            PoolClassStat &cs = kv.second;
            if (cs.high < cs.total) continue;                      // the busiest moment left a buffer of this class unused: enough headroom
            for (int k = cs.total; k < cs.high + spare && cs.high > 0; ++k) { if (held + kv.first.second > cap) break; want.push_back(kv.first.second); held += kv.first.second; }
        }
    }
    for (size_t bytes : want) {
        void *p = nullptr;
        AllocTrace tr("pool spare", bytes);
        if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); break; }        // (a spare is a convenience: no flush-and-retry for it)
        std::lock_guard<std::mutex> lk(g_pool.mu);
        g_pool_capacity[p] = bytes;
        g_pool_stats[std::make_pair(device, bytes)].total += 1;
        g_pool.idle.insert(std::make_pair(std::make_pair(device, bytes), p)); g_pool.held[device] += bytes;
    }
}
void helm_pool_free(int device, void *p, size_t bytes) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_pool.mu);
        auto ic = g_pool_capacity.find(p);
        if (ic != g_pool_capacity.end()) bytes = ic->second;            // (a buffer that did not come from the pool is taken in under the size the caller states)
        else g_pool_capacity[p] = bytes;
        if (bytes >= kSpareMin) { auto is = g_pool_stats.find(std::make_pair(device, bytes)); if (is != g_pool_stats.end() && is->second.in_use > 0) is->second.in_use -= 1; }
        const size_t cap = pool_cap_bytes(device);
        size_t &held = g_pool.held[device];
        if (g_carved.count(p) || (bytes >= kPoolMinBytes && (held + bytes <= cap || bytes < ((size_t)1 << 20)))) {
            g_pool.idle.insert(std::make_pair(std::make_pair(device, bytes), p)); held += bytes;
            return;
        }
        g_pool_capacity.erase(p);
        if (bytes >= kSpareMin) { auto is = g_pool_stats.find(std::make_pair(device, bytes)); if (is != g_pool_stats.end() && is->second.total > 0) is->second.total -= 1; }
    }
    AllocTrace tr("pool hipFree", bytes);
    hipFree(p);
}

// Scratch of a factorisation that helm_prefactor[_many] has enqueued goes back to the pool when the factorisation has FINISHED on the GPU, not when its operator
// is first solved with: a set is factored long before its turn in the pipeline comes, and held until then the scratch of four sets (4 GB each at 1024^2 x 2) was
// alive at once.  An event recorded behind the factorisation; every later prefactor / retire on the device looks which ones have completed.
namespace {
struct PendingScratch { int device; hipEvent_t ev; void *ws; size_t bytes; };
std::mutex g_ps_mu;
std::vector<PendingScratch> g_pending_scratch;
}
void scratch_sweep(int device, bool wait) {
    std::vector<PendingScratch> done;
    {
        std::lock_guard<std::mutex> lk(g_ps_mu);
        for (size_t i = 0; i < g_pending_scratch.size(); ) {
            PendingScratch &ps = g_pending_scratch[i];
            bool fin = false;
            if (ps.device == device) {
                if (wait) { (void)hipEventSynchronize(ps.ev); fin = true; }
                else { const hipError_t q = hipEventQuery(ps.ev); if (q == hipSuccess) fin = true; else (void)hipGetLastError(); }
            }
            if (fin) { done.push_back(ps); g_pending_scratch.erase(g_pending_scratch.begin() + i); } else ++i;
        }
    }
    for (PendingScratch &ps : done) { hipEventDestroy(ps.ev); helm_pool_free(ps.device, ps.ws, ps.bytes); }
}
void scratch_sweep_all_wait() {
    std::vector<int> devs;
    { std::lock_guard<std::mutex> lk(g_ps_mu); for (const PendingScratch &ps : g_pending_scratch) devs.push_back(ps.device); }
    for (int d : devs) { hipSetDevice(d); scratch_sweep(d, true); }
}
// ws is handed over: released behind everything enqueued on `st` so far (at once if no event can be had)
void scratch_defer(int device, hipStream_t st, void *ws, size_t bytes) {
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, st) != hipSuccess) {
        (void)hipGetLastError();
        if (ev) hipEventDestroy(ev);
        hipStreamSynchronize(st);
        helm_pool_free(device, ws, bytes);
        return;
    }
    std::lock_guard<std::mutex> lk(g_ps_mu);
    g_pending_scratch.push_back(PendingScratch{device, ev, ws, bytes});
}

// Release what the library caches between calls (the shared scratch of the direct path).  The scratch is kept across
// handles on purpose -- allocating tens of GB costs far more than a solve -- so a host that wants the memory back says so.
extern "C" int helm_pool_spares(int device, int spare) {
    helm_tuning_refresh();
    if (spare < 0) return HELM_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); helm_set_error(nullptr, "helm_pool_spares: hipSetDevice failed"); return HELM_ERR_DEVICE; }
    scratch_sweep(device, false);
    if (spare > 0) helm_pool_top_up(device, spare);
    return HELM_OK;
}
extern "C" int helm_trim(void) {
    helm_tuning_refresh();
    int cur = 0;
    (void)hipGetDevice(&cur);
    scratch_sweep_all_wait();
    {
        std::lock_guard<std::mutex> lk(g_shared_ws.mu);
        for (auto &kv : g_shared_ws.dev) for (int i = 0; i < WS_SLOTS_MAX; ++i) if (kv.second.slot[i].busy) return HELM_ERR_STATE;
        for (auto &kv : g_shared_ws.dev)
            for (int i = 0; i < WS_SLOTS_MAX; ++i) {
                WsSlot &w = kv.second.slot[i];
                if (w.ptr) { hipSetDevice(kv.first); hipFree(w.ptr); }
                w.ptr = nullptr; w.bytes = 0;
            }
        std::lock_guard<std::mutex> lp(g_pool.mu);
        std::map<int, size_t> kept;
        for (auto it = g_pool.idle.begin(); it != g_pool.idle.end(); ) {
            if (g_carved.count(it->second)) { kept[it->first.first] += it->first.second; ++it; continue; }       // (pieces of a slab stay idle: slabs live as long as the process)
            hipSetDevice(it->first.first); hipFree(it->second); pool_forget(it->second);
            it = g_pool.idle.erase(it);
        }
        g_pool.held = kept;
        for (auto &kv : g_pool_stats) { kv.second.total = kv.second.in_use; kv.second.high = kv.second.in_use; }
    }
    (void)hipSetDevice(cur);
    return helm_host_trim();
}

// (tests) how many scratch slots of `device` hold a buffer of at least `bytes`; -1: the number of slots per device
extern "C" int helm_debug_ws_slots(int device, long long bytes) {
    helm_tuning_refresh();
    if (device < 0) return shared_ws_slots();
    std::lock_guard<std::mutex> lk(g_shared_ws.mu);
    auto it = g_shared_ws.dev.find(device);
    if (it == g_shared_ws.dev.end()) return 0;
    int n = 0;
    for (int i = 0; i < WS_SLOTS_MAX; ++i) if (it->second.slot[i].ptr && (long long)it->second.slot[i].bytes >= bytes) n += 1;
    return n;
}

// Host array -> device through pinned buffers of the library (two chunks of 4 MB from the host pool: the memcpy of chunk k+1 runs beside the DMA of chunk k); the
// caller's pages are never handed to the runtime.  A copy of a few MB straight from pageable memory makes HIP pin the caller's pages in place (a user-pointer
// registration); when those pages go back to the system afterwards -- numpy frees an array of that size with munmap -- the kernel driver takes EVERY queue of the
// process off the GPU while it deals with the registration: 15-20 ms in which nothing of this process runs, charged to whatever is submitted next (round 6:
// one dpred(m) of config 4 in three took 55-65 ms instead of 39; with glibc told never to unmap, none did -- profiles/r06_config4_dpred_spread.txt).
namespace {
std::mutex g_upload_mu;
std::map<int, std::vector<hipEvent_t>> g_upload_events;              // per device, recycled (an event per chunk buffer of an upload in flight)
}
// is this host address memory the runtime already knows as pinned (hipHostMalloc / hipHostRegister, the library's own host pool included)?
static bool host_ptr_is_pinned(const void *p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}
// One direction of a staged copy: `up` host -> device, else device -> host; returns when the data is where it was asked to be.
static int copy_staged(helm_op *op, void *dst, const void *src, size_t bytes, bool up) {
    const size_t chunk = (size_t)4 << 20;
    if (bytes == 0) return HELM_OK;
    // The copies run on a stream of another priority class (xs; the low one, which the 2-D path uses for nothing else), not on the operator's: the copy of a chunk is a small kernel (or an SDMA packet behind one), and
    // on the operator's normal-priority stream it waited its turn behind the solve kernels of other operators -- a 24-MB model took 10 ms of the pipeline's prepare
    // thread in every other set (tools/pipeline_timeline.py).  The call returns when the data has arrived, so nothing the operator's stream gets afterwards can
    // overtake it; what that stream has queued BEFORE the call is waited for first (a download reads what those launches produce).
    hipStream_t ops = op->stream;
    if (hipStreamSynchronize(ops) != hipSuccess) { (void)hipGetLastError(); helm_set_error(op, "host / device copy failed"); return HELM_ERR_DEVICE; }
    static const int xprio = getenv("HELM_XFER_PRIO") ? atoi(getenv("HELM_XFER_PRIO")) : -1;
    hipStream_t xs = helm_stream_acquire(op->device, xprio);
    if (!xs) { helm_set_error(op, "host / device copy: no stream"); return HELM_ERR_DEVICE; }
    struct XsGuard { int dev, prio; hipStream_t s; ~XsGuard() { helm_stream_release(dev, prio, s); } } xs_guard{op->device, xprio, xs};
    if (host_ptr_is_pinned(up ? src : dst)) {                     // nothing to protect: the runtime moves it straight
        if (hipMemcpyAsync(dst, src, bytes, up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, xs) != hipSuccess || hipStreamSynchronize(xs) != hipSuccess) {
            (void)hipGetLastError(); helm_set_error(op, "host / device copy failed"); return HELM_ERR_DEVICE;
        }
        return HELM_OK;
    }
    const int nbuf = bytes > chunk ? 2 : 1;
    char *buf[2] = {(char *)helm_hostpool_alloc(chunk), nbuf > 1 ? (char *)helm_hostpool_alloc(chunk) : nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    {
        std::lock_guard<std::mutex> lk(g_upload_mu);
        std::vector<hipEvent_t> &v = g_upload_events[op->device];
        for (int b = 0; b < nbuf; ++b) if (!v.empty()) { ev[b] = v.back(); v.pop_back(); }
    }
    int rc = HELM_OK;
    for (int b = 0; b < nbuf; ++b) {
        if (!buf[b]) rc = HELM_ERR_DEVICE;
        if (!ev[b] && hipEventCreateWithFlags(&ev[b], hipEventDisableTiming) != hipSuccess) { ev[b] = nullptr; rc = HELM_ERR_DEVICE; }
    }
    bool used[2] = {false, false};
    size_t pend_off[2] = {0, 0}, pend_n[2] = {0, 0};             // (down: the chunk that sits in buf[b] and still has to reach the caller's array)
    for (size_t off = 0, k = 0; off < bytes && rc == HELM_OK; off += chunk, ++k) {
        const int b = (int)(k % nbuf);
        const size_t n = std::min(chunk, bytes - off);
        if (used[b]) {
            if (hipEventSynchronize(ev[b]) != hipSuccess) { rc = HELM_ERR_DEVICE; break; }
            if (!up) memcpy((char *)dst + pend_off[b], buf[b], pend_n[b]);
        }
        if (up) memcpy(buf[b], (const char *)src + off, n);
        const hipError_t e = up ? hipMemcpyAsync((char *)dst + off, buf[b], n, hipMemcpyHostToDevice, xs)
                                : hipMemcpyAsync(buf[b], (const char *)src + off, n, hipMemcpyDeviceToHost, xs);
        if (e != hipSuccess || hipEventRecord(ev[b], xs) != hipSuccess) { rc = HELM_ERR_DEVICE; break; }
        used[b] = true; pend_off[b] = off; pend_n[b] = n;
    }
    // (the chunks still in flight, oldest first)
    const size_t nchunks = (bytes + chunk - 1) / chunk;
    for (int q = 0; q < nbuf; ++q) {
        const int b = (int)((nchunks + q) % nbuf);
        if (used[b]) {
            if (hipEventSynchronize(ev[b]) != hipSuccess) rc = HELM_ERR_DEVICE;
            else if (!up && rc == HELM_OK) memcpy((char *)dst + pend_off[b], buf[b], pend_n[b]);
            used[b] = false;
        }
    }
    for (int b = 0; b < nbuf; ++b) if (buf[b]) helm_hostpool_free(buf[b], chunk);
    {
        std::lock_guard<std::mutex> lk(g_upload_mu);
        for (int b = 0; b < nbuf; ++b) if (ev[b]) g_upload_events[op->device].push_back(ev[b]);
    }
    if (rc) { (void)hipGetLastError(); helm_set_error(op, "host / device copy failed"); }
    return rc;
}
int helm_upload_staged(helm_op *op, void *dst, const void *src, size_t bytes) { return copy_staged(op, dst, src, bytes, true); }
int helm_download_staged(helm_op *op, void *dst, const void *src, size_t bytes) { return copy_staged(op, dst, src, bytes, false); }

// the slot table's two operations, over any table and allocator (the library's own: g_shared_ws with hipMalloc; helm_debug_ws_selftest: a
// scratch table with malloc, so that the booking logic is testable without a GPU)
typedef void *(*ws_alloc_fn)(int device, size_t bytes);
typedef void (*ws_free_fn)(int device, void *p);
static void *ws_dev_alloc(int device, size_t bytes) { void *p = nullptr; AllocTrace tr("ws slot alloc", bytes); (void)helm_malloc_retry(device, &p, bytes); return p; }
static void ws_dev_free(int, void *p) { hipFree(p); }
// an idle slot of `device` that is already big enough, else any idle one (grown to `bytes`); nullptr when every slot of the device is taken or
// the allocation fails.  *lease = device * WS_SLOTS_MAX + slot.
static void *ws_table_checkout(SharedWs &T, int device, size_t bytes, int *lease, ws_alloc_fn al, ws_free_fn fr) {
    std::lock_guard<std::mutex> lk(T.mu);
    const int ns = shared_ws_slots();
    WsDevice &D = T.dev[device];
    int pick = -1;
    for (int i = 0; i < ns; ++i) { WsSlot &w = D.slot[i]; if (!w.busy && w.ptr && w.bytes >= bytes) { pick = i; break; } }
    if (pick < 0) for (int i = 0; i < ns; ++i) { WsSlot &w = D.slot[i]; if (!w.busy) { pick = i; break; } }
    if (pick < 0) return nullptr;
    WsSlot &w = D.slot[pick];
    if (w.bytes < bytes) {
        if (w.ptr) fr(device, w.ptr);
        w.ptr = al(device, bytes);
        w.bytes = w.ptr ? bytes : 0;
    }
    if (!w.ptr) return nullptr;
    w.busy = true; *lease = device * WS_SLOTS_MAX + pick;
    return w.ptr;
}
static void ws_table_checkin(SharedWs &T, int lease) {
    if (lease < 0) return;
    std::lock_guard<std::mutex> lk(T.mu);
    T.dev[lease / WS_SLOTS_MAX].slot[lease % WS_SLOTS_MAX].busy = false;
}
// make sure `concurrent` slots of `device` hold at least `bytes` each (idle slots that are too small are re-allocated; another device's table is
// never touched); returns the number of slots that are ready
static int ws_table_reserve(SharedWs &T, int device, size_t bytes, int concurrent, ws_alloc_fn al, ws_free_fn fr) {
    std::lock_guard<std::mutex> lk(T.mu);
    const int ns = shared_ws_slots();
    WsDevice &D = T.dev[device];
    int ready = 0;
    for (int i = 0; i < ns; ++i) { const WsSlot &w = D.slot[i]; if (w.ptr && w.bytes >= bytes) ready += 1; }
    for (int i = 0; i < ns && ready < concurrent; ++i) {
        WsSlot &w = D.slot[i];
        if (w.busy || (w.ptr && w.bytes >= bytes)) continue;
        if (w.ptr) { fr(device, w.ptr); w.ptr = nullptr; w.bytes = 0; }
        w.ptr = al(device, bytes);
        if (!w.ptr) break;
        w.bytes = bytes; ready += 1;
    }
    return ready;
}

void *ws_checkout(int device, size_t bytes, int *slot_out) { return ws_table_checkout(g_shared_ws, device, bytes, slot_out, ws_dev_alloc, ws_dev_free); }
void ws_checkin(int slot) { ws_table_checkin(g_shared_ws, slot); }
int ws_reserve(int device, size_t bytes, int concurrent) { return ws_table_reserve(g_shared_ws, device, bytes, concurrent, ws_dev_alloc, ws_dev_free); }

// (tests, no GPU needed) the slot table with `ndev` logical devices and host memory: every device books `concurrent` slots of `bytes`, then
// `concurrent` leases are taken on every device at once.  Returns 0 when every lease is a booked slot of its own device, no lease needed a
// new allocation, one lease more than the table has slots is refused, and a device's bookings survive the other devices' bookings; a negative
// code says which of these failed.
static int g_selftest_allocs = 0;
static void *ws_host_alloc(int, size_t bytes) { g_selftest_allocs += 1; return malloc(bytes); }
static void ws_host_free(int, void *p) { free(p); }
extern "C" int helm_debug_ws_selftest(int ndev, int concurrent, long long bytes) {
    helm_tuning_refresh();
    if (ndev < 1 || concurrent < 1 || bytes < 1) return HELM_ERR_ARG;
    SharedWs T;
    int rc = 0;
    const int ns = shared_ws_slots();
    const int want = std::min(concurrent, ns);
    g_selftest_allocs = 0;
    for (int d = 0; d < ndev; ++d) if (ws_table_reserve(T, d, (size_t)bytes, concurrent, ws_host_alloc, ws_host_free) != want) rc = -1;
    if (g_selftest_allocs != ndev * want) rc = rc ? rc : -2;
    std::vector<int> leases;
    std::vector<void *> ptrs;
    for (int d = 0; d < ndev && !rc; ++d)
        for (int k = 0; k < want; ++k) {
            int lease = -1;
            void *p = ws_table_checkout(T, d, (size_t)bytes, &lease, ws_host_alloc, ws_host_free);
            if (!p || lease / WS_SLOTS_MAX != d) { rc = -3; break; }
            for (void *q : ptrs) if (q == p) rc = -4;                   // two leases on one buffer
            leases.push_back(lease); ptrs.push_back(p);
        }
    if (!rc && g_selftest_allocs != ndev * want) rc = -5;              // a lease after the booking allocated
    if (!rc && want == ns) { int lease = -1; if (ws_table_checkout(T, 0, (size_t)bytes, &lease, ws_host_alloc, ws_host_free)) rc = -6; }   // all of device 0's slots are out
    for (int l : leases) ws_table_checkin(T, l);
    if (!rc) { int lease = -1; if (!ws_table_checkout(T, ndev - 1, (size_t)bytes / 2 + 1, &lease, ws_host_alloc, ws_host_free) || g_selftest_allocs != ndev * want) rc = -7; else ws_table_checkin(T, lease); }
    for (auto &kv : T.dev) for (int i = 0; i < WS_SLOTS_MAX; ++i) if (kv.second.slot[i].ptr) free(kv.second.slot[i].ptr);
    return rc;
}
