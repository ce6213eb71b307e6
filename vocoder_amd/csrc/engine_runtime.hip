// The process-wide runtime state of libfishvoc_hip.so: error text, last kernel, experiment knobs, the conv-algorithm scope, the per-thread
// profiler hook — what the kernel units reach through fv_internal.h — and the ABI entries that expose it.
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <string>

#include "engine_internal.h"

namespace fv {

static thread_local std::string g_err;
static thread_local std::string g_kernel;

void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}
void set_last_kernel(const char* name) { g_kernel = name; }
static thread_local bool g_lds_refused = false;
bool dynamic_lds_refused() {   // true once after a failed ensure_dynamic_lds (lets the caller keep that error text)
    const bool r = g_lds_refused;
    g_lds_refused = false;
    return r;
}
bool ensure_dynamic_lds(const void* kernel, int bytes, unsigned long long* done_mask) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && dev >= 0 && dev < 64 && (__atomic_load_n(done_mask, __ATOMIC_ACQUIRE) >> dev & 1ull)) return true;
    if (e == hipSuccess) e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) {
        set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize = %d B) failed on device %d: %s", bytes, dev, hipGetErrorString(e));
        g_lds_refused = true;
        return false;
    }
    if (dev >= 0 && dev < 64) __atomic_fetch_or(done_mask, 1ull << dev, __ATOMIC_RELEASE);   // devices >= 64: set every time
    return true;
}
// The knob set is immutable once published: knobs() is one acquire load on the launch path, fv_reload_env() publishes a fresh
// copy (the old one is leaked on purpose — a concurrent forward may still be reading it; a harness reloads a handful of times)
static std::atomic<const Knobs*> g_knobs{nullptr};
static std::once_flag g_knobs_once;
static const Knobs* load_knobs() {
    Knobs* k = new Knobs();
    if (const char* v = std::getenv("FV_PW")) {
        const int n = std::atoi(v);
        k->pw = (v[0] == 'o' || n < 0 || n >= GEMM_PW_COUNT) ? -1 : n;
    }
    if (const char* v = std::getenv("FV_PW_PX")) k->pw_px = std::atoi(v);
    k->dwln_ng8 = std::getenv("FV_DWLN_NG8") != nullptr;
    k->dwln_rr = std::getenv("FV_DWLN_RR") != nullptr;
    k->old_dwln = std::getenv("FV_OLD_DWLN") != nullptr;
    if (const char* v = std::getenv("FV_WINO")) k->wino = std::atoi(v);
    if (const char* v = std::getenv("FV_WINO_MIN_M")) k->wino_min_m = std::atoi(v);
    if (const char* v = std::getenv("FV_WINO_CFG")) k->wino_cfg = std::atoi(v);
    if (const char* v = std::getenv("FV_WINO_MIN_BLOCKS")) k->wino_min_blocks = std::atoi(v);
    if (const char* v = std::getenv("FV_PAIR_WINO")) k->pair_wino = std::atoi(v);
    if (const char* v = std::getenv("FV_WINO4")) k->wino4 = std::atoi(v);
    if (const char* v = std::getenv("FV_WINO44")) k->wino44 = std::atoi(v);
    if (const char* v = std::getenv("FV_WINO44_ROWS")) k->wino44_rows = std::atoi(v);
    if (const char* v = std::getenv("FV_WINO_LAT")) k->wino_lat = std::atoi(v);
    if (const char* v = std::getenv("FV_LAT_WINO44")) k->lat_wino44 = std::atoi(v);
    if (const char* v = std::getenv("FV_SPLITK_DIRECT")) k->splitk_direct = std::atoi(v);
    if (const char* v = std::getenv("FV_WINO44_FLAT")) k->wino44_flat = std::atoi(v);
    if (const char* v = std::getenv("FV_VEC_STORE")) k->vec_store = std::atoi(v);
    if (const char* v = std::getenv("FV_PAIR_WINO44")) k->pair_wino44 = std::atoi(v);
    if (const char* v = std::getenv("FV_PAIR_WINO4")) k->pair_wino4 = std::atoi(v);
    if (const char* v = std::getenv("FV_CONV_TILE")) {
        k->conv_tile = conv_tile_by_name(v);
        if (k->conv_tile < 0 && v[0]) std::fprintf(stderr, "fishvoc: FV_CONV_TILE=%s names no conv tile; ignored\n", v);
    }
    if (const char* v = std::getenv("FV_X_UPS_TILE256")) k->ups_tile256 = std::atoi(v);
    k->no_sum3 = std::getenv("FV_NO_SUM3") != nullptr;
    if (const char* v = std::getenv("FV_BRANCH_MEAN")) k->branch_mean_chain = v[0] == 'c';
    if (const char* v = std::getenv("FV_SPLITK")) k->splitk = v[0] == '3' ? 32 : 64;
    if (const char* v = std::getenv("FV_SPLITK_MAX")) k->splitk_max = std::atoll(v);
    if (const char* v = std::getenv("FV_AA_VEC4")) k->aa_vec4 = v[0] != '0';
    k->no_f16x3_pairs = std::getenv("FV_NO_F16X3_PAIRS") != nullptr;
    k->w44_no_qr = std::getenv("FV_X_W44_NO_QR") != nullptr;
    return k;
}
const Knobs& knobs() {
    const Knobs* k = g_knobs.load(std::memory_order_acquire);
    if (!k) {
        std::call_once(g_knobs_once, [] { g_knobs.store(load_knobs(), std::memory_order_release); });
        k = g_knobs.load(std::memory_order_acquire);
    }
    return *k;
}
static void reload_knobs() {
    (void)knobs();   // (the first-use initialisation has happened: nothing can overwrite the copy published below)
    g_knobs.store(load_knobs(), std::memory_order_release);
}

static thread_local int g_algo = FV_CONV_ALGO_AUTO;
static thread_local bool g_invariant = false;
AlgoScope::AlgoScope(int algo, bool invariant) : prev_algo(g_algo), prev_inv(g_invariant) {
    g_algo = algo;
    g_invariant = invariant;
}
AlgoScope::~AlgoScope() {
    g_algo = prev_algo;
    g_invariant = prev_inv;
}
int cur_algo() { return g_algo; }
bool cur_invariant() { return g_invariant; }

int num_cus() {
    static thread_local int cached_dev = -1, cached = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev != cached_dev) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached = n;
        cached_dev = dev;
    }
    return cached;
}

static thread_local Profiler* g_prof = nullptr;
Profiler* current_profiler() { return g_prof; }
Profiler* set_profiler(Profiler* p) {
    Profiler* prev = g_prof;
    g_prof = p;
    return prev;
}
int prof_begin(hipStream_t s) {
    if (!g_prof) return -1;
    ProfRec r;
    if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return -1;
    (void)hipEventRecord(r.e0, s);
    g_prof->recs.push_back(r);
    return (int)g_prof->recs.size() - 1;
}
void prof_end(hipStream_t s, int idx, const char* label, double flops, double bytes) {
    if (!g_prof || idx < 0) return;
    ProfRec& r = g_prof->recs[idx];
    (void)hipEventRecord(r.e1, s);
    r.label = label;
    r.flops = flops;
    r.bytes = bytes;
}

}  // namespace fv

extern "C" {

FV_API void fv_reload_env(void) { fv::reload_knobs(); }
FV_API const char* fv_last_error(void) { return g_err.c_str(); }
FV_API int32_t fv_abi_version(void) { return FV_ABI_VERSION; }
FV_API const char* fv_last_kernel(void) { return g_kernel.c_str(); }

}  // extern "C"
