// qps_runtime.hip -- what every handle of libqps_hip draws on besides its own data: the per-device pools (a stream, a pinned read-back block and a device block
// per dense handle; the pinned rings of the uploaders), the host thread count of the boundary's hand-over, the per-ordinal device queries, and the launch-timing
// scope of the profiler.  No solver and no entry point lives here.
#include <atomic>
#include <thread>

#include "qps_internal.h"
#include "qps_kernels.h"

namespace qps {
namespace {
constexpr size_t kRecycleBlockMax = (size_t)512 << 20;   // blocks above 512 MiB go back to the driver (at most 4 x that per device stay cached, of 288 GB)
constexpr int kRecyclePerDevice = 4;
std::mutex g_res_mu;
std::vector<HandleResources> g_res[kMaxDevices];
std::atomic<int> g_cus[kMaxDevices];   // 0 = not asked yet
}  // namespace
int current_device() { int dev = 0; if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; } return dev; }
int device_cu_count(int device) {
    if (device < 0 || device >= kMaxDevices) return 0;
    int c = g_cus[device].load(std::memory_order_acquire);
    if (c == 0) {
        if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) { (void)hipGetLastError(); c = -1; }
        g_cus[device].store(c, std::memory_order_release);
    }
    return c > 0 ? c : 0;
}
HandleResources acquire_resources(int device, size_t block_need) {
    HandleResources r;
    {
        std::lock_guard<std::mutex> lk(g_res_mu);
        if (device >= 0 && device < kMaxDevices && !g_res[device].empty()) { r = g_res[device].back(); g_res[device].pop_back(); }
    }
    try {
        if (!r.st) HIPC(hipStreamCreateWithFlags(&r.st, hipStreamNonBlocking));
        if (!r.pinned) HIPC(hipHostMalloc(&r.pinned, kPinnedBytes));
    } catch (...) { recycle_resources(device, r); throw; }   // (an entry without a pinned block is completed by its next user)
    if (r.block && (r.block_bytes < block_need || r.block_bytes > 4 * block_need + ((size_t)1 << 20))) { (void)hipFree(r.block); r.block = nullptr; r.block_bytes = 0; }
    return r;
}
void recycle_resources(int device, HandleResources r) {
    if (r.block && r.block_bytes > kRecycleBlockMax) { (void)hipFree(r.block); r.block = nullptr; r.block_bytes = 0; }
    {
        std::lock_guard<std::mutex> lk(g_res_mu);
        if (device >= 0 && device < kMaxDevices && (int)g_res[device].size() < kRecyclePerDevice) { g_res[device].push_back(r); return; }
    }
    if (r.block) (void)hipFree(r.block);
    if (r.pinned) (void)hipHostFree(r.pinned);
    if (r.st) (void)hipStreamDestroy(r.st);
}
int host_threads() {
    static const int n = [] {
        const char* e = getenv("QPS_HOST_THREADS");
        const int hw = (int)std::max(1u, std::thread::hardware_concurrency());
        return std::max(1, std::min(e ? atoi(e) : 8, hw));
    }();
    return n;
}
namespace {
constexpr size_t kRingHalf = (size_t)32 << 20;
std::vector<PinnedRing> g_rings[kMaxDevices];
}  // namespace
PinnedRing acquire_ring(int device) {
    PinnedRing r;
    {
        std::lock_guard<std::mutex> lk(g_res_mu);
        if (device >= 0 && device < kMaxDevices && !g_rings[device].empty()) { r = g_rings[device].back(); g_rings[device].pop_back(); }
    }
    if (!r.base) { HIPC(hipHostMalloc((void**)&r.base, 2 * kRingHalf)); r.half = kRingHalf; }
    return r;
}
void recycle_ring(int device, PinnedRing r) {
    if (!r.base) return;
    {
        std::lock_guard<std::mutex> lk(g_res_mu);
        if (device >= 0 && device < kMaxDevices && (int)g_rings[device].size() < kRecyclePerDevice) { g_rings[device].push_back(r); return; }
    }
    (void)hipHostFree(r.base);
}
thread_local LaunchTiming g_launch_timing;
ProfLaunchScope::ProfLaunchScope(Profiler& pr, int c, int lvl) : p(pr), cat(c), a(nullptr), b(nullptr), active(pr.on(lvl)) {
    if (active) { a = p.get(); b = p.get(); g_launch_timing.start = a; g_launch_timing.stop = b; }
}
ProfLaunchScope::~ProfLaunchScope() {
    if (!active) return;
    const bool consumed = (g_launch_timing.start == nullptr);
    g_launch_timing = LaunchTiming();
    if (consumed) p.pending.push_back({cat, a, b}); else { p.pool.push_back(a); p.pool.push_back(b); }
}
}  // namespace qps
