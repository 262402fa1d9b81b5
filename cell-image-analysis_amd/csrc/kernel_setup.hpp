// kernel_setup.hpp -- what a launcher has to do and know about one kernel on one device, done once per (kernel, device): the
// opt-in to its dynamic LDS size, the device's CU count, and how many of its workgroups the device holds at once (CUs x
// resident workgroups per CU for the kernel's registers and LDS).  A persistent grid is min(work, resident) -- a larger grid
// would queue the surplus behind the first wave of workgroups and run it at a fraction of the occupancy -- or min(work, CUs)
// for the LDS-bound kernels that run one workgroup per CU.
// Also the cycle-stamp tables of the kernels' DIAG builds (allocated on the same once-per-device path) and their reader.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <vector>

namespace cs {

constexpr int MAX_DEVICES = 64;

struct KernelSetup { int device, cus, resident; };

// Diagnostic builds only: `words` 64-bit cycle sums per workgroup (waves x phases), one buffer per device, sized for the
// largest grid of the kernel that fills it.
struct StampTable {
    int words;
    unsigned long long* buf[MAX_DEVICES];
    int groups[MAX_DEVICES];                 // workgroups of the last stamped launch
    unsigned long long* begin(const KernelSetup& ks, unsigned grid) { groups[ks.device] = (int)grid; return buf[ks.device]; }
};

struct KernelSetupSlot { std::atomic<bool> ready; int cus, resident; };

inline hipError_t kernel_setup_once(const void* kernel, int threads, int lds, int dev, KernelSetupSlot& s, StampTable* stamps)
{
    static std::mutex mu;                    // one for every kernel: this runs once per (kernel, device)
    std::lock_guard<std::mutex> lock(mu);
    if (s.ready.load(std::memory_order_relaxed)) return hipSuccess;
    int cus = 0, per_cu = 0;
    hipError_t e;
    if ((e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds)) != hipSuccess) return e;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds)) != hipSuccess) return e;
    if (cus < 1) cus = 1;
    if (per_cu < 1) per_cu = 1;
    if (stamps && !stamps->buf[dev]) {
        e = hipMalloc(&stamps->buf[dev], (size_t)cus * per_cu * stamps->words * sizeof(unsigned long long));
        if (e != hipSuccess) return e;
    }
    s.cus = cus;
    s.resident = cus * per_cu;
    s.ready.store(true, std::memory_order_release);
    return hipSuccess;
}

// Keyed by the CURRENT device; safe when threads make the first call together; afterwards a call costs hipGetDevice.
template <auto Kernel>
hipError_t kernel_setup(int threads, int lds, KernelSetup& ks, StampTable* stamps = nullptr)
{
    static KernelSetupSlot slots[MAX_DEVICES];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= MAX_DEVICES) return hipErrorInvalidDevice;
    KernelSetupSlot& s = slots[dev];
    if (!s.ready.load(std::memory_order_acquire) &&
        (e = kernel_setup_once((const void*)Kernel, threads, lds, dev, s, stamps)) != hipSuccess)
        return e;
    ks = KernelSetup{dev, s.cus, s.resident};
    return hipSuccess;
}

// The stamps of the last launch into `t` on the current device, averaged over its waves: out[k] for k < phases (`words` is a
// multiple of phases).  0, or -1 no stamped launch yet, -2 the device failed to synchronise, -3 the copy failed.
inline int stamp_table_average(const StampTable& t, int phases, double* out)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES || !t.buf[dev] || t.groups[dev] < 1) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -2;
    std::vector<unsigned long long> h((size_t)t.groups[dev] * t.words);
    if (hipMemcpy(h.data(), t.buf[dev], h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -3;
    for (int k = 0; k < phases; ++k) out[k] = 0.0;
    for (size_t i = 0; i < h.size(); ++i) out[i % phases] += (double)h[i];
    for (int k = 0; k < phases; ++k) out[k] /= (double)(h.size() / phases);
    return 0;
}

}  // namespace cs
