// Host-side helpers shared by the hipt_*_launch functions: the per-device one-time setup of a kernel family, the zeroing of a
// tile queue, and (diagnostic builds only) the buffer behind the in-kernel time stamps.
#pragma once
#include <atomic>
#include <initializer_list>

#include "common.h"

// hipFuncSetAttribute (the > 64 KiB dynamic-LDS opt-in) is a PER-DEVICE setting and a process may drive several GPUs (HIPT_4K's
// device256 != device4k placement, a module on cuda:1 while cuda:0 is current), from several threads (nn.DataParallel): a launcher
// keeps one `static DeviceSetup` per kernel family -- per instantiation where the launcher is a template -- and calls it once per launch.
// The first call on a device opts every kernel of the family into `lds` bytes of dynamic LDS (0: no opt-in) and reads the device's CU
// count; every later one is hipGetDevice and one load.
// Threading: the CU count IS the done flag -- 0 until the setup has succeeded, then stored with release order and loaded with acquire
// order, so a thread that sees the device done sees its count and the attributes set before it.  Two threads that arrive first
// together both run the setup; it is idempotent.  A failed setup stores nothing: the next launch tries again.
constexpr int HIPT_MAX_DEV = 64;
class DeviceSetup {
    std::atomic<int> ncu_[HIPT_MAX_DEV] = {};

public:
    // HIPT_OK and the current device's CU count in *ncu (where asked for), or HIPT_E_LAUNCH with the error text set
    int operator()(std::initializer_list<const void*> kernels, int lds, const char* name, int* ncu = nullptr) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= HIPT_MAX_DEV) {
            hipt_set_error("%s: hipGetDevice failed", name);
            return HIPT_E_LAUNCH;
        }
        int n = ncu_[dev].load(std::memory_order_acquire);
        if (n == 0) {
            if (lds > 0)
                for (const void* k : kernels)
                    if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) {
                        hipt_set_error("hipFuncSetAttribute(%s) failed", name);
                        return HIPT_E_LAUNCH;
                    }
            if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
                hipt_set_error("%s: cannot query the device", name);
                return HIPT_E_LAUNCH;
            }
            ncu_[dev].store(n, std::memory_order_release);
        }
        if (ncu) *ncu = n;
        return HIPT_OK;
    }
};

// The tile queue of a persistent kernel starts at zero: one 4-byte memset on the launch's stream, unless the caller guarantees it
// (`zeroed`: a chain of launches whose kernels each leave the counter at zero again -- kernels.h, counter_zeroed).
inline int hipt_zero_queue(int* counter, bool zeroed, hipStream_t st, const char* name) {
    if (!zeroed && hipMemsetAsync(counter, 0, sizeof(int), st) != hipSuccess) {
        hipt_set_error("%s: hipMemsetAsync(counter) failed", name);
        return HIPT_E_LAUNCH;
    }
    return HIPT_OK;
}

// In-kernel time stamps, ROWS workgroups x SLOTS stamps each (diagnostic builds only: make DEBUG_STAMPS=1 -> libhipt_abmil_dbg.so; the
// release library never allocates and never synchronises).  A launcher keeps one `static StampBuffer<..> stamps("HIPT_..._STAMPS")`;
// with that environment variable unset both calls return nullptr and touch nothing.
#ifdef HIPT_DEBUG_STAMPS
template <int ROWS, int SLOTS>
class StampBuffer {
    const bool on_;
    unsigned long long* dev_ = nullptr;
    unsigned long long host_[ROWS * SLOTS];

public:
    explicit StampBuffer(const char* env) : on_(getenv(env) != nullptr) {}
    // before the launch: the device buffer, zeroed on `st`, for the kernel's `stamps` argument
    unsigned long long* arm(hipStream_t st) {
        if (!on_) return nullptr;
        if (!dev_) (void)hipMalloc(&dev_, sizeof(host_));
        (void)hipMemsetAsync(dev_, 0, sizeof(host_), st);
        return dev_;
    }
    // after the launch: waits for `st` and returns the stamps of the `grid` workgroups, row-major (nullptr where grid > ROWS)
    const unsigned long long* read(int grid, hipStream_t st) {
        if (!on_ || grid > ROWS) return nullptr;
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(host_, dev_, (size_t)grid * SLOTS * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        return host_;
    }
};
#endif
