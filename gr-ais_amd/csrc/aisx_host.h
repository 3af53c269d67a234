// aisx_host.h -- host-side helpers shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <utility>

#include "../../include/aisx.h"
#include "aisx_common.h"

namespace aisx {

static_assert(sizeof(tag_rec) == sizeof(aisx_tag), "tag layout");
static_assert(sizeof(cf) == sizeof(aisx_cf32), "complex layout");

char* err_buf(); // thread-local message buffer (aisx_lib.hip)

inline void set_err(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
}

#define AISX_HIPCHK(expr)                                                                      \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess) {                                                               \
            ::aisx::set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return AISX_ERR_HIP;                                                               \
        }                                                                                      \
    } while (0)

// Experiment knobs.  The product library reads NO environment variable: its behaviour is what the API was told.
// A build made with -DAISX_EXPERIMENTS (lib/libaisx_exp.so: tools/ab_*, the profiling scripts, the tests of the
// alternative kernels) answers these look-ups from the environment; in the product build they fold to "unset".
inline const char* exp_env(const char* name)
{
#ifdef AISX_EXPERIMENTS
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

inline int require_device()
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_err("no HIP device available (libaisx has no CPU fallback)");
        return AISX_ERR_NO_DEVICE;
    }
    return AISX_OK;
}

// The dynamic-LDS limit hipFuncSetAttribute sets belongs to a kernel on a device, not to a handle: handles of one kernel
// that ask for different sizes (template lengths, placement claims) share it, and one that set it lower than another
// had raised it would make that one's next launch ask for more than the limit.  ensure_dyn_lds raises the current
// device's limit for `kernel` to at least `bytes` and never lowers it: one record per (device, kernel), starting at
// the runtime's 64 KB default, behind a mutex (handles are driven from several host threads).  A size above the
// device's LDS per CU is refused (AISX_ERR_INVALID, `who` in the message) and nothing is set.
inline int ensure_dyn_lds(const void* kernel, int bytes, const char* who)
{
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, int> raised; // (device, kernel) -> limit set so far
    static std::map<int, int> lds_cu;                         // device -> hipDeviceProp_t::maxSharedMemoryPerMultiProcessor
    int dev = 0;
    AISX_HIPCHK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    auto d = lds_cu.find(dev);
    if (d == lds_cu.end()) {
        hipDeviceProp_t prop;
        AISX_HIPCHK(hipGetDeviceProperties(&prop, dev));
        d = lds_cu.emplace(dev, (int)prop.maxSharedMemoryPerMultiProcessor).first;
    }
    if (bytes > d->second) {
        set_err("%s: a workgroup would need %d bytes of LDS, device %d has %d per CU", who, bytes, dev, d->second);
        return AISX_ERR_INVALID;
    }
    int& limit = raised.emplace(std::make_pair(dev, kernel), 64 * 1024).first->second;
    if (bytes > limit) {
        AISX_HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        limit = bytes;
    }
    return AISX_OK;
}

template <class T>
inline int dev_alloc(T** p, size_t count, bool zero = true)
{
    *p = nullptr;
    size_t bytes = sizeof(T) * (count ? count : 1);
    AISX_HIPCHK(hipMalloc((void**)p, bytes));
    if (zero)
        AISX_HIPCHK(hipMemset(*p, 0, bytes));
    return AISX_OK;
}

template <class T>
inline void dev_free(T*& p)
{
    if (p)
        (void)hipFree(p);
    p = nullptr;
}

// a handle's calls run on the device that was current when it was created, and leave the caller's current
struct OnDevice {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit OnDevice(int dev)
    {
        if ((err = hipGetDevice(&prev)) == hipSuccess && prev != dev)
            err = hipSetDevice(dev);
    }
    ~OnDevice()
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev)
            (void)hipSetDevice(prev);
    }
};

} // namespace aisx
