// aisx_host.h -- host-side helpers shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
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

// The same for what a launch plan's callable kept of hipGetLastError() behind the launch its sequence stopped at.
#define AISX_LAUNCHCHK(err)                                                                    \
    do {                                                                                       \
        if ((err) != hipSuccess) {                                                             \
            ::aisx::set_err("hipGetLastError() failed: %s (%s:%d)", hipGetErrorString(err), __FILE__, __LINE__); \
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

// ---- owners: what a handle holds is released when the handle is deleted (move-only; members are destroyed in
// reverse declaration order, so a handle declares its streams BEFORE the buffers and events used on them)
template <class T>
class DevBuf { // a hipMalloc block
    T* p_ = nullptr;
    size_t cap_ = 0; // elements asked for

public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
        o.reset();
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset()
    {
        dev_free(p_);
        cap_ = 0;
    }
    int alloc(size_t count, bool zero = true) // dev_alloc; whatever was held before is freed first
    {
        reset();
        const int rc = dev_alloc(&p_, count, zero);
        if (rc != AISX_OK)
            reset();
        else
            cap_ = count;
        return rc;
    }
    int alloc(const PlanBuf& b) { return alloc(b.n, b.zeroed); } // a buffer of a stage's launch plan
    // grow-only: nothing while `count` fits, else free and allocate ({nullptr, 0} is left behind on failure).  An empty
    // buffer allocates even for count == 0 (one element, as dev_alloc).  *fresh is set once it HAS allocated: the zero
    // fill runs on the null stream, the caller synchronises as it needs to
    int reserve(size_t count, bool zero = true, bool* fresh = nullptr)
    {
        if (p_ && count <= cap_)
            return AISX_OK;
        const int rc = alloc(count, zero);
        if (rc == AISX_OK && fresh)
            *fresh = true;
        return rc;
    }
    T* get() const { return p_; }
    size_t cap() const { return cap_; }
    operator T*() const { return p_; }
};

template <class T>
class PinnedBuf { // a hipHostMalloc block
    T* p_ = nullptr;

public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    PinnedBuf& operator=(PinnedBuf&& o) noexcept
    {
        std::swap(p_, o.p_);
        o.reset();
        return *this;
    }
    ~PinnedBuf() { reset(); }
    void reset()
    {
        if (p_)
            (void)hipHostFree(p_);
        p_ = nullptr;
    }
    int alloc(size_t count)
    {
        reset();
        AISX_HIPCHK(hipHostMalloc((void**)&p_, sizeof(T) * (count ? count : 1)));
        return AISX_OK;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
};

class Event {
    hipEvent_t e_ = nullptr;

public:
    Event() = default;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event& operator=(Event&& o) noexcept
    {
        std::swap(e_, o.e_);
        o.reset();
        return *this;
    }
    ~Event() { reset(); }
    void reset()
    {
        if (e_)
            (void)hipEventDestroy(e_);
        e_ = nullptr;
    }
    int create(unsigned flags) // hipEventDisableTiming or hipEventDefault
    {
        reset();
        AISX_HIPCHK(hipEventCreateWithFlags(&e_, flags));
        return AISX_OK;
    }
    int ensure(unsigned flags) { return e_ ? AISX_OK : create(flags); } // first use
    operator hipEvent_t() const { return e_; }
    explicit operator bool() const { return e_ != nullptr; }
};

class Stream { // a stream the handle made; one the caller handed in stays a raw hipStream_t
    hipStream_t s_ = nullptr;

public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept
    {
        std::swap(s_, o.s_);
        o.reset();
        return *this;
    }
    ~Stream() { reset(); }
    void reset()
    {
        if (s_) {
            (void)hipStreamSynchronize(s_);
            (void)hipStreamDestroy(s_);
        }
        s_ = nullptr;
    }
    int create_nonblocking()
    {
        reset();
        AISX_HIPCHK(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
        return AISX_OK;
    }
    void adopt(hipStream_t s) // (one made some other way: hipExtStreamCreateWithCUMask)
    {
        reset();
        s_ = s;
    }
    operator hipStream_t() const { return s_; }
    explicit operator bool() const { return s_ != nullptr; }
};

// the profiling ring: a pair of events around one kernel of every call, the last NEV calls readable afterwards
struct EventRing {
    static constexpr int NEV = 64;
    Event ev0[NEV], ev1[NEV];
    bool on = false;
    long ncalls = 0;

    int enable() // all events or none
    {
        if (ev0[0])
            return AISX_OK;
        Event a[NEV], b[NEV];
        int rc;
        for (int k = 0; k < NEV; k++)
            if ((rc = a[k].create(hipEventDefault)) != AISX_OK || (rc = b[k].create(hipEventDefault)) != AISX_OK)
                return rc;
        for (int k = 0; k < NEV; k++) {
            ev0[k] = std::move(a[k]);
            ev1[k] = std::move(b[k]);
        }
        return AISX_OK;
    }
    int set_profiling(int want) // counting starts again at every call, on or off
    {
        const int rc = want ? enable() : AISX_OK;
        if (rc != AISX_OK)
            return rc;
        on = want != 0;
        ncalls = 0;
        return AISX_OK;
    }
    int begin(hipStream_t st)
    {
        if (on)
            AISX_HIPCHK(hipEventRecord(ev0[ncalls % NEV], st));
        return AISX_OK;
    }
    int end(hipStream_t st)
    {
        if (on) {
            AISX_HIPCHK(hipEventRecord(ev1[ncalls % NEV], st));
            ncalls++;
        }
        return AISX_OK;
    }
    int elapsed(long call, float* ms) const
    {
        AISX_HIPCHK(hipEventSynchronize(ev1[call % NEV]));
        AISX_HIPCHK(hipEventElapsedTime(ms, ev0[call % NEV], ev1[call % NEV]));
        return AISX_OK;
    }
    int last_ms(float* ms) const { return ev0[0] && ncalls >= 1 ? elapsed(ncalls - 1, ms) : AISX_ERR_INVALID; }
    int history(float* ms, int cap, int* n) const
    {
        if (!ev0[0])
            return AISX_ERR_INVALID;
        int w = 0, rc;
        for (long k = ncalls - std::min<long>(ncalls, NEV); k < ncalls && w < cap; k++, w++)
            if ((rc = elapsed(k, &ms[w])) != AISX_OK)
                return rc;
        *n = w;
        return AISX_OK;
    }
};

// a handle under construction: a *_create that returns early destroys it through the handle's own *_destroy,
// one that succeeds release()s it into *out
template <class H, int (*Destroy)(H*)>
struct HandleDeleter {
    void operator()(H* h) const { (void)Destroy(h); }
};
template <class H, int (*Destroy)(H*)>
using HandlePtr = std::unique_ptr<H, HandleDeleter<H, Destroy>>;

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
