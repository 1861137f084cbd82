// device_res.h — what the host code of libxrt holds on a device, as move-only owners that free what they hold: DevBuf<T> (hipMalloc, under
// XRT_GUARD with a guard area behind it), Event, Stream, Pinned<T> (hipHostMalloc).  A null owner calls no HIP function, in its destructor or
// anywhere else: a host-only scene (device -1) is made and destroyed on machines without a GPU.  With them the error reporting every owner
// needs (fail / HIPCHECK / guarded) and the roctx ranges.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/xrt.h"

namespace xrt {

inline thread_local std::string g_err = "";
inline int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIPCHECK(expr)                                                                                         \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess)                                                                                  \
            return fail(e_ == hipErrorOutOfMemory ? XRT_E_OOM : XRT_E_HIP, "%s failed: %s (%s:%d)", #expr,     \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                            \
    } while (0)

// roctx ranges around the stages of a frame, for `rocprofv3 --marker-trace --kernel-trace`: XRT_ROCTX=1 loads the
// marker library on first use (no load-time dependency, nothing is called otherwise).  The ranges bracket the ENQUEUE of a
// stage on the host; the kernels they enqueue carry the same names in the kernel trace.
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    bool on = false;
    Roctx() {
        if (!getenv("XRT_ROCTX")) return;
        for (const char *n : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
            if (void *h = dlopen(n, RTLD_NOW | RTLD_GLOBAL)) {
                push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
                pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
                if (push && pop) { on = true; return; }
            }
        }
    }
};
inline Roctx &roctx() { static Roctx r; return r; }
struct Range {   // RAII: a named range for the enclosing scope
    bool on;
    explicit Range(const char *fmt, int k = 0) : on(roctx().on) {
        if (!on) return;
        char buf[64];
        snprintf(buf, sizeof(buf), fmt, k);
        roctx().push(buf);
    }
    ~Range() { if (on) roctx().pop(); }
};

// No C++ exception may cross the C boundary (a P/Invoke, ctypes or C host would be terminated): the entry points that
// allocate host memory from caller-given sizes run inside this guard.
template <class F>
int guarded(const char *fn, F &&f) {
    try { return f(); }
    catch (const std::bad_alloc &) { return fail(XRT_E_OOM, "%s: out of host memory", fn); }
    catch (const std::exception &e) { return fail(XRT_E_INVALID_ARG, "%s: %s", fn, e.what()); }
    catch (...) { return fail(XRT_E_INTERNAL, "%s: unknown exception", fn); }
}

// XRT_GUARD=1 (read by xrt_scene_create / xrt_scene_load; a test and debugging mode): every device buffer allocated from then on gets
// GUARD_BYTES of a known pattern behind its last element, and the end of every frame and of every batched query checks that the pattern
// is intact -- a kernel that writes past an array it was given is then XRT_E_INTERNAL naming the buffer's size, not a corrupted
// neighbour or a GPU fault somewhere else.  (Round 3 sized the generation-0 arrays by the root box's screen rectangle while one of them
// was still indexed by path: a process abort in the GPU suite that the next edit hid.  tests/test_gpu_parity.py runs the frame modes
// under the guards.)
constexpr size_t GUARD_BYTES = 4096;
constexpr unsigned char GUARD_PATTERN = 0xA5;
inline std::atomic<int> g_guardMode{0};
struct GuardRegistry {
    std::mutex m;
    std::unordered_map<void *, size_t> bytesOf;   // buffer -> payload bytes (the guard follows)
};
inline GuardRegistry g_guards;
inline int guard_alloc(void **p, size_t bytes) {
    const bool on = g_guardMode.load() != 0;
    HIPCHECK(hipMalloc(p, bytes + (on ? GUARD_BYTES : 0)));
    if (on) {
        HIPCHECK(hipMemset((char *)*p + bytes, GUARD_PATTERN, GUARD_BYTES));
        std::lock_guard<std::mutex> lk(g_guards.m);
        g_guards.bytesOf[*p] = bytes;
    }
    return XRT_OK;
}
inline void guard_free(void *p) {
    // (whatever the mode is NOW: a buffer registered while the mode was on and freed after it was switched off must not stay in the registry --
    // its address is handed out again, to this library without a guard or to somebody else, and the next check under the mode would read it)
    { std::lock_guard<std::mutex> lk(g_guards.m); g_guards.bytesOf.erase(p); }
    (void)hipFree(p);
}
// All guards of the process (buffers of every scene on the CURRENT device are readable; others are skipped on error).
inline int guards_check(const char *where) {
    if (g_guardMode.load() == 0) return XRT_OK;
    if (hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return XRT_OK; }
    std::lock_guard<std::mutex> lk(g_guards.m);
    std::vector<unsigned char> tail(GUARD_BYTES);
    for (const auto &kv : g_guards.bytesOf) {
        if (hipMemcpy(tail.data(), (const char *)kv.first + kv.second, GUARD_BYTES, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); continue; }
        for (size_t i = 0; i < GUARD_BYTES; i++)
            if (tail[i] != GUARD_PATTERN)
                return fail(XRT_E_INTERNAL, "%s: a kernel wrote %zu bytes past the end of a device buffer of %zu bytes (XRT_GUARD)", where, i + 1, kv.second);
    }
    return XRT_OK;
}

// Device memory.  ensure(n) only grows (a buffer that is large enough is one compare); the contents do not survive a growth.
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;   // elements
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }   // (what this held goes with o)
    ~DevBuf() { release(); }
    int ensure(size_t n) {
        if (n <= cap && p) return XRT_OK;
        release();
        if (n == 0) n = 1;
        int rc = guard_alloc((void **)&p, n * sizeof(T));
        if (rc != XRT_OK) { p = nullptr; return rc; }
        cap = n;
        return XRT_OK;
    }
    void release() { if (p) guard_free(p); p = nullptr; cap = 0; }
};

template <class T>
int upload(DevBuf<T> &b, const std::vector<T> &v) {
    int rc = b.ensure(v.size());
    if (rc != XRT_OK) return rc;
    if (!v.empty()) HIPCHECK(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return XRT_OK;
}

// An event or a stream the library made itself (never a caller's).  Reads as the raw handle wherever one is expected.
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Handle &operator=(Handle &&o) noexcept { std::swap(h, o.h); return *this; }
    ~Handle() { reset(); }
    void reset() { if (h) (void)Destroy(h); h = nullptr; }
    operator H() const { return h; }
};
struct Event : Handle<hipEvent_t, hipEventDestroy> {
    int create(unsigned flags = hipEventDisableTiming) { if (!h) HIPCHECK(hipEventCreateWithFlags(&h, flags)); return XRT_OK; }   // made on first use, kept
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
    int create() { if (!h) HIPCHECK(hipStreamCreateWithFlags(&h, hipStreamNonBlocking)); return XRT_OK; }
};

// Page-locked host memory; `dev` is its device view where the flags ask for mapped memory.  ensure() only grows and keeps no contents.
template <class T>
struct Pinned {
    T *p = nullptr, *dev = nullptr;
    size_t bytes = 0;
    Pinned() = default;
    Pinned(Pinned &&o) noexcept { *this = std::move(o); }
    Pinned &operator=(Pinned &&o) noexcept { std::swap(p, o.p); std::swap(dev, o.dev); std::swap(bytes, o.bytes); return *this; }
    ~Pinned() { reset(); }
    int ensure(size_t n, unsigned flags) {
        if (p && n <= bytes) return XRT_OK;
        reset();
        HIPCHECK(hipHostMalloc((void **)&p, n, flags));
        bytes = n;
        if (flags & hipHostMallocMapped)   // (without its device view the memory is of no use: nothing is kept)
            if (hipError_t e = hipHostGetDevicePointer((void **)&dev, p, 0)) { reset(); return fail(XRT_E_HIP, "hipHostGetDevicePointer failed: %s", hipGetErrorString(e)); }
        return XRT_OK;
    }
    void reset() { if (p) (void)hipHostFree(p); p = dev = nullptr; bytes = 0; }
};

}  // namespace xrt
