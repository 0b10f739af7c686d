// nmpc_host.h -- what the host side of the C ABI (nmpc_kernels.hip, nmpc_loop_host.h, nmpc_plan_host.h) owns on a device: memory, pinned host memory and events, each released
// with the struct that holds it, so that no list of frees follows the structs by hand.  Not copyable; move assignment only, which is what
// a group of them uses to let go of everything it holds (`*this = {}`).
#pragma once
#include <hip/hip_runtime.h>

#include <utility>

namespace nmpc {

template <class T>
struct DevBuf {          // n elements of T on the current device
    T *p = nullptr;
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); return *this; }
    ~DevBuf() { (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc((void **)&p, n * sizeof(T)); }      // (of an empty one)
    hipError_t alloc_fill(size_t n, int byte)          // alloc + every byte set
    {
        const hipError_t e = alloc(n);
        return e == hipSuccess ? hipMemset(p, byte, n * sizeof(T)) : e;
    }
    hipError_t upload(const T *src, size_t n)          // alloc + n elements from host memory
    {
        const hipError_t e = alloc(n);
        return e == hipSuccess ? hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice) : e;
    }
    // n elements to host memory; dst NULL: the caller did not ask for them
    hipError_t read(T *dst, size_t n) const { return dst ? hipMemcpy(dst, p, n * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess; }
    operator T *() const { return p; }
};

struct PinBuf {          // pinned host bytes
    char *p = nullptr;
    PinBuf &operator=(PinBuf &&o) noexcept { std::swap(p, o.p); return *this; }
    ~PinBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t bytes) { return hipHostMalloc((void **)&p, bytes, hipHostMallocDefault); }
    operator char *() const { return p; }
};

struct Event {
    hipEvent_t e = nullptr;
    Event &operator=(Event &&o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};

}  // namespace nmpc
