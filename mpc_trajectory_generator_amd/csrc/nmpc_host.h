// nmpc_host.h -- what the host side of the C ABI (nmpc_kernels.hip) owns on a device: memory, pinned host memory and events, each released
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
