// What every translation unit's entry points do with a device before they compute: open it (open_device) and own scratch
// memory, events and, where asked, a stream on it until they return (DevBufs).
#pragma once
#include "salnmf_error.h"

#include <algorithm>
#include <string>
#include <vector>

namespace salnmf {

// `device` made current, its properties in *prop; refused when it is out of range or not the architecture this build targets
inline int open_device(int device, hipDeviceProp_t* prop) {
    int ndev = 0;
    HIPCK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail("device %d out of range (%d visible)", device, ndev);
    HIPCK(hipSetDevice(device));
    HIPCK(hipGetDeviceProperties(prop, device));
    if (std::string(prop->gcnArchName).rfind("gfx950", 0) != 0) return fail("this build targets gfx950 only; device %d is %s", device, prop->gcnArchName);
    return 0;
}

// The device buffers and events of one call, freed when it returns, by whichever path.
// (the destructor waits for the stream first: on an early return no pending copy outlives a buffer, host or device)
struct DevBufs {
    hipStream_t stream;  // the caller's (null: the default stream), or its own after own_stream()
    bool owned = false;
    std::vector<void*> ptrs;
    std::vector<hipEvent_t> events;
    explicit DevBufs(hipStream_t s = nullptr) : stream(s) {}
    DevBufs(const DevBufs&) = delete;
    DevBufs& operator=(const DevBufs&) = delete;
    ~DevBufs() {
        (void)hipStreamSynchronize(stream);
        for (void* p : ptrs) (void)hipFree(p);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        if (owned) (void)hipStreamDestroy(stream);
    }
    int own_stream() {
        HIPCK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        owned = true;
        return 0;
    }
    template <typename T>
    T* get(size_t n) {
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return (T*)p;
    }
    // an event recorded on the stream now, or null
    hipEvent_t mark() {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        events.push_back(e);
        return hipEventRecord(e, stream) == hipSuccess ? e : nullptr;
    }
};

}  // namespace salnmf
