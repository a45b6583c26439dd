// One owner per handle for what a handle takes from the HIP runtime: device memory, pinned host memory, events and streams.  Every handle struct that owns anything has
// a bf::Resources member; its destructor gives back whatever is still held, newest first, each through the call that matches its acquisition.  A create builds its
// handle under a bf::CreateGuard, which runs the type's _destroy on every early return, so a failed create keeps nothing.  No pooling, no caching, no locks.
// (The order and sizes of the acquisitions are behaviour on this device - DESIGN.md 2 - and this class does not change them: every call here is one runtime call.)
#pragma once
#include <atomic>
#include <vector>

#include "bf_internal.h"

namespace bf {

// process-wide, read by bf_debug_live_resources; failIn: bf_debug_fail_acquire's countdown (0: off)
struct ResourceCounters {
    std::atomic<uint64_t> owners{0}, deviceAllocs{0}, deviceBytes{0}, others{0}, acquisitions{0}, releaseErrors{0};
    std::atomic<int64_t> failIn{0};
};
extern ResourceCounters g_resources;      // common.cpp

class Resources {
public:
    Resources() { g_resources.owners.fetch_add(1, std::memory_order_relaxed); }
    ~Resources() {
        while (!held.empty()) { give_back(held.back()); held.pop_back(); }
        g_resources.owners.fetch_sub(1, std::memory_order_relaxed);
    }
    Resources(const Resources&) = delete;
    Resources& operator=(const Resources&) = delete;

    // `count` elements of device memory (through bf_debug_malloc: BF_DEBUG_POISON=<file>:<line> names the caller's line)
    template <typename T>
    int device(T** p, size_t count, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
        const size_t bytes = count * sizeof(T);
        void* q = nullptr;
        const bool inj = injected();
        const hipError_t e = inj ? hipErrorOutOfMemory : bf_debug_malloc(&q, bytes, file, line);
        if (e != hipSuccess) return failed("device memory", bytes, e, inj, file, line);
        *p = (T*)q;
        if (q) keep(q, DEVICE, bytes);
        return BF_OK;
    }
    // void*: `count` is in bytes
    int device(void** p, size_t count, const char* file = __builtin_FILE(), int line = __builtin_LINE()) { return device((char**)p, count, file, line); }
    template <typename T>
    int pinned(T** p, size_t bytes, unsigned flags = hipHostMallocDefault, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
        void* q = nullptr;
        const bool inj = injected();
        const hipError_t e = inj ? hipErrorOutOfMemory : hipHostMalloc(&q, bytes, flags);
        if (e != hipSuccess) return failed("pinned host memory", bytes, e, inj, file, line);
        *p = (T*)q;
        if (q) keep(q, PINNED, bytes);
        return BF_OK;
    }
    int event(hipEvent_t* ev, unsigned flags = hipEventDefault, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
        hipEvent_t q = nullptr;
        const bool inj = injected();
        const hipError_t e = inj ? hipErrorOutOfMemory : hipEventCreateWithFlags(&q, flags);
        if (e != hipSuccess) return failed("event", 0, e, inj, file, line);
        *ev = q;
        keep(q, EVENT, 0);
        return BF_OK;
    }
    // a stream the caller has just created, by whatever call it needed.  A failed adoption destroys the stream.
    int adopt(hipStream_t s, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
        if (injected()) { (void)hipStreamDestroy(s); return failed("stream", 0, hipErrorOutOfMemory, true, file, line); }
        keep(s, STREAM, 0);
        return BF_OK;
    }
    // give one thing back early: frees it, nulls the caller's pointer, forgets it (null, or not held: nothing happens to it)
    template <typename T>
    void release(T*& p) {
        for (size_t i = held.size(); i-- > 0;)
            if (held[i].handle == (void*)p) { give_back(held[i]); held.erase(held.begin() + (long)i); break; }
        p = nullptr;
    }
    template <typename T>
    int regrow(T** p, size_t count, const char* file = __builtin_FILE(), int line = __builtin_LINE()) {
        release(*p);
        return device(p, count, file, line);
    }

private:
    enum Kind : uint8_t { DEVICE, PINNED, EVENT, STREAM };
    struct Held { void* handle; size_t bytes; Kind kind; };
    std::vector<Held> held;

    static bool injected() {
        if (g_resources.failIn.load(std::memory_order_relaxed) <= 0) return false;
        return g_resources.failIn.fetch_sub(1, std::memory_order_relaxed) == 1;
    }
    static int failed(const char* what, size_t bytes, hipError_t e, bool inj, const char* file, int line) {
        set_error("acquiring %s (%zu B) failed: %s%s (%s:%d)", what, bytes, hipGetErrorString(e), inj ? " [injected by bf_debug_fail_acquire]" : "", file, line);
        return BF_ERR_HIP;
    }
    void keep(void* handle, Kind kind, size_t bytes) {
        held.push_back({handle, bytes, kind});
        g_resources.acquisitions.fetch_add(1, std::memory_order_relaxed);
        if (kind == DEVICE) { g_resources.deviceAllocs.fetch_add(1, std::memory_order_relaxed); g_resources.deviceBytes.fetch_add(bytes, std::memory_order_relaxed); }
        else g_resources.others.fetch_add(1, std::memory_order_relaxed);
    }
    static void give_back(const Held& h) {
        hipError_t e = hipSuccess;
        switch (h.kind) {
            case DEVICE: e = hipFree(h.handle); g_resources.deviceAllocs.fetch_sub(1, std::memory_order_relaxed); g_resources.deviceBytes.fetch_sub(h.bytes, std::memory_order_relaxed); break;
            case PINNED: e = hipHostFree(h.handle); break;
            case EVENT: e = hipEventDestroy((hipEvent_t)h.handle); break;
            case STREAM: e = hipStreamDestroy((hipStream_t)h.handle); break;
        }
        if (h.kind != DEVICE) g_resources.others.fetch_sub(1, std::memory_order_relaxed);
        if (e != hipSuccess) g_resources.releaseErrors.fetch_add(1, std::memory_order_relaxed);
    }
};

// A create builds its handle under this guard: any early return runs the type's _destroy (which takes a handle in any partially built state); the one exit that
// publishes the handle dismisses the guard first.
template <typename H>
class CreateGuard {
public:
    CreateGuard(H* h, int (*destroy)(H*)) : h(h), destroy(destroy) {}
    ~CreateGuard() { if (h) (void)destroy(h); }
    CreateGuard(const CreateGuard&) = delete;
    CreateGuard& operator=(const CreateGuard&) = delete;
    H* dismiss() { H* r = h; h = nullptr; return r; }

private:
    H* h;
    int (*destroy)(H*);
};

}  // namespace bf
