// host_util.hpp — the host plumbing the .hip files share (host only, not part of the ABI): HIP_TRY, the event-pair kernel clocks
// behind the *_profile / *_kernel_time hooks, the body of the *_set_stream functions, and what the entry points that come in a host
// and a _device form share: the staging arena, the chunk loop, the grow-only region.
#ifndef RP_HOST_UTIL_HPP
#define RP_HOST_UTIL_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "rp_internal.h"

#define HIP_TRY(expr)                                                                                 \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) return rp::fail(RP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

namespace rp {

// One clock per name of a fixed list: HIP event pairs around the launches of a kernel group, read back by drain().  The stream is an
// argument of begin / end, not a member: a handle's stream can change under it (rp_*_set_stream).
struct KernelClocks {
    using Pair = std::pair<hipEvent_t, hipEvent_t>;
    struct Clock {
        std::vector<Pair> pending;
        std::vector<Pair> shared;  // pairs another clock owns (begin's `also`): read here, destroyed there
        double total_ms = 0.0;
        uint64_t launches = 0;
    };
    const char* const* names;
    std::vector<Clock> clk;
    bool on = false;  // the profiling flag: begin and end do nothing while it is false

    KernelClocks(const char* const* names_, int count) : names(names_), clk((size_t)count) {}

    // `also`: a second clock that counts the same interval (a clock inside a clock): the SAME pair of events, so that it puts nothing
    // more on the stream
    void begin(hipStream_t stream, int id, int also = -1) {
        if (!on) return;
        hipEvent_t a, b;
        (void)hipEventCreate(&a);
        (void)hipEventCreate(&b);
        (void)hipEventRecord(a, stream);
        clk[id].pending.emplace_back(a, b);
        if (also >= 0) clk[also].shared.emplace_back(a, b);
    }
    void end(hipStream_t stream, int id, int also = -1) {
        if (!on || clk[id].pending.empty()) return;
        (void)hipEventRecord(clk[id].pending.back().second, stream);
        clk[id].launches += 1;
        if (also >= 0) clk[also].launches += 1;
    }
    // A pair counts only if both calls succeed: one whose end was never recorded (an error return between begin and end) adds nothing.
    void drain() {
        auto add = [](Clock& c, const Pair& pr) {
            float ms = 0.0f;
            if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) c.total_ms += ms;
        };
        for (Clock& c : clk) {  // every reader first: a shared pair is destroyed by the clock that owns it
            for (const Pair& pr : c.shared) add(c, pr);
            c.shared.clear();
        }
        for (Clock& c : clk) {
            for (const Pair& pr : c.pending) {
                add(c, pr);
                (void)hipEventDestroy(pr.first);
                (void)hipEventDestroy(pr.second);
            }
            c.pending.clear();
        }
    }
    void reset() {
        for (Clock& c : clk) c.total_ms = 0.0, c.launches = 0;
    }
    int find(const char* name) const {
        for (size_t i = 0; i < clk.size(); ++i)
            if (!strcmp(name, names[i])) return (int)i;
        return -1;
    }
};

// the lookup and copy-out of the *_kernel_time functions (the caller has set the device and synchronised the stream)
inline int kernel_time(KernelClocks& c, const char* who, const char* name, double* total_ms, uint64_t* launches) {
    c.drain();
    const int id = c.find(name);
    if (id < 0) return rp::fail(RP_ERR_INVALID, "%s: unknown kernel '%s'", who, name);
    if (total_ms) *total_ms = c.clk[id].total_ms;
    if (launches) *launches = c.clk[id].launches;
    return RP_OK;
}

// the body of the *_set_stream functions: the handle leaves its stream (destroyed if it owns it) for the caller's, or for a new
// non-blocking one of its own when hip_stream is NULL
inline int swap_stream(hipStream_t& stream, bool& own, void* hip_stream) {
    HIP_TRY(hipStreamSynchronize(stream));
    if (own && stream) HIP_TRY(hipStreamDestroy(stream));
    own = false;
    if (hip_stream) {
        stream = reinterpret_cast<hipStream_t>(hip_stream);
    } else {
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        own = true;
    }
    return RP_OK;
}

// ---- entry points in pairs.  The _device form takes every array in device memory and queues its launches on its handle's stream; the
// host form stages the same arrays through one device allocation (Stage), calls the _device form and synchronises.  The two forms of
// a pair share ONE check of their arguments: the refusals of include/rp_mi355x.h in its order, made before a device is touched,
// naming the un-suffixed function; RP_OK from a check with n == 0 is the call's answer.  Every entry point that may need more than
// one launch runs chunks, whatever its chunk size.

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// device scratch of one host-form call.  The host form names its arrays — in(p, count): copied to the device, out(p, count): copied
// back from it; a NULL array (an optional argument left out) or an empty one is no bytes and stays, or becomes, NULL — then up()
// makes the ONE allocation, queues the uploads and points every named p at its device copy (16-byte aligned each), so that the
// _device form is called with the host form's own arguments; down() queues the downloads and synchronises.  The allocation is freed
// on every way out, a refusal after a launch was queued included: hipFree waits for the device.
struct Stage {
    struct Part {
        void* p;  // the caller's pointer variable, whatever it points to
        void* host;
        size_t bytes, at;
        bool in;
    };
    int device;
    hipStream_t st;
    std::vector<Part> parts;
    size_t bytes = 0;
    unsigned char* base = nullptr;
    Stage(int device_, hipStream_t stream) : device(device_), st(stream) {}
    Stage(const Stage&) = delete;
    ~Stage() {
        if (base) (void)hipFree(base);
    }
    template <typename T>
    Stage& add(T*& p, size_t count, bool in) {
        parts.push_back(Part{(void*)&p, (void*)p, p ? count * sizeof(T) : 0, bytes, in});
        bytes += align16(parts.back().bytes);
        return *this;
    }
    template <typename T>
    Stage& in(const T*& p, size_t count) {
        return add(p, count, true);
    }
    template <typename T>
    Stage& out(T*& p, size_t count) {
        return add(p, count, false);
    }
    int up() {
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipMalloc(&base, bytes));
        for (const Part& p : parts) {
            void* dev = p.bytes ? base + p.at : nullptr;
            memcpy(p.p, &dev, sizeof(dev));
            if (p.in && p.bytes) HIP_TRY(hipMemcpyAsync(base + p.at, p.host, p.bytes, hipMemcpyHostToDevice, st));
        }
        return RP_OK;
    }
    int down() {
        for (const Part& p : parts)
            if (!p.in && p.bytes) HIP_TRY(hipMemcpyAsync(p.host, base + p.at, p.bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return RP_OK;
    }
};
// items at .. at + m of n, at most `chunk` per launch: f(at, m) queues one launch
template <typename F>
int chunks(uint64_t n, uint64_t chunk, F f) {
    for (uint64_t at = 0; at < n; at += chunk) {
        f(at, (uint32_t)std::min<uint64_t>(chunk, n - at));
        HIP_TRY(hipGetLastError());
    }
    return RP_OK;
}
// an optional array from its item i on
template <typename T>
T* from(T* p, uint64_t i) {
    return p ? p + i : nullptr;
}
// a grow-only region of the handle that queued launches write: an earlier call's launch may still write the old one
inline int grow(void*& region, size_t& bytes, size_t need, hipStream_t st) {
    if (need <= bytes) return RP_OK;
    HIP_TRY(hipStreamSynchronize(st));
    if (region) HIP_TRY(hipFree(region));
    region = nullptr;
    bytes = 0;
    HIP_TRY(hipMalloc(&region, need));
    bytes = need;
    return RP_OK;
}

}  // namespace rp

#endif
