// host_util.hpp — the host plumbing the .hip files share (host only, not part of the ABI): HIP_TRY, the event-pair kernel clocks
// behind the *_profile / *_kernel_time hooks, and the body of the *_set_stream functions.
#ifndef RP_HOST_UTIL_HPP
#define RP_HOST_UTIL_HPP

#include <hip/hip_runtime.h>

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

}  // namespace rp

#endif
