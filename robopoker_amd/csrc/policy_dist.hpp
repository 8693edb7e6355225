// policy_dist.hpp — the three distributions a profile row is read through, one definition for every table that answers
// policy queries on the device (nlmc_query.hpp by NlheInfo key, sparse.hip by row).
//
// Reference: RefProf::iterated_distribution / averaged_distribution (mccfr/src/strategy/profile.rs:40-51),
// CfrFlow::sampling_distribution (strategy/flow.rs:24-42).  The arithmetic is rp_mccfr_policy's (mccfr.hip) and the opponent
// branch's of nl_expand_item (nlmc_level.hpp): f32, left folds over a = 0 .. n-1, every operation rounded on its own.
#ifndef RP_POLICY_DIST_HPP
#define RP_POLICY_DIST_HPP

#include <hip/hip_runtime.h>

#include "../../include/rp_math.h"
#include "../../include/rp_mi355x.h"

namespace rp {

struct DistParams {
    float temperature, smoothing, curiosity;
};

// v[a], a < n: the accumulated regrets (RP_DIST_ITERATED) or weights (AVERAGED, SAMPLING) of the row; out[a] = 0 for a >= n.
// A is a compile-time bound so that v and out stay in registers.
template <uint32_t A>
__device__ __forceinline__ void policy_distribution(int kind, const DistParams& hp, const float* v, uint32_t n, float* out) {
    float sum = 0.0f;
#pragma unroll
    for (uint32_t a = 0; a < A; ++a)
        if (a < n) sum += rp_maxf(v[a], RP_EPSILON);
    if (kind != (int)RP_DIST_SAMPLING) {  // max(x, eps) / sum max(x, eps)
#pragma unroll
        for (uint32_t a = 0; a < A; ++a) out[a] = a < n ? rp_maxf(v[a], RP_EPSILON) / sum : 0.0f;
        return;
    }
    const float denom = sum + hp.smoothing;
    float z = 0.0f;
#pragma unroll
    for (uint32_t a = 0; a < A; ++a) {
        out[a] = 0.0f;
        if (a < n) {
            out[a] = rp_maxf((rp_maxf(v[a], RP_EPSILON) / hp.temperature + hp.smoothing) / denom, hp.curiosity);
            z += out[a];
        }
    }
#pragma unroll
    for (uint32_t a = 0; a < A; ++a)
        if (a < n) out[a] = out[a] / z;
}

}  // namespace rp

#endif
