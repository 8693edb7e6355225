// nlmc_query.hpp — the read side of the NLHE blueprint: batched, read-only queries BY NlheInfo KEY against the
// device-resident table (rp_nlhe_policy / rp_nlhe_memory).
//
// Reference: Brain::policy (parlor/src/players/brain.rs:45-55) and Source::strategy / Source::memory (nlhe/src/source.rs:40-87)
// ask the blueprint one infoset at a time; RefProf::{iterated,averaged}_distribution (mccfr/src/strategy/profile.rs:40-51) and
// CfrFlow::sampling_distribution (flow.rs:24-42) are the distributions (policy_dist.hpp); an infoset without a row reads as
// default regret, zero weight (book.rs:93-122).
//
// A query is a gather: one 32-byte slot (the home slot, usually the only probe) and a piece of one 144-byte row.  The home slot and
// the home row are loaded together, the row again only when the key was found further down its probe chain.  Nothing here writes
// to the table: no atomic, no insertion (nl_row_of inserts and is not used), n_keys untouched.
//
// Two shapes of the policy kernel exist so that they can be measured against each other (scripts/nlhe_policy_rate.py):
//   group: NLQ_GROUP lanes per query; lane j < 3 loads one 16-byte piece of the row, the nine values are handed round the group
//          with shuffles, every lane folds them (the folds are sequential by contract), lane a writes out[a]: one wave-instruction
//          covers 8 rows and the group's outputs are contiguous.
//   lane:  one lane per query (nl_load_row), outputs staged through LDS so that they leave coalesced.
#ifndef RP_NLMC_QUERY_HPP
#define RP_NLMC_QUERY_HPP

#include "nlmc_common.hpp"
#include "policy_dist.hpp"

namespace rp {

#define NLQ_BLOCK 256u
#define NLQ_GROUP 8u    // lanes per query, policy (group shape)
#define NLQ_MGROUP 16u  // lanes per query, memory: lane a < 9 carries the Encounter of slot a

// consecutive non-zero 5-bit groups from bit 0, at most 9: the length nl_choices_path gave the path
__device__ __forceinline__ uint32_t nlq_nch(uint64_t choices) {
    uint32_t nch = 0;
#pragma unroll
    for (uint32_t a = 0; a < NLMC_A; ++a) nch += (nch == a && ((choices >> (5u * a)) & 31ull) != 0) ? 1u : 0u;
    return nch;
}
__device__ __forceinline__ bool nlq_match(const uint4& lo, const uint4& hi, uint64_t past, uint64_t choices, uint32_t present) {
    return ((uint64_t)lo.x | ((uint64_t)lo.y << 32)) == past && ((uint64_t)lo.z | ((uint64_t)lo.w << 32)) == choices && hi.x == present;
}
// The probe chain of a key from the slot AFTER its home slot (whose two halves the caller loaded itself, beside the row): stops at
// the first slot that is not ready (absent) or after mask + 1 probes in all (absent: a full table is a legal state after
// rp_nlhe_import).  No wave collective inside: lanes leave at different trip counts.
__device__ __forceinline__ bool nlq_find(const NlTable& t, uint64_t past, uint64_t choices, uint32_t present, uint32_t home, const uint4& lo0,
                                         const uint4& hi0, uint32_t* row) {
    *row = home;
    if (hi0.z != 2u) return false;
    if (nlq_match(lo0, hi0, past, choices, present)) return true;
    uint32_t s = home;
    for (uint32_t probes = 1; probes <= t.mask; ++probes) {
        s = (s + 1u) & t.mask;
        const uint4* sl = reinterpret_cast<const uint4*>(t.slots + s);
        const uint4 lo = sl[0], hi = sl[1];
        if (hi.z != 2u) return false;
        if (nlq_match(lo, hi, past, choices, present)) {
            *row = s;
            return true;
        }
    }
    return false;
}

// 16-byte pieces FIRST .. FIRST + N of an infoset's row (a row is 9 pieces: regret[9] weight[9] payoff[9] visits[9]), and whether
// it has one.  The home slot and the home row's pieces are loaded together, the row again only when the key was found further down
// its probe chain.  pc is the row's bytes as stored (slots past the infoset's actions included); an absent infoset leaves the home
// row's in it: read `found` first.
template <uint32_t FIRST, uint32_t N>
__device__ __forceinline__ bool nlq_row_pieces(const NlTable& t, uint64_t past, uint64_t choices, uint32_t present, float4* pc) {
    static_assert(FIRST + N <= NLMC_A, "a row is 4 x 9 floats = 9 pieces");
    const uint32_t home = (uint32_t)nl_key_hash(past, choices, present) & t.mask;
    const uint4* sl = reinterpret_cast<const uint4*>(t.slots + home);
    const uint4 lo = sl[0], hi = sl[1];
    const float4* rw = reinterpret_cast<const float4*>(t.rows + (size_t)home * 4u * NLMC_A);
#pragma unroll
    for (uint32_t i = 0; i < N; ++i) pc[i] = rw[FIRST + i];
    uint32_t row;
    const bool found = nlq_find(t, past, choices, present, home, lo, hi, &row);
    if (found && row != home) {
        const float4* rr = reinterpret_cast<const float4*>(t.rows + (size_t)row * 4u * NLMC_A);
#pragma unroll
        for (uint32_t i = 0; i < N; ++i) pc[i] = rr[FIRST + i];
    }
    return found;
}
// The nine weights of an infoset's row: floats 9..17, pieces 2..4 hold floats 8..19
__device__ __forceinline__ bool nlq_row_weights(const NlTable& t, uint64_t past, uint64_t choices, uint32_t present, float* w) {
    float4 p[3];
    const bool found = nlq_row_pieces<2, 3>(t, past, choices, present, p);
    w[0] = p[0].y, w[1] = p[0].z, w[2] = p[0].w, w[3] = p[1].x, w[4] = p[1].y, w[5] = p[1].z, w[6] = p[1].w, w[7] = p[2].x, w[8] = p[2].y;
    return found;
}
// The nine weights and the nine payoffs: floats 9..17 and 18..26, pieces 2..6 hold floats 8..27
__device__ __forceinline__ bool nlq_row_weights_payoffs(const NlTable& t, uint64_t past, uint64_t choices, uint32_t present, float* w, float* v) {
    float4 p[5];
    const bool found = nlq_row_pieces<2, 5>(t, past, choices, present, p);
    const float f[20] = {p[0].x, p[0].y, p[0].z, p[0].w, p[1].x, p[1].y, p[1].z, p[1].w, p[2].x, p[2].y,
                         p[2].z, p[2].w, p[3].x, p[3].y, p[3].z, p[3].w, p[4].x, p[4].y, p[4].z, p[4].w};
#pragma unroll
    for (uint32_t a = 0; a < NLMC_A; ++a) w[a] = f[1u + a], v[a] = f[10u + a];
    return found;
}

struct NlQuery {
    uint64_t n;
    const uint64_t* past;
    const uint32_t* present;
    const uint64_t* choices;
    uint8_t *edges, *n_actions, *found;  // any may be NULL
};

// ---- policy, group shape: NLQ_GROUP lanes per query.  The loop's trip count is uniform over the workgroup (the shuffles are wave
// collectives); a group past the end of the batch loads and stores nothing.
template <bool WEIGHTS>  // the row's weights (AVERAGED, SAMPLING) or its regrets (ITERATED)
__global__ __launch_bounds__(NLQ_BLOCK) void k_nl_policy_group(NlTable t, NlQuery q, int kind, DistParams hp, float* policy) {
    constexpr uint32_t QPB = NLQ_BLOCK / NLQ_GROUP;
    constexpr uint32_t FIRST = WEIGHTS ? 2u : 0u, OFF = WEIGHTS ? 1u : 0u;  // weights = floats 9..17 of the row = pieces 2..4 from float 8
    const uint32_t lane = threadIdx.x % NLQ_GROUP;
    for (uint64_t base = (uint64_t)blockIdx.x * QPB; base < q.n; base += (uint64_t)gridDim.x * QPB) {
        const uint64_t i = base + threadIdx.x / NLQ_GROUP;
        const bool active = i < q.n;
        uint64_t past = 0, choices = 0;
        uint32_t present = 0, nch = 0;
        bool found = false;
        float4 pc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (active) {
            past = q.past[i];
            choices = q.choices[i];
            present = q.present[i];
            nch = nlq_nch(choices);
            const uint32_t home = (uint32_t)nl_key_hash(past, choices, present) & t.mask;
            const uint4* sl = reinterpret_cast<const uint4*>(t.slots + home);
            const uint4 lo = sl[0], hi = sl[1];
            if (lane < 3u) pc = reinterpret_cast<const float4*>(t.rows + (size_t)home * 4u * NLMC_A)[FIRST + lane];
            uint32_t row;
            found = nlq_find(t, past, choices, present, home, lo, hi, &row);
            if (found && row != home && lane < 3u) pc = reinterpret_cast<const float4*>(t.rows + (size_t)row * 4u * NLMC_A)[FIRST + lane];
        }
        float v[NLMC_A], out[NLMC_A];
#pragma unroll
        for (uint32_t a = 0; a < NLMC_A; ++a) {
            const uint32_t f = OFF + a;  // float f of the three pieces: lane f / 4, component f % 4
            const float c = (f & 3u) == 0u ? pc.x : ((f & 3u) == 1u ? pc.y : ((f & 3u) == 2u ? pc.z : pc.w));
            v[a] = __shfl(c, (int)(f >> 2), (int)NLQ_GROUP);
            if (!found) v[a] = WEIGHTS ? 0.0f : nl_default_regret((uint32_t)(choices >> (5u * a)) & 31u);
        }
        policy_distribution<NLMC_A>(kind, hp, v, nch, out);
        if (active) {
            // lane l writes slot l, lane 0 slot 8 as well: 36 contiguous bytes per group, 288 per wavefront
            static_assert(NLQ_GROUP + 1u == NLMC_A, "the group writes slots 0..7 by lane and slot 8 by lane 0");
            float mine = out[0];
#pragma unroll
            for (uint32_t a = 1; a < NLQ_GROUP; ++a) mine = lane == a ? out[a] : mine;
            policy[i * NLMC_A + lane] = mine;
            if (q.edges) q.edges[i * NLMC_A + lane] = lane < nch ? (uint8_t)((choices >> (5u * lane)) & 31u) : (uint8_t)0;
            if (lane == 0u) {
                policy[i * NLMC_A + NLQ_GROUP] = out[NLQ_GROUP];
                if (q.edges) q.edges[i * NLMC_A + NLQ_GROUP] = NLQ_GROUP < nch ? (uint8_t)((choices >> (5u * NLQ_GROUP)) & 31u) : (uint8_t)0;
                if (q.n_actions) q.n_actions[i] = (uint8_t)nch;
                if (q.found) q.found[i] = found ? 1u : 0u;
            }
        }
    }
}

// ---- policy, lane shape: one lane per query; policy and edges leave through LDS, a workgroup's 256 x 9 values in one contiguous run
__global__ __launch_bounds__(NLQ_BLOCK) void k_nl_policy_lane(NlTable t, NlQuery q, int kind, DistParams hp, float* policy) {
    __shared__ float s_pol[NLQ_BLOCK * NLMC_A];
    __shared__ uint8_t s_edge[NLQ_BLOCK * NLMC_A];
    const bool weights = kind != (int)RP_DIST_ITERATED;
    for (uint64_t base = (uint64_t)blockIdx.x * NLQ_BLOCK; base < q.n; base += (uint64_t)gridDim.x * NLQ_BLOCK) {
        const uint64_t i = base + threadIdx.x;
        if (i < q.n) {
            const uint64_t past = q.past[i], choices = q.choices[i];
            const uint32_t present = q.present[i], nch = nlq_nch(choices);
            const uint32_t home = (uint32_t)nl_key_hash(past, choices, present) & t.mask;
            const uint4* sl = reinterpret_cast<const uint4*>(t.slots + home);
            const uint4 lo = sl[0], hi = sl[1];
            float rf[20];
            nl_load_row(t.rows, home, weights, rf);
            uint32_t row;
            const bool found = nlq_find(t, past, choices, present, home, lo, hi, &row);
            if (found && row != home) nl_load_row(t.rows, row, weights, rf);
            float v[NLMC_A], out[NLMC_A];
#pragma unroll
            for (uint32_t a = 0; a < NLMC_A; ++a) {
                v[a] = weights ? rf[NLMC_A + a] : rf[a];
                if (!found) v[a] = weights ? 0.0f : nl_default_regret((uint32_t)(choices >> (5u * a)) & 31u);
            }
            policy_distribution<NLMC_A>(kind, hp, v, nch, out);
#pragma unroll
            for (uint32_t a = 0; a < NLMC_A; ++a) {
                s_pol[threadIdx.x * NLMC_A + a] = out[a];
                s_edge[threadIdx.x * NLMC_A + a] = a < nch ? (uint8_t)((choices >> (5u * a)) & 31u) : (uint8_t)0;
            }
            if (q.n_actions) q.n_actions[i] = (uint8_t)nch;
            if (q.found) q.found[i] = found ? 1u : 0u;
        }
        __syncthreads();
        const uint64_t left = q.n - base;
        const uint32_t cells = (uint32_t)(left < NLQ_BLOCK ? left : NLQ_BLOCK) * NLMC_A;
        for (uint32_t c = threadIdx.x; c < cells; c += NLQ_BLOCK) {
            policy[base * NLMC_A + c] = s_pol[c];
            if (q.edges) q.edges[base * NLMC_A + c] = s_edge[c];
        }
        __syncthreads();
    }
}

// ---- memory: NLQ_MGROUP lanes per query, lane a < 9 reads the four fields of slot a (each wave-instruction covers 36 contiguous
// bytes of 4 rows) and writes its 16-byte Encounter: 144 contiguous bytes per query.  No collective.
__global__ __launch_bounds__(NLQ_BLOCK) void k_nl_memory(NlTable t, NlQuery q, rp_encounter* enc) {
    constexpr uint32_t QPB = NLQ_BLOCK / NLQ_MGROUP;
    const uint32_t a = threadIdx.x % NLQ_MGROUP;
    for (uint64_t i = (uint64_t)blockIdx.x * QPB + threadIdx.x / NLQ_MGROUP; i < q.n; i += (uint64_t)gridDim.x * QPB) {
        const uint64_t past = q.past[i], choices = q.choices[i];
        const uint32_t present = q.present[i], nch = nlq_nch(choices);
        const uint32_t home = (uint32_t)nl_key_hash(past, choices, present) & t.mask;
        const uint4* sl = reinterpret_cast<const uint4*>(t.slots + home);
        const uint4 lo = sl[0], hi = sl[1];
        uint4 e = make_uint4(0u, 0u, 0u, 0u);  // weight, regret, payoff, visits: rp_encounter's order
        if (a < NLMC_A) {
            const uint32_t* r = reinterpret_cast<const uint32_t*>(t.rows + (size_t)home * 4u * NLMC_A);
            e = make_uint4(r[NLMC_A + a], r[a], r[2u * NLMC_A + a], r[3u * NLMC_A + a]);
        }
        uint32_t row;
        const bool found = nlq_find(t, past, choices, present, home, lo, hi, &row);
        if (a < NLMC_A) {
            if (found && row != home) {
                const uint32_t* r = reinterpret_cast<const uint32_t*>(t.rows + (size_t)row * 4u * NLMC_A);
                e = make_uint4(r[NLMC_A + a], r[a], r[2u * NLMC_A + a], r[3u * NLMC_A + a]);
            }
            if (!found) e = make_uint4(0u, rp_f2u(nl_default_regret((uint32_t)(choices >> (5u * a)) & 31u)), 0u, 0u);
            if (a >= nch) e = make_uint4(0u, 0u, 0u, 0u);
            reinterpret_cast<uint4*>(enc)[i * NLMC_A + a] = e;
        }
        if (a == 0u) {
            if (q.n_actions) q.n_actions[i] = (uint8_t)nch;
            if (q.found) q.found[i] = found ? 1u : 0u;
        }
    }
}

}  // namespace rp

#endif
