// nlmc_world.hpp — the worlds of subgame solving: the opponent's range cut into RP_NLHE_WORLDS quantile worlds (rp_nlhe_partition,
// rp_nlhe_belief) and opponent holes dealt from a stated or sampled world (rp_nlhe_restrict).  Read-only, like nlmc_range.hpp.
//
// Reference: Partition::partition::<4> for Posterior<NlheSecret> (subgame/src/world/partition.rs:26-52), Belief::remember / weights
// (subgame/src/world/belief.rs:43-49), Nlhe::setup (nlhe/src/solver.rs:129-136), NlheEncoder::restrict (nlhe/src/encoder.rs:148-186).
// The rules are stated in include/rp_mi355x.h above rp_nlhe_partition.
//
// The factorisation.  The reference builds the belief once per solver and then, on every iteration, rejection-samples a hole: each
// attempt deals two cards, canonicalises the observation, looks its abstraction up and asks the belief's map.  The range kernel
// already leaves the bucket of EVERY hole the opponent could hold in LDS, so one workgroup answers one recall in five phases:
//   A, B  nlmc_range.hpp's, shared as functions: the public replay by lane 0; reach and head-street bucket of every candidate;
//   C     nlmc_range.hpp's: lane b folds the mass of bucket b;
//   D     the partition.  Lane b ranks its bucket among the entries (how many precede it: a larger mass, or an equal one and a
//         smaller b — 256 broadcast LDS reads) and scatters sorted[rank] = its mass; lane 0 runs the scan over at most 256 entries,
//         which is a serial f32 chain by definition and is not re-associated; then the lanes turn s_bucket[j] into the world of
//         candidate j;
//   E     the deals.  Lanes stride over the deals, each running its own attempt loop: two 32-bit hashes, two picks among the free
//         cards, the index of that pair among the candidates (j = hi (hi - 1) / 2 + lo, the inverse of nr_pair) and ONE LDS byte.
//         No isomorphism, no table probe, no global memory inside the loop.  A world without a member skips to the fallback attempt;
//         the loop bound is the constant RP_NLHE_MAX_REJECTIONS, so no input can hang it.
// No atomic and no store touches the table.  LDS: NrPublic 1.3 KB + reach 5.2 KB + bucket 1.3 KB + NwBelief 2.6 KB.
#ifndef RP_NLMC_WORLD_HPP
#define RP_NLMC_WORLD_HPP

#include "nlmc_range.hpp"

namespace rp {

#define NW_BLOCK NR_BLOCK
static_assert(NW_BLOCK == 256u, "one lane per bucket of the partition");
static_assert(RP_NLHE_WORLDS == 4u, "pokerkit::N_WORLDS");
static_assert(RP_NLHE_MAX_REJECTIONS < 32768u, "attempts are reported as uint16, and draw 2 + 2 a stays a small key");

struct NwArgs {
    const rp_nlhe_recall* recalls;
    // belief (any may be NULL): world [n][256], weights [n][4], hole_world [n][1326]
    uint8_t* world;
    float* weights;
    uint8_t* hole_world;
    // restrict (deals == 0: none): worlds [n][deals] (may be NULL: every world is drawn), holes / world_out / attempts [n][deals]
    uint32_t deals;
    const uint8_t* worlds;
    uint64_t step_hash;  // rp_node_hash_step(seed, 1)
    uint64_t first_id;   // the id of recalls[0]
    uint64_t* holes;
    uint8_t* world_out;
    uint16_t* attempts;
    uint8_t* status;  // may be NULL
};

#define NW_NEVER 0xffffffffu
struct NwBelief {
    float mass[256];
    float sorted[256];  // the entries' masses, descending and stable
    float weights[RP_NLHE_WORLDS];
    uint32_t members[RP_NLHE_WORLDS];  // entries of each world; an entry is a bucket some candidate has, so 0 here = no hole there
    uint32_t cut[RP_NLHE_WORLDS - 1];  // the sorted position after which the scan advanced from world k to k + 1, or NW_NEVER
    uint32_t flat;                     // total <= 0: every entry is of world 0
    uint8_t seen[256];
    uint8_t world[256];
};

// Phase D.  Called by the whole workgroup (it holds barriers) with lane b's mass and seen flag; on return bl.world[b] is the world of
// bucket b (RP_WORLD_NONE where it is no entry), bl.weights and bl.members are set, and every lane may read them.  The scan of lane 0
// only loads (the sorted masses, in order) and keeps the at most three positions where the world advances; the world of an entry is
// the number of those positions before its rank, which its own lane knows.
__device__ __forceinline__ void nw_partition(NwBelief& bl, float m, uint32_t any, uint32_t tid) {
    bl.mass[tid] = m;
    bl.seen[tid] = (uint8_t)(any ? 1u : 0u);
    bl.sorted[tid] = 0.0f;  // every slot is defined whatever the masses are (a NaN ranks nowhere)
    __syncthreads();
    uint32_t rank = 0;
    if (any) {
        for (uint32_t c = 0; c < 256u; ++c) {
            const float mc = bl.mass[c];
            const bool before = mc > m || (mc == m && c < tid);
            rank += (bl.seen[c] && before) ? 1u : 0u;
        }
        bl.sorted[rank] = m;  // rank < the number of entries <= 256
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t n = 0;
        float total = 0.0f;
        for (uint32_t b = 0; b < 256u; ++b)
            if (bl.seen[b]) {
                total += bl.mass[b];
                n += 1u;
            }
        uint32_t cut[RP_NLHE_WORLDS - 1] = {NW_NEVER, NW_NEVER, NW_NEVER};
        float weights[RP_NLHE_WORLDS] = {0.0f, 0.0f, 0.0f, 0.0f};
        const bool flat = total <= 0.0f;
        if (flat) {
#pragma unroll
            for (uint32_t w = 0; w < RP_NLHE_WORLDS; ++w) weights[w] = 0.25f;
        } else {
            const float segment = total / 4.0f;
            uint32_t index = 0;
            float bucket = 0.0f, accumulated = 0.0f;
            for (uint32_t i = 0; i < n; ++i) {
                const float reach = bl.sorted[i];
                bucket += reach;
                accumulated += reach;
                if (accumulated >= segment * (float)(index + 1u) && index < RP_NLHE_WORLDS - 1u) {
                    const float weight = bucket / total;
#pragma unroll
                    for (uint32_t w = 0; w < RP_NLHE_WORLDS - 1u; ++w) {
                        weights[w] = w == index ? weight : weights[w];
                        cut[w] = w == index ? i : cut[w];
                    }
                    index += 1u;
                    bucket = 0.0f;
                }
            }
            const float weight = bucket / total;
#pragma unroll
            for (uint32_t w = 0; w < RP_NLHE_WORLDS; ++w) weights[w] = w == index ? weight : weights[w];
        }
        bl.flat = flat ? 1u : 0u;
        // world w holds the sorted positions (cut[w - 1], cut[w]], the first from 0 and the last one reached up to n - 1
#pragma unroll
        for (uint32_t w = 0; w < RP_NLHE_WORLDS; ++w) {
            const uint32_t lo = w == 0u ? 0u : (cut[w - 1u] == NW_NEVER ? n : cut[w - 1u] + 1u);
            const uint32_t hi = (w < RP_NLHE_WORLDS - 1u && cut[w] != NW_NEVER) ? cut[w] + 1u : n;
            bl.weights[w] = weights[w];
            bl.members[w] = hi - lo;
            if (w < RP_NLHE_WORLDS - 1u) bl.cut[w] = cut[w];
        }
    }
    __syncthreads();
    uint32_t w = 0;
#pragma unroll
    for (uint32_t k = 0; k < RP_NLHE_WORLDS - 1u; ++k) w += bl.cut[k] < rank ? 1u : 0u;
    bl.world[tid] = (uint8_t)(!any ? RP_WORLD_NONE : (bl.flat ? 0u : w));
    __syncthreads();
}

// the world a deal draws (Density::sample shape over belief.weights()): x = u * the left fold of the weights, the first world whose
// running sum exceeds x; none: the highest world of non-zero weight (world 0 if there is none)
__device__ __forceinline__ uint32_t nw_draw_world(const float* weights, float u) {
    float total = 0.0f;
#pragma unroll
    for (uint32_t w = 0; w < RP_NLHE_WORLDS; ++w) total += weights[w];
    const float x = u * total;
    float acc = 0.0f;
    uint32_t world = 0, last = 0;
    bool hit = false;
#pragma unroll
    for (uint32_t w = 0; w < RP_NLHE_WORLDS; ++w) {
        acc += weights[w];
        const bool first = !hit && x < acc;
        world = first ? w : world;
        hit = hit || first;
        last = weights[w] != 0.0f ? w : last;
    }
    return hit ? world : last;
}

// attempt a of a deal: two distinct free cards as indices into free_card, hi > lo
__device__ __forceinline__ void nw_attempt(uint64_t tree_hash, uint32_t a, uint32_t n_free, uint32_t* hi, uint32_t* lo) {
    const uint32_t first = rp_pick_uniform(rp_node_hash_key(tree_hash, 1u + 2u * a), n_free);
    uint32_t second = rp_pick_uniform(rp_node_hash_key(tree_hash, 2u + 2u * a), n_free - 1u);
    second += second >= first ? 1u : 0u;  // the pick-th lowest of the rest
    *hi = max(first, second);
    *lo = min(first, second);
}

__global__ __launch_bounds__(NW_BLOCK) void k_nl_world(NlTable t, NlParams p, NwArgs q) {
    __shared__ NrPublic pub;
    __shared__ NwBelief bl;
    __shared__ float s_reach[RP_NLHE_MAX_HOLES];
    __shared__ uint8_t s_bucket[RP_NLHE_MAX_HOLES];  // phases B, C: the bucket of candidate j; from D on: its world
    const uint32_t r = blockIdx.x, tid = threadIdx.x;

    const uint32_t status = nr_recall(t, p, q.recalls[r], (int)RP_REACH_OPPONENT, true, pub, s_reach, s_bucket, nullptr, tid);
    const uint32_t count = status == RP_RECALL_OK ? pub.count : 0u;
    if (tid == 0 && q.status) q.status[r] = (uint8_t)status;

    float m;
    uint32_t any;
    nr_bucket_mass(s_reach, s_bucket, count, tid, &m, &any);
    nw_partition(bl, m, any, tid);
    if (q.world) q.world[(size_t)r * 256u + tid] = bl.world[tid];
    if (q.weights && tid < RP_NLHE_WORLDS) q.weights[(size_t)r * RP_NLHE_WORLDS + tid] = bl.weights[tid];
    for (uint32_t j = tid; j < RP_NLHE_MAX_HOLES; j += NW_BLOCK) {
        const uint32_t w = j < count ? (uint32_t)bl.world[s_bucket[j]] : RP_WORLD_NONE;
        if (j < count) s_bucket[j] = (uint8_t)w;
        if (q.hole_world) q.hole_world[(size_t)r * RP_NLHE_MAX_HOLES + j] = (uint8_t)w;
    }
    if (q.deals == 0u) return;
    __syncthreads();

    const uint32_t deals = q.deals, n_free = pub.n_free;
    for (uint32_t d = tid; d < deals; d += NW_BLOCK) {
        const size_t at = (size_t)r * deals + d;
        const uint32_t request = q.worlds ? (uint32_t)q.worlds[at] : RP_WORLD_NONE;
        uint64_t hole = 0;
        uint32_t world = RP_WORLD_NONE, attempts = 0;
        if (count != 0u && (request < RP_NLHE_WORLDS || request == RP_WORLD_NONE)) {
            const uint64_t tree_hash = rp_node_hash_tree(q.step_hash, (q.first_id + r) * deals + d);  // wrapping
            world = request < RP_NLHE_WORLDS ? request : nw_draw_world(bl.weights, rp_u01(rp_node_hash_key(tree_hash, 0)));
            uint32_t hi = 0, lo = 0, a = RP_NLHE_MAX_REJECTIONS;
            if (bl.members[world] != 0u)
                for (a = 0; a < RP_NLHE_MAX_REJECTIONS; ++a) {
                    nw_attempt(tree_hash, a, n_free, &hi, &lo);  // hi (hi - 1) / 2 + lo < count = n_free (n_free - 1) / 2
                    if (s_bucket[hi * (hi - 1u) / 2u + lo] == world) break;
                }
            if (a == RP_NLHE_MAX_REJECTIONS) nw_attempt(tree_hash, a, n_free, &hi, &lo);  // the fallback: whatever its world
            hole = (1ull << pub.free_card[hi]) | (1ull << pub.free_card[lo]);
            attempts = a;
        }
        q.holes[at] = hole;
        if (q.world_out) q.world_out[at] = (uint8_t)world;
        if (q.attempts) q.attempts[at] = (uint16_t)attempts;
    }
}

// rp_nlhe_partition: phase D alone, one workgroup per row
__global__ __launch_bounds__(NW_BLOCK) void k_nl_partition(const float* mass, const uint8_t* seen, uint8_t* world, float* weights) {
    __shared__ NwBelief bl;
    const uint32_t r = blockIdx.x, tid = threadIdx.x;
    nw_partition(bl, mass[(size_t)r * 256u + tid], seen[(size_t)r * 256u + tid] != 0, tid);
    world[(size_t)r * 256u + tid] = bl.world[tid];
    if (tid < RP_NLHE_WORLDS) weights[(size_t)r * RP_NLHE_WORLDS + tid] = bl.weights[tid];
}

}  // namespace rp

#endif
