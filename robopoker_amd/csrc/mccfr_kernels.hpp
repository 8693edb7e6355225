// mccfr_kernels.hpp — device-side data layout shared by the MCCFR kernels (mccfr_traverse.hpp, mccfr_update.hpp, traverse_static.hpp,
// sparse.hip) and mccfr.hip's host code, the per-cell map algebra of the composed update and the steps more than one kernel performs.
#ifndef RP_MCCFR_KERNELS_HPP
#define RP_MCCFR_KERNELS_HPP

#include <hip/hip_runtime.h>

#include "../../include/rp_math.h"
#include "../../include/rp_refrng.h"
#include "../../include/rp_libm_glibc.h"
#include "rp_internal.h"

namespace rp {

// rp_state repacked to one 16-byte load: x = turn | n_children << 8, y = info (chance states: rp_state.chance_info), z = offset
struct DevGame {
    const uint4* states;
    const uint32_t* children;
    const uint4* kids;            // [n_children] the child's state record, w = its state id; a terminal child of a
                                  // two-player game carries its payoffs in y, z (no further load on arrival)
    const float* payoffs;         // [n_terminals][n_players]
    const uint8_t* info_actions;  // [n_infos]
    const uint8_t* info_player;   // [n_infos]
    // infoset ids are in discovery order, so the players' infosets interleave: an infoset's rank among its player's infosets, the way
    // back, and the per-player counts (the block maps of the composed update are compacted by walker: bmap_index)
    const uint32_t* info_rank;    // [n_infos]
    const uint32_t* rank_info;    // [n_players][rank_max]
    uint32_t rank_count[8];       // infosets of player w (rp_game_table: at most 8 players)
    uint32_t rank_max;            // the largest of them, at least 1
    uint32_t n_players;
    uint32_t n_infos;
    uint32_t A;                   // table row stride (max_actions)
    uint32_t root;                // train_root
    uint4 root_rec;               // states[root] with w = root
    // games that match a compile-time skeleton (traverse_static.hpp), when every instance of a skeleton chance node has the
    // same number of outcomes: the words the traversal needs of the nodes below skeleton chance node c, down to the next chance
    // nodes (infoset ids, payoffs, the next draws' keys: RowLayout, traverse_static.hpp), side by side in one row per sequence of
    // chance outcomes (o_1, o_2, ..., o_c) on the path, root first: row (o_1 * fan_2 + o_2) * fan_3 + ... of the rows at
    // rows + row_base[c], RowLayout::stride[c] words apart.  What a node holds then depends on the sampled outcomes only, not on
    // its parent's record (a chain of ten dependent loads becomes four), and a lane fetches one row per chance outcome instead of
    // one record per node (Leduc: 13 16-byte loads from 5 rows instead of 37 from 37 records; the table is 25 KB, not 56)
    const uint4* rows;            // NULL: follow the child records
    uint32_t row_base[48];        // by skeleton chance node, in 16-byte units; a multiple of 8 (128-byte lines)
    uint32_t row_fan[48];         // outcomes of skeleton chance node s
};

// regret/strategy tables, SoA by field, row-major [info][A] (Encounter, solver/encounter.rs:22-27)
struct DevTables {
    float* regret;
    float* weight;
    float* payoff;
    uint32_t* visits;
};

// per-tree scratch, lane-interleaved: element (slot, tree) lives at base[slot * stride + tree] so the
// 64 lanes of a wave (64 consecutive trees) touch 64 consecutive dwords
struct DevScratch {
    uint32_t* n_meta;  // parent | edge << 8 | ptype << 16 | leaf << 18 | walker << 19 | nact << 24
    uint32_t* n_info;
    float* n_frel;
    float* n_fsmp;
    float* n_pay;
    float* n_rel;
    float* n_smp;
    float* n_acc;
    uint32_t* s_state;  // leaf stack (TreeBuilder::todo, builder.rs:54)
    uint32_t* s_meta;   // parent | edge << 8 | ptype << 16
    float* s_frel;
    float* s_fsmp;
    float* t_v;         // [A] action values of the span root being evaluated
    size_t stride;
    uint32_t maxn;      // node capacity per tree
    uint32_t maxs;      // stack capacity per tree
};

// Decisions of one batch (solver/decisions.rs:23-32), slot-major and lane-interleaved like the scratch
struct DevDecisions {
    uint32_t* info;     // [maxdec][stride]   0xffffffff = empty slot
    uint32_t* mask;     // [maxdec][stride]   edges present in the regret vector
    float* payoff;      // [maxdec][stride]
    float* regret;      // [maxdec][A][stride]
    float* policy;      // [maxdec][A][stride]
    uint8_t* slotmap;   // [n_infos][stride]  slot + 1 of the tree's Decisions for that infoset, 0 = none (large games)
    uint8_t* ndec;      // [stride]           Decisions produced by the tree
    size_t stride;
    uint32_t maxdec;
};

struct StepParams {
    uint64_t seed;
    uint64_t epoch;
    uint64_t tree_base;  // first tree id of this shard (rank * batch)
    uint32_t batch;
    uint32_t walker;
    int R, W, S;
    float temperature, smoothing, curiosity;
    float prune_threshold, prune_explore;
    uint64_t prune_warmup;
    float regret_min;
    float pow15, pow05;  // powf(t, 1.5), powf(t, 0.5) of t = (float)epoch: DiscountedRegret (host: rp_libm_glibc.h)
    unsigned long long* counters;  // [0] nodes, [1] infos, [2] error flags
    // reference-seed mode (rp_rng_kind RP_RNG_REFERENCE), NULL otherwise: DefaultHasher after t.hash() and info.hash()
    // (flow.rs:290-293) per infoset / per in-tree chance info, refreshed by k_prepare_ref every step
    const rp_sip_mid* ref_info;
    const rp_sip_mid* ref_chance;
};

// ------------------------------------------------------------------------------------------------
// the three draws of SamplingScheme::sample (sample/{mod,external,pluribus}.rs) in either rp_rng_kind.  `ci` = a chance state's
// chance_info (the record's y; 0 = the root deal, which keeps the counter hash in both modes), n its number of outcomes.
// REF is a compile-time switch in the skeleton kernels and p.ref_info != NULL elsewhere.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t d_draw_chance(const StepParams& p, bool ref, uint64_t tree_id, uint32_t state, uint32_t n, uint32_t ci) {
    if (ref && ci) return rp_ref_draw_range(rp_ref_seed_finish(&p.ref_chance[ci - 1u], tree_id), n);  // rng.random_range(0..n)
    return rp_pick_uniform(rp_node_hash(p.seed, p.epoch, tree_id, 0x80000000ull | state), n);
}
__device__ __forceinline__ float d_draw_weight(const StepParams& p, bool ref, uint64_t tree_id, uint32_t info, float total) {
    if (ref) return rp_ref_draw_weight(rp_ref_seed_finish(&p.ref_info[info], tree_id), total);  // Uniform::new(0, total).sample(rng)
    return rp_u01(rp_node_hash(p.seed, p.epoch, tree_id, info)) * total;
}
__device__ __forceinline__ float d_draw_coin(const StepParams& p, bool ref, uint64_t tree_id, uint32_t info) {
    if (ref) return rp_ref_draw_f32(rp_ref_seed_finish(&p.ref_info[info], tree_id));  // rng.random::<f32>()
    return rp_u01(rp_node_hash(p.seed, p.epoch, tree_id, info));
}

// per-cell composed map of the multi-GPU exchange (rp_mccfr_step_local / step_apply)
struct Cell {
    float ra, rb, rm;
    float wa, wb, wm;
    uint32_t rn, wn;
};
struct InfoSum {
    uint32_t count;
    float psum;
};

// the batch's Decisions sorted into one tree-id-ordered segment per infoset (k_count / k_scan / k_compact)
struct DevSorted {
    float* rw;         // [cap][2A]  per Decisions: regret delta a=0..A-1, then weight delta a=0..A-1
    uint32_t* mask;    // [cap]      edges present in the regret vector
    float* payoff;     // [cap]
    uint32_t* counts;  // [n_infos][n_chunks]
    uint32_t* offs;    // [n_infos][n_chunks]
    uint32_t* total;   // [n_infos]  segment length
    uint32_t n_chunks;
};

enum : uint32_t { PT_CHANCE = 0, PT_WALKER = 1, PT_OPP = 2, PT_NONE = 3 };
enum : uint32_t { ERR_NODE_CAPACITY = 1u, ERR_STACK_CAPACITY = 2u, ERR_DEC_CAPACITY = 4u };

// ------------------------------------------------------------------------------------------------
// schedules (regret/*.rs, policy/*.rs) and the per-cell map algebra of the composed update
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float d_regret_gain(int kind, float acc, float imm, float t, float pow15, float pow05, float floor_r) {
    float v;
    switch (kind) {
        case RP_REGRET_LINEAR: {
            const float discount = t / (t + 1.0f);
            v = acc * discount + imm;
        } break;
        case RP_REGRET_DISCOUNTED: {
            float x;
            if (acc > 0.0f) x = pow15;
            else if (acc < 0.0f) x = pow05;
            else x = t / 1.0f;
            const float discount = x / (x + 1.0f);
            v = acc * discount + imm;
        } break;
        case RP_REGRET_ASYMMETRIC: {
            if (acc > 0.0f) v = acc + imm;
            else {
                const float discount = t / (t + 1.0f);
                v = acc * discount + imm;
            }
        } break;
        default: v = acc + imm; break;  // Summed, Floored
    }
    return rp_maxf(v, floor_r);
}
__device__ __forceinline__ float d_weight_learn(int kind, float acc, float imm, float t) {
    float v;
    switch (kind) {
        case RP_WEIGHT_LINEAR: v = acc + imm * t; break;
        case RP_WEIGHT_QUADRATIC: v = acc + imm * t * t; break;
        case RP_WEIGHT_EXPONENTIAL: v = acc * 0.9999f + imm; break;
        default: v = acc + imm; break;
    }
    return rp_maxf(v, RP_EPSILON);
}
__host__ __device__ inline float regret_floor_of(int R, float regret_min) {
    if (R == RP_REGRET_FLOORED) return 0.0f;
    if (R == RP_REGRET_SUMMED) return rp_u2f(0xff800000u);
    return regret_min;
}

// WeightSchedule::accumulate's immediate term (policy/{linear,quadratic}.rs): sigma * t, sigma * t * t
__device__ __forceinline__ float weight_delta(int W, float sigma, float tf) {
    return W == RP_WEIGHT_LINEAR ? sigma * tf : (W == RP_WEIGHT_QUADRATIC ? sigma * tf * tf : sigma);
}
// per-cell constants of a composed chain: the sign-independent discount d and the floor of a regret or a weight cell
struct ChainParams {
    float d, fl;
};
__device__ __forceinline__ ChainParams chain_params(const StepParams& p, bool isreg, float tf) {
    const float fl = isreg ? regret_floor_of(p.R, p.regret_min) : RP_EPSILON;
    const float d = isreg ? (p.R == RP_REGRET_LINEAR ? tf / (tf + 1.0f) : 1.0f) : (p.W == RP_WEIGHT_EXPONENTIAL ? 0.9999f : 1.0f);
    return ChainParams{d, fl};
}

struct Map {
    float a, b, m;
    uint32_t n;
};
// The block maps of the composed update, and the group maps of their fold (k_combine2), are chunk-major and compacted by walker:
// row `blk` (a block = one chunk of RP_COMPOSE_CHUNK trees; a group = RP_FOLD_GROUP blocks) holds, for every infoset of the walker
// in rank order, 2A + 1 slots of 16 bytes: the cell maps (regret a = 0..A-1, then weight) and one slot {., payoff sum, ., count} with
// the sum in Map::b and the count in Map::n.  A chunk's writer fills one contiguous row; the fold reads lane = (rank, slot)
// and meets consecutive 16-byte words.  Every writer and the reader index through this function.
__host__ __device__ inline size_t bmap_index(uint32_t blk, uint32_t rank, uint32_t slot, uint32_t rank_max, uint32_t W2) {
    return ((size_t)blk * rank_max + rank) * (W2 + 1u) + slot;
}
// touches per LDS tile of the block-map chains
__host__ __device__ inline uint32_t compose_block(uint32_t max_actions) { return (1024u / (2u * max_actions)) & ~3u; }
// the composition of two maps that both hold a touch; `first` is applied first.  The one spelling of the algebra: map_compose and
// map_compose_select only decide when it applies
__device__ __forceinline__ Map map_compose_touched(const Map& first, const Map& second) {
    Map r;
    r.a = second.a * first.a;
    r.b = second.a * first.b + second.b;
    const float t = rp_f2u(first.m) == 0xff800000u ? first.m : second.a * first.m + second.b;
    r.m = rp_maxf(t, second.m);
    r.n = first.n + second.n;
    return r;
}
__device__ __forceinline__ Map map_compose(const Map& first, const Map& second) {  // `first` is applied first
    if (second.n == 0) return first;
    if (first.n == 0) return second;
    return map_compose_touched(first, second);
}
// map_compose without a branch, for the folds whose lanes run in lock step (k_combine2): the general case computed whether needed or
// not, then selected, so the bits are those of map_compose(first, second).  r.n == first.n + second.n in all three cases.
__device__ __forceinline__ Map map_compose_select(const Map& first, const Map& second) {
    const Map r = map_compose_touched(first, second);
    const bool keep = second.n == 0, take = first.n == 0;
    return Map{keep ? first.a : (take ? second.a : r.a), keep ? first.b : (take ? second.b : r.b), keep ? first.m : (take ? second.m : r.m), r.n};
}

// first touch of an empty map sets (d, delta, floor); later touches compose one step (oracle: map_touch)
__device__ __forceinline__ void map_touch(Map& mp, float d, float delta, float floor_v) {
    if (mp.n == 0) {
        mp.a = d;
        mp.b = delta;
        mp.m = floor_v;
    } else {
        mp.a = mp.a * d;
        mp.b = mp.b * d + delta;
        mp.m = rp_maxf(mp.m * d + delta, floor_v);
    }
    mp.n += 1;
}
// map_touch without a branch, for the chains that run in lock step: equals map_touch when `skip` is false and leaves the map
// alone when it is true (a pruned edge is not touched at all: a touch would apply the discount)
__device__ __forceinline__ void map_touch_unless(Map& mp, bool skip, float d, float delta, float floor_v) {
    const float na = mp.n ? mp.a * d : d;
    const float nb = mp.n ? mp.b * d + delta : delta;
    const float nm = mp.n ? rp_maxf(mp.m * d + delta, floor_v) : floor_v;
    mp.a = skip ? mp.a : na;
    mp.b = skip ? mp.b : nb;
    mp.m = skip ? mp.m : nm;
    mp.n += skip ? 0u : 1u;
}
// map_touch_unless for a discount of exactly 1.0f (Summed / Floored regret, Constant / Linear / Quadratic weight: chain_params):
// the same expressions without the `* d`.  x * 1.0f == x for every float, -0 and +-inf included, so the bits are those of
// map_touch_unless(mp, skip, 1.0f, delta, floor_v).
__device__ __forceinline__ void map_touch_unit_unless(Map& mp, bool skip, float delta, float floor_v) {
    const float na = mp.n ? mp.a : 1.0f;
    const float nb = mp.n ? mp.b + delta : delta;
    const float nm = mp.n ? rp_maxf(mp.m + delta, floor_v) : floor_v;
    mp.a = skip ? mp.a : na;
    mp.b = skip ? mp.b : nb;
    mp.m = skip ? mp.m : nm;
    mp.n += skip ? 0u : 1u;
}
__device__ __forceinline__ Map map_identity() { return Map{1.0f, 0.0f, rp_u2f(0xff800000u), 0u}; }
// the payoff slot of a block-map row (bmap_index): only b and n are read
__device__ __forceinline__ Map map_sum_slot(float psum, uint32_t count) { return Map{1.0f, psum, rp_u2f(0xff800000u), count}; }
// F(x) = max(a x + b, m) of a map that holds at least one touch; map_apply: any map (no touch = the identity)
__device__ __forceinline__ float map_eval(const Map& mp, float x) { return rp_maxf(mp.a * x + mp.b, mp.m); }
__device__ __forceinline__ float map_apply(const Map& mp, float x) { return mp.n ? map_eval(mp, x) : x; }
// a batch's (payoff sum, count) folded into a cell's (mean payoff, visits)
__device__ __forceinline__ void fold_payoff(float& ev, uint32_t& visits, float psum, uint32_t count) {
    if (count) {
        const uint32_t n2 = visits + count;
        ev = ev + (psum - (float)count * ev) / (float)n2;
        visits = n2;
    }
}
// the regret and the weight half of a Cell as maps
__device__ __forceinline__ Map cell_regret(const Cell& c) { return Map{c.ra, c.rb, c.rm, c.rn}; }
__device__ __forceinline__ Map cell_weight(const Cell& c) { return Map{c.wa, c.wb, c.wm, c.wn}; }
__device__ __forceinline__ void cell_set_regret(Cell& c, const Map& mp) { c.ra = mp.a; c.rb = mp.b; c.rm = mp.m; c.rn = mp.n; }
__device__ __forceinline__ void cell_set_weight(Cell& c, const Map& mp) { c.wa = mp.a; c.wb = mp.b; c.wm = mp.m; c.wn = mp.n; }

// ------------------------------------------------------------------------------------------------
// per-infoset, tree-ordered lists of one chunk of CH_TREES trees: an LDS bitmap [infoset][tree] marks the trees that produced
// Decisions for the infoset; the place of a tree's Decisions in the infoset's list is a prefix popcount of that bitmap row
// ------------------------------------------------------------------------------------------------
#define CH_TREES 256u     // trees per compaction chunk == RP_COMPOSE_CHUNK (a block of the composed update)
#define SM_WORDS (CH_TREES / 32u)
static_assert(CH_TREES == RP_COMPOSE_CHUNK, "a block of the composed update is one compaction chunk of trees");
// pre[info][w] = trees before word w that visited the infoset; returns the length of the infoset's list
__device__ __forceinline__ uint32_t list_prefix(const uint32_t* bits, uint16_t* pre, uint32_t info) {
    uint32_t run = 0;
    for (uint32_t w = 0; w < SM_WORDS; ++w) {
        pre[info * SM_WORDS + w] = (uint16_t)run;
        run += __popc(bits[info * SM_WORDS + w]);
    }
    return run;
}
// place of local tree `lt` in the infoset's list
__device__ __forceinline__ uint32_t list_rank(const uint32_t* bits, const uint16_t* pre, uint32_t info, uint32_t lt) {
    return pre[info * SM_WORDS + (lt >> 5)] + __popc(bits[info * SM_WORDS + (lt >> 5)] & ((1u << (lt & 31u)) - 1u));
}

}  // namespace rp

#endif
