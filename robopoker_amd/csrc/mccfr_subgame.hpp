// mccfr_subgame.hpp — the safe subgame re-solve for rp_game_table games (rp_mccfr_subgame_belief / rp_mccfr_subgame_solve, include/
// rp_mi355x.h): SubGameSolver with origin = None over WorldProfile over the handle's dense tables, and the Posterior -> Belief step
// in front of it.  f32 order is part of the contract (the header's paragraphs); compiled -ffp-contract=off.
//
// Shape: ONE WAVEFRONT PER SOLVE (workgroup = 64 lanes, wave-synchronous: ms_sync, no workgroup barrier).  The iterations of a solve
// are a serial chain, so the width comes from the nodes of one small tree (<= 62: a lane per node) and from the solves in flight.
//   per iteration   world and restricted entry state (every lane, the same scalars) -> tree (lane 0: the builder's stack is serial, and
//                   it draws at the other seat's nodes) -> pol = iterated distribution per decision node (a lane per node) -> per
//                   walker node `root`, in node order: rr / sr top-down and the nested value folds bottom-up, one tree level per
//                   step, a lane per node of root's subtree; lane 0 folds root's action values into the infoset's Decisions ->
//                   rows of new infosets allocated (lane 0) -> the four updates, a lane per (Decisions, slot).
//   LDS (16.5 KB per solve, nine solves per CU by LDS; 93 VGPRs, no scratch): the tree, pol and q per node, the Decisions.
//   device region   per solve, kept on the handle between the launches of one call: a header (status, counters), the u16 index
//                   [4][n_infos] -> row, the rows' keys and the rows themselves ([rows][A] rp_encounter).  The blueprint is read
//                   from the handle's tables in place; there is no LDS copy of either (what that costs has not been measured).
// A launch runs iterations [t_begin, t_end) of every solve; the last one harvests.  Every loop is bounded by a constant of this file
// or a count the table check has validated; every index an entry supplies is checked before it is used.
//
// The kernel is instantiated twice.  FR = false is rp_mccfr_subgame_solve's and carries none of what follows (same registers, LDS and
// code as before the frontiers existed).  FR = true is rp_mccfr_depth_solve's (SubGameSolver::with_origin, DepthSolver): a chance state
// deeper than the solve's origin grows the Pick game — the frontier node keeps one Internal(k) child, that node D External(k, j)
// leaves — so a node carries a kind beside its state (k and j are the slots of the Internal and the External node), a Pick infoset is
// numbered n_infos + pick id in the index, the keys and the Decisions, and the matrix is read in place at the leaf.  64 + 4 bytes of
// LDS more (16 608 B, still nine solves per CU), no scratch.
#ifndef RP_MCCFR_SUBGAME_HPP
#define RP_MCCFR_SUBGAME_HPP

#include <type_traits>

#include "mccfr_kernels.hpp"
#include "policy_dist.hpp"

namespace rp {

constexpr uint32_t MS_LANES = 64;
constexpr uint32_t MS_NODES = RP_MCCFR_SUBGAME_MAX_NODES;
constexpr uint32_t MS_A = RP_MAX_ACTIONS;
constexpr uint32_t MS_NONE = 0xffu;      // no parent / no kid
constexpr uint32_t MS_NO_ROW = 0xffffu;  // the index's "no local row"
constexpr uint32_t MS_MAX_CHUNK = 2048;  // solves per launch

// the per-solve region's header
struct MsHead {
    uint32_t status, n_rows;
    unsigned long long nodes, infosets;
    uint32_t drawn[4];
    uint32_t fallbacks, frontiers, pad[4];
};  // 64 bytes

struct MsRegion {
    uint8_t* base;
    size_t stride;       // bytes per solve
    uint32_t off_index;  // u16 [4][n_keys]: n_keys = n_infos, + n_pick with frontiers
    uint32_t off_keys;   // u32 [rows_alloc]: world * n_keys + info
    uint32_t off_perm;   // u16 [rows_alloc]: the rows in exported order
    uint32_t off_rows;   // rp_encounter [rows_alloc][A]
    uint32_t rows_alloc;
};

struct MsParams {
    const rp_mccfr_subgame_entry* entries;
    rp_mccfr_subgame_result* results;
    rp_mccfr_subgame_row* rows;
    uint32_t rows_cap, n, n_states, n_terminals;
    uint64_t seed, first_id;  // first_id: the id of this launch's solve 0
    uint32_t t_begin, t_end, iterations;
    float prior;  // k of the warmstart; its regret (blueprint * k / epoch) is unobservable (PROFILE) and is not computed
    DistParams hp;
};

// the handle's frontier tables (rp_mccfr_set_frontiers), validated on the host against the game table
struct MsFrontiers {
    const uint8_t* depth;        // [n_states]
    const uint32_t* pick_info;   // [n_states]
    const uint32_t* payoff_ref;  // [n_states]
    const float* matrices;       // [n_matrices][D][D]
    uint32_t n_pick, n_matrices, D;
};
struct MsParamsDepth : MsParams {
    MsFrontiers fr;
    const uint8_t* origin;  // [n] or nullptr = RP_MCCFR_ORIGIN_ENTRY
};
template <bool FR>
using MsParamsOf = typename std::conditional<FR, MsParamsDepth, MsParams>::type;

enum : uint32_t { MS_GAME = 0, MS_FRONTIER = 1, MS_INTERNAL = 2, MS_EXTERNAL = 3 };  // a node's kind

__device__ __forceinline__ void ms_sync() {  // orders this wavefront's LDS and region traffic
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

struct MsLds {
    rp_mccfr_subgame_entry entry;
    uint32_t state[MS_LANES], info[MS_LANES], off[MS_LANES];
    uint8_t parent[MS_LANES], slot[MS_LANES], turn[MS_LANES], nch[MS_LANES], depth[MS_LANES], in[MS_LANES];
    uint8_t kid[MS_LANES][MS_A];
    float pol[MS_LANES][MS_A], q[MS_LANES][MS_A];
    float rr[MS_LANES], sr[MS_LANES], val[MS_LANES];
    uint32_t st_state[MS_LANES];
    uint8_t st_parent[MS_LANES], st_slot[MS_LANES];
    uint32_t dec_info[MS_LANES];
    uint16_t dec_row[MS_LANES];
    uint8_t dec_head[MS_LANES], dec_new[MS_LANES];
    float dec_pay[MS_LANES], dec_delta[MS_LANES][MS_A];
    uint32_t n_nodes, n_dec, max_depth, fail;
};
template <bool FR>
struct MsLdsOf : MsLds {};
template <>
struct MsLdsOf<true> : MsLds {
    uint8_t kind[MS_LANES];
    uint32_t n_front;  // the frontier nodes of this tree
};

// one solve's view of the profile: the handle's tables under the region's local rows.  With frontiers `info` at or past n_infos is
// the Pick infoset info - n_infos, which the blueprint does not hold: DepthView's constants answer for an absent edge.
template <bool FR>
struct MsProfile {
    DevTables t;
    uint32_t A, n_infos;
    uint16_t* index;
    rp_encounter* rows;
    uint32_t n_keys;    // the index's stride: n_infos (+ n_pick)
    uint32_t row_A;     // the slots of a local row: max(A, D), a Pick row has D
    float pick_weight;  // 1.0f / (float)D

    __device__ __forceinline__ uint32_t row_slots() const { return FR ? row_A : A; }

    __device__ __forceinline__ uint32_t row(uint32_t world, uint32_t info) const { return index[(size_t)world * (FR ? n_keys : n_infos) + info]; }
    __device__ __forceinline__ float cum_regret(uint32_t r, uint32_t info, uint32_t a) const {
        if (FR && r == MS_NO_ROW && info >= n_infos) return RP_EPSILON;
        return r != MS_NO_ROW ? rows[(size_t)r * row_slots() + a].regret : rp_maxf(t.regret[(size_t)info * A + a], RP_EPSILON);
    }
    __device__ __forceinline__ float cum_weight(uint32_t r, uint32_t info, uint32_t a) const {
        if (FR && r == MS_NO_ROW && info >= n_infos) return pick_weight;
        return r != MS_NO_ROW ? rows[(size_t)r * row_slots() + a].weight : rp_maxf(t.weight[(size_t)info * A + a], RP_EPSILON);
    }
    __device__ __forceinline__ float cum_payoff(uint32_t r, uint32_t info, uint32_t a) const {
        if (FR && r == MS_NO_ROW && info >= n_infos) return 0.0f;
        return r != MS_NO_ROW ? rows[(size_t)r * row_slots() + a].payoff : t.payoff[(size_t)info * A + a];
    }
    __device__ __forceinline__ uint32_t cum_visits(uint32_t r, uint32_t info, uint32_t a) const {
        if (FR && r == MS_NO_ROW && info >= n_infos) return 0u;
        return r != MS_NO_ROW ? rows[(size_t)r * row_slots() + a].visits : t.visits[(size_t)info * A + a];
    }
    // iterated_distribution of regret() / sampling_distribution of weight(): out[a], a < na
    __device__ __forceinline__ void iterated(uint32_t r, uint32_t info, uint32_t na, float* out) const {
        float v[MS_A];
        for (uint32_t a = 0; a < MS_A; ++a) v[a] = a < na ? cum_regret(r, info, a) : 0.0f;
        policy_distribution<MS_A>((int)RP_DIST_ITERATED, DistParams{}, v, na, out);
    }
    __device__ __forceinline__ void sampling(const DistParams& hp, uint32_t r, uint32_t info, uint32_t na, float* out) const {
        float v[MS_A];
        for (uint32_t a = 0; a < MS_A; ++a) v[a] = a < na ? cum_weight(r, info, a) : 0.0f;
        policy_distribution<MS_A>((int)RP_DIST_SAMPLING, hp, v, na, out);
    }
};

// the statuses an entry has before any iteration, in the header's order
__device__ __forceinline__ uint32_t ms_validate(const rp_mccfr_subgame_entry& e, uint32_t n_states, uint32_t n_infos) {
    if (e.external > 1) return RP_MSUB_SEAT;
    if (e.n_worlds < 1 || e.n_worlds > 4) return RP_MSUB_WORLDS;
    if (e.n_candidates > RP_MCCFR_SUBGAME_MAX_CANDIDATES) return RP_MSUB_COUNT;
    if (e.observed >= n_states) return RP_MSUB_STATE;
    for (uint32_t c = 0; c < e.n_candidates; ++c)
        if (e.candidate[c] >= n_states) return RP_MSUB_STATE;
    for (uint32_t c = 0; c < e.n_candidates; ++c)
        if (e.secret[c] >= 16) return RP_MSUB_SECRET;
    for (uint32_t w = 0; w < e.n_worlds; ++w) {
        const float x = e.weights[w];
        if (!(x >= 0.0f) || x > RP_F32_MAX) return RP_MSUB_WEIGHT;
    }
    if (e.harvest_info != RP_NO_INFO && e.harvest_info >= n_infos) return RP_MSUB_INFO;
    return RP_MSUB_OK;
}

// World rule of RESTRICT over weights[0 .. W)
__device__ __forceinline__ uint32_t ms_draw_world(const rp_mccfr_subgame_entry& e, uint64_t h) {
    const uint32_t W = e.n_worlds;
    float total = 0.0f;
    for (uint32_t w = 0; w < W; ++w) total += e.weights[w];
    const float x = rp_u01(h) * total;
    float run = 0.0f;
    for (uint32_t w = 0; w < W; ++w) {
        run += e.weights[w];
        if (x < run) return w;
    }
    uint32_t last = 0;
    for (uint32_t w = 0; w < W; ++w)
        if (e.weights[w] != 0.0f) last = w;
    return last;
}

// the weighted draw of DRAWS over q[0 .. nch) with the node's hash; q is kept for the node's sr
template <bool FR>
__device__ __forceinline__ uint32_t ms_weighted_pick(MsLdsOf<FR>& L, uint32_t idx, const float* q, uint32_t nch, uint64_t tree_hash) {
    float total = 0.0f;
    for (uint32_t a = 0; a < nch; ++a) {
        L.q[idx][a] = q[a];
        total += rp_maxf(q[a], RP_EPSILON);
    }
    const float u = rp_u01(rp_node_hash_key(tree_hash, idx)) * total;
    float cum = 0.0f;
    uint32_t pick = 0;
    for (uint32_t a = 0; a + 1 < nch; ++a) {
        cum += rp_maxf(q[a], RP_EPSILON);
        if (pick == a && cum <= u) pick = a + 1;
    }
    return pick;
}

// lane 0: TreeBuilder with ExternalSampling; RP_MSUB_OK, RP_MSUB_TREE when the tree outgrows MS_NODES, with frontiers RP_MSUB_FRONTIER
// too, and a node under a frontier keeps the frontier's state (the Internal node and its External leaves).
template <bool FR>
__device__ inline uint32_t ms_build(MsLdsOf<FR>& L, const DevGame& g, const MsProfile<FR>& P, const MsParamsOf<FR>& p, uint32_t entry_state,
                                    uint32_t world, uint32_t walker, uint64_t tree_hash, uint32_t origin, uint32_t external) {
    uint32_t n = 0, sp = 0, max_depth = 0;
    L.st_state[0] = entry_state;
    L.st_parent[0] = (uint8_t)MS_NONE;
    L.st_slot[0] = 0;
    sp = 1;
    if constexpr (FR) L.n_front = 0;
    while (sp > 0) {
        sp -= 1;
        const uint32_t state = L.st_state[sp], parent = L.st_parent[sp], slot = L.st_slot[sp];
        if (n >= MS_NODES) return RP_MSUB_TREE;
        const uint32_t idx = n++;
        const uint4 rec = g.states[state];
        const uint32_t turn = rec.x & 255u, nch = (rec.x >> 8) & 255u;
        const uint32_t depth = parent == MS_NONE ? 0u : (uint32_t)L.depth[parent] + 1u;
        max_depth = depth > max_depth ? depth : max_depth;
        L.state[idx] = state;
        L.info[idx] = rec.y;
        L.off[idx] = rec.z;
        L.parent[idx] = (uint8_t)parent;
        L.slot[idx] = (uint8_t)slot;
        L.turn[idx] = (uint8_t)turn;
        L.depth[idx] = (uint8_t)depth;
        for (uint32_t a = 0; a < MS_A; ++a) L.kid[idx][a] = (uint8_t)MS_NONE;
        if (parent != MS_NONE) L.kid[parent][slot] = (uint8_t)idx;
        if constexpr (FR) {
            const MsFrontiers& f = p.fr;
            const uint32_t above = parent == MS_NONE ? (uint32_t)MS_GAME : (uint32_t)L.kind[parent];
            if (above == MS_INTERNAL) {  // External(k, j): k the Internal node's slot, j this node's
                L.kind[idx] = (uint8_t)MS_EXTERNAL;
                L.turn[idx] = (uint8_t)RP_TURN_TERMINAL;
                L.nch[idx] = 0;
                continue;
            }
            if (above == MS_FRONTIER) {  // Internal(k): the seat `external` picks j, by the Pick infoset of the frontier's state
                const uint32_t D = f.D, info = P.n_infos + f.pick_info[state];  // checked when the frontier was grown
                L.kind[idx] = (uint8_t)MS_INTERNAL;
                L.turn[idx] = (uint8_t)external;
                L.info[idx] = info;
                L.nch[idx] = (uint8_t)D;
                uint32_t first = 0, count = D;
                if (external != walker) {
                    float q[MS_A];
                    P.sampling(p.hp, P.row(world, info), info, D, q);
                    first = ms_weighted_pick<FR>(L, idx, q, D, tree_hash);
                    count = 1;
                }
                if (n + sp + count > MS_NODES) return RP_MSUB_TREE;
                for (uint32_t k = first; k < first + count; ++k) {
                    L.st_state[sp] = state;
                    L.st_parent[sp] = (uint8_t)idx;
                    L.st_slot[sp] = (uint8_t)k;
                    sp += 1;
                }
                continue;
            }
            L.kind[idx] = (uint8_t)MS_GAME;
            if (turn == RP_TURN_CHANCE && (uint32_t)f.depth[state] > origin) {  // DepthGame::at_frontier
                const uint32_t ref = f.payoff_ref[state];
                const bool named = ref == RP_NO_INFO || ((ref & 0x80000000u) ? (ref & 0x7fffffffu) < f.n_matrices : ref < P.n_infos);
                if (f.pick_info[state] >= f.n_pick || !named || f.D < 1 || f.D > 4) return RP_MSUB_FRONTIER;
                L.kind[idx] = (uint8_t)MS_FRONTIER;
                L.nch[idx] = 0;
                L.n_front += 1;
                if (n + sp + 1 > MS_NODES) return RP_MSUB_TREE;
                L.st_state[sp] = state;
                L.st_parent[sp] = (uint8_t)idx;
                L.st_slot[sp] = (uint8_t)rp_pick_uniform(rp_node_hash_key(tree_hash, idx), f.D);
                sp += 1;
                continue;
            }
        }
        // rp_game_table_check (games.cpp) refuses a state that is not terminal and has no child, or more than RP_MAX_ACTIONS: the two
        // conditions on nch only keep the loops below bounded for a table that was not checked; such a node would read as a leaf of value 0
        const bool decision = turn < 2u && nch > 0 && nch <= MS_A;
        L.nch[idx] = decision ? (uint8_t)nch : 0;
        if (!decision) continue;  // a chance or terminal state has no branch
        uint32_t first = 0, count = nch;
        if (turn != walker) {  // the weighted draw of DRAWS
            float q[MS_A];
            P.sampling(p.hp, P.row(world, rec.y), rec.y, nch, q);
            first = ms_weighted_pick<FR>(L, idx, q, nch, tree_hash);
            count = 1;
        }
        if (n + sp + count > MS_NODES) return RP_MSUB_TREE;  // every pending branch becomes a node
        for (uint32_t k = first; k < first + count; ++k) {
            L.st_state[sp] = g.children[rec.z + k];
            L.st_parent[sp] = (uint8_t)idx;
            L.st_slot[sp] = (uint8_t)k;
            sp += 1;
        }
    }
    L.n_nodes = n;
    L.max_depth = max_depth;
    return RP_MSUB_OK;
}

// CfrNash::terminal_value of a leaf for hero
template <bool FR>
__device__ __forceinline__ float ms_leaf_value(const MsLdsOf<FR>& L, const DevGame& g, const MsProfile<FR>& P, const MsParamsOf<FR>& p, uint32_t node,
                                               uint32_t world, uint32_t hero, uint32_t external) {
    if constexpr (FR) {
        if (L.kind[node] == MS_EXTERNAL) {  // DepthGame::payoff at External(k, j): payoffs[k][j] to `internal`, negated to the other seat
            const MsFrontiers& f = p.fr;
            const uint32_t par = L.parent[node], j = L.slot[node], k = par < MS_LANES ? (uint32_t)L.slot[par] : 0u;
            const uint32_t ref = f.payoff_ref[L.state[node]];  // checked when the frontier was grown
            float v = 0.0f;  // RP_NO_INFO: Payoffs::uniform(0.0)
            if (ref != RP_NO_INFO) {
                if (ref & 0x80000000u) {
                    const uint32_t m = ref & 0x7fffffffu;
                    if (m < f.n_matrices && k < f.D && j < f.D) v = f.matrices[((size_t)m * f.D + k) * f.D + j];
                } else if (ref < P.n_infos) {
                    v = P.t.payoff[(size_t)ref * P.A];  // the blueprint's cum_payoff(info, slot 0), never a local row
                }
            }
            return hero == 1u - external ? v : -v;
        }
    }
    const uint32_t turn = L.turn[node];
    if (turn == RP_TURN_TERMINAL) return L.off[node] < p.n_terminals ? g.payoffs[(size_t)L.off[node] * 2 + hero] : 0.0f;
    const uint32_t par = L.parent[node];
    if (turn != RP_TURN_CHANCE || par == MS_NONE) return 0.0f;
    const uint32_t info = L.info[par];  // a chance state has no branch here, so the parent is the nearest ancestor that is not chance
    return P.cum_payoff(P.row(world, info), info, 0);
}

template <bool FR>
__global__ __launch_bounds__(MS_LANES) void k_mccfr_subgame_solve(DevGame g, DevTables tab, MsRegion R, MsParamsOf<FR> p) {
    __shared__ MsLdsOf<FR> L;
    const uint32_t lane = threadIdx.x, solve = blockIdx.x;
    if (solve >= p.n) return;
    uint8_t* reg = R.base + (size_t)solve * R.stride;
    MsHead* head = reinterpret_cast<MsHead*>(reg);
    MsProfile<FR> P{tab, g.A, g.n_infos, reinterpret_cast<uint16_t*>(reg + R.off_index), reinterpret_cast<rp_encounter*>(reg + R.off_rows)};
    uint32_t* keys = reinterpret_cast<uint32_t*>(reg + R.off_keys);
    uint16_t* perm = reinterpret_cast<uint16_t*>(reg + R.off_perm);
    const uint32_t A = g.A, NI = g.n_infos;
    uint32_t NK = NI, PD = 0, RA = A;  // the keys of one world (infosets, then Pick infosets), the Pick game's D, a local row's slots
    if constexpr (FR) {
        PD = p.fr.D;
        NK = NI + p.fr.n_pick;
        RA = A > PD ? A : PD;
        P.n_keys = NK;
        P.row_A = RA;
        P.pick_weight = 1.0f / (float)PD;
    }
    // the slots of a key: an infoset's actions, D at a Pick infoset
    const auto actions_of = [&](uint32_t info) -> uint32_t { return FR && info >= NI ? PD : (uint32_t)g.info_actions[info]; };

    {  // the entry, once per launch
        const uint32_t* src = reinterpret_cast<const uint32_t*>(p.entries + solve);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&L.entry);
        for (uint32_t i = lane; i < sizeof(rp_mccfr_subgame_entry) / 4; i += MS_LANES) dst[i] = src[i];
    }
    if (p.t_begin == 0) {  // a new solve: an empty local profile
        for (uint32_t i = lane; i < 4 * NK; i += MS_LANES) P.index[i] = (uint16_t)MS_NO_ROW;
        if (lane < sizeof(MsHead) / 4) reinterpret_cast<uint32_t*>(head)[lane] = 0u;
    }
    ms_sync();
    const rp_mccfr_subgame_entry& E = L.entry;
    uint32_t status = p.t_begin == 0 ? ms_validate(E, p.n_states, NI) : head->status;
    uint32_t n_rows = head->n_rows, fallbacks = head->fallbacks, drawn[4] = {head->drawn[0], head->drawn[1], head->drawn[2], head->drawn[3]};
    unsigned long long nodes = head->nodes, infosets = head->infosets;
    const uint64_t id = p.first_id + solve;
    bool members_empty = true;
    if (status == RP_MSUB_OK)
        for (uint32_t s = 0; s < 16; ++s) members_empty = members_empty && E.world_of[s] >= E.n_worlds;
    uint32_t entry_state = 0;
    uint32_t origin = RP_MCCFR_ORIGIN_NONE, frontiers = 0;
    if constexpr (FR) {
        frontiers = head->frontiers;
        origin = p.origin ? (uint32_t)p.origin[solve] : (uint32_t)RP_MCCFR_ORIGIN_ENTRY;
        if (origin == RP_MCCFR_ORIGIN_ENTRY) origin = status == RP_MSUB_OK ? (uint32_t)p.fr.depth[E.observed] : (uint32_t)RP_MCCFR_ORIGIN_NONE;
    }

    for (uint32_t t = p.t_begin; t < p.t_end && status == RP_MSUB_OK; ++t) {
        const uint32_t walker = t & 1u;
        const uint32_t world = ms_draw_world(E, rp_node_hash(p.seed, 1, id, t));
        drawn[world] += 1;
        entry_state = E.observed;
        bool chosen = false;
        for (uint32_t c = 0; c < E.n_candidates && !chosen; ++c)
            if (members_empty || E.world_of[E.secret[c]] == world) {
                entry_state = E.candidate[c];
                chosen = true;
            }
        fallbacks += chosen ? 0u : 1u;
        if (lane == 0) {
            const uint64_t tree_hash = rp_node_hash_tree(rp_node_hash_step(p.seed, 2), id * RP_MCCFR_SUBGAME_MAX_ITERATIONS + t);
            L.n_dec = 0;
            const uint32_t built = ms_build<FR>(L, g, P, p, entry_state, world, walker, tree_hash, origin, E.external);
            L.fail = FR ? built : (built != RP_MSUB_OK ? 1u : 0u);
        }
        ms_sync();
        if (L.fail) {
            status = FR ? L.fail : (uint32_t)RP_MSUB_TREE;
            break;
        }
        const uint32_t N = L.n_nodes, max_depth = L.max_depth;
        nodes += N;
        if constexpr (FR) frontiers += L.n_front;
        // pol = iterated_distribution (= regret(a) / rd, the same operations) of every decision node
        if (lane < N && L.nch[lane] > 0) {
            float out[MS_A];
            const uint32_t info = L.info[lane];
            P.iterated(P.row(world, info), info, L.nch[lane], out);
            for (uint32_t a = 0; a < MS_A; ++a) L.pol[lane][a] = out[a];
        }
        ms_sync();
        // VALUES: the walker's nodes in node order
        for (uint32_t root = 0; root < N; ++root) {
            if (L.turn[root] != walker || L.nch[root] == 0) continue;
            const uint32_t d0 = L.depth[root];
            const bool mine = lane < N && L.depth[lane] > d0;
            L.in[lane] = 0;
            ms_sync();
            for (uint32_t d = d0 + 1; d <= max_depth; ++d) {  // rr, sr from the root's children down
                if (mine && L.depth[lane] == d) {
                    const uint32_t par = L.parent[lane], s = L.slot[lane];
                    if (par == root) {
                        L.rr[lane] = 1.0f;
                        L.sr[lane] = 1.0f;
                        L.in[lane] = 1;
                    } else if (L.in[par]) {
                        bool chance = false;  // a frontier node is the chance node it was grown as: neither rr nor sr moves
                        if constexpr (FR) chance = L.kind[par] == MS_FRONTIER;
                        if (chance) {
                            L.rr[lane] = L.rr[par];
                            L.sr[lane] = L.sr[par];
                        } else {
                            L.rr[lane] = L.rr[par] * L.pol[par][s];
                            L.sr[lane] = L.turn[par] != walker ? L.sr[par] * L.q[par][s] : L.sr[par];
                        }
                        L.in[lane] = 1;
                    }
                }
                ms_sync();
            }
            for (uint32_t d = max_depth; d > d0; --d) {  // recursed_value, the deepest level first
                if (mine && L.depth[lane] == d && L.in[lane]) {
                    float v;
                    bool leaf = L.nch[lane] == 0;
                    if constexpr (FR) leaf = leaf && L.kind[lane] != MS_FRONTIER;  // a frontier node folds its one child
                    if (leaf) {
                        v = (L.rr[lane] / L.sr[lane]) * ms_leaf_value<FR>(L, g, P, p, lane, world, walker, E.external);
                    } else {
                        v = 0.0f;
                        for (uint32_t a = 0; a < MS_A; ++a)
                            if (L.kid[lane][a] != MS_NONE) v += L.val[L.kid[lane][a]];
                    }
                    L.val[lane] = v;
                }
                ms_sync();
            }
            if (lane == 0) {
                float cf = 1.0f, sm = 1.0f;  // ancestor_reach, nearest first
                for (uint32_t child = root, par = L.parent[root], s = 0; par != MS_NONE && s < MS_NODES; ++s) {
                    bool sampled = L.turn[par] != walker;
                    if constexpr (FR) sampled = sampled && L.kind[par] != MS_FRONTIER;
                    if (sampled) {
                        cf = cf * L.pol[par][L.slot[child]];
                        sm = sm * L.q[par][L.slot[child]];
                    }
                    child = par;
                    par = L.parent[par];
                }
                const float reach = cf / sm;
                const uint32_t na = L.nch[root], info = L.info[root];
                float v[MS_A], ev = 0.0f;
                for (uint32_t a = 0; a < na; ++a) {
                    v[a] = reach * L.val[L.kid[root][a]];
                    ev += L.pol[root][a] * v[a];
                }
                uint32_t dd = L.n_dec;  // Tree::partition: the span of this infoset, by its head
                for (uint32_t k = 0; k < L.n_dec; ++k)
                    if (L.dec_info[k] == info) dd = k;
                if (dd == L.n_dec) {
                    L.n_dec += 1;
                    L.dec_info[dd] = info;
                    L.dec_head[dd] = (uint8_t)root;
                    L.dec_pay[dd] = 0.0f;
                    for (uint32_t a = 0; a < MS_A; ++a) L.dec_delta[dd][a] = 0.0f;
                }
                L.dec_pay[dd] = L.dec_pay[dd] + ev;
                for (uint32_t a = 0; a < na; ++a) L.dec_delta[dd][a] = L.dec_delta[dd][a] + (v[a] - ev);
            }
            ms_sync();
        }
        // UPDATE: rows for the new infosets, then the four updates of every (Decisions, slot)
        if (lane == 0) {
            uint32_t r_count = n_rows;
            L.fail = 0;
            for (uint32_t k = 0; k < L.n_dec; ++k) {
                const uint32_t info = L.dec_info[k];
                uint32_t r = P.row(world, info);
                L.dec_new[k] = 0;
                if (r == MS_NO_ROW) {
                    if (r_count >= R.rows_alloc) {
                        L.fail = 1;
                        break;
                    }
                    r = r_count++;
                    P.index[(size_t)world * NK + info] = (uint16_t)r;
                    keys[r] = world * NK + info;
                    L.dec_new[k] = 1;
                }
                L.dec_row[k] = (uint16_t)r;
            }
            L.st_state[0] = r_count;
        }
        ms_sync();
        if (L.fail) {
            status = RP_MSUB_ROWS;
            break;
        }
        n_rows = L.st_state[0];
        const uint32_t n_dec = L.n_dec;
        infosets += n_dec;
        for (uint32_t pair = lane; pair < n_dec * MS_A; pair += MS_LANES) {
            const uint32_t k = pair / MS_A, a = pair % MS_A, info = L.dec_info[k], na = actions_of(info);
            if (a >= RA) continue;
            rp_encounter* cell = P.rows + (size_t)L.dec_row[k] * RA + a;
            if (a >= na) {
                if (L.dec_new[k]) *cell = rp_encounter{0.0f, 0.0f, 0.0f, 0u};
                continue;
            }
            rp_encounter e = *cell;
            float cum = e.regret;
            if (FR && L.dec_new[k] && info >= NI) {  // a Pick edge: DepthView's absent regret, then Encounter::default()
                cum = RP_EPSILON;
                e = rp_encounter{0.0f, 0.0f, 0.0f, 0u};
            } else if (L.dec_new[k]) {  // warmstart; update_regret has read cum_regret before the edge existed
                float sum = 0.0f;
                for (uint32_t b = 0; b < na; ++b) sum += rp_maxf(tab.weight[(size_t)info * A + b], RP_EPSILON);
                const float avg = rp_maxf(tab.weight[(size_t)info * A + a], RP_EPSILON) / sum;
                cum = rp_maxf(tab.regret[(size_t)info * A + a], RP_EPSILON);
                e.weight = ((avg * p.prior) * (p.prior + 1.0f)) / 2.0f;
                e.payoff = 0.0f;
                e.visits = 0u;
            }
            e.regret = rp_maxf(cum + L.dec_delta[k][a], -__builtin_inff());
            e.weight = rp_maxf(e.weight + L.pol[L.dec_head[k]][a] * (float)t, RP_EPSILON);
            e.payoff = e.payoff + (L.dec_pay[k] - e.payoff) / (float)(e.visits + 1u);
            e.visits += 1u;
            *cell = e;
        }
        ms_sync();
    }

    if (p.t_end < p.iterations) {  // more launches follow
        if (lane == 0) {
            head->status = status;
            head->n_rows = n_rows;
            head->nodes = nodes;
            head->infosets = infosets;
            head->fallbacks = fallbacks;
            for (uint32_t w = 0; w < 4; ++w) head->drawn[w] = drawn[w];
            if constexpr (FR) head->frontiers = frontiers;
        }
        return;
    }

    // RESULT = Harvest
    uint32_t hinfo = RP_NO_INFO, hna = 0;
    if (status == RP_MSUB_OK) {
        hinfo = E.harvest_info;
        if (hinfo == RP_NO_INFO) {
            const uint4 rec = g.states[entry_state];
            if ((rec.x & 255u) < 2u && ((rec.x >> 8) & 255u) > 0) hinfo = rec.y;
        }
        if (hinfo != RP_NO_INFO) {
            hna = g.info_actions[hinfo] <= MS_A ? g.info_actions[hinfo] : MS_A;
            uint32_t seen = 0;
            for (uint32_t a = 0; a < hna; ++a)
                if (E.harvest_order[a] < hna) seen |= 1u << E.harvest_order[a];
            if (seen != (hna >= 32 ? 0xffffffffu : (1u << hna) - 1u)) status = RP_MSUB_ORDER;
        }
    }
    rp_mccfr_subgame_result* out = p.results + solve;
    rp_mccfr_subgame_row* out_rows = p.rows ? p.rows + (size_t)solve * p.rows_cap : nullptr;
    {
        uint32_t* w = reinterpret_cast<uint32_t*>(out);
        for (uint32_t i = lane; i < sizeof(rp_mccfr_subgame_result) / 4; i += MS_LANES) w[i] = 0u;
        if (out_rows) {
            uint32_t* wr = reinterpret_cast<uint32_t*>(out_rows);
            const size_t words = (size_t)p.rows_cap * (sizeof(rp_mccfr_subgame_row) / 4);
            for (size_t i = lane; i < words; i += MS_LANES) wr[i] = 0u;
        }
    }
    ms_sync();
    if (status != RP_MSUB_OK) {
        if (lane == 0) {
            out->info = RP_NO_INFO;
            out->status = (uint8_t)status;
        }
        return;
    }
    const uint32_t W = E.n_worlds;
    // the rows in (world, info) order — (world, kind, info) with frontiers, a Pick infoset's key lying past the infosets': keys are distinct, a row's rank is the number of smaller keys
    for (uint32_t i = lane; i < n_rows; i += MS_LANES) {
        const uint32_t key = keys[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n_rows; ++j) rank += keys[j] < key ? 1u : 0u;
        perm[rank] = (uint16_t)i;
    }
    ms_sync();
    if (out_rows)
        for (uint32_t i = lane; i < n_rows && i < p.rows_cap; i += MS_LANES) {
            const uint32_t r = perm[i], key = keys[r], info = key % NK, na = actions_of(info);
            rp_mccfr_subgame_row* o = out_rows + i;
            o->world = (uint8_t)(key / NK);
            o->n_actions = (uint8_t)na;
            o->info = info;
            if constexpr (FR)
                if (info >= NI) {  // a Pick row: its kind and the pick id
                    o->kind = 1;
                    o->info = info - NI;
                }
            for (uint32_t a = 0; a < na && a < RA; ++a) o->enc[a] = P.rows[(size_t)r * RA + a];
        }
    if (lane < hna) {
        float refined = 0.0f;
        uint32_t visits = 0;
        for (uint32_t w = 0; w < W; ++w) {
            float pw[MS_A];
            const uint32_t r = P.row(w, hinfo);
            P.iterated(r, hinfo, hna, pw);
            float mine = 0.0f;
            for (uint32_t a = 0; a < MS_A; ++a) mine = a == lane ? pw[a] : mine;
            refined += mine / (float)W;
            visits += P.cum_visits(r, hinfo, lane);
        }
        out->refined[lane] = refined;
        out->visits[lane] = visits;
    }
    if (lane == 0) {
        float regret = 0.0f;
        for (uint32_t k = 0; k < hna; ++k)
            for (uint32_t w = 0; w < W; ++w) regret += rp_maxf(P.cum_regret(P.row(w, hinfo), hinfo, E.harvest_order[k]), 0.0f);
        float sum = 0.0f;
        for (uint32_t i = 0; i < n_rows; ++i) {
            const uint32_t r = perm[i], na = actions_of(keys[r] % NK);
            for (uint32_t a = 0; a < na && a < RA; ++a) sum += rp_maxf(P.rows[(size_t)r * RA + a].regret, 0.0f);
        }
        out->info = hinfo;
        out->n_actions = (uint8_t)hna;
        out->status = 0;
        out->regret = regret;
        out->sum_regret = sum / (float)(p.iterations > 1 ? p.iterations : 1);
        out->iterations = p.iterations;
        out->n_rows = n_rows;
        out->nodes = nodes;
        out->infosets = infosets;
        for (uint32_t w = 0; w < 4; ++w) out->drawn[w] = drawn[w];
        out->fallbacks = fallbacks;
        if constexpr (FR) out->frontiers = frontiers;
    }
}

// BELIEF: one wavefront per entry; a lane per candidate walks the path, lane 0 adds and partitions (at most 16 secrets)
__global__ __launch_bounds__(MS_LANES) void k_mccfr_subgame_belief(DevGame g, DevTables tab, uint32_t n_states, uint32_t n,
                                                                    const rp_mccfr_subgame_prior* priors, uint8_t* world_of, float* weights,
                                                                    uint8_t* status_out) {
    __shared__ rp_mccfr_subgame_prior E;
    __shared__ float mass[16];
    __shared__ uint32_t bad[16];
    const uint32_t lane = threadIdx.x, entry = blockIdx.x;
    if (entry >= n) return;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(priors + entry);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&E);
        for (uint32_t i = lane; i < sizeof(rp_mccfr_subgame_prior) / 4; i += MS_LANES) dst[i] = src[i];
    }
    ms_sync();
    uint32_t status = RP_MSUB_OK;
    if (E.internal > 1) status = RP_MSUB_SEAT;
    else if (E.mode > 1) status = RP_MSUB_MODE;
    else if (E.n_worlds < 1 || E.n_worlds > 4) status = RP_MSUB_WORLDS;
    else if (E.n_prior > 16 || E.n_path > 16) status = RP_MSUB_COUNT;
    if (status == RP_MSUB_OK && lane < 16) {
        uint32_t st = RP_MSUB_OK;
        float m = 1.0f;
        if (lane < E.n_prior) {
            if (E.secret[lane] >= 16) st = RP_MSUB_SECRET;
            else if (E.root_state[lane] >= n_states) st = RP_MSUB_STATE;
            uint32_t s = st == RP_MSUB_OK ? E.root_state[lane] : 0u;
            for (uint32_t k = 0; k < E.n_path && st == RP_MSUB_OK; ++k) {
                const uint4 rec = g.states[s];
                const uint32_t turn = rec.x & 255u, nch = (rec.x >> 8) & 255u, slot = E.path[k];
                if (slot >= nch) {
                    st = RP_MSUB_PATH;
                    break;
                }
                if (E.mode == 1 && turn == 1u - E.internal) {  // averaged_policy(info, edge) of the seat that is not `internal`
                    const uint32_t na = g.info_actions[rec.y];
                    float sum = 0.0f;
                    for (uint32_t a = 0; a < na && a < MS_A; ++a) sum += rp_maxf(tab.weight[(size_t)rec.y * g.A + a], RP_EPSILON);
                    m = m * (rp_maxf(tab.weight[(size_t)rec.y * g.A + slot], RP_EPSILON) / sum);
                }
                s = g.children[rec.z + slot];
            }
        }
        mass[lane] = m;
        bad[lane] = st;
    }
    ms_sync();
    if (lane != 0) return;
    for (uint32_t c = 0; status == RP_MSUB_OK && c < E.n_prior; ++c) status = bad[c];
    uint8_t* wo = world_of + (size_t)entry * 16;
    float* wt = weights + (size_t)entry * 4;
    for (uint32_t s = 0; s < 16; ++s) wo[s] = (uint8_t)RP_WORLD_NONE;
    for (uint32_t w = 0; w < 4; ++w) wt[w] = 0.0f;
    if (status_out) status_out[entry] = (uint8_t)status;
    if (status != RP_MSUB_OK) return;
    const uint32_t W = E.n_worlds;
    float post[16];
    uint32_t seen = 0;
    for (uint32_t s = 0; s < 16; ++s) post[s] = 0.0f;
    for (uint32_t c = 0; c < E.n_prior; ++c) {  // Posterior::add, in candidate order
        float add = mass[c];
        for (uint32_t s = 0; s < 16; ++s)
            if (s == E.secret[c]) post[s] = post[s] + add;
        seen |= 1u << E.secret[c];
    }
    float total = 0.0f;
    for (uint32_t s = 0; s < 16; ++s)
        if (seen >> s & 1u) total += post[s];
    if (!(total > 0.0f)) {
        for (uint32_t s = 0; s < 16; ++s)
            if (seen >> s & 1u) wo[s] = 0;
        for (uint32_t w = 0; w < W; ++w) wt[w] = 1.0f / (float)W;
        return;
    }
    uint8_t order[16];
    uint32_t m = 0;
    for (uint32_t s = 0; s < 16; ++s) {  // stable insertion, descending mass: an entry passes only strictly smaller ones
        if (!(seen >> s & 1u)) continue;
        uint32_t at = m++;
        for (; at > 0 && post[order[at - 1]] < post[s]; --at) order[at] = order[at - 1];
        order[at] = (uint8_t)s;
    }
    const float segment = total / (float)W;
    float bucket = 0.0f, accumulated = 0.0f;
    uint32_t index = 0;
    for (uint32_t i = 0; i < m; ++i) {
        const uint32_t s = order[i];
        bucket += post[s];
        accumulated += post[s];
        wo[s] = (uint8_t)index;
        if (accumulated >= segment * (float)(index + 1) && index < W - 1) {
            wt[index] = bucket / total;
            index += 1;
            bucket = 0.0f;
        }
    }
    wt[index] = bucket / total;
}

}  // namespace rp

#endif
