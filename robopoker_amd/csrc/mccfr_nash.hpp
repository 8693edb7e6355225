// mccfr_nash.hpp — CfrNash::exploitability (crates/mccfr/src/strategy/nash.rs:31-38,103-194) on the device: the full-tree best
// response against the average profile, bit for bit what rp_mccfr_exploitability computes on the host (mccfr.hip) and
// ora_mccfr_exploitability in the oracle.  f32 order is part of the contract; everything is compiled -ffp-contract=off.
//
// Static per-game data (NashTree), built on the host by the first call that asks and kept: the VanillaSampling expansion from
// exploit_root in TreeBuilder's pop-last order (the node numbering of rp_mccfr_exploitability's own loop), one record per node, the
// nodes listed by depth level, and per infoset its span (its nodes in ascending node index).
//
// Phases of one call (the per-hero ones for every hero 0..n_players-1, independent of each other):
//   avg     avg[info][a] = max(w, EPS) / sum_k max(w_k, EPS), the sum from +0.0f over ascending k (RefProf::averaged_distribution)
//   a       v[node] under the average profile, bottom-up by level: terminal payoffs[row * n_players + hero]; chance
//           (sum_k v[kid_k]) / (float)n; player nodes (the hero's too) sum_k avg * v, both sums from 0.0f in k order
//   b1      every child c of a hero node: v[c] <- external_reach(c) * v[c], in place.  The reach starts at 1.0f and is multiplied
//           LEAF TO ROOT by avg[parent.info][edge] at every non-chance, non-hero parent on the walk from c up: the reference's
//           association (a top-down prefix product rounds differently), so it is walked per node, at most n_levels steps
//   b2      cfv[info][a] = sum over the span of v[kid_a], from 0.0f in ascending node index: one lane per cell, serial over the span
//   c       choice[info] = argmax_a cfv[info][a], the LAST maximum (max_by: a >= scan; a NaN cell never replaces the incumbent)
//   d       v[node] again bottom-up, hero nodes taking v[kid[choice[info]]]; value[hero] = v[root]
//   final   exploitability = (sum_hero value[hero], from 0.0f in hero order) / (float)n_players
//
// Two launch shapes, same bits (rp_mccfr_nash_variant):
//   0 "one"     k_nash_one: one launch, one workgroup of NASH_ONE_THREADS per hero, the levels separated by __syncthreads();
//               avg, v, cfv and choice in LDS.  Chosen when 4 * (n_nodes + 2 * n_infos * max_actions + n_infos) bytes are at most
//               NASH_ONE_LDS_BYTES (Leduc: 3 517 nodes, 120 x 2 cells: 16 KB).
//   1 "levels"  plain launches over a grid, one per level and phase (both heroes in one launch: grid.y), the arrays in device
//               scratch (L2-resident at these sizes).
// RP_NASH_VARIANT=one|levels, read when the static data is built, forces a shape (tests); "one" forced on a game past the LDS limit
// keeps the launch shape and puts the arrays in device scratch (k_nash_one<false>).
// k_nash_final is a last one-thread launch in both.  No workgroup ever waits for another one; every loop is bounded by a count of
// the static data.
//
// Limits: node ids are 32-bit and the host builds the tree in memory: a tree of more than NASH_MAX_NODES nodes is refused with
// RP_ERR_CAPACITY, as is one whose arrays the device cannot hold (28 bytes per node + 4 per node and player).
#ifndef RP_MCCFR_NASH_HPP
#define RP_MCCFR_NASH_HPP

#include "mccfr_kernels.hpp"

namespace rp {

constexpr uint32_t NASH_MAX_NODES = 1u << 24;
// dynamic LDS of k_nash_one<true>: what a launch may ask for without opting in to more (every kernel of this library stays within it)
constexpr size_t NASH_ONE_LDS_BYTES = 64 * 1024;
constexpr uint32_t NASH_ONE_THREADS = 1024;
constexpr uint32_t NASH_THREADS = 256;
constexpr uint32_t NASH_ROOT = 0xFFFFFFFFu;  // NashTree::rec[0].z: the root has no parent

struct NashTree {
    const uint4* rec;             // [n_nodes] x = turn | n_children << 8 | incoming edge << 16, y = infoset (player node) or payoff row
                                  // (terminal), z = parent (NASH_ROOT: none), w = first of its slots in kids[]
    const uint32_t* kids;         // kid k of node n = kids[rec[n].w + k]
    const uint32_t* level_nodes;  // [n_nodes] by depth, then by node index
    const uint32_t* level_off;    // [n_levels + 1]
    const uint32_t* span_nodes;   // the player nodes by infoset, then by node index
    const uint32_t* span_off;     // [n_infos + 1]
    uint32_t n_nodes, n_levels;
};

// what a call writes: device scratch of the handle
struct NashWork {
    float* avg;       // [n_infos][A]; k_nash_one<false>: a copy per hero
    float* cfv;       // [n_infos][A]; slots past an infoset's actions stay 0
    uint8_t* choice;  // [n_infos]
    float* values;    // [n_players]
    float* expl;      // [1]
    float* v;         // [n_players][n_nodes]; NULL when k_nash_one keeps it in LDS
};

__device__ __forceinline__ void nash_avg_row(const float* weight, uint32_t A, uint32_t na, uint32_t info, float* avg) {
    const float* w = weight + (size_t)info * A;
    float sum = 0.0f;
    for (uint32_t k = 0; k < na; ++k) sum += rp_maxf(w[k], RP_EPSILON);
    for (uint32_t k = 0; k < na; ++k) avg[(size_t)info * A + k] = rp_maxf(w[k], RP_EPSILON) / sum;
}

// phases a and d (BR): XCtx::value of mccfr.hip with the kids' values already in v
template <bool BR, class Choice>
__device__ __forceinline__ float nash_node_value(const NashTree& T, const DevGame& g, uint32_t n, uint32_t hero, const float* v, const float* avg,
                                                 const Choice* choice) {
    const uint4 r = T.rec[n];
    const uint32_t turn = r.x & 255u, nch = (r.x >> 8) & 255u;
    if (nch == 0) return g.payoffs[(size_t)r.y * g.n_players + hero];
    const uint32_t* kid = T.kids + r.w;
    if (turn == RP_TURN_CHANCE) {
        float s = 0.0f;
        for (uint32_t k = 0; k < nch; ++k) s += v[kid[k]];
        return s / (float)nch;
    }
    if (BR && turn == hero) return v[kid[choice[r.y]]];
    float s = 0.0f;
    for (uint32_t k = 0; k < nch; ++k) s += avg[(size_t)r.y * g.A + k] * v[kid[k]];
    return s;
}

// phase b1: XCtx::reach times the value, for a child of a hero node; any other node is left alone
__device__ __forceinline__ void nash_term(const NashTree& T, const DevGame& g, uint32_t c, uint32_t hero, float* v, const float* avg) {
    uint4 r = T.rec[c];
    if (r.z == NASH_ROOT || (T.rec[r.z].x & 255u) != hero) return;
    float p = 1.0f;
    for (uint32_t s = 0; s < T.n_levels && r.z != NASH_ROOT; ++s) {
        const uint4 pr = T.rec[r.z];
        const uint32_t turn = pr.x & 255u;
        if (turn != RP_TURN_CHANCE && turn != hero) p = p * avg[(size_t)pr.y * g.A + ((r.x >> 16) & 255u)];
        r = pr;
    }
    v[c] = p * v[c];
}

// phase b2, one cell of an infoset with actions: the sum over the span
__device__ __forceinline__ float nash_cell(const NashTree& T, uint32_t info, uint32_t a, const float* v) {
    float s = 0.0f;
    for (uint32_t i = T.span_off[info]; i < T.span_off[info + 1]; ++i) s += v[T.kids[T.rec[T.span_nodes[i]].w + a]];
    return s;
}

// phase c
__device__ __forceinline__ uint32_t nash_choice(const float* cfv_row, uint32_t na) {
    float best = cfv_row[0];
    uint32_t c = 0;
    for (uint32_t a = 1; a < na; ++a)
        if (cfv_row[a] >= best) {  // max_by keeps the last maximum (nash.rs:184-193)
            best = cfv_row[a];
            c = a;
        }
    return c;
}

// ---- variant 1: a launch per level and phase; blockIdx.y = hero where the phase is per hero ---------------------------------------
__global__ __launch_bounds__(NASH_THREADS) void k_nash_avg(DevGame g, DevTables t, NashWork w) {
    const uint32_t info = blockIdx.x * NASH_THREADS + threadIdx.x;
    if (info < g.n_infos) nash_avg_row(t.weight, g.A, g.info_actions[info], info, w.avg);
}

template <bool BR>
__global__ __launch_bounds__(NASH_THREADS) void k_nash_level(NashTree T, DevGame g, NashWork w, uint32_t level) {
    const uint32_t i = T.level_off[level] + blockIdx.x * NASH_THREADS + threadIdx.x, hero = blockIdx.y;
    if (i >= T.level_off[level + 1]) return;
    float* v = w.v + (size_t)hero * T.n_nodes;
    const uint32_t n = T.level_nodes[i];
    v[n] = nash_node_value<BR>(T, g, n, hero, v, w.avg, w.choice);
}

__global__ __launch_bounds__(NASH_THREADS) void k_nash_term(NashTree T, DevGame g, NashWork w) {
    const uint32_t c = blockIdx.x * NASH_THREADS + threadIdx.x, hero = blockIdx.y;
    if (c < T.n_nodes) nash_term(T, g, c, hero, w.v + (size_t)hero * T.n_nodes, w.avg);
}

// an infoset belongs to one player: the cells and the choices of all heroes in one launch
__global__ __launch_bounds__(NASH_THREADS) void k_nash_cfv(NashTree T, DevGame g, NashWork w) {
    const uint32_t cell = blockIdx.x * NASH_THREADS + threadIdx.x;
    if (cell >= g.n_infos * g.A) return;
    const uint32_t info = cell / g.A, a = cell % g.A, hero = g.info_player[info];
    if (hero < g.n_players && a < g.info_actions[info]) w.cfv[cell] = nash_cell(T, info, a, w.v + (size_t)hero * T.n_nodes);
}

__global__ __launch_bounds__(NASH_THREADS) void k_nash_choice(DevGame g, NashWork w) {
    const uint32_t info = blockIdx.x * NASH_THREADS + threadIdx.x;
    if (info < g.n_infos && g.info_player[info] < g.n_players)
        w.choice[info] = (uint8_t)nash_choice(w.cfv + (size_t)info * g.A, g.info_actions[info]);
}

// value[hero] = root_v[hero * stride]; the exploitability to `out` (the caller's) and to w.expl
__global__ void k_nash_final(DevGame g, NashWork w, const float* root_v, size_t stride, float* out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float total = 0.0f;
    for (uint32_t hero = 0; hero < g.n_players; ++hero) {
        const float x = root_v[(size_t)hero * stride];
        w.values[hero] = x;
        total += x;
    }
    total = total / (float)g.n_players;
    *w.expl = total;
    if (out) *out = total;
}

// ---- variant 0: one workgroup per hero runs every phase; IN_LDS: the arrays in LDS, else in the handle's scratch --------------------
template <bool IN_LDS>
__global__ __launch_bounds__(NASH_ONE_THREADS) void k_nash_one(NashTree T, DevGame g, DevTables t, NashWork w) {
    extern __shared__ __attribute__((aligned(16))) float nash_lds[];
    const uint32_t hero = blockIdx.x, tid = threadIdx.x, cells = g.n_infos * g.A;
    // LDS: v[n_nodes], avg[cells], cfv[cells], choice[n_infos] (a word each).  Scratch: avg is written by every hero's workgroup with
    // the same values, so each keeps a copy of its own; cfv and choice are per infoset, hence per hero, and shared
    float* v = IN_LDS ? nash_lds : w.v + (size_t)hero * T.n_nodes;
    float* avg = IN_LDS ? nash_lds + T.n_nodes : w.avg + (size_t)hero * cells;
    float* cfv = IN_LDS ? nash_lds + T.n_nodes + cells : w.cfv;
    uint32_t* choice_l = reinterpret_cast<uint32_t*>(nash_lds + T.n_nodes + 2 * (size_t)cells);
    for (uint32_t info = tid; info < g.n_infos; info += NASH_ONE_THREADS) nash_avg_row(t.weight, g.A, g.info_actions[info], info, avg);
    __syncthreads();
    for (uint32_t level = T.n_levels; level-- > 0;) {
        for (uint32_t i = T.level_off[level] + tid; i < T.level_off[level + 1]; i += NASH_ONE_THREADS) {
            const uint32_t n = T.level_nodes[i];
            v[n] = nash_node_value<false>(T, g, n, hero, v, avg, (const uint32_t*)nullptr);
        }
        __syncthreads();
    }
    for (uint32_t c = tid; c < T.n_nodes; c += NASH_ONE_THREADS) nash_term(T, g, c, hero, v, avg);
    __syncthreads();
    for (uint32_t cell = tid; cell < cells; cell += NASH_ONE_THREADS) {
        const uint32_t info = cell / g.A, a = cell % g.A;
        if (g.info_player[info] != hero || a >= g.info_actions[info]) continue;
        const float s = nash_cell(T, info, a, v);
        cfv[cell] = s;
        if (IN_LDS) w.cfv[cell] = s;
    }
    __syncthreads();
    for (uint32_t info = tid; info < g.n_infos; info += NASH_ONE_THREADS) {
        if (g.info_player[info] != hero) continue;
        const uint32_t c = nash_choice(cfv + (size_t)info * g.A, g.info_actions[info]);
        if (IN_LDS) choice_l[info] = c;
        w.choice[info] = (uint8_t)c;
    }
    __syncthreads();
    for (uint32_t level = T.n_levels; level-- > 0;) {
        for (uint32_t i = T.level_off[level] + tid; i < T.level_off[level + 1]; i += NASH_ONE_THREADS) {
            const uint32_t n = T.level_nodes[i];
            v[n] = IN_LDS ? nash_node_value<true>(T, g, n, hero, v, avg, choice_l) : nash_node_value<true>(T, g, n, hero, v, avg, w.choice);
        }
        __syncthreads();
    }
    if (tid == 0) w.values[hero] = v[0];
}

}  // namespace rp

#endif
