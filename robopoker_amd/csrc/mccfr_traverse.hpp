// mccfr_traverse.hpp — the generic traversal kernels of mccfr.hip (Solver::batch, crates/mccfr/src/solver/solver.rs:225-250): profile
// reads and sampling, the metric counters, k_traverse (per-tree scratch in HBM), the per-infoset tables of an epoch (DevInfoTab,
// k_prepare_infos / k_prepare_ref) and k_traverse_lds (scratch in LDS).  The skeleton kernels are in traverse_static.hpp.
#ifndef RP_MCCFR_TRAVERSE_HPP
#define RP_MCCFR_TRAVERSE_HPP

#include "mccfr_kernels.hpp"

namespace rp {

// ------------------------------------------------------------------------------------------------
// device: profile reads (RefProf::{regret,weight} profile.rs:31-37; CfrFlow flow.rs:20-59)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float d_regret(const DevTables& t, uint32_t A, uint32_t info, uint32_t a) {
    return rp_maxf(t.regret[info * A + a], RP_EPSILON);
}
__device__ __forceinline__ float d_weight(const DevTables& t, uint32_t A, uint32_t info, uint32_t a) {
    return rp_maxf(t.weight[info * A + a], RP_EPSILON);
}
__device__ __forceinline__ float d_regret_denom(const DevTables& t, uint32_t A, uint32_t info, uint32_t n) {
    float s = 0.0f;
    for (uint32_t a = 0; a < n; ++a) s += d_regret(t, A, info, a);
    return s;
}
__device__ __forceinline__ float d_weight_denom(const DevTables& t, uint32_t A, uint32_t info, uint32_t n,
                                                float smoothing) {
    float s = 0.0f;
    for (uint32_t a = 0; a < n; ++a) s += d_weight(t, A, info, a);
    return s + smoothing;
}
__device__ __forceinline__ float d_sampling_weight(const DevTables& t, uint32_t A, uint32_t info, uint32_t a,
                                                   float denom, const StepParams& p) {
    return rp_maxf((d_weight(t, A, info, a) / p.temperature + p.smoothing) / denom, p.curiosity);
}
__device__ __forceinline__ float d_sampling_z(const DevTables& t, uint32_t A, uint32_t info, uint32_t n,
                                              float denom, const StepParams& p) {
    float z = 0.0f;
    for (uint32_t a = 0; a < n; ++a) z += d_sampling_weight(t, A, info, a, denom, p);
    return z;
}

// SamplingScheme::sample as a bitmask over child slots (sample/{mod,external,pruning,pluribus}.rs)
__device__ uint32_t d_sample_mask(const DevGame& g, const DevTables& t, const StepParams& p, uint64_t tree_id,
                                  uint32_t state, uint32_t turn, uint32_t n, uint32_t info, uint32_t off) {
    const uint32_t all = (1u << n) - 1u;
    const bool ref = p.ref_info != nullptr;
    if (n == 0) return 0;
    if (turn == RP_TURN_CHANCE) return 1u << d_draw_chance(p, ref, tree_id, state, n, info);  // a chance record carries chance_info in y
    if (turn != p.walker) {
        // weighted (external.rs:41-64): WeightedIndex over sampling_distribution().max(EPSILON)
        const float denom = d_weight_denom(t, g.A, info, n, p.smoothing);
        const float z = d_sampling_z(t, g.A, info, n, denom, p);
        float total = 0.0f;
        for (uint32_t a = 0; a < n; ++a)
            total += rp_maxf(d_sampling_weight(t, g.A, info, a, denom, p) / z, RP_EPSILON);
        const float x = d_draw_weight(p, ref, tree_id, info, total);
        float cum = 0.0f;
        uint32_t idx = 0;
        bool open = true;
        for (uint32_t a = 0; a + 1 < n; ++a) {
            cum += rp_maxf(d_sampling_weight(t, g.A, info, a, denom, p) / z, RP_EPSILON);
            open = open && (cum <= x);
            if (open) idx = a + 1;
        }
        return 1u << idx;
    }
    if (p.S == RP_SAMPLING_EXTERNAL) return all;
    if (p.S == RP_SAMPLING_PLURIBUS) {
        if (p.epoch < p.prune_warmup) return all;
        if (d_draw_coin(p, ref, tree_id, info) < p.prune_explore) return all;
    }
    uint32_t mask = 0;
    for (uint32_t a = 0; a < n; ++a) {
        bool keep = t.regret[info * g.A + a] > p.prune_threshold;
        if (p.S == RP_SAMPLING_PLURIBUS) {
            const uint4 c = g.states[g.children[off + a]];
            keep = keep || ((c.x & 0xffu) == RP_TURN_TERMINAL);
        }
        if (keep) mask |= 1u << a;
    }
    return mask ? mask : all;
}

__device__ __forceinline__ uint32_t lane_of() { return threadIdx.x & 63u; }

// Metrics (metrics/mod.rs:21-80; solver.rs:273): nodes / infos, one atomic per WAVE — a million lanes adding to the
// same two addresses would serialise in the L2 atomic unit
// The counters are STRIPED: 16 384 waves adding to ONE address serialise at its L2 channel (~9 ns per atomic: 0.29 ms
// of a 0.52 ms launch was spent there, found by ablation); stripe s owns its own 128-byte line, the host sums them.
#define METRIC_STRIPES 256u
#define METRIC_STRIDE 16u  // u64 per stripe (128 B)
__device__ __forceinline__ void count_metrics(const StepParams& p, uint32_t nn, uint32_t ndec, uint32_t err) {
    unsigned long long* c = p.counters + (size_t)(blockIdx.x % METRIC_STRIPES) * METRIC_STRIDE;
    if (__ballot(1) == ~0ull) {
        uint32_t a = nn, b = ndec;
        for (int d = 32; d > 0; d >>= 1) {
            a += __shfl_xor(a, d, 64);
            b += __shfl_xor(b, d, 64);
        }
        if (lane_of() == 0) {
            atomicAdd(&c[0], (unsigned long long)a);
            atomicAdd(&c[1], (unsigned long long)b);
        }
    } else {  // the ragged last wave
        atomicAdd(&c[0], (unsigned long long)nn);
        atomicAdd(&c[1], (unsigned long long)ndec);
    }
    if (err) atomicOr(&c[2], (unsigned long long)err);
}

#define META_PARENT(m) ((m)&0xffu)
#define META_EDGE(m) (((m) >> 8) & 0xffu)
#define META_PTYPE(m) (((m) >> 16) & 3u)
#define META_LEAF(m) (((m) >> 18) & 1u)
#define META_WALKER(m) (((m) >> 19) & 1u)
#define META_NACT(m) (((m) >> 24) & 0xffu)
#define NO_PARENT 0xffu

// ------------------------------------------------------------------------------------------------
// k_traverse: Solver::batch for one shard of trees
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_traverse(DevGame g, DevTables t, DevScratch sc, DevDecisions dc,
                                                  StepParams p) {
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= p.batch) return;
    const uint64_t tree_id = p.tree_base + lane;
    const size_t S = sc.stride;
    uint32_t err = 0;

    // ---- TreeBuilder::build (builder.rs:74-87,141-161): pop-last DFS -----------------------------
    uint32_t nn = 0, sp = 0;
    uint32_t cur_state = g.root;
    uint32_t cur_meta_in = NO_PARENT | (PT_NONE << 16);
    float cur_frel = 1.0f, cur_fsmp = 1.0f;
    for (;;) {
        const uint4 st = g.states[cur_state];
        const uint32_t turn = st.x & 0xffu, nch = (st.x >> 8) & 0xffu, info = st.y, off = st.z;
        const uint32_t me = nn;
        if (nn >= sc.maxn) {
            err |= ERR_NODE_CAPACITY;
            break;
        }
        const bool is_walker = turn == p.walker;
        uint32_t meta = cur_meta_in | ((nch == 0 ? 1u : 0u) << 18) | ((is_walker ? 1u : 0u) << 19) | (nch << 24);
        sc.n_meta[me * S + lane] = meta;
        sc.n_info[me * S + lane] = info;
        sc.n_frel[me * S + lane] = cur_frel;
        sc.n_fsmp[me * S + lane] = cur_fsmp;
        if (nch == 0) sc.n_pay[me * S + lane] = g.payoffs[off * g.n_players + p.walker];
        nn += 1;
        if (nch > 0) {
            const uint32_t mask = d_sample_mask(g, t, p, tree_id, cur_state, turn, nch, info, off);
            const bool chance = turn == RP_TURN_CHANCE;
            const uint32_t ptype = chance ? PT_CHANCE : (is_walker ? PT_WALKER : PT_OPP);
            float rd = 0.0f, denom = 0.0f, z = 0.0f;
            if (!chance) rd = d_regret_denom(t, g.A, info, nch);
            if (ptype == PT_OPP) {
                denom = d_weight_denom(t, g.A, info, nch, p.smoothing);
                z = d_sampling_z(t, g.A, info, nch, denom, p);
            }
            for (uint32_t k = 0; k < nch; ++k) {
                if (!((mask >> k) & 1u)) continue;
                if (sp >= sc.maxs) {
                    err |= ERR_STACK_CAPACITY;
                    break;
                }
                // reach factors of the edge parent->child (flow.rs:195-212)
                const float frel = chance ? 1.0f : d_regret(t, g.A, info, k) / rd;
                const float fsmp = ptype == PT_OPP ? d_sampling_weight(t, g.A, info, k, denom, p) / z : 1.0f;
                sc.s_state[sp * S + lane] = g.children[off + k];
                sc.s_meta[sp * S + lane] = me | (k << 8) | (ptype << 16);
                sc.s_frel[sp * S + lane] = frel;
                sc.s_fsmp[sp * S + lane] = fsmp;
                sp += 1;
            }
        }
        if (sp == 0 || err) break;
        sp -= 1;
        cur_state = sc.s_state[sp * S + lane];
        cur_meta_in = sc.s_meta[sp * S + lane];
        cur_frel = sc.s_frel[sp * S + lane];
        cur_fsmp = sc.s_fsmp[sp * S + lane];
    }

    // ---- Tree::partition + CfrFlow::dfs per walker infoset (tree.rs:88-98, flow.rs:64-87) --------
    uint32_t ndec = 0;
    if (!err) {
        for (uint32_t i = 0; i < nn; ++i) {
            const uint32_t mi = sc.n_meta[i * S + lane];
            if (!META_WALKER(mi) || META_LEAF(mi)) continue;
            const uint32_t info = sc.n_info[i * S + lane];
            bool head = true;
            for (uint32_t j = 0; j < i; ++j) {
                const uint32_t mj = sc.n_meta[j * S + lane];
                if (META_WALKER(mj) && !META_LEAF(mj) && sc.n_info[j * S + lane] == info) head = false;
            }
            if (!head) continue;
            if (ndec >= dc.maxdec) {
                err |= ERR_DEC_CAPACITY;
                break;
            }
            const uint32_t nact = META_NACT(mi);
            const uint32_t slot = ndec++;
            const size_t D = dc.stride;
            const float rd = d_regret_denom(t, g.A, info, nact);
            for (uint32_t a = 0; a < nact; ++a) {  // policy_vector = iterated_distribution (profile.rs:47-51)
                dc.policy[(slot * g.A + a) * D + lane] = d_regret(t, g.A, info, a) / rd;
                dc.regret[(slot * g.A + a) * D + lane] = 0.0f;
            }
            float payoff = 0.0f;
            uint32_t expanded = 0;
            for (uint32_t j = i; j < nn; ++j) {  // span in ascending node index
                const uint32_t mj = sc.n_meta[j * S + lane];
                if (!META_WALKER(mj) || META_LEAF(mj) || sc.n_info[j * S + lane] != info) continue;
                // top-down: reach products below root j, starting at 1 on j's children (flow.rs:72)
                uint32_t end = j;
                for (uint32_t n = j + 1; n < nn; ++n) {
                    const uint32_t mn = sc.n_meta[n * S + lane];
                    const uint32_t par = META_PARENT(mn);
                    if (par < j) break;
                    float rel = 1.0f, smp = 1.0f;
                    if (par != j) {
                        rel = sc.n_rel[par * S + lane] * sc.n_frel[n * S + lane];
                        smp = sc.n_smp[par * S + lane] * sc.n_fsmp[n * S + lane];
                    }
                    sc.n_rel[n * S + lane] = rel;
                    sc.n_smp[n * S + lane] = smp;
                    sc.n_acc[n * S + lane] = 0.0f;
                    end = n;
                }
                // bottom-up: children were created in reverse choices() order, so descending node index
                // adds them to the parent's sum in choices() order, as node.edges() does (node.rs:103-107)
                uint32_t kids = 0;
                for (uint32_t n = end; n > j; --n) {
                    const uint32_t mn = sc.n_meta[n * S + lane];
                    const float v = META_LEAF(mn)
                                        ? sc.n_rel[n * S + lane] / sc.n_smp[n * S + lane] * sc.n_pay[n * S + lane]
                                        : sc.n_acc[n * S + lane];
                    const uint32_t par = META_PARENT(mn);
                    if (par == j) {
                        sc.t_v[META_EDGE(mn) * S + lane] = v;
                        kids |= 1u << META_EDGE(mn);
                    } else {
                        sc.n_acc[par * S + lane] = sc.n_acc[par * S + lane] + v;
                    }
                }
                // ancestor_reach (flow.rs:166-174): upward over opponent decision ancestors
                float cf = 1.0f, sm = 1.0f;
                for (uint32_t n = j;;) {
                    const uint32_t mn = sc.n_meta[n * S + lane];
                    const uint32_t par = META_PARENT(mn);
                    if (par == NO_PARENT) break;
                    if (META_PTYPE(mn) == PT_OPP) {
                        cf = cf * sc.n_frel[n * S + lane];
                        sm = sm * sc.n_fsmp[n * S + lane];
                    }
                    n = par;
                }
                const float reach = cf / sm;
                float ev = 0.0f;
                for (uint32_t a = 0; a < nact; ++a) {
                    if (!((kids >> a) & 1u)) continue;
                    const float v = reach * sc.t_v[a * S + lane];
                    sc.t_v[a * S + lane] = v;
                }
                for (uint32_t a = 0; a < nact; ++a) {
                    if (!((kids >> a) & 1u)) continue;
                    ev += d_regret(t, g.A, info, a) / rd * sc.t_v[a * S + lane];
                }
                payoff += ev;
                for (uint32_t a = 0; a < nact; ++a) {
                    if (!((kids >> a) & 1u)) continue;
                    const size_t k = (slot * g.A + a) * D + lane;
                    dc.regret[k] = dc.regret[k] + (sc.t_v[a * S + lane] - ev);
                }
                expanded |= kids;
            }
            dc.info[slot * D + lane] = info;
            dc.mask[slot * D + lane] = expanded;
            dc.payoff[slot * D + lane] = payoff;
            if (dc.slotmap) dc.slotmap[(size_t)info * D + lane] = (uint8_t)(slot + 1);
        }
    }
    dc.ndec[lane] = (uint8_t)ndec;
    // Metrics: nodes / infos (metrics/mod.rs:21-80; solver.rs:273)
    count_metrics(p, nn, ndec, err);
}

// ------------------------------------------------------------------------------------------------
// k_prepare_infos: everything a node needs from its infoset, computed ONCE per epoch per infoset instead of at
// every visited node: regret-matching policy sigma(a) = regret(a)/sum (profile.rs:47-51), the normalised sampling
// distribution q(a) (flow.rs:33-42), the cumulative weights WeightedIndex draws from (external.rs:52-62) and the
// regret-based pruning mask (pruning.rs:57-63).  Same expressions, same order => same bits as the per-node code.
// ------------------------------------------------------------------------------------------------
struct DevInfoTab {
    float* sigma;    // [n_infos][A]
    float* q;        // [n_infos][A]
    float* cum;      // [n_infos][A] inclusive cumulative of max(q, EPSILON)
    float* total;    // [n_infos]
    uint32_t* keep;  // [n_infos] edges with cum_regret > prune_threshold
    float2* sq;      // [n_infos][A] (sigma, q) side by side: one load per edge in the traversal's sweeps
    float* row2;     // [n_infos][8] two-action games (NULL otherwise): {sigma0, sigma1, q0, q1, total, cum0, keep, 0} — all a node of
                     // the skeleton traversal needs of its infoset, in one 32-byte row (traverse_static.hpp)
};

__device__ __forceinline__ void prepare_one(const DevGame& g, const DevTables& t, const StepParams& p, const DevInfoTab& it,
                                            uint32_t info) {
    const uint32_t A = g.A, n = g.info_actions[info];
    const float rd = d_regret_denom(t, A, info, n);
    const float denom = d_weight_denom(t, A, info, n, p.smoothing);
    const float z = d_sampling_z(t, A, info, n, denom, p);
    float total = 0.0f;
    uint32_t keep = 0;
    for (uint32_t a = 0; a < n; ++a) {
        it.sigma[info * A + a] = d_regret(t, A, info, a) / rd;
        const float qa = d_sampling_weight(t, A, info, a, denom, p) / z;
        it.q[info * A + a] = qa;
        it.sq[info * A + a] = make_float2(it.sigma[info * A + a], qa);
        if (it.row2) {
            it.row2[info * 8u + a] = it.sigma[info * A + a];
            it.row2[info * 8u + 2u + a] = qa;
        }
        total += rp_maxf(qa, RP_EPSILON);
        it.cum[info * A + a] = total;
        if (t.regret[info * A + a] > p.prune_threshold) keep |= 1u << a;
    }
    it.total[info] = total;
    it.keep[info] = keep;
    if (it.row2) {
        it.row2[info * 8u + 4u] = total;
        it.row2[info * 8u + 5u] = it.cum[info * A];
        it.row2[info * 8u + 6u] = rp_u2f(keep);
        it.row2[info * 8u + 7u] = 0.0f;
    }
}
__global__ void k_prepare_infos(DevGame g, DevTables t, StepParams p, DevInfoTab it) {
    const uint32_t info = blockIdx.x * blockDim.x + threadIdx.x;
    if (info >= g.n_infos) return;
    prepare_one(g, t, p, it, info);
}

// reference-seed mode: DefaultHasher after t.hash() and info.hash() for every infoset and every in-tree chance info
// (flow.rs:290-293); a node continues with node.seed().hash() and finish() (rp_ref_seed_finish).  Depends on the epoch: every step.
__global__ void k_prepare_ref(const rp_hash_stream* infos, uint32_t n_infos, const rp_hash_stream* chance, uint32_t n_chance,
                              uint64_t epoch, rp_sip_mid* info_mid, rp_sip_mid* chance_mid) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_infos) rp_ref_seed_prefix(&info_mid[i], epoch, infos[i].bytes, infos[i].len);
    else if (i < n_infos + n_chance) rp_ref_seed_prefix(&chance_mid[i - n_infos], epoch, chance[i - n_infos].bytes, chance[i - n_infos].len);
}

// SamplingScheme::sample with the per-infoset tables
__device__ __forceinline__ uint32_t d_sample_mask_tab(const DevGame& g, const DevInfoTab& it, const StepParams& p,
                                                      uint64_t tree_id, uint32_t state, uint32_t turn, uint32_t n,
                                                      uint32_t info, uint32_t off) {
    const uint32_t all = (1u << n) - 1u;
    const bool ref = p.ref_info != nullptr;
    if (turn == RP_TURN_CHANCE) return 1u << d_draw_chance(p, ref, tree_id, state, n, info);  // a chance record carries chance_info in y
    if (turn != p.walker) {
        const float x = d_draw_weight(p, ref, tree_id, info, it.total[info]);
        uint32_t idx = 0;
        bool open = true;
        for (uint32_t a = 0; a + 1 < n; ++a) {
            open = open && (it.cum[info * g.A + a] <= x);
            if (open) idx = a + 1;
        }
        return 1u << idx;
    }
    if (p.S == RP_SAMPLING_EXTERNAL) return all;
    if (p.S == RP_SAMPLING_PLURIBUS) {
        if (p.epoch < p.prune_warmup) return all;
        if (d_draw_coin(p, ref, tree_id, info) < p.prune_explore) return all;
    }
    uint32_t mask = it.keep[info] & all;
    if (p.S == RP_SAMPLING_PLURIBUS) {
        for (uint32_t a = 0; a < n; ++a) {
            if ((g.kids[off + a].x & 0xffu) == RP_TURN_TERMINAL) mask |= 1u << a;
        }
    }
    return mask ? mask : all;
}

// ------------------------------------------------------------------------------------------------
// k_traverse_lds: the same traversal with the per-tree scratch in LDS instead of HBM.
//
// The HBM variant moves ~1.1 GB per 262 144-tree launch (profiles/r01_mccfr_hbm_traffic.json) against ~72 MB of
// algorithmic bytes: the multi-pass evaluation re-reads the node list.  Here a node is 4 dwords
// (meta | frel | fsmp | value) in a lane-interleaved LDS array (bank = lane: conflict free), the leaf stack 4
// dwords per entry; reach products of a leaf are rebuilt by walking its (<= 10 node) path instead of being stored.
// One wave per workgroup; 4*maxn + 4*maxs + A dwords per lane (Leduc: 472 B/lane, 30 KB/wave, 5 waves/CU).
// Used when the game fits: <= 62 nodes per sampled tree, depth <= 10, <= 8191 infosets, <= 16 actions.
// ------------------------------------------------------------------------------------------------
#define LM_PARENT(m) ((m)&63u)
#define LM_EDGE(m) (((m) >> 6) & 15u)
#define LM_PTYPE(m) (((m) >> 10) & 3u)
#define LM_LEAF(m) (((m) >> 12) & 1u)
#define LM_WALKER(m) (((m) >> 13) & 1u)
#define LM_ISLOT(m) (((m) >> 14) & 31u)  // internal nodes: rank among the internal nodes (their reach-prefix slot)
#define LM_INFO(m) ((m) >> 19)
#define LM_NO_PARENT 63u

// TVREG:  at most 4 actions, the per-action values of a root live in registers, not LDS.
// The per-infoset sigma / q tables are read through L1 (a per-wave LDS copy measured slower on Leduc: 0.57 vs 0.54 ms per 2^20 trees).
// A node is TWO dwords (meta, value): the reach factor of its incoming edge is not stored but looked up as
// table[infoset(parent)][edge] whenever a sweep needs it.  Leduc: 78 dwords per lane = 8 waves/CU.
template <bool TVREG>
__global__ __launch_bounds__(64) void k_traverse_lds(DevGame g, DevInfoTab it, DevDecisions dc, StepParams p, uint32_t maxn,
                                                     uint32_t maxs, uint32_t maxi) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t ln = threadIdx.x;
    const uint32_t lane = blockIdx.x * 64 + ln;
    uint32_t* nm = lds;                                              // [maxn][64] meta
    float* nv = reinterpret_cast<float*>(nm + (size_t)maxn * 64);    // [maxn][64] leaf: payoff; internal: child-value sum
    float* tv = nv + (size_t)maxn * 64;                              // [A][64] (absent when TVREG)
    float tvr[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    auto tv_set = [&](uint32_t e, float v) {
        if (TVREG) {
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) tvr[q] = e == q ? v : tvr[q];
        } else {
            tv[e * 64 + ln] = v;
        }
    };
    auto tv_get = [&](uint32_t e) -> float {
        if (TVREG) {
            float r = tvr[0];
#pragma unroll
            for (uint32_t q = 1; q < 4; ++q) r = e == q ? tvr[q] : r;
            return r;
        }
        return tv[e * 64 + ln];
    };
    // build phase: the DFS stack; evaluation phase: per-root reach prefixes of internal nodes (same storage)
    uint32_t* ss = reinterpret_cast<uint32_t*>(tv + (TVREG ? 0 : (size_t)g.A * 64));  // [maxs][4][64] stack: record x | meta << 16, y, z, w
    // reach prefixes exist for INTERNAL nodes only: slot = rank of the node among the internal nodes (popcount of a
    // register mask)
    float* xr = reinterpret_cast<float*>(ss);                        // [maxi][64] relative reach root's child -> node
    float* xs = xr + (size_t)maxi * 64;                              // [maxi][64] sampling reach root's child -> node
    const uint32_t cells = g.n_infos * g.A;
    auto SIG = [&](uint32_t e) -> float { return it.sigma[e]; };
    if (lane >= p.batch) return;
    const uint64_t tree_id = p.tree_base + lane;
    uint32_t err = 0;
#define L(arr, slot) arr[(slot)*64 + ln]
#define STK(e, f) ss[((e)*4u + (f)) * 64u + ln]
    // reach factors of the edge into a node (meta mn): sigma / q of the parent's infoset at the node's edge
    // (sigma, q) of the edge into a node: (1, 1) below chance, (sigma, 1) below the walker, (sigma, q) below an opponent
    // mp: the meta of mn's parent
    auto f_of = [&](uint32_t mn, uint32_t mp) -> float2 {
        const uint32_t pt = LM_PTYPE(mn);
        if (pt != PT_WALKER && pt != PT_OPP) return make_float2(1.0f, 1.0f);
        const uint32_t e = LM_INFO(mp) * g.A + LM_EDGE(mn);
        float2 f = it.sq[e];
        if (pt != PT_OPP) f.y = 1.0f;
        return f;
    };
    // the same lookup issued AHEAD of its use, for metas that may lie past the subtree (stale LDS): a bounds-checked
    // buffer load (out of range -> 0) of the raw (sigma, q) pair; f_fix applies the parent-type rule once it is used
    const __amdgpu_buffer_rsrc_t sq_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2*>(it.sq), 0, (int)(cells * 8u), 0x00020000);
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    auto f_issue = [&](uint32_t mn, uint32_t mp) -> float2 {
        const uint32_t e = LM_INFO(mp) * g.A + LM_EDGE(mn);
        const u32x2 raw = __builtin_amdgcn_raw_buffer_load_b64(sq_rsrc, (int)(e * 8u), 0, 0);
        return make_float2(rp_u2f(raw.x), rp_u2f(raw.y));
    };
    auto f_fix = [&](uint32_t mn, float2 f) -> float2 {
        const uint32_t pt = LM_PTYPE(mn);
        if (pt != PT_WALKER && pt != PT_OPP) return make_float2(1.0f, 1.0f);
        if (pt != PT_OPP) f.y = 1.0f;
        return f;
    };

    // ---- TreeBuilder::build (builder.rs:74-87,141-161): pop-last DFS -----------------------------
    // A node arrives as its RECORD (DevGame::kids): the records of all sampled children are requested together
    // when their parent is expanded, so a tree pays one L2 round trip per internal node, not two or three per node.
    // The last child pushed is the next node popped: it is carried in registers instead of through the stack.
    uint32_t nn = 0, sp = 0;
    uint4 rec = g.root_rec;
    uint32_t cur_in = LM_NO_PARENT | (PT_NONE << 10);
    unsigned long long wmask = 0;  // walker decision nodes
    uint32_t n_int = 0;            // internal nodes so far
    for (;;) {
        const uint32_t turn = rec.x & 0xffu, nch = (rec.x >> 8) & 0xffu, info = rec.y, off = rec.z;
        const uint32_t me = nn;
        if (nn >= maxn) {
            err |= ERR_NODE_CAPACITY;
            break;
        }
        const bool is_walker = turn == p.walker;
        L(nm, me) = cur_in | ((nch == 0 ? 1u : 0u) << 12) | ((is_walker ? 1u : 0u) << 13) | ((n_int & 31u) << 14) |
                    ((turn < RP_TURN_CHANCE ? info : 0u) << 19);
        nn += 1;
        if (nch > 0) {
            n_int += 1;
            if (is_walker) wmask |= 1ull << me;
            uint32_t mask = d_sample_mask_tab(g, it, p, tree_id, rec.w, turn, nch, info, off);
            const bool chance = turn == RP_TURN_CHANCE;
            const uint32_t ptype = chance ? PT_CHANCE : (is_walker ? PT_WALKER : PT_OPP);
            const uint32_t last = 31u - (uint32_t)__builtin_clz(mask);
            mask &= ~(1u << last);
            rec = g.kids[off + last];
            while (mask) {
                const uint32_t k = (uint32_t)__builtin_ctz(mask);
                mask &= mask - 1u;
                if (sp >= maxs) {
                    err |= ERR_STACK_CAPACITY;
                    break;
                }
                const uint4 kr = g.kids[off + k];
                STK(sp, 0) = kr.x | ((me | (k << 6) | (ptype << 10)) << 16);
                STK(sp, 1) = kr.y;
                STK(sp, 2) = kr.z;
                STK(sp, 3) = kr.w;
                sp += 1;
            }
            if (err) break;
            cur_in = me | (last << 6) | (ptype << 10);
            continue;
        }
        L(nv, me) = g.n_players == 2 ? rp_u2f(p.walker == 0 ? rec.y : rec.z) : g.payoffs[off * g.n_players + p.walker];
        if (sp == 0) break;
        sp -= 1;
        const uint32_t xm = STK(sp, 0);
        rec = make_uint4(xm & 0xffffu, STK(sp, 1), STK(sp, 2), STK(sp, 3));
        cur_in = xm >> 16;
    }
#undef STK

    // ---- Tree::partition + CfrFlow::dfs per walker infoset (tree.rs:88-98, flow.rs:64-87) --------
    const bool fuse = g.A <= 2;  // every node has at most two children
    uint32_t ndec = 0;
    if (n_int > maxi || n_int > 32u) err |= ERR_NODE_CAPACITY;
    if (!err) {
        unsigned long long todo = wmask;
        while (todo) {
            const uint32_t i = (uint32_t)__builtin_ctzll(todo);  // head of the next infoset span
            const uint32_t mi = L(nm, i);
            const uint32_t info = LM_INFO(mi);
            if (ndec >= dc.maxdec) {
                err |= ERR_DEC_CAPACITY;
                break;
            }
            const uint32_t nact = g.info_actions[info];
            const uint32_t slot = ndec++;
            const size_t D = dc.stride;
            float payoff = 0.0f;
            uint32_t expanded = 0;
            unsigned long long span = todo;
            while (span) {  // roots of the span in ascending node index
                const uint32_t j = (uint32_t)__builtin_ctzll(span);
                span &= span - 1ull;
                if (j != i && LM_INFO(L(nm, j)) != info) continue;
                todo &= ~(1ull << j);
                // top-down over the (contiguous) subtree of j: reach products from j's child (flow.rs:195-212),
                // which start at 1 there; internal nodes also start their child-value sum at 0
                // With at most two children per node (fuse) a sum of child values does not depend on the order of its
                // additions (0 + x = x, x + y = y + x exactly), so a leaf hands its value to its parent right here and
                // the bottom-up sweep only moves the internal nodes' sums: one factor lookup per node instead of two.
                // The sweep is a three-stage software pipeline: while node n is processed, the factor pair of node n + 1,
                // the parent meta of node n + 2 and the meta of node n + 3 are in flight (a lone wave per SIMD pays every
                // LDS / L1 round trip in full otherwise).  Stages may run past the subtree: they only read.
                uint32_t end = j;
                uint32_t kids = 0;
                uint32_t mnA = L(nm, j + 1), mnB = L(nm, j + 2), mnC = L(nm, j + 3);
                uint32_t mpA = L(nm, LM_PARENT(mnA)), mpB = L(nm, LM_PARENT(mnB));
                float2 fA = f_issue(mnA, mpA);
                for (uint32_t n = j + 1; n < nn; ++n) {
                    const uint32_t mn = mnA, mp = mpA;
                    const float2 fraw = fA;
                    fA = f_issue(mnB, mpB);
                    mpA = mpB;
                    mpB = L(nm, LM_PARENT(mnC));
                    mnA = mnB;
                    mnB = mnC;
                    mnC = L(nm, n + 3);
                    const uint32_t par = LM_PARENT(mn);
                    if (par < j) break;
                    end = n;
                    const bool leaf = LM_LEAF(mn);
                    if (leaf && !fuse) continue;
                    float rel = 1.0f, smp = 1.0f;
                    if (par != j) {
                        const uint32_t ps = LM_ISLOT(mp);
                        const float2 f = f_fix(mn, fraw);
                        rel = L(xr, ps) * f.x;
                        smp = L(xs, ps) * f.y;
                    }
                    if (leaf) {
                        const float v = rel / smp * L(nv, n);
                        if (par == j) {
                            tv_set(LM_EDGE(mn), v);
                            kids |= 1u << LM_EDGE(mn);
                        } else {
                            L(nv, par) = L(nv, par) + v;
                        }
                        continue;
                    }
                    const uint32_t ns = LM_ISLOT(mn);
                    L(xr, ns) = rel;
                    L(xs, ns) = smp;
                    L(nv, n) = 0.0f;
                }
                // bottom-up: descending node index adds children in choices() order (node.rs:103-107)
                uint32_t mn_prev = L(nm, end);
                float v_prev = L(nv, end);
                for (uint32_t n = end; n > j; --n) {
                    const uint32_t mn = mn_prev;
                    const uint32_t par = LM_PARENT(mn);
                    float v = v_prev;
                    mn_prev = L(nm, n - 1);  // one node ahead; its value is patched below if this node is its child
                    v_prev = L(nv, n - 1);
                    if (fuse && LM_LEAF(mn)) continue;  // already with its parent
                    if (LM_LEAF(mn)) {
                        float rel = 1.0f, smp = 1.0f;
                        if (par != j) {
                            const uint32_t mp = L(nm, par), ps = LM_ISLOT(mp);
                            const float2 f = f_of(mn, mp);
                            rel = L(xr, ps) * f.x;
                            smp = L(xs, ps) * f.y;
                        }
                        v = rel / smp * v;
                    }
                    if (par == j) {
                        tv_set(LM_EDGE(mn), v);
                        kids |= 1u << LM_EDGE(mn);
                    } else {
                        const float sum = (par == n - 1 ? v_prev : L(nv, par)) + v;
                        L(nv, par) = sum;
                        if (par == n - 1) v_prev = sum;
                    }
                }
                // ancestor_reach (flow.rs:166-174)
                float cf = 1.0f, sm_ = 1.0f;
                for (uint32_t mn = L(nm, j);;) {
                    const uint32_t par = LM_PARENT(mn);
                    if (par == LM_NO_PARENT) break;
                    const uint32_t mp = L(nm, par);
                    if (LM_PTYPE(mn) == PT_OPP) {
                        const float2 f = f_of(mn, mp);
                        cf = cf * f.x;
                        sm_ = sm_ * f.y;
                    }
                    mn = mp;
                }
                const float reach = cf / sm_;
                float ev = 0.0f;
                for (uint32_t a = 0; a < nact; ++a) {
                    if (!((kids >> a) & 1u)) continue;
                    const float u = reach * tv_get(a);
                    tv_set(a, u);
                    ev += SIG(info * g.A + a) * u;
                }
                payoff += ev;
                for (uint32_t a = 0; a < nact; ++a) {
                    if (!((kids >> a) & 1u)) continue;
                    const size_t k = (slot * g.A + a) * D + lane;
                    // first root of the span writes, later roots accumulate (0 + x = x exactly)
                    const float prev = (expanded >> a) & 1u ? dc.regret[k] : 0.0f;
                    dc.regret[k] = prev + (tv_get(a) - ev);
                }
                expanded |= kids;
            }
            for (uint32_t a = 0; a < nact; ++a) {  // policy_vector = iterated_distribution (profile.rs:47-51)
                dc.policy[(slot * g.A + a) * D + lane] = SIG(info * g.A + a);
                if (!((expanded >> a) & 1u)) dc.regret[(slot * g.A + a) * D + lane] = 0.0f;
            }
            dc.info[slot * D + lane] = info;
            dc.mask[slot * D + lane] = expanded;
            dc.payoff[slot * D + lane] = payoff;
            if (dc.slotmap) dc.slotmap[(size_t)info * D + lane] = (uint8_t)(slot + 1);
        }
    }
#undef L
    dc.ndec[lane] = (uint8_t)ndec;
    count_metrics(p, nn, ndec, err);
}

}  // namespace rp

#endif
