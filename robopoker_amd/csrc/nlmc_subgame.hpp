// nlmc_subgame.hpp — the safe subgame re-solve (rp_nlhe_subgame_solve): `iterations` steps of SubGameSolver, each on one small tree
// whose opponent was dealt for that iteration from a world of the belief, the world-tagged local profile beside them, the rollouts of
// every frontier in the same launch, then the harvest over the four worlds.  Read-only with respect to the blueprint, like
// nlmc_depth.hpp, of which this is the second kernel: the tree, the sweeps and the update, phases B and C, the ranking, the head of
// the result, the read of the entry infoset and the row export are that file's nd_* functions, one copy for both kernels.
//
// Reference: SubGameSolver::step / harvest (subgame/src/solver.rs:146-229), SubGameEncoder (subgame/src/encoder.rs), WorldInfo
// (world/info.rs), WorldProfile (world/profile.rs) over DepthView (depth/view.rs), NlheEncoder::restrict (nlhe/src/encoder.rs:148-186).
// The rules are stated in include/rp_mi355x.h above rp_nlhe_subgame_solve, as deltas against the depth solve's.
//
// One workgroup per solve.  What is added to an iteration of k_nl_depth:
//   D  the deal, by all lanes.  Lane 0 draws the world; then lane l tries attempts l, l + 256, .. of the header's sequential rule — two
//      hashes, two picks among the free cards, one LDS byte of the belief — and after every round of 256 the workgroup takes the minimum
//      accepted index (an LDS integer atomic).  A world without a member costs ceil(10 000 / 256) = 40 rounds instead of 10 000 serial
//      attempts; one that has none at all goes straight to the fallback.  Lane 0 turns the winning attempt into the hole and puts it
//      into the entry state's cards, from where phases A - C take it: the buckets of that seat, the showdowns, the rollouts' holes.
//   the tag.  A local row's key carries the iteration's world in bits 29-30 of present_kind (present is street << 8 | index: 10 bits);
//      the blueprint is asked for the untagged present.  Within one tree every infoset has the same world.
//   the harvest.  The entry infoset is read in each of the four worlds (its local row of that world, else the blueprint) and folded as
//      the header states; the regret fold runs over the edges in kicker::Edge's derived order, which is not slot order (ns_edge_order).
// The profile is larger than the depth solve's — the tag splits the rows of `internal` four ways, and the other seat's rows follow the
// holes dealt (DESIGN.md §3i has the counts): RP_NLHE_SUBGAME_MAX_ROWS rows, the first ND_ROWS_LDS in LDS, the rest in an overflow
// region of this kernel's own, 16 bits of every key in LDS for the lookups.  The ranks of the export live in the rollouts' buffer.
#ifndef RP_NLMC_SUBGAME_HPP
#define RP_NLMC_SUBGAME_HPP

#include "nlmc_depth.hpp"
#include "nlmc_world.hpp"

namespace rp {

#define NS_BLOCK ND_BLOCK
#define NS_ROWS RP_NLHE_SUBGAME_MAX_ROWS
#define NS_ROWS_OVF (NS_ROWS - ND_ROWS_LDS)
#define NS_TAG_SHIFT ND_PRESENT_BITS
#define NS_NEVER 4  // sh.origin of RP_NLHE_SUBGAME_ORIGIN_NONE: no street lies beyond it
static_assert(NS_BLOCK == NW_BLOCK, "the attempt rounds are one lane per attempt");
static_assert(sizeof(rp_nlhe_subgame_args) == 48 && sizeof(rp_nlhe_subgame_result) == 176 && sizeof(rp_nlhe_subgame_row) == 168 &&
                  sizeof(rp_nlhe_subgame_deal) == 16,
              "INTEGRATION.md mirrors them");
static_assert(NF_CELLS * NF_CHUNK * sizeof(int16_t) >= NS_ROWS * sizeof(uint16_t), "the ranks of the export live in the rollouts' buffer");
static_assert(NS_ROWS <= 0xffffu, "ranks are uint16");

struct NsArgs {
    const rp_nlhe_frontier* entries;
    const uint8_t* hole_world;  // [n][RP_NLHE_MAX_HOLES]: the belief, as rp_nlhe_belief writes it
    const float* weights;       // [n][RP_NLHE_WORLDS]
    const int8_t* origin;       // may be NULL: every solve RP_NLHE_SUBGAME_ORIGIN_NONE
    uint32_t iterations, rollouts, rows_cap, deals_cap;
    float bias, prior;
    uint64_t step_hash_rollout;  // rp_node_hash_step(seed, 0)
    uint64_t step_hash_deal;     // rp_node_hash_step(seed, 1): rp_nlhe_restrict's stream
    uint64_t step_hash_tree;     // rp_node_hash_step(seed, 2)
    uint64_t first_id;
    const uint64_t* ids;  // [n] the id of every solve, or NULL (the public entry points): solve i is first_id + i
    NdRow* overflow;  // [n][NS_ROWS_OVF]
    rp_nlhe_subgame_result* results;
    rp_nlhe_subgame_row* rows;    // [n][rows_cap], may be NULL
    rp_nlhe_subgame_deal* deals;  // [n][deals_cap], may be NULL
};

struct NsShared {  // the belief and the deal of one solve
    uint64_t attempts, deal_hash;
    float weights[RP_NLHE_WORLDS];
    uint32_t members[RP_NLHE_WORLDS];  // candidate holes of each world
    uint32_t drawn[RP_NLHE_WORLDS];
    uint32_t fallbacks, n_free, world, first;  // first: the lowest accepted attempt so far, NW_NEVER: none
    uint8_t free_card[52];
    uint8_t hole_world[RP_NLHE_MAX_HOLES];
};

// the place of an edge code in kicker::Edge's derived Ord (edge.rs:18-27): Draw < Fold < Check < Call < Open(n) < Raise(Odds(n, d)) <
// Shove, Odds compared as the pair (n, d).  The raise codes 10 .. 19 are Odds::GRID in grid order — (1,4) (1,3) (1,2) (2,3) (3,4) (1,1)
// (5,4) (3,2) (2,1) (3,1) — whose ranks as pairs are 3 2 1 5 8 0 9 7 4 6: one nibble each.  Codes outside 1 .. 19 do not occur.
#define NS_EDGE_ORDERS 19u
__device__ __forceinline__ uint32_t ns_edge_order(uint32_t e) {
    if (e == NE_SHOVE) return 18u;
    if (e < NE_SHOVE) return e - 1u;        // Draw 0, Fold 1, Check 2, Call 3
    if (e < NE_RAISE0) return e - 2u;       // Open(2 .. 5): 4 .. 7
    return 8u + (uint32_t)((0x6479085123ull >> (4u * ((e - NE_RAISE0) % 10u))) & 15u);
}

__device__ __forceinline__ bool ns_row_less(const NdRow& a, const NdRow& b) {  // (world, kind, past, present, choices)
    const uint32_t wa = (a.present_kind >> NS_TAG_SHIFT) & 3u, wb = (b.present_kind >> NS_TAG_SHIFT) & 3u;
    if (wa != wb) return wa < wb;
    return nd_row_less(a, b);  // the tags are equal: present_kind compares as present
}

__global__ __launch_bounds__(NS_BLOCK) void k_nl_subgame(NlTable t, NlParams p, NsArgs q) {
    __shared__ NdShared sh;
    __shared__ NsShared sw;
    __shared__ NdNode nodes[ND_NODES];
    __shared__ NdInfo infos[ND_INFOS];
    __shared__ NdRow rows_lds[ND_ROWS_LDS];
    __shared__ uint16_t row_hash[NS_ROWS];  // 16 bits of a key: one lookup in 32 meets a row to refuse at 2 048 rows
    const NdRowsT<uint16_t> rows{rows_lds, q.overflow + (size_t)blockIdx.x * NS_ROWS_OVF, row_hash};
    __shared__ float s_buf[NF_CELLS * NF_CHUNK / 2u];  // the rollouts' int16 buffer; between rollouts the sweeps' floats; at the end the ranks
    int16_t* s_won = reinterpret_cast<int16_t*>(s_buf);
    uint16_t* s_rank = reinterpret_cast<uint16_t*>(s_buf);
    const uint32_t i = blockIdx.x, tid = threadIdx.x;
    const uint64_t id = q.ids ? q.ids[i] : q.first_id + i;  // wrapping

    if (tid == 0) {
        // the hole of the seat opposite `internal` is no input: that seat holds nothing until the first deal
        uint32_t st = nf_replay(q.entries[i], sh.pub, false);
        if (st == RP_RECALL_OK) st = nd_origin(q.origin, i, (int)RP_NLHE_SUBGAME_ORIGIN_NONE, NS_NEVER, &sh.origin);
        for (uint32_t w = 0; w < RP_NLHE_WORLDS; ++w) {
            const float x = q.weights[(size_t)i * RP_NLHE_WORLDS + w];
            if (st == RP_RECALL_OK && (!(x >= 0.0f) || x == INFINITY)) st = RP_RECALL_CARDS;  // a belief that is none
            sw.weights[w] = x;
            sw.members[w] = sw.drawn[w] = 0u;
        }
        uint32_t n_free = 0;
        if (st == RP_RECALL_OK) {  // the free cards in ascending order: the 52 minus internal's hole and the entry's board
            const uint64_t taken = (sh.pub.internal ? sh.pub.game.cards[1] : sh.pub.game.cards[0]) | sh.pub.game.board;
            for (uint32_t c = 0; c < 52u; ++c)
                if (!((taken >> c) & 1ull)) sw.free_card[n_free++] = (uint8_t)c;
        }
        sw.n_free = n_free;  // 52 - 2 - (0, 3, 4 or 5)
        sw.attempts = 0;
        sw.fallbacks = 0;
        sw.first = NW_NEVER;
        nd_begin(sh, st);
    }
    __syncthreads();
    {  // the belief into LDS: a byte that is no world, or lies past the candidates, reads as RP_WORLD_NONE
        const uint32_t n_free = sw.n_free, count = n_free * (n_free - (n_free ? 1u : 0u)) / 2u;  // <= 1 225
        for (uint32_t j = tid; j < RP_NLHE_MAX_HOLES; j += NS_BLOCK) {
            uint32_t w = j < count ? (uint32_t)q.hole_world[(size_t)i * RP_NLHE_MAX_HOLES + j] : RP_WORLD_NONE;
            w = w < RP_NLHE_WORLDS ? w : RP_WORLD_NONE;
            sw.hole_world[j] = (uint8_t)w;
            if (w < RP_NLHE_WORLDS) atomicAdd(&sw.members[w], 1u);
        }
    }
    __syncthreads();
    for (uint32_t it = 0; it < q.iterations; ++it) {
        if (sh.status != RP_RECALL_OK) break;  // uniform: read after a barrier, written before the next
        __syncthreads();
        // Phase D: the deal of this iteration — deal `it` of recall `id` among RP_NLHE_DEPTH_MAX_ITERATIONS, rp_nlhe_restrict's rules
        if (tid == 0) {
            sw.deal_hash = rp_node_hash_tree(q.step_hash_deal, id * RP_NLHE_DEPTH_MAX_ITERATIONS + it);
            sw.world = nw_draw_world(sw.weights, rp_u01(rp_node_hash_key(sw.deal_hash, 0)));
            sw.first = NW_NEVER;
        }
        __syncthreads();
        {
            const uint64_t deal_hash = sw.deal_hash;
            const uint32_t world = sw.world, n_free = sw.n_free;
            if (sw.members[world] != 0u) {  // uniform
                for (uint32_t base = 0; base < RP_NLHE_MAX_REJECTIONS; base += NS_BLOCK) {
                    const uint32_t a = base + tid;
                    if (a < RP_NLHE_MAX_REJECTIONS) {
                        uint32_t hi, lo;
                        nw_attempt(deal_hash, a, n_free, &hi, &lo);  // hi (hi - 1) / 2 + lo < n_free (n_free - 1) / 2 <= 1 225
                        if (sw.hole_world[hi * (hi - 1u) / 2u + lo] == world) atomicMin(&sw.first, a);
                    }
                    __syncthreads();
                    const uint32_t first = sw.first;
                    __syncthreads();  // every lane has read it before a lane of the next round can lower it
                    if (first != NW_NEVER) break;  // uniform.  Later rounds hold higher indices only
                }
            }
        }
        if (tid == 0) {
            const uint32_t a = sw.first == NW_NEVER ? RP_NLHE_MAX_REJECTIONS : sw.first, world = sw.world;
            uint32_t hi, lo;
            nw_attempt(sw.deal_hash, a, sw.n_free, &hi, &lo);  // a = RP_NLHE_MAX_REJECTIONS: the fallback, whatever its world
            const uint64_t hole = (1ull << sw.free_card[hi]) | (1ull << sw.free_card[lo]);
            if (sh.pub.internal) sh.pub.game.cards[0] = hole;
            else sh.pub.game.cards[1] = hole;
            sw.drawn[world] += 1u;
            sw.attempts += a;
            sw.fallbacks += a == RP_NLHE_MAX_REJECTIONS ? 1u : 0u;
            if (q.deals && it < q.deals_cap) {
                rp_nlhe_subgame_deal d{};
                d.hole = hole;
                d.world = (uint8_t)world;
                d.attempts = (uint16_t)a;
                q.deals[(size_t)i * q.deals_cap + it] = d;
            }
            // Phase A
            sh.status = nd_build(t, p, sh, nodes, infos, rows, it & 1u, rp_node_hash_tree(q.step_hash_tree, id * RP_NLHE_DEPTH_MAX_ITERATIONS + it),
                                 world << NS_TAG_SHIFT);
        }
        __syncthreads();
        if (sh.status != RP_RECALL_OK) break;
        nd_frontiers(t, p, sh, nodes, q.entries[i], id, it, q.bias, q.rollouts, q.step_hash_rollout, s_won);
        if (sh.status != RP_RECALL_OK) break;
        if (tid == 0) nd_updates<NS_ROWS, true>(t, sh, nodes, infos, rows, it, q.prior, s_buf);
        __syncthreads();
    }
    __syncthreads();
    if (sh.status == RP_RECALL_OK) nd_rank<ns_row_less>(rows, sh.n_rows, s_rank);
    __syncthreads();
    // the harvest
    if (tid == 0 && nd_result_head(q.results[i], sh, rows, s_rank, q.rollouts)) {
        rp_nlhe_subgame_result& out = q.results[i];
        for (uint32_t w = 0; w < RP_NLHE_WORLDS; ++w) out.drawn[w] = sw.drawn[w];
        out.attempts = sw.attempts;
        out.fallbacks = sw.fallbacks;
        const G2 g = sh.pub.game;  // as the last iteration dealt it
        const int turn = g.turn();
        if (turn >= 0) {  // Harvest at WorldInfo(w, Game(info of the entry state)), w = 0 .. 3
            const NdEntry e = nd_entry(p, g, turn, sh.pub.path);
            const DistParams none{1.0f, 0.0f, 0.0f};
            float* policy = sh.tmp[4];
            uint32_t* v = sh.tmpu;
            for (uint32_t w = 0; w < RP_NLHE_WORLDS; ++w) {
                float* r = sh.tmp[w];  // kept for the regret fold
                nd_entry_row(t, rows, sh.n_rows, sh.pub.path.tail, e, w << NS_TAG_SHIFT, r, v, sh.tmp[5], sh.tmp[6]);
                policy_distribution<NLMC_A>((int)RP_DIST_ITERATED, none, r, e.nch, policy);
                for (uint32_t a = 0; a < e.nch; ++a) {
                    out.refined[a] += policy[a] / 4.0f;  // from the zero of the cleared result
                    out.visits[a] += v[a];                // wrapping
                }
            }
            float regret = 0.0f;  // edges outer, in the BTreeMap's key order; worlds inner
            for (uint32_t k = 0; k < NS_EDGE_ORDERS; ++k)
                for (uint32_t a = 0; a < e.nch; ++a) {
                    if (ns_edge_order((uint32_t)(e.choices >> (5u * a)) & 31u) != k) continue;
                    for (uint32_t w = 0; w < RP_NLHE_WORLDS; ++w) regret += rp_maxf(sh.tmp[w][a], 0.0f);
                }
            nd_result_entry(out, sh, e, regret);
        }
    }
    __syncthreads();
    const bool ok = sh.status == RP_RECALL_OK;
    if (q.rows) nd_export(q.rows + (size_t)i * q.rows_cap, q.rows_cap, ok ? sh.n_rows : 0u, rows, s_rank);
    if (q.deals) {  // the deals of the iterations done; none of a solve that failed
        const uint32_t done = ok ? sh.t : 0u;
        for (uint32_t x = tid; x < q.deals_cap; x += NS_BLOCK)
            if (x >= done) q.deals[(size_t)i * q.deals_cap + x] = rp_nlhe_subgame_deal{};
    }
}

}  // namespace rp

#endif
