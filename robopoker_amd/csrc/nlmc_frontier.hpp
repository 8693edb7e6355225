// nlmc_frontier.hpp — the frontier payoff matrix of depth-limited solving (rp_nlhe_frontier_payoffs): for each of the 4 x 4 pairs of
// continuation strategies, `rollouts` Monte-Carlo games from the frontier state to the end under the blueprint's averaged policy,
// biased towards folding / calling / raising.  Read-only, like nlmc_query.hpp and nlmc_range.hpp.
//
// Reference: DepthSampler::payoffs (nlhe/src/solver.rs:39-67), NlheEncoder::biased_rollout / sample_biased
// (nlhe/src/encoder.rs:70-147), resume (:59-67), Game::apply / reveal / settlements (kicker/src/game.rs:234-248, 605-616),
// Settlement::won (settlement.rs:30-32).  The rules are stated in include/rp_mi355x.h above rp_nlhe_frontier_payoffs.
//
// The factorisation.  The reference plays 16 x rollouts independent games per frontier, each a chain of rules-engine steps with one
// abstraction lookup and one policy lookup per decision.  Every game of a frontier starts from the same state and the same prefix
// path, so one workgroup answers one frontier in three phases:
//   A  lane 0 validates the record and replays its history ONCE (nlmc_replay.hpp, shared with the ranges), leaving the game, and
//      the 12-edge path of the prefix, in LDS;
//   B  one lane per rollout, the game and the path in registers.  The story is never an array: a key reads only the first 12
//      edges of prefix ++ rollout edges, and of those only the trailing choice edges and their aggression (NrpPath: one register
//      pair and three counters).  Per decision: nl_bucket, the home slot and the home row's weights loaded together with the
//      probe (nlq_row_weights), the averaged fold, the biased scan.  Rollouts are laid out cell-major — cell = 4 k + j, then r —
//      so that the lanes of a wavefront share (k, j) whenever a pass holds 64 or more rollouts per cell, and k otherwise: lanes
//      that bias alike take the same branches more often;
//   C  sixteen lanes each fold one cell.
// Rollouts are taken NF_CHUNK per cell and pass (4 096 lanes' worth of int16 in LDS), phase C carrying its sums from pass to pass.
// No atomic and no store touches the table; nlq_find runs divergent and no wave collective sits inside the rollout loop (the
// barriers stand between the passes, where the trip count is the same for every lane).
#ifndef RP_NLMC_FRONTIER_HPP
#define RP_NLMC_FRONTIER_HPP

#include "nlmc_query.hpp"
#include "nlmc_replay.hpp"

namespace rp {

#define NF_BLOCK 256u
#define NF_CELLS (RP_NLHE_FRONTIER_LEAVES * RP_NLHE_FRONTIER_LEAVES)
#define NF_CHUNK 256u  // rollouts per cell and pass
// The step bound of one rollout.  Chips are finite and every aggressive action commits some: a raise puts in at least to_raise() >=
// the big blind (2 chips), a shove a whole non-empty stack, and the two stacks hold at most 2 x 32 767 chips (int16), so a game has
// at most 32 767 aggressive actions.  Between two of them lie at most the passive actions and the deals of four streets: heads-up,
// a street takes two checks, or a call (before the flop: a call and a check), and then it closes — 2 x 4 passive steps and 3 deals,
// 11 in all.  12 x 32 768 steps therefore end every game the rules allow; with the reference's 200-chip stacks a game has at most
// 200 aggressive actions and the bound is never near.
#define NF_MAX_STEPS (12u * 32768u)
static_assert(sizeof(rp_nlhe_frontier) == 112, "rp_nlhe_frontier is 112 bytes (INTEGRATION.md mirrors it)");
static_assert(RP_NLHE_FRONTIER_LEAVES == 4u, "continuations: none, fold, call, raise (pokerkit FRONTIER_LEAVES)");

struct NfArgs {
    const rp_nlhe_frontier* frontiers;
    float bias;
    uint32_t rollouts;   // 1 .. 4096
    uint64_t step_hash;  // rp_node_hash_step(seed, 0)
    uint64_t first_id;   // the id of frontiers[0]
    float* payoffs;      // [n][4][4]
    int16_t* won;        // [n][16][rollouts], may be NULL
    uint8_t* status;     // [n], may be NULL
};

struct NfPublic {
    G2 game;       // the frontier state, both seats holding their cards
    NrpPath path;  // the prefix as a key reads it
    uint32_t status, internal;
};

// Phase A: validation and the replay.  Returns the status; on RP_RECALL_OK the game and the prefix path are set.  `both`: the holes of
// both seats are inputs; else only `internal`'s is, and the other seat holds nothing (the subgame solve deals it, nlmc_subgame.hpp).
__device__ __forceinline__ uint32_t nf_replay(const rp_nlhe_frontier& fr, NfPublic& pub, bool both) {
    if (fr.n_edges > RP_NLHE_MAX_HISTORY || fr.n_prefix > RP_NLHE_MAX_PREFIX) return RP_RECALL_LENGTH;
    uint32_t st = nrp_check_seats(fr.internal, fr.dealer, (uint32_t)(fr.reserved[0] | fr.reserved[1] | fr.reserved[2] | fr.reserved[3]), fr.stacks);
    if (st != RP_RECALL_OK) return st;
    uint64_t gone = 0;
    const uint64_t hole0 = both || fr.internal == 0 ? fr.holes[0] : 0ull, hole1 = both || fr.internal != 0 ? fr.holes[1] : 0ull;
    if ((st = nrp_check_hole(both ? hole0 : hole0 | hole1, &gone)) != RP_RECALL_OK) return st;  // not both: the one hole there is
    if (both && (st = nrp_check_hole(hole1, &gone)) != RP_RECALL_OK) return st;
    if ((st = nrp_check_draws(fr.draws, gone)) != RP_RECALL_OK) return st;
    uint32_t n_draw_edges = 0;
    if ((st = nrp_check_edges(fr.edges, fr.n_edges, &n_draw_edges)) != RP_RECALL_OK) return st;
    if ((st = nrp_check_edges(fr.prefix, fr.n_prefix, &n_draw_edges)) != RP_RECALL_OK) return st;
    G2 g;
    nrp_from_start(g, fr.dealer, fr.stacks, hole0, hole1);
    for (uint32_t i = 0; i < fr.n_edges; ++i)
        if ((st = nrp_apply(g, fr.edges[i], fr.draws)) != RP_RECALL_OK) return st;
    NrpPath path;
    path.clear();
    for (uint32_t i = 0; i < fr.n_prefix; ++i) path.push(fr.prefix[i]);
    pub.game = g;
    pub.path = path;
    pub.internal = fr.internal;
    return RP_RECALL_OK;
}

// sample_biased's multiplier (encoder.rs:126-132): continuation 1 favours Fold, 2 Check / Call, 3 Open / Raise / Shove, 0 nothing
__device__ __forceinline__ float nf_multiplier(uint32_t continuation, uint32_t e, float bias) {
    const bool folded = e == NE_FOLD, aggro = e == NE_SHOVE || e >= NE_OPEN0;
    const bool hit = continuation == 1u ? folded : (continuation == 2u ? (!folded && !aggro) : (continuation == 3u && aggro));
    return hit ? bias : 1.0f;
}

// One rollout (biased_rollout, encoder.rs:89-115): the utility of seat `internal` in chips.  Draw c of the rollout is
// rp_node_hash_key(tree_hash, c), c counting from 0 in consumption order.  *stuck: the step bound was reached, a decision had no
// choices, or a snapped action was refused (the reference panics, or never returns); *err: nl_bucket's.
__device__ __forceinline__ int nf_rollout(const NlTable& t, const NlParams& p, G2 g, NrpPath path, int internal, uint32_t k, uint32_t j, float bias,
                                          uint64_t tree_hash, uint32_t* err, bool* stuck) {
    const DistParams none{1.0f, 0.0f, 0.0f};  // RP_DIST_AVERAGED reads no hyper-parameter
    uint32_t c = 0;
    for (uint32_t step = 0; step < NF_MAX_STEPS; ++step) {
        const int turn = g.turn();
        if (turn == NT_TERMINAL) {
            int reward[2];
            nl_settle(g, reward);
            return g.at(reward, internal) - g.at(g.spent, internal);  // Settlement::won
        }
        if (turn == NT_CHANCE) {  // game.apply(game.reveal()): one street, the cards picked from the deck one by one
            uint64_t deck = g.deck(), cards = 0;
            const int n_cards = g.street() == 0 ? 3 : 1;
            for (int i = 0; i < n_cards; ++i) {
                const uint64_t card = nl_nth_card(deck, rp_pick_uniform(rp_node_hash_key(tree_hash, c++), (uint32_t)__popcll(deck)));
                cards |= card;
                deck &= ~card;
            }
            g.force_act(NlAction{NA_DRAW, 0, cards});
            path.push(NE_DRAW);
            continue;
        }
        // resume(story, game): the key of the actor's infoset
        const NlView v = nl_view(g);
        uint64_t choices;
        const uint32_t nch = nl_choices_path(v, (int)path.aggr, &choices);
        if (nch == 0u) break;
        const uint64_t c0 = g.cards[0], c1 = g.cards[1];
        const uint32_t present = nl_bucket(p, v.street, turn ? c1 : c0, g.board, err);
        float w[NLMC_A], dist[NLMC_A];
        const bool found = nlq_row_weights(t, path.tail, choices, present, w);
#pragma unroll
        for (uint32_t a = 0; a < NLMC_A; ++a) w[a] = found ? w[a] : 0.0f;
        policy_distribution<NLMC_A>((int)RP_DIST_AVERAGED, none, w, nch, dist);
        // sample_biased (encoder.rs:121-146): f32, one rounding per operation, both folds from 0 in slot order
        const uint32_t continuation = turn == internal ? k : j;
        float total = 0.0f;
#pragma unroll
        for (uint32_t a = 0; a < NLMC_A; ++a) {
            w[a] = dist[a] * nf_multiplier(continuation, (uint32_t)(choices >> (5u * a)) & 31u, bias);
            if (a < nch) total += w[a];
        }
        const float threshold = rp_u01(rp_node_hash_key(tree_hash, c++)) * total;
        float acc = 0.0f;
        uint32_t slot = nch - 1u;  // no slot with threshold < acc: the last one
        bool hit = false;
#pragma unroll
        for (uint32_t a = 0; a < NLMC_A; ++a) {
            if (a < nch) acc += w[a];
            const bool first = !hit && a < nch && threshold < acc;
            slot = first ? a : slot;
            hit = hit || first;
        }
        const uint32_t e = (uint32_t)(choices >> (5u * slot)) & 31u;
        const NlAction act = nl_action_v(v, e);  // game.snap(game.actionize(edge))
        if (!g.allowed(act)) break;
        g.force_act(act);
        path.push(e);
    }
    *stuck = true;
    return 0;
}

// What the status of a frontier needs beside its replay: set by any lane of the workgroup, read after a barrier
struct NfFlags {
    uint32_t lookup_miss, stuck;
};

// Phases B and C for one frontier state by the whole workgroup (NF_BLOCK lanes, every lane calls it: the barriers inside are
// reached uniformly): the 16 x rollouts games of stream `id`, folded per cell.  Lane c < 16 returns the f32 sum of cell c over r
// ascending (the caller divides); `valid` = false plays nothing.  Shared by k_nl_frontier and the depth solver (nlmc_depth.hpp),
// which hands in the state of a tree's frontier node.  s_won: NF_CELLS * NF_CHUNK values of LDS; won: global, may be NULL.
__device__ __forceinline__ float nf_cells(const NlTable& t, const NlParams& p, bool valid, const G2& game, const NrpPath& path, int internal, float bias,
                                          uint32_t rollouts, uint64_t step_hash, uint64_t id, int16_t* s_won, int16_t* won, NfFlags* flags) {
    const uint32_t tid = threadIdx.x;
    float sum = 0.0f;  // lanes 0..15: the cell's running sum
    for (uint32_t r0 = 0; r0 < rollouts; r0 += NF_CHUNK) {
        const uint32_t rc = min(NF_CHUNK, rollouts - r0);
        uint32_t err = 0;
        bool stuck = false;
        if (valid) {
            for (uint32_t x = tid; x < NF_CELLS * rc; x += NF_BLOCK) {
                const uint32_t cell = x / rc, r = r0 + x % rc;
                const uint64_t rid = (id * NF_CELLS + cell) * rollouts + r;  // wrapping
                const int w = nf_rollout(t, p, game, path, internal, cell >> 2, cell & 3u, bias, rp_node_hash_tree(step_hash, rid), &err, &stuck);
                s_won[x] = (int16_t)w;
                if (won) won[(size_t)cell * rollouts + r] = (int16_t)w;
            }
        }
        // every lane that saw one stores the same value; the barrier orders the stores before the read
        if (err) flags->lookup_miss = 1;
        if (stuck) flags->stuck = 1;
        __syncthreads();
        // Phase C.  The reference sums a cell's utilities left to right in f32; this is that fold, r ascending.  The order is in
        // fact immaterial wherever |won| x rollouts <= 2^24 — with the reference's 200-chip stacks |won| <= 200 and rollouts <= 4 096,
        // so every partial sum is an integer below 2^20, exact in f32, and any reduction order gives the same bits.
        if (valid && tid < NF_CELLS)
            for (uint32_t x = 0; x < rc; ++x) sum += (float)s_won[tid * rc + x];
        __syncthreads();
    }
    return sum;
}

__global__ __launch_bounds__(NF_BLOCK) void k_nl_frontier(NlTable t, NlParams p, NfArgs q) {
    __shared__ NfPublic pub;
    __shared__ NfFlags flags;
    __shared__ int16_t s_won[NF_CELLS * NF_CHUNK];
    const uint32_t i = blockIdx.x, tid = threadIdx.x, rollouts = q.rollouts;

    if (tid == 0) {
        pub.status = nf_replay(q.frontiers[i], pub, true);
        flags.lookup_miss = flags.stuck = 0;
    }
    __syncthreads();
    const bool valid = pub.status == RP_RECALL_OK;
    const G2 game = pub.game;
    const NrpPath path = pub.path;
    const float sum = nf_cells(t, p, valid, game, path, (int)pub.internal, q.bias, rollouts, q.step_hash, q.first_id + i, s_won,
                               q.won ? q.won + (size_t)i * NF_CELLS * rollouts : nullptr, &flags);
    // a hole the encoder's tables do not know (the reference panics) or a rollout that could not go on: answered as malformed
    const uint32_t status = !valid ? pub.status : (flags.lookup_miss ? (uint32_t)RP_RECALL_LOOKUP : (flags.stuck ? (uint32_t)RP_RECALL_ILLEGAL : (uint32_t)RP_RECALL_OK));
    if (tid < NF_CELLS) q.payoffs[(size_t)i * NF_CELLS + tid] = status == RP_RECALL_OK ? sum / (float)rollouts : 0.0f;
    if (tid == 0 && q.status) q.status[i] = (uint8_t)status;
    if (status != RP_RECALL_OK && q.won)
        for (uint32_t x = tid; x < NF_CELLS * rollouts; x += NF_BLOCK) q.won[(size_t)i * NF_CELLS * rollouts + x] = 0;
}

}  // namespace rp

#endif
