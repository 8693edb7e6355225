// nlmc_match.hpp — matches: heads-up hands played from the deal to the settlement between two agents, each reading a device-resident
// blueprint, written as rp_aivat_hand records (rp_nlhe_match).  Read-only on both tables, like nlmc_query.hpp.
//
// Reference: the table of parlor/src/engine.rs:48-68 (recall), 268-320 (ask / next_action / poll_action), Agent::sample and
// Brain::policy (parlor/src/players/agent.rs, brain.rs:45-55), Dirac::distrib over nlhe::argmax (dirac.rs, nlhe/src/strategy.rs:77-89),
// Fish::decide (fish.rs), Game::legal / actionize / snap / passive (kicker/src/game.rs:253-280, 741-751, 835-854), Edge's derived Ord
// (kicker/src/edge.rs:18-27, odds.rs:10-11), Settlement::won (settlement.rs:30-32).  The rules are stated in include/rp_mi355x.h above
// rp_nlhe_match.
//
// One lane per hand, NM_BLOCK per workgroup, the game and the witness's counters (NaCounts, nlmc_aivat.hpp) in registers: the engine's
// witness is built on the real buy-ins and dealer and sees the board as dealt, so its game IS the real game and one game is kept.  The
// plays of a record are indexed at run time and are therefore never a per-lane array: each play's kind and chips go to the record in
// global memory as the play is made, the fixed fields and n_plays at the end.  Two tables arrive as two NlTable arguments; the actor
// selects between their pointers.  nlq_find runs divergent: no wave collective and no barrier anywhere in the kernel.
#ifndef RP_NLMC_MATCH_HPP
#define RP_NLMC_MATCH_HPP

#include "nlmc_aivat.hpp"
#include "nlmc_frontier.hpp"

namespace rp {

#define NM_BLOCK 256u
static_assert(sizeof(rp_nlhe_match_args) == 32, "rp_nlhe_match_args is 32 bytes (INTEGRATION.md mirrors it)");
static_assert(sizeof(rp_match_summary) == 40, "rp_match_summary is 40 bytes (INTEGRATION.md mirrors it)");

// ---- Edge's derived Ord as ranks of the edge codes: RP_EDGE_ORD_RANKS restated from the declaration order and checked against it
constexpr uint8_t NM_RANKS[20] = RP_EDGE_ORD_RANKS;
constexpr int NM_OPENS_CE[4] = {2, 3, 4, 5};                                                                                  // NL_OPENS
constexpr int NM_RAISES_CE[10][2] = {{1, 4}, {1, 3}, {1, 2}, {2, 3}, {3, 4}, {1, 1}, {5, 4}, {3, 2}, {2, 1}, {3, 1}};  // NL_RAISES
// (variant, payload, payload) of an edge code as #[derive(Ord)] compares it: the variant's place in the declaration first
constexpr int nm_ord_field(uint32_t e, int f) {
    const int variant = e == NE_DRAW ? 0 : e == NE_FOLD ? 1 : e == NE_CHECK ? 2 : e == NE_CALL ? 3 : e == NE_SHOVE ? 6 : e < NE_RAISE0 ? 4 : 5;
    return f == 0 ? variant : variant == 4 ? (f == 1 ? NM_OPENS_CE[e - NE_OPEN0] : 0) : variant == 5 ? NM_RAISES_CE[e - NE_RAISE0][f - 1] : 0;
}
constexpr bool nm_ord_less(uint32_t a, uint32_t b) {
    for (int f = 0; f < 3; ++f)
        if (nm_ord_field(a, f) != nm_ord_field(b, f)) return nm_ord_field(a, f) < nm_ord_field(b, f);
    return false;
}
constexpr bool nm_ranks_hold() {
    for (uint32_t a = 1; a < 20u; ++a) {
        uint32_t below = 0;
        for (uint32_t b = 1; b < 20u; ++b) below += nm_ord_less(b, a) ? 1u : 0u;
        if (NM_RANKS[a] != below) return false;
    }
    return NM_RANKS[0] == 31;
}
static_assert(nm_ranks_hold(), "RP_EDGE_ORD_RANKS is Edge's derived Ord");
// the table as two words of 5-bit fields: a rank is a shift and a mask, not a load
constexpr uint64_t nm_ranks_packed(uint32_t first) {
    uint64_t w = 0;
    for (uint32_t i = 0; i < 10u; ++i) w |= (uint64_t)NM_RANKS[first + i] << (5u * i);
    return w;
}
__device__ __forceinline__ uint32_t nm_rank(uint32_t e) {
    constexpr uint64_t LO = nm_ranks_packed(0), HI = nm_ranks_packed(10);
    return (uint32_t)((e < 10u ? LO >> (5u * e) : HI >> (5u * (e - 10u))) & 31ull);
}

struct NmArgs {
    uint64_t deal_hash, play_hash;  // rp_node_hash_step(seed, 0) / (seed, 1)
    uint64_t first_id;              // the id of hand 0 of this launch
    uint32_t n;
    int16_t stacks[2];
    uint8_t agent[2], dealer, hero, mirror, snap, board_mode;
    rp_aivat_hand* hands;  // any of the four may be NULL
    int16_t* won;
    uint8_t *rejected, *status;
};

// the nine cards of a deal: *h0, *h1 the holes of seat 0 and seat 1, draws[3] the streets
__device__ __forceinline__ void nm_deal(uint64_t deal_hash, uint64_t deal_id, uint64_t* h0, uint64_t* h1, uint64_t* flop, uint64_t* turn, uint64_t* river) {
    const uint64_t th = rp_node_hash_tree(deal_hash, deal_id);
    uint64_t deck = HAND_MASK, part[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (uint32_t c = 0; c < 9u; ++c) {
        const uint64_t card = nl_nth_card(deck, rp_pick_uniform(rp_node_hash_key(th, c), (uint32_t)__popcll(deck)));
        deck &= ~card;
        part[c < 2u ? 0u : (c < 4u ? 1u : (c < 7u ? 2u : c - 4u))] |= card;  // a compile-time index: the loop is unrolled
    }
    *h0 = part[0], *h1 = part[1], *flop = part[2], *turn = part[3], *river = part[4];
}

// Fish::decide: uniform over legal() without the shove, in legal()'s order: raise (the minimum), call, fold, check
__device__ __forceinline__ bool nm_fish(const NlView& v, uint64_t draw, NlAction* act) {
    const uint32_t n_raise = v.may_raise ? 1u : 0u, n_call = v.may_call ? 1u : 0u, n_fold = v.may_fold ? 1u : 0u, n_check = v.may_check ? 1u : 0u;
    const uint32_t count = n_raise + n_call + n_fold + n_check;
    if (count == 0u) return false;  // the reference's expect(): a lone shove never is the only legal action of a seat asked to move
    const uint32_t pick = rp_pick_uniform(draw, count);
    if (pick < n_raise) *act = NlAction{NA_RAISE, v.to_raise, 0};
    else if (pick < n_raise + n_call) *act = NlAction{NA_CALL, v.to_call, 0};
    else if (pick < n_raise + n_call + n_fold) *act = NlAction{NA_FOLD, 0, 0};
    else *act = NlAction{NA_CHECK, 0, 0};
    return true;
}

// Agent<Blueprint>::sample / Dirac over Brain::policy: the edge played.  dist: RP_DIST_AVERAGED of the row, slot order; the slots are
// visited in Edge's Ord through their place among the infoset's edges
__device__ __forceinline__ uint32_t nm_choose(const float* dist, uint64_t choices, uint32_t nch, bool dirac, uint64_t draw) {
    uint32_t rank[NLMC_A];
#pragma unroll
    for (uint32_t a = 0; a < NLMC_A; ++a) rank[a] = a < nch ? nm_rank((uint32_t)(choices >> (5u * a)) & 31u) : 32u + a;
    float p[NLMC_A];     // the probabilities in Edge order
    uint32_t e[NLMC_A];  // ... and their edges
#pragma unroll
    for (uint32_t k = 0; k < NLMC_A; ++k) p[k] = 0.0f, e[k] = 0;
#pragma unroll
    for (uint32_t a = 0; a < NLMC_A; ++a) {
        uint32_t place = 0;
#pragma unroll
        for (uint32_t b = 0; b < NLMC_A; ++b) place += rank[b] < rank[a] ? 1u : 0u;
#pragma unroll
        for (uint32_t k = 0; k < NLMC_A; ++k) {
            const bool here = a < nch && place == k;
            p[k] = here ? dist[a] : p[k];
            e[k] = here ? (uint32_t)(choices >> (5u * a)) & 31u : e[k];
        }
    }
    uint32_t at = 0;
    if (dirac) {  // max_by, ties Equal: the later of two that do not compare Greater
        float best = p[0];
#pragma unroll
        for (uint32_t k = 1; k < NLMC_A; ++k) {
            const bool take = k < nch && !(best > p[k]);
            best = take ? p[k] : best;
            at = take ? k : at;
        }
    } else {  // WeightedIndex: f32 left folds from 0 in Edge order
        float total = 0.0f;
#pragma unroll
        for (uint32_t k = 0; k < NLMC_A; ++k) total = k < nch ? total + p[k] : total;
        const float threshold = rp_u01(draw) * total;
        float acc = 0.0f;
        bool hit = false;
        at = nch - 1u;  // no edge with threshold < acc: the last one
#pragma unroll
        for (uint32_t k = 0; k < NLMC_A; ++k) {
            acc = k < nch ? acc + p[k] : acc;
            const bool first = !hit && k < nch && threshold < acc;
            at = first ? k : at;
            hit = hit || first;
        }
    }
    uint32_t edge = e[0];
#pragma unroll
    for (uint32_t k = 1; k < NLMC_A; ++k) edge = at == k ? e[k] : edge;
    return edge;
}

// one hand between two of its steps: the game, the witness's counters, the nine cards and the counters of the loop.  k_nl_match keeps it
// in registers from the deal to the settlement; the search match (nlmc_search.hpp) parks it in device memory at a search decision
struct NmHand {
    G2 g;
    NaCounts w;
    uint64_t hole0, hole1, flop, turn_card, river;
    uint32_t status, n_plays, rejected, streets, decision, step, dealer;
    int won;
};

// what a search seat adds to the loop (nlmc_search.hpp); here: nothing, and every call folds away
struct NmNoSearch {
    __device__ __forceinline__ bool seat(int) const { return false; }
    __device__ __forceinline__ bool decide(const NmHand&, int, int, uint64_t, uint32_t, uint32_t, float*) { return true; }
    __device__ __forceinline__ void chose(uint32_t) {}
    __device__ __forceinline__ void edge(uint32_t) {}
};

// the record starts as zeros (the plays past n_plays, and everything of a hand that ends without outputs); the deal; the game
__device__ __forceinline__ void nm_begin(NmHand& h, const NmArgs& q, uint64_t hand_id, rp_aivat_hand* rec) {
    if (rec) {
        uint4* z = reinterpret_cast<uint4*>(rec);
#pragma unroll
        for (uint32_t k = 0; k < sizeof(rp_aivat_hand) / 16u; ++k) z[k] = make_uint4(0u, 0u, 0u, 0u);
    }
    nm_deal(q.deal_hash, q.mirror ? hand_id >> 1 : hand_id, &h.hole0, &h.hole1, &h.flop, &h.turn_card, &h.river);
    if (q.mirror && (hand_id & 1ull)) {
        const uint64_t x = h.hole0;
        h.hole0 = h.hole1;
        h.hole1 = x;
    }
    h.dealer = q.dealer == 2u ? (uint32_t)(hand_id & 1ull) : (uint32_t)q.dealer;
    nrp_from_start(h.g, h.dealer, q.stacks, h.hole0, h.hole1);
    h.w.run.clear();
    h.w.street_begins();
    h.status = RP_RECALL_ILLEGAL;  // what the step bound leaves
    h.n_plays = h.rejected = h.streets = h.decision = h.step = 0;
    h.won = 0;
}

// the hand's loop, from where it stands to its end (true) or to a search decision that waits for its solve (false: nothing of the
// decision is consumed, the same call takes it up again).  The one copy of the loop body: k_nl_match and k_nl_search_advance
template <typename Search>
__device__ __forceinline__ bool nm_play(NmHand& h, const NlTable& t0, const NlTable& t1, const NlParams& p, const NmArgs& q, uint64_t hand_id,
                                        rp_aivat_hand* rec, Search& search) {
    G2& g = h.g;
    NaCounts& w = h.w;
    const uint64_t play_hash = rp_node_hash_tree(q.play_hash, hand_id);
    const DistParams none{1.0f, 0.0f, 0.0f};  // RP_DIST_AVERAGED reads no hyper-parameter
    uint32_t err = 0;
    for (; h.step < NF_MAX_STEPS; ++h.step) {
        const int turn = g.turn();
        if (turn == NT_TERMINAL) {
            int reward[2];
            nl_settle(g, reward);
            h.won = g.at(reward, (int)q.hero) - g.at(g.spent, (int)q.hero);  // Settlement::won
            h.status = h.n_plays > RP_AIVAT_MAX_PLAYS ? (uint32_t)RP_RECALL_LENGTH : (uint32_t)RP_RECALL_OK;
            break;
        }
        if (turn == NT_CHANCE) {
            const int s = g.street();
            g.force_act(NlAction{NA_DRAW, 0, s == 0 ? h.flop : (s == 1 ? h.turn_card : h.river)});
            w.dealt();
            search.edge(NE_DRAW);
            h.streets = (uint32_t)s + 1u;
            continue;
        }
        const uint64_t draw = rp_node_hash_key(play_hash, h.decision);  // read whether the agent uses it or not
        const uint32_t agent = turn ? q.agent[1] : q.agent[0];
        const NlView v = nl_view(g);
        NlAction act;
        if (agent == (uint32_t)RP_AGENT_FISH) {
            if (!nm_fish(v, draw, &act)) break;
        } else {
            uint64_t choices;
            const uint32_t nch = nl_choices_path(v, (int)w.sub_aggr, &choices);
            if (nch == 0u) break;
            const uint64_t c0 = g.cards[0], c1 = g.cards[1];
            const uint32_t present = nl_bucket(p, v.street, turn ? c1 : c0, g.board, &err);
            if (err) {
                h.status = RP_RECALL_LOOKUP;
                break;
            }
            NlTable t;  // the actor's table: both sets of pointers are kernel arguments, the actor selects
            t.slots = turn ? t1.slots : t0.slots;
            t.mask = turn ? t1.mask : t0.mask;
            t.n_keys = nullptr;
            t.rows = turn ? t1.rows : t0.rows;
            float wt[NLMC_A], dist[NLMC_A];
            const bool found = nlq_row_weights(t, w.sub, choices, present, wt);
#pragma unroll
            for (uint32_t a = 0; a < NLMC_A; ++a) wt[a] = found ? wt[a] : 0.0f;
            policy_distribution<NLMC_A>((int)RP_DIST_AVERAGED, none, wt, nch, dist);
            // a search seat past the flop: the blend of its solve's harvest and the blueprint takes dist's place
            if (search.seat(turn) && v.street > 0 && !search.decide(h, turn, v.street, choices, nch, present, dist)) return false;
            const uint32_t e = nm_choose(dist, choices, nch, agent == (uint32_t)RP_AGENT_DIRAC, draw);
            search.chose(e);
            act = nl_actionize(g, e, 0ull);
        }
        h.decision += 1u;
        if (q.snap) {
            act = g.snap(act);
            if (!g.allowed(act)) break;
        } else if (!g.allowed(act)) {  // rejected; the seat times out into passive()
            act = g.passive();
            h.rejected = min(h.rejected + 1u, 255u);
        }
        if (rec && h.n_plays < RP_AIVAT_MAX_PLAYS) {
            rec->kind[h.n_plays] = (uint8_t)act.kind;
            rec->chips[h.n_plays] = (int16_t)((act.kind == NA_FOLD || act.kind == NA_CHECK) ? 0 : act.chips);
        }
        h.n_plays += 1u;
        search.edge(w.note(g, act));
        g.force_act(act);
    }
    return true;
}

// the hand's outputs; -> whether it has any (a hand refused on the way leaves zeros)
__device__ __forceinline__ bool nm_finish(const NmHand& h, const NmArgs& q, uint32_t i, rp_aivat_hand* rec) {
    const bool outputs = h.status == RP_RECALL_OK || h.status == RP_RECALL_LENGTH;
    if (rec) {
        if (outputs) {
            rec->hole[0] = h.hole0;
            rec->hole[1] = h.hole1;
            rec->draws[0] = h.streets > 0u ? h.flop : 0ull;
            rec->draws[1] = h.streets > 1u ? h.turn_card : 0ull;
            rec->draws[2] = h.streets > 2u ? h.river : 0ull;
            rec->stacks[0] = q.stacks[0];
            rec->stacks[1] = q.stacks[1];
            rec->seat = q.hero;
            rec->dealer = (uint8_t)h.dealer;
            rec->n_plays = (uint8_t)min(h.n_plays, RP_AIVAT_MAX_PLAYS);
            rec->board_mode = q.board_mode;
        } else {  // the plays made so far are taken back
            const uint32_t made = min(h.n_plays, RP_AIVAT_MAX_PLAYS);
            for (uint32_t k = 0; k < made; ++k) {
                rec->kind[k] = 0;
                rec->chips[k] = 0;
            }
        }
    }
    if (q.won) q.won[i] = outputs ? (int16_t)h.won : (int16_t)0;
    if (q.rejected) q.rejected[i] = outputs ? (uint8_t)h.rejected : (uint8_t)0;
    if (q.status) q.status[i] = (uint8_t)h.status;
    return outputs;
}

__global__ __launch_bounds__(NM_BLOCK) void k_nl_match(NlTable t0, NlTable t1, NlParams p, NmArgs q) {
    const uint32_t i = blockIdx.x * NM_BLOCK + threadIdx.x;
    if (i >= q.n) return;
    const uint64_t hand_id = q.first_id + i;
    rp_aivat_hand* rec = q.hands ? q.hands + i : nullptr;
    NmHand h;
    NmNoSearch none;
    nm_begin(h, q, hand_id, rec);
    nm_play(h, t0, t1, p, q, hand_id, rec, none);
    nm_finish(h, q, i, rec);
}

}  // namespace rp

#endif
