// nlmc_replay.hpp — one definition of what every query that REPLAYS an edge-level history shares (nlmc_range.hpp: the ranges,
// nlmc_frontier.hpp: the frontier payoffs): the checks a record passes before it is replayed, Game::from_start, the 12-edge Path a
// key is formed from, and NlheGame::apply with the record's own draws.  The rules are stated in include/rp_mi355x.h above
// rp_nlhe_reaches (REPLAY, KEY, STATUS).
//
// Reference: CfrEncoder::replay (mccfr/src/strategy/encoder.rs:72-84), NlheGame::apply (nlhe/src/game.rs:50-70), Game::from_start
// (kicker/src/game.rs:80-85), NlheEncoder::resume (nlhe/src/encoder.rs:59-67), NlheInfo::from((Path, Abstraction, Path))
// (nlhe/src/info.rs:125-139), Path::from_iter / aggression (kicker/src/path.rs:169-181, 32-38).
#ifndef RP_NLMC_REPLAY_HPP
#define RP_NLMC_REPLAY_HPP

#include "nlmc_common.hpp"

namespace rp {

// ---- the checks that need no replay; each returns RP_RECALL_OK or the status the record is refused with
// seats and stacks: stacks 0,0 = the reference's STACK, otherwise both positive
__device__ __forceinline__ uint32_t nrp_check_seats(uint32_t seat, uint32_t dealer, uint32_t reserved, const int16_t* stacks) {
    if (seat > 1u || dealer > 1u || reserved != 0u) return RP_RECALL_SEAT;
    const bool std_stacks = stacks[0] == 0 && stacks[1] == 0;
    if (!std_stacks && (stacks[0] <= 0 || stacks[1] <= 0)) return RP_RECALL_SEAT;
    return RP_RECALL_OK;
}
// a hole: two cards, none of them in *gone, which it joins
__device__ __forceinline__ uint32_t nrp_check_hole(uint64_t hole, uint64_t* gone) {
    if ((hole & ~HAND_MASK) != 0 || __popcll(hole) != 2 || (hole & *gone) != 0) return RP_RECALL_CARDS;
    *gone |= hole;
    return RP_RECALL_OK;
}
// the draws: 3 / 1 / 1 cards in street order, disjoint from each other and from `gone` (the holes)
__device__ __forceinline__ uint32_t nrp_check_draws(const uint64_t* draws, uint64_t gone) {
    for (uint32_t s = 0; s < 3u; ++s) {
        const uint64_t d = draws[s];
        if (d == 0) continue;
        if ((d & ~HAND_MASK) != 0 || __popcll(d) != (s == 0 ? 3 : 1) || (d & gone) != 0) return RP_RECALL_CARDS;
        if (s > 0 && draws[s - 1] == 0) return RP_RECALL_CARDS;  // a street without the one before it
        gone |= d;
    }
    return RP_RECALL_OK;
}
// edge codes 1..19 (kicker/src/edge.rs:101-120); *n_draw_edges += the Draw edges among them
__device__ __forceinline__ uint32_t nrp_check_edges(const uint8_t* edges, uint32_t n, uint32_t* n_draw_edges) {
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t e = edges[i];
        if (e < NE_DRAW || e >= NE_RAISE0 + 10u) return RP_RECALL_EDGE;
        *n_draw_edges += e == NE_DRAW ? 1u : 0u;
    }
    return RP_RECALL_OK;
}

// Game::from_start(dealer, stacks) (kicker game.rs:80-85) with the seats' cards (0: nothing public depends on them)
__device__ __forceinline__ void nrp_from_start(G2& g, uint32_t dealer, const int16_t* stacks, uint64_t cards0, uint64_t cards1) {
    const bool std_stacks = stacks[0] == 0 && stacks[1] == 0;
    g.n = 2;
    g.dealer = (int)dealer;
    g.ticker = 0;
    g.pot = 0;
    g.board = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        g.state[i] = NL_BETTING;
        g.stack[i] = std_stacks ? 200 : (int)stacks[i];
        g.stake[i] = g.spent[i] = 0;
    }
    g.cards[0] = cards0;
    g.cards[1] = cards1;
    for (int b = 0; b < 2; ++b) g.force_act(NlAction{NA_BLIND, g.to_post(), 0});
}

// The Path resume() collects the edges so far into, as far as a key reads it: Path::from_iter keeps the FIRST 12 edges
// (MAX_PATH_EDGES) and drops the rest, so from the 13th push on nothing changes.  `tail` = the trailing choice edges of that path
// (5-bit fields, first edge lowest: the key's `past`), `aggr` = Path::aggression, the raises / shoves among them.
struct NrpPath {
    uint64_t tail;
    uint32_t tail_len, aggr, n;
    __device__ __forceinline__ void clear() {
        tail = 0;
        tail_len = aggr = n = 0;
    }
    __device__ __forceinline__ void push(uint32_t e) {
        if (n >= 12u) return;
        n += 1u;
        if (e == NE_DRAW) {
            tail = 0;
            tail_len = aggr = 0;
        } else {
            tail |= (uint64_t)e << (5u * tail_len++);
            aggr += (e == NE_SHOVE || e >= NE_OPEN0) ? 1u : 0u;
        }
    }
};

// NlheGame::apply (nlhe/src/game.rs:50-70) with one deviation: where the reference's reveal() deals random cards, street s deals
// draws[s].  At a terminal state nothing changes; a choice edge met at a chance node first deals the pending streets; a Draw edge
// met at a choice node leaves the game unchanged.  RP_RECALL_DRAW: a street is needed and not carried; RP_RECALL_ILLEGAL: the
// snapped action is one the rules refuse.
__device__ __forceinline__ uint32_t nrp_apply(G2& g, uint32_t e, const uint64_t* draws) {
    if (g.turn() == NT_TERMINAL) return RP_RECALL_OK;
    if (e != NE_DRAW) {
        while (g.turn() == NT_CHANCE) {
            const uint64_t d = draws[g.street()];
            if (d == 0) return RP_RECALL_DRAW;
            g.force_act(NlAction{NA_DRAW, 0, d});
        }
        if (g.turn() == NT_TERMINAL) return RP_RECALL_OK;
    } else {
        if (g.turn() != NT_CHANCE) return RP_RECALL_OK;
        const uint64_t d = draws[g.street()];
        if (d == 0) return RP_RECALL_DRAW;
        g.force_act(NlAction{NA_DRAW, 0, d});
        return RP_RECALL_OK;
    }
    const NlAction a = nl_action_v(nl_view(g), e);
    if (!g.allowed(a)) return RP_RECALL_ILLEGAL;
    g.force_act(a);
    return RP_RECALL_OK;
}

}  // namespace rp

#endif
