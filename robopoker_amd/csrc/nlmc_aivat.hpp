// nlmc_aivat.hpp — AIVAT control variates from the NLHE blueprint, one played hand per wavefront (rp_nlhe_aivat).  Read-only, like
// nlmc_query.hpp; the one consumer of the table's payoff column.
//
// Reference: Aivat::corrections / action_node_correction / chance_node_correction (arena/src/aivat.rs:63-229), strategy_ev /
// observed_ev (arena/src/correction.rs:4-22), Replayer (arena/src/replay.rs:90-168), eval_chance_correction's SQL
// (arena/src/repository.rs:397-442), Witness::try_arrange / try_push / sprout (kicker/src/witness.rs:193-213, 456-463, 497-505),
// Recall::aggression / history / subgame (kicker/src/recall.rs:63-112), NlheInfo::from((&Recall, Abstraction))
// (nlhe/src/info.rs:117-122), GameN::edgify (kicker/src/game.rs:754-766, 813-818).  The rules are stated in include/rp_mi355x.h
// above rp_nlhe_aivat.
//
// Two games advance together, both wave-uniform and replayed by every lane, in registers: the WALKER (the hand's dealer and stacks,
// the real actions) and the WITNESS game (dealer 0, STACK stacks, whatever the hand says; it deals every street the hand carries as
// soon as its head reaches a chance node).  The two witnesses of the reference differ only in the cards they have seen, so one game
// serves both.  Three aggression counts live beside the witness:
//   run   the reference's running Path of history(): the FIRST 12 edges of the whole history, Draws included (NrpPath); its
//         aggression is the depth the history's own edges are snapped with;
//   sub   subgame(): the FIRST 12 edges of the current street; the key's `past`, and its aggression picks the key's `choices`;
//   act   Recall::aggression(): the Raise / Shove ACTIONS of the current street, no cut; the depth the OBSERVED edge is snapped with.
// An action node is one probe: every lane loads the same row (a broadcast) and folds its slots in slot order.  At a chance node lane
// d owns deal d (at most 45 of 64): canonicalisation, bucket, probe and the 9-slot fold run per lane, divergent, up to 45 probes in
// flight per wavefront; then every lane folds the deals in deal order out of shuffles.  nlq_find holds no wave collective.
#ifndef RP_NLMC_AIVAT_HPP
#define RP_NLMC_AIVAT_HPP

#include "nlmc_query.hpp"
#include "nlmc_replay.hpp"

namespace rp {

#define NA_BLOCK 64u
static_assert(sizeof(rp_aivat_hand) == 192, "rp_aivat_hand is 192 bytes (INTEGRATION.md mirrors it)");
static_assert(RP_PLAY_FOLD == NA_FOLD && RP_PLAY_CALL == NA_CALL && RP_PLAY_CHECK == NA_CHECK && RP_PLAY_RAISE == NA_RAISE &&
                  RP_PLAY_SHOVE == NA_SHOVE,
              "rp_aivat_play is the engine's action kind");

struct NaArgs {
    const rp_aivat_hand* hands;
    float *hero, *villain, *chance, *total;
    uint8_t *n_action, *n_chance, *status;  // any may be NULL
};

// what Recall derives from a witness's actions, kept beside its game (shared with the match kernel, nlmc_match.hpp, whose
// witness game is the real game)
struct NaCounts {
    NrpPath run;                 // history()'s running Path: only its aggression is read
    uint64_t sub;                // subgame(): the street's first 12 edges, 5-bit fields
    uint32_t sub_len, sub_aggr;  // ... their number and the raises / shoves among them
    uint32_t act_aggr;           // Recall::aggression()
    __device__ __forceinline__ void street_begins() {
        sub = 0;
        sub_len = sub_aggr = act_aggr = 0;
    }
    // the action joins the history as the edge history() gives it on the game BEFORE the action; -> that edge
    __device__ __forceinline__ uint32_t note(const G2& g, const NlAction& a) {
        const uint32_t e = nl_edgify(g, a, (int)run.aggr);
        run.push(e);
        if (sub_len < 12u) {
            sub |= (uint64_t)e << (5u * sub_len++);
            sub_aggr += (e == NE_SHOVE || e >= NE_OPEN0) ? 1u : 0u;
        }
        act_aggr += (a.kind == NA_RAISE || a.kind == NA_SHOVE) ? 1u : 0u;
        return e;
    }
    // note() for a history whose edges come from Game::translate (nlmc_translate.hpp): the action joins as the edge given
    __device__ __forceinline__ void note_edge(const NlAction& a, uint32_t e) {
        run.push(e);
        if (sub_len < 12u) {
            sub |= (uint64_t)e << (5u * sub_len++);
            sub_aggr += (e == NE_SHOVE || e >= NE_OPEN0) ? 1u : 0u;
        }
        act_aggr += (a.kind == NA_RAISE || a.kind == NA_SHOVE) ? 1u : 0u;
    }
    // a street was dealt into the witness game
    __device__ __forceinline__ void dealt() {
        run.push(NE_DRAW);
        street_begins();
    }
};

// the witness game and what Recall derives from its actions
struct NaWitness : NaCounts {
    G2 g;
    uint32_t streets;            // seen().street(): the streets the hand's draws carry
    // try_push after can_push: the action joins the history as the edge history() gives it, then sprout()
    __device__ __forceinline__ void push(const NlAction& a, const uint64_t* draws) {
        note(g, a);
        g.force_act(a);
        while ((uint32_t)g.street() < streets && g.turn() == NT_CHANCE) {
            g.force_act(NlAction{NA_DRAW, 0, draws[g.street()]});
            dealt();
        }
    }
    // head().choices(subgame().aggression()); no choices where the head is no decision node
    __device__ __forceinline__ uint32_t choices(uint64_t* path) const {
        *path = 0;
        return g.turn() < 0 ? 0u : nl_choices_path(nl_view(g), (int)sub_aggr, path);
    }
};

// Σ_slots in slot order, f32, every operation rounded on its own (include/rp_math.h)
__device__ __forceinline__ float na_sum(const float* x, uint32_t nch) {
    float s = 0.0f;
#pragma unroll
    for (uint32_t a = 0; a < NLMC_A; ++a) s = a < nch ? s + x[a] : s;
    return s;
}

// action_node_correction: false = None
__device__ __forceinline__ bool na_action(const NlTable& t, const NlParams& p, const NaWitness& w, const G2& walker, const NlAction& act, uint64_t pocket,
                                          uint64_t board, int street, float* delta) {
    uint32_t err = 0;
    const uint32_t present = nl_bucket(p, street, pocket, board, &err);
    if (err) return false;  // eval_abstraction: no row of the lookup tables
    uint64_t choices;
    const uint32_t nch = w.choices(&choices);
    if (nch == 0u) return false;  // an infoset without slots has no rows
    float wt[NLMC_A], v[NLMC_A];
    if (!nlq_row_weights_payoffs(t, w.sub, choices, present, wt, v)) return false;
    const float total = na_sum(wt, nch);
    if (total <= 0.0f) return false;
    const uint32_t edge = nl_edgify(walker, act, (int)w.act_aggr);
    float ev = 0.0f, seen = 0.0f;
    bool among = false;
#pragma unroll
    for (uint32_t a = 0; a < NLMC_A; ++a) {
        if (a < nch) ev = ev + (wt[a] / total) * v[a];
        if (a < nch && !among && ((choices >> (5u * a)) & 31ull) == edge) among = true, seen = v[a];
    }
    *delta = ev - (among ? seen : ev);
    return true;
}

// chance_node_correction at the walker's chance node of street 1 or 2 (flop -> turn, turn -> river): false = None
__device__ __forceinline__ bool na_chance(const NlTable& t, const NlParams& p, const NaWitness& w, const G2& walker, const rp_aivat_hand& h, uint64_t observed,
                                          uint32_t lane, float* delta) {
    G2 sample = walker;
    sample.force_act(NlAction{NA_DRAW, 0, observed});
    const int next = sample.turn();
    if (next < 0) return false;
    const bool hero_next = next == (int)h.seat;
    const uint64_t pocket = h.hole[hero_next ? h.seat : 1u - h.seat];
    uint64_t choices;
    const uint32_t nch = w.choices(&choices);
    if (nch == 0u) return false;  // nothing joins
    const uint64_t free_cards = ~(h.hole[0] | h.hole[1] | walker.board) & HAND_MASK;
    const uint32_t count = (uint32_t)__popcll(free_cards);  // 45 or 44
    const int street = walker.street() + 1;
    // lane d: deal d of HandIterator::from((1, mask)).  state 0: dropped by the join, 1: joined, baseline NULL, 2: joined with a value
    uint32_t state = 0;
    float base = 0.0f;
    if (lane < count) {
        const uint64_t card = nl_nth_card(free_cards, lane);
        uint32_t err = 0;
        const uint32_t present = nl_bucket(p, street, pocket, walker.board | card, &err);
        float wt[NLMC_A], v[NLMC_A], wv[NLMC_A];
        if (!err && nlq_row_weights_payoffs(t, w.sub, choices, present, wt, v)) {
#pragma unroll
            for (uint32_t a = 0; a < NLMC_A; ++a) wv[a] = wt[a] * v[a];
            const float sw = na_sum(wt, nch), swv = na_sum(wv, nch);
            state = sw == 0.0f ? 1u : 2u;  // NULLIF(SUM(weight), 0)
            base = sw == 0.0f ? 0.0f : swv / sw;
        }
    }
    // Σ_deals in deal order; COUNT(*) counts the NULL baselines, SUM skips them
    float sum = 0.0f;
    uint32_t joined = 0, valued = 0;
    for (uint32_t d = 0; d < count; ++d) {
        const uint32_t s = (uint32_t)__shfl((int)state, (int)d);
        const float b = __shfl(base, (int)d);
        joined += s != 0u ? 1u : 0u;
        valued += s == 2u ? 1u : 0u;
        sum = s == 2u ? sum + b : sum;
    }
    const uint32_t at = (uint32_t)__popcll(free_cards & (observed - 1ull));  // the observed deal's place among the deals
    const uint32_t obs_state = (uint32_t)__shfl((int)state, (int)at);
    const float obs = __shfl(base, (int)at);
    if (valued == 0u || obs_state != 2u) return false;
    const float avg = (float)((double)sum / (double)joined);
    const float d = avg - obs;
    *delta = hero_next ? d : -d;
    return true;
}

struct NaOut {
    float hero, villain, chance;
    uint32_t n_action, n_chance;
};

// Aivat::corrections, statement by statement; returns the hand's status
__device__ __forceinline__ uint32_t na_hand(const NlTable& t, const NlParams& p, const rp_aivat_hand& h, uint32_t lane, NaOut& o) {
    o.hero = o.villain = o.chance = 0.0f;
    o.n_action = o.n_chance = 0;
    if (h.n_plays > RP_AIVAT_MAX_PLAYS) return RP_RECALL_LENGTH;
    uint32_t st = nrp_check_seats(h.seat, h.dealer, h.board_mode > 1u ? 1u : 0u, h.stacks);
    if (st != RP_RECALL_OK) return st;
    uint64_t gone = 0;
    if ((st = nrp_check_hole(h.hole[0], &gone)) != RP_RECALL_OK) return st;
    if ((st = nrp_check_hole(h.hole[1], &gone)) != RP_RECALL_OK) return st;
    if ((st = nrp_check_draws(h.draws, gone)) != RP_RECALL_OK) return st;
    for (uint32_t i = 0; i < h.n_plays; ++i)
        if (h.kind[i] < (uint8_t)RP_PLAY_FOLD || h.kind[i] > (uint8_t)RP_PLAY_SHOVE) return RP_RECALL_EDGE;

    G2 walker;
    nrp_from_start(walker, h.dealer, h.stacks, h.hole[0], h.hole[1]);
    NaWitness w;
    const int16_t std_stacks[2] = {0, 0};
    nrp_from_start(w.g, 0u, std_stacks, 0ull, 0ull);
    w.run.clear();
    w.street_begins();
    w.streets = (h.draws[0] != 0) + (h.draws[1] != 0) + (h.draws[2] != 0);
    const uint64_t all_board = h.draws[0] | h.draws[1] | h.draws[2];

    for (uint32_t i = 0; i < h.n_plays; ++i) {
        if (walker.turn() == NT_TERMINAL) break;
        while (walker.turn() == NT_CHANCE) {
            const int s = walker.street();
            const uint64_t d = h.draws[s];
            if (d == 0) return RP_RECALL_DRAW;
            float delta;
            if (s != 0 && na_chance(t, p, w, walker, h, d, lane, &delta)) {
                o.chance += delta;
                o.n_chance += 1u;
            }
            walker.force_act(NlAction{NA_DRAW, 0, d});
        }
        const int kind = (int)h.kind[i];
        const NlAction act{kind, (kind == NA_FOLD || kind == NA_CHECK) ? 0 : (int)h.chips[i], 0};
        const int turn = walker.turn();
        if (turn >= 0) {
            const bool hero = turn == (int)h.seat;
            const bool at_node = h.board_mode != 0u;
            float delta;
            if (na_action(t, p, w, walker, act, h.hole[turn], at_node ? walker.board : all_board, at_node ? walker.street() : (int)w.streets, &delta)) {
                if (hero) o.hero += delta;
                else o.villain -= delta;
                o.n_action += 1u;
            }
        }
        if (!w.g.allowed(act)) return walker.allowed(act) ? (uint32_t)RP_AIVAT_WITNESS : (uint32_t)RP_RECALL_ILLEGAL;
        w.push(act, h.draws);
        if (!walker.allowed(act)) return RP_RECALL_ILLEGAL;
        walker.force_act(act);
    }
    return RP_RECALL_OK;
}

__global__ __launch_bounds__(NA_BLOCK) void k_nl_aivat(NlTable t, NlParams p, NaArgs q) {
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const rp_aivat_hand& h = q.hands[r];  // read where it lies: every index into it is wave-uniform
    NaOut o;
    const uint32_t status = na_hand(t, p, h, lane, o);
    if (lane != 0u) return;
    const bool ok = status == RP_RECALL_OK;
    const float hero = ok ? o.hero : 0.0f, villain = ok ? o.villain : 0.0f, chance = ok ? o.chance : 0.0f;
    q.hero[r] = hero;
    q.villain[r] = villain;
    q.chance[r] = chance;
    q.total[r] = ok ? hero + villain + chance : 0.0f;
    if (q.n_action) q.n_action[r] = ok ? (uint8_t)o.n_action : (uint8_t)0;
    if (q.n_chance) q.n_chance[r] = ok ? (uint8_t)o.n_chance : (uint8_t)0;
    if (q.status) q.status[r] = (uint8_t)status;
}
static_assert(NA_BLOCK == 64u, "k_nl_aivat: one wavefront per hand, the deals of a chance node on its lanes");

}  // namespace rp

#endif
