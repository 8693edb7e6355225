// nlmc_translate.hpp — played hands to recalls: every play of an rp_aivat_hand becomes the edge Recall::history() gives it under one
// of the reference's three translations, and the hand becomes the rp_nlhe_recall the ranges, beliefs, worlds and re-solves read, with
// the key of its head (rp_nlhe_translate).  Reads no table: only the encoder's parameters, for the head's bucket.
//
// Reference: Recall::history / subgame (kicker/src/recall.rs:81-112), Game::translate (kicker/src/game.rs:778-811), Size::translate /
// translate_axis (kicker/src/size.rs:48-92), Lattice::bracket / snap / pharmonic / harmonic / phargmax
// (pokerkit/src/translate/lattice.rs:118-189), Witness::initial_with (kicker/src/witness.rs:77), NlheInfo::from((&Recall, Abstraction))
// (nlhe/src/info.rs:117-122).  The rules are stated in include/rp_mi355x.h above rp_nlhe_translate.
//
// One lane per hand, NX_BLOCK per workgroup, the game and the witness's counters (NaCounts, nlmc_aivat.hpp) in registers, as
// k_nl_match runs.  The records are indexed at run time on both sides (play j of the hand, edge n_edges of the recall), and a lane's
// record is 192 B in and 88 B out, so a lane working on its own record in global memory would move bytes and half-words at a stride
// of 192 B.  Instead the workgroup stages its records through LDS: it reads its NX_BLOCK hands as one contiguous run of 8-byte words
// (8 bytes is the alignment the record types give; consecutive lanes read consecutive words), each lane replays its hand out of LDS
// and appends to its recall in LDS, and the workgroup writes its recalls and play edges as contiguous runs again.  A record's LDS
// stride is an odd number of dwords (49 and 23), so that the lanes of a wavefront, each at the same offset of its own record, fall on
// different banks.  The edge of play j takes the place of the play's kind in the staged hand: the kind is read before the edge is
// known and never again, and the 48 bytes leave as play_edges.
#ifndef RP_NLMC_TRANSLATE_HPP
#define RP_NLMC_TRANSLATE_HPP

#include <cstddef>

#include "nlmc_aivat.hpp"

namespace rp {

#define NX_BLOCK 64u
#define NX_HAND_WORDS (sizeof(rp_aivat_hand) / 8u)    // 24 words of 8 bytes
#define NX_RECALL_WORDS (sizeof(rp_nlhe_recall) / 8u)  // 11
#define NX_HAND_STRIDE 49u                             // dwords per staged hand: 48 and one of padding
#define NX_RECALL_STRIDE 23u                           // dwords per staged recall: 22 and one of padding
static_assert(sizeof(rp_nlhe_translate_args) == 24, "rp_nlhe_translate_args is 24 bytes (INTEGRATION.md mirrors it)");
static_assert(sizeof(rp_aivat_hand) == 192 && sizeof(rp_nlhe_recall) == 88 && alignof(rp_aivat_hand) == 8 && alignof(rp_nlhe_recall) == 8,
              "k_nl_translate moves both records as 8-byte words");
static_assert(NX_HAND_STRIDE * 4u >= sizeof(rp_aivat_hand) && NX_RECALL_STRIDE * 4u >= sizeof(rp_nlhe_recall) && NX_HAND_STRIDE % 2u == 1u &&
                  NX_RECALL_STRIDE % 2u == 1u,
              "a staged record holds the record, at an odd dword stride");
static_assert(offsetof(rp_aivat_hand, kind) % 4u == 0 && RP_AIVAT_MAX_PLAYS % 4u == 0, "play_edges leave the staged hand as dwords");
static_assert(RP_AIVAT_MAX_PLAYS <= 255u && RP_NLHE_MAX_HISTORY <= 255u, "plays and edges are counted in a byte");

struct NxArgs {
    const rp_aivat_hand* hands;
    const uint8_t *pov, *upto;  // either may be NULL
    uint64_t hash;              // rp_node_hash_step(seed, 3)
    uint64_t first_id;          // the id of hand 0 of this launch
    uint32_t n, kind;
    rp_nlhe_recall* recalls;    // every output may be NULL
    uint8_t* play_edges;
    uint64_t* past;
    uint32_t* present;
    uint64_t* choices;
    uint8_t *n_choices, *status;
};

// Game::translate on the game before the play (`v` its view): the edge of action `a` at `depth` under rp_translation_kind `kind`,
// `u` the hand's uniform draw for this play (read by RP_TRANSLATE_HARMONIC alone).  f64 throughout, one rounding per operation.
__device__ __forceinline__ uint32_t nl_translate(const NlView& v, const NlAction& a, int depth, uint32_t kind, double u) {
    switch (a.kind) {
        case NA_FOLD: return NE_FOLD;
        case NA_CHECK: return NE_CHECK;
        case NA_DRAW: return NE_DRAW;
        case NA_CALL: case NA_BLIND: return NE_CALL;
        case NA_SHOVE: return NE_SHOVE;
    }
    uint32_t grid[6] = {0, 0, 0, 0, 0, 0};
    const int n = nl_raise_edges(v.street, depth, grid);
    if (n == 0) return NE_SHOVE;  // past MAX_RAISE_REPEATS the cell is empty
    const bool opening = v.street == 0 && depth == 0;
    const double x = opening ? (double)a.chips / (double)NL_BBLIND : (double)a.chips / (double)v.pot;
    // one pass over the cell's anchors, ascending: the nearest (the first of equally near ones), the last one below x and the first
    // one not below it (partition_point), the first and the last
    uint32_t near_e = 0, lo_e = 0, hi_e = 0, first_e = 0, last_e = 0;
    double near_gap = 0.0, lo_s = 0.0, hi_s = 0.0, first_s = 0.0, last_s = 0.0;
    bool have_hi = false;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        if (i >= n) continue;
        const uint32_t e = grid[i];
        const double s = opening ? (double)NL_OPENS[e - NE_OPEN0] : (double)NL_RAISES[e - NE_RAISE0][0] / (double)NL_RAISES[e - NE_RAISE0][1];
        const double gap = fabs(s - x);
        if (i == 0 || gap < near_gap) near_e = e, near_gap = gap;
        if (i == 0) first_e = e, first_s = s;
        last_e = e, last_s = s;
        if (s < x) lo_e = e, lo_s = s;
        else if (!have_hi) hi_e = e, hi_s = s, have_hi = true;
    }
    if (kind == (uint32_t)RP_TRANSLATE_SNAP) return near_e;
    if (x <= first_s) return first_e;  // the bracket is clamped
    if (x >= last_s) return last_e;
    const double p = ((hi_s - x) * (1.0 + lo_s)) / ((hi_s - lo_s) * (1.0 + x));  // pharmonic: the probability of the lower anchor
    const bool lower = kind == (uint32_t)RP_TRANSLATE_HARMONIC ? u < p : p >= 0.5;
    return lower ? lo_e : hi_e;
}

// a lane's staged records
struct NxStaged {
    const uint8_t* hand;  // the rp_aivat_hand's bytes, 4-byte aligned
    uint8_t* hand_kind;   // its kind[], which the plays' edges overwrite
    uint8_t* recall;      // the rp_nlhe_recall's bytes, 4-byte aligned
    __device__ __forceinline__ uint64_t hand_u64(uint32_t at) const {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(hand + at);
        return (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    }
    __device__ __forceinline__ int16_t hand_i16(uint32_t at) const { return *reinterpret_cast<const int16_t*>(hand + at); }
    __device__ __forceinline__ void recall_u64(uint32_t at, uint64_t x) const {
        uint32_t* w = reinterpret_cast<uint32_t*>(recall + at);
        w[0] = (uint32_t)x;
        w[1] = (uint32_t)(x >> 32);
    }
};

struct NxKey {
    uint64_t past, choices;
    uint32_t present, n_choices;
};

// one hand, statement by statement of the contract; returns its status.  The recall's edges and the plays' edges are written as the
// replay goes; the recall's other fields and the key only where the hand is answered
__device__ __forceinline__ uint32_t nx_hand(const NlParams& p, const NxArgs& q, uint32_t i, const NxStaged& s, NxKey& key) {
    const uint32_t n_plays = s.hand[offsetof(rp_aivat_hand, n_plays)], seat = s.hand[offsetof(rp_aivat_hand, seat)];
    const uint32_t dealer = s.hand[offsetof(rp_aivat_hand, dealer)];
    const uint32_t pov = q.pov ? q.pov[i] : seat, upto = q.upto ? q.upto[i] : n_plays;
    if (n_plays > RP_AIVAT_MAX_PLAYS || upto > n_plays) return RP_RECALL_LENGTH;
    const int16_t stacks[2] = {s.hand_i16(offsetof(rp_aivat_hand, stacks)), s.hand_i16(offsetof(rp_aivat_hand, stacks) + 2u)};
    uint32_t st = nrp_check_seats(seat, dealer, pov > 1u ? 1u : 0u, stacks);
    if (st != RP_RECALL_OK) return st;
    const uint64_t hole[2] = {s.hand_u64(offsetof(rp_aivat_hand, hole)), s.hand_u64(offsetof(rp_aivat_hand, hole) + 8u)};
    const uint64_t draws[3] = {s.hand_u64(offsetof(rp_aivat_hand, draws)), s.hand_u64(offsetof(rp_aivat_hand, draws) + 8u),
                               s.hand_u64(offsetof(rp_aivat_hand, draws) + 16u)};
    uint64_t gone = 0;
#pragma unroll
    for (uint32_t k = 0; k < 2u; ++k)  // the other seat's hole may be unknown
        if ((k == pov || hole[k] != 0) && (st = nrp_check_hole(hole[k], &gone)) != RP_RECALL_OK) return st;
    if ((st = nrp_check_draws(draws, gone)) != RP_RECALL_OK) return st;
    for (uint32_t j = 0; j < n_plays; ++j)
        if (s.hand_kind[j] < (uint8_t)RP_PLAY_FOLD || s.hand_kind[j] > (uint8_t)RP_PLAY_SHOVE) return RP_RECALL_EDGE;

    G2 g;
    nrp_from_start(g, dealer, stacks, hole[0], hole[1]);
    NaCounts w;
    w.run.clear();
    w.street_begins();
    const uint64_t th = rp_node_hash_tree(q.hash, q.first_id + i);
    uint32_t n_edges = 0, streets = 0;
    uint8_t* edges = s.recall + offsetof(rp_nlhe_recall, edges);
    // the pending streets; `need`: a street the hand does not carry refuses it.  At most three rounds: a deal moves to the next street
    auto deal = [&](bool need) -> uint32_t {
        while (g.turn() == NT_CHANCE) {
            const int street = g.street();
            const uint64_t d = street == 0 ? draws[0] : (street == 1 ? draws[1] : draws[2]);
            if (d == 0) return need ? (uint32_t)RP_RECALL_DRAW : (uint32_t)RP_RECALL_OK;
            if (n_edges >= RP_NLHE_MAX_HISTORY) return RP_RECALL_LENGTH;
            g.force_act(NlAction{NA_DRAW, 0, d});
            w.dealt();
            edges[n_edges++] = (uint8_t)NE_DRAW;
            streets = (uint32_t)street + 1u;
        }
        return RP_RECALL_OK;
    };
    for (uint32_t j = 0; j < upto; ++j) {
        if ((st = deal(true)) != RP_RECALL_OK) return st;
        if (g.turn() == NT_TERMINAL) return RP_RECALL_ILLEGAL;
        const int kind = (int)s.hand_kind[j];
        const NlAction act{kind, (kind == NA_FOLD || kind == NA_CHECK) ? 0 : (int)s.hand_i16(offsetof(rp_aivat_hand, chips) + 2u * j), 0};
        if (!g.allowed(act)) return RP_RECALL_ILLEGAL;
        const double u = (double)(rp_node_hash_key(th, j) >> 11) * 0x1.0p-53;
        const uint32_t e = nl_translate(nl_view(g), act, (int)w.run.aggr, q.kind, u);
        if (n_edges >= RP_NLHE_MAX_HISTORY) return RP_RECALL_LENGTH;
        w.note_edge(act, e);
        edges[n_edges++] = (uint8_t)e;
        s.hand_kind[j] = (uint8_t)e;
        g.force_act(act);
    }
    if ((st = deal(false)) != RP_RECALL_OK) return st;

    // the head's key
    const int turn = g.turn();
    uint32_t err = 0;
    key.present = nl_bucket(p, g.street(), pov ? hole[1] : hole[0], g.board, &err);
    if (err) return RP_RECALL_LOOKUP;
    key.past = w.sub;
    key.choices = 0;
    key.n_choices = turn < 0 ? 0u : nl_choices_path(nl_view(g), (int)w.sub_aggr, &key.choices);
    // the recall's fixed fields
    s.recall_u64(offsetof(rp_nlhe_recall, hole), pov ? hole[1] : hole[0]);
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k) s.recall_u64(offsetof(rp_nlhe_recall, draws) + 8u * k, k < streets ? draws[k] : 0ull);
    *reinterpret_cast<int16_t*>(s.recall + offsetof(rp_nlhe_recall, stacks)) = stacks[0];
    *reinterpret_cast<int16_t*>(s.recall + offsetof(rp_nlhe_recall, stacks) + 2u) = stacks[1];
    s.recall[offsetof(rp_nlhe_recall, pov)] = (uint8_t)pov;
    s.recall[offsetof(rp_nlhe_recall, dealer)] = (uint8_t)dealer;
    s.recall[offsetof(rp_nlhe_recall, n_edges)] = (uint8_t)n_edges;
    for (uint32_t j = upto; j < RP_AIVAT_MAX_PLAYS; ++j) s.hand_kind[j] = 0;  // play_edges past upto
    return RP_RECALL_OK;
}

__global__ __launch_bounds__(NX_BLOCK) void k_nl_translate(NlParams p, NxArgs q) {
    __shared__ uint32_t hands[NX_BLOCK * NX_HAND_STRIDE];
    __shared__ uint32_t recalls[NX_BLOCK * NX_RECALL_STRIDE];
    const uint32_t lane = threadIdx.x, base = blockIdx.x * NX_BLOCK;  // base < q.n: the grid is ceil(n / NX_BLOCK)
    const uint32_t m = min(NX_BLOCK, q.n - base);
    // in: the workgroup's hands as one run of 8-byte words, every load issued before the first is waited for
    const uint64_t* src = reinterpret_cast<const uint64_t*>(q.hands + base);
    uint64_t word[NX_HAND_WORDS];
#pragma unroll
    for (uint32_t k = 0; k < NX_HAND_WORDS; ++k) {
        const uint32_t at = k * NX_BLOCK + lane;
        word[k] = at < m * NX_HAND_WORDS ? src[at] : 0ull;
    }
#pragma unroll
    for (uint32_t k = 0; k < NX_HAND_WORDS; ++k) {
        const uint32_t at = k * NX_BLOCK + lane;
        const uint32_t to = (at / NX_HAND_WORDS) * NX_HAND_STRIDE + 2u * (at % NX_HAND_WORDS);
        hands[to] = (uint32_t)word[k];
        hands[to + 1u] = (uint32_t)(word[k] >> 32);
    }
    for (uint32_t k = 0; k < NX_RECALL_STRIDE; ++k) recalls[lane * NX_RECALL_STRIDE + k] = 0u;
    __syncthreads();
    if (lane < m) {
        const uint32_t i = base + lane;
        uint32_t* hand = hands + lane * NX_HAND_STRIDE;
        uint32_t* recall = recalls + lane * NX_RECALL_STRIDE;
        const NxStaged s{reinterpret_cast<const uint8_t*>(hand), reinterpret_cast<uint8_t*>(hand) + offsetof(rp_aivat_hand, kind),
                         reinterpret_cast<uint8_t*>(recall)};
        NxKey key{0ull, 0ull, 0u, 0u};
        const uint32_t status = nx_hand(p, q, i, s, key);
        if (status != RP_RECALL_OK) {  // a refused hand: zero outputs
            for (uint32_t k = 0; k < NX_RECALL_STRIDE; ++k) recall[k] = 0u;
            for (uint32_t k = 0; k < RP_AIVAT_MAX_PLAYS / 4u; ++k) hand[offsetof(rp_aivat_hand, kind) / 4u + k] = 0u;
            key = NxKey{0ull, 0ull, 0u, 0u};
        }
        if (q.past) q.past[i] = key.past;
        if (q.present) q.present[i] = key.present;
        if (q.choices) q.choices[i] = key.choices;
        if (q.n_choices) q.n_choices[i] = (uint8_t)key.n_choices;
        if (q.status) q.status[i] = (uint8_t)status;
    }
    __syncthreads();
    // out: the workgroup's recalls as one run of 8-byte words, its play edges as one run of dwords (of bytes where the caller's
    // array is not 4-byte aligned)
    if (q.recalls) {
        uint64_t* dst = reinterpret_cast<uint64_t*>(q.recalls + base);
        for (uint32_t at = lane; at < m * NX_RECALL_WORDS; at += NX_BLOCK) {
            const uint32_t from = (at / NX_RECALL_WORDS) * NX_RECALL_STRIDE + 2u * (at % NX_RECALL_WORDS);
            dst[at] = (uint64_t)recalls[from] | ((uint64_t)recalls[from + 1u] << 32);
        }
    }
    if (q.play_edges) {
        uint8_t* dst = q.play_edges + (size_t)base * RP_AIVAT_MAX_PLAYS;
        constexpr uint32_t PER = RP_AIVAT_MAX_PLAYS / 4u, KIND = offsetof(rp_aivat_hand, kind) / 4u;
        if ((reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
            for (uint32_t at = lane; at < m * PER; at += NX_BLOCK)
                reinterpret_cast<uint32_t*>(dst)[at] = hands[(at / PER) * NX_HAND_STRIDE + KIND + at % PER];
        } else {
            const uint8_t* bytes = reinterpret_cast<const uint8_t*>(hands);
            for (uint32_t at = lane; at < m * RP_AIVAT_MAX_PLAYS; at += NX_BLOCK)
                dst[at] = bytes[(at / RP_AIVAT_MAX_PLAYS) * NX_HAND_STRIDE * 4u + KIND * 4u + at % RP_AIVAT_MAX_PLAYS];
        }
    }
}

}  // namespace rp

#endif
