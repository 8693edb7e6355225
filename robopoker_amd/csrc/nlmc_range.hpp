// nlmc_range.hpp — ranges from the NLHE blueprint: the reach of every hole one seat could hold, given what the other seat has seen
// (rp_nlhe_reaches), and its projection onto abstraction buckets (rp_nlhe_opponent_range).  Read-only, like nlmc_query.hpp.
//
// Reference: Nlhe::reach / opponent_reaches / opponent_range / opponent_observations / signalled_observations / signalled_reaches /
// normalize (nlhe/src/solver.rs:137-260) over CfrEncoder::replay (mccfr/src/strategy/encoder.rs:72-84), NlheGame::apply
// (nlhe/src/game.rs:50-70), NlheEncoder::resume (nlhe/src/encoder.rs:59-67), NlheInfo::from((Path, Abstraction, Path))
// (nlhe/src/info.rs:125-139), Path::from_iter (kicker/src/path.rs:169-181), Posterior::add (mccfr/src/strategy/posterior.rs:47-50).
// The rules are stated in include/rp_mi355x.h above rp_nlhe_reaches.
//
// The factorisation.  The reference replays one perfect-information game per candidate hole.  With the board cards given, nothing
// PUBLIC in that replay depends on the candidate: turns, chips, the 12-edge path, `past` and `choices` of every node are the same
// for all of them, and the only thing that differs is the bucket of (candidate, board of the node's street) — at most four
// values.  So one workgroup answers one recall in three phases:
//   A  lane 0 validates the recall and replays it ONCE with the engine (nlhe_engine.hpp), leaving in LDS the list of the subject's
//      nodes (past, choices, street, slot of the edge taken or NR_NONE), the board of every street and the cards still free;
//   B  the lanes stride over the candidates.  Candidate j is the j-th pair of free cards by (high card, low card), which is
//      HandIterator's order (ascending mask) with the taken cards already left out: no compaction pass.  Per candidate: one
//      nl_bucket per street that has a subject node, then per node the home slot and the row's weights loaded together, nlq_find,
//      the averaged fold over all nch slots, ONE divide (the slot of the edge taken) and the multiply;
//   C  reaches: the total is one lane's f32 fold in candidate order, then every lane divides its own entries;
//      range:   lane b owns bucket b and scans (bucket, reach) of all candidates in order — every lane reads the same LDS address
//               in the same iteration (a broadcast), and each sum is the reference's left fold.
// No atomic and no store touches the table; nlq_find runs divergent and holds no wave collective.
#ifndef RP_NLMC_RANGE_HPP
#define RP_NLMC_RANGE_HPP

#include "nlmc_query.hpp"
#include "nlmc_replay.hpp"

namespace rp {

#define NR_BLOCK 256u
#define NR_NONE 0xffu  // the edge taken is not among the node's choices: factor 0
static_assert(RP_NLHE_MAX_HOLES == 52u * 51u / 2u, "two cards of 52");
static_assert(sizeof(rp_nlhe_recall) == 88, "rp_nlhe_recall is 88 bytes (INTEGRATION.md mirrors it)");

struct NrArgs {
    const rp_nlhe_recall* recalls;
    int kind, normalize;
    // reaches (mass == NULL): count [n], holes [n][1326] (may be NULL), reach [n][1326]
    uint32_t* count;
    uint64_t* holes;
    float* reach;
    // range (mass != NULL): mass [n][256], seen [n][256]
    float* mass;
    uint8_t* seen;
    uint8_t* status;  // may be NULL
};

struct NrNode {
    uint64_t past, choices;
    uint8_t street, slot, nch, pad;
};

// Phase A: validation and the public replay.  Returns the status; on RP_RECALL_OK the node list, boards and free cards are set.
struct NrPublic {
    NrNode node[RP_NLHE_MAX_HISTORY];
    uint64_t board[4];   // the board a node of street s sees: draws[0 .. s)
    uint64_t head;       // the board the candidates are disjoint from, and the range's buckets are taken on
    uint32_t n_nodes, streets, head_street, n_free, count, status, lookup_miss;
    float total;
    uint8_t free_card[52];
};

__device__ __forceinline__ uint32_t nr_replay(const rp_nlhe_recall& rc, int kind, NrPublic& pub) {
    if (rc.n_edges > RP_NLHE_MAX_HISTORY) return RP_RECALL_LENGTH;
    // the checks, from_start, the 12-edge path and apply are nlmc_replay.hpp's: one definition for every query that replays
    uint32_t st = nrp_check_seats(rc.pov, rc.dealer, rc.reserved, rc.stacks);
    if (st != RP_RECALL_OK) return st;
    uint64_t gone = 0;
    if ((st = nrp_check_hole(rc.hole, &gone)) != RP_RECALL_OK) return st;
    if ((st = nrp_check_draws(rc.draws, gone)) != RP_RECALL_OK) return st;
    uint32_t n_draw_edges = 0;
    if ((st = nrp_check_edges(rc.edges, rc.n_edges, &n_draw_edges)) != RP_RECALL_OK) return st;
    const int subject = kind == (int)RP_REACH_OPPONENT ? 1 - (int)rc.pov : (int)rc.pov;

    // the seats hold no cards: nothing public depends on them, and the recall's own cards were checked against each other above
    G2 g;
    nrp_from_start(g, rc.dealer, rc.stacks, 0ull, 0ull);

    // the first 12 edges as resume() sees them: the trailing choice edges and their aggression
    NrpPath path;
    path.clear();
    uint32_t n_nodes = 0, streets = 0;
    for (uint32_t i = 0; i < rc.n_edges; ++i) {
        const uint32_t e = rc.edges[i];
        if (g.turn() == subject) {
            const NlView v = nl_view(g);
            uint64_t choices;
            const uint32_t nch = nl_choices_path(v, (int)path.aggr, &choices);
            uint32_t slot = NR_NONE;
            for (uint32_t a = 0; a < nch; ++a)
                if (((choices >> (5u * a)) & 31ull) == e) slot = a;
            NrNode& nd = pub.node[n_nodes++];
            nd.past = path.tail;
            nd.choices = choices;
            nd.street = (uint8_t)v.street;
            nd.slot = (uint8_t)slot;
            nd.nch = (uint8_t)nch;
            nd.pad = 0;
            streets |= 1u << v.street;
        }
        path.push(e);
        if ((st = nrp_apply(g, e, rc.draws)) != RP_RECALL_OK) return st;
    }
    // the board: the streets the history's Draw edges dealt, and any the replay dealt on its own
    const uint32_t dealt = max(min(n_draw_edges, 3u), (uint32_t)g.street());
    uint64_t b = 0;
    pub.board[0] = 0;
    for (uint32_t s = 0; s < 3u; ++s) {
        if (s < dealt) {
            if (rc.draws[s] == 0) return RP_RECALL_DRAW;
            b |= rc.draws[s];
        }
        pub.board[s + 1] = b;  // for s >= dealt: never read (no node of that street)
    }
    pub.head = pub.board[dealt];
    pub.head_street = dealt;
    pub.n_nodes = n_nodes;
    pub.streets = streets;
    const uint64_t taken = pub.head | (kind == (int)RP_REACH_OPPONENT ? rc.hole : 0ull);
    uint32_t n_free = 0;
    for (uint32_t c = 0; c < 52u; ++c)
        if (!((taken >> c) & 1ull)) pub.free_card[n_free++] = (uint8_t)c;
    pub.n_free = n_free;
    pub.count = n_free * (n_free - 1u) / 2u;
    return RP_RECALL_OK;
}

// candidate j -> (hi, lo) with j = hi (hi - 1) / 2 + lo, lo < hi: the pairs of free cards by high card, then low card
__device__ __forceinline__ void nr_pair(uint32_t j, uint32_t* hi, uint32_t* lo) {
    uint32_t h = (uint32_t)((1.0f + sqrtf(1.0f + 8.0f * (float)j)) * 0.5f);
    while (h * (h - 1u) / 2u > j) h -= 1u;
    while ((h + 1u) * h / 2u <= j) h += 1u;
    *hi = h;
    *lo = j - h * (h - 1u) / 2u;
}

// one factor: averaged_distribution(info).density(edge) for the infoset (nd.past, present, nd.choices) — the fold of
// policy_distribution<>(RP_DIST_AVERAGED) over all nch slots, and the one quotient that is asked for
__device__ __forceinline__ float nr_factor(const NlTable& t, const NrNode& nd, uint32_t present) {
    float w[NLMC_A];
    const bool found = nlq_row_weights(t, nd.past, nd.choices, present, w);
    float sum = 0.0f, mine = 0.0f;
#pragma unroll
    for (uint32_t a = 0; a < NLMC_A; ++a) {
        const float v = rp_maxf(found ? w[a] : 0.0f, RP_EPSILON);
        if (a < nd.nch) sum += v;
        mine = a == nd.slot ? v : mine;
    }
    return nd.slot == NR_NONE ? 0.0f : mine / sum;
}

// Phase B: the lanes stride over the candidates of a recall whose replay succeeded.  s_reach[j] = the reach of candidate j; with
// `range`, s_bucket[j] = its bucket on the head board, otherwise its mask goes to holes_row (may be NULL).  *err: nl_bucket's.
__device__ __forceinline__ void nr_candidates(const NlTable& t, const NlParams& p, const NrPublic& pub, bool range, float* s_reach, uint8_t* s_bucket,
                                              uint64_t* holes_row, uint32_t tid, uint32_t* err) {
    const uint32_t count = pub.count, streets = pub.streets, n_nodes = pub.n_nodes;
    for (uint32_t j = tid; j < count; j += NR_BLOCK) {
        uint32_t hi, lo;
        nr_pair(j, &hi, &lo);
        const uint64_t hole = (1ull << pub.free_card[hi]) | (1ull << pub.free_card[lo]);
        uint32_t bucket[4] = {0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if ((streets >> s) & 1u) bucket[s] = nl_bucket(p, s, hole, pub.board[s], err);
        float reach = 1.0f;
        for (uint32_t k = 0; k < n_nodes; ++k) {
            const NrNode nd = pub.node[k];
            const uint32_t present = nd.street == 0 ? bucket[0] : (nd.street == 1 ? bucket[1] : (nd.street == 2 ? bucket[2] : bucket[3]));
            reach *= nr_factor(t, nd, present);
        }
        s_reach[j] = reach;
        if (range) s_bucket[j] = (uint8_t)nl_bucket(p, (int)pub.head_street, hole, pub.head, err);
        else if (holes_row) holes_row[j] = hole;
    }
}

// Phases A and B of one recall, by the whole workgroup (it holds two barriers): returns the recall's status, the same in every lane;
// on RP_RECALL_OK pub, s_reach and (range) s_bucket are set for pub.count candidates.
__device__ __forceinline__ uint32_t nr_recall(const NlTable& t, const NlParams& p, const rp_nlhe_recall& rc, int kind, bool range, NrPublic& pub,
                                              float* s_reach, uint8_t* s_bucket, uint64_t* holes_row, uint32_t tid) {
    if (tid == 0) {
        pub.status = nr_replay(rc, kind, pub);
        pub.lookup_miss = 0;
    }
    __syncthreads();
    uint32_t err = 0;
    if (pub.status == RP_RECALL_OK) nr_candidates(t, p, pub, range, s_reach, s_bucket, holes_row, tid, &err);
    // a hole the encoder's tables do not know (the reference panics): the recall is answered as malformed.  Every lane that saw
    // one stores the same value; the barrier orders the stores before the read
    if (err) pub.lookup_miss = 1;
    __syncthreads();
    return pub.status != RP_RECALL_OK ? pub.status : (pub.lookup_miss ? (uint32_t)RP_RECALL_LOOKUP : (uint32_t)RP_RECALL_OK);
}

// Phase C of a range: lane b = bucket b, Posterior::add in candidate order — every lane reads the same LDS address in the same
// iteration (a broadcast), and each sum is the reference's left fold
__device__ __forceinline__ void nr_bucket_mass(const float* s_reach, const uint8_t* s_bucket, uint32_t count, uint32_t tid, float* mass, uint32_t* seen) {
    float m = 0.0f;
    uint32_t any = 0;
    for (uint32_t j = 0; j < count; ++j) {
        const bool mine = s_bucket[j] == tid;
        m = mine ? m + s_reach[j] : m;
        any |= mine ? 1u : 0u;
    }
    *mass = m;
    *seen = any;
}

__global__ __launch_bounds__(NR_BLOCK) void k_nl_range(NlTable t, NlParams p, NrArgs q) {
    __shared__ NrPublic pub;
    __shared__ float s_reach[RP_NLHE_MAX_HOLES];
    __shared__ uint8_t s_bucket[RP_NLHE_MAX_HOLES];
    const uint32_t r = blockIdx.x, tid = threadIdx.x;
    const bool range = q.mass != nullptr;

    const uint32_t status = nr_recall(t, p, q.recalls[r], q.kind, range, pub, s_reach, s_bucket,
                                      q.holes ? q.holes + (size_t)r * RP_NLHE_MAX_HOLES : nullptr, tid);
    const uint32_t count = status == RP_RECALL_OK ? pub.count : 0u;
    if (tid == 0 && q.status) q.status[r] = (uint8_t)status;

    if (range) {
        float m;
        uint32_t any;
        nr_bucket_mass(s_reach, s_bucket, count, tid, &m, &any);
        q.mass[(size_t)r * 256u + tid] = m;
        q.seen[(size_t)r * 256u + tid] = (uint8_t)any;
        return;
    }
    if (q.normalize) {
        if (tid == 0) {
            float total = 0.0f;
            for (uint32_t j = 0; j < count; ++j) total += s_reach[j];
            pub.total = total;
        }
        __syncthreads();
    }
    const float total = q.normalize ? pub.total : 0.0f;
    if (tid == 0) q.count[r] = count;
    for (uint32_t j = tid; j < RP_NLHE_MAX_HOLES; j += NR_BLOCK) {
        float v = j < count ? s_reach[j] : 0.0f;
        if (j < count && total != 0.0f) v = v / total;  // a zero total (either sign) leaves the stream untouched
        q.reach[(size_t)r * RP_NLHE_MAX_HOLES + j] = v;
        if (q.holes && j >= count) q.holes[(size_t)r * RP_NLHE_MAX_HOLES + j] = 0ull;
    }
}
static_assert(NR_BLOCK == 256u, "k_nl_range: one lane per bucket of the range");

}  // namespace rp

#endif
