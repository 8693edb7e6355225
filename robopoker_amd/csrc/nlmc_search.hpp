// nlmc_search.hpp — matches in which a seat may be a search agent (rp_nlhe_search_match): Agent<World<Blueprint>> and its Dirac form
// re-solve every postflop decision with the safe subgame solver and play the blend of its harvest and the blueprint.  Read-only on
// both tables, like nlmc_match.hpp, whose loop body (nm_play) this file runs unchanged.
//
// Reference: Brain::distrib / World::solve / Solved::run, blend (parlor/src/players/brain.rs:45-71, world.rs, solved.rs:133-152),
// Nlhe::adapt_safe / adapt_full (nlhe/src/solver.rs:103-136).  The rules are stated in include/rp_mi355x.h above rp_nlhe_search_match.
//
// k_nl_match plays a whole hand in registers and cannot stop for a workgroup-sized solve, so a batch is played in ROUNDS over hands
// that live in device memory (NsHand):
//   k_nl_search_advance  one lane per hand, NM_BLOCK per workgroup, divergent, no wave collective and no barrier.  A lane loads its
//                        hand, runs nm_play until the hand ends or a search seat meets a postflop decision, and stores it.  At such a
//                        decision it writes the recall, the entry and the solve's id into the hand's request and parks; the next
//                        round the same decision is taken up again (the blueprint row is probed a second time — one probe against a
//                        solve), the result of the solve is consumed — fallback, blend, trace — and the hand goes on.
//   k_nl_search_compact  one workgroup per chunk: an exclusive scan over the hands' parked flags (thread-local over 4 hands, then a
//                        Hillis-Steele scan of the 256 partial sums in LDS) gives every parked hand its place in a dense request list,
//                        seat 0's requests first, then seat 1's — each list is solved against its own seat's table.  The requests are
//                        copied there, the hand remembers its place, and the two counts are posted to pinned host memory.
//   k_nl_world, k_nl_subgame on the dense lists: the public entry points' kernels, the subgame kernel with the per-solve id array.
// Nothing a hand outputs depends on the order of the dense list: a solve is identified by its explicit id alone.
#ifndef RP_NLMC_SEARCH_HPP
#define RP_NLMC_SEARCH_HPP

#include "nlmc_match.hpp"
#include "nlmc_subgame.hpp"

namespace rp {

#define NSM_CHUNK 1024u  // hands in flight: what the per-hand state, the request lists and the solves' overflow rows are sized for
#define NSM_SCAN 256u    // k_nl_search_compact's workgroup: NSM_CHUNK / NSM_SCAN hands per thread
static_assert(NSM_CHUNK % NSM_SCAN == 0 && NSM_CHUNK <= 0xffffu, "the scan packs two 16-bit counts into a word");
static_assert(sizeof(rp_nlhe_search_args) == 72 && sizeof(rp_nlhe_search_step) == 352, "INTEGRATION.md mirrors them");
static_assert(RP_NLHE_SEARCH_MAX_SOLVES <= 255u, "solves of a hand are counted in a byte's range");

struct NsRequest {  // what a parked hand asks for
    rp_nlhe_recall recall;
    rp_nlhe_frontier entry;
    uint64_t solve_id;
    int8_t origin;
};

struct NsHand {  // one hand in device memory between two rounds
    NmHand core;
    uint32_t n_edges;   // history()'s length, past RP_NLHE_MAX_HISTORY counted and not kept
    uint32_t searched, unsolved, solves, n_steps;
    uint32_t parked;    // 0: not waiting; 1 + s: seat s waits for its solve
    uint32_t place;     // ... which is the place-th of the round's dense list
    uint32_t done;
    uint8_t edges[RP_NLHE_MAX_HISTORY];
    NsRequest request;
};

struct NsmArgs {
    NmArgs match;
    uint8_t search[2];
    uint8_t origin_mode;
    uint32_t visit_threshold, steps_cap;
    uint32_t first;  // the chunk's first round: every hand is dealt
    NsHand* hands;   // [n]
    uint8_t *searched, *unsolved;  // may be NULL
    rp_nlhe_search_step* steps;    // [n][steps_cap], may be NULL
    // the dense lists of the round before
    const rp_nlhe_subgame_result* results;
    const uint8_t* belief_status;
};

// Solved::blend (solved.rs:133-152): per slot, f32, one rounding per operation; the total folds in Edge's derived order
__device__ __forceinline__ void nsm_blend(const rp_nlhe_subgame_result& r, const float* bp, uint64_t choices, uint32_t nch, uint32_t visit_threshold,
                                          float* p) {
    float raw[NLMC_A];
    uint32_t rank[NLMC_A];
    const float th = (float)visit_threshold;
#pragma unroll
    for (uint32_t a = 0; a < NLMC_A; ++a) {
        const float v = (float)r.visits[a];
        const float w = v / (v + th);
        raw[a] = w * r.refined[a] + (1.0f - w) * bp[a];
        rank[a] = a < nch ? nm_rank((uint32_t)(choices >> (5u * a)) & 31u) : 32u + a;
    }
    float total = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < NLMC_A; ++k) {  // the k-th edge in Edge order
#pragma unroll
        for (uint32_t a = 0; a < NLMC_A; ++a) {
            uint32_t below = 0;
#pragma unroll
            for (uint32_t b = 0; b < NLMC_A; ++b) below += rank[b] < rank[a] ? 1u : 0u;
            total = (a < nch && below == k) ? total + raw[a] : total;
        }
    }
    total = rp_maxf(total, RP_EPSILON);
#pragma unroll
    for (uint32_t a = 0; a < NLMC_A; ++a) p[a] = a < nch ? raw[a] / total : 0.0f;
}

// the search seat's part of nm_play, one per lane; the counters travel in registers, the history and the request stay in device memory
struct NsmSearch {
    const NsmArgs* q;
    NsHand* x;
    rp_nlhe_search_step* steps;  // this hand's, or NULL
    uint64_t hand_id;
    uint32_t n_edges, searched, unsolved, solves, n_steps, parked;
    bool traced;  // the decision being taken has a step in the trace: chose() completes it

    __device__ __forceinline__ bool seat(int turn) const { return q->search[turn ? 1 : 0] != 0u; }
    __device__ __forceinline__ void edge(uint32_t e) {
        if (n_edges < RP_NLHE_MAX_HISTORY) x->edges[n_edges] = (uint8_t)e;
        n_edges += 1u;
    }
    __device__ __forceinline__ rp_nlhe_search_step* step_begin(int turn, uint32_t decision, uint32_t code, const float* bp, const float* p) {
        traced = steps != nullptr && n_steps < q->steps_cap;
        n_steps += 1u;
        unsolved = min(unsolved + (code ? 1u : 0u), 255u);
        if (!traced) return nullptr;
        rp_nlhe_search_step* s = steps + (n_steps - 1u);  // zero since the hand began
#pragma unroll
        for (uint32_t a = 0; a < NLMC_A; ++a) {
            s->bp[a] = bp[a];
            s->p[a] = p[a];
        }
        s->seat = (uint8_t)turn;
        s->fallback = (uint8_t)code;
        s->decision = decision;
        return s;
    }
    __device__ __forceinline__ void chose(uint32_t e) {
        if (traced) steps[n_steps - 1u].edge = (uint8_t)e;
        traced = false;
    }
    // false: the hand parks with its request written
    __device__ __forceinline__ bool decide(const NmHand& h, int turn, int street, uint64_t choices, uint32_t nch, uint32_t present, float* dist) {
        const uint64_t solve_id = hand_id * 256ull + (uint64_t)(h.decision & 255u);  // wrapping
        if (!parked) {
            searched = min(searched + 1u, 255u);
            const uint32_t code = n_edges > RP_NLHE_MAX_HISTORY ? (uint32_t)RP_SEARCH_FALLBACK_LENGTH
                                  : solves >= RP_NLHE_SEARCH_MAX_SOLVES ? (uint32_t)RP_SEARCH_FALLBACK_CAP : 0u;
            if (code) {  // no solve is asked for: the blueprint's policy
                rp_nlhe_search_step* s = step_begin(turn, h.decision, code, dist, dist);
                if (s) s->solve_id = solve_id;
                return true;
            }
            NsRequest& r = x->request;
            const uint64_t hole = turn ? h.hole1 : h.hole0;
            const uint64_t draws[3] = {h.streets > 0u ? h.flop : 0ull, h.streets > 1u ? h.turn_card : 0ull, h.streets > 2u ? h.river : 0ull};
            r.recall.hole = hole;
            r.entry.holes[0] = turn ? 0ull : hole;
            r.entry.holes[1] = turn ? hole : 0ull;
#pragma unroll
            for (uint32_t s = 0; s < 3u; ++s) r.recall.draws[s] = r.entry.draws[s] = draws[s];
#pragma unroll
            for (uint32_t s = 0; s < 2u; ++s) r.recall.stacks[s] = r.entry.stacks[s] = q->match.stacks[s];
            r.recall.pov = r.entry.internal = (uint8_t)turn;
            r.recall.dealer = r.entry.dealer = (uint8_t)h.dealer;
            r.recall.n_edges = r.entry.n_edges = (uint8_t)n_edges;
            r.recall.reserved = 0;
            r.entry.n_prefix = (uint8_t)h.w.sub_len;  // subgame(): the trailing choice edges, first 12
            for (uint32_t k = 0; k < RP_NLHE_MAX_HISTORY; ++k) r.recall.edges[k] = r.entry.edges[k] = k < n_edges ? x->edges[k] : (uint8_t)0;
#pragma unroll
            for (uint32_t k = 0; k < RP_NLHE_MAX_PREFIX; ++k) r.entry.prefix[k] = k < h.w.sub_len ? (uint8_t)((h.w.sub >> (5u * k)) & 31ull) : (uint8_t)0;
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) r.entry.reserved[k] = 0;
            r.solve_id = solve_id;
            r.origin = q->origin_mode ? (int8_t)(street - 1) : (int8_t)RP_NLHE_SUBGAME_ORIGIN_NONE;
            solves += 1u;
            parked = 1u + (uint32_t)(turn ? 1 : 0);
            // The hand as it stands at this decision: nothing of the decision is consumed.  KEEP THIS STORE HERE, inside the decision.
            // Stored by k_nl_search_advance after nm_play had returned through its divergent exit, h.decision read back as 0 in the
            // next round on gfx950 (the comparison with the model failed on it), while the host execution model played the same source
            // correctly.  The cause was not found: the compiler's handling of h across that exit, or undefined behaviour in the shared
            // body that only the device build exposes.  test_gpu_nlhe_search_match.py's byte comparisons guard a move of this line.
            x->core = h;
            return false;
        }
        parked = 0u;
        const rp_nlhe_subgame_result& res = q->results[x->place];
        const uint32_t bstatus = q->belief_status[x->place];
        const bool same_key = res.past == h.w.sub && res.present == present && res.choices == choices;
        const uint32_t code = bstatus != RP_RECALL_OK ? (uint32_t)RP_SEARCH_FALLBACK_BELIEF
                              : res.status != RP_RECALL_OK ? (uint32_t)RP_SEARCH_FALLBACK_SOLVE
                              : !same_key ? (uint32_t)RP_SEARCH_FALLBACK_KEY : 0u;
        float p[NLMC_A];
        nsm_blend(res, dist, choices, nch, q->visit_threshold, p);
#pragma unroll
        for (uint32_t a = 0; a < NLMC_A; ++a) p[a] = code ? dist[a] : p[a];
        rp_nlhe_search_step* s = step_begin(turn, h.decision, code, dist, p);
        if (s) {
            s->solve_id = solve_id;
            s->recall = x->request.recall;
            s->result = res;
            s->belief_status = (uint8_t)bstatus;
        }
#pragma unroll
        for (uint32_t a = 0; a < NLMC_A; ++a) dist[a] = p[a];
        return true;
    }
};

__global__ __launch_bounds__(NM_BLOCK) void k_nl_search_advance(NlTable t0, NlTable t1, NlParams p, NsmArgs q) {
    const uint32_t i = blockIdx.x * NM_BLOCK + threadIdx.x;
    if (i >= q.match.n) return;
    const uint64_t hand_id = q.match.first_id + i;
    rp_aivat_hand* rec = q.match.hands ? q.match.hands + i : nullptr;
    NsHand* x = q.hands + i;
    NsmSearch s;
    s.q = &q;
    s.x = x;
    s.steps = q.steps && q.steps_cap ? q.steps + (size_t)i * q.steps_cap : nullptr;
    s.hand_id = hand_id;
    s.traced = false;
    NmHand h;
    if (q.first) {
        nm_begin(h, q.match, hand_id, rec);
        s.n_edges = s.searched = s.unsolved = s.solves = s.n_steps = s.parked = 0u;
        if (s.steps) {  // zero past the hand's search decisions
            uint4* z = reinterpret_cast<uint4*>(s.steps);
            for (uint32_t k = 0; k < q.steps_cap * (uint32_t)(sizeof(rp_nlhe_search_step) / 16u); ++k) z[k] = make_uint4(0u, 0u, 0u, 0u);
        }
    } else {
        if (x->done) return;
        h = x->core;
        s.n_edges = x->n_edges, s.searched = x->searched, s.unsolved = x->unsolved, s.solves = x->solves, s.n_steps = x->n_steps, s.parked = x->parked;
    }
    if (nm_play(h, t0, t1, p, q.match, hand_id, rec, s)) {
        const bool outputs = nm_finish(h, q.match, i, rec);
        if (q.searched) q.searched[i] = outputs ? (uint8_t)s.searched : (uint8_t)0;
        if (q.unsolved) q.unsolved[i] = outputs ? (uint8_t)s.unsolved : (uint8_t)0;
        if (!outputs && s.steps) {  // the steps traced so far are taken back
            uint4* z = reinterpret_cast<uint4*>(s.steps);
            const uint32_t made = min(s.n_steps, q.steps_cap);
            for (uint32_t k = 0; k < made * (uint32_t)(sizeof(rp_nlhe_search_step) / 16u); ++k) z[k] = make_uint4(0u, 0u, 0u, 0u);
        }
        x->done = 1u;
        x->parked = 0u;
        return;
    }
    // parked: decide() stored the hand beside its request
    x->n_edges = s.n_edges, x->searched = s.searched, x->unsolved = s.unsolved, x->solves = s.solves, x->n_steps = s.n_steps, x->parked = s.parked;
    x->done = 0u;
}

struct NsmPost {  // pinned, mapped host memory
    uint32_t count[2];  // the round's requests of seat 0 and seat 1
};

struct NsmLists {  // the dense lists of one round: seat 0's requests, then seat 1's
    rp_nlhe_recall* recalls;
    rp_nlhe_frontier* entries;
    uint64_t* ids;
    int8_t* origin;
};

// one workgroup of NSM_SCAN threads over the chunk's n <= NSM_CHUNK hands
__global__ __launch_bounds__(NSM_SCAN) void k_nl_search_compact(NsHand* hands, uint32_t n, NsmLists out, NsmPost* post) {
    constexpr uint32_t PER = NSM_CHUNK / NSM_SCAN;
    __shared__ uint32_t scan[2][NSM_SCAN];
    const uint32_t tid = threadIdx.x;
    uint32_t mine = 0;  // seat 0's count in the low half, seat 1's in the high half
    uint32_t kind[PER];
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        const uint32_t i = tid * PER + k;
        kind[k] = (i < n && !hands[i].done) ? hands[i].parked : 0u;
        mine += kind[k] == 1u ? 1u : (kind[k] == 2u ? 0x10000u : 0u);
    }
    scan[0][tid] = mine;
    __syncthreads();
    uint32_t from = 0;
    for (uint32_t d = 1; d < NSM_SCAN; d <<= 1) {  // inclusive, Hillis-Steele, two buffers
        scan[from ^ 1u][tid] = scan[from][tid] + (tid >= d ? scan[from][tid - d] : 0u);
        from ^= 1u;
        __syncthreads();
    }
    const uint32_t total = scan[from][NSM_SCAN - 1u], before = scan[from][tid] - mine;
    const uint32_t n0 = total & 0xffffu, n1 = total >> 16;
    uint32_t at0 = before & 0xffffu, at1 = n0 + (before >> 16);
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
        if (kind[k] == 0u) continue;
        const uint32_t i = tid * PER + k, place = kind[k] == 1u ? at0++ : at1++;  // place < n0 + n1 <= n <= NSM_CHUNK
        const NsRequest& r = hands[i].request;
        out.recalls[place] = r.recall;
        out.entries[place] = r.entry;
        out.ids[place] = r.solve_id;
        out.origin[place] = r.origin;
        hands[i].place = place;
    }
    if (tid == 0) {
        post->count[0] = n0;
        post->count[1] = n1;
    }
}

}  // namespace rp

#endif
