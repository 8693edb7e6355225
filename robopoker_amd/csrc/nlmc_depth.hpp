// nlmc_depth.hpp — the depth-limited re-solve (rp_nlhe_depth_solve): `iterations` steps of DepthSolver on one small tree per step, the
// local profile beside it, the rollouts of every frontier of the tree in the same launch, then the harvest.  Read-only with respect to
// the blueprint, like nlmc_query.hpp, nlmc_range.hpp and nlmc_frontier.hpp.
//
// Reference: DepthSolver::step / harvest (subgame/src/depth/solver.rs:76-123), DepthEncoder::branches (depth/encoder.rs:93-121),
// DepthGame (depth/game.rs), DepthProfile / DepthView (depth/profile.rs, depth/view.rs), TreeBuilder (mccfr/src/solver/builder.rs),
// ExternalSampling (sample/external.rs), Tree::partition (state/tree.rs:138-147), CfrFlow::dfs / recursed_value / ancestor_reach
// (strategy/flow.rs:64-154), CfrNash::terminal_value (strategy/nash.rs:66-79), Solver::update_* (solver/solver.rs:143-192),
// RefProf::warmstart (strategy/profile.rs:94-104).  The rules are stated in include/rp_mi355x.h above rp_nlhe_depth_solve.
//
// One workgroup per solve, every iteration inside the one launch, workgroup barriers between the phases of an iteration:
//   A  lane 0 grows the tree in LDS (one street's tree is small and serial by nature: the builder's stack decides the node numbers).
//      A node keeps its game packed in 24 bytes (the cards are the solve's), its path as a key reads it, its parent, its newest child
//      and its next-older sibling (petgraph's adjacency lists: walking them is slot order), and the sampling probability of the one
//      child kept below a sampled node.  An infoset met in the tree gets one entry holding cum_regret / cum_weight of its slots and
//      cum_payoff of its first as the profile answers them at the start of the iteration — from the local row, else gathered from the
//      blueprint (nlq_find, one row) — so phases A and C read the profile AS IT STOOD however far the updates have got, and the
//      Decisions need no buffer: an infoset is updated as soon as its vectors are known.  Entries are found by key and made in node
//      order, so their order is the partition's head order and a node's entry links the span.
//   B  every lane: the 16 x rollouts games of each frontier node, nf_cells of nlmc_frontier.hpp (nf_rollout, chunked and folded as
//      k_nl_frontier does it), with the stream id the header states;
//   C  lane 0: per updated infoset two linear sweeps over the root's subtree (a contiguous run of node numbers) instead of the
//      reference's recursion: down for the reach products, up — in descending node number, which visits a node's children in slot
//      order — for the sums.  Then the update of its row.
// The local profile keeps its first ND_ROWS_LDS rows in LDS and the rest in the solve's overflow region of device memory (NdRows); 32
// bits of every key stay in LDS for the lookups.  After the last iteration the lanes rank the rows by key (one lane per row), lane 0
// folds sum_regret and writes the result; the rows leave one lane per row.
// Everything but the kernel's own skeleton is a function the subgame solve calls too (nlmc_subgame.hpp): a float fold, the frontier
// id or the status rule changed here changes both.
#ifndef RP_NLMC_DEPTH_HPP
#define RP_NLMC_DEPTH_HPP

#include "nlmc_frontier.hpp"

namespace rp {

#define ND_BLOCK NF_BLOCK
#define ND_NODES RP_NLHE_DEPTH_MAX_NODES
#define ND_ROWS RP_NLHE_DEPTH_MAX_ROWS
#define ND_ROWS_LDS 64u  // the rows kept in LDS; the rest of a solve's profile overflows into its region of global memory
#define ND_ROWS_OVF (ND_ROWS - ND_ROWS_LDS)
#define ND_FRONTIERS RP_NLHE_DEPTH_MAX_FRONTIERS
#define ND_INFOS 96u   // distinct infosets with children in one tree
#define ND_TODO 256u   // pending branches
#define ND_NONE 0xffffu
#define ND_PRESENT_BITS 29u  // present is street << 8 | index; bits 29-30 of a local key are free for a tag, bit 31 is the kind
static_assert(sizeof(rp_nlhe_depth_args) == 40 && sizeof(rp_nlhe_depth_result) == 144 && sizeof(rp_nlhe_depth_row) == 168, "INTEGRATION.md mirrors them");
static_assert(NF_CELLS * NF_CHUNK * sizeof(int16_t) >= 3u * ND_NODES * sizeof(float), "the sweeps' three floats per node live in the rollouts' buffer");

enum : uint32_t { NDP_DELEGATE = 0, NDP_INTERNAL = 1, NDP_EXTERNAL = 2 };               // DepthPhase
enum : uint32_t { NDT_SEAT0 = 0, NDT_SEAT1 = 1, NDT_CHANCE = 2, NDT_TERMINAL = 3 };     // DepthGame::turn of the node as grown

struct NdArgs {
    const rp_nlhe_frontier* entries;
    const int8_t* origin;  // may be NULL: every entry's own street
    uint32_t iterations, rollouts, rows_cap;
    float bias, prior;
    uint64_t step_hash_rollout;  // rp_node_hash_step(seed, 0): the frontier's stream
    uint64_t step_hash_tree;     // rp_node_hash_step(seed, 2): the tree's own draws
    uint64_t first_id;           // the id of entries[0]
    struct NdRow* overflow;      // [n][ND_ROWS_OVF]: the rows past ND_ROWS_LDS of each solve
    rp_nlhe_depth_result* results;
    rp_nlhe_depth_row* rows;     // [n][rows_cap], may be NULL
};

struct NdNode {  // 56 bytes
    uint64_t board;
    union {
        uint64_t tail;  // NrpPath::tail of a node that is not a terminal state
        float tv[2];    // a terminal state: game.payoff(seat)
    };
    uint32_t g0;              // ticker (< 48 + ND_NODES: 10 bits) | state[0] << 10 | state[1] << 12 | pot << 14 (at most 2 x 32 767)
    int16_t stack[2], stake[2], spent[2];
    uint16_t pathc;           // NrpPath: tail_len | aggr << 4 | n << 8 (each at most 12)
    uint16_t parent, first, next, info, span_next, last, depth;
    uint32_t meta;            // phase | k << 2 | j << 4 | turn << 6 | slot << 8 | frontier << 12 (63: none) | sampled << 18
    float fsk;                // a sampled node: q of the child it kept
};
__device__ __forceinline__ uint32_t nd_phase(uint32_t m) { return m & 3u; }
__device__ __forceinline__ uint32_t nd_k(uint32_t m) { return (m >> 2) & 3u; }
__device__ __forceinline__ uint32_t nd_j(uint32_t m) { return (m >> 4) & 3u; }
__device__ __forceinline__ uint32_t nd_turn(uint32_t m) { return (m >> 6) & 3u; }
__device__ __forceinline__ uint32_t nd_slot(uint32_t m) { return (m >> 8) & 15u; }
__device__ __forceinline__ uint32_t nd_frontier(uint32_t m) { return (m >> 12) & 63u; }
__device__ __forceinline__ bool nd_sampled(uint32_t m) { return ((m >> 18) & 1u) != 0; }

struct NdInfo {  // an infoset of the tree as the profile read at the start of the iteration: 120 bytes
    uint64_t past, choices;
    uint32_t present_kind;  // present | kind << 31
    uint32_t nch;
    int32_t row;            // its local row, -1: none
    uint32_t head, tail;    // the span: first and last node
    float rd;               // regret_denom
    float r[NLMC_A], w[NLMC_A];  // cum_regret, cum_weight
    float p0;               // cum_payoff of the first choice
    uint32_t pad;
};
struct NdRow {  // a local row: 168 bytes
    uint64_t past, choices;
    uint32_t present_kind, nch;
    float w[NLMC_A], r[NLMC_A], p[NLMC_A];
    uint32_t v[NLMC_A];
};
// A solve's local profile: the first ND_ROWS_LDS rows in LDS, later ones in the solve's overflow region; `hash` (LDS) holds 32 bits of
// every row's key so that a lookup scans LDS and touches a row only to confirm.  H: how many of the 32 bits are kept (the subgame
// solve, whose profile is four times as deep, keeps 16)
template <class H>
struct NdRowsT {
    typedef H hash_t;
    NdRow* lds;
    NdRow* ovf;
    H* hash;
    __device__ __forceinline__ NdRow& at(uint32_t i) const { return i < ND_ROWS_LDS ? lds[i] : ovf[i - ND_ROWS_LDS]; }
};
typedef NdRowsT<uint32_t> NdRows;
struct NdShared {
    NfPublic pub;
    NfFlags flags;
    uint32_t status, n_nodes, n_infos, n_rows, n_frontiers, n_todo, t;
    int origin;
    uint64_t c_nodes, c_infosets, c_frontiers;
    uint16_t fnode[ND_FRONTIERS];
    uint32_t todo[ND_TODO];  // parent | slot << 16
    float pay[ND_FRONTIERS][NF_CELLS];
    // lane 0's vectors over the slots of one infoset: indexed by a run-time slot, they would live in scratch memory as locals
    float tmp[7][NLMC_A];
    uint32_t tmpu[NLMC_A];
};

static_assert(sizeof(NdNode) == 56 && sizeof(NdInfo) == 120 && sizeof(NdRow) == 168, "the LDS budget of k_nl_depth counts on these");

__device__ __forceinline__ void nd_pack(const G2& g, NdNode& n) {
    n.board = g.board;
    n.g0 = (uint32_t)g.ticker | ((uint32_t)g.state[0] << 10) | ((uint32_t)g.state[1] << 12) | ((uint32_t)g.pot << 14);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        n.stack[i] = (int16_t)g.stack[i];
        n.stake[i] = (int16_t)g.stake[i];
        n.spent[i] = (int16_t)g.spent[i];
    }
}
__device__ __forceinline__ void nd_unpack(const NdNode& n, const G2& entry, G2& g) {
    g.n = 2;
    g.dealer = entry.dealer;
    g.cards[0] = entry.cards[0];
    g.cards[1] = entry.cards[1];
    g.board = n.board;
    g.ticker = (int)(n.g0 & 0x3ffu);
    g.state[0] = (int)((n.g0 >> 10) & 3u);
    g.state[1] = (int)((n.g0 >> 12) & 3u);
    g.pot = (int)(n.g0 >> 14);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        g.stack[i] = n.stack[i];
        g.stake[i] = n.stake[i];
        g.spent[i] = n.spent[i];
    }
}
__device__ __forceinline__ NrpPath nd_path(const NdNode& n) {
    NrpPath p;
    p.tail = n.tail;
    p.tail_len = n.pathc & 15u;
    p.aggr = (n.pathc >> 4) & 15u;
    p.n = (uint32_t)n.pathc >> 8;
    return p;
}

// the blueprint's row of a Game infoset as DepthView reads it: found -> the stored regrets, weights, payoffs and visits; absent -> the
// table's defaults (rp_nlhe_memory)
__device__ __forceinline__ bool nd_blueprint(const NlTable& t, uint64_t past, uint64_t choices, uint32_t present, float* r, float* w, float* p, uint32_t* v) {
    const uint32_t home = (uint32_t)nl_key_hash(past, choices, present) & t.mask;
    const uint4* sl = reinterpret_cast<const uint4*>(t.slots + home);
    const uint4 lo = sl[0], hi = sl[1];
    uint32_t row;
    const bool found = nlq_find(t, past, choices, present, home, lo, hi, &row);
    const float* q = t.rows + (size_t)row * 4u * NLMC_A;
    for (uint32_t a = 0; a < NLMC_A; ++a) {
        r[a] = found ? q[a] : nl_default_regret((uint32_t)(choices >> (5u * a)) & 31u);
        w[a] = found ? q[NLMC_A + a] : 0.0f;
        if (p) p[a] = found ? q[2u * NLMC_A + a] : 0.0f;
        if (v) v[a] = found ? reinterpret_cast<const uint32_t*>(q)[3u * NLMC_A + a] : 0u;
    }
    return found;
}

__device__ __forceinline__ uint32_t nd_row_hash(uint64_t past, uint64_t choices, uint32_t present_kind) {
    return (uint32_t)(nl_key_hash(past, choices, present_kind) >> 32);
}
template <class R>
__device__ __forceinline__ int nd_find_row(const R& rows, uint32_t n, uint64_t past, uint64_t choices, uint32_t present_kind) {
    const typename R::hash_t h = (typename R::hash_t)nd_row_hash(past, choices, present_kind);
    for (uint32_t i = 0; i < n; ++i) {
        if (rows.hash[i] != h) continue;
        const NdRow& r = rows.at(i);
        if (r.past == past && r.choices == choices && r.present_kind == present_kind) return (int)i;
    }
    return -1;
}

// the entry of an infoset in this tree's table: found by key or made from the profile as it stands.  ND_NONE: the table is full.
// tag: bits above `present` that belong to the LOCAL key only (the subgame solve's world, nlmc_subgame.hpp); the blueprint is asked
// without them
template <class R>
__device__ __forceinline__ uint32_t nd_info_of(const NlTable& t, NdShared& sh, NdInfo* infos, const R& rows, uint64_t past, uint64_t choices,
                                               uint32_t present, uint32_t kind, uint32_t nch, uint32_t node, uint32_t tag = 0u) {
    const uint32_t pk = present | tag | (kind << 31);
    for (uint32_t i = 0; i < sh.n_infos; ++i)
        if (infos[i].past == past && infos[i].choices == choices && infos[i].present_kind == pk) return i;
    if (sh.n_infos >= ND_INFOS) return ND_NONE;
    NdInfo& e = infos[sh.n_infos];
    e.past = past;
    e.choices = choices;
    e.present_kind = pk;
    e.nch = nch;
    e.head = e.tail = node;
    e.row = nd_find_row(rows, sh.n_rows, past, choices, pk);
    if (e.row >= 0) {
        const NdRow& row = rows.at(e.row);
        for (uint32_t a = 0; a < NLMC_A; ++a) {
            e.r[a] = row.r[a];
            e.w[a] = row.w[a];
        }
        e.p0 = row.p[0];
    } else if (kind == 1u) {  // DepthView's Pick edges
        for (uint32_t a = 0; a < NLMC_A; ++a) {
            e.r[a] = RP_EPSILON;
            e.w[a] = 0.25f;
        }
        e.p0 = 0.0f;
    } else {
        float *r = sh.tmp[0], *w = sh.tmp[1], *p = sh.tmp[2];
        nd_blueprint(t, past, choices, present, r, w, p, nullptr);
        for (uint32_t a = 0; a < NLMC_A; ++a) {
            e.r[a] = rp_maxf(r[a], RP_EPSILON);
            e.w[a] = rp_maxf(w[a], RP_EPSILON);
        }
        e.p0 = p[0];
    }
    float rd = 0.0f;
    for (uint32_t a = 0; a < nch; ++a) rd += rp_maxf(e.r[a], RP_EPSILON);
    e.rd = rd;
    return sh.n_infos++;
}

// the weighted draw of a sampled node (sample/external.rs:41-64): the slot kept and its sampling probability
__device__ __forceinline__ uint32_t nd_weighted(const NlParams& p, const NdInfo& e, uint64_t h, float* q /* [NLMC_A] */, float* q_kept) {
    const DistParams hp{p.temperature, p.smoothing, p.curiosity};
    policy_distribution<NLMC_A>((int)RP_DIST_SAMPLING, hp, e.w, e.nch, q);
    float total = 0.0f;
    for (uint32_t a = 0; a < e.nch; ++a) total += rp_maxf(q[a], RP_EPSILON);
    const float u = rp_u01(h) * total;
    uint32_t pick = 0;
    float cum = 0.0f;
    for (uint32_t a = 0; a + 1 < e.nch; ++a) {
        cum += rp_maxf(q[a], RP_EPSILON);
        if (pick == a && cum <= u) pick = a + 1;
    }
    *q_kept = q[pick];
    return pick;
}

// One node: TreeBuilder::next's grow + branches + sample.  `g`, `path`: the node's state; the branches kept go onto the stack in slot
// order.  Returns a status.
template <class R>
__device__ __forceinline__ uint32_t nd_grow(const NlTable& t, const NlParams& p, NdShared& sh, NdNode* nodes, NdInfo* infos, const R& rows, const G2& g,
                                            const NrpPath& path, uint32_t parent, uint32_t slot, uint32_t phase, uint32_t k, uint32_t j,
                                            uint32_t depth, uint32_t walker, uint64_t tree_hash, uint32_t tag = 0u) {
    if (sh.n_nodes >= ND_NODES) return RP_DEPTH_NODES;
    const uint32_t idx = sh.n_nodes++;
    NdNode& n = nodes[idx];
    nd_pack(g, n);
    n.tail = path.tail;
    n.pathc = (uint16_t)(path.tail_len | (path.aggr << 4) | (path.n << 8));
    n.parent = (uint16_t)parent;
    n.first = n.next = n.info = n.span_next = ND_NONE;
    n.last = (uint16_t)idx;
    n.depth = (uint16_t)depth;
    n.fsk = 1.0f;
    if (parent != ND_NONE) {  // petgraph: the newest edge heads the list
        n.next = nodes[parent].first;
        nodes[parent].first = (uint16_t)idx;
    }
    const int inner = g.turn();
    const int internal = (int)sh.pub.internal;
    uint32_t turn = phase == NDP_INTERNAL ? (uint32_t)(1 - internal) : (phase == NDP_EXTERNAL ? (uint32_t)NDT_TERMINAL
                    : (inner == NT_TERMINAL ? (uint32_t)NDT_TERMINAL : (inner == NT_CHANCE ? (uint32_t)NDT_CHANCE : (uint32_t)inner)));
    uint32_t frontier = 63u, sampled = 0u, err = 0u;
    const uint64_t h = rp_node_hash_key(tree_hash, (uint64_t)idx);
    uint32_t first_slot = 0, n_slots = 0;  // the branches kept: first_slot .. first_slot + n_slots
    if (phase == NDP_DELEGATE && inner == NT_TERMINAL) {
        int reward[2];
        nl_settle(g, reward);
        n.tv[0] = (float)(reward[0] - g.spent[0]);
        n.tv[1] = (float)(reward[1] - g.spent[1]);
    } else if (phase == NDP_DELEGATE && inner == NT_CHANCE) {
        if (g.street() > sh.origin) {  // at_frontier: `randomly` keeps one Pick
            if (sh.n_frontiers >= ND_FRONTIERS) return RP_DEPTH_FRONTIERS;
            frontier = sh.n_frontiers;
            sh.fnode[sh.n_frontiers++] = (uint16_t)idx;
            first_slot = rp_pick_uniform(h, RP_NLHE_FRONTIER_LEAVES);
            n_slots = 1;
        }
    } else if (phase != NDP_EXTERNAL) {
        uint64_t choices = NE_DRAW;
        uint32_t nch = RP_NLHE_FRONTIER_LEAVES, kind = 1u;
        const int seat = phase == NDP_INTERNAL ? g.actor() : inner;  // sweat(): the ticker's seat at a chance node
        if (phase == NDP_DELEGATE) {
            kind = 0u;
            nch = nl_choices_path(nl_view(g), (int)path.aggr, &choices);
            if (nch == 0u) return RP_RECALL_ILLEGAL;
        }
        const uint32_t present = nl_bucket(p, g.street(), seat ? g.cards[1] : g.cards[0], g.board, &err);
        if (err) return RP_RECALL_LOOKUP;
        const uint32_t e = nd_info_of(t, sh, infos, rows, path.tail, choices, present, kind, nch, idx, tag);
        if (e == ND_NONE) return RP_DEPTH_NODES;
        n.info = (uint16_t)e;
        if (infos[e].head != idx) {  // a later node of the span
            nodes[infos[e].tail].span_next = (uint16_t)idx;
            infos[e].tail = idx;
        }
        if (turn == walker) {
            n_slots = nch;
        } else {
            sampled = 1u;
            first_slot = nd_weighted(p, infos[e], h, sh.tmp[0], &n.fsk);
            n_slots = 1;
        }
    }
    n.meta = phase | (k << 2) | (j << 4) | (turn << 6) | (slot << 8) | (frontier << 12) | (sampled << 18);
    if (sh.n_todo + n_slots > ND_TODO) return RP_DEPTH_NODES;
    for (uint32_t a = 0; a < n_slots; ++a) sh.todo[sh.n_todo++] = idx | ((first_slot + a) << 16);
    return RP_RECALL_OK;
}

// Phase A: the tree of iteration sh.t.  Returns a status.
template <class R>
__device__ __forceinline__ uint32_t nd_build(const NlTable& t, const NlParams& p, NdShared& sh, NdNode* nodes, NdInfo* infos, const R& rows,
                                             uint32_t walker, uint64_t tree_hash, uint32_t tag = 0u) {
    sh.n_nodes = sh.n_infos = sh.n_frontiers = sh.n_todo = 0;
    const G2 entry = sh.pub.game;
    uint32_t st = nd_grow(t, p, sh, nodes, infos, rows, entry, sh.pub.path, ND_NONE, 0, NDP_DELEGATE, 0, 0, 0, walker, tree_hash, tag);
    while (st == RP_RECALL_OK && sh.n_todo > 0) {
        const uint32_t leaf = sh.todo[--sh.n_todo], parent = leaf & 0xffffu, slot = leaf >> 16;
        const NdNode& pn = nodes[parent];
        G2 g;
        nd_unpack(pn, entry, g);
        NrpPath path = nd_path(pn);
        const uint32_t pm = pn.meta;
        uint32_t phase = NDP_DELEGATE, k = 0, j = 0, depth = pn.depth;
        if (nd_phase(pm) == NDP_INTERNAL) {
            phase = NDP_EXTERNAL;
            k = nd_k(pm);
            j = slot;
        } else if (nd_turn(pm) == NDT_CHANCE) {
            phase = NDP_INTERNAL;
            k = slot;
        } else {  // game.apply(game.snap(game.actionize(edge)))
            const uint32_t e = (uint32_t)(infos[pn.info].choices >> (5u * slot)) & 31u;
            const NlAction act = nl_action_v(nl_view(g), e);
            if (!g.allowed(act)) return RP_RECALL_ILLEGAL;
            g.force_act(act);
            path.push(e);
            depth += 1u;
        }
        st = nd_grow(t, p, sh, nodes, infos, rows, g, path, parent, slot, phase, k, j, depth, walker, tree_hash, tag);
    }
    // the last descendant of every node: a subtree is the run of node numbers [node, last]
    for (uint32_t x = sh.n_nodes; st == RP_RECALL_OK && x-- > 1u;) {
        NdNode& pn = nodes[nodes[x].parent];
        pn.last = pn.last > nodes[x].last ? pn.last : nodes[x].last;
    }
    return st;
}

// regret(edge) / rd of the edge into node x, read at its parent (instant_policy)
__device__ __forceinline__ float nd_instant(const NdInfo* infos, const NdNode& parent, const NdNode& x) {
    const NdInfo& e = infos[parent.info];
    return rp_maxf(e.r[nd_slot(x.meta)], RP_EPSILON) / e.rd;
}

// terminal_value (nash.rs:66-79) of a node without children for `hero`
__device__ __forceinline__ float nd_terminal(const NdShared& sh, const NdNode* nodes, const NdInfo* infos, const NdNode& x, uint32_t hero) {
    const uint32_t m = x.meta;
    if (nd_phase(m) == NDP_EXTERNAL) {
        const uint32_t f = nd_frontier(nodes[nodes[x.parent].parent].meta);
        const float val = sh.pay[f][nd_k(m) * RP_NLHE_FRONTIER_LEAVES + nd_j(m)];
        return hero == sh.pub.internal ? val : -val;
    }
    if (nd_turn(m) == NDT_TERMINAL) return x.tv[hero];
    return infos[nodes[x.parent].info].p0;  // a chance leaf: its parent is a decision node (a chance node's children are Picks)
}

// CfrFlow::dfs for the infoset `e` + Solver::update_*: Phase C for one infoset.  rr / sr / val: three floats per node.  Returns a status.
// ROWS: the cap of the local profile; TAGGED: present_kind carries a tag above ND_PRESENT_BITS that the blueprint's key does not have.
template <uint32_t ROWS = ND_ROWS, bool TAGGED = false, class R>
__device__ __forceinline__ uint32_t nd_update(const NlTable& t, NdShared& sh, const NdNode* nodes, const NdInfo* infos, const R& rows,
                                              uint32_t ei, uint32_t walker, float prior, float* rr, float* sr, float* val) {
    const NdInfo& e = infos[ei];
    const uint32_t nch = e.nch;
    float *delta = sh.tmp[0], *v = sh.tmp[1], *policy = sh.tmp[2], *ws = sh.tmp[3], payoff = 0.0f;
    for (uint32_t a = 0; a < NLMC_A; ++a) delta[a] = 0.0f;
    for (uint32_t root = e.head; root != ND_NONE; root = nodes[root].span_next) {
        const NdNode& rn = nodes[root];
        const uint32_t hero = nd_turn(rn.meta);
        // ancestor_reach
        float cf = 1.0f, sm = 1.0f;
        for (uint32_t c = root; nodes[c].parent != ND_NONE; c = nodes[c].parent) {
            const NdNode& pn = nodes[nodes[c].parent];
            const uint32_t pt = nd_turn(pn.meta);
            if (pt != NDT_CHANCE && pt != walker) {
                cf *= nd_instant(infos, pn, nodes[c]);
                sm *= pn.fsk;
            }
        }
        const float reach = cf / sm;
        // recursed_value of every child of root: down ...
        const uint32_t last = rn.last;
        for (uint32_t x = root + 1u; x <= last; ++x) {
            const NdNode& xn = nodes[x];
            const NdNode& pn = nodes[xn.parent];
            if (xn.parent == root) {
                rr[x] = sr[x] = 1.0f;
            } else {
                rr[x] = nd_turn(pn.meta) == NDT_CHANCE ? rr[xn.parent] : rr[xn.parent] * nd_instant(infos, pn, xn);
                sr[x] = nd_sampled(pn.meta) ? sr[xn.parent] * pn.fsk : sr[xn.parent];
            }
            val[x] = 0.0f;
        }
        // ... and up: descending node numbers meet a node's children in slot order, each complete when it is added
        for (uint32_t x = last; x > root; --x) {
            const NdNode& xn = nodes[x];
            if (xn.first == ND_NONE) val[x] = (rr[x] / sr[x]) * nd_terminal(sh, nodes, infos, xn, hero);
            if (xn.parent != root) val[xn.parent] += val[x];
        }
        float ev = 0.0f;
        for (uint32_t c = rn.first; c != ND_NONE; c = nodes[c].next) {
            const uint32_t a = nd_slot(nodes[c].meta);
            v[a] = reach * val[c];
            ev += (rp_maxf(e.r[a], RP_EPSILON) / e.rd) * v[a];
        }
        payoff += ev;
        for (uint32_t c = rn.first; c != ND_NONE; c = nodes[c].next) {
            const uint32_t a = nd_slot(nodes[c].meta);
            delta[a] += v[a] - ev;
        }
    }
    const DistParams none{1.0f, 0.0f, 0.0f};
    policy_distribution<NLMC_A>((int)RP_DIST_ITERATED, none, e.r, nch, policy);
    // the update.  The head's turn is the walker, so every slot has a child at the head and a delta.
    const float tf = (float)sh.t;
    int ri = e.row;
    if (ri < 0) {
        if (sh.n_rows >= ROWS) return RP_DEPTH_ROWS;
        ri = (int)sh.n_rows++;
        rows.hash[ri] = (typename R::hash_t)nd_row_hash(e.past, e.choices, e.present_kind);
        NdRow& row = rows.at(ri);
        row.past = e.past;
        row.choices = e.choices;
        row.present_kind = e.present_kind;
        row.nch = nch;
        for (uint32_t a = 0; a < NLMC_A; ++a) ws[a] = 0.0f;  // a Pick edge: Encounter::default()
        if ((e.present_kind >> 31) == 0u) {                   // warmstart: the blueprint's averaged policy scaled by k (k + 1) / 2
            float *br = sh.tmp[4], *bw = sh.tmp[5], *avg = sh.tmp[6];
            nd_blueprint(t, e.past, e.choices, TAGGED ? e.present_kind & ((1u << ND_PRESENT_BITS) - 1u) : e.present_kind, br, bw, nullptr, nullptr);
            policy_distribution<NLMC_A>((int)RP_DIST_AVERAGED, none, bw, nch, avg);
            for (uint32_t a = 0; a < nch; ++a) ws[a] = ((avg[a] * prior) * (prior + 1.0f)) / 2.0f;
        }
        for (uint32_t a = 0; a < NLMC_A; ++a) {
            const bool live = a < nch;
            // update_regret reads cum_regret before the edge exists: max(blueprint, EPSILON), not the warmstart's regret
            row.r[a] = live ? rp_maxf(e.r[a] + delta[a], -INFINITY) : 0.0f;
            row.w[a] = live ? rp_maxf(ws[a] + policy[a] * tf, RP_EPSILON) : 0.0f;
            float pay = 0.0f;
            pay += (payoff - pay) / (float)(0u + 1u);
            row.p[a] = live ? pay : 0.0f;
            row.v[a] = live ? 1u : 0u;
        }
    } else {
        NdRow& row = rows.at(ri);
        for (uint32_t a = 0; a < nch; ++a) {
            row.r[a] = rp_maxf(row.r[a] + delta[a], -INFINITY);
            row.w[a] = rp_maxf(row.w[a] + policy[a] * tf, RP_EPSILON);
            row.p[a] += (payoff - row.p[a]) / (float)(row.v[a] + 1u);
            row.v[a] += 1u;
        }
    }
    // the warmstart's regret (blueprint regret * k / epoch) is never computed: update_regret overwrites it before anything can read it
    return RP_RECALL_OK;
}

__device__ __forceinline__ bool nd_row_less(const NdRow& a, const NdRow& b) {  // (kind, past, present, choices)
    const uint32_t ka = a.present_kind >> 31, kb = b.present_kind >> 31;
    if (ka != kb) return ka < kb;
    if (a.past != b.past) return a.past < b.past;
    if (a.present_kind != b.present_kind) return a.present_kind < b.present_kind;
    return a.choices < b.choices;
}

// ---- what the two solves share beside the tree: k_nl_depth below and k_nl_subgame (nlmc_subgame.hpp) call these ----

// sh.origin of solve i.  `none`: the caller's constant for "no origin given", read as `none_is`; any other value outside -1 .. 3 is
// RP_RECALL_SEAT
__device__ __forceinline__ uint32_t nd_origin(const int8_t* origin, uint32_t i, int none, int none_is, int* out) {
    const int o = origin ? (int)origin[i] : none;
    *out = o == none ? none_is : o;
    return o != none && (o < -1 || o > 3) ? (uint32_t)RP_RECALL_SEAT : (uint32_t)RP_RECALL_OK;
}

// lane 0 before the first iteration: the status of the entry, an empty profile, the counters at zero
__device__ __forceinline__ void nd_begin(NdShared& sh, uint32_t st) {
    sh.status = st;
    sh.flags.lookup_miss = sh.flags.stuck = 0;
    sh.n_rows = sh.t = 0;
    sh.c_nodes = sh.c_infosets = sh.c_frontiers = 0;
}

// Phase B: the payoffs of every frontier of the tree into sh.pay, and the status.  Called by all ND_BLOCK lanes under uniform control
// flow: the barriers of nf_cells and the one here are reached by every lane, and what decides the trip count (sh.n_frontiers,
// sh.status) is read after a barrier.  entry: the solve's record, for the length of its history; id, it: the solve's and the iteration's.
// The length and the tree's number are taken anew for every frontier: held across nf_cells they cost k_nl_subgame 36 more scalar
// spills and 1 - 3 % of its time.
__device__ __forceinline__ void nd_frontiers(const NlTable& t, const NlParams& p, NdShared& sh, const NdNode* nodes, const rp_nlhe_frontier& entry,
                                             uint64_t id, uint32_t it, float bias, uint32_t rollouts, uint64_t step_hash, int16_t* s_won) {
    const uint32_t tid = threadIdx.x, n_frontiers = sh.n_frontiers;
    for (uint32_t f = 0; f < n_frontiers; ++f) {
        const NdNode& fn = nodes[sh.fnode[f]];
        const bool fits = (uint32_t)entry.n_edges + fn.depth <= RP_NLHE_MAX_HISTORY;
        G2 g;
        nd_unpack(fn, sh.pub.game, g);
        const NrpPath path = sh.pub.path;  // payoffs(&self.prefix, ..): a rollout's story starts from the PREFIX, not from the node's path
        const uint64_t fid = (id * RP_NLHE_DEPTH_MAX_ITERATIONS + it) * RP_NLHE_DEPTH_MAX_FRONTIERS + f;
        const float sum = nf_cells(t, p, fits, g, path, (int)sh.pub.internal, bias, rollouts, step_hash, fid, s_won, nullptr, &sh.flags);
        if (tid < NF_CELLS) sh.pay[f][tid] = sum / (float)rollouts;
        if (tid == 0 && sh.status == RP_RECALL_OK)  // the first frontier that fails gives the status
            sh.status = !fits ? (uint32_t)RP_RECALL_LENGTH
                              : (sh.flags.lookup_miss ? (uint32_t)RP_RECALL_LOOKUP : (sh.flags.stuck ? (uint32_t)RP_RECALL_ILLEGAL : (uint32_t)RP_RECALL_OK));
        __syncthreads();
        if (sh.status != RP_RECALL_OK) break;
    }
}

// Phase C, lane 0 only: the update of every infoset of iteration `it`'s walker, in entry order, then the counters.  buf: the sweeps'
// 3 x ND_NODES floats.  ROWS, TAGGED: nd_update's.
template <uint32_t ROWS, bool TAGGED, class R>
__device__ __forceinline__ void nd_updates(const NlTable& t, NdShared& sh, const NdNode* nodes, const NdInfo* infos, const R& rows, uint32_t it,
                                           float prior, float* buf) {
    const uint32_t walker = it & 1u;
    uint32_t st = RP_RECALL_OK, updated = 0;
    for (uint32_t e = 0; e < sh.n_infos && st == RP_RECALL_OK; ++e) {
        if (nd_turn(nodes[infos[e].head].meta) != walker) continue;  // record_infosets
        st = nd_update<ROWS, TAGGED>(t, sh, nodes, infos, rows, e, walker, prior, buf, buf + ND_NODES, buf + 2u * ND_NODES);
        updated += 1u;
    }
    sh.status = st;
    sh.c_nodes += sh.n_nodes;
    sh.c_infosets += updated;
    sh.c_frontiers += sh.n_frontiers;
    sh.t = it + 1u;
}

// the rows ranked by key, one lane per row: keys are distinct, so the ranks are a permutation.  rank[x]: the row of rank x (LDS).  No
// barrier inside; the caller's follows.
template <bool (*LESS)(const NdRow&, const NdRow&), class R>
__device__ __forceinline__ void nd_rank(const R& rows, uint32_t n_rows, uint16_t* rank) {
    for (uint32_t a = threadIdx.x; a < n_rows; a += ND_BLOCK) {
        const NdRow& ra = rows.at(a);
        uint32_t below = 0;
        for (uint32_t b = 0; b < n_rows; ++b) below += LESS(rows.at(b), ra) ? 1u : 0u;
        rank[below] = (uint16_t)a;
    }
}

// lane 0: the result cleared, its status, and of a solve that went well the fields the two results share — sum_regret folded in
// ranked order, slots ascending, and the counters.  OUT: written in place, a local copy's arrays would be indexed at run time.
// Returns whether the solve went well.
template <class OUT, class R>
__device__ __forceinline__ bool nd_result_head(OUT& out, const NdShared& sh, const R& rows, const uint16_t* rank, uint32_t rollouts) {
    out = OUT{};
    out.status = (uint8_t)sh.status;
    if (sh.status != RP_RECALL_OK) return false;
    const uint32_t n_rows = sh.n_rows;
    float total = 0.0f;
    for (uint32_t x = 0; x < n_rows; ++x) {
        const NdRow& row = rows.at(rank[x]);
        for (uint32_t a = 0; a < row.nch; ++a) total += rp_maxf(row.r[a], 0.0f);
    }
    out.sum_regret = total / (float)(sh.t > 1u ? sh.t : 1u);
    out.iterations = sh.t;
    out.n_rows = n_rows;
    out.nodes = sh.c_nodes;
    out.infosets = sh.c_infosets;
    out.frontiers = sh.c_frontiers;
    out.rollouts = sh.c_frontiers * NF_CELLS * rollouts;
    return true;
}

// the infoset of the entry state, whose turn it is (turn >= 0): DepthInfo::Game(info).  err: nl_bucket's
struct NdEntry {
    uint64_t choices;
    uint32_t nch, present, err;
};
__device__ __forceinline__ NdEntry nd_entry(const NlParams& p, const G2& g, int turn, const NrpPath& path) {
    NdEntry e;
    e.err = 0;
    e.nch = nl_choices_path(nl_view(g), (int)path.aggr, &e.choices);
    e.present = nl_bucket(p, g.street(), turn ? g.cards[1] : g.cards[0], g.board, &e.err);
    return e;
}
// cum_regret r[] and visits v[] of the entry infoset as the harvest reads them: from the local row of key (past, choices, present | tag)
// if there is one, else from the blueprint's row of the untagged key with max(r, RP_EPSILON).  w, pp: NLMC_A floats each for the rest
// of the blueprint's answer
template <class R>
__device__ __forceinline__ void nd_entry_row(const NlTable& t, const R& rows, uint32_t n_rows, uint64_t past, const NdEntry& e, uint32_t tag, float* r,
                                             uint32_t* v, float* w, float* pp) {
    const int ri = nd_find_row(rows, n_rows, past, e.choices, e.present | tag);
    if (ri >= 0) {
        for (uint32_t a = 0; a < NLMC_A; ++a) {
            r[a] = rows.at(ri).r[a];
            v[a] = rows.at(ri).v[a];
        }
    } else {
        nd_blueprint(t, past, e.choices, e.present, r, w, pp, v);
        for (uint32_t a = 0; a < NLMC_A; ++a) r[a] = rp_maxf(r[a], RP_EPSILON);
    }
}
// lane 0: the entry infoset's key and regret into the result; a bucket the tables do not know makes the whole result its status
template <class OUT>
__device__ __forceinline__ void nd_result_entry(OUT& out, NdShared& sh, const NdEntry& e, float regret) {
    out.regret = regret;
    out.past = sh.pub.path.tail;
    out.choices = e.choices;
    out.present = e.present;
    out.n_actions = (uint8_t)e.nch;
    if (e.err) {
        out = OUT{};
        out.status = (uint8_t)RP_RECALL_LOOKUP;
        sh.status = RP_RECALL_LOOKUP;
    }
}

// the export of one solve's rows in ranked order, one lane per row; rows from n_rows on (all rows of a failed solve: n_rows = 0) are
// zero.  The two row structs differ in one byte: the world of a subgame row, padding (and a tag of 0) in a depth row.
__device__ __forceinline__ void nd_set_world(rp_nlhe_depth_row&, uint32_t) {}
__device__ __forceinline__ void nd_set_world(rp_nlhe_subgame_row& o, uint32_t world) { o.world = (uint8_t)world; }
template <class ROW, class R>
__device__ __forceinline__ void nd_export(ROW* out /* [rows_cap] */, uint32_t rows_cap, uint32_t n_rows, const R& rows, const uint16_t* rank) {
    for (uint32_t x = threadIdx.x; x < rows_cap; x += ND_BLOCK) {
        ROW& o = out[x];
        o = ROW{};
        if (x < n_rows) {
            const NdRow& row = rows.at(rank[x]);
            o.kind = (uint8_t)(row.present_kind >> 31);
            o.n_actions = (uint8_t)row.nch;
            nd_set_world(o, (row.present_kind >> ND_PRESENT_BITS) & 3u);
            o.present = row.present_kind & ((1u << ND_PRESENT_BITS) - 1u);
            o.past = row.past;
            o.choices = row.choices;
            for (uint32_t a = 0; a < row.nch; ++a) o.enc[a] = rp_encounter{row.w[a], row.r[a], row.p[a], row.v[a]};
        }
    }
}

__global__ __launch_bounds__(ND_BLOCK) void k_nl_depth(NlTable t, NlParams p, NdArgs q) {
    __shared__ NdShared sh;
    __shared__ NdNode nodes[ND_NODES];
    __shared__ NdInfo infos[ND_INFOS];
    __shared__ NdRow rows_lds[ND_ROWS_LDS];
    __shared__ uint32_t row_hash[ND_ROWS];
    __shared__ uint16_t s_rank[ND_ROWS];
    const NdRows rows{rows_lds, q.overflow + (size_t)blockIdx.x * ND_ROWS_OVF, row_hash};
    __shared__ float s_buf[NF_CELLS * NF_CHUNK / 2u];  // the rollouts' int16 buffer; between rollouts the sweeps' floats
    int16_t* s_won = reinterpret_cast<int16_t*>(s_buf);
    const uint32_t i = blockIdx.x, tid = threadIdx.x;
    const uint64_t id = q.first_id + i;  // wrapping

    if (tid == 0) {
        uint32_t st = nf_replay(q.entries[i], sh.pub, true);
        if (st == RP_RECALL_OK) st = nd_origin(q.origin, i, (int)RP_NLHE_DEPTH_ORIGIN_ENTRY, sh.pub.game.street(), &sh.origin);
        nd_begin(sh, st);
    }
    __syncthreads();
    for (uint32_t it = 0; it < q.iterations; ++it) {
        if (sh.status != RP_RECALL_OK) break;  // uniform: read after a barrier, written before the next
        __syncthreads();
        if (tid == 0) sh.status = nd_build(t, p, sh, nodes, infos, rows, it & 1u, rp_node_hash_tree(q.step_hash_tree, id * RP_NLHE_DEPTH_MAX_ITERATIONS + it));
        __syncthreads();
        if (sh.status != RP_RECALL_OK) break;
        nd_frontiers(t, p, sh, nodes, q.entries[i], id, it, q.bias, q.rollouts, q.step_hash_rollout, s_won);
        if (sh.status != RP_RECALL_OK) break;
        if (tid == 0) nd_updates<ND_ROWS, false>(t, sh, nodes, infos, rows, it, q.prior, s_buf);
        __syncthreads();
    }
    __syncthreads();
    if (sh.status == RP_RECALL_OK) nd_rank<nd_row_less>(rows, sh.n_rows, s_rank);
    __syncthreads();
    // the harvest
    if (tid == 0 && nd_result_head(q.results[i], sh, rows, s_rank, q.rollouts)) {
        rp_nlhe_depth_result& out = q.results[i];
        const G2 g = sh.pub.game;
        const int turn = g.turn();
        if (turn >= 0) {  // Harvest at DepthInfo::Game(info of the entry state)
            const NdEntry e = nd_entry(p, g, turn, sh.pub.path);
            float* r = sh.tmp[0];
            nd_entry_row(t, rows, sh.n_rows, sh.pub.path.tail, e, 0u, r, sh.tmpu, sh.tmp[1], sh.tmp[2]);
            const DistParams none{1.0f, 0.0f, 0.0f};
            policy_distribution<NLMC_A>((int)RP_DIST_ITERATED, none, r, e.nch, out.refined);
            float regret = 0.0f;
            for (uint32_t a = 0; a < e.nch; ++a) {
                regret += rp_maxf(r[a], 0.0f);
                out.visits[a] = sh.tmpu[a];
            }
            nd_result_entry(out, sh, e, regret);
        }
    }
    __syncthreads();
    if (q.rows) nd_export(q.rows + (size_t)i * q.rows_cap, q.rows_cap, sh.status == RP_RECALL_OK ? sh.n_rows : 0u, rows, s_rank);
}

}  // namespace rp

#endif
