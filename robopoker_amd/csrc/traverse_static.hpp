// traverse_static.hpp — Solver::batch (crates/mccfr/src/solver/solver.rs:225-250) for games whose ACTION tree does not
// depend on the cards: the traversal instantiated per game, as the reference's Solver<G> is monomorphised per CfrGame.
//
// k_traverse_lds walks each sampled tree with a per-lane DFS: 64 lanes = 64 different node sequences, half of the lanes
// idle on average (profiles/r01_mccfr_sq_counters.txt) and every step of a lane waits for the one before it.  In Kuhn and
// Leduc the sampled tree of ANY deal is a sub-tree of one fixed skeleton (the public betting tree with its chance nodes
// collapsed to the sampled outcome): what varies per tree is which skeleton nodes are live (the opponent's sampled
// actions), their infoset ids and their payoffs.  So the skeleton is a compile-time constant, the node loop is unrolled
// over it, every lane executes the same instruction stream (no divergence, no LDS, no stack), all per-node state sits in
// registers with static indices, and the loads of independent sub-trees overlap.
//
// A lane does not evaluate the whole skeleton, though.  What can never be live in the same tree is evaluated once (the
// packed-row variant; "mutually exclusive sub-trees" below): two sub-trees of the same shape below two edges of an OPPONENT
// node — the opponent samples one action — share one instance, built and valued for whichever the opponent's pick selects
// (Leduc: round 2 after check-check with round 2 after check-raise-call for walker 0, with round 2 after raise-call for
// walker 1: 29 of the 38 nodes are evaluated), and the two terminal children of an opponent node (fold / call) share one
// division.  Dead nodes are still masked out of the sums, and every live node sees the operations it saw unmerged, in the same
// order: the tables stay bit-identical (tests/test_gpu_mccfr_exclusive.py).  The child-record variant merges nothing.
//
// Same arithmetic as k_traverse_lds, operation for operation (TreeBuilder::build builder.rs:74-87,141-161 in pop-last
// order = pre-order with children in DESCENDING edge order; CfrFlow::dfs / recursed_value / ancestor_reach
// flow.rs:64-87,166-216): the Decisions are bit-identical (tests/test_gpu_mccfr.py::test_static_skeleton_equals_generic).
// Used when the game's tables match the skeleton node for node (skel_matches, checked once at rp_mccfr_create) and
// max_actions == 2; everything else takes k_traverse_lds.  PRUNED = false: external sampling (the walker expands every action).
// PRUNED = true: PrunableSampling / PluribusSampling (sample/pruning.rs:44-66, pluribus.rs:72-101) — a walker node's surviving
// edges come from the per-infoset keep masks (k_prepare_infos), the explore draw of (epoch, infoset, tree) and, for Pluribus,
// the edges whose child is a terminal node of the SKELETON (a compile-time fact); a pruned child is a dead skeleton node,
// exactly like an opponent action that was not sampled, and its edge takes no part in the node's value, regret or mask.
#pragma once

#include <type_traits>

#include "mccfr_kernels.hpp"
#include "mccfr_traverse.hpp"  // DevInfoTab, count_metrics, the draws

namespace rp {

enum : int { SK_CHANCE = 0, SK_P0 = 1, SK_P1 = 2, SK_TERMINAL = 3 };
#define SK_MAXN 48

struct Skeleton {
    int n = 0;
    int kind[SK_MAXN] = {};
    int parent[SK_MAXN] = {};  // -1 at the root
    int edge[SK_MAXN] = {};    // the action leading here; ignored below a chance node (the sampled outcome)
    int end[SK_MAXN] = {};     // last node of the sub-tree (pre-order: the sub-tree of s is [s, end[s]])
    constexpr int add(int k, int p, int e) {
        const int i = n++;
        kind[i] = k;
        parent[i] = p;
        edge[i] = e;
        end[i] = i;
        return i;
    }
    constexpr void close(int s) { end[s] = n - 1; }
};

// ---- Kuhn (crates/kuhn/src/game.rs:7-15,131-151): Start -> Dealt -> Open{Check{T, CheckBet{T,T}}, Bet{T,T}} ----
struct KuhnSkel {
    static constexpr Skeleton make() {
        Skeleton b;
        const int start = b.add(SK_CHANCE, -1, 0);
        const int dealt = b.add(SK_CHANCE, start, 0);
        const int open = b.add(SK_P0, dealt, 0);
        {  // children in descending edge order (the last child pushed is the first popped)
            const int bet = b.add(SK_P1, open, 1);
            b.add(SK_TERMINAL, bet, 1);
            b.add(SK_TERMINAL, bet, 0);
            b.close(bet);
            const int check = b.add(SK_P1, open, 0);
            const int cb = b.add(SK_P0, check, 1);
            b.add(SK_TERMINAL, cb, 1);
            b.add(SK_TERMINAL, cb, 0);
            b.close(cb);
            b.add(SK_TERMINAL, check, 0);
            b.close(check);
        }
        b.close(open);
        b.close(dealt);
        b.close(start);
        return b;
    }
};

// ---- Leduc (crates/leduc/src/game.rs:7-12,152-223): two betting rounds of the same shape, a Deal between them ----
struct LeducSkel {
    enum { OPEN, CHECKED, RAISED, CHECKRAISED };
    // one betting round below `parent`; `next` = 1: a closed round continues with the Deal and round 2, 0: it ends
    static constexpr void round(Skeleton& b, int parent, int edge, int spot, int next) {
        const int actor = (spot == OPEN || spot == CHECKRAISED) ? SK_P0 : SK_P1;
        const int s = b.add(actor, parent, edge);
        auto closes = [&](int e) {  // the child that closes the round: Deal -> round 2, or the showdown
            if (next) {
                const int deal = b.add(SK_CHANCE, s, e);
                round(b, deal, 0, OPEN, 0);
                b.close(deal);
            } else {
                b.add(SK_TERMINAL, s, e);
            }
        };
        switch (spot) {
            case OPEN:  // [Check, Raise]
                round(b, s, 1, RAISED, next);
                round(b, s, 0, CHECKED, next);
                break;
            case CHECKED:  // [Check -> closes, Raise]
                round(b, s, 1, CHECKRAISED, next);
                closes(0);
                break;
            default:  // RAISED / CHECKRAISED: [Fold, Call -> closes]
                closes(1);
                b.add(SK_TERMINAL, s, 0);
                break;
        }
        b.close(s);
    }
    static constexpr Skeleton make() {
        Skeleton b;
        const int start = b.add(SK_CHANCE, -1, 0);
        const int dealt = b.add(SK_CHANCE, start, 0);
        round(b, dealt, 0, OPEN, 1);
        b.close(dealt);
        b.close(start);
        return b;
    }
};

// ---- the packed rows of a skeleton (DevGame::rows) -------------------------------------------------------------------
// The nodes between a chance node c and the next chance nodes below it (c's GROUP: every node whose nearest chance ancestor is
// c) are reached under the same sampled outcomes, so the words the traversal needs of them sit side by side in one row per
// (c, outcomes on the path down to and including c's).  A decision node has one word (its infoset id), a chance node two (its
// state id = the hash key of its draw; chance_info for the reference-seed draw), a terminal node two (the two players' payoffs).
// The words are ordered by class — infoset ids, state ids, player 0's payoffs, player 1's payoffs, chance_infos — so that an
// instantiation for one walker / one draw kind finds what it uses in as few 16-byte slices as possible.  A row is padded to a
// power of two words (to a multiple of 32 above 32): 16-byte aligned slices that never straddle a 128-byte line.
struct RowLayout {
    int group[SK_MAXN] = {};   // node s: its nearest chance ancestor, -1 at the root
    int word[SK_MAXN] = {};    // node s: decision: infoset id; chance: state id; terminal: payoff of player 0
    int word2[SK_MAXN] = {};   // node s: chance: chance_info; terminal: payoff of player 1
    int words[SK_MAXN] = {};   // chance node c: words of its group
    int stride[SK_MAXN] = {};  // chance node c: words from one row to the next
};
constexpr RowLayout make_rows(const Skeleton& S) {
    RowLayout L;
    for (int s = 0; s < S.n; ++s) {
        int p = S.parent[s];
        while (p >= 0 && S.kind[p] != SK_CHANCE) p = S.parent[p];
        L.group[s] = p;
    }
    for (int c = 0; c < S.n; ++c) {
        if (S.kind[c] != SK_CHANCE) continue;
        int at = 0;
        for (int cls = 0; cls < 5; ++cls)
            for (int s = c + 1; s <= S.end[c]; ++s) {
                if (L.group[s] != c) continue;
                const bool dec = S.kind[s] == SK_P0 || S.kind[s] == SK_P1;
                if ((cls == 0 && dec) || (cls == 1 && S.kind[s] == SK_CHANCE) || (cls == 2 && S.kind[s] == SK_TERMINAL)) L.word[s] = at++;
                if ((cls == 3 && S.kind[s] == SK_TERMINAL) || (cls == 4 && S.kind[s] == SK_CHANCE)) L.word2[s] = at++;
            }
        L.words[c] = at;
        const int padded = (at + 3) & ~3;
        int st = 4;
        while (st < padded && st < 32) st *= 2;
        L.stride[c] = padded <= 32 ? st : (padded + 31) & ~31;
    }
    return L;
}

template <class G>
struct SkelOf {
    static constexpr Skeleton S = G::make();
    static constexpr RowLayout R = make_rows(S);
};

// does an instantiation (walker W, reference draws or not) use a word of slice k (words 4k .. 4k+3) of group c's row?
template <class G, int W, bool REF>
constexpr bool sk_slice_used(int c, int k) {
    constexpr Skeleton S = SkelOf<G>::S;
    constexpr RowLayout R = SkelOf<G>::R;
    for (int s = c + 1; s <= S.end[c]; ++s) {
        if (R.group[s] != c) continue;
        if (S.kind[s] == SK_TERMINAL) {
            if ((W == 0 ? R.word[s] : R.word2[s]) / 4 == k) return true;
        } else if (R.word[s] / 4 == k || (S.kind[s] == SK_CHANCE && REF && R.word2[s] / 4 == k)) {
            return true;
        }
    }
    return false;
}

// the skeleton child of node s along edge e is a terminal node?  (walker nodes: the Pluribus exemption, pluribus.rs:96)
template <class G>
constexpr bool sk_child_terminal(int s, int e) {
    for (int c = 0; c < SkelOf<G>::S.n; ++c)
        if (SkelOf<G>::S.parent[c] == s && SkelOf<G>::S.edge[c] == e) return SkelOf<G>::S.kind[c] == SK_TERMINAL;
    return false;
}

// ---- mutually exclusive sub-trees ---------------------------------------------------------------------------------------
// An opponent node samples exactly ONE action under every sampling scheme (pruning only removes further nodes), so two
// sub-trees whose lowest common ancestor is an opponent node of this walker are never live in the same tree.  Where two such
// sub-trees hang below chance nodes lo < hi, have the same shape (kinds, parents, edges) and the same row layout, the packed-row
// traversal evaluates ONE instance of them, at hi's place, for whichever the opponent's pick at the common ancestor selects:
// lo keeps only what its parent's row says about it (state id, fan-out) and its own liveness.
struct ExclPair {
    int lo = -1, hi = -1;  // the two chance nodes; -1: this skeleton / walker has no such pair
    int anc = -1;          // their lowest common ancestor, an opponent node
    int edge_lo = 0;       // anc's edge towards lo: pick[anc] == edge_lo selects lo, anything else hi
};
constexpr int sk_lca(const Skeleton& S, int a, int b) {  // pre-order: a is b's ancestor (or b) iff a <= b <= end[a]
    while (!(a <= b && b <= S.end[a])) a = S.parent[a];
    return a;
}
// the k-th opponent edge on the way from node n up to the root, as 2 * (opponent node) + edge; -1: there are fewer
constexpr int sk_outer_edge(const Skeleton& S, int opp, int n, int k) {
    for (; S.parent[n] >= 0; n = S.parent[n])
        if (S.kind[S.parent[n]] == opp && k-- == 0) return S.parent[n] * 2 + S.edge[n];
    return -1;
}
constexpr bool sk_same_shape(const Skeleton& S, const RowLayout& R, int x, int y) {
    if (S.end[x] - x != S.end[y] - y || R.group[x] != R.group[y]) return false;
    for (int i = 0; i <= S.end[x] - x; ++i) {
        if (S.kind[x + i] != S.kind[y + i]) return false;
        if (i && (S.parent[x + i] - x != S.parent[y + i] - y || S.edge[x + i] != S.edge[y + i])) return false;
        if (i && (R.word[x + i] != R.word[y + i] || R.word2[x + i] != R.word2[y + i])) return false;
        if (S.kind[x + i] == SK_CHANCE && (R.words[x + i] != R.words[y + i] || R.stride[x + i] != R.stride[y + i])) return false;
    }
    return true;
}
constexpr ExclPair sk_exclusive_pair(const Skeleton& S, const RowLayout& R, int walker) {
    const int wk = walker == 0 ? SK_P0 : SK_P1, opp = walker == 0 ? SK_P1 : SK_P0;
    ExclPair best;
    bool best_even = false;
    for (int x = 0; x < S.n; ++x) {
        if (S.kind[x] != SK_CHANCE) continue;
        for (int y = S.end[x] + 1; y < S.n; ++y) {
            if (S.kind[y] != SK_CHANCE) continue;
            const int a = sk_lca(S, x, y);
            if (S.kind[a] != opp || !sk_same_shape(S, R, x, y)) continue;
            // the merged instance hands its Decisions over at hi's place: ascending node order survives iff no walker node
            // between the two sub-trees can be live together with lo
            bool ordered = true;
            for (int n = S.end[x] + 1; n < y; ++n)
                if (S.kind[n] == wk && S.kind[sk_lca(S, x, n)] != opp) ordered = false;
            if (!ordered) continue;
            // prefer partners with equally many opponent edges above them (ancestor_reach: no padding factor)
            int kx = 0, ky = 0;
            while (sk_outer_edge(S, opp, x, kx) >= 0) ++kx;
            while (sk_outer_edge(S, opp, y, ky) >= 0) ++ky;
            if (best.lo >= 0 && (best_even || kx != ky)) continue;
            int c = x;
            while (S.parent[c] != a) c = S.parent[c];
            best.lo = x;
            best.hi = y;
            best.anc = a;
            best.edge_lo = S.edge[c];
            best_even = kx == ky;
        }
    }
    return best;
}
// MERGE = false: nothing is merged (the child-record variant, the unmerged cross-check)
template <class G, int W, bool MERGE>
struct SkelExcl {
    using SK = SkelOf<G>;
    static constexpr ExclPair X = MERGE ? sk_exclusive_pair(SK::S, SK::R, W) : ExclPair{};
    static constexpr int LO = X.lo, HI = X.hi, SHIFT = X.hi - X.lo;
    static constexpr bool in_lo(int n) { return LO >= 0 && LO <= n && n <= SK::S.end[LO]; }
    static constexpr bool in_hi(int n) { return HI >= 0 && HI <= n && n <= SK::S.end[HI]; }
    static constexpr bool skipped(int n) { return in_lo(n) && n != LO; }  // never built: its partner in hi's sub-tree stands for it
    static constexpr int at(int n) { return in_lo(n) ? n + SHIFT : n; }   // where the traversal keeps what it knows of node n
    static constexpr bool both_below(int j) { return LO >= 0 && j < LO && HI <= SK::S.end[j]; }
};
// an opponent node whose children are all terminal: only the sampled child can be live, one division serves the pair
template <class G>
constexpr bool sk_leaf_pair(int s) {
    int kids = 0;
    for (int c = 0; c < SkelOf<G>::S.n; ++c)
        if (SkelOf<G>::S.parent[c] == s) {
            if (SkelOf<G>::S.kind[c] != SK_TERMINAL) return false;
            ++kids;
        }
    return kids == 2;
}
template <class G>
constexpr int sk_child(int s, int e) {
    for (int c = 0; c < SkelOf<G>::S.n; ++c)
        if (SkelOf<G>::S.parent[c] == s && SkelOf<G>::S.edge[c] == e) return c;
    return -1;
}

static_assert(SkelOf<KuhnSkel>::S.n == 11, "Kuhn: two deals, four decision nodes, five terminals");
static_assert(SkelOf<LeducSkel>::S.n == 38, "Leduc: two deals, 4 + 3 x 4 decision nodes, three board draws, 2 + 3 x 5 terminals");
static_assert(SkelOf<LeducSkel>::S.end[0] == 37 && SkelOf<LeducSkel>::S.kind[2] == SK_P0, "pre-order, the first decision is P0's");
static_assert(SkelOf<LeducSkel>::R.words[0] == 2 && SkelOf<LeducSkel>::R.words[1] == 14 && SkelOf<LeducSkel>::R.stride[1] == 16,
              "Leduc: the second deal alone below the first; round 1 = 4 infosets, 3 board deals, 2 folds in a 64-byte row");
static_assert(SkelOf<KuhnSkel>::R.words[1] == 14 && SkelOf<KuhnSkel>::R.stride[1] == 16, "Kuhn: 4 infosets, 5 terminals");

static_assert(SkelExcl<LeducSkel, 0, true>::LO == 17 && SkelExcl<LeducSkel, 0, true>::HI == 28 && SkelExcl<LeducSkel, 0, true>::X.anc == 15 &&
                  SkelExcl<LeducSkel, 0, true>::X.edge_lo == 1,
              "Leduc, walker 0: CHECKED is the opponent's, so round 2 after check-raise-call and round 2 after check-check never meet");
static_assert(SkelExcl<LeducSkel, 1, true>::LO == 4 && SkelExcl<LeducSkel, 1, true>::HI == 28 && SkelExcl<LeducSkel, 1, true>::X.anc == 2 &&
                  SkelExcl<LeducSkel, 1, true>::X.edge_lo == 1,
              "Leduc, walker 1: OPEN is the opponent's; round 2 after raise-call pairs with the one after check-check (one opponent edge each)");
static_assert(SkelExcl<KuhnSkel, 0, true>::LO < 0 && SkelExcl<KuhnSkel, 1, true>::LO < 0, "Kuhn: one deal, nothing to pair");
static_assert(SkelExcl<LeducSkel, 0, false>::LO < 0 && !SkelExcl<LeducSkel, 0, false>::skipped(20) && SkelExcl<LeducSkel, 0, false>::at(20) == 20,
              "unmerged: every node stands for itself");
static_assert(sk_leaf_pair<LeducSkel>(6) && sk_leaf_pair<LeducSkel>(10) && !sk_leaf_pair<LeducSkel>(3) && sk_leaf_pair<KuhnSkel>(3) &&
                  sk_leaf_pair<KuhnSkel>(7),
              "fold / call below a raise: RAISED', CHECKRAISED' and Kuhn's Bet, CheckBet");

// compile-time loops: f(std::integral_constant<int, I>) for I = LO .. HI-1, ascending / descending
template <int I, int HI, class F>
__device__ __forceinline__ void sk_for(F&& f) {
    if constexpr (I < HI) {
        f(std::integral_constant<int, I>{});
        sk_for<I + 1, HI>(f);
    }
}
template <int I, int LO, class F>
__device__ __forceinline__ void sk_for_down(F&& f) {  // I = HI-1 down to LO
    if constexpr (I >= LO) {
        f(std::integral_constant<int, I>{});
        sk_for_down<I - 1, LO>(f);
    }
}

// The traversal of one tree by one lane.  W = the walker (epoch % 2).  `present` = this lane has a tree (the ragged last
// workgroup).  on_built(info_of, live_of) runs once the tree is sampled — before any value is computed — with two callables
// over the skeleton's node index; on_decision(j, info, regret0, regret1, sigma0, sigma1, payoff) once per LIVE walker node,
// ascending node index (= the order of Tree::partition's spans).  Returns the number of nodes of the sampled tree.
// on_decision's `mask`: the expanded edges (3 under external sampling).
// REF: the draws come from the reference's own chain (rp_rng_kind RP_RNG_REFERENCE, mccfr_kernels.hpp d_draw_*).
// ROWS: what a node holds comes from the packed rows (DevGame::rows), one row per chance outcome; else from the child records
// (DevGame::kids), one dependent load per node.  The kernels branch once, on g.rows (wave-uniform), around the whole traversal:
// with the choice made per load, the two variants' loads are merged behind the join and lose their width.
template <class G, int W, bool PRUNED, bool REF, bool ROWS, class OnBuilt, class OnDecision>
__device__ __forceinline__ uint32_t static_traverse(const DevGame& g, const DevInfoTab& it, const StepParams& p, uint64_t tree_id,
                                                    bool present, OnBuilt&& on_built, OnDecision&& on_decision) {
    using SK = SkelOf<G>;
    using EX = SkelExcl<G, W, ROWS>;  // the packed-row variant merges the exclusive pair and the leaf pairs; the child-record one nothing
    constexpr int N = SK::S.n;
    constexpr int K_WALKER = W == 0 ? SK_P0 : SK_P1;
    constexpr int K_OPP = W == 0 ? SK_P1 : SK_P0;

    // ---- TreeBuilder::build over the skeleton ----------------------------------------------------------------------
    uint32_t ry[N], rz[N], rw[N];  // the node's words: infoset id / chance_info, child offset (the child-record chain only), state id
    uint32_t pay[N];               // terminal: the walker's payoff (bits)
    uint32_t nout[N];              // chance: the number of outcomes
    uint32_t ridx[N];              // chance: the row index of its group = the outcomes on the path, mixed radix, root first
    uint32_t pick[N];              // chance: the sampled outcome; opponent: the sampled action; walker (PRUNED): the surviving edges
    bool live[N];
    float sg0[N], sg1[N];  // walker: the sigmas of the node's two edges
    // opponent: (sigma, q) of the SAMPLED edge alone.  The other edge leads to dead nodes only, and what a dead node computes is dropped
    // by a select on live[], never by a multiplication (the sweeps, the leaf pairs; ancestor_reach is read under live[j], whose
    // chain holds sampled edges only): the dead sub-tree carries the wrong factor and nothing reads it
    float sgp[N], qp[N];
    // the exclusive pair: the opponent's pick selects lo, and the two chance nodes' own liveness (live[hi] becomes the merged one)
    bool sel_lo = false, live_lo = false, live_hi = false;
    // every draw of this tree: rp_node_hash(seed, epoch, tree, key) with the (seed, epoch, tree) part hashed once
    const uint64_t th = rp_node_hash_tree(rp_node_hash_step(p.seed, p.epoch), tree_id);
    const char* const irows = reinterpret_cast<const char*>(it.row2);
    ry[0] = g.root_rec.y;
    rz[0] = g.root_rec.z;
    rw[0] = g.root_rec.w;
    live[0] = present;
    nout[0] = ROWS ? g.row_fan[0] : (g.root_rec.x >> 8) & 0xffu;
    sk_for<0, N>([&](auto I) __attribute__((always_inline)) {
        constexpr int s = I;
        constexpr int par = SK::S.parent[s];
        if constexpr (EX::skipped(s)) return;  // inside lo: its partner inside hi is built for both
        if constexpr (par >= 0) {
            if constexpr (!ROWS) {
                uint32_t k = (uint32_t)SK::S.edge[s];
                if constexpr (SK::S.kind[par] == SK_CHANCE) k = pick[par];
                const uint4 r = g.kids[rz[par] + k];
                ry[s] = r.y;
                rz[s] = r.z;
                rw[s] = r.w;
                pay[s] = W == 0 ? r.y : r.z;
                nout[s] = (r.x >> 8) & 0xffu;
            } else if constexpr (SK::S.kind[par] == SK_CHANCE) {  // the first node of par's group: the whole row, by slices
                constexpr int c = par;
                constexpr int up = SK::R.group[c];
                if constexpr (up >= 0) ridx[c] = ridx[up] * nout[c] + pick[c];
                else ridx[c] = pick[c];
                // one scalar base, one 32-bit lane offset, the slices at immediate offsets
                const char* row = reinterpret_cast<const char*>(g.rows + g.row_base[c]);
                uint32_t off = ridx[c] * (uint32_t)(SK::R.stride[c] * 4);
                if constexpr (EX::in_hi(c)) {  // the selected alternative's table (same layout: sk_same_shape)
                    row = reinterpret_cast<const char*>(g.rows);
                    const uint32_t base_lo = g.row_base[c - EX::SHIFT], base_hi = g.row_base[c];
                    off += (sel_lo ? base_lo : base_hi) * 16u;
                }
                constexpr int NS = (SK::R.words[c] + 3) / 4;
                uint32_t w[NS * 4];
                sk_for<0, NS>([&](auto K) __attribute__((always_inline)) {
                    constexpr int k = K;
                    if constexpr (sk_slice_used<G, W, REF>(c, k)) {
                        const uint4 v = *reinterpret_cast<const uint4*>(row + off + (uint32_t)(k * 16));
                        w[4 * k + 0] = v.x;
                        w[4 * k + 1] = v.y;
                        w[4 * k + 2] = v.z;
                        w[4 * k + 3] = v.w;
                    }
                });
                sk_for<s, SK::S.end[c] + 1>([&](auto M) __attribute__((always_inline)) {
                    constexpr int m = M;
                    if constexpr (SK::R.group[m] == c) {
                        if constexpr (SK::S.kind[m] == SK_TERMINAL) {
                            pay[m] = w[W == 0 ? SK::R.word[m] : SK::R.word2[m]];
                        } else if constexpr (SK::S.kind[m] == SK_CHANCE) {
                            rw[m] = w[SK::R.word[m]];
                            if constexpr (REF) ry[m] = w[SK::R.word2[m]];
                            nout[m] = g.row_fan[m];
                            if constexpr (EX::in_hi(c)) {
                                const uint32_t fan_lo = g.row_fan[m - EX::SHIFT];
                                nout[m] = sel_lo ? fan_lo : nout[m];
                            }
                        } else {
                            ry[m] = w[SK::R.word[m]];
                        }
                    }
                });
            }
            if constexpr (SK::S.kind[par] == K_OPP) live[s] = live[par] && pick[par] == (uint32_t)SK::S.edge[s];
            else if constexpr (PRUNED && SK::S.kind[par] == K_WALKER) live[s] = live[par] && ((pick[par] >> SK::S.edge[s]) & 1u);
            else live[s] = live[par];
        }
        if constexpr (s == EX::LO) return;  // drawn at hi, if it is the selected one
        if constexpr (s == EX::HI) {  // from here on hi stands for the alternative the opponent's pick leads to (both dead: either)
            sel_lo = pick[EX::X.anc] == (uint32_t)EX::X.edge_lo;
            // (selects between values, never between array elements: the arrays must stay in registers)
            live_lo = live[EX::LO];
            live_hi = live[s];
            const uint32_t key_lo = rw[EX::LO], key_hi = rw[s], fan_lo = nout[EX::LO], fan_hi = nout[s];
            rw[s] = sel_lo ? key_lo : key_hi;
            nout[s] = sel_lo ? fan_lo : fan_hi;
            if constexpr (REF) {
                const uint32_t ci_lo = ry[EX::LO], ci_hi = ry[s];
                ry[s] = sel_lo ? ci_lo : ci_hi;
            }
            live[s] = sel_lo ? live_lo : live_hi;
        }
        if constexpr (SK::S.kind[s] == SK_CHANCE) {  // SamplingScheme::sample at a chance node: uniform (external.rs:41-64)
            // ry = chance_info (read under REF only); 0: the root deal (thread RNG in the reference)
            if (REF && ry[s]) pick[s] = rp_ref_draw_range(rp_ref_seed_finish(&p.ref_chance[ry[s] - 1u], tree_id), nout[s]);
            else pick[s] = rp_pick_uniform(rp_node_hash_key(th, 0x80000000ull | rw[s]), nout[s]);
        } else if constexpr (SK::S.kind[s] == SK_P0 || SK::S.kind[s] == SK_P1) {
            const uint32_t info = ry[s];
            const char* const ir = irows + info * 32u;  // DevInfoTab::row2: {sigma0, sigma1, q0, q1, total, cum0, keep, 0}
            if constexpr (SK::S.kind[s] == K_OPP) {  // WeightedIndex over max(q, EPSILON): two actions = one threshold
                const float4 f = *reinterpret_cast<const float4*>(ir);
                const float2 tc = *reinterpret_cast<const float2*>(ir + 16);  // (total, cum[0])
                const float x = REF ? rp_ref_draw_weight(rp_ref_seed_finish(&p.ref_info[info], tree_id), tc.x)
                                    : rp_u01(rp_node_hash_key(th, info)) * tc.x;
                const bool e1 = tc.y <= x;
                pick[s] = e1 ? 1u : 0u;
                sgp[s] = e1 ? f.y : f.x;
                qp[s] = e1 ? f.w : f.z;
            } else {  // a walker node's q take no part in anything
                const float2 f = *reinterpret_cast<const float2*>(ir);
                sg0[s] = f.x;
                sg1[s] = f.y;
            }
            if constexpr (SK::S.kind[s] == K_WALKER && PRUNED) {  // SamplingScheme::sample at a walker node (d_sample_mask_tab: same draw, same masks)
                uint32_t mask = 3u;
                bool prune = true;
                if (p.S == RP_SAMPLING_PLURIBUS)
                    prune = p.epoch >= p.prune_warmup &&
                            !((REF ? rp_ref_draw_f32(rp_ref_seed_finish(&p.ref_info[info], tree_id)) : rp_u01(rp_node_hash_key(th, info))) <
                              p.prune_explore);
                if (prune) {
                    mask = *reinterpret_cast<const uint32_t*>(ir + 24) & 3u;
                    if (p.S == RP_SAMPLING_PLURIBUS)
                        mask |= (sk_child_terminal<G>(s, 0) ? 1u : 0u) | (sk_child_terminal<G>(s, 1) ? 2u : 0u);
                    mask = mask ? mask : 3u;  // pruning.rs:64, pluribus.rs:99
                }
                pick[s] = mask;
            }
        }
    });

    // ---- Tree::partition + CfrFlow::dfs per walker decision node (tree.rs:88-98, flow.rs:64-87) ---------------------
    // A node of lo's sub-tree is counted, listed and valued through its partner in hi's: at most one of the two is live.
    uint32_t nn = 0;
    sk_for<0, N>([&](auto I) __attribute__((always_inline)) {
        if constexpr (!EX::in_lo(decltype(I)::value)) nn += live[decltype(I)::value] ? 1u : 0u;
    });
    on_built([&](auto I) __attribute__((always_inline)) { return ry[EX::at(decltype(I)::value)]; },
             [&](auto I) __attribute__((always_inline)) { return EX::in_lo(decltype(I)::value) ? false : live[decltype(I)::value]; });
    sk_for<0, N>([&](auto J) __attribute__((always_inline)) {
        constexpr int j = J;
        if constexpr (SK::S.kind[j] == K_WALKER && !EX::in_lo(j)) {
            constexpr int E = SK::S.end[j];
            // both alternatives below j: their reach products come down both paths, the merged instance is entered at hi with the
            // selected pair and its sum goes up to lo's parent under lo's liveness, to hi's under hi's.  Only one of them below
            // j (or j inside hi): j live means that one is the selected one.
            constexpr bool BOTH = EX::both_below(j);
            float rel[N], smp[N], acc[N], tv[2] = {0.0f, 0.0f};
            float rel_lo = 1.0f, smp_lo = 1.0f;
            // top-down over the sub-tree: reach products from j's children (flow.rs:195-212); a leaf hands its value to its
            // parent right here, an internal node starts its sum at 0 (the two-children argument of k_traverse_lds)
            sk_for<j + 1, E + 1>([&](auto Nn) __attribute__((always_inline)) {
                constexpr int n = Nn;
                constexpr int par = SK::S.parent[n];
                constexpr int e = SK::S.edge[n];
                // where node n and its parent keep their state.  A node of lo's sub-tree reads and writes its partner's slots in
                // hi's: for a root on lo's path (not BOTH) hi's slots hold the lo alternative whenever the root is live, so the
                // sweep runs over lo's nodes with hi's storage.  lo's own parent lies outside the pair and stands for itself.
                constexpr int an = EX::at(n), ap = n == EX::LO ? par : EX::at(par);
                if constexpr (BOTH && EX::skipped(n)) return;
                float r = 1.0f, sm = 1.0f;
                if constexpr (ROWS && SK::S.kind[n] == SK_TERMINAL && SK::S.kind[par] == K_OPP && sk_leaf_pair<G>(par)) {
                    // the opponent's two terminal children: the unsampled one is dead, so the sampled one's r / sm * payoff is the
                    // only value that enters the parent's sum — computed with the sampled edge's factors and payoff, added once
                    if constexpr (e == 1) {
                        const bool e1 = pick[ap] != 0u;
                        constexpr int sib = EX::at(sk_child<G>(par, 0));
                        const uint32_t p_0 = pay[sib], p_1 = pay[an];
                        r = rel[ap] * sgp[ap];
                        sm = smp[ap] * qp[ap];
                        const float v = r / sm * rp_u2f(e1 ? p_1 : p_0);
                        acc[ap] = live[ap] ? acc[ap] + v : acc[ap];
                    }
                    return;
                }
                if constexpr (par != j) {
                    r = rel[ap];
                    sm = smp[ap];
                    if constexpr (SK::S.kind[par] == K_WALKER) r = r * (e ? sg1[ap] : sg0[ap]);
                    if constexpr (SK::S.kind[par] == K_OPP) {  // the sampled edge's: n is dead if it hangs below the other
                        r = r * sgp[ap];
                        sm = sm * qp[ap];
                    }
                }
                if constexpr (BOTH && n == EX::LO) {  // kept for hi
                    rel_lo = r;
                    smp_lo = sm;
                    return;
                }
                if constexpr (BOTH && n == EX::HI) {
                    r = sel_lo ? rel_lo : r;
                    sm = sel_lo ? smp_lo : sm;
                }
                if constexpr (SK::S.kind[n] == SK_TERMINAL) {
                    const float v = r / sm * rp_u2f(pay[an]);
                    if constexpr (par == j) tv[e] = v;
                    else acc[ap] = live[an] ? acc[ap] + v : acc[ap];
                } else {
                    rel[an] = r;
                    smp[an] = sm;
                    acc[an] = 0.0f;
                }
            });
            // bottom-up: the internal nodes' sums, descending node index (node.rs:103-107)
            sk_for_down<E, j + 1>([&](auto Nn) __attribute__((always_inline)) {
                constexpr int n = Nn;
                constexpr int par = SK::S.parent[n];
                constexpr int an = EX::at(n), ap = n == EX::LO ? par : EX::at(par);  // as in the sweep above
                if constexpr (BOTH && EX::skipped(n)) return;  // summed when hi's sub-tree came by
                if constexpr (SK::S.kind[n] != SK_TERMINAL) {
                    bool lv = live[an];
                    if constexpr (n == EX::LO) lv = live_lo;
                    if constexpr (n == EX::HI) lv = live_hi;
                    if constexpr (par == j) tv[SK::S.edge[n]] = acc[an];
                    else acc[ap] = lv ? acc[ap] + acc[an] : acc[ap];
                }
            });
            // ancestor_reach (flow.rs:166-174): the opponent's edges on the way up
            float cf = 1.0f, sm_ = 1.0f;
            sk_for<0, N>([&](auto Q) __attribute__((always_inline)) {
                // ancestors of j in the order j, parent(j), ...: node index DESCENDS along the chain, so visit candidates from
                // j downwards and keep those on the chain
                constexpr int n = j - decltype(Q)::value;
                if constexpr (n > 0 && !(EX::in_hi(j) && n <= EX::HI)) {
                    // is n on the parent chain of j (n == j or an ancestor)?  pre-order: n <= j <= end[n]
                    if constexpr (n <= j && j <= SK::S.end[n]) {
                        constexpr int par = SK::S.parent[n];
                        if constexpr (SK::S.kind[par] == K_OPP) {  // j live: its chain holds sampled edges only
                            cf = cf * sgp[par];
                            sm_ = sm_ * qp[par];
                        }
                    }
                }
            });
            if constexpr (EX::in_hi(j)) {
                // j inside the merged instance: from hi upwards the chain is the selected alternative's, edge by edge in the same
                // order; the shorter chain is padded with the factor 1 (exact)
                sk_for<0, N>([&](auto Q) __attribute__((always_inline)) {
                    constexpr int fl = sk_outer_edge(SK::S, K_OPP, EX::LO, decltype(Q)::value);
                    constexpr int fh = sk_outer_edge(SK::S, K_OPP, EX::HI, decltype(Q)::value);
                    if constexpr (fl >= 0 || fh >= 0) {
                        float cl = 1.0f, ql = 1.0f, ch = 1.0f, qh = 1.0f;
                        // j live: the selected alternative is live, and the edges above it are sampled ones
                        if constexpr (fl >= 0) {
                            cl = sgp[fl >> 1];
                            ql = qp[fl >> 1];
                        }
                        if constexpr (fh >= 0) {
                            ch = sgp[fh >> 1];
                            qh = qp[fh >> 1];
                        }
                        cf = cf * (sel_lo ? cl : ch);
                        sm_ = sm_ * (sel_lo ? ql : qh);
                    }
                });
            }
            const float reach = cf / sm_;
            const float u0 = reach * tv[0], u1 = reach * tv[1];
            if constexpr (!PRUNED) {
                float ev = 0.0f;
                ev += sg0[j] * u0;
                ev += sg1[j] * u1;
                const float payoff = 0.0f + ev;
                const float g0 = 0.0f + (u0 - ev), g1 = 0.0f + (u1 - ev);
                if (live[j]) on_decision(J, ry[j], g0, g1, sg0[j], sg1[j], payoff, 3u);
            } else {  // only the expanded edges enter the node's value and receive a regret (k_traverse_lds, the same order)
                const uint32_t mask = pick[j];
                float ev = 0.0f;
                if (mask & 1u) ev += sg0[j] * u0;
                if (mask & 2u) ev += sg1[j] * u1;
                const float payoff = 0.0f + ev;
                const float g0 = (mask & 1u) ? 0.0f + (u0 - ev) : 0.0f, g1 = (mask & 2u) ? 0.0f + (u1 - ev) : 0.0f;
                if (live[j]) on_decision(J, ry[j], g0, g1, sg0[j], sg1[j], payoff, mask);
            }
        }
    });
    return nn;
}

// Decisions to HBM (DevDecisions), for the ordered update, the sorted large-game path and the debugging views.
// One lane per tree, 256 trees per workgroup, no LDS.
template <class G, int W, bool PRUNED, bool REF>
__global__ __launch_bounds__(256) void k_traverse_static(DevGame g, DevInfoTab it, DevDecisions dc, StepParams p) {
    const uint32_t lane = blockIdx.x * 256u + threadIdx.x;
    if (lane >= p.batch) return;
    const size_t D = dc.stride;
    uint32_t ndec = 0;
    auto on_built = [](auto, auto) __attribute__((always_inline)) {};
    auto on_decision =
        [&](auto, uint32_t info, float g0, float g1, float s0, float s1, float payoff, uint32_t mask) __attribute__((always_inline)) {
            const uint32_t slot = ndec;
            dc.regret[((size_t)slot * 2u + 0u) * D + lane] = g0;
            dc.regret[((size_t)slot * 2u + 1u) * D + lane] = g1;
            dc.policy[((size_t)slot * 2u + 0u) * D + lane] = s0;
            dc.policy[((size_t)slot * 2u + 1u) * D + lane] = s1;
            dc.info[(size_t)slot * D + lane] = info;
            dc.mask[(size_t)slot * D + lane] = mask;
            dc.payoff[(size_t)slot * D + lane] = payoff;
            if (dc.slotmap) dc.slotmap[(size_t)info * D + lane] = (uint8_t)(slot + 1u);
            ndec += 1u;
        };
    const uint64_t tree_id = p.tree_base + lane;
    const uint32_t nn = g.rows ? static_traverse<G, W, PRUNED, REF, true>(g, it, p, tree_id, true, on_built, on_decision)
                               : static_traverse<G, W, PRUNED, REF, false>(g, it, p, tree_id, true, on_built, on_decision);
    dc.ndec[lane] = (uint8_t)ndec;
    count_metrics(p, nn, ndec, 0u);
}

// Composed update, small games: the traversal AND the block maps of its 256-tree chunk in one kernel — the Decisions never
// reach HBM.  What k_chunk_maps does with the Decisions it reads back (per-infoset, tree-ordered lists by LDS bitmap +
// prefix popcount; one sequential composition per (infoset, cell) from the identity: include/rp_mi355x.h "Composed
// update") happens here on the values as they are produced: the lists' places are known once the trees are sampled
// (on_built), each Decisions drops its three values (two regret deltas, the payoff) at its place in LDS — its two weight deltas
// are the same for every entry of the infoset's list (the infoset's sigmas, the epoch): the first entry leaves the two sigmas in
// `wsig`, and the chain's lane makes the delta of them once —
// and the chains of ALL cells run side by side, one thread per (infoset, cell).  Same lists, same order, same operations
// as k_chunk_maps: the chunk's row of block maps (bmap_index) is bit-identical (tests/test_gpu_mccfr.py).
// A chain is sequential and as long as its list (a root infoset meets a third of the chunk's trees, a river infoset a few):
// the (infoset, cell) tasks are handed out in descending order of list length (a counting sort by log2 class), so the 64
// chains of a wave have similar lengths instead of every wave waiting for one long chain.  Only the walker's infosets have
// lists: `order` holds those alone (rank_count[W] entries), and pre / lcount / lbase are written for them alone.
// LDS (dynamic): bits u32[NI][8] | lcount u32[NI] | lbase u32[NI] | pre u16[NI][8] | order u16[NI + (NI & 1)] | wsig f32[NI][2]
//                | vals f32[3][maxdec * 256 + lpad]
//                | (PRUNED) lmask u32[maxdec * 256]: the expanded edges of every list entry — a regret cell skips the entries
//                  whose edge was pruned (no touch at all: a touch would apply the discount), as k_chunk_maps<true> does
// Workgroups per CU the registers are allocated for (__launch_bounds__).  With three value cells five workgroups fit in LDS (Leduc,
// external sampling: 26 436 B each), and the kernel is a latency kernel: counter draws under external sampling take the 96 VGPRs of five
// waves per SIMD, at the price of 14 - 20 spilled registers (60 - 84 B of scratch), and run 8 % faster for it than at four without scratch
// (DESIGN.md §3 "Five workgroups per CU").  The pruned samplings and the reference draws spill hundreds of bytes at 128 already: four.
constexpr int tm_workgroups(bool pruned, bool ref) { return (!pruned && !ref) ? 5 : 4; }
template <class G, int W, bool PRUNED, bool REF>
__global__ __launch_bounds__(256, tm_workgroups(PRUNED, REF)) void k_traverse_maps_static(DevGame g, DevInfoTab it, StepParams p, Map* bmaps,
                                                              uint32_t maxdec, uint32_t lpad) {
    extern __shared__ __attribute__((aligned(16))) uint32_t tm_lds[];
    static_assert(SM_WORDS == 8u, "a bitmap row is two 16-byte LDS reads, its prefix counts two 8-byte writes");
    const uint32_t NI = g.n_infos, chunk = blockIdx.x, lt = threadIdx.x;
    // the lists are built by wavefront 0, lane r those of the walker's infoset of rank r (traverse_maps_fused: at most 64 ranks); the
    // infoset is fetched here, long before its use
    const uint32_t nr = g.rank_count[W];
    const uint32_t my_info = lt < nr ? g.rank_info[(size_t)W * g.rank_max + lt] : 0u;
    uint32_t* bits = tm_lds;
    uint32_t* lcount = bits + NI * SM_WORDS;
    uint32_t* lbase = lcount + NI;
    uint16_t* pre = reinterpret_cast<uint16_t*>(lbase + NI);
    uint16_t* order = pre + NI * SM_WORDS;
    float* wsig = reinterpret_cast<float*>(order + NI + (NI & 1u));
    float* vals = wsig + 2u * NI;
    // places per cell.  The chains of an infoset read vals[k L + base + e], k = 0 .. 2, in the same instruction (a weight lane reads its
    // regret neighbour's word: a broadcast): with L a multiple of 32 the three share a bank (a 3-way conflict at every step); lpad = 7
    // words moves the cells apart (measured round 4 with five cells, profiles/r04_optin_ab.json: pads 0 / 3 / 7 / 13 within 1 % of
    // each other — the conflicts were not the limiter)
    const uint32_t L = maxdec * 256u + lpad;
    uint32_t* lmask = reinterpret_cast<uint32_t*>(vals + 3u * L);
    for (uint32_t e = lt; e < NI * SM_WORDS; e += 256u) bits[e] = 0;
    __syncthreads();
    const uint32_t lane = chunk * 256u + lt;
    uint32_t ndec = 0;
    auto on_built =
        [&](auto info_of, auto live_of) __attribute__((always_inline)) {
            sk_for<0, SkelOf<G>::S.n>([&](auto J) __attribute__((always_inline)) {
                if constexpr (SkelOf<G>::S.kind[decltype(J)::value] == (W == 0 ? SK_P0 : SK_P1)) {
                    if (live_of(J)) atomicOr(&bits[info_of(J) * SM_WORDS + (lt >> 5)], 1u << (lt & 31u));
                }
            });
            __syncthreads();
            // wavefront 0, everything in registers: the prefix counts of the lane's bitmap row (list_prefix), the lists' bases by a
            // scan across the lanes, the places in `order` by one ballot per length class.  The other wavefronts wait at the barrier
            if (lt < 64u) {
                const bool mine = lt < nr;
                // the row in halves, each half's prefix counts stored before the next is read: the sampled tree is live in registers
                uint2* const pw = reinterpret_cast<uint2*>(pre + my_info * SM_WORDS);
                const uint4 lo = *reinterpret_cast<const uint4*>(bits + my_info * SM_WORDS);
                const uint32_t p1 = __popc(lo.x), p2 = p1 + __popc(lo.y), p3 = p2 + __popc(lo.z), p4 = p3 + __popc(lo.w);
                if (mine) pw[0] = make_uint2(p1 << 16, p2 | p3 << 16);
                const uint4 hi = *reinterpret_cast<const uint4*>(bits + my_info * SM_WORDS + 4u);
                const uint32_t p5 = p4 + __popc(hi.x), p6 = p5 + __popc(hi.y), p7 = p6 + __popc(hi.z);
                if (mine) pw[1] = make_uint2(p4 | p5 << 16, p6 | p7 << 16);
                const uint32_t run = mine ? p7 + __popc(hi.w) : 0u;
                uint32_t incl = run;
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t o = __shfl_up(incl, d, 64);
                    if ((int)lt >= d) incl += o;
                }
                // long lists first: classes by bit length, 9 (a list of all CH_TREES trees) down to 0 (empty); ascending rank within one
                const uint32_t len = run ? 32u - (uint32_t)__builtin_clz(run) : 0u;
                uint32_t place = 0, at = 0;
                for (uint32_t k = 10u; k-- > 0u;) {
                    const unsigned long long m = __ballot(mine && len == k);
                    if (len == k) place = at + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    at += (uint32_t)__popcll(m);
                }
                if (mine) {
                    lcount[my_info] = run;
                    lbase[my_info] = incl - run;
                    // the infoset and its rank among its player's infosets (bmap_index) share the entry, 8 bits each: the launch is
                    // made for at most CH_THREADS infosets (traverse_maps_fused)
                    order[place] = (uint16_t)(my_info | lt << 8);
                }
            }
            __syncthreads();
        };
    // the sigmas of a Decisions are row2[info].x/.y, the same two floats for every entry of the infoset's list: the first entry alone
    // keeps them, for the weight chains
    auto on_decision =
        [&](auto, uint32_t info, float g0, float g1, float s0, float s1, float payoff, uint32_t mask) __attribute__((always_inline)) {
            const uint32_t at = list_rank(bits, pre, info, lt), pos = lbase[info] + at;
            if (at == 0u) {
                wsig[2u * info] = s0;
                wsig[2u * info + 1u] = s1;
            }
            if constexpr (PRUNED) lmask[pos] = mask;
            vals[pos] = g0;
            vals[L + pos] = g1;
            vals[2u * L + pos] = payoff;
            ndec += 1u;
        };
    const uint64_t tree_id = p.tree_base + lane;
    const bool present = lane < p.batch;
    const uint32_t nn = g.rows ? static_traverse<G, W, PRUNED, REF, true>(g, it, p, tree_id, present, on_built, on_decision)
                               : static_traverse<G, W, PRUNED, REF, false>(g, it, p, tree_id, present, on_built, on_decision);
    __syncthreads();
    // the chains of an infoset's list: two regret cells, two weight cells, the payoff sum.  Both discounts are uniform over the grid:
    // branched on once, around the whole phase.  A weight cell's delta is the same for every entry of its list — weight_delta of the
    // infoset's sigma, which every tree of the step read from row2[info], and of the epoch — so its lane computes it once, from the
    // sigma the list's first entry left in wsig (an empty list leaves none, and touches nothing), and touches with the register: the
    // operand, the operation and the order of per-entry values
    const float tf = (float)p.epoch;
    const ChainParams cpr = chain_params(p, true, tf), cpw = chain_params(p, false, tf);
    if (cpr.d == 1.0f && cpw.d == 1.0f) {
        // unit discounts (Summed / Floored regret with Constant / Linear / Quadratic weight): five lanes per infoset — regret 0, 1,
        // weight 0, 1, payoff — 12 infosets per wavefront in `order`, all lanes in ONE loop without the multiplications.  The payoff
        // lane runs the same touch with the floor -inf and takes no pruned-edge skip: its b is v[0] + v[1] + ... in list order.  A
        // payoff is produced as 0.0f + ev and is never -0, so v[0] == 0.0f + v[0] and b equals the left fold from 0.0f bit for bit;
        // the final 0.0f + b gives the empty list its 0.0f (b of the identity).  Its m is ignored.
        const uint32_t ln = lt & 63u, sub = ln / 5u, c = ln - 5u * sub;
        const float fl = c < 2u ? cpr.fl : (c < 4u ? cpw.fl : rp_u2f(0xff800000u));
        const bool isw = c == 2u || c == 3u;
        const uint32_t cell = c == 4u ? 2u : c & 1u;  // a weight lane's reads land on its regret neighbour's word and are not used
        for (uint32_t i = (lt >> 6) * 12u + sub; ln < 60u && i < nr; i += 4u * 12u) {
            const uint32_t info = order[i] & 255u, rank = order[i] >> 8;
            const uint32_t n = lcount[info], base = lbase[info];
            const float* v = vals + (size_t)cell * L + base;
            const float wd = weight_delta(p.W, wsig[2u * info + (c & 1u)], tf);
            // the entry's value or the lane's own delta, by bit masks: a select on the lane's kind is loop-invariant, the compiler
            // splits the loop on it, and a wavefront with both kinds of lanes runs the two loops one after the other (measured: 6 % of
            // the step, profiles/leduc_five_workgroups_before_after.json)
            const uint32_t keep = isw ? 0u : ~0u, own = isw ? rp_f2u(wd) : 0u;
            Map mp = map_identity();
            for (uint32_t e = 0; e < n; ++e)
                map_touch_unit_unless(mp, PRUNED && c < 2u && !((lmask[base + e] >> c) & 1u), rp_u2f((rp_f2u(v[e]) & keep) | own), fl);
            if (c == 4u) mp.b = 0.0f + mp.b;  // the payoff slot {., sum, ., count}: no entry is skipped, so mp.n == n
            bmaps[bmap_index(chunk, rank, c, g.rank_max, 4u)] = mp;
        }
    } else {
        // any other discount: task = (cell c, infoset); cells 0,1 regret, 2,3 weight, 4 the payoff sum.  The payoff sums are handed out
        // after all the map chains, so that no wavefront mixes the two loops (measured round 4: 0.582 -> 0.562 ms per launch against
        // task % 5)
        for (uint32_t task = lt; task < 5u * nr; task += 256u) {
            const uint32_t c = task < 4u * nr ? task & 3u : 4u;
            const uint32_t oi = order[task < 4u * nr ? task >> 2 : task - 4u * nr], info = oi & 255u, rank = oi >> 8;
            const uint32_t n = lcount[info], base = lbase[info];
            const size_t out = bmap_index(chunk, rank, c, g.rank_max, 4u);
            if (c == 4u) {  // payoff sum of the block, left fold from 0.0f
                const float* v = vals + (size_t)2u * L + base;
                float sum = 0.0f;
                for (uint32_t e = 0; e < n; ++e) sum += v[e];
                bmaps[out] = map_sum_slot(sum, n);
                continue;
            }
            const bool isreg = c < 2u;
            const ChainParams cp = isreg ? cpr : cpw;
            const float* v = vals + (size_t)(c & 1u) * L + base;  // a weight task's reads land on its regret neighbour's word, unused
            const float wd = weight_delta(p.W, wsig[2u * info + (c & 1u)], tf);
            const uint32_t keep = isreg ? ~0u : 0u, own = isreg ? 0u : rp_f2u(wd);  // as in the unit-discount loop
            Map mp = map_identity();
            for (uint32_t e = 0; e < n; ++e)
                map_touch_unless(mp, PRUNED && isreg && !((lmask[base + e] >> c) & 1u), cp.d, rp_u2f((rp_f2u(v[e]) & keep) | own), cp.fl);
            bmaps[out] = mp;
        }
    }
    count_metrics(p, nn, ndec, 0u);
}

}  // namespace rp
