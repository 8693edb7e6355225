// mccfr.hip — external-sampling MCCFR on MI355X (gfx950): the host side — the solver handle, the launchers, the rp_mccfr_* C ABI,
// exploitability.  The kernels are in headers, in dependency order: mccfr_kernels.hpp (layouts, the per-cell map algebra and the
// steps the kernels share), mccfr_traverse.hpp, mccfr_update.hpp, traverse_static.hpp, mccfr_nash.hpp (the best response on the device).
//
// Reference path (crates/mccfr): Solver::step (solver/solver.rs:96-105) = batch() (:225-250) then the
// sequential update_{regret,weight,payoff,visits} (:143-192).  MI355X mapping:
//
//   k_traverse   one LANE per sampled tree (trees of the table-driven games have <= a few dozen nodes):
//                TreeBuilder's explicit DFS stack (builder.rs:141-161) and the node list live in a
//                lane-interleaved HBM scratch (64 lanes = 64 consecutive dwords), the regret/strategy
//                tables are read through L1/L2.  Each walker infoset is evaluated exactly as CfrFlow::dfs /
//                recursed_value / ancestor_reach do (flow.rs:64-87,166-216) — same f32 operation order —
//                by a top-down reach sweep and a bottom-up value sweep over the contiguous subtree.
//   k_count / k_scan / k_compact   stable counting sort of the batch's Decisions into one tree-id-ordered
//                segment per infoset (slot map -> chunk counts -> offsets -> scatter), all CUs busy.
//   k_chain      one workgroup per infoset streams its segment through LDS tiles; one lane per table cell
//                applies the touches sequentially: the reference's order-dependent semantics
//                (R <- max(R*d + delta, floor) per touch, Welford payoff mean), bit for bit.
//   k_summarize / k_fold   the multi-GPU exchange: per-cell composed maps.
//
// Everything f32 is spelled with the primitives of include/rp_math.h and compiled -ffp-contract=off.
#include "mccfr_kernels.hpp"
#include "mccfr_traverse.hpp"
#include "mccfr_update.hpp"
#include "traverse_static.hpp"
#include "mccfr_nash.hpp"
#include "mccfr_subgame.hpp"
#include "host_util.hpp"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <functional>
#include <string>
#include <type_traits>
#include <vector>

// =================================================================================================
// host side
// =================================================================================================
using namespace rp;

namespace {
const char* const CLOCK_NAMES[] = {"traverse", "compact", "update", "subgame"};
enum { CK_TRAVERSE, CK_COMPACT, CK_UPDATE, CK_SUBGAME, CK_COUNT };
}  // namespace

struct rp_mccfr {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // host copy of the game (exploitability, validation)
    std::vector<rp_state> states;
    std::vector<uint32_t> children;
    std::vector<float> payoffs;
    std::vector<uint8_t> info_actions, info_player;
    std::vector<float> default_regret;
    rp_game_table tbl{};
    // device
    DevGame g{};
    DevTables t{};
    DevScratch sc{};
    DevDecisions dc{};
    void* d_states = nullptr;
    void* d_children = nullptr;
    void* d_kids = nullptr;
    void* d_rows = nullptr;  // DevGame::rows
    size_t rows_bytes = 0;
    void* d_payoffs = nullptr;
    void* d_info_actions = nullptr;
    void* d_info_player = nullptr;
    void* d_info_rank = nullptr;  // DevGame::info_rank, then DevGame::rank_info
    void* d_scratch = nullptr;
    void* d_dec = nullptr;
    void* d_summary = nullptr;
    void* d_window = nullptr;      // rp_mccfr_step_comm: this rank's window summary, then every rank's (all-gathered)
    uint32_t window_world = 0;
    void* d_sorted = nullptr;
    void* d_bmaps = nullptr;
    uint32_t maxint = 1;  // most internal nodes of a sampled tree
    void* d_itab = nullptr;
    DevInfoTab itab{};
    DevSorted so{};
    unsigned long long* d_counters = nullptr;
    int R = 0, W = 0, S = 0;
    rp_hyper hp{};
    uint64_t seed = 0;
    // rp_mccfr_set_rng: RP_RNG_REFERENCE draws from the reference's own chain (include/rp_refrng.h)
    rp_rng_kind rng = RP_RNG_COUNTER;
    uint32_t n_chance_infos = 0;
    void* d_info_streams = nullptr;    // rp_hash_stream[n_infos]
    void* d_chance_streams = nullptr;  // rp_hash_stream[n_chance_infos]
    void* d_ref_mid = nullptr;         // rp_sip_mid[n_infos + n_chance_infos], of epoch ref_mid_epoch
    uint64_t ref_mid_epoch = ~0ull;
    uint32_t batch = 1, capacity = 0;
    uint64_t epoch = 0;
    uint32_t rank = 0, world = 1;
    uint32_t maxdec = 1;
    rp_update_mode mode = RP_UPDATE_ORDERED;
    bool use_lds_traverse = false;
    // the per-infoset tables of the traversal (DevInfoTab) are a function of the regret/strategy tables: refreshed when stale
    uint64_t tables_version = 1, itab_version = 0;
    static constexpr uint32_t cell_pad = 7;  // words between the cells' value arrays in k_traverse_maps_static's LDS (bank spread)
    bool fuse_maps = true;  // composed update: traversal + block maps in one kernel when the game allows (RP_TRAV_UNFUSED=1: never)
    uint32_t fold_split_groups = 0;  // composed update: batches of at least this many groups fold them in k_fold_groups (RP_FOLD_SPLIT=1 | 0: all | none)
    int static_skel = 0;  // 0: none (k_traverse_lds / k_traverse), 1: KuhnSkel, 2: LeducSkel (traverse_static.hpp)
    KernelClocks clk{CLOCK_NAMES, CK_COUNT};  // rp_mccfr_profile
    // CfrNash on the device (mccfr_nash.hpp): built by the first call that asks (nash_prepare), kept until destroy
    void* d_nash = nullptr;  // NashTree's arrays, then NashWork's
    NashTree nt{};
    NashWork nw{};
    int nash_variant = -1;  // -1: not built; 0 one, 1 levels
    bool nash_in_lds = false;
    std::vector<uint32_t> nash_level_size;  // nodes per depth level: the grids of k_nash_level
    float* nash_pinned = nullptr;  // rp_mccfr_solve_to: the check's value, mapped host memory
    // the safe subgame re-solve (mccfr_subgame.hpp): the per-solve regions of one launch, grow-only
    void* d_msub = nullptr;
    size_t msub_bytes = 0;
    // rp_mccfr_set_frontiers: the frontier tables of the depth-limited re-solve, one allocation; fr.depth == nullptr: none
    void* d_front = nullptr;
    MsFrontiers fr{};
};

namespace {

int set_device(const rp_mccfr* h) {
    HIP_TRY(hipSetDevice(h->device));
    return RP_OK;
}

size_t chain_lds_bytes() { return (size_t)CHAIN_LDS_WORDS * 4; }

size_t summary_bytes_of(const rp_mccfr* h) {
    return (size_t)h->tbl.n_infos * h->tbl.max_actions * sizeof(Cell) + (size_t)h->tbl.n_infos * sizeof(InfoSum);
}

// largest number of walker nodes / stack entries an externally sampled tree can have
void sampled_tree_bounds(const rp_mccfr* h, uint32_t* maxdec, uint32_t* maxstack, uint32_t* maxint) {
    const rp::TableBounds b = rp::table_bounds(h->tbl, h->tbl.train_root);  // the sweep rp_game_table_check runs (games.cpp)
    *maxdec = std::max(b.decisions, 1u);
    *maxstack = std::max(b.stack, 1u) + 1;
    *maxint = std::max(b.internal, 1u);
}

size_t chunk_maps_lds_bytes(const rp_mccfr* h);
int alloc_batch_buffers(rp_mccfr* h, uint32_t batch) {
    if (batch <= h->capacity) return RP_OK;
    if (h->d_scratch) HIP_TRY(hipFree(h->d_scratch));
    if (h->d_dec) HIP_TRY(hipFree(h->d_dec));
    h->d_scratch = h->d_dec = nullptr;
    const size_t stride = ((size_t)batch + 255) & ~(size_t)255;
    const uint32_t A = h->tbl.max_actions;
    DevScratch& sc = h->sc;
    sc.stride = stride;
    const size_t node_words = (size_t)sc.maxn * stride, stack_words = (size_t)sc.maxs * stride;
    const size_t total_words = 8 * node_words + 4 * stack_words + (size_t)A * stride;
    HIP_TRY(hipMalloc(&h->d_scratch, total_words * 4));
    uint32_t* base = reinterpret_cast<uint32_t*>(h->d_scratch);
    sc.n_meta = base; base += node_words;
    sc.n_info = base; base += node_words;
    sc.n_frel = reinterpret_cast<float*>(base); base += node_words;
    sc.n_fsmp = reinterpret_cast<float*>(base); base += node_words;
    sc.n_pay = reinterpret_cast<float*>(base); base += node_words;
    sc.n_rel = reinterpret_cast<float*>(base); base += node_words;
    sc.n_smp = reinterpret_cast<float*>(base); base += node_words;
    sc.n_acc = reinterpret_cast<float*>(base); base += node_words;
    sc.s_state = base; base += stack_words;
    sc.s_meta = base; base += stack_words;
    sc.s_frel = reinterpret_cast<float*>(base); base += stack_words;
    sc.s_fsmp = reinterpret_cast<float*>(base); base += stack_words;
    sc.t_v = reinterpret_cast<float*>(base);

    DevDecisions& dc = h->dc;
    dc.stride = stride;
    dc.maxdec = h->maxdec;
    const size_t slot_words = (size_t)dc.maxdec * stride;
    // chunk-local sort: no per-infoset slot map (RP_MCCFR_SLOTMAP=1 forces the large-game path, for tests)
    const bool small = chunk_maps_lds_bytes(h) <= 64 * 1024 && h->tbl.n_infos <= CM_PASSES * CH_THREADS && !getenv("RP_MCCFR_SLOTMAP");
    const size_t dec_bytes = (3 * slot_words + 2 * slot_words * A) * 4 + (small ? 0 : (size_t)h->tbl.n_infos * stride) + stride;
    HIP_TRY(hipMalloc(&h->d_dec, dec_bytes));
    uint32_t* d = reinterpret_cast<uint32_t*>(h->d_dec);
    dc.info = d; d += slot_words;
    dc.mask = d; d += slot_words;
    dc.payoff = reinterpret_cast<float*>(d); d += slot_words;
    dc.regret = reinterpret_cast<float*>(d); d += slot_words * A;
    dc.policy = reinterpret_cast<float*>(d); d += slot_words * A;
    dc.ndec = reinterpret_cast<uint8_t*>(d);
    dc.slotmap = small ? nullptr : dc.ndec + stride;
    // tree-ordered segments: at most maxdec Decisions per tree
    if (h->d_sorted) HIP_TRY(hipFree(h->d_sorted));
    h->d_sorted = nullptr;
    DevSorted& so = h->so;
    so.n_chunks = (uint32_t)((stride + CH_TREES - 1) / CH_TREES);
    const size_t cap = slot_words;
    const size_t nic = (size_t)h->tbl.n_infos * so.n_chunks;
    const size_t sorted_words = cap * 2 * A + 2 * cap + 2 * nic + h->tbl.n_infos;
    HIP_TRY(hipMalloc(&h->d_sorted, sorted_words * 4));
    uint32_t* sw = reinterpret_cast<uint32_t*>(h->d_sorted);
    so.rw = reinterpret_cast<float*>(sw); sw += cap * 2 * A;
    so.mask = sw; sw += cap;
    so.payoff = reinterpret_cast<float*>(sw); sw += cap;
    so.counts = sw; sw += nic;
    so.offs = sw; sw += nic;
    so.total = sw;
    // per-block rows of the composed update's maps (bmap_index): one walker's infosets at a time, so sized by the larger player
    if (h->d_bmaps) HIP_TRY(hipFree(h->d_bmaps));
    h->d_bmaps = nullptr;
    const size_t nblk_max = (stride + RP_COMPOSE_CHUNK - 1) / RP_COMPOSE_CHUNK;
    // ... followed by the group maps and the arrival counters of k_combine2
    const size_t ngrp_max = (nblk_max + RP_FOLD_GROUP - 1) / RP_FOLD_GROUP;
    const size_t bytes = bmap_index((uint32_t)(nblk_max + ngrp_max), 0, 0, h->g.rank_max, 2 * A) * sizeof(Map) + (size_t)h->tbl.n_infos * sizeof(uint32_t);
    HIP_TRY(hipMalloc(&h->d_bmaps, bytes));
    HIP_TRY(hipMemset(h->d_bmaps, 0, bytes));
    HIP_TRY(hipDeviceSynchronize());  // the memset runs on the null stream; the solver's stream is non-blocking (rp_mccfr_set_batch)
    h->capacity = batch;
    return RP_OK;
}

StepParams make_params(const rp_mccfr* h) {
    StepParams p{};
    p.seed = h->seed;
    p.epoch = h->epoch;
    p.tree_base = (uint64_t)h->rank * h->batch;
    p.batch = h->batch;
    p.walker = (uint32_t)(h->epoch % h->tbl.n_players);  // CfrSampling::walker (book.rs:142-144)
    p.R = h->R; p.W = h->W; p.S = h->S;
    p.temperature = h->hp.temperature; p.smoothing = h->hp.smoothing; p.curiosity = h->hp.curiosity;
    p.prune_threshold = h->hp.prune_threshold; p.prune_explore = h->hp.prune_explore;
    p.prune_warmup = h->hp.prune_warmup;
    p.regret_min = h->hp.regret_min;
    if (h->R == RP_REGRET_DISCOUNTED) {  // (t / PERIOD).powf(ALPHA | BETA), PERIOD = 1 (discounted.rs:23,33,37)
        p.pow15 = rp_pow15((float)h->epoch);
        p.pow05 = rp_pow05((float)h->epoch);
    }
    p.counters = h->d_counters;
    if (h->rng == RP_RNG_REFERENCE) {
        p.ref_info = reinterpret_cast<const rp_sip_mid*>(h->d_ref_mid);
        p.ref_chance = p.ref_info + h->tbl.n_infos;
    }
    return p;
}

// run-time flags -> template arguments: f(std::bool_constant<a>{}, std::bool_constant<b>{})
template <class F>
void with_bool(bool a, F&& f) {
    if (a) f(std::true_type{});
    else f(std::false_type{});
}
template <class F>
void with_bools(bool a, bool b, F&& f) {
    with_bool(a, [&](auto ta) { with_bool(b, [&](auto tb) { f(ta, tb); }); });
}

// rp_mccfr::static_skel -> the skeleton type: f(KuhnSkel{}) or f(LeducSkel{}); and the instantiations of the skeleton kernels:
// f(G{}, std::integral_constant<int, walker>{}, std::bool_constant<pruned>{}, std::bool_constant<ref>{})
template <class F>
void with_skeleton(int static_skel, F&& f) {
    if (static_skel == 1) f(KuhnSkel{});
    else if (static_skel == 2) f(LeducSkel{});  // 0: the game matches no skeleton, nothing to instantiate
}
template <class F>
void with_static_traversal(int static_skel, uint32_t walker, bool pruned, bool ref, F&& f) {
    with_skeleton(static_skel, [&](auto gt) {
        with_bool(walker == 0, [&](auto w0) {
            with_bools(pruned, ref, [&](auto pr, auto rf) { f(gt, std::integral_constant<int, decltype(w0)::value ? 0 : 1>{}, pr, rf); });
        });
    });
}

// Does the game's state table match skeleton G node for node, for EVERY chance outcome?  (traverse_static.hpp)  Also: an
// infoset belongs to one skeleton node only, so a sampled tree meets each walker infoset at most once (a span of the
// reference's Tree::partition has a single root) — the static kernel writes one Decisions per live walker node.
template <class G>
bool skel_matches(const rp_game_table* game, const std::vector<uint32_t>& children) {
    constexpr Skeleton S = SkelOf<G>::S;
    if (game->n_players != 2 || game->max_actions != 2) return false;
    std::vector<std::vector<int>> kids(S.n);
    for (int s = 1; s < S.n; ++s) kids[S.parent[s]].push_back(s);
    std::vector<int> node_of_info(game->n_infos, -1);
    std::function<bool(uint32_t, int)> match = [&](uint32_t sid, int s) -> bool {
        const rp_state& st = game->states[sid];
        if (S.kind[s] == SK_TERMINAL) return st.n_children == 0;
        if (S.kind[s] == SK_CHANCE) {
            if (st.turn != RP_TURN_CHANCE || st.n_children == 0 || kids[s].size() != 1) return false;
            for (uint32_t k = 0; k < st.n_children; ++k)
                if (!match(children[st.offset + k], kids[s][0])) return false;
            return true;
        }
        if (st.turn != (uint8_t)(S.kind[s] - SK_P0) || st.n_children != 2 || kids[s].size() != 2 || st.info >= game->n_infos) return false;
        if (node_of_info[st.info] >= 0 && node_of_info[st.info] != s) return false;
        node_of_info[st.info] = s;
        for (int c : kids[s])
            if (S.edge[c] > 1 || !match(children[st.offset + (uint32_t)S.edge[c]], c)) return false;
        return kids[s][0] != kids[s][1] && S.edge[kids[s][0]] != S.edge[kids[s][1]];
    };
    return match(game->train_root, 0);
}

// DevGame::rows for a game that matches skeleton G: the words of every group of nodes (RowLayout, traverse_static.hpp), one row per
// sequence of chance outcomes on the path.  Returns false (no table) when two instances of a skeleton chance node differ in their
// number of outcomes, or when the table would be unreasonably large.
template <class G>
bool build_rows(const rp_game_table* game, const std::vector<uint32_t>& children, const std::function<uint4(uint32_t)>& rec_of,
                std::vector<uint32_t>& rows, uint32_t* base, uint32_t* fan) {
    constexpr Skeleton S = SkelOf<G>::S;
    constexpr RowLayout R = SkelOf<G>::R;
    std::vector<std::vector<int>> kids(S.n);
    for (int s = 1; s < S.n; ++s) kids[S.parent[s]].push_back(s);
    for (int s = 0; s < S.n; ++s) fan[s] = base[s] = 0;
    bool uniform = true;
    std::function<void(uint32_t, int)> fans = [&](uint32_t sid, int s) {
        const rp_state& st = game->states[sid];
        if (S.kind[s] == SK_CHANCE) {
            if (fan[s] == 0) fan[s] = st.n_children;
            else if (fan[s] != st.n_children) uniform = false;
            for (uint32_t k = 0; k < st.n_children; ++k) fans(children[st.offset + k], kids[s][0]);
        } else if (S.kind[s] != SK_TERMINAL) {
            for (int c : kids[s]) fans(children[st.offset + (uint32_t)S.edge[c]], c);
        }
    };
    fans(game->train_root, 0);
    if (!uniform) return false;
    // rows of chance node c = product of the fans of c and of its chance ancestors; every group starts on a 128-byte line
    uint64_t total = 0;  // words
    for (int c = 0; c < S.n; ++c) {
        if (S.kind[c] != SK_CHANCE) continue;
        uint64_t count = 1;
        for (int a = 0; a <= c; ++a)
            if (S.kind[a] == SK_CHANCE && c <= S.end[a]) count *= fan[a];
        base[c] = (uint32_t)(total / 4);
        total += (count * (uint64_t)R.stride[c] + 31) & ~(uint64_t)31;
        if (total > (1ull << 28)) return false;  // 1 GB; also keeps a row's byte offset in 32 bits
    }
    rows.assign(total, 0u);
    std::function<void(uint32_t, int, uint64_t)> fill = [&](uint32_t sid, int s, uint64_t idx) {  // idx: the outcomes above s
        const rp_state& st = game->states[sid];
        if (const int c = R.group[s]; c >= 0) {
            uint32_t* row = &rows[(size_t)base[c] * 4 + idx * (uint64_t)R.stride[c]];
            const uint4 r = rec_of(sid);
            if (S.kind[s] == SK_CHANCE) {
                row[R.word[s]] = r.w;
                row[R.word2[s]] = r.y;
            } else if (S.kind[s] == SK_TERMINAL) {
                row[R.word[s]] = r.y;
                row[R.word2[s]] = r.z;
            } else {
                row[R.word[s]] = r.y;
            }
        }
        if (S.kind[s] == SK_CHANCE) {
            for (uint32_t k = 0; k < st.n_children; ++k) fill(children[st.offset + k], kids[s][0], idx * fan[s] + k);
        } else if (S.kind[s] != SK_TERMINAL) {
            for (int c : kids[s]) fill(children[st.offset + (uint32_t)S.edge[c]], c, idx);
        }
    };
    fill(game->train_root, 0, 0);
    return true;
}

size_t traverse_lds_bytes(const rp_mccfr* h) {
    const size_t shared = std::max<size_t>(2 * (size_t)h->maxint, 4 * (size_t)h->sc.maxs);  // stack, then reach prefixes
    return ((size_t)2 * h->sc.maxn + shared + (h->tbl.max_actions <= 4 ? 0 : h->tbl.max_actions)) * 64 * 4;
}
bool traverse_fits_lds(const rp_mccfr* h) {
    return h->sc.maxn <= 62 && h->maxint <= 32 && h->tbl.max_depth <= 10 && h->tbl.n_infos <= 8191 && h->tbl.max_actions <= 16 &&
           traverse_lds_bytes(h) <= 64 * 1024;
}

// k_prepare_infos, unless the tables have not changed since the per-infoset tables were last derived from them (an exchange
// window traverses against a frozen table; k_combine2<APPLY> refreshes the rows it changes itself)
void launch_prepare_ref(rp_mccfr* h, const StepParams& p) {
    if (h->rng == RP_RNG_REFERENCE && h->ref_mid_epoch != p.epoch) {
        const uint32_t n = h->tbl.n_infos + h->n_chance_infos;
        rp_sip_mid* mid = reinterpret_cast<rp_sip_mid*>(h->d_ref_mid);
        hipLaunchKernelGGL(k_prepare_ref, dim3((n + 63) / 64), dim3(64), 0, h->stream, reinterpret_cast<const rp_hash_stream*>(h->d_info_streams),
                           h->tbl.n_infos, reinterpret_cast<const rp_hash_stream*>(h->d_chance_streams), h->n_chance_infos, p.epoch, mid,
                           mid + h->tbl.n_infos);
        h->ref_mid_epoch = p.epoch;
    }
}
void launch_prepare(rp_mccfr* h, const StepParams& p) {
    launch_prepare_ref(h, p);
    if (h->itab_version == h->tables_version) return;
    hipLaunchKernelGGL(k_prepare_infos, dim3((h->tbl.n_infos + 63) / 64), dim3(64), 0, h->stream, h->g, h->t, p, h->itab);
    h->itab_version = h->tables_version;
}

int launch_traverse(rp_mccfr* h, const StepParams& p) {
    if (h->dc.slotmap) HIP_TRY(hipMemsetAsync(h->dc.slotmap, 0, (size_t)h->tbl.n_infos * h->dc.stride, h->stream));
    h->clk.begin(h->stream, CK_TRAVERSE);
    if (h->static_skel) {
        launch_prepare(h, p);
        const dim3 grid((h->batch + 255) / 256), block(256);
        with_static_traversal(h->static_skel, p.walker, p.S != RP_SAMPLING_EXTERNAL, p.ref_info != nullptr, [&](auto gt, auto wk, auto pr, auto rf) {
            hipLaunchKernelGGL((k_traverse_static<decltype(gt), decltype(wk)::value, decltype(pr)::value, decltype(rf)::value>), grid, block, 0,
                               h->stream, h->g, h->itab, h->dc, p);
        });
    } else if (h->use_lds_traverse) {
        launch_prepare(h, p);
        const size_t lds = traverse_lds_bytes(h);
        const dim3 grid((h->batch + 63) / 64), block(64);
        with_bool(h->tbl.max_actions <= 4, [&](auto tv) {
            hipLaunchKernelGGL((k_traverse_lds<decltype(tv)::value>), grid, block, lds, h->stream, h->g, h->itab, h->dc, p, h->sc.maxn, h->sc.maxs,
                               h->maxint);
        });
    } else {
        launch_prepare_ref(h, p);
        const uint32_t threads = 256, blocks = (h->batch + threads - 1) / threads;
        hipLaunchKernelGGL(k_traverse, dim3(blocks), dim3(threads), 0, h->stream, h->g, h->t, h->sc, h->dc, p);
    }
    h->clk.end(h->stream, CK_TRAVERSE);
    HIP_TRY(hipGetLastError());
    return RP_OK;
}

// stable counting sort of the batch's Decisions into per-infoset, tree-ordered segments
int launch_sort(rp_mccfr* h, const StepParams& p) {
    const uint32_t nchunks = (h->batch + CH_TREES - 1) / CH_TREES;
    h->so.n_chunks = nchunks;
    h->clk.begin(h->stream, CK_COMPACT);
    if (!h->dc.slotmap) {
        const size_t NI = h->tbl.n_infos;
        hipLaunchKernelGGL(k_count_small, dim3(nchunks), dim3(CH_THREADS), NI * SM_WORDS * 4, h->stream, h->g, h->dc, h->so, p);
        hipLaunchKernelGGL(k_scan, dim3(h->tbl.n_infos), dim3(CH_THREADS), 0, h->stream, h->g, h->so, p);
        hipLaunchKernelGGL(k_compact_small, dim3(nchunks), dim3(CH_THREADS), NI * SM_WORDS * 4 + 2 * NI * 4 + NI * SM_WORDS * 2,
                           h->stream, h->g, h->dc, h->so, p);
    } else {
        hipLaunchKernelGGL(k_count, dim3(nchunks, h->tbl.n_infos), dim3(SLOT_THREADS), 0, h->stream, h->g, h->dc, h->so, p);
        hipLaunchKernelGGL(k_scan, dim3(h->tbl.n_infos), dim3(CH_THREADS), 0, h->stream, h->g, h->so, p);
        hipLaunchKernelGGL(k_compact, dim3(nchunks, h->tbl.n_infos), dim3(SLOT_THREADS), 0, h->stream, h->g, h->dc, h->so, p);
    }
    h->clk.end(h->stream, CK_COMPACT);
    HIP_TRY(hipGetLastError());
    return RP_OK;
}

int launch_chain(rp_mccfr* h, const StepParams& p) {
    const size_t lds = chain_lds_bytes();
    const bool sgn = h->R == RP_REGRET_DISCOUNTED || h->R == RP_REGRET_ASYMMETRIC;
    const bool prn = h->S != RP_SAMPLING_EXTERNAL;
    const dim3 grid(h->tbl.n_infos), block(128);
    h->clk.begin(h->stream, CK_UPDATE);
    with_bools(sgn, prn, [&](auto sg, auto pr) {
        hipLaunchKernelGGL((k_chain<decltype(sg)::value, decltype(pr)::value>), grid, block, lds, h->stream, h->g, h->t, h->so, p);
    });
    h->clk.end(h->stream, CK_UPDATE);
    HIP_TRY(hipGetLastError());
    return RP_OK;
}

// block bookkeeping of the composed update: one block per (infoset, chunk of RP_COMPOSE_CHUNK trees)
uint32_t chunks_of(size_t trees) { return (uint32_t)((trees + RP_COMPOSE_CHUNK - 1) / RP_COMPOSE_CHUNK); }
size_t chunk_maps_lds_bytes(const rp_mccfr* h) {
    const size_t NI = h->tbl.n_infos;
    return NI * SM_WORDS * 4 + 2 * NI * 4 + (size_t)CH_TREES * h->maxdec * 4 + NI * SM_WORDS * 2 +
           2 * (size_t)CH_TREES * h->maxdec * 2;
}

// Decisions of the batch -> one composed map per table cell (+ payoff sum and count per infoset) in `blob_dev`.
// Small games compose straight from the traversal's output; large ones from the sorted segments (launch_sort first).
// the traversal and the block maps in one kernel (k_traverse_maps_static): composed update of a small game whose traversal is
// instantiated over its skeleton, external sampling
size_t traverse_maps_lds_bytes(const rp_mccfr* h) {
    const size_t NI = h->tbl.n_infos;
    const size_t masks = h->S != RP_SAMPLING_EXTERNAL ? (size_t)h->maxdec * 256 * 4 : 0;  // the expanded edges of every list entry
    return (NI * 8 + 2 * NI) * 4 + NI * 8 * 2 + (NI + (NI & 1)) * 2 + 2 * NI * 4 + (size_t)3 * (h->maxdec * 256 + h->cell_pad) * 4 + masks;
}
static_assert(CH_THREADS <= 256u, "k_traverse_maps_static packs (infoset, rank of the infoset) into the 16 bits of an `order` entry");
// rank_max <= 64: one wavefront builds the chunk's lists, a lane per infoset of the walker (Kuhn 6, Leduc 60; a skeleton game with more
// takes k_chunk_maps)
bool traverse_maps_fused(const rp_mccfr* h) {
    return h->static_skel && !h->dc.slotmap && h->tbl.n_infos <= CH_THREADS && h->g.rank_max <= 64u &&
           traverse_maps_lds_bytes(h) <= 64 * 1024 && h->fuse_maps;
}

// composed update: whether a batch's group maps are folded by a launch of their own (k_combine2<false, false> + k_fold_groups) or by the
// last workgroup of each tile of k_combine2.  FOLD_SPLIT_GROUPS: DESIGN.md §3, "The group fold as a launch of its own" and "Unit slabs"
constexpr uint32_t FOLD_SPLIT_GROUPS = 64;
bool fold_split(const rp_mccfr* h, uint32_t batch) {
    const uint32_t ngrp = (chunks_of(batch) + RP_FOLD_GROUP - 1) / RP_FOLD_GROUP;
    return ngrp >= h->fold_split_groups;
}

// apply = true: the summary is applied to the tables by the fold itself (single-GPU step), `blob_dev` is not written
int launch_summarize(rp_mccfr* h, const StepParams& p, void* blob_dev, bool fused = false, bool apply = false) {
    unsigned char* blob = reinterpret_cast<unsigned char*>(blob_dev);
    Cell* cells = reinterpret_cast<Cell*>(blob);
    InfoSum* sums = reinterpret_cast<InfoSum*>(blob + (size_t)h->tbl.n_infos * h->tbl.max_actions * sizeof(Cell));
    const uint32_t A = h->tbl.max_actions;
    const uint32_t nblk_max = chunks_of(h->dc.stride), nblk = chunks_of(h->batch);
    Map* bmaps = reinterpret_cast<Map*>(h->d_bmaps);
    const bool pruned = h->S != RP_SAMPLING_EXTERNAL;
    if (fused) {
        h->clk.begin(h->stream, CK_TRAVERSE);
        launch_prepare(h, p);
        const size_t lds = traverse_maps_lds_bytes(h);
        with_static_traversal(h->static_skel, p.walker, pruned, p.ref_info != nullptr, [&](auto gt, auto wk, auto pr, auto rf) {
            hipLaunchKernelGGL((k_traverse_maps_static<decltype(gt), decltype(wk)::value, decltype(pr)::value, decltype(rf)::value>), dim3(nblk),
                               dim3(256), lds, h->stream, h->g, h->itab, p, bmaps, h->maxdec, h->cell_pad);
        });
        h->clk.end(h->stream, CK_TRAVERSE);
    }
    h->clk.begin(h->stream, CK_UPDATE);
    if (fused) {
    } else if (!h->dc.slotmap) {
        const size_t lds = chunk_maps_lds_bytes(h);
        with_bools(pruned, h->tbl.n_infos <= CH_THREADS, [&](auto pr, auto one) {
            hipLaunchKernelGGL((k_chunk_maps<decltype(pr)::value, decltype(one)::value ? 1u : CM_PASSES>), dim3(nblk), dim3(CH_THREADS), lds,
                               h->stream, h->g, h->dc, p, bmaps);
        });
    } else {
        with_bool(pruned, [&](auto pr) {
            hipLaunchKernelGGL((k_block_maps<decltype(pr)::value>), dim3(nblk, h->tbl.n_infos), dim3(128), 0, h->stream, h->g, h->so, p, bmaps);
        });
    }
    {
        const uint32_t W2 = 2 * A, nr = h->g.rank_count[p.walker];
        const uint32_t ngrp_max = (nblk_max + RP_FOLD_GROUP - 1) / RP_FOLD_GROUP, ngrp = (nblk + RP_FOLD_GROUP - 1) / RP_FOLD_GROUP;
        FoldScratch fs;
        fs.gmaps = bmaps + bmap_index(nblk_max, 0, 0, h->g.rank_max, W2);
        fs.done = reinterpret_cast<uint32_t*>(bmaps + bmap_index(nblk_max + ngrp_max, 0, 0, h->g.rank_max, W2));
        const dim3 grid(std::max(ngrp, 1u), cb2_tiles(nr, W2)), fold_grid(std::max(nr, 1u));
        // few groups: the last workgroup of a tile folds them in the same launch; many: a launch of its own, a workgroup per infoset
        const bool split = fold_split(h, h->batch);
        if (split) hipLaunchKernelGGL((k_combine2<false, false>), grid, dim3(CB2_THREADS), 0, h->stream, h->g, h->t, h->itab, p, bmaps, nr, fs, cells, sums);
        if (apply) {
            if (split) hipLaunchKernelGGL((k_fold_groups<true>), fold_grid, dim3(CB2_THREADS), 0, h->stream, h->g, h->t, h->itab, p, fs.gmaps, nr, cells, sums);
            else hipLaunchKernelGGL((k_combine2<true>), grid, dim3(CB2_THREADS), 0, h->stream, h->g, h->t, h->itab, p, bmaps, nr, fs, cells, sums);
            h->tables_version += 1;  // the kernel refreshes the rows of the per-infoset tables it changes
            if (h->itab_version + 1 == h->tables_version) h->itab_version = h->tables_version;
        } else {
            if (split) hipLaunchKernelGGL((k_fold_groups<false>), fold_grid, dim3(CB2_THREADS), 0, h->stream, h->g, h->t, h->itab, p, fs.gmaps, nr, cells, sums);
            else hipLaunchKernelGGL((k_combine2<false>), grid, dim3(CB2_THREADS), 0, h->stream, h->g, h->t, h->itab, p, bmaps, nr, fs, cells, sums);
        }
    }
    h->clk.end(h->stream, CK_UPDATE);
    HIP_TRY(hipGetLastError());
    return RP_OK;
}

// Solver::batch + the composed maps of its Decisions -> one summary blob
int launch_batch_summary(rp_mccfr* h, const StepParams& p, void* blob_dev, bool apply = false) {
    if (traverse_maps_fused(h)) return launch_summarize(h, p, blob_dev, true, apply);
    int rc = launch_traverse(h, p);
    if (rc) return rc;
    if (h->dc.slotmap && (rc = launch_sort(h, p))) return rc;
    return launch_summarize(h, p, blob_dev, false, apply);
}

int enqueue_step(rp_mccfr* h) {
    const StepParams p = make_params(h);
    int rc;
    // the ordered chains and the large-game composed path read the sorted segments; small games compose from the
    // traversal's output directly
    if (h->mode == RP_UPDATE_ORDERED) {
        if ((rc = launch_traverse(h, p))) return rc;
        if ((rc = launch_sort(h, p))) return rc;
        if ((rc = launch_chain(h, p))) return rc;
        h->tables_version += 1;
    } else {
        // the fold applies the summary to the tables itself (k_combine2<APPLY> or k_fold_groups<APPLY>: fold + k_fold + k_prepare_infos)
        if ((rc = launch_batch_summary(h, p, h->d_summary, true))) return rc;
    }
    h->epoch += 1;  // CfrSampling::increment via Solver::advance (solver.rs:103-104)
    return RP_OK;
}

// nodes, infos, error flags: the sums (resp. the OR) over the stripes
int read_counters(rp_mccfr* h, unsigned long long c[3]) {
    std::vector<unsigned long long> all((size_t)METRIC_STRIPES * METRIC_STRIDE);
    HIP_TRY(hipMemcpyAsync(all.data(), h->d_counters, all.size() * 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    c[0] = c[1] = c[2] = 0;
    for (uint32_t s = 0; s < METRIC_STRIPES; ++s) {
        c[0] += all[(size_t)s * METRIC_STRIDE];
        c[1] += all[(size_t)s * METRIC_STRIDE + 1];
        c[2] |= all[(size_t)s * METRIC_STRIDE + 2];
    }
    return RP_OK;
}

int check_device_errors(rp_mccfr* h) {
    unsigned long long c[3];
    int rc = read_counters(h, c);
    if (rc) return rc;
    if (c[2]) return rp::fail(RP_ERR_CAPACITY, "mccfr kernel capacity exceeded (flags %llu): nodes/stack/decisions", c[2]);
    return RP_OK;
}

int composed_supported(const rp_mccfr* h) {
    if (h->R == RP_REGRET_DISCOUNTED || h->R == RP_REGRET_ASYMMETRIC)
        return rp::fail(RP_ERR_UNSUPPORTED,
                        "composed update needs a sign-independent discount (Summed/Linear/Floored regret)");
    return RP_OK;
}

int fetch_tables(rp_mccfr* h, std::vector<float>& regret, std::vector<float>& weight, std::vector<float>& payoff,
                 std::vector<uint32_t>& visits) {
    const size_t cells = (size_t)h->tbl.n_infos * h->tbl.max_actions;
    regret.resize(cells); weight.resize(cells); payoff.resize(cells); visits.resize(cells);
    HIP_TRY(hipMemcpyAsync(regret.data(), h->t.regret, cells * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(weight.data(), h->t.weight, cells * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(payoff.data(), h->t.payoff, cells * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(visits.data(), h->t.visits, cells * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return RP_OK;
}

}  // namespace

extern "C" {

int rp_mccfr_create(const rp_game_table* game, rp_regret_kind r, rp_weight_kind w, rp_sampling_kind s,
                    uint32_t batch_size, const rp_hyper* hp, uint64_t seed, int device, rp_mccfr** out) {
    if (!game || !out) return rp::fail(RP_ERR_INVALID, "rp_mccfr_create: NULL argument");
    int rc = rp_game_table_check(game);
    if (rc) return rc;
    if ((int)r < 0 || (int)r > 4 || (int)w < 0 || (int)w > 3 || (int)s < 0 || (int)s > 2)
        return rp::fail(RP_ERR_INVALID, "rp_mccfr_create: unknown schedule / sampling kind");
    if (batch_size == 0) return rp::fail(RP_ERR_INVALID, "rp_mccfr_create: batch_size must be > 0");
    if (rp_device_count() <= 0)
        return rp::fail(RP_ERR_NO_DEVICE, "rp_mccfr_create: no HIP device visible; the MI355X path has no CPU fallback");
    if (game->max_tree_nodes == 0 || game->max_tree_nodes >= 255)
        return rp::fail(RP_ERR_CAPACITY, "rp_mccfr_create: sampled trees of up to %u nodes exceed the per-lane limit (254)",
                        game->max_tree_nodes);
    rp_mccfr* h = new rp_mccfr();
    h->device = device;
    h->tbl = *game;
    h->states.assign(game->states, game->states + game->n_states);
    h->children.assign(game->children, game->children + game->n_children);
    h->payoffs.assign(game->payoffs, game->payoffs + (size_t)game->n_terminals * game->n_players);
    h->info_actions.assign(game->info_actions, game->info_actions + game->n_infos);
    h->info_player.assign(game->info_player, game->info_player + game->n_infos);
    const size_t cells = (size_t)game->n_infos * game->max_actions;
    h->default_regret.assign(cells, 0.0f);
    if (game->default_regret) h->default_regret.assign(game->default_regret, game->default_regret + cells);
    h->tbl.states = h->states.data();
    h->tbl.children = h->children.data();
    h->tbl.payoffs = h->payoffs.data();
    h->tbl.info_actions = h->info_actions.data();
    h->tbl.info_player = h->info_player.data();
    h->tbl.default_regret = h->default_regret.data();
    h->R = r; h->W = w; h->S = s;
    if (hp) h->hp = *hp; else rp_hyper_default(&h->hp);
    h->seed = seed;
    h->batch = batch_size;

#define CREATE_TRY(expr)                                                                             \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess) {                                                                      \
            int _rc = rp::fail(RP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));           \
            rp_mccfr_destroy(h);                                                                     \
            return _rc;                                                                              \
        }                                                                                            \
    } while (0)

    CREATE_TRY(hipSetDevice(device));
    CREATE_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
    // game table -> HBM (states repacked to 16 B)
    std::vector<uint4> packed(game->n_states);
    for (uint32_t i = 0; i < game->n_states; ++i) {
        const rp_state& st = game->states[i];
        packed[i] = make_uint4((uint32_t)st.turn | ((uint32_t)st.n_children << 8), st.turn == RP_TURN_CHANCE ? (uint32_t)st.chance_info : st.info, st.offset, 0u);
    }
    CREATE_TRY(hipMalloc(&h->d_states, packed.size() * sizeof(uint4)));
    CREATE_TRY(hipMemcpy(h->d_states, packed.data(), packed.size() * sizeof(uint4), hipMemcpyHostToDevice));
    CREATE_TRY(hipMalloc(&h->d_children, h->children.size() * 4));
    CREATE_TRY(hipMemcpy(h->d_children, h->children.data(), h->children.size() * 4, hipMemcpyHostToDevice));
    // child records: one load on arrival at a node instead of children[] -> states[] -> payoffs[]
    const std::function<uint4(uint32_t)> rec_of = [&](uint32_t sid) {
        uint4 r = packed[sid];
        r.w = sid;
        if (game->states[sid].n_children == 0 && game->n_players == 2) {
            r.y = rp_f2u(h->payoffs[(size_t)game->states[sid].offset * 2 + 0]);
            r.z = rp_f2u(h->payoffs[(size_t)game->states[sid].offset * 2 + 1]);
        }
        return r;
    };
    std::vector<uint4> kids(h->children.size());
    for (size_t c = 0; c < h->children.size(); ++c) kids[c] = rec_of(h->children[c]);
    CREATE_TRY(hipMalloc(&h->d_kids, std::max<size_t>(kids.size(), 1) * sizeof(uint4)));
    CREATE_TRY(hipMemcpy(h->d_kids, kids.data(), kids.size() * sizeof(uint4), hipMemcpyHostToDevice));
    CREATE_TRY(hipMalloc(&h->d_payoffs, h->payoffs.size() * 4));
    CREATE_TRY(hipMemcpy(h->d_payoffs, h->payoffs.data(), h->payoffs.size() * 4, hipMemcpyHostToDevice));
    CREATE_TRY(hipMalloc(&h->d_info_actions, game->n_infos));
    CREATE_TRY(hipMemcpy(h->d_info_actions, h->info_actions.data(), game->n_infos, hipMemcpyHostToDevice));
    CREATE_TRY(hipMalloc(&h->d_info_player, game->n_infos));
    CREATE_TRY(hipMemcpy(h->d_info_player, h->info_player.data(), game->n_infos, hipMemcpyHostToDevice));
    h->g.states = reinterpret_cast<const uint4*>(h->d_states);
    h->g.children = reinterpret_cast<const uint32_t*>(h->d_children);
    h->g.kids = reinterpret_cast<const uint4*>(h->d_kids);
    h->g.root_rec = packed[game->train_root];
    h->g.root_rec.w = game->train_root;
    h->g.payoffs = reinterpret_cast<const float*>(h->d_payoffs);
    h->g.info_actions = reinterpret_cast<const uint8_t*>(h->d_info_actions);
    h->g.info_player = reinterpret_cast<const uint8_t*>(h->d_info_player);
    {
        // an infoset's rank among its player's infosets and the way back (bmap_index: block maps compacted by walker)
        std::vector<uint32_t> rank(game->n_infos), count(8, 0u);
        const auto owned = [&](uint32_t i) { return h->info_player[i] < game->n_players; };  // rp_game_table_check: at most 8 players
        for (uint32_t i = 0; i < game->n_infos; ++i) rank[i] = owned(i) ? count[h->info_player[i]]++ : 0u;
        uint32_t rank_max = 1;
        for (uint32_t w = 0; w < 8; ++w) {
            h->g.rank_count[w] = count[w];
            rank_max = std::max(rank_max, count[w]);
        }
        h->g.rank_max = rank_max;
        std::vector<uint32_t> tab((size_t)game->n_infos + (size_t)game->n_players * rank_max, 0u);
        for (uint32_t i = 0; i < game->n_infos; ++i) {
            tab[i] = rank[i];
            if (owned(i)) tab[(size_t)game->n_infos + (size_t)h->info_player[i] * rank_max + rank[i]] = i;
        }
        CREATE_TRY(hipMalloc(&h->d_info_rank, tab.size() * 4));
        CREATE_TRY(hipMemcpy(h->d_info_rank, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        h->g.info_rank = reinterpret_cast<const uint32_t*>(h->d_info_rank);
        h->g.rank_info = h->g.info_rank + game->n_infos;
    }
    h->g.n_players = game->n_players;
    h->g.n_infos = game->n_infos;
    h->g.A = game->max_actions;
    h->g.root = game->train_root;
    // tables: a missing Encounter reads (weight 0, regret default_regret, payoff 0, visits 0) (book.rs:93-122)
    CREATE_TRY(hipMalloc(&h->t.regret, cells * 4));
    CREATE_TRY(hipMalloc(&h->t.weight, cells * 4));
    CREATE_TRY(hipMalloc(&h->t.payoff, cells * 4));
    CREATE_TRY(hipMalloc(&h->t.visits, cells * 4));
    CREATE_TRY(hipMemcpy(h->t.regret, h->default_regret.data(), cells * 4, hipMemcpyHostToDevice));
    CREATE_TRY(hipMemset(h->t.weight, 0, cells * 4));
    CREATE_TRY(hipMemset(h->t.payoff, 0, cells * 4));
    CREATE_TRY(hipMemset(h->t.visits, 0, cells * 4));
    CREATE_TRY(hipMalloc(&h->d_counters, (size_t)METRIC_STRIPES * METRIC_STRIDE * sizeof(unsigned long long)));
    CREATE_TRY(hipMemset(h->d_counters, 0, (size_t)METRIC_STRIPES * METRIC_STRIDE * sizeof(unsigned long long)));
    CREATE_TRY(hipMalloc(&h->d_summary, summary_bytes_of(h)));
    CREATE_TRY(hipMalloc(&h->d_itab, (5 * cells + 2 * (size_t)game->n_infos + 4 + 8 * (size_t)game->n_infos + 8) * 4));
    {
        float* f = reinterpret_cast<float*>(h->d_itab);
        h->itab.sigma = f;
        h->itab.q = f + cells;
        h->itab.cum = f + 2 * cells;
        h->itab.total = f + 3 * cells;
        h->itab.keep = reinterpret_cast<uint32_t*>(f + 3 * cells + game->n_infos);
        const size_t used = 3 * cells + 2 * (size_t)game->n_infos;
        h->itab.sq = reinterpret_cast<float2*>(f + ((used + 3) & ~(size_t)3));  // 16-byte aligned: a two-action row is one float4
        const size_t used2 = ((used + 3) & ~(size_t)3) + 2 * cells;
        h->itab.row2 = game->max_actions == 2 ? f + ((used2 + 7) & ~(size_t)7) : nullptr;  // 32-byte aligned rows
    }
    uint32_t maxstack = 1;
    sampled_tree_bounds(h, &h->maxdec, &maxstack, &h->maxint);
    h->sc.maxn = game->max_tree_nodes;
    h->sc.maxs = maxstack;
    if (h->maxdec > 254) {
        rp_mccfr_destroy(h);
        return rp::fail(RP_ERR_CAPACITY, "rp_mccfr_create: more than 254 walker infosets per tree");
    }
    if (chain_lds_bytes() > 64 * 1024) {
        rp_mccfr_destroy(h);
        return rp::fail(RP_ERR_CAPACITY, "rp_mccfr_create: chain tiles need %zu B of LDS", chain_lds_bytes());
    }
    h->use_lds_traverse = traverse_fits_lds(h) && getenv("RP_MCCFR_HBM_SCRATCH") == nullptr;
    h->fuse_maps = getenv("RP_TRAV_UNFUSED") == nullptr;
    // read at creation, for tests: RP_FOLD_SPLIT=1 folds the group maps in k_fold_groups from one group upward, RP_FOLD_SPLIT=0 never
    const char* fold_env = getenv("RP_FOLD_SPLIT");
    h->fold_split_groups = !fold_env ? FOLD_SPLIT_GROUPS : (atoi(fold_env) ? 1u : UINT32_MAX);
    if (h->use_lds_traverse && getenv("RP_TRAV_GENERIC") == nullptr) {
        for (int k = 1; k <= 2 && !h->static_skel; ++k)
            with_skeleton(k, [&](auto gt) {
                if (skel_matches<decltype(gt)>(game, h->children)) h->static_skel = k;
            });
    }
    h->g.rows = nullptr;
    if (h->static_skel && getenv("RP_TRAV_NO_FLAT") == nullptr) {
        std::vector<uint32_t> rows;
        bool ok = false;
        with_skeleton(h->static_skel, [&](auto gt) { ok = build_rows<decltype(gt)>(game, h->children, rec_of, rows, h->g.row_base, h->g.row_fan); });
        if (ok) {
            CREATE_TRY(hipMalloc(&h->d_rows, rows.size() * 4));
            CREATE_TRY(hipMemcpy(h->d_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
            h->g.rows = reinterpret_cast<const uint4*>(h->d_rows);
            h->rows_bytes = rows.size() * 4;
        }
    }
    rc = alloc_batch_buffers(h, batch_size);
    if (rc) {
        rp_mccfr_destroy(h);
        return rc;
    }
#undef CREATE_TRY
    // hipMemset on device memory returns before it has run, and a non-blocking stream does not wait for the null stream: the
    // first launch on this handle's stream could otherwise overtake the initialisation above and be overwritten by it
    (void)hipDeviceSynchronize();
    *out = h;
    return RP_OK;
}

int rp_mccfr_destroy(rp_mccfr* h) {
    if (!h) return RP_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->clk.drain();
    void* ptrs[] = {h->d_info_streams, h->d_chance_streams, h->d_ref_mid, h->d_rows, h->d_states, h->d_children, h->d_kids, h->d_payoffs, h->d_info_actions, h->d_info_player, h->d_info_rank, h->d_scratch,
                    h->d_dec, h->d_sorted, h->d_bmaps, h->d_itab, h->d_summary, h->d_window, h->d_counters, h->t.regret, h->t.weight, h->t.payoff,
                    h->t.visits};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (h->d_nash) (void)hipFree(h->d_nash);
    if (h->d_msub) (void)hipFree(h->d_msub);
    if (h->d_front) (void)hipFree(h->d_front);
    if (h->nash_pinned) (void)hipHostFree(h->nash_pinned);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return RP_OK;
}

int rp_mccfr_set_rng(rp_mccfr* h, rp_rng_kind kind, const rp_hash_streams* st) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_mccfr_set_rng: NULL handle");
    int rc = set_device(h);
    if (rc) return rc;
    if (kind == RP_RNG_COUNTER) {
        h->rng = RP_RNG_COUNTER;
        return RP_OK;
    }
    if (kind != RP_RNG_REFERENCE) return rp::fail(RP_ERR_INVALID, "rp_mccfr_set_rng: unknown rp_rng_kind");
    if (!st || !st->infos || st->n_infos != h->tbl.n_infos || (st->n_chance && !st->chance))
        return rp::fail(RP_ERR_INVALID, "rp_mccfr_set_rng: RP_RNG_REFERENCE needs the hash stream of each of the game's %u infosets", h->tbl.n_infos);
    for (uint32_t i = 0; i < st->n_infos; ++i)
        if (st->infos[i].len > RP_HASH_STREAM_MAX) return rp::fail(RP_ERR_INVALID, "rp_mccfr_set_rng: stream %u is longer than %u bytes", i, RP_HASH_STREAM_MAX);
    for (uint32_t i = 0; i < st->n_chance; ++i)
        if (st->chance[i].len > RP_HASH_STREAM_MAX) return rp::fail(RP_ERR_INVALID, "rp_mccfr_set_rng: chance stream %u is longer than %u bytes", i, RP_HASH_STREAM_MAX);
    for (const rp_state& s : h->states)
        if (s.turn == RP_TURN_CHANCE && s.chance_info > st->n_chance)
            return rp::fail(RP_ERR_INVALID, "rp_mccfr_set_rng: a chance state names chance info %u of %u", s.chance_info, st->n_chance);
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (void** q : {&h->d_info_streams, &h->d_chance_streams, &h->d_ref_mid}) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
    HIP_TRY(hipMalloc(&h->d_info_streams, sizeof(rp_hash_stream) * std::max<size_t>(1, st->n_infos)));
    HIP_TRY(hipMalloc(&h->d_chance_streams, sizeof(rp_hash_stream) * std::max<size_t>(1, st->n_chance)));
    HIP_TRY(hipMalloc(&h->d_ref_mid, sizeof(rp_sip_mid) * ((size_t)st->n_infos + st->n_chance + 1)));
    HIP_TRY(hipMemcpy(h->d_info_streams, st->infos, sizeof(rp_hash_stream) * st->n_infos, hipMemcpyHostToDevice));
    if (st->n_chance) HIP_TRY(hipMemcpy(h->d_chance_streams, st->chance, sizeof(rp_hash_stream) * st->n_chance, hipMemcpyHostToDevice));
    h->n_chance_infos = st->n_chance;
    h->ref_mid_epoch = ~0ull;
    h->rng = RP_RNG_REFERENCE;
    return RP_OK;
}

int rp_mccfr_step_async(rp_mccfr* h, uint32_t steps) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_mccfr_step_async: NULL handle");
    int rc = set_device(h);
    if (rc) return rc;
    if (h->mode == RP_UPDATE_COMPOSED && (rc = composed_supported(h))) return rc;
    for (uint32_t i = 0; i < steps; ++i)
        if ((rc = enqueue_step(h))) return rc;
    return RP_OK;
}

int rp_mccfr_sync(rp_mccfr* h) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_mccfr_sync: NULL handle");
    int rc = set_device(h);
    if (rc) return rc;
    rc = check_device_errors(h);
    h->clk.drain();
    return rc;
}

int rp_mccfr_step(rp_mccfr* h) {
    int rc = rp_mccfr_step_async(h, 1);
    if (rc) return rc;
    return rp_mccfr_sync(h);
}

int rp_mccfr_solve(rp_mccfr* h, uint64_t trees) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_mccfr_solve: NULL handle");
    uint64_t steps = trees / h->batch;
    while (steps) {  // bounded queue depth; the loop shape of Solver::solve (solver.rs:111-122)
        const uint32_t n = (uint32_t)std::min<uint64_t>(steps, 256);
        int rc = rp_mccfr_step_async(h, n);
        if (rc) return rc;
        if ((rc = rp_mccfr_sync(h))) return rc;
        steps -= n;
    }
    return RP_OK;
}

int rp_mccfr_spend(rp_mccfr* h, double seconds, uint64_t* iterations, double* elapsed) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_mccfr_spend: NULL handle");
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t it = 0;
    double el = 0.0;
    for (;;) {
        el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (el >= seconds) break;
        int rc = rp_mccfr_step(h);
        if (rc) return rc;
        it += 1;
    }
    if (iterations) *iterations = it;
    if (elapsed) *elapsed = el;
    return RP_OK;
}

// Trainer::train: rp::train_loop (common.cpp).  The counters live on the device: they are read back at a checkpoint and for the
// summary only, so a flush reports those of the last checkpoint.
int rp_mccfr_train(rp_mccfr* h, uint64_t max_steps, double max_seconds, double log_interval, double flush_interval,
                   rp_train_event_fn on_event, void* user, const volatile int* interrupt, char* summary, size_t summary_cap) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_mccfr_train: NULL handle");
    auto step = [h](TrainCounts& c) {
        const int rc = rp_mccfr_step(h);
        c.epoch = h->epoch;
        return rc;
    };
    auto refresh = [h](TrainCounts& c) { return rp_mccfr_counters(h, &c.nodes, &c.infos); };
    return train_loop(step, refresh, max_steps, max_seconds, log_interval, flush_interval, on_event, user, interrupt, summary, summary_cap);
}

int rp_mccfr_epoch(rp_mccfr* h, uint64_t* epoch) {
    if (!h || !epoch) return rp::fail(RP_ERR_INVALID, "rp_mccfr_epoch: NULL argument");
    *epoch = h->epoch;
    return RP_OK;
}

int rp_mccfr_counters(rp_mccfr* h, uint64_t* nodes, uint64_t* infos) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_mccfr_counters: NULL handle");
    int rc = set_device(h);
    if (rc) return rc;
    unsigned long long c[3];
    if ((rc = read_counters(h, c))) return rc;
    if (nodes) *nodes = c[0];
    if (infos) *infos = c[1];
    return RP_OK;
}

int rp_mccfr_get(rp_mccfr* h, uint32_t info, uint32_t edge, rp_encounter* out) {
    if (!h || !out) return rp::fail(RP_ERR_INVALID, "rp_mccfr_get: NULL argument");
    if (info >= h->tbl.n_infos || edge >= h->info_actions[info]) return rp::fail(RP_ERR_INVALID, "rp_mccfr_get: out of range");
    int rc = set_device(h);
    if (rc) return rc;
    const size_t c = (size_t)info * h->tbl.max_actions + edge;
    HIP_TRY(hipMemcpyAsync(&out->regret, h->t.regret + c, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&out->weight, h->t.weight + c, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&out->payoff, h->t.payoff + c, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&out->visits, h->t.visits + c, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return RP_OK;
}

int rp_mccfr_set(rp_mccfr* h, uint32_t info, uint32_t edge, const rp_encounter* in) {
    if (!h || !in) return rp::fail(RP_ERR_INVALID, "rp_mccfr_set: NULL argument");
    if (info >= h->tbl.n_infos || edge >= h->info_actions[info]) return rp::fail(RP_ERR_INVALID, "rp_mccfr_set: out of range");
    int rc = set_device(h);
    if (rc) return rc;
    const size_t c = (size_t)info * h->tbl.max_actions + edge;
    HIP_TRY(hipMemcpyAsync(h->t.regret + c, &in->regret, 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->t.weight + c, &in->weight, 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->t.payoff + c, &in->payoff, 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->t.visits + c, &in->visits, 4, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->tables_version += 1;
    return RP_OK;
}

int rp_mccfr_export(rp_mccfr* h, rp_encounter* rows, uint64_t cap) {
    if (!h || !rows) return rp::fail(RP_ERR_INVALID, "rp_mccfr_export: NULL argument");
    const size_t cells = (size_t)h->tbl.n_infos * h->tbl.max_actions;
    if (cap < cells) return rp::fail(RP_ERR_INVALID, "rp_mccfr_export: need %zu rows", cells);
    int rc = set_device(h);
    if (rc) return rc;
    std::vector<float> r, w, p;
    std::vector<uint32_t> v;
    if ((rc = fetch_tables(h, r, w, p, v))) return rc;
    for (size_t c = 0; c < cells; ++c) rows[c] = rp_encounter{w[c], r[c], p[c], v[c]};
    return RP_OK;
}

int rp_mccfr_import(rp_mccfr* h, const rp_encounter* rows, uint64_t n, uint64_t epoch) {
    if (!h || !rows) return rp::fail(RP_ERR_INVALID, "rp_mccfr_import: NULL argument");
    const size_t cells = (size_t)h->tbl.n_infos * h->tbl.max_actions;
    if (n != cells) return rp::fail(RP_ERR_INVALID, "rp_mccfr_import: expected %zu rows", cells);
    int rc = set_device(h);
    if (rc) return rc;
    std::vector<float> r(cells), w(cells), p(cells);
    std::vector<uint32_t> v(cells);
    for (size_t c = 0; c < cells; ++c) {
        w[c] = rows[c].weight; r[c] = rows[c].regret; p[c] = rows[c].payoff; v[c] = rows[c].visits;
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(h->t.regret, r.data(), cells * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->t.weight, w.data(), cells * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->t.payoff, p.data(), cells * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->t.visits, v.data(), cells * 4, hipMemcpyHostToDevice));
    h->tables_version += 1;
    h->epoch = epoch;
    return RP_OK;
}

int rp_mccfr_policy(rp_mccfr* h, uint32_t info, rp_dist_kind kind, float* out, uint32_t* n) {
    if (!h || !out) return rp::fail(RP_ERR_INVALID, "rp_mccfr_policy: NULL argument");
    if (info >= h->tbl.n_infos) return rp::fail(RP_ERR_INVALID, "rp_mccfr_policy: info out of range");
    int rc = set_device(h);
    if (rc) return rc;
    const uint32_t A = h->tbl.max_actions, na = h->info_actions[info];
    float reg[RP_MAX_ACTIONS], wgt[RP_MAX_ACTIONS];
    HIP_TRY(hipMemcpyAsync(reg, h->t.regret + (size_t)info * A, na * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(wgt, h->t.weight + (size_t)info * A, na * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (kind == RP_DIST_ITERATED) {  // profile.rs:47-51
        float denom = 0.0f;
        for (uint32_t a = 0; a < na; ++a) denom += rp_maxf(reg[a], RP_EPSILON);
        for (uint32_t a = 0; a < na; ++a) out[a] = rp_maxf(reg[a], RP_EPSILON) / denom;
    } else if (kind == RP_DIST_AVERAGED) {  // profile.rs:40-44
        float sum = 0.0f;
        for (uint32_t a = 0; a < na; ++a) sum += rp_maxf(wgt[a], RP_EPSILON);
        for (uint32_t a = 0; a < na; ++a) out[a] = rp_maxf(wgt[a], RP_EPSILON) / sum;
    } else if (kind == RP_DIST_SAMPLING) {  // flow.rs:33-42
        float denom = 0.0f;
        for (uint32_t a = 0; a < na; ++a) denom += rp_maxf(wgt[a], RP_EPSILON);
        denom = denom + h->hp.smoothing;
        float raw[RP_MAX_ACTIONS], z = 0.0f;
        for (uint32_t a = 0; a < na; ++a) {
            raw[a] = rp_maxf((rp_maxf(wgt[a], RP_EPSILON) / h->hp.temperature + h->hp.smoothing) / denom, h->hp.curiosity);
            z += raw[a];
        }
        for (uint32_t a = 0; a < na; ++a) out[a] = raw[a] / z;
    } else {
        return rp::fail(RP_ERR_INVALID, "rp_mccfr_policy: unknown distribution kind");
    }
    if (n) *n = na;
    return RP_OK;
}

int rp_mccfr_sum_regret(rp_mccfr* h, float* out) {
    if (!h || !out) return rp::fail(RP_ERR_INVALID, "rp_mccfr_sum_regret: NULL argument");
    int rc = set_device(h);
    if (rc) return rc;
    std::vector<float> r, w, p;
    std::vector<uint32_t> v;
    if ((rc = fetch_tables(h, r, w, p, v))) return rc;
    float s = 0.0f;
    for (uint32_t info = 0; info < h->tbl.n_infos; ++info)
        for (uint32_t a = 0; a < h->info_actions[info]; ++a) s += rp_maxf(r[(size_t)info * h->tbl.max_actions + a], 0.0f);
    *out = s / (float)(h->epoch > 1 ? h->epoch : 1);
    return RP_OK;
}

int rp_mccfr_set_batch(rp_mccfr* h, uint32_t batch_size) {
    if (!h || batch_size == 0) return rp::fail(RP_ERR_INVALID, "rp_mccfr_set_batch: bad argument");
    int rc = set_device(h);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if ((rc = alloc_batch_buffers(h, batch_size))) return rc;
    h->batch = batch_size;
    return RP_OK;
}

// rp_mccfr_create with the update mode chosen up front (a caller that wants the fast, shardable composed update does not have to
// know about a second call; schedules the composed mode cannot express are refused here, not at the first step)
int rp_mccfr_create_mode(const rp_game_table* game, rp_regret_kind r, rp_weight_kind w, rp_sampling_kind s, uint32_t batch_size,
                         const rp_hyper* hp, uint64_t seed, int device, rp_update_mode mode, rp_mccfr** out) {
    if (mode != RP_UPDATE_ORDERED && mode != RP_UPDATE_COMPOSED) return rp::fail(RP_ERR_INVALID, "rp_mccfr_create_mode: unknown update mode");
    int rc = rp_mccfr_create(game, r, w, s, batch_size, hp, seed, device, out);
    if (rc) return rc;
    (*out)->mode = mode;
    if (mode == RP_UPDATE_COMPOSED && (rc = composed_supported(*out))) {
        rp_mccfr_destroy(*out);
        *out = nullptr;
        return rc;
    }
    return RP_OK;
}

int rp_mccfr_set_update_mode(rp_mccfr* h, rp_update_mode mode) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_mccfr_set_update_mode: NULL handle");
    if (mode != RP_UPDATE_ORDERED && mode != RP_UPDATE_COMPOSED) return rp::fail(RP_ERR_INVALID, "unknown update mode");
    h->mode = mode;
    return RP_OK;
}

int rp_mccfr_set_stream(rp_mccfr* h, void* hip_stream) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_mccfr_set_stream: NULL handle");
    int rc = set_device(h);
    if (rc) return rc;
    return swap_stream(h->stream, h->own_stream, hip_stream);
}

int rp_mccfr_set_shard(rp_mccfr* h, uint32_t rank, uint32_t world) {
    if (!h || world == 0 || rank >= world) return rp::fail(RP_ERR_INVALID, "rp_mccfr_set_shard: bad rank/world");
    h->rank = rank;
    h->world = world;
    return RP_OK;
}

int rp_mccfr_summary_bytes(rp_mccfr* h, size_t* bytes) {
    if (!h || !bytes) return rp::fail(RP_ERR_INVALID, "rp_mccfr_summary_bytes: NULL argument");
    *bytes = summary_bytes_of(h);
    return RP_OK;
}

int rp_mccfr_step_local(rp_mccfr* h, void* summary_dev) {
    if (!h || !summary_dev) return rp::fail(RP_ERR_INVALID, "rp_mccfr_step_local: NULL argument");
    int rc = set_device(h);
    if (rc) return rc;
    if ((rc = composed_supported(h))) return rc;
    const StepParams p = make_params(h);
    return launch_batch_summary(h, p, summary_dev);
}

int rp_mccfr_step_apply(rp_mccfr* h, const void* gathered_dev, uint32_t world) {
    if (!h || !gathered_dev || world == 0) return rp::fail(RP_ERR_INVALID, "rp_mccfr_step_apply: bad argument");
    int rc = set_device(h);
    if (rc) return rc;
    const uint32_t ncell = h->tbl.n_infos * h->tbl.max_actions;
    hipLaunchKernelGGL(k_fold, dim3((ncell + 255) / 256), dim3(256), 0, h->stream, h->g, h->t,
                       reinterpret_cast<const unsigned char*>(gathered_dev), summary_bytes_of(h), world);
    HIP_TRY(hipGetLastError());
    h->tables_version += 1;
    h->epoch += 1;
    return RP_OK;
}

// The periodic exchange (north_star: "periodic RCCL all-reduce of regret/strategy tables"): a rank runs `window` local
// steps against the table as it stood at the start of the window — the table is not touched, the epoch advances (the
// sampled trees, the walker and the discounts are those of each step) — and folds each step's composed maps into ONE
// window summary; the summaries are all-gathered once per window and applied in rank order.  window = 1 is
// step_local + step_apply.
int rp_mccfr_window_local(rp_mccfr* h, void* window_dev, int first) {
    if (!h || !window_dev) return rp::fail(RP_ERR_INVALID, "rp_mccfr_window_local: NULL argument");
    int rc = set_device(h);
    if (rc) return rc;
    if ((rc = composed_supported(h))) return rc;
    const StepParams p = make_params(h);
    if ((rc = launch_batch_summary(h, p, h->d_summary))) return rc;
    const uint32_t ncell = h->tbl.n_infos * h->tbl.max_actions;
    hipLaunchKernelGGL(k_accumulate, dim3((ncell + 255) / 256), dim3(256), 0, h->stream, h->g, reinterpret_cast<unsigned char*>(window_dev),
                       reinterpret_cast<const unsigned char*>(h->d_summary), first ? 1u : 0u);
    HIP_TRY(hipGetLastError());
    h->epoch += 1;
    return RP_OK;
}

int rp_mccfr_window_apply(rp_mccfr* h, const void* gathered_dev, uint32_t world) {
    if (!h || !gathered_dev || world == 0) return rp::fail(RP_ERR_INVALID, "rp_mccfr_window_apply: bad argument");
    int rc = set_device(h);
    if (rc) return rc;
    const uint32_t ncell = h->tbl.n_infos * h->tbl.max_actions;
    hipLaunchKernelGGL(k_fold, dim3((ncell + 255) / 256), dim3(256), 0, h->stream, h->g, h->t,
                       reinterpret_cast<const unsigned char*>(gathered_dev), summary_bytes_of(h), world);
    HIP_TRY(hipGetLastError());
    h->tables_version += 1;
    return RP_OK;
}

int rp_mccfr_step_comm(rp_mccfr* h, rp_comm* c, uint32_t steps, uint32_t window) {
    if (!h || !c) return rp::fail(RP_ERR_INVALID, "rp_mccfr_step_comm: NULL argument");
    if (window == 0) window = 1;
    int rc = set_device(h);
    if (rc) return rc;
    if ((rc = composed_supported(h))) return rc;
    const uint32_t world = (uint32_t)rp::comm_world(c);
    h->rank = (uint32_t)rp::comm_rank(c);
    h->world = world;
    const size_t nb = summary_bytes_of(h);
    if (!h->d_window || h->window_world != world) {  // [mine][all ranks]
        if (h->d_window) (void)hipFree(h->d_window);
        h->d_window = nullptr;
        HIP_TRY(hipMalloc(&h->d_window, nb * (world + 1)));
        h->window_world = world;
    }
    unsigned char* mine = reinterpret_cast<unsigned char*>(h->d_window);
    unsigned char* all = mine + nb;
    uint32_t pending = 0;
    for (uint32_t s = 0; s < steps; ++s) {
        if ((rc = rp_mccfr_window_local(h, mine, pending == 0))) return rc;
        pending += 1;
        if (pending == window || s + 1 == steps) {
            if ((rc = rp::comm_all_gather(c, mine, all, nb, h->stream))) return rc;
            if ((rc = rp_mccfr_window_apply(h, all, world))) return rc;
            pending = 0;
        }
    }
    return RP_OK;
}

int rp_mccfr_profile(rp_mccfr* h, int enable) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_mccfr_profile: NULL handle");
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->clk.drain();
    h->clk.on = enable != 0;
    h->clk.reset();
    return RP_OK;
}

int rp_game_skeleton(const rp_game_table* game, int* out) {
    if (!game || !out) return rp::fail(RP_ERR_INVALID, "rp_game_skeleton: NULL argument");
    int rc = rp_game_table_check(game);
    if (rc) return rc;
    const std::vector<uint32_t> children(game->children, game->children + game->n_children);
    *out = skel_matches<KuhnSkel>(game, children) ? 1 : (skel_matches<LeducSkel>(game, children) ? 2 : 0);
    return RP_OK;
}

int rp_mccfr_traversal_rows_bytes(rp_mccfr* h, size_t* out) {
    if (!h || !out) return rp::fail(RP_ERR_INVALID, "rp_mccfr_traversal_rows_bytes: NULL argument");
    *out = h->rows_bytes;
    return RP_OK;
}

int rp_mccfr_traversal_variant(rp_mccfr* h, int* out) {
    if (!h || !out) return rp::fail(RP_ERR_INVALID, "rp_mccfr_traversal_variant: NULL argument");
    *out = h->static_skel ? 2 : (h->use_lds_traverse ? 1 : 0);
    return RP_OK;
}

int rp_mccfr_fold_variant(rp_mccfr* h, int* out) {
    if (!h || !out) return rp::fail(RP_ERR_INVALID, "rp_mccfr_fold_variant: NULL argument");
    *out = fold_split(h, h->batch) ? 1 : 0;
    return RP_OK;
}

int rp_mccfr_kernel_time(rp_mccfr* h, const char* name, double* total_ms, uint64_t* launches) {
    if (!h || !name) return rp::fail(RP_ERR_INVALID, "rp_mccfr_kernel_time: NULL argument");
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    return kernel_time(h->clk, "rp_mccfr_kernel_time", name, total_ms, launches);
}

// ---- Solver::exploitability (solver.rs:327-337) on the host: validation, not the hot path -------------
// Full-tree best response exactly as CfrNash does it (nash.rs:31-38,103-194): per-infoset argmax of
// sum_{n in span} external_reach * average-strategy value, then evaluation with those choices.
namespace {
struct XNode {
    uint32_t state;
    int32_t parent, edge;
    int32_t kids[RP_MAX_ACTIONS];
};
struct XCtx {
    const rp_mccfr* h;
    const float* weight;
    std::vector<XNode> nodes;
    float wt(uint32_t info, uint32_t a) const { return rp_maxf(weight[(size_t)info * h->tbl.max_actions + a], RP_EPSILON); }
    float averaged(uint32_t info, uint32_t a) const {
        float sum = 0.0f;
        for (uint32_t k = 0; k < h->info_actions[info]; ++k) sum += wt(info, k);
        return wt(info, a) / sum;
    }
    float value(int32_t n, uint32_t hero, const int32_t* br) const {
        const XNode& nd = nodes[n];
        const rp_state& st = h->states[nd.state];
        if (st.n_children == 0) return h->payoffs[(size_t)st.offset * h->tbl.n_players + hero];
        if (st.turn == RP_TURN_CHANCE) {
            float s = 0.0f;
            for (uint32_t k = 0; k < st.n_children; ++k) s += value(nd.kids[k], hero, br);
            return s / (float)st.n_children;
        }
        if (st.turn == hero && br) return value(nd.kids[br[st.info]], hero, br);
        float s = 0.0f;
        for (uint32_t k = 0; k < st.n_children; ++k) s += averaged(st.info, k) * value(nd.kids[k], hero, br);
        return s;
    }
    float reach(int32_t n, uint32_t hero) const {
        float p = 1.0f;
        const XNode* nd = &nodes[n];
        while (nd->parent >= 0) {
            const XNode& par = nodes[nd->parent];
            const rp_state& ps = h->states[par.state];
            if (ps.turn != RP_TURN_CHANCE && ps.turn != hero) p = p * averaged(ps.info, (uint32_t)nd->edge);
            nd = &par;
        }
        return p;
    }
};
}  // namespace

int rp_mccfr_exploitability(rp_mccfr* h, float* out) {
    if (!h || !out) return rp::fail(RP_ERR_INVALID, "rp_mccfr_exploitability: NULL argument");
    int rc = set_device(h);
    if (rc) return rc;
    std::vector<float> r, w, p;
    std::vector<uint32_t> v;
    if ((rc = fetch_tables(h, r, w, p, v))) return rc;
    XCtx x{h, w.data(), {}};
    // VanillaSampling tree in TreeBuilder's pop-last order (builder.rs:141-161) so spans ascend like the reference's
    struct Leaf { uint32_t state; int32_t parent, edge; };
    std::vector<Leaf> todo;
    auto push = [&](uint32_t state, int32_t parent, int32_t edge) {
        XNode nd{state, parent, edge, {}};
        for (auto& k : nd.kids) k = -1;
        x.nodes.push_back(nd);
        const int32_t me = (int32_t)x.nodes.size() - 1;
        if (parent >= 0) x.nodes[parent].kids[edge] = me;
        const rp_state& st = h->states[state];
        for (uint32_t k = 0; k < st.n_children; ++k) todo.push_back(Leaf{h->children[st.offset + k], me, (int32_t)k});
    };
    push(h->tbl.exploit_root, -1, -1);
    while (!todo.empty()) {
        Leaf lf = todo.back();
        todo.pop_back();
        push(lf.state, lf.parent, lf.edge);
    }
    std::vector<int32_t> br(h->tbl.n_infos, 0);
    std::vector<float> cfv((size_t)h->tbl.n_infos * RP_MAX_ACTIONS);
    float total = 0.0f;
    for (uint32_t hero = 0; hero < h->tbl.n_players; ++hero) {
        std::fill(cfv.begin(), cfv.end(), 0.0f);
        for (size_t i = 0; i < x.nodes.size(); ++i) {
            const XNode& nd = x.nodes[i];
            const rp_state& st = h->states[nd.state];
            if (st.turn != hero || st.n_children == 0) continue;
            for (uint32_t a = 0; a < st.n_children; ++a) {
                const int32_t c = nd.kids[a];
                cfv[(size_t)st.info * RP_MAX_ACTIONS + a] += x.reach(c, hero) * x.value(c, hero, nullptr);
            }
        }
        for (uint32_t info = 0; info < h->tbl.n_infos; ++info) {
            br[info] = 0;
            if (h->info_player[info] != hero) continue;
            float best = cfv[(size_t)info * RP_MAX_ACTIONS];
            for (uint32_t a = 1; a < h->info_actions[info]; ++a)
                if (cfv[(size_t)info * RP_MAX_ACTIONS + a] >= best) {  // max_by keeps the last maximum (nash.rs:184-193)
                    best = cfv[(size_t)info * RP_MAX_ACTIONS + a];
                    br[info] = (int32_t)a;
                }
        }
        total += x.value(0, hero, br.data());
    }
    *out = total / (float)h->tbl.n_players;
    return RP_OK;
}

}  // extern "C"

// ---- CfrNash::exploitability on the device (mccfr_nash.hpp) ---------------------------------------------------------------------------
namespace {

size_t nash_one_bytes(const rp_mccfr* h, size_t n_nodes) {
    return 4 * (n_nodes + 2 * (size_t)h->tbl.n_infos * h->tbl.max_actions + h->tbl.n_infos);
}

// The static data, on the first call that asks: the expansion (the loop of rp_mccfr_exploitability above, node for node), the level
// lists, the spans, one upload.  Synchronises; every later call only launches.
int nash_prepare(rp_mccfr* h) {
    if (h->nash_variant >= 0) return RP_OK;
    const char* force = getenv("RP_NASH_VARIANT");
    if (force && std::string(force) != "one" && std::string(force) != "levels")
        return rp::fail(RP_ERR_INVALID, "RP_NASH_VARIANT is '%s': one or levels", force);
    // VanillaSampling tree in TreeBuilder's pop-last order (builder.rs:141-161)
    std::vector<XNode> nodes;
    std::vector<uint32_t> depth;
    struct Leaf { uint32_t state; int32_t parent, edge; };
    std::vector<Leaf> todo;
    auto push = [&](uint32_t state, int32_t parent, int32_t edge) {
        XNode nd{state, parent, edge, {}};
        for (auto& k : nd.kids) k = -1;
        nodes.push_back(nd);
        depth.push_back(parent >= 0 ? depth[parent] + 1 : 0u);
        const int32_t me = (int32_t)nodes.size() - 1;
        if (parent >= 0) nodes[parent].kids[edge] = me;
        const rp_state& st = h->states[state];
        for (uint32_t k = 0; k < st.n_children; ++k) todo.push_back(Leaf{h->children[st.offset + k], me, (int32_t)k});
    };
    push(h->tbl.exploit_root, -1, -1);
    while (!todo.empty()) {
        if (nodes.size() >= NASH_MAX_NODES)
            return rp::fail(RP_ERR_CAPACITY, "the tree from exploit_root has more than %u nodes: the best response on the device cannot hold it", NASH_MAX_NODES);
        Leaf lf = todo.back();
        todo.pop_back();
        push(lf.state, lf.parent, lf.edge);
    }
    const size_t n = nodes.size(), NI = h->tbl.n_infos, cells = NI * h->tbl.max_actions, np = h->tbl.n_players;
    uint32_t n_levels = 0;
    for (uint32_t d : depth) n_levels = std::max(n_levels, d + 1);
    const bool fits = nash_one_bytes(h, n) <= NASH_ONE_LDS_BYTES;
    const int variant = force ? (std::string(force) == "one" ? 0 : 1) : (fits ? 0 : 1);
    const bool in_lds = variant == 0 && fits;
    // one image, in words: rec (16-byte records first), kids, level_nodes, level_off, span_nodes, span_off | avg (a copy per hero for
    // k_nash_one<false>), cfv, values, expl, choice (bytes); v (not initialised) behind it
    std::vector<uint32_t> img;
    img.reserve(8 * n + 3 * cells + 2 * NI + n_levels + 64);
    std::vector<uint32_t> level_off(n_levels + 1, 0u), span_off(NI + 1, 0u);
    uint32_t kid0 = 0;
    for (size_t i = 0; i < n; ++i) {
        const rp_state& st = h->states[nodes[i].state];
        const uint32_t y = st.n_children == 0 ? st.offset : st.info;
        img.insert(img.end(), {(uint32_t)st.turn | ((uint32_t)st.n_children << 8) | ((uint32_t)(nodes[i].edge < 0 ? 0 : nodes[i].edge) << 16), y,
                               nodes[i].parent < 0 ? NASH_ROOT : (uint32_t)nodes[i].parent, kid0});
        kid0 += st.n_children;
        level_off[depth[i] + 1] += 1;
        if (st.n_children != 0 && st.turn != RP_TURN_CHANCE) span_off[st.info + 1] += 1;
    }
    const size_t o_kids = img.size();
    for (size_t i = 0; i < n; ++i)
        for (uint32_t k = 0; k < h->states[nodes[i].state].n_children; ++k) img.push_back((uint32_t)nodes[i].kids[k]);
    img.push_back(0u);  // a tree of one node has no kid
    for (uint32_t l = 0; l < n_levels; ++l) level_off[l + 1] += level_off[l];
    for (size_t i = 0; i < NI; ++i) span_off[i + 1] += span_off[i];
    const size_t o_level_nodes = img.size();
    img.resize(img.size() + n);
    {
        std::vector<uint32_t> at(level_off.begin(), level_off.end() - 1);
        for (size_t i = 0; i < n; ++i) img[o_level_nodes + at[depth[i]]++] = (uint32_t)i;  // ascending node index inside a level
    }
    const size_t o_level_off = img.size();
    img.insert(img.end(), level_off.begin(), level_off.end());
    const size_t o_span_nodes = img.size();
    img.resize(img.size() + span_off[NI] + 1);
    {
        std::vector<uint32_t> at(span_off.begin(), span_off.end() - 1);
        for (size_t i = 0; i < n; ++i) {
            const rp_state& st = h->states[nodes[i].state];
            if (st.n_children != 0 && st.turn != RP_TURN_CHANCE) img[o_span_nodes + at[st.info]++] = (uint32_t)i;  // ascending node index
        }
    }
    const size_t o_span_off = img.size();
    img.insert(img.end(), span_off.begin(), span_off.end());
    const size_t o_avg = img.size(), avg_words = (variant == 0 && !in_lds ? np : 1) * cells;
    const size_t o_cfv = o_avg + avg_words, o_values = o_cfv + cells, o_expl = o_values + np, o_choice = o_expl + 1;
    img.resize(o_choice + (NI + 3) / 4, 0u);
    const size_t o_v = img.size(), v_words = in_lds ? 0 : np * n;
    void* d = nullptr;
    if (hipMalloc(&d, (o_v + v_words) * 4) != hipSuccess) {
        (void)hipGetLastError();
        return rp::fail(RP_ERR_CAPACITY, "the best response on the device needs %zu bytes for a tree of %zu nodes", (o_v + v_words) * 4, n);
    }
    if (hipMemcpy(d, img.data(), img.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return rp::fail(RP_ERR_HIP, "nash_prepare: the upload of the tree failed");
    }
    uint32_t* w = reinterpret_cast<uint32_t*>(d);
    h->d_nash = d;
    h->nt = NashTree{reinterpret_cast<const uint4*>(w), w + o_kids, w + o_level_nodes, w + o_level_off, w + o_span_nodes, w + o_span_off,
                     (uint32_t)n, n_levels};
    h->nw = NashWork{reinterpret_cast<float*>(w + o_avg), reinterpret_cast<float*>(w + o_cfv), reinterpret_cast<uint8_t*>(w + o_choice),
                     reinterpret_cast<float*>(w + o_values), reinterpret_cast<float*>(w + o_expl),
                     v_words ? reinterpret_cast<float*>(w + o_v) : nullptr};
    h->nash_level_size.resize(n_levels);
    for (uint32_t l = 0; l < n_levels; ++l) h->nash_level_size[l] = level_off[l + 1] - level_off[l];
    h->nash_in_lds = in_lds;
    h->nash_variant = variant;
    return RP_OK;
}

// every phase of one call, queued on the handle's stream; `out_dev` (may be NULL) receives the exploitability, as does NashWork::expl
int launch_nash(rp_mccfr* h, float* out_dev) {
    int rc = nash_prepare(h);
    if (rc) return rc;
    const NashTree& T = h->nt;
    const uint32_t np = h->tbl.n_players, NI = h->tbl.n_infos, cells = NI * h->tbl.max_actions;
    const auto blocks = [](uint32_t n) { return (n + NASH_THREADS - 1) / NASH_THREADS; };
    if (h->nash_variant == 0) {
        if (h->nash_in_lds)
            hipLaunchKernelGGL((k_nash_one<true>), dim3(np), dim3(NASH_ONE_THREADS), nash_one_bytes(h, T.n_nodes), h->stream, T, h->g, h->t, h->nw);
        else
            hipLaunchKernelGGL((k_nash_one<false>), dim3(np), dim3(NASH_ONE_THREADS), 0, h->stream, T, h->g, h->t, h->nw);
        hipLaunchKernelGGL(k_nash_final, dim3(1), dim3(1), 0, h->stream, h->g, h->nw, h->nw.values, (size_t)1, out_dev);
    } else {
        hipLaunchKernelGGL(k_nash_avg, dim3(blocks(NI)), dim3(NASH_THREADS), 0, h->stream, h->g, h->t, h->nw);
        for (uint32_t level = T.n_levels; level-- > 0;)
            hipLaunchKernelGGL((k_nash_level<false>), dim3(blocks(h->nash_level_size[level]), np), dim3(NASH_THREADS), 0, h->stream, T, h->g, h->nw, level);
        hipLaunchKernelGGL(k_nash_term, dim3(blocks(T.n_nodes), np), dim3(NASH_THREADS), 0, h->stream, T, h->g, h->nw);
        hipLaunchKernelGGL(k_nash_cfv, dim3(blocks(cells)), dim3(NASH_THREADS), 0, h->stream, T, h->g, h->nw);
        hipLaunchKernelGGL(k_nash_choice, dim3(blocks(NI)), dim3(NASH_THREADS), 0, h->stream, h->g, h->nw);
        for (uint32_t level = T.n_levels; level-- > 0;)
            hipLaunchKernelGGL((k_nash_level<true>), dim3(blocks(h->nash_level_size[level]), np), dim3(NASH_THREADS), 0, h->stream, T, h->g, h->nw, level);
        hipLaunchKernelGGL(k_nash_final, dim3(1), dim3(1), 0, h->stream, h->g, h->nw, h->nw.v, (size_t)T.n_nodes, out_dev);
    }
    HIP_TRY(hipGetLastError());
    return RP_OK;
}

}  // namespace

extern "C" {

int rp_mccfr_exploitability_device(rp_mccfr* h, float* out_dev) {
    if (!out_dev) return rp::fail(RP_ERR_INVALID, "rp_mccfr_exploitability_device: out_dev is NULL");
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_mccfr_exploitability_device: h is NULL");
    int rc = set_device(h);
    if (rc) return rc;
    return launch_nash(h, out_dev);
}

int rp_mccfr_best_response(rp_mccfr* h, float* exploitability, float* values, uint8_t* choice, float* cfv) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_mccfr_best_response: h is NULL");
    int rc = set_device(h);
    if (rc) return rc;
    if ((rc = launch_nash(h, nullptr))) return rc;
    const size_t NI = h->tbl.n_infos;
    if (exploitability) HIP_TRY(hipMemcpyAsync(exploitability, h->nw.expl, 4, hipMemcpyDeviceToHost, h->stream));
    if (values) HIP_TRY(hipMemcpyAsync(values, h->nw.values, 4 * (size_t)h->tbl.n_players, hipMemcpyDeviceToHost, h->stream));
    if (choice) HIP_TRY(hipMemcpyAsync(choice, h->nw.choice, NI, hipMemcpyDeviceToHost, h->stream));
    if (cfv) HIP_TRY(hipMemcpyAsync(cfv, h->nw.cfv, 4 * NI * h->tbl.max_actions, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return RP_OK;
}

int rp_mccfr_nash_variant(rp_mccfr* h, int* out) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_mccfr_nash_variant: h is NULL");
    if (!out) return rp::fail(RP_ERR_INVALID, "rp_mccfr_nash_variant: out is NULL");
    int rc = set_device(h);
    if (rc) return rc;
    if ((rc = nash_prepare(h))) return rc;
    *out = h->nash_variant;
    return RP_OK;
}

int rp_mccfr_solve_to(rp_mccfr* h, float target, uint32_t check_every, uint64_t max_steps, uint64_t* steps, float* exploitability,
                      int* reached) {
    if (check_every == 0) return rp::fail(RP_ERR_INVALID, "rp_mccfr_solve_to: check_every must be > 0");
    if (target != target) return rp::fail(RP_ERR_INVALID, "rp_mccfr_solve_to: target is NaN");
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_mccfr_solve_to: h is NULL");
    int rc = set_device(h);
    if (rc) return rc;
    if (h->mode == RP_UPDATE_COMPOSED && (rc = composed_supported(h))) return rc;
    if ((rc = nash_prepare(h))) return rc;
    if (!h->nash_pinned) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h->nash_pinned), 4, hipHostMallocMapped));
    void* pinned_dev = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&pinned_dev, h->nash_pinned, 0));
    uint64_t done = 0;
    float value = 0.0f;
    int hit = 0;
    do {  // max_steps = 0: no step, one check of the table as it stands
        const uint32_t n = (uint32_t)std::min<uint64_t>(check_every, max_steps - done);
        for (uint32_t i = 0; i < n; ++i)
            if ((rc = enqueue_step(h))) return rc;
        done += n;
        if ((rc = launch_nash(h, reinterpret_cast<float*>(pinned_dev)))) return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
        value = *reinterpret_cast<volatile float*>(h->nash_pinned);
        hit = value < target ? 1 : 0;
    } while (!hit && done < max_steps);
    if (steps) *steps = done;
    if (exploitability) *exploitability = value;
    if (reached) *reached = hit;
    rc = check_device_errors(h);  // the capacity flags of the steps, once, as rp_mccfr_sync reads them
    h->clk.drain();
    return rc;
}

}  // extern "C"

// ---- the safe subgame re-solve for table games (mccfr_subgame.hpp): pairs by the rule of host_util.hpp ("entry points in pairs") ----
namespace {

// iterations per launch: RP_MCCFR_SUBGAME_SEGMENT (tests), else 8 192
int msub_segment(uint32_t* out) {
    *out = 8192;
    const char* s = getenv("RP_MCCFR_SUBGAME_SEGMENT");
    if (!s || !*s) return RP_OK;
    char* end = nullptr;
    const long v = strtol(s, &end, 10);
    if (*end || v < 1 || v > (long)RP_MCCFR_SUBGAME_MAX_ITERATIONS)
        return rp::fail(RP_ERR_INVALID, "RP_MCCFR_SUBGAME_SEGMENT is '%s': 1 .. %u", s, RP_MCCFR_SUBGAME_MAX_ITERATIONS);
    *out = (uint32_t)v;
    return RP_OK;
}

int msub_check_args(const char* who, const rp_mccfr_subgame_args* args) {
    if (!args) return rp::fail(RP_ERR_INVALID, "%s: args is NULL", who);
    if (args->iterations < 1 || args->iterations > RP_MCCFR_SUBGAME_MAX_ITERATIONS)
        return rp::fail(RP_ERR_INVALID, "%s: iterations %u outside 1 .. %u", who, args->iterations, RP_MCCFR_SUBGAME_MAX_ITERATIONS);
    if (!(args->prior > 0.0f) || args->prior > RP_F32_MAX) return rp::fail(RP_ERR_INVALID, "%s: prior must be finite and positive", who);
    if (args->reserved != 0) return rp::fail(RP_ERR_INVALID, "%s: reserved must be 0", who);
    return RP_OK;
}

int msub_check_game(const char* who, const rp_mccfr* h) {
    if (h->tbl.n_players != 2) return rp::fail(RP_ERR_UNSUPPORTED, "%s: two player game expected, the table has %u", who, h->tbl.n_players);
    return RP_OK;
}

// every launch of one call, queued on the handle's stream; every array in device memory.  FR: the depth-limited call's instantiation
// over the handle's frontier tables (`origin` in device memory or nullptr)
template <bool FR>
int msub_launch_solve(const char* who, rp_mccfr* h, uint64_t n, const rp_mccfr_subgame_entry* entries, const uint8_t* origin,
                      const rp_mccfr_subgame_args* a, rp_mccfr_subgame_result* results, rp_mccfr_subgame_row* rows) {
    const uint32_t NI = h->tbl.n_infos, A = h->tbl.max_actions;
    if (NI > RP_MCCFR_SUBGAME_MAX_INFOS)
        return rp::fail(RP_ERR_CAPACITY, "%s: %u infosets, the local profile's index holds %u", who, NI, RP_MCCFR_SUBGAME_MAX_INFOS);
    uint32_t segment = 0;
    int rc = msub_segment(&segment);
    if (rc) return rc;
    // a world's keys and a local row's slots: with frontiers the Pick infosets follow the infosets and a Pick row has D slots
    const uint32_t NK = FR ? NI + h->fr.n_pick : NI, RA = FR ? std::max(A, h->fr.D) : A;
    MsRegion R{};
    R.rows_alloc = std::min<uint32_t>(RP_MCCFR_SUBGAME_MAX_ROWS, 4 * NK);
    R.off_index = (uint32_t)sizeof(MsHead);
    R.off_keys = (uint32_t)align16(R.off_index + 2 * (size_t)4 * NK);
    R.off_perm = (uint32_t)align16(R.off_keys + 4 * (size_t)R.rows_alloc);
    R.off_rows = (uint32_t)align16(R.off_perm + 2 * (size_t)R.rows_alloc);
    R.stride = align16(R.off_rows + (size_t)R.rows_alloc * RA * sizeof(rp_encounter));
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(n, MS_MAX_CHUNK);
    const size_t need = R.stride * chunk;
    if (need > h->msub_bytes) {
        if (h->d_msub) HIP_TRY(hipFree(h->d_msub));  // waits for the launches that still use it
        h->d_msub = nullptr;
        h->msub_bytes = 0;
        if (hipMalloc(&h->d_msub, need) != hipSuccess) {
            (void)hipGetLastError();
            return rp::fail(RP_ERR_CAPACITY, "%s: %zu bytes of local profiles for %u solves do not fit", who, need, chunk);
        }
        h->msub_bytes = need;
    }
    R.base = reinterpret_cast<uint8_t*>(h->d_msub);
    MsParamsOf<FR> p{};
    p.rows_cap = a->rows_cap;
    p.n_states = h->tbl.n_states;
    p.n_terminals = h->tbl.n_terminals;
    p.seed = a->seed;
    p.iterations = a->iterations;
    p.prior = a->prior;
    p.hp = DistParams{h->hp.temperature, h->hp.smoothing, h->hp.curiosity};
    if constexpr (FR) p.fr = h->fr;
    h->clk.begin(h->stream, CK_SUBGAME);
    rc = rp::chunks(n, chunk, [&](uint64_t at, uint32_t m) {
        p.n = m;
        p.entries = entries + at;
        p.results = results + at;
        p.rows = rp::from(rows, at * a->rows_cap);
        p.first_id = a->first_id + at;
        if constexpr (FR) p.origin = rp::from(origin, at);
        for (uint32_t t = 0; t < a->iterations; t += segment) {
            p.t_begin = t;
            p.t_end = (uint32_t)std::min<uint64_t>((uint64_t)t + segment, a->iterations);
            hipLaunchKernelGGL(k_mccfr_subgame_solve<FR>, dim3(p.n), dim3(MS_LANES), 0, h->stream, h->g, h->t, R, p);
        }
    });
    h->clk.end(h->stream, CK_SUBGAME);
    return rc;
}

// the ONE check of a solve pair, in the header's order: the args, n == 0 (RP_OK is the call's answer), then the handle and the arrays
int msub_check_solve(const char* who, const rp_mccfr* h, uint64_t n, const void* entries, const void* results, const void* rows,
                     const rp_mccfr_subgame_args* args, bool frontiers) {
    int rc = msub_check_args(who, args);
    if (rc || n == 0) return rc;
    if (!h) return rp::fail(RP_ERR_INVALID, "%s: h is NULL", who);
    if (!entries || !results) return rp::fail(RP_ERR_INVALID, "%s: entries or results is NULL", who);
    if (!rows && args->rows_cap > 0) return rp::fail(RP_ERR_INVALID, "%s: rows is NULL with rows_cap > 0", who);
    if ((rc = msub_check_game(who, h))) return rc;
    if (frontiers && !h->fr.depth) return rp::fail(RP_ERR_INVALID, "%s: the handle has no frontier tables (rp_mccfr_set_frontiers)", who);
    return RP_OK;
}

// the ONE check of the belief pair
int msub_check_belief(const rp_mccfr* h, uint64_t n, const void* priors, const void* world_of, const void* weights) {
    if (n == 0) return RP_OK;
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_mccfr_subgame_belief: h is NULL");
    if (!priors || !world_of || !weights) return rp::fail(RP_ERR_INVALID, "rp_mccfr_subgame_belief: priors, world_of or weights is NULL");
    if (n > 0x7fffffffull) return rp::fail(RP_ERR_INVALID, "rp_mccfr_subgame_belief: n is larger than 2^31 - 1");
    return msub_check_game("rp_mccfr_subgame_belief", h);
}

template <bool FR>
int msub_solve_device(const char* who, rp_mccfr* h, uint64_t n, const rp_mccfr_subgame_entry* entries_dev, const uint8_t* origin_dev,
                      const rp_mccfr_subgame_args* args, rp_mccfr_subgame_result* results_dev, rp_mccfr_subgame_row* rows_dev) {
    int rc = msub_check_solve(who, h, n, entries_dev, results_dev, rows_dev, args, FR);
    if (rc || n == 0) return rc;
    if ((rc = set_device(h))) return rc;
    return msub_launch_solve<FR>(who, h, n, entries_dev, origin_dev, args, results_dev, rows_dev);
}

// the host form of both solves; origin is a host array or nullptr.  The clocks are drained on every way out past the check
template <bool FR>
int msub_solve_host(const char* who, rp_mccfr* h, uint64_t n, const rp_mccfr_subgame_entry* entries, const uint8_t* origin,
                    const rp_mccfr_subgame_args* args, rp_mccfr_subgame_result* results, rp_mccfr_subgame_row* rows) {
    int rc = msub_check_solve(who, h, n, entries, results, rows, args, FR);
    if (rc || n == 0) return rc;
    Stage s(h->device, h->stream);
    s.in(entries, n).in(origin, n).out(results, n).out(rows, n * (size_t)args->rows_cap);
    if (!(rc = s.up()) && !(rc = msub_solve_device<FR>(who, h, n, entries, origin, args, results, rows))) rc = s.down();
    h->clk.drain();
    return rc;
}

}  // namespace

extern "C" {

void rp_mccfr_subgame_args_default(rp_mccfr_subgame_args* out) {
    if (!out) return;
    *out = rp_mccfr_subgame_args{};
    out->iterations = 1;
    out->prior = 16384.0f;
}

int rp_mccfr_subgame_belief_device(rp_mccfr* h, uint64_t n, const rp_mccfr_subgame_prior* priors_dev, uint8_t* world_of_dev, float* weights_dev,
                                   uint8_t* status_dev) {
    int rc = msub_check_belief(h, n, priors_dev, world_of_dev, weights_dev);
    if (rc || n == 0) return rc;
    if ((rc = set_device(h))) return rc;
    hipLaunchKernelGGL(k_mccfr_subgame_belief, dim3((uint32_t)n), dim3(MS_LANES), 0, h->stream, h->g, h->t, h->tbl.n_states, (uint32_t)n, priors_dev,
                       world_of_dev, weights_dev, status_dev);
    HIP_TRY(hipGetLastError());
    return RP_OK;
}

int rp_mccfr_subgame_belief(rp_mccfr* h, uint64_t n, const rp_mccfr_subgame_prior* priors, uint8_t* world_of, float* weights, uint8_t* status) {
    int rc = msub_check_belief(h, n, priors, world_of, weights);
    if (rc || n == 0) return rc;
    Stage s(h->device, h->stream);
    s.in(priors, n).out(world_of, n * 16).out(weights, n * 4).out(status, n);  // world_of[n][16], weights[n][4]
    if ((rc = s.up()) || (rc = rp_mccfr_subgame_belief_device(h, n, priors, world_of, weights, status))) return rc;
    return s.down();
}

int rp_mccfr_subgame_solve_device(rp_mccfr* h, uint64_t n, const rp_mccfr_subgame_entry* entries_dev, const rp_mccfr_subgame_args* args,
                                  rp_mccfr_subgame_result* results_dev, rp_mccfr_subgame_row* rows_dev) {
    return msub_solve_device<false>("rp_mccfr_subgame_solve", h, n, entries_dev, nullptr, args, results_dev, rows_dev);
}

int rp_mccfr_subgame_solve(rp_mccfr* h, uint64_t n, const rp_mccfr_subgame_entry* entries, const rp_mccfr_subgame_args* args,
                           rp_mccfr_subgame_result* results, rp_mccfr_subgame_row* rows) {
    return msub_solve_host<false>("rp_mccfr_subgame_solve", h, n, entries, nullptr, args, results, rows);
}

int rp_mccfr_depth_solve_device(rp_mccfr* h, uint64_t n, const rp_mccfr_subgame_entry* entries_dev, const uint8_t* origin_dev,
                                const rp_mccfr_subgame_args* args, rp_mccfr_subgame_result* results_dev, rp_mccfr_subgame_row* rows_dev) {
    return msub_solve_device<true>("rp_mccfr_depth_solve", h, n, entries_dev, origin_dev, args, results_dev, rows_dev);
}

int rp_mccfr_depth_solve(rp_mccfr* h, uint64_t n, const rp_mccfr_subgame_entry* entries, const uint8_t* origin, const rp_mccfr_subgame_args* args,
                         rp_mccfr_subgame_result* results, rp_mccfr_subgame_row* rows) {
    return msub_solve_host<true>("rp_mccfr_depth_solve", h, n, entries, origin, args, results, rows);
}

// the frontier tables: the struct's own fields (no handle needed), the handle, then every chance state against the game table — all
// on the host, before the device is touched
int rp_mccfr_set_frontiers(rp_mccfr* h, const rp_mccfr_frontiers* f) {
    const char* who = "rp_mccfr_set_frontiers";
    if (f) {
        if (f->leaves < 1 || f->leaves > 4) return rp::fail(RP_ERR_INVALID, "%s: leaves %u outside 1 .. 4", who, f->leaves);
        if (f->reserved != 0) return rp::fail(RP_ERR_INVALID, "%s: reserved must be 0", who);
        if (!f->depth) return rp::fail(RP_ERR_INVALID, "%s: depth is NULL", who);
        if (!f->pick_info) return rp::fail(RP_ERR_INVALID, "%s: pick_info is NULL", who);
        if (!f->payoff_ref) return rp::fail(RP_ERR_INVALID, "%s: payoff_ref is NULL", who);
        if (f->n_matrices > 0 && !f->matrices) return rp::fail(RP_ERR_INVALID, "%s: matrices is NULL with n_matrices > 0", who);
        if (f->n_pick > RP_MCCFR_SUBGAME_MAX_INFOS)
            return rp::fail(RP_ERR_INVALID, "%s: n_pick %u above %u", who, f->n_pick, RP_MCCFR_SUBGAME_MAX_INFOS);
        if (f->n_matrices >= 0x7fffffffu) return rp::fail(RP_ERR_INVALID, "%s: n_matrices %u cannot be named by a payoff_ref", who, f->n_matrices);
        const size_t cells = (size_t)f->n_matrices * f->leaves * f->leaves;
        for (size_t i = 0; i < cells; ++i)
            if (!(f->matrices[i] >= -RP_F32_MAX && f->matrices[i] <= RP_F32_MAX))
                return rp::fail(RP_ERR_INVALID, "%s: matrices[%zu][%zu][%zu] is not finite", who, i / (f->leaves * f->leaves),
                                i / f->leaves % f->leaves, i % f->leaves);
    }
    if (!h) return rp::fail(RP_ERR_INVALID, "%s: h is NULL", who);
    const uint32_t NS = h->tbl.n_states;
    if (f)
        for (uint32_t s = 0; s < NS; ++s) {
            if (h->states[s].turn != RP_TURN_CHANCE) continue;
            if (f->depth[s] > 0 && f->pick_info[s] >= f->n_pick)
                return rp::fail(RP_ERR_INVALID, "%s: pick_info[%u] = %u of a chance state with depth %u is not below n_pick %u", who, s,
                                f->pick_info[s], (unsigned)f->depth[s], f->n_pick);
            const uint32_t ref = f->payoff_ref[s];
            const bool named = ref == RP_NO_INFO || ((ref & 0x80000000u) ? (ref & 0x7fffffffu) < f->n_matrices : ref < h->tbl.n_infos);
            if (!named)
                return rp::fail(RP_ERR_INVALID, "%s: payoff_ref[%u] = 0x%08x is neither RP_NO_INFO, an infoset nor a matrix below n_matrices %u", who,
                                s, ref, f->n_matrices);
        }
    int rc = set_device(h);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));  // no solve still reads the tables this call replaces
    if (h->d_front) HIP_TRY(hipFree(h->d_front));
    h->d_front = nullptr;
    h->fr = MsFrontiers{};
    if (!f) return RP_OK;
    const size_t b_ref = (size_t)NS * 4, b_mat = align16((size_t)f->n_matrices * f->leaves * f->leaves * 4), b_dep = align16(NS);
    const size_t off_ref = align16(b_ref), off_mat = off_ref + align16(b_ref), off_dep = off_mat + b_mat;
    uint8_t* d = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d), off_dep + b_dep + 16));
    h->d_front = d;
    HIP_TRY(hipMemcpy(d, f->pick_info, b_ref, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d + off_ref, f->payoff_ref, b_ref, hipMemcpyHostToDevice));
    if (f->n_matrices) HIP_TRY(hipMemcpy(d + off_mat, f->matrices, (size_t)f->n_matrices * f->leaves * f->leaves * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d + off_dep, f->depth, NS, hipMemcpyHostToDevice));
    h->fr.pick_info = reinterpret_cast<const uint32_t*>(d);
    h->fr.payoff_ref = reinterpret_cast<const uint32_t*>(d + off_ref);
    h->fr.matrices = reinterpret_cast<const float*>(d + off_mat);
    h->fr.depth = d + off_dep;
    h->fr.n_pick = f->n_pick;
    h->fr.n_matrices = f->n_matrices;
    h->fr.D = f->leaves;
    return RP_OK;
}

}  // extern "C"
