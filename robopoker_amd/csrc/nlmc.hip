// nlmc.hip — external-sampling MCCFR over no-limit hold'em on the device: the producer of the blueprint trainer's
// Decisions (BASELINE configs[3]).  rp_nlhe_*.
//
// Reference path: mccfr!(Nlhe, NlheEncoder, NlheTurn, NlheEdge, NlheGame, NlheInfo, 128) (crates/nlhe/src/solver.rs:11) =
//   Solver::step (mccfr/src/solver/solver.rs:96-105): batch() -> per tree TreeBuilder (builder.rs:74-161) over NlheGame
//   (nlhe/src/game.rs:33-65) with NlheEncoder::info (encoder.rs:30-68, info.rs:145-160: key = (subgame Path, bucket,
//   choices Path)), ExternalSampling (sample/external.rs:17-64), CfrFlow::dfs per walker infoset (strategy/flow.rs:64-216);
//   then the sequential update (solver.rs:143-192) = rp_profile_apply on the row-addressed table (sparse.hip).
// Oracle: oracle/rp_oracle_nlmc.c (same RNG contract: rp_node_hash of (seed, epoch, tree, key)).
//
// MAPPING (first device version: correctness and the data path).  One LANE per sampled tree — the trees of a
// batch are independent and 10^2-10^3 nodes each; a lane runs the reference's pop-last DFS with its stack and node list in
// its own HBM scratch region.  Node order = the reference's creation order, which makes the bottom-up evaluation a single
// descending sweep (every node's index exceeds its parent's; descending index adds a node's children in choices() order)
// and Tree::partition's "first node of an infoset, span in ascending index" a single ascending sweep.
//   per node:  turn -> choices (nl_choices) -> NlheInfo key -> row (open addressing in HBM: keys beside the rows, a new
//              infoset's row starts at the edge-wise default regrets, kicker/src/edge.rs:61-72) -> regret matching / sampling
//              distribution from the row -> children (walker: all, opponent: one, chance: one Draw with hashed cards)
//   per tree:  D(node) = sum_children f(edge) D(child) with f = sigma (walker), sigma / q (opponent), 1 (chance), leaves =
//              payoff(walker); reach(node) = prod of sigma / q over opponent ancestors; per walker node cfv_a = reach * D(child_a),
//              ev = sum sigma_a cfv_a; regret_a += cfv_a - ev and payoff += ev summed over the nodes that share an infoset.
// Integer state (tree shapes, keys, rows' identities, expanded masks, counters) is the oracle's bit for bit; D is the
// factorised form of recursed_value (flow.rs:182-216 multiplies the reach products at the leaves), so regret vectors agree to
// f32 re-association (tests state the tolerance), like the composed update.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "nlmc_frontier.hpp"
#include "nlmc_depth.hpp"
#include "nlmc_level.hpp"
#include "nlmc_query.hpp"
#include "nlmc_range.hpp"
#include "nlmc_world.hpp"
#include "nlmc_subgame.hpp"
#include "nlmc_aivat.hpp"
#include "nlmc_match.hpp"
#include "nlmc_translate.hpp"
#include "nlmc_search.hpp"
#include "nlmc_census.hpp"
#include "nlmc_table.hpp"
#include "../../include/rp_libm_glibc.h"
#include "host_util.hpp"
#include "sortscan.hpp"

namespace rp {

// ---- the multi-GPU exchange by infoset key (every rank's table assigns rows in its own insertion order) ----
// entries: rp_profile_summarize's records, [row u32][count u32][psum f32][n_actions u32][maps]; keys beside them
__global__ __launch_bounds__(256) void k_nlhe_entry_keys(NlTable t, const unsigned char* entries, uint32_t eb, uint32_t n, uint64_t* past,
                                                         uint32_t* present, uint64_t* choices) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t row = *reinterpret_cast<const uint32_t*>(entries + (size_t)i * eb);
    past[i] = t.slots[row].past;
    present[i] = t.slots[row].present;
    choices[i] = t.slots[row].choices;
}
__global__ __launch_bounds__(256) void k_nlhe_entry_remap(NlTable t, unsigned char* entries, uint32_t eb, uint32_t n, const uint64_t* past,
                                                          const uint32_t* present, const uint64_t* choices, uint32_t tag, uint32_t* errflags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t nch = 0, err = 0;
    for (uint64_t c = choices[i]; nch < 12u && (c & 0x1full) != 0; c >>= 5) nch += 1;
    const uint32_t row = nl_row_of(t, past[i], choices[i], present[i], nl_key_hash(past[i], choices[i], present[i]), nch, tag, &err);
    *reinterpret_cast<uint32_t*>(entries + (size_t)i * eb) = row;
    if (err) atomicOr(errflags, err);
}

}  // namespace rp

using namespace rp;

namespace {
// sweeps: up + down; decide: scan + fill + group + emit
const char* const CLOCK_NAMES[] = {"expand", "children", "sweeps", "decide", "apply"};
enum { CK_EXPAND, CK_CHILDREN, CK_SWEEPS, CK_DECIDE, CK_APPLY, CK_COUNT };
}  // namespace

struct rp_nlhe {
    int device = 0;
    rp_profile* prof = nullptr;
    uint32_t cap_log2 = 0, batch = 128;
    rp_hyper hp{};
    uint64_t seed = 0;
    NlTable tab{};
    NlParams prm{};
    NlNodes lv{};                // level-synchronous traversal
    NlBatch out{};
    uint32_t out_cap = 0;
    uint32_t* d_offset = nullptr;
    uint32_t* d_total = nullptr;   // [0] Decisions of the batch, [1] walker nodes of the batch
    void* d_scan = nullptr;                    // scratch of the per-tree scans
    void *x_keys = nullptr, *x_counts = nullptr, *x_all = nullptr, *x_packed = nullptr;  // rp_nlhe_step_comm: grow-only exchange buffers
    size_t x_keys_bytes = 0, x_counts_bytes = 0, x_all_bytes = 0, x_packed_bytes = 0;
    uint32_t* d_remap_err = nullptr;           // rp_nlhe_step_apply: table full while inserting exchanged keys
    std::vector<void*> allocs;
    uint32_t last_n = 0;
    uint32_t tag = 0;              // launch tags handed to nl_row_of (never 0)
    uint64_t nodes = 0, infos = 0;  // Metrics (mccfr/src/metrics/mod.rs): nodes grown, Decisions recorded
    uint32_t last_levels = 0, last_nodes = 0;
    // profiling (rp_nlhe_profile): HIP event pairs around the launches of each kernel group, on the launch stream
    KernelClocks clk{CLOCK_NAMES, CK_COUNT};
    uint64_t census[5] = {0, 0, 0, 0, 0};  // nodes by kind + walker children, summed over the profiled steps
    // small batches (the reference's 128): one tree per workgroup, the whole traversal in one launch (k_nl_tree); tree_cap = nodes of a
    // tree's region (0: the node arrays were not sized for it), level_ncap = the batch-wide path's own node budget (its launch sizes)
    uint32_t tree_cap = 0, level_ncap = 0;
    NlPost* post = nullptr;      // pinned, mapped host memory (k_nl_finish)
    NlPost* post_dev = nullptr;  // the same words as the device addresses them
    uint32_t post_seq = 0;
    bool ctl_clean = false;      // the control block is zero (k_nl_finish cleared it; the batch-wide path leaves it dirty)
    uint32_t tree_bt = 512;  // k_nl_tree's workgroup (RP_NL_TREE_BT = 256 / 1024: the experiment; measured round 6: 256 / 512 / 1024 = 0.483 / 0.428 / 0.443 ms per step)
    bool tree_mode_off = false;  // a tree outgrew its region once: the handle stays on the batch-wide path
    uint32_t* ex_k_parked = nullptr;  // rp_nlhe_set_exact(h, 0) on a large-batch handle: lv.ex_k while the exact evaluation is off
    uint32_t chunks = 1;  // passes per batch (RP_NLHE_CHUNKS; doubled when a pass runs out of nodes)
    void* depth_rows = nullptr;  // rp_nlhe_depth_solve: the overflow rows of a launch's solves (grow-only)
    size_t depth_rows_bytes = 0;
    void* subgame_rows = nullptr;  // rp_nlhe_subgame_solve: likewise, its own region
    size_t subgame_rows_bytes = 0;
    void* search_scratch = nullptr;  // rp_nlhe_search_match: the hands in flight, the request lists and the solves' answers (grow-only)
    size_t search_scratch_bytes = 0;
    NsmPost* search_post = nullptr;      // pinned, mapped host memory: the round's counts of solves (k_nl_search_compact)
    NsmPost* search_post_dev = nullptr;  // the same words as the device addresses them
    void* census_scratch = nullptr;  // rp_nlhe_table_census: one partial per segment of the table (grow-only)
    size_t census_scratch_bytes = 0;
    uint32_t grid_cap = 16384;  // workgroups of the grid-stride kernels (measured: 1024 -14 %, 4096 -4 %)
    // the table itself (nlmc_table.hpp).  keys: *tab.n_keys as the host last saw it — with the counts a traversal brings to the host
    // anyway, after an import, after a resize; keys_valid is false behind anything that may have inserted without telling (a failed
    // step, rp_nlhe_step_apply), and the next reader then asks the device once.
    uint64_t keys = 0;
    bool keys_valid = true;
    uint32_t grow_max = 0;       // rp_nlhe_set_growth: 0 = off
    uint64_t grow_headroom = 0;  // 0 = the default, nl_default_headroom
    void* table_scratch = nullptr;  // segment counts and offsets of an export, the rows of an import chunk, their flag words (grow-only)
    size_t table_scratch_bytes = 0;
};

namespace {
template <typename T>
int nl_alloc(rp_nlhe* h, T** out, size_t count) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)));
    HIP_TRY(hipMemset(p, 0, std::max<size_t>(count, 1) * sizeof(T)));
    h->allocs.push_back(p);
    *out = reinterpret_cast<T*>(p);
    return RP_OK;
}
// the arrays of the evaluation in the reference's own order (nlmc_level.hpp nl_ex_*): per node sigma and q of its edge, a 64-byte row of
// chains for each of rel / smp / value, per walker slot its nine action values.  192 B per node on top of the 92.
int nl_alloc_exact(rp_nlhe* h) {
    NlNodes& lv = h->lv;
    if (lv.ex_k) return RP_OK;
    const size_t N = lv.ncap;
    int rc;
    if ((rc = nl_alloc(h, &lv.fsig, N)) || (rc = nl_alloc(h, &lv.fq, N)) || (rc = nl_alloc(h, &lv.ex_r, N * NL_EX_K)) ||
        (rc = nl_alloc(h, &lv.ex_s, N * NL_EX_K)) || (rc = nl_alloc(h, &lv.ex_v, N * NL_EX_K)) ||
        (rc = nl_alloc(h, &lv.wval, (size_t)lv.lcap * NLMC_A)))
        return rc;
    return nl_alloc(h, &lv.ex_k, N);  // last: the kernels take a non-NULL ex_k as "all of them are there"
}
uint32_t nl_next_tag(rp_nlhe* h) {
    h->tag += 1;
    if (h->tag == 0) h->tag = 1;
    return h->tag;
}
int nl_capacity_error(unsigned long long flags) {
    return rp::fail(RP_ERR_CAPACITY, "rp_nlhe: traversal failed (flags %llu: 1 node budget, 2 stack, 4 walker nodes of a tree, 8 decisions, "
                                     "16 illegal action, 32 infoset table full, 64 isomorphism not found in the encoder table, 128 tree deeper "
                                     "than the level table, 256 work list full, 512 more than 16 walker decisions on one path with the exact evaluation on)", flags);
}
void nl_begin_step(rp_nlhe* h) {
    h->prm.epoch = rp::profile_epoch(h->prof);
    h->prm.walker = (uint32_t)(h->prm.epoch % 2u);  // CfrSampling::walker (book.rs:142-144)
    h->prm.step_hash = rp_node_hash_step(h->prm.seed, h->prm.epoch);
    if (h->prm.ref_rng) {  // DefaultHasher::new(); self.t().hash(hasher)  (flow.rs:289-291)
        rp_sip s;
        rp_defaulthasher_new(&s);
        rp_defaulthasher_write_u64(&s, h->prm.epoch);
        h->prm.ref_v[0] = s.v0; h->prm.ref_v[1] = s.v1; h->prm.ref_v[2] = s.v2; h->prm.ref_v[3] = s.v3;
    }
}

// waits for k_nl_finish's post of this step (h->post_seq).  Looks at the stream now and then: a failed launch never posts.
int nl_wait_post(rp_nlhe* h, hipStream_t st) {
    const volatile uint32_t* seq = &h->post->seq;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t spins = 1;; ++spins) {
        if (__atomic_load_n(seq, __ATOMIC_ACQUIRE) == h->post_seq) return RP_OK;
        if ((spins & 0x3fffu) == 0) {
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess) {  // everything launched has run: the word is there, or the kernel did not run
                if (__atomic_load_n(seq, __ATOMIC_ACQUIRE) == h->post_seq) return RP_OK;
                return rp::fail(RP_ERR_HIP, "rp_nlhe: the traversal finished without posting its counts");
            }
            if (q != hipErrorNotReady) return rp::fail(RP_ERR_HIP, "rp_nlhe: %s while waiting for the traversal", hipGetErrorString(q));
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 30.0)
                return rp::fail(RP_ERR_HIP, "rp_nlhe: no post from the traversal after 30 s");
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
}

// ---- the level-synchronous traversal (nlmc_level.hpp)
// the trees [lo, lo + B) of the batch, grown and evaluated together; their Decisions go behind the `d_base` already emitted.
// *flags: the traversal's error flags when the return code is RP_ERR_CAPACITY (the caller retries a spent node budget in chunks)
int nl_traverse_chunk(rp_nlhe* h, uint32_t lo, uint32_t B, uint32_t d_base, uint32_t* n_dec, uint32_t* n_nod, uint32_t* n_lev, uint32_t* flags) {
    hipStream_t st = rp::profile_stream(h->prof);
    h->keys_valid = false;  // until this pass has brought the table's key count to the host with its own counts
    NlNodes& lv = h->lv;
    NlParams prm = h->prm;
    prm.batch = B;
    prm.tree_base = h->prm.tree_base + lo;
    *flags = 0;
    const dim3 wide(std::min<uint32_t>(h->grid_cap, std::max<uint32_t>(1u, (h->level_ncap / 4u + 255u) / 256u))), blk(256);
    const dim3 wide_x(std::min<uint32_t>(h->grid_cap * 2u, std::max<uint32_t>(1u, (h->level_ncap / 4u + NL_TILE - 1u) / NL_TILE)));  // one tile per workgroup
    if (h->tree_cap && !h->tree_mode_off && lo == 0 && B == h->batch) {
        // ---- a small batch: one tree per workgroup, one launch (k_nl_tree), then the partition and the Decisions as below
        const uint32_t WC = NL_WMAX;
        if (!h->ctl_clean) HIP_TRY(hipMemsetAsync(lv.ctl, 0, sizeof(NlCtl), st));
        h->ctl_clean = false;
        prm.tag = nl_next_tag(h);
        h->clk.begin(st, CK_EXPAND);
        // the workgroup that finishes last scans the trees' Decisions counts and posts the batch's total and control block to the host
        // through pinned memory: the host spins on the sequence word (a scan launch + two copies + hipStreamSynchronize until round 6:
        // three launches and an interrupt round trip per step)
        h->post_seq += 1;
        if (h->post_seq == 0) h->post_seq = 1;
        if (h->tree_bt == 256u) hipLaunchKernelGGL(k_nl_tree<256>, dim3(B), blk, 0, st, prm, h->tab, lv, h->tree_cap, WC, h->d_total, h->post_dev, h->post_seq);
        else if (h->tree_bt == 1024u) hipLaunchKernelGGL(k_nl_tree<1024>, dim3(B), dim3(1024), 0, st, prm, h->tab, lv, h->tree_cap, WC, h->d_total, h->post_dev, h->post_seq);
        else hipLaunchKernelGGL(k_nl_tree<512>, dim3(B), dim3(512), 0, st, prm, h->tab, lv, h->tree_cap, WC, h->d_total, h->post_dev, h->post_seq);
        h->clk.end(st, CK_EXPAND);
        h->clk.begin(st, CK_DECIDE);
        // the Decisions are emitted behind the traversal without waiting for the host (nothing of the launch depends on the counts; a
        // tree that failed has no Decisions, and the host discards the buffer of a failed step): the post's way to the host and the
        // update's launches hide behind this kernel
        hipLaunchKernelGGL(k_nl_emit, dim3(B), blk, 0, st, lv, h->tab, B * WC, d_base, lo, h->out_cap, h->out, WC, (const float*)lv.wval);
        HIP_TRY(hipGetLastError());
        {
            int rcw = nl_wait_post(h, st);
            if (rcw) return rcw;
        }
        h->ctl_clean = true;
        const uint32_t total0 = h->post->total;
        NlCtl ctl{};
        ctl.err = h->post->err;
        ctl.n_nodes = h->post->n_nodes;
        ctl.pad[0] = h->post->levels;
        for (int k = 0; k < 4; ++k) ctl.kinds[k] = h->post->kinds[k];
        ctl.walker_kids = h->post->walker_kids;
        if (ctl.err & (NERR_NODES | NERR_WALKERS)) {
            h->tree_mode_off = true;  // a tree outgrew its region: this step and the following ones on the batch-wide path
            h->clk.end(st, CK_DECIDE);
        } else {
            if (ctl.err) {
                *flags = ctl.err;
                return nl_capacity_error(ctl.err);
            }
            if (h->clk.on) {
                for (int k = 0; k < 4; ++k) h->census[k] += ctl.kinds[k];
                h->census[4] += ctl.walker_kids;
            }
            if ((uint64_t)d_base + total0 > h->out_cap)
                return rp::fail(RP_ERR_CAPACITY, "rp_nlhe: %llu Decisions in one batch exceed the buffer (%u)", (unsigned long long)d_base + total0, h->out_cap);
            h->clk.end(st, CK_DECIDE);
            HIP_TRY(hipGetLastError());
            h->keys = h->post->keys;
            h->keys_valid = true;
            *n_dec = total0;
            *n_nod = ctl.n_nodes;
            *n_lev = ctl.pad[0];
            return RP_OK;
        }
    }
    h->ctl_clean = false;
    HIP_TRY(hipMemsetAsync(lv.ctl, 0, sizeof(NlCtl), st));
    HIP_TRY(hipMemsetAsync(lv.t_nw, 0, (size_t)B * 4, st));
    prm.tag = nl_next_tag(h);
    hipLaunchKernelGGL(k_nl_roots, dim3((B + 255u) / 256u), blk, 0, st, prm, lv);
    NlCtl ctl;
    uint32_t L = 0;
    for (;;) {  // grow all trees one level per pair of launches; look at the frontier every few levels
        const uint32_t stop = std::min<uint32_t>(NL_MAXL - 1u, L + (L == 0 ? 22u : 6u));
        for (; L < stop; ++L) {
            prm.tag = nl_next_tag(h);
            h->clk.begin(st, CK_EXPAND);
            hipLaunchKernelGGL((k_nl_expand<4, 256>), wide_x, blk, 0, st, prm, h->tab, lv, L);
            h->clk.end(st, CK_EXPAND);
            h->clk.begin(st, CK_CHILDREN);
            hipLaunchKernelGGL(k_nl_children, wide, blk, 0, st, prm, lv, L);
            h->clk.end(st, CK_CHILDREN);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&ctl, lv.ctl, sizeof(NlCtl), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (ctl.err) {
            *flags = ctl.err;
            return nl_capacity_error(ctl.err);
        }
        // level L = the children the last launch pair created; an empty level ends every tree
        const bool alive = ctl.lvl_node[L + 1] > ctl.lvl_node[L];
        if (!alive) break;
        if (L >= NL_MAXL - 1u) return nl_capacity_error(NERR_LEVELS);
    }
    uint32_t levels = 0;
    while (levels < NL_MAXL && ctl.lvl_node[levels + 1] > ctl.lvl_node[levels]) levels += 1;
    const uint32_t n_nodes = ctl.lvl_node[levels];
    h->clk.begin(st, CK_SWEEPS);
    for (uint32_t l = levels; l-- > 0;) hipLaunchKernelGGL(k_nl_up, wide, blk, 0, st, lv, l);
    for (uint32_t l = 0; l + 1 < levels; ++l) hipLaunchKernelGGL(k_nl_down, wide, blk, 0, st, lv, l);
    h->clk.end(st, CK_SWEEPS);
    h->clk.begin(st, CK_DECIDE);
    HIP_TRY(rp::ss::exclusive_scan<uint32_t>(lv.t_nw, lv.t_woff, B, h->d_scan, st, h->d_total + 1));
    hipLaunchKernelGGL(k_nl_fill, dim3(std::min<uint32_t>(wide.x, 2048u)), blk, 0, st, lv, n_nodes);
    hipLaunchKernelGGL((k_nl_group<256>), dim3(B), dim3(64), 0, st, lv, B);
    hipLaunchKernelGGL(k_nl_group_big, dim3(std::min<uint32_t>(B, 1280u)), dim3(64), 0, st, lv);
    HIP_TRY(rp::ss::exclusive_scan<uint32_t>(lv.t_dcount, lv.t_doff, B, h->d_scan, st, h->d_total));
    HIP_TRY(hipGetLastError());
    uint32_t total[2] = {0, 0};
    unsigned int keys_now = 0;  // no launch behind this point inserts
    HIP_TRY(hipMemcpyAsync(total, h->d_total, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&ctl, lv.ctl, sizeof(NlCtl), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&keys_now, h->tab.n_keys, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (ctl.err) {
        *flags = ctl.err;
        return nl_capacity_error(ctl.err);
    }
    if (h->clk.on) {
        for (int k = 0; k < 4; ++k) h->census[k] += ctl.kinds[k];
        h->census[4] += ctl.walker_kids;
    }
    if ((uint64_t)d_base + total[0] > h->out_cap)
        return rp::fail(RP_ERR_CAPACITY, "rp_nlhe: %llu Decisions in one batch exceed the buffer (%u)", (unsigned long long)d_base + total[0], h->out_cap);
    if (total[1] > lv.lcap) {  // as many walker nodes as this is a spent node budget too
        *flags = NERR_NODES;
        return rp::fail(RP_ERR_CAPACITY, "rp_nlhe: %u walker nodes in one pass exceed the buffer (%u)", total[1], lv.lcap);
    }
    hipLaunchKernelGGL(k_nl_emit, wide, blk, 0, st, lv, h->tab, total[1], d_base, lo, h->out_cap, h->out, 0u, (const float*)(lv.ex_k ? lv.wval : nullptr));
    h->clk.end(st, CK_DECIDE);
    HIP_TRY(hipGetLastError());
    h->keys = keys_now;
    h->keys_valid = true;
    *n_dec = total[0];
    *n_nod = n_nodes;
    *n_lev = levels;
    return RP_OK;
}
// Solver::batch for the whole batch.  The node arrays hold 1 536 nodes per tree of the batch; trees grow with training, and when a
// pass runs out of nodes the batch is traversed in twice as many passes from then on (same trees, same Decisions in the same
// order: a pass is a contiguous range of tree ids) instead of failing the step.
int nl_traverse_levels(rp_nlhe* h) {
    nl_begin_step(h);
    const uint32_t B = h->batch;
    for (;;) {
        const uint32_t K = std::min<uint32_t>(h->chunks, B);
        uint32_t dec = 0, nodes = 0, levels = 0;
        bool again = false;
        for (uint32_t c = 0; c < K; ++c) {
            const uint32_t lo = (uint32_t)((uint64_t)B * c / K), hi = (uint32_t)((uint64_t)B * (c + 1) / K);
            if (hi == lo) continue;
            uint32_t d = 0, nn = 0, nl = 0, flags = 0;
            const int rc = nl_traverse_chunk(h, lo, hi - lo, dec, &d, &nn, &nl, &flags);
            if (rc) {
                if (flags == NERR_NODES && K < B && K < 4096u) {  // only the node budget: more, smaller passes
                    h->chunks = K * 2u;
                    again = true;
                    break;
                }
                return rc;
            }
            dec += d;
            nodes += nn;
            levels = std::max(levels, nl);
        }
        if (again) continue;
        h->last_n = dec;
        h->nodes += nodes;
        h->infos += dec;
        h->last_levels = levels;
        h->last_nodes = nodes;
        return RP_OK;
    }
}
int nl_traverse(rp_nlhe* h) { return nl_traverse_levels(h); }
int nl_grow_table(rp_nlhe* h, uint64_t headroom);  // with the table's own code, behind the census
uint64_t nl_default_headroom(const rp_nlhe* h);
}  // namespace

extern "C" {

int rp_nlhe_create(int device, uint32_t cap_log2, rp_regret_kind regret, rp_weight_kind weight, const rp_hyper* hp, uint64_t seed,
                   uint32_t batch, const rp_lookup* const* tables, rp_nlhe** out) {
    if (!out || !hp || cap_log2 < 8 || cap_log2 > 30) return rp::fail(RP_ERR_INVALID, "rp_nlhe_create: bad argument");
    if (rp_device_count() <= 0) return rp::fail(RP_ERR_NO_DEVICE, "rp_nlhe_create: no HIP device visible; the MI355X path has no CPU fallback");
    if (batch == 0) batch = 128;  // nlhe/src/solver.rs:11
    rp_nlhe* h = new rp_nlhe();
    h->device = device;
    h->cap_log2 = cap_log2;
    h->batch = batch;
    h->hp = *hp;
    h->seed = seed;
    if (getenv("RP_NLHE_CHUNKS")) h->chunks = (uint32_t)std::max(1, atoi(getenv("RP_NLHE_CHUNKS")));
    if (getenv("RP_NL_TREE_BT")) h->tree_bt = (uint32_t)atoi(getenv("RP_NL_TREE_BT"));
#define NL_TRY(expr)                    \
    do {                                \
        int _rc = (expr);               \
        if (_rc) {                      \
            rp_nlhe_destroy(h);         \
            return _rc;                 \
        }                               \
    } while (0)
    if (hipSetDevice(device) != hipSuccess) {
        delete h;
        return rp::fail(RP_ERR_HIP, "rp_nlhe_create: hipSetDevice(%d) failed", device);
    }
    const uint64_t rows = 1ull << cap_log2;
    // Decisions per tree: ~40 / ~90 on average by walker, 483 the largest seen in 20 000 oracle trees; the batch buffer holds 160 per
    // tree.  Nodes per tree: 280 / 660 on average by walker on a fresh table, 3 300 the largest — and they GROW with training (the
    // opponent's average strategy calls and raises more than the warm-start bias: 760 per tree after a few steps on the trained
    // abstraction): 1 536 per tree of budget, 92 B each (the batch's total is what counts)
    // (round 5: 224 — after a few steps of external sampling in the reference's float order a 262 144-tree batch emitted 175 per tree)
    const uint64_t dec_cap64 = std::max<uint64_t>((uint64_t)batch * 224u, 4096u);
    // RP_NLHE_NODE_BUDGET = "<nodes per tree>[,<walker divisor>]" (tests of the chunked retry): the node budget per tree, and the
    // share of it the walker-node arrays hold (a quarter by default: ",16" makes a pass overflow THOSE arrays with nodes to spare)
    const char* budget_env = getenv("RP_NLHE_NODE_BUDGET");
    const uint64_t per_tree = budget_env ? (uint64_t)std::max(64, atoi(budget_env)) : 1536u;
    uint64_t walker_div = 4;
    if (budget_env && strchr(budget_env, ',')) walker_div = (uint64_t)std::min(4096, std::max(1, atoi(strchr(budget_env, ',') + 1)));
    const uint64_t ncap64 = budget_env ? (uint64_t)batch * per_tree : std::max<uint64_t>((uint64_t)batch * per_tree, 1u << 17);
    if (dec_cap64 >= (1ull << 31) || ncap64 >= (1ull << 32)) {
        delete h;
        return rp::fail(RP_ERR_INVALID, "rp_nlhe_create: batch too large (at most %u trees per step)", (uint32_t)((1ull << 32) / 1536u));
    }
    NL_TRY(rp_profile_create(device, rows, NLMC_A, regret, weight, hp, nullptr, (uint32_t)dec_cap64, &h->prof));
    NL_TRY(nl_alloc(h, &h->tab.slots, rows));
    NL_TRY(nl_alloc(h, &h->tab.n_keys, 1));
    h->tab.mask = (uint32_t)(rows - 1);
    h->tab.rows = rp::profile_table(h->prof);
    h->prm.seed = seed;
    h->prm.batch = batch;
    h->prm.temperature = hp->temperature;
    h->prm.smoothing = hp->smoothing;
    h->prm.curiosity = hp->curiosity;
    h->prm.sampling = RP_SAMPLING_EXTERNAL;  // the mccfr! macro's default scheme; rp_nlhe_set_sampling selects Flagship's
    h->prm.prune_threshold = hp->prune_threshold;
    h->prm.prune_explore = hp->prune_explore;
    h->prm.prune_warmup = hp->prune_warmup;
    h->prm.check_legal = getenv("RP_NLHE_CHECK_LEGAL") ? 1u : 0u;
    h->prm.encoder = 0;
    if (tables) {
        for (int s = 0; s < 4; ++s) {
            int street = -1;
            const uint8_t* abs_ = nullptr;
            NL_TRY(rp::lookup_view(tables[s], &h->prm.tkeys[s], &abs_, &h->prm.tn[s], &street));
            h->prm.tabs[s] = abs_;
            if (street != s) NL_TRY(rp::fail(RP_ERR_INVALID, "rp_nlhe_create: tables[%d] is a lookup of street %d", s, street));
        }
        h->prm.encoder = 1;
    }
    const size_t B = batch;
    {
        NlNodes& lv = h->lv;
        // a batch of at most NL_TREE_BATCH trees also gets a region of NL_TREE_CAP nodes and NL_WMAX walker slots per tree (k_nl_tree)
        const bool tree_mode = !budget_env && batch <= NL_TREE_BATCH;
        h->level_ncap = (uint32_t)ncap64;
        h->tree_cap = tree_mode ? NL_TREE_CAP : 0u;
        const size_t N = std::max<size_t>((size_t)ncap64, tree_mode ? (size_t)batch * NL_TREE_CAP : 0);
        const size_t LC = std::max<size_t>(std::max<size_t>((size_t)ncap64 / walker_div, 64), tree_mode ? (size_t)batch * NL_WMAX : 0);  // walker nodes of a batch (a seventh of its nodes): a quarter of the node budget
        lv.ncap = (uint32_t)N;
        lv.lcap = (uint32_t)LC;
        NL_TRY(nl_alloc(h, &lv.link, N)); NL_TRY(nl_alloc(h, &lv.tree, N)); NL_TRY(nl_alloc(h, &lv.meta, N));
        NL_TRY(nl_alloc(h, &lv.kid0, N)); NL_TRY(nl_alloc(h, &lv.row, N)); NL_TRY(nl_alloc(h, &lv.size, N));
        NL_TRY(nl_alloc(h, &lv.dfs, N)); NL_TRY(nl_alloc(h, &lv.aux, N));
        NL_TRY(nl_alloc(h, &lv.fac, N)); NL_TRY(nl_alloc(h, &lv.val, N)); NL_TRY(nl_alloc(h, &lv.reach, N));
        NL_TRY(nl_alloc(h, &lv.ga, N)); NL_TRY(nl_alloc(h, &lv.gb, N)); NL_TRY(nl_alloc(h, &lv.gc, N));
        NL_TRY(nl_alloc(h, &lv.hole0, B)); NL_TRY(nl_alloc(h, &lv.hole1, B));
        NL_TRY(nl_alloc(h, &lv.t_nw, B)); NL_TRY(nl_alloc(h, &lv.t_woff, B));
        NL_TRY(nl_alloc(h, &lv.t_dcount, B)); NL_TRY(nl_alloc(h, &lv.t_doff, B));
        NL_TRY(nl_alloc(h, &lv.wl, LC)); NL_TRY(nl_alloc(h, &lv.ws, LC)); NL_TRY(nl_alloc(h, &lv.gdesc, LC));
        NL_TRY(nl_alloc(h, &lv.big, B));
        NL_TRY(nl_alloc(h, &lv.ctl, 1));
        if (tree_mode) NL_TRY(nl_alloc_exact(h));  // a small batch is always evaluated in the reference's own order (k_nl_tree)
        if (tree_mode) {
            void* hp_ = nullptr;
            void* dp_ = nullptr;
            if (hipHostMalloc(&hp_, sizeof(NlPost), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
                hipHostGetDevicePointer(&dp_, hp_, 0) != hipSuccess) {
                if (hp_) (void)hipHostFree(hp_);
                NL_TRY(rp::fail(RP_ERR_HIP, "rp_nlhe_create: no pinned host memory for the traversal's post"));
            }
            memset(hp_, 0, sizeof(NlPost));
            h->post = reinterpret_cast<NlPost*>(hp_);
            h->post_dev = reinterpret_cast<NlPost*>(dp_);
        }
    }
    h->out_cap = (uint32_t)dec_cap64;
    NL_TRY(nl_alloc(h, &h->out.row, h->out_cap));
    NL_TRY(nl_alloc(h, &h->out.nact, h->out_cap));
    NL_TRY(nl_alloc(h, &h->out.expanded, h->out_cap));
    NL_TRY(nl_alloc(h, &h->out.regret, (size_t)h->out_cap * NLMC_A));
    NL_TRY(nl_alloc(h, &h->out.policy, (size_t)h->out_cap * NLMC_A));
    NL_TRY(nl_alloc(h, &h->out.payoff, h->out_cap));
    NL_TRY(nl_alloc(h, &h->out.tree, h->out_cap));
    NL_TRY(nl_alloc(h, &h->d_total, 2));
    NL_TRY(nl_alloc(h, &h->d_remap_err, 1));
    {
        unsigned char* scratch = nullptr;
        NL_TRY(nl_alloc(h, &scratch, rp::ss::scan_scratch_bytes(B)));
        h->d_scan = scratch;
    }
#undef NL_TRY
    // hipMemset on device memory returns before it has run, and a non-blocking stream does not wait for the null stream: the
    // first launch on this handle's stream could otherwise overtake the initialisation above and be overwritten by it
    (void)hipDeviceSynchronize();
    *out = h;
    return RP_OK;
}

// the SamplingScheme of the solver type at walker nodes: ExternalSampling (the mccfr! macro's default, nlhe/src/solver.rs:11),
// PrunableSampling, PluribusSampling (Flagship, nlhe/src/lib.rs:86-90); thresholds from the rp_hyper given at creation
int rp_nlhe_set_sampling(rp_nlhe* h, rp_sampling_kind sampling) {
    if (!h || (int)sampling < 0 || (int)sampling > (int)RP_SAMPLING_PLURIBUS) return rp::fail(RP_ERR_INVALID, "rp_nlhe_set_sampling: bad argument");
    h->prm.sampling = (int)sampling;
    return RP_OK;
}

// shape of the last traversed batch (level-synchronous traversal): levels grown and nodes
int rp_nlhe_set_rng(rp_nlhe* h, rp_rng_kind kind) {
    if (!h || (kind != RP_RNG_COUNTER && kind != RP_RNG_REFERENCE)) return rp::fail(RP_ERR_INVALID, "rp_nlhe_set_rng: bad argument");
    h->prm.ref_rng = kind == RP_RNG_REFERENCE ? 1u : 0u;
    return RP_OK;
}
int rp_nlhe_set_exact(rp_nlhe* h, int on) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_set_exact: NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(rp::profile_stream(h->prof)));
    if (!on) {
        if (h->tree_cap) return rp::fail(RP_ERR_UNSUPPORTED, "rp_nlhe_set_exact: a batch of at most %u trees is always evaluated in the reference's order", NL_TREE_BATCH);
        if (h->lv.ex_k) h->ex_k_parked = h->lv.ex_k;
        h->lv.ex_k = nullptr;  // the kernels look at ex_k only; the arrays stay with the handle
        return RP_OK;
    }
    if (!h->lv.ex_k && h->ex_k_parked) {
        h->lv.ex_k = h->ex_k_parked;
        return RP_OK;
    }
    return nl_alloc_exact(h);
}
int rp_nlhe_last_shape(rp_nlhe* h, uint32_t* levels, uint32_t* nodes) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_last_shape: NULL handle");
    if (levels) *levels = h->last_levels;
    if (nodes) *nodes = h->last_nodes;
    return RP_OK;
}

int rp_nlhe_destroy(rp_nlhe* h) {
    if (!h) return RP_OK;
    (void)hipSetDevice(h->device);
    if (h->prof) {
        (void)rp_profile_sync(h->prof);
        (void)rp_profile_destroy(h->prof);
    }
    for (void* p : h->allocs) (void)hipFree(p);
    if (h->post) (void)hipHostFree(h->post);
    if (h->search_post) (void)hipHostFree(h->search_post);
    for (void* p : {h->x_keys, h->x_counts, h->x_all, h->x_packed, h->depth_rows, h->subgame_rows, h->search_scratch, h->census_scratch, h->table_scratch})
        if (p) (void)hipFree(p);
    delete h;
    return RP_OK;
}

int rp_nlhe_step(rp_nlhe* h, rp_update_mode mode) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_step: NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    int rc = h->grow_max ? nl_grow_table(h, h->grow_headroom ? h->grow_headroom : nl_default_headroom(h)) : RP_OK;
    if (rc || (rc = nl_traverse(h))) return rc;
    rp_decisions b{h->last_n, h->out.row, h->out.nact, h->out.expanded, h->out.regret, h->out.policy, h->out.payoff};
    h->clk.begin(rp::profile_stream(h->prof), CK_APPLY);
    rc = rp_profile_apply(h->prof, &b, mode);
    h->clk.end(rp::profile_stream(h->prof), CK_APPLY);
    return rc;
}

// Trainer::train (crates/forge/src/trainer.rs:18-66) over the NLHE solver — what forge runs on the Flagship type: loop { step;
// checkpoint; flush; interrupt? } with Metrics::checkpoint's rate (mccfr/src/metrics/mod.rs:67-80), Checkpoint's display line
// (metrics/checkpoint.rs:39-50) and Progress::summary (progress.rs:24-26); the same contract as rp_mccfr_train.  The counters
// live on the host (the step synchronises once anyway), so a checkpoint costs nothing.
int rp_nlhe_train(rp_nlhe* h, rp_update_mode mode, uint64_t max_steps, double max_seconds, double log_interval, double flush_interval,
                  rp_train_event_fn on_event, void* user, const volatile int* interrupt, char* summary, size_t summary_cap) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_train: NULL handle");
    auto counts = [h](TrainCounts& c) {
        c = {rp::profile_epoch(h->prof), h->nodes, h->infos};
        return RP_OK;
    };
    auto step = [&](TrainCounts& c) {
        const int rc = rp_nlhe_step(h, mode);
        counts(c);
        return rc;
    };
    return train_loop(step, counts, max_steps, max_seconds, log_interval, flush_interval, on_event, user, interrupt, summary, summary_cap);
}

// ---- profiling hooks used by bench.py: HIP events on the launch stream around each kernel group
int rp_nlhe_profile(rp_nlhe* h, int enable) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_profile: NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(rp::profile_stream(h->prof)));
    h->clk.drain();
    h->clk.on = enable != 0;
    h->clk.reset();
    for (auto& c : h->census) c = 0;
    return RP_OK;
}
int rp_nlhe_kernel_time(rp_nlhe* h, const char* name, double* total_ms, uint64_t* launches) {
    if (!h || !name) return rp::fail(RP_ERR_INVALID, "rp_nlhe_kernel_time: NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(rp::profile_stream(h->prof)));
    return kernel_time(h->clk, "rp_nlhe_kernel_time", name, total_ms, launches);
}
// nodes of the profiled steps by kind {terminal, chance, walker, opponent} and the children of their walker nodes
int rp_nlhe_census(rp_nlhe* h, uint64_t* kinds4, uint64_t* walker_children) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_census: NULL handle");
    if (kinds4)
        for (int k = 0; k < 4; ++k) kinds4[k] = h->census[k];
    if (walker_children) *walker_children = h->census[4];
    return RP_OK;
}

int rp_nlhe_batch(rp_nlhe* h, uint32_t cap, uint32_t* n, uint32_t* tree, uint64_t* past, uint32_t* present, uint64_t* choices,
                  uint8_t* n_actions, uint16_t* expanded, float* regret, float* policy, float* payoff) {
    if (!h || !n) return rp::fail(RP_ERR_INVALID, "rp_nlhe_batch: NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = rp::profile_stream(h->prof);
    const uint64_t nodes0 = h->nodes, infos0 = h->infos;
    int rc = nl_traverse(h);
    h->nodes = nodes0;  // a debugging view: counters not advanced
    h->infos = infos0;
    if (rc) return rc;
    *n = h->last_n;
    const uint32_t m = std::min(cap, h->last_n);
    if (m == 0) return RP_OK;
    std::vector<uint32_t> rows(m);
    HIP_TRY(hipMemcpyAsync(rows.data(), h->out.row, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    if (tree) HIP_TRY(hipMemcpyAsync(tree, h->out.tree, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    if (n_actions) HIP_TRY(hipMemcpyAsync(n_actions, h->out.nact, m, hipMemcpyDeviceToHost, st));
    if (expanded) HIP_TRY(hipMemcpyAsync(expanded, h->out.expanded, (size_t)m * 2, hipMemcpyDeviceToHost, st));
    if (regret) HIP_TRY(hipMemcpyAsync(regret, h->out.regret, (size_t)m * NLMC_A * 4, hipMemcpyDeviceToHost, st));
    if (policy) HIP_TRY(hipMemcpyAsync(policy, h->out.policy, (size_t)m * NLMC_A * 4, hipMemcpyDeviceToHost, st));
    if (payoff) HIP_TRY(hipMemcpyAsync(payoff, h->out.payoff, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));  // every copy above has landed before any return below
    if (past || present || choices) {  // the infoset behind each row (rows differ between implementations; keys do not)
        const size_t rowsn = (size_t)1 << h->cap_log2;
        std::vector<NlSlot> slots(rowsn);
        HIP_TRY(hipMemcpy(slots.data(), h->tab.slots, rowsn * sizeof(NlSlot), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < m; ++i) {
            if (past) past[i] = slots[rows[i]].past;
            if (choices) choices[i] = slots[rows[i]].choices;
            if (present) present[i] = slots[rows[i]].present;
        }
    }
    return RP_OK;
}

int rp_nlhe_epoch(rp_nlhe* h, uint64_t* epoch) {
    if (!h || !epoch) return rp::fail(RP_ERR_INVALID, "rp_nlhe_epoch: NULL argument");
    *epoch = rp::profile_epoch(h->prof);
    return RP_OK;
}

int rp_nlhe_counters(rp_nlhe* h, uint64_t* nodes, uint64_t* infos, uint64_t* keys) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_counters: NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = rp::profile_stream(h->prof);
    unsigned int k = 0;
    HIP_TRY(hipMemcpyAsync(&k, h->tab.n_keys, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (nodes) *nodes = h->nodes;
    if (infos) *infos = h->infos;
    if (keys) *keys = k;
    return RP_OK;
}

// every infoset of the table with its Encounters, in slot order
int rp_nlhe_export(rp_nlhe* h, uint64_t cap, uint64_t* n, uint64_t* past, uint32_t* present, uint64_t* choices, rp_encounter* enc) {
    if (!h || !n) return rp::fail(RP_ERR_INVALID, "rp_nlhe_export: NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    int rc = rp_profile_sync(h->prof);
    if (rc) return rc;
    const size_t rowsn = (size_t)1 << h->cap_log2;
    std::vector<NlSlot> slots(rowsn);
    std::vector<uint32_t> rows;
    HIP_TRY(hipMemcpy(slots.data(), h->tab.slots, rowsn * sizeof(NlSlot), hipMemcpyDeviceToHost));
    for (size_t s = 0; s < rowsn; ++s)
        if (slots[s].state == 2u) rows.push_back((uint32_t)s);
    *n = rows.size();
    const size_t m = std::min<size_t>(cap, rows.size());
    if (m == 0 || !past || !present || !choices || !enc) return RP_OK;
    for (size_t i = 0; i < m; ++i) {
        past[i] = slots[rows[i]].past;
        choices[i] = slots[rows[i]].choices;
        present[i] = slots[rows[i]].present;
    }
    return rp_profile_get_rows(h->prof, m, rows.data(), enc);
}

// load Encounters by key (hydrate / resynchronisation): unknown keys are inserted (host-side probing, same hash)
int rp_nlhe_import(rp_nlhe* h, uint64_t n, const uint64_t* past, const uint32_t* present, const uint64_t* choices, const rp_encounter* enc,
                   uint64_t epoch) {
    if (!h || (n && (!past || !present || !choices || !enc))) return rp::fail(RP_ERR_INVALID, "rp_nlhe_import: NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    int rc = rp_profile_sync(h->prof);
    if (rc) return rc;
    const size_t rowsn = (size_t)1 << h->cap_log2;
    std::vector<NlSlot> slots(rowsn);
    std::vector<uint32_t> rows(n);
    HIP_TRY(hipMemcpy(slots.data(), h->tab.slots, rowsn * sizeof(NlSlot), hipMemcpyDeviceToHost));
    unsigned int added = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t hk = rp_mix64(rp_mix64(past[i] ^ 0x9e3779b97f4a7c15ull) ^ rp_mix64(choices[i] + 0xd1342543de82ef95ull) ^
                                     ((uint64_t)present[i] * 0xaf251af3b0f025b5ull));
        uint32_t s = (uint32_t)hk & h->tab.mask;
        for (size_t probes = 0;; ++probes) {
            if (probes > rowsn) return rp::fail(RP_ERR_CAPACITY, "rp_nlhe_import: infoset table full");
            NlSlot& sl = slots[s];
            if (sl.state != 2u) {
                sl.state = 2u;
                sl.born = 0u;
                sl.past = past[i];
                sl.choices = choices[i];
                sl.present = present[i];
                added += 1;
                break;
            }
            if (sl.past == past[i] && sl.choices == choices[i] && sl.present == present[i]) break;
            s = (s + 1u) & h->tab.mask;
        }
        rows[i] = s;
    }
    HIP_TRY(hipMemcpy(h->tab.slots, slots.data(), rowsn * sizeof(NlSlot), hipMemcpyHostToDevice));
    unsigned int k = 0;
    HIP_TRY(hipMemcpy(&k, h->tab.n_keys, 4, hipMemcpyDeviceToHost));
    k += added;
    HIP_TRY(hipMemcpy(h->tab.n_keys, &k, 4, hipMemcpyHostToDevice));
    h->keys = k;
    h->keys_valid = true;
    if ((rc = rp_profile_set_rows(h->prof, n, rows.data(), enc))) return rc;
    return rp_profile_set_epoch(h->prof, epoch);
}

int rp_nlhe_set_shard(rp_nlhe* h, uint32_t rank, uint32_t world) {
    if (!h || world == 0 || rank >= world) return rp::fail(RP_ERR_INVALID, "rp_nlhe_set_shard: bad rank/world");
    h->prm.tree_base = (uint64_t)rank * h->batch;
    return RP_OK;
}

int rp_nlhe_entry_bytes(rp_nlhe* h, size_t* bytes, uint32_t* max_entries) {
    if (!h || !bytes) return rp::fail(RP_ERR_INVALID, "rp_nlhe_entry_bytes: NULL argument");
    int rc = rp_profile_entry_bytes(h->prof, bytes);
    if (max_entries) *max_entries = h->out_cap;
    return rc;
}

int rp_nlhe_step_local(rp_nlhe* h, void* entries_dev, uint64_t* past_dev, uint32_t* present_dev, uint64_t* choices_dev, uint32_t* n_entries) {
    if (!h || !entries_dev || !past_dev || !present_dev || !choices_dev || !n_entries)
        return rp::fail(RP_ERR_INVALID, "rp_nlhe_step_local: NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    int rc = nl_traverse(h);
    if (rc) return rc;
    rp_decisions b{h->last_n, h->out.row, h->out.nact, h->out.expanded, h->out.regret, h->out.policy, h->out.payoff};
    if ((rc = rp_profile_summarize(h->prof, &b, entries_dev, n_entries))) return rc;  // synchronises: *n_entries is valid
    if (*n_entries) {
        size_t eb = 0;
        (void)rp_profile_entry_bytes(h->prof, &eb);
        hipLaunchKernelGGL(k_nlhe_entry_keys, dim3((*n_entries + 255u) / 256u), dim3(256), 0, rp::profile_stream(h->prof), h->tab,
                           reinterpret_cast<const unsigned char*>(entries_dev), (uint32_t)eb, *n_entries, past_dev, present_dev, choices_dev);
        HIP_TRY(hipGetLastError());
    }
    return RP_OK;
}

int rp_nlhe_step_apply(rp_nlhe* h, void* entries_dev, const uint64_t* past_dev, const uint32_t* present_dev, const uint64_t* choices_dev,
                       uint32_t n_entries) {
    if (!h || (n_entries && (!entries_dev || !past_dev || !present_dev || !choices_dev)))
        return rp::fail(RP_ERR_INVALID, "rp_nlhe_step_apply: NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    if (n_entries) {
        size_t eb = 0;
        (void)rp_profile_entry_bytes(h->prof, &eb);
        hipLaunchKernelGGL(k_nlhe_entry_remap, dim3((n_entries + 255u) / 256u), dim3(256), 0, rp::profile_stream(h->prof), h->tab,
                           reinterpret_cast<unsigned char*>(entries_dev), (uint32_t)eb, n_entries, past_dev, present_dev, choices_dev,
                           nl_next_tag(h), h->d_remap_err);
        HIP_TRY(hipGetLastError());
        h->keys_valid = false;
    }
    return rp_profile_fold(h->prof, entries_dev, n_entries);
}

// Solver::step across the ranks of an rp_comm (the library's own RCCL communicator; hosts without torch.distributed): step_local,
// the entry counts of all ranks (4 bytes each — ncclAllGather takes host-known sizes, so this is the one host read of a step),
// entries and keys all-gathered padded to the longest list, packed rank-major on the device, step_apply.  `steps` steps.
int rp_nlhe_step_comm(rp_nlhe* h, rp_comm* c, uint32_t steps) {
    if (!h || !c) return rp::fail(RP_ERR_INVALID, "rp_nlhe_step_comm: NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    const uint32_t world = (uint32_t)rp::comm_world(c), rank = (uint32_t)rp::comm_rank(c);
    int rc = rp_nlhe_set_shard(h, rank, world);
    if (rc) return rc;
    size_t eb = 0;
    (void)rp_profile_entry_bytes(h->prof, &eb);
    hipStream_t st = rp::profile_stream(h->prof);
    unsigned char* mine_ent = rp::profile_entries(h->prof);
    if (!mine_ent) return rp::fail(RP_ERR_INVALID, "rp_nlhe_step_comm: the profile has no summary buffer");
    auto grow = [&](void** p, size_t* have, size_t need) -> int {
        if (*have >= need) return RP_OK;
        HIP_TRY(hipStreamSynchronize(st));
        if (*p) (void)hipFree(*p);
        *p = nullptr;
        *have = 0;
        HIP_TRY(hipMalloc(p, need + need / 4));
        *have = need + need / 4;
        return RP_OK;
    };
    for (uint32_t s = 0; s < steps; ++s) {
        // A rank that fails here (a full table, the Decisions buffer, the node budget after its retries) must not leave the others
        // waiting in the gather: its failure travels in the count exchange (NL_RANK_FAILED) and every rank leaves the step with an
        // error together.
        constexpr uint32_t NL_RANK_FAILED = 0xffffffffu;
        uint32_t n_mine = 0;
        int local_rc = nl_traverse(h);
        if (!local_rc) {
            rp_decisions b{h->last_n, h->out.row, h->out.nact, h->out.expanded, h->out.regret, h->out.policy, h->out.payoff};
            local_rc = rp_profile_summarize(h->prof, &b, mine_ent, &n_mine);  // synchronises: n_mine is valid
        }
        const std::string local_msg = local_rc ? rp_last_error() : "";
        if (local_rc) n_mine = NL_RANK_FAILED;
        // every rank's count
        if ((rc = grow(&h->x_counts, &h->x_counts_bytes, (size_t)(world + 1) * 4u))) return rc;
        uint32_t* d_counts = reinterpret_cast<uint32_t*>(h->x_counts);
        HIP_TRY(hipMemcpyAsync(d_counts + world, &n_mine, 4, hipMemcpyHostToDevice, st));
        if ((rc = rp::comm_all_gather(c, d_counts + world, d_counts, 4, st))) return rc;
        std::vector<uint32_t> counts(world);
        HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, (size_t)world * 4u, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (local_rc) return rp::fail(local_rc, "%s", local_msg.c_str());
        for (uint32_t r = 0; r < world; ++r)
            if (counts[r] == NL_RANK_FAILED) return rp::fail(RP_ERR_CAPACITY, "rp_nlhe_step_comm: rank %u failed its part of the step", r);
        uint32_t width = 0, total = 0;
        for (uint32_t r = 0; r < world; ++r) width = std::max(width, counts[r]), total += counts[r];
        // keys of my entries: [past u64][choices u64][present u32] planes of `width` items (the gather sends `width` of each)
        if ((rc = grow(&h->x_keys, &h->x_keys_bytes, (size_t)std::max<uint32_t>(width, 1u) * 20u))) return rc;
        uint64_t* kp = reinterpret_cast<uint64_t*>(h->x_keys);
        uint64_t* kc = kp + width;
        uint32_t* kb = reinterpret_cast<uint32_t*>(kc + width);
        if (n_mine)
            hipLaunchKernelGGL(k_nlhe_entry_keys, dim3((n_mine + 255u) / 256u), dim3(256), 0, st, h->tab, mine_ent, (uint32_t)eb, n_mine, kp, kb, kc);
        // padded gathers: four planes (entries, past, choices, present), each world x width items
        const size_t unit[4] = {eb, 8, 8, 4};
        size_t all_bytes = 0, pk_bytes = 0;
        for (int q = 0; q < 4; ++q) all_bytes += (size_t)world * width * unit[q], pk_bytes += (size_t)std::max(total, 1u) * unit[q];
        if ((rc = grow(&h->x_all, &h->x_all_bytes, std::max<size_t>(all_bytes, 64)))) return rc;
        if ((rc = grow(&h->x_packed, &h->x_packed_bytes, std::max<size_t>(pk_bytes, 64)))) return rc;
        unsigned char* all = reinterpret_cast<unsigned char*>(h->x_all);
        unsigned char* pk = reinterpret_cast<unsigned char*>(h->x_packed);
        const void* src[4] = {mine_ent, kp, kc, kb};
        unsigned char* pk_plane[4];
        size_t all_off = 0, pk_off = 0;
        for (int q = 0; q < 4 && width; ++q) {
            unsigned char* plane = all + all_off;
            if ((rc = rp::comm_all_gather(c, src[q], plane, (size_t)width * unit[q], st))) return rc;  // reads `width` items of mine: within its buffers
            pk_plane[q] = pk + pk_off;
            size_t at = 0;
            for (uint32_t r = 0; r < world; ++r) {  // rank-major packing
                if (counts[r])
                    HIP_TRY(hipMemcpyAsync(pk_plane[q] + at, plane + (size_t)r * width * unit[q], (size_t)counts[r] * unit[q], hipMemcpyDeviceToDevice, st));
                at += (size_t)counts[r] * unit[q];
            }
            all_off += (size_t)world * width * unit[q];
            pk_off += (size_t)total * unit[q];
        }
        if (!width) pk_plane[0] = pk_plane[1] = pk_plane[2] = pk_plane[3] = pk;
        if ((rc = rp_nlhe_step_apply(h, pk_plane[0], reinterpret_cast<const uint64_t*>(pk_plane[1]), reinterpret_cast<const uint32_t*>(pk_plane[3]),
                                     reinterpret_cast<const uint64_t*>(pk_plane[2]), total)))
            return rc;
    }
    return RP_OK;
}

int rp_nlhe_set_stream(rp_nlhe* h, void* hip_stream) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_set_stream: null handle");
    return rp_profile_set_stream(h->prof, hip_stream);
}

int rp_nlhe_sync(rp_nlhe* h) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_sync: null handle");
    int rc = rp_profile_sync(h->prof);
    if (rc) return rc;
    uint32_t err = 0;  // keys of an exchange that did not fit the table: reported once, then cleared
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpy(&err, h->d_remap_err, 4, hipMemcpyDeviceToHost));
    if (err) {
        HIP_TRY(hipMemset(h->d_remap_err, 0, 4));
        return nl_capacity_error(err);
    }
    return RP_OK;
}

}  // extern "C"

#ifdef NL_TREE_PROF  // diagnostic build only (scripts/r6_nltree_prof.sh): k_nl_tree's phase clocks
extern "C" RP_API int rp_nl_tree_prof(uint64_t* out16, int reset) {
    unsigned long long z[16] = {0};
    if (out16) HIP_TRY(hipMemcpyFromSymbol(out16, HIP_SYMBOL(rp::g_nl_prof), sizeof(z)));
    if (reset) HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(rp::g_nl_prof), z, sizeof(z)));
    return RP_OK;
}
extern "C" RP_API int rp_nl_tree_rec(uint32_t* out, uint32_t trees) {
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(rp::g_nl_rec), (size_t)std::min<uint32_t>(trees, 2048u) * 16u * 4u));
    return RP_OK;
}
#endif

// ---- the read side: read-only entry points in pairs, by the rule of host_util.hpp ("entry points in pairs"), on the profile's stream
namespace {
// ---- queries by NlheInfo key (nlmc_query.hpp): one launch
uint32_t nlq_blocks(const rp_nlhe* h, uint64_t n, uint32_t per_block) {
    return (uint32_t)std::min<uint64_t>((n + per_block - 1) / per_block, h->grid_cap);
}
int nlq_policy_check(const rp_nlhe* h, rp_dist_kind kind, uint64_t n, const void* past, const void* present, const void* choices, const void* policy) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_policy: NULL handle");
    if (kind != RP_DIST_ITERATED && kind != RP_DIST_AVERAGED && kind != RP_DIST_SAMPLING)
        return rp::fail(RP_ERR_INVALID, "rp_nlhe_policy: unknown distribution kind %d", (int)kind);
    if (n == 0) return RP_OK;
    if (!past || !present || !choices || !policy) return rp::fail(RP_ERR_INVALID, "rp_nlhe_policy: NULL keys or NULL policy with n > 0");
    return RP_OK;
}
int nlq_memory_check(const rp_nlhe* h, uint64_t n, const void* past, const void* present, const void* choices, const void* enc) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_memory: NULL handle");
    if (n == 0) return RP_OK;
    if (!past || !present || !choices || !enc) return rp::fail(RP_ERR_INVALID, "rp_nlhe_memory: NULL keys or NULL enc with n > 0");
    return RP_OK;
}
}  // namespace

extern "C" {

int rp_nlhe_policy_device(rp_nlhe* h, rp_dist_kind kind, uint64_t n, const uint64_t* past, const uint32_t* present, const uint64_t* choices,
                          float* policy, uint8_t* edges, uint8_t* n_actions, uint8_t* found) {
    int rc = nlq_policy_check(h, kind, n, past, present, choices, policy);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = rp::profile_stream(h->prof);
    const NlQuery q{n, past, present, choices, edges, n_actions, found};
    const DistParams hp{h->hp.temperature, h->hp.smoothing, h->hp.curiosity};
    // RP_NLHE_QUERY_SHAPE=lane (read at every call, so that one table answers through both shapes alternately:
    // scripts/nlhe_policy_rate.py): the one-lane-per-query kernel the shipped shape is measured against
    const char* shape = getenv("RP_NLHE_QUERY_SHAPE");
    if (shape && !strcmp(shape, "lane"))
        hipLaunchKernelGGL(k_nl_policy_lane, dim3(nlq_blocks(h, n, NLQ_BLOCK)), dim3(NLQ_BLOCK), 0, st, h->tab, q, (int)kind, hp, policy);
    else if (kind == RP_DIST_ITERATED)
        hipLaunchKernelGGL(k_nl_policy_group<false>, dim3(nlq_blocks(h, n, NLQ_BLOCK / NLQ_GROUP)), dim3(NLQ_BLOCK), 0, st, h->tab, q, (int)kind, hp, policy);
    else
        hipLaunchKernelGGL(k_nl_policy_group<true>, dim3(nlq_blocks(h, n, NLQ_BLOCK / NLQ_GROUP)), dim3(NLQ_BLOCK), 0, st, h->tab, q, (int)kind, hp, policy);
    HIP_TRY(hipGetLastError());
    return RP_OK;
}

int rp_nlhe_policy(rp_nlhe* h, rp_dist_kind kind, uint64_t n, const uint64_t* past, const uint32_t* present, const uint64_t* choices,
                   float* policy, uint8_t* edges, uint8_t* n_actions, uint8_t* found) {
    int rc = nlq_policy_check(h, kind, n, past, present, choices, policy);
    if (rc || n == 0) return rc;
    rp::Stage s(h->device, rp::profile_stream(h->prof));
    s.in(past, n).in(present, n).in(choices, n).out(policy, n * NLMC_A).out(edges, n * NLMC_A).out(n_actions, n).out(found, n);
    if ((rc = s.up()) || (rc = rp_nlhe_policy_device(h, kind, n, past, present, choices, policy, edges, n_actions, found))) return rc;
    return s.down();
}

int rp_nlhe_memory_device(rp_nlhe* h, uint64_t n, const uint64_t* past, const uint32_t* present, const uint64_t* choices, rp_encounter* enc,
                          uint8_t* n_actions, uint8_t* found) {
    int rc = nlq_memory_check(h, n, past, present, choices, enc);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(h->device));
    const NlQuery q{n, past, present, choices, nullptr, n_actions, found};
    hipLaunchKernelGGL(k_nl_memory, dim3(nlq_blocks(h, n, NLQ_BLOCK / NLQ_MGROUP)), dim3(NLQ_BLOCK), 0, rp::profile_stream(h->prof), h->tab, q, enc);
    HIP_TRY(hipGetLastError());
    return RP_OK;
}

int rp_nlhe_memory(rp_nlhe* h, uint64_t n, const uint64_t* past, const uint32_t* present, const uint64_t* choices, rp_encounter* enc,
                   uint8_t* n_actions, uint8_t* found) {
    int rc = nlq_memory_check(h, n, past, present, choices, enc);
    if (rc || n == 0) return rc;
    rp::Stage s(h->device, rp::profile_stream(h->prof));
    s.in(past, n).in(present, n).in(choices, n).out(enc, n * NLMC_A).out(n_actions, n).out(found, n);
    if ((rc = s.up()) || (rc = rp_nlhe_memory_device(h, n, past, present, choices, enc, n_actions, found))) return rc;
    return s.down();
}

}  // extern "C"

// ---- ranges (nlmc_range.hpp): one workgroup per recall, at most NR_CHUNK recalls per launch
namespace {
constexpr uint64_t NR_CHUNK = 1ull << 20;
// items per launch of the calls cut by NR_CHUNK (ranges, frontier payoffs, worlds, AIVAT, matches, translation): RP_NLHE_READ_CHUNK
// (tests: a batch of a few items in several launches), 1 .. 2^20, else NR_CHUNK.  Read at every call
int nr_chunk(uint64_t* out) {
    *out = NR_CHUNK;
    const char* s = getenv("RP_NLHE_READ_CHUNK");
    if (!s || !*s) return RP_OK;
    char* end = nullptr;
    const long long v = strtoll(s, &end, 10);
    if (*end || v < 1 || v > (long long)NR_CHUNK)
        return rp::fail(RP_ERR_INVALID, "RP_NLHE_READ_CHUNK is '%s': 1 .. %llu", s, (unsigned long long)NR_CHUNK);
    *out = (uint64_t)v;
    return RP_OK;
}
int nr_launch(rp_nlhe* h, int kind, int normalize, uint64_t n, const rp_nlhe_recall* recalls, uint32_t* count, uint64_t* holes, float* reach,
              float* mass, uint8_t* seen, uint8_t* status) {
    uint64_t chunk = 0;
    int rc = nr_chunk(&chunk);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = rp::profile_stream(h->prof);
    return rp::chunks(n, chunk, [&](uint64_t at, uint32_t m) {
        NrArgs q{};
        q.recalls = recalls + at;
        q.kind = kind;
        q.normalize = normalize;
        q.count = rp::from(count, at);
        q.holes = rp::from(holes, at * RP_NLHE_MAX_HOLES);
        q.reach = rp::from(reach, at * RP_NLHE_MAX_HOLES);
        q.mass = rp::from(mass, at * 256u);
        q.seen = rp::from(seen, at * 256u);
        q.status = rp::from(status, at);
        hipLaunchKernelGGL(k_nl_range, dim3(m), dim3(NR_BLOCK), 0, st, h->tab, h->prm, q);
    });
}
int nr_reaches_check(const rp_nlhe* h, rp_reach_kind kind, uint64_t n, const void* recalls, const void* count, const void* reach) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_reaches: NULL handle");
    if (kind != RP_REACH_OPPONENT && kind != RP_REACH_SIGNALLED) return rp::fail(RP_ERR_INVALID, "rp_nlhe_reaches: unknown reach kind %d", (int)kind);
    if (n == 0) return RP_OK;
    if (!recalls || !count || !reach) return rp::fail(RP_ERR_INVALID, "rp_nlhe_reaches: NULL recalls, count or reach with n_recalls > 0");
    return RP_OK;
}
int nr_range_check(const rp_nlhe* h, uint64_t n, const void* recalls, const void* mass, const void* seen) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_opponent_range: NULL handle");
    if (n == 0) return RP_OK;
    if (!recalls || !mass || !seen) return rp::fail(RP_ERR_INVALID, "rp_nlhe_opponent_range: NULL recalls, mass or seen with n_recalls > 0");
    return RP_OK;
}
}  // namespace

extern "C" {

int rp_nlhe_reaches_device(rp_nlhe* h, rp_reach_kind kind, int normalize, uint64_t n, const rp_nlhe_recall* recalls, uint32_t* count,
                           uint64_t* holes, float* reach, uint8_t* status) {
    int rc = nr_reaches_check(h, kind, n, recalls, count, reach);
    if (rc || n == 0) return rc;
    return nr_launch(h, (int)kind, normalize ? 1 : 0, n, recalls, count, holes, reach, nullptr, nullptr, status);
}

int rp_nlhe_reaches(rp_nlhe* h, rp_reach_kind kind, int normalize, uint64_t n, const rp_nlhe_recall* recalls, uint32_t* count, uint64_t* holes,
                    float* reach, uint8_t* status) {
    int rc = nr_reaches_check(h, kind, n, recalls, count, reach);
    if (rc || n == 0) return rc;
    rp::Stage s(h->device, rp::profile_stream(h->prof));
    s.in(recalls, n).out(holes, n * RP_NLHE_MAX_HOLES).out(reach, n * RP_NLHE_MAX_HOLES).out(count, n).out(status, n);
    if ((rc = s.up()) || (rc = rp_nlhe_reaches_device(h, kind, normalize, n, recalls, count, holes, reach, status))) return rc;
    return s.down();
}

int rp_nlhe_opponent_range_device(rp_nlhe* h, uint64_t n, const rp_nlhe_recall* recalls, float* mass, uint8_t* seen, uint8_t* status) {
    int rc = nr_range_check(h, n, recalls, mass, seen);
    if (rc || n == 0) return rc;
    return nr_launch(h, (int)RP_REACH_OPPONENT, 0, n, recalls, nullptr, nullptr, nullptr, mass, seen, status);
}

int rp_nlhe_opponent_range(rp_nlhe* h, uint64_t n, const rp_nlhe_recall* recalls, float* mass, uint8_t* seen, uint8_t* status) {
    int rc = nr_range_check(h, n, recalls, mass, seen);
    if (rc || n == 0) return rc;
    rp::Stage s(h->device, rp::profile_stream(h->prof));
    s.in(recalls, n).out(mass, n * 256u).out(seen, n * 256u).out(status, n);
    if ((rc = s.up()) || (rc = rp_nlhe_opponent_range_device(h, n, recalls, mass, seen, status))) return rc;
    return s.down();
}

}  // extern "C"

// ---- frontier payoffs (nlmc_frontier.hpp): one workgroup per frontier, at most NR_CHUNK frontiers per launch
namespace {
// rollouts = 0 is 1
int nf_check(const rp_nlhe* h, uint64_t n, const void* frontiers, float bias, uint32_t* rollouts, const void* payoffs) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_frontier_payoffs: NULL handle");
    if (!(bias > 0.0f) || std::isinf(bias)) return rp::fail(RP_ERR_INVALID, "rp_nlhe_frontier_payoffs: bias must be finite and positive");
    if (*rollouts > 4096u) return rp::fail(RP_ERR_INVALID, "rp_nlhe_frontier_payoffs: rollouts %u above 4096", *rollouts);
    if (*rollouts == 0u) *rollouts = 1u;
    if (n == 0) return RP_OK;
    if (!frontiers || !payoffs) return rp::fail(RP_ERR_INVALID, "rp_nlhe_frontier_payoffs: NULL frontiers or payoffs with n > 0");
    return RP_OK;
}
}  // namespace

extern "C" {

int rp_nlhe_frontier_payoffs_device(rp_nlhe* h, uint64_t n, const rp_nlhe_frontier* frontiers, float bias, uint32_t rollouts, uint64_t seed,
                                    uint64_t first_id, float* payoffs, int16_t* won, uint8_t* status) {
    int rc = nf_check(h, n, frontiers, bias, &rollouts, payoffs);
    if (rc || n == 0) return rc;
    uint64_t chunk = 0;
    if ((rc = nr_chunk(&chunk))) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = rp::profile_stream(h->prof);
    return rp::chunks(n, chunk, [&](uint64_t at, uint32_t m) {
        NfArgs q{};
        q.frontiers = frontiers + at;
        q.bias = bias;
        q.rollouts = rollouts;
        q.step_hash = rp_node_hash_step(seed, 0);
        q.first_id = first_id + at;
        q.payoffs = payoffs + at * NF_CELLS;
        q.won = rp::from(won, at * NF_CELLS * rollouts);
        q.status = rp::from(status, at);
        hipLaunchKernelGGL(k_nl_frontier, dim3(m), dim3(NF_BLOCK), 0, st, h->tab, h->prm, q);
    });
}

int rp_nlhe_frontier_payoffs(rp_nlhe* h, uint64_t n, const rp_nlhe_frontier* frontiers, float bias, uint32_t rollouts, uint64_t seed,
                             uint64_t first_id, float* payoffs, int16_t* won, uint8_t* status) {
    int rc = nf_check(h, n, frontiers, bias, &rollouts, payoffs);
    if (rc || n == 0) return rc;
    rp::Stage s(h->device, rp::profile_stream(h->prof));
    s.in(frontiers, n).out(payoffs, n * NF_CELLS).out(won, n * NF_CELLS * rollouts).out(status, n);
    if ((rc = s.up()) || (rc = rp_nlhe_frontier_payoffs_device(h, n, frontiers, bias, rollouts, seed, first_id, payoffs, won, status))) return rc;
    return s.down();
}

}  // extern "C"

// ---- depth-limited re-solve (nlmc_depth.hpp): one workgroup per solve, at most ND_CHUNK solves per launch
namespace {
constexpr uint64_t ND_CHUNK = 4096;  // solves per launch: what the overflow region is sized for
// the fields the depth and the subgame args share: refused before anything else is looked at (so that they can be checked without a
// device); rollouts = 0 is 1
template <typename Args>
int nd_args_check(const char* name, const Args* a, uint32_t* rollouts) {
    if (!a) return rp::fail(RP_ERR_INVALID, "%s: NULL args", name);
    if (a->iterations < 1u || a->iterations > RP_NLHE_DEPTH_MAX_ITERATIONS)
        return rp::fail(RP_ERR_INVALID, "%s: iterations %u outside 1 .. %u", name, a->iterations, RP_NLHE_DEPTH_MAX_ITERATIONS);
    if (a->rollouts > 4096u) return rp::fail(RP_ERR_INVALID, "%s: rollouts %u above 4096", name, a->rollouts);
    if (!(a->bias > 0.0f) || std::isinf(a->bias)) return rp::fail(RP_ERR_INVALID, "%s: bias must be finite and positive", name);
    if (!(a->prior > 0.0f) || std::isinf(a->prior)) return rp::fail(RP_ERR_INVALID, "%s: prior must be finite and positive", name);
    uint32_t reserved[2] = {0u, 0u};  // one word in the depth args, two in the subgame args
    static_assert(sizeof(Args::reserved) <= sizeof(reserved), "the reserved words of an args struct");
    memcpy(reserved, &a->reserved, sizeof(Args::reserved));
    if (reserved[0] != 0u || reserved[1] != 0u) return rp::fail(RP_ERR_INVALID, "%s: reserved must be 0", name);
    *rollouts = a->rollouts == 0u ? 1u : a->rollouts;
    return RP_OK;
}
int nd_check(const rp_nlhe* h, uint64_t n, const void* entries, const rp_nlhe_depth_args* args, const void* results, const void* rows,
             uint32_t* rollouts) {
    int rc = nd_args_check("rp_nlhe_depth_solve", args, rollouts);
    if (rc || n == 0) return rc;
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_depth_solve: NULL handle");
    if (!entries || !results) return rp::fail(RP_ERR_INVALID, "rp_nlhe_depth_solve: NULL entries or results with n > 0");
    if (args->rows_cap > 0u && !rows) return rp::fail(RP_ERR_INVALID, "rp_nlhe_depth_solve: NULL rows with rows_cap > 0");
    return RP_OK;
}
}  // namespace

extern "C" {

void rp_nlhe_depth_args_default(rp_nlhe_depth_args* out) {
    if (!out) return;
    *out = rp_nlhe_depth_args{};
    out->iterations = 1;
    out->rollouts = 16;          // FrontierHyperParams::default
    out->bias = 5.0f;
    out->prior = 16384.0f;       // WarmstartHyperParams::default: 1 << 14
}

int rp_nlhe_depth_solve_device(rp_nlhe* h, uint64_t n, const rp_nlhe_frontier* entries, const int8_t* origin, const rp_nlhe_depth_args* args,
                               rp_nlhe_depth_result* results, rp_nlhe_depth_row* rows) {
    uint32_t rollouts = 0;
    int rc = nd_check(h, n, entries, args, results, rows, &rollouts);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = rp::profile_stream(h->prof);
    // the overflow rows of one launch's solves: launches of one call follow each other on the stream and share the region
    const size_t need = (size_t)std::min<uint64_t>(ND_CHUNK, n) * ND_ROWS_OVF * sizeof(NdRow);
    if ((rc = rp::grow(h->depth_rows, h->depth_rows_bytes, need, st))) return rc;
    return rp::chunks(n, ND_CHUNK, [&](uint64_t at, uint32_t m) {
        NdArgs q{};
        q.entries = entries + at;
        q.origin = rp::from(origin, at);
        q.iterations = args->iterations;
        q.rollouts = rollouts;
        q.rows_cap = rows ? args->rows_cap : 0u;
        q.bias = args->bias;
        q.prior = args->prior;
        q.step_hash_rollout = rp_node_hash_step(args->seed, 0);
        q.step_hash_tree = rp_node_hash_step(args->seed, 2);
        q.first_id = args->first_id + at;
        q.overflow = static_cast<NdRow*>(h->depth_rows);
        q.results = results + at;
        q.rows = rp::from(rows, at * args->rows_cap);
        hipLaunchKernelGGL(k_nl_depth, dim3(m), dim3(ND_BLOCK), 0, st, h->tab, h->prm, q);
    });
}

int rp_nlhe_depth_solve(rp_nlhe* h, uint64_t n, const rp_nlhe_frontier* entries, const int8_t* origin, const rp_nlhe_depth_args* args,
                        rp_nlhe_depth_result* results, rp_nlhe_depth_row* rows) {
    uint32_t rollouts = 0;
    int rc = nd_check(h, n, entries, args, results, rows, &rollouts);
    if (rc || n == 0) return rc;
    rp::Stage s(h->device, rp::profile_stream(h->prof));
    s.in(entries, n).in(origin, n).out(results, n).out(rows, n * args->rows_cap);
    if ((rc = s.up()) || (rc = rp_nlhe_depth_solve_device(h, n, entries, origin, args, results, rows))) return rc;
    return s.down();
}

}  // extern "C"

// ---- subgame worlds (nlmc_world.hpp): one workgroup per recall (partition: per row), at most NR_CHUNK per launch
namespace {
constexpr uint32_t NW_MAX_DEALS = 4096u;
// belief (deals == 0) and restrict (deals > 0) are one kernel: every pointer in device memory
int nw_launch(rp_nlhe* h, uint64_t n, const rp_nlhe_recall* recalls, uint8_t* world, float* weights, uint8_t* hole_world, uint32_t deals,
              const uint8_t* worlds, uint64_t seed, uint64_t first_id, uint64_t* holes, uint8_t* world_out, uint16_t* attempts, uint8_t* status) {
    uint64_t chunk = 0;
    int rc = nr_chunk(&chunk);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = rp::profile_stream(h->prof);
    return rp::chunks(n, chunk, [&](uint64_t at, uint32_t m) {
        NwArgs q{};
        q.recalls = recalls + at;
        q.world = rp::from(world, at * 256u);
        q.weights = rp::from(weights, at * RP_NLHE_WORLDS);
        q.hole_world = rp::from(hole_world, at * RP_NLHE_MAX_HOLES);
        q.deals = deals;
        q.worlds = rp::from(worlds, at * deals);
        q.step_hash = rp_node_hash_step(seed, 1);
        q.first_id = first_id + at;
        q.holes = rp::from(holes, at * deals);
        q.world_out = rp::from(world_out, at * deals);
        q.attempts = rp::from(attempts, at * deals);
        q.status = rp::from(status, at);
        hipLaunchKernelGGL(k_nl_world, dim3(m), dim3(NW_BLOCK), 0, st, h->tab, h->prm, q);
    });
}
int nw_partition_check(const rp_nlhe* h, uint64_t n, const void* mass, const void* seen, const void* world, const void* weights) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_partition: NULL handle");
    if (n == 0) return RP_OK;
    if (!mass || !seen || !world || !weights) return rp::fail(RP_ERR_INVALID, "rp_nlhe_partition: NULL mass, seen, world or weights with n > 0");
    return RP_OK;
}
int nw_belief_check(const rp_nlhe* h, uint64_t n, const void* recalls, const void* world, const void* weights) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_belief: NULL handle");
    if (n == 0) return RP_OK;
    if (!recalls || !world || !weights) return rp::fail(RP_ERR_INVALID, "rp_nlhe_belief: NULL recalls, world or weights with n_recalls > 0");
    return RP_OK;
}
// RP_OK with n == 0 or deals == 0 is the call's answer
int nw_restrict_check(const rp_nlhe* h, uint64_t n, const void* recalls, uint32_t deals, const void* holes) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_restrict: NULL handle");
    if (deals > NW_MAX_DEALS) return rp::fail(RP_ERR_INVALID, "rp_nlhe_restrict: deals %u above %u", deals, NW_MAX_DEALS);
    if (n == 0 || deals == 0) return RP_OK;
    if (!recalls || !holes) return rp::fail(RP_ERR_INVALID, "rp_nlhe_restrict: NULL recalls or holes with n_recalls > 0");
    return RP_OK;
}
}  // namespace

extern "C" {

int rp_nlhe_partition_device(rp_nlhe* h, uint64_t n, const float* mass, const uint8_t* seen, uint8_t* world, float* weights) {
    int rc = nw_partition_check(h, n, mass, seen, world, weights);
    if (rc || n == 0) return rc;
    uint64_t chunk = 0;
    if ((rc = nr_chunk(&chunk))) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = rp::profile_stream(h->prof);
    return rp::chunks(n, chunk, [&](uint64_t at, uint32_t m) {
        hipLaunchKernelGGL(k_nl_partition, dim3(m), dim3(NW_BLOCK), 0, st, mass + at * 256u, seen + at * 256u, world + at * 256u,
                           weights + at * RP_NLHE_WORLDS);
    });
}

int rp_nlhe_partition(rp_nlhe* h, uint64_t n, const float* mass, const uint8_t* seen, uint8_t* world, float* weights) {
    int rc = nw_partition_check(h, n, mass, seen, world, weights);
    if (rc || n == 0) return rc;
    rp::Stage s(h->device, rp::profile_stream(h->prof));
    s.in(mass, n * 256u).in(seen, n * 256u).out(world, n * 256u).out(weights, n * RP_NLHE_WORLDS);
    if ((rc = s.up()) || (rc = rp_nlhe_partition_device(h, n, mass, seen, world, weights))) return rc;
    return s.down();
}

int rp_nlhe_belief_device(rp_nlhe* h, uint64_t n, const rp_nlhe_recall* recalls, uint8_t* world, float* weights, uint8_t* hole_world,
                          uint8_t* status) {
    int rc = nw_belief_check(h, n, recalls, world, weights);
    if (rc || n == 0) return rc;
    return nw_launch(h, n, recalls, world, weights, hole_world, 0, nullptr, 0, 0, nullptr, nullptr, nullptr, status);
}

int rp_nlhe_belief(rp_nlhe* h, uint64_t n, const rp_nlhe_recall* recalls, uint8_t* world, float* weights, uint8_t* hole_world, uint8_t* status) {
    int rc = nw_belief_check(h, n, recalls, world, weights);
    if (rc || n == 0) return rc;
    rp::Stage s(h->device, rp::profile_stream(h->prof));
    s.in(recalls, n).out(world, n * 256u).out(weights, n * RP_NLHE_WORLDS).out(hole_world, n * RP_NLHE_MAX_HOLES).out(status, n);
    if ((rc = s.up()) || (rc = rp_nlhe_belief_device(h, n, recalls, world, weights, hole_world, status))) return rc;
    return s.down();
}

int rp_nlhe_restrict_device(rp_nlhe* h, uint64_t n, const rp_nlhe_recall* recalls, uint32_t deals, const uint8_t* worlds, uint64_t seed,
                            uint64_t first_id, uint64_t* holes, uint8_t* world_out, uint16_t* attempts, uint8_t* status) {
    int rc = nw_restrict_check(h, n, recalls, deals, holes);
    if (rc || n == 0 || deals == 0) return rc;
    return nw_launch(h, n, recalls, nullptr, nullptr, nullptr, deals, worlds, seed, first_id, holes, world_out, attempts, status);
}

int rp_nlhe_restrict(rp_nlhe* h, uint64_t n, const rp_nlhe_recall* recalls, uint32_t deals, const uint8_t* worlds, uint64_t seed, uint64_t first_id,
                     uint64_t* holes, uint8_t* world_out, uint16_t* attempts, uint8_t* status) {
    int rc = nw_restrict_check(h, n, recalls, deals, holes);
    if (rc || n == 0 || deals == 0) return rc;
    rp::Stage s(h->device, rp::profile_stream(h->prof));
    s.in(recalls, n).in(worlds, n * deals).out(holes, n * deals).out(world_out, n * deals).out(attempts, n * deals).out(status, n);
    if ((rc = s.up()) || (rc = rp_nlhe_restrict_device(h, n, recalls, deals, worlds, seed, first_id, holes, world_out, attempts, status))) return rc;
    return s.down();
}

}  // extern "C"

// ---- safe subgame re-solve (nlmc_subgame.hpp): one workgroup per solve, at most NS_CHUNK solves per launch
namespace {
constexpr uint64_t NS_CHUNK = 1024;  // solves per launch: what the overflow region is sized for
int ns_check(const rp_nlhe* h, uint64_t n, const void* entries, const void* hole_world, const void* weights, const rp_nlhe_subgame_args* args,
             const void* results, const void* rows, const void* deals, uint32_t* rollouts) {
    int rc = nd_args_check("rp_nlhe_subgame_solve", args, rollouts);
    if (rc || n == 0) return rc;
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_subgame_solve: NULL handle");
    if (!entries || !hole_world || !weights || !results)
        return rp::fail(RP_ERR_INVALID, "rp_nlhe_subgame_solve: NULL entries, hole_world, weights or results with n > 0");
    if (args->rows_cap > 0u && !rows) return rp::fail(RP_ERR_INVALID, "rp_nlhe_subgame_solve: NULL rows with rows_cap > 0");
    if (args->deals_cap > 0u && !deals) return rp::fail(RP_ERR_INVALID, "rp_nlhe_subgame_solve: NULL deals with deals_cap > 0");
    return RP_OK;
}
}  // namespace

extern "C" {

void rp_nlhe_subgame_args_default(rp_nlhe_subgame_args* out) {
    if (!out) return;
    *out = rp_nlhe_subgame_args{};
    out->iterations = 1;
    out->rollouts = 16;     // FrontierHyperParams::default
    out->bias = 5.0f;
    out->prior = 16384.0f;  // WarmstartHyperParams::default: 1 << 14
}

int rp_nlhe_subgame_solve_device(rp_nlhe* h, uint64_t n, const rp_nlhe_frontier* entries, const uint8_t* hole_world, const float* weights,
                                 const int8_t* origin, const rp_nlhe_subgame_args* args, rp_nlhe_subgame_result* results, rp_nlhe_subgame_row* rows,
                                 rp_nlhe_subgame_deal* deals) {
    uint32_t rollouts = 0;
    int rc = ns_check(h, n, entries, hole_world, weights, args, results, rows, deals, &rollouts);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = rp::profile_stream(h->prof);
    // the overflow rows of one launch's solves: launches of one call follow each other on the stream and share the region
    const size_t need = (size_t)std::min<uint64_t>(NS_CHUNK, n) * NS_ROWS_OVF * sizeof(NdRow);
    if ((rc = rp::grow(h->subgame_rows, h->subgame_rows_bytes, need, st))) return rc;
    return rp::chunks(n, NS_CHUNK, [&](uint64_t at, uint32_t m) {
        NsArgs q{};
        q.entries = entries + at;
        q.hole_world = hole_world + at * RP_NLHE_MAX_HOLES;
        q.weights = weights + at * RP_NLHE_WORLDS;
        q.origin = rp::from(origin, at);
        q.iterations = args->iterations;
        q.rollouts = rollouts;
        q.rows_cap = rows ? args->rows_cap : 0u;
        q.deals_cap = deals ? args->deals_cap : 0u;
        q.bias = args->bias;
        q.prior = args->prior;
        q.step_hash_rollout = rp_node_hash_step(args->seed, 0);
        q.step_hash_deal = rp_node_hash_step(args->seed, 1);
        q.step_hash_tree = rp_node_hash_step(args->seed, 2);
        q.first_id = args->first_id + at;
        q.overflow = static_cast<NdRow*>(h->subgame_rows);
        q.results = results + at;
        q.rows = q.rows_cap ? rows + at * args->rows_cap : nullptr;
        q.deals = q.deals_cap ? deals + at * args->deals_cap : nullptr;
        hipLaunchKernelGGL(k_nl_subgame, dim3(m), dim3(NS_BLOCK), 0, st, h->tab, h->prm, q);
    });
}

int rp_nlhe_subgame_solve(rp_nlhe* h, uint64_t n, const rp_nlhe_frontier* entries, const uint8_t* hole_world, const float* weights, const int8_t* origin,
                          const rp_nlhe_subgame_args* args, rp_nlhe_subgame_result* results, rp_nlhe_subgame_row* rows, rp_nlhe_subgame_deal* deals) {
    uint32_t rollouts = 0;
    int rc = ns_check(h, n, entries, hole_world, weights, args, results, rows, deals, &rollouts);
    if (rc || n == 0) return rc;
    rp::Stage s(h->device, rp::profile_stream(h->prof));
    s.in(entries, n).in(hole_world, n * RP_NLHE_MAX_HOLES).in(weights, n * RP_NLHE_WORLDS).in(origin, n);
    s.out(results, n).out(rows, n * args->rows_cap).out(deals, n * args->deals_cap);
    if ((rc = s.up()) || (rc = rp_nlhe_subgame_solve_device(h, n, entries, hole_world, weights, origin, args, results, rows, deals))) return rc;
    return s.down();
}

}  // extern "C"

// ---- AIVAT (nlmc_aivat.hpp): one wavefront per hand, at most NR_CHUNK hands per launch
namespace {
int na_check(const rp_nlhe* h, uint64_t n, const void* hands, const void* hero, const void* villain, const void* chance, const void* total) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_aivat: NULL handle");
    if (n == 0) return RP_OK;
    if (!hands || !hero || !villain || !chance || !total)
        return rp::fail(RP_ERR_INVALID, "rp_nlhe_aivat: NULL hands, hero, villain, chance or total with n > 0");
    return RP_OK;
}
// ratio and erf of pokerkit/src/metrics.rs:102-119
float na_ratio(float num, float den) { return den > 0.0f ? num / den : 0.0f; }
float na_erf(float x) {
    const float A = 0.2316419f, B = 0.3989423f, C = 0.3193815f, D = -0.3565638f, E = 1.781478f, F = -1.821256f, G = 1.330274f;
    const float t = 1.0f / (1.0f + A * fabsf(x));
    const float d = B * rp_glibc_expf(-x * x / 2.0f);
    const float p = d * t * (C + t * (D + t * (E + t * (F + t * G))));
    return x > 0.0f ? 1.0f - p : p;
}
}  // namespace

extern "C" {

int rp_nlhe_aivat_device(rp_nlhe* h, uint64_t n, const rp_aivat_hand* hands, float* hero, float* villain, float* chance, float* total,
                         uint8_t* n_action, uint8_t* n_chance, uint8_t* status) {
    int rc = na_check(h, n, hands, hero, villain, chance, total);
    if (rc || n == 0) return rc;
    uint64_t chunk = 0;
    if ((rc = nr_chunk(&chunk))) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = rp::profile_stream(h->prof);
    return rp::chunks(n, chunk, [&](uint64_t at, uint32_t m) {
        const NaArgs q{hands + at, hero + at, villain + at, chance + at, total + at, rp::from(n_action, at), rp::from(n_chance, at), rp::from(status, at)};
        hipLaunchKernelGGL(k_nl_aivat, dim3(m), dim3(NA_BLOCK), 0, st, h->tab, h->prm, q);
    });
}

int rp_nlhe_aivat(rp_nlhe* h, uint64_t n, const rp_aivat_hand* hands, float* hero, float* villain, float* chance, float* total, uint8_t* n_action,
                  uint8_t* n_chance, uint8_t* status) {
    int rc = na_check(h, n, hands, hero, villain, chance, total);
    if (rc || n == 0) return rc;
    rp::Stage s(h->device, rp::profile_stream(h->prof));
    s.in(hands, n).out(hero, n).out(villain, n).out(chance, n).out(total, n).out(n_action, n).out(n_chance, n).out(status, n);
    if ((rc = s.up()) || (rc = rp_nlhe_aivat_device(h, n, hands, hero, villain, chance, total, n_action, n_chance, status))) return rc;
    return s.down();
}

int rp_aivat_summarize(uint64_t n, const float* adjusted, float raw_stddev, rp_aivat_summary* out) {
    if (!out) return rp::fail(RP_ERR_INVALID, "rp_aivat_summarize: NULL out");
    if (n > 0 && !adjusted) return rp::fail(RP_ERR_INVALID, "rp_aivat_summarize: NULL adjusted with n > 0");
    const float nf = (float)n;
    float won = 0.0f;
    for (uint64_t i = 0; i < n; ++i) won = won + adjusted[i];
    const float mean = na_ratio(won, nf);
    float squares = 0.0f;
    for (uint64_t i = 0; i < n; ++i) squares = squares + (adjusted[i] - mean) * (adjusted[i] - mean);
    const float variance = na_ratio(squares, nf);
    const float stderr_ = na_ratio(sqrtf(variance), sqrtf(nf));
    const float raw = raw_stddev * raw_stddev, adj = stderr_ * stderr_ * nf;
    out->won = won;
    out->mean = mean;
    out->stderr_ = stderr_;
    out->reduction = adj > 0.0f ? raw / adj : 1.0f;
    out->pvalue = stderr_ > 0.0f ? 2.0f * na_erf(-fabsf(mean) / stderr_) : 1.0f;
    return RP_OK;
}

}  // extern "C"

// ---- matches (nlmc_match.hpp): one lane per hand, at most NR_CHUNK hands per launch
namespace {
// the args alone, without a device; `name`: the un-suffixed function that refuses
int nm_args_check(const char* name, const rp_nlhe_match_args* a) {
    if (a->agent[0] > (uint8_t)RP_AGENT_FISH || a->agent[1] > (uint8_t)RP_AGENT_FISH)
        return rp::fail(RP_ERR_INVALID, "%s: agent %u / %u is no rp_agent_kind", name, a->agent[0], a->agent[1]);
    if (a->dealer > 2u) return rp::fail(RP_ERR_INVALID, "%s: dealer %u above 2", name, a->dealer);
    if (a->hero > 1u) return rp::fail(RP_ERR_INVALID, "%s: hero %u above 1", name, a->hero);
    if (a->mirror > 1u || a->snap > 1u || a->board_mode > 1u) return rp::fail(RP_ERR_INVALID, "%s: mirror, snap and board_mode are 0 or 1", name);
    const bool std_stacks = a->stacks[0] == 0 && a->stacks[1] == 0;
    if (!std_stacks && (a->stacks[0] <= 0 || a->stacks[1] <= 0))
        return rp::fail(RP_ERR_INVALID, "%s: stacks %d, %d are neither 0,0 nor both positive", name, a->stacks[0], a->stacks[1]);
    for (uint8_t r : a->reserved)
        if (r != 0u) return rp::fail(RP_ERR_INVALID, "%s: reserved must be 0", name);
    return RP_OK;
}
// two handles play on one device and one encoder
int nm_pair_check(const char* name, const rp_nlhe* h0, const rp_nlhe* h1) {
    if (h1 && h1 != h0) {
        if (h1->device != h0->device) return rp::fail(RP_ERR_INVALID, "%s: the two handles are on devices %d and %d", name, h0->device, h1->device);
        bool same = h1->prm.encoder == h0->prm.encoder;
        for (int s = 0; s < 4 && same && h0->prm.encoder; ++s)
            same = h1->prm.tkeys[s] == h0->prm.tkeys[s] && h1->prm.tabs[s] == h0->prm.tabs[s] && h1->prm.tn[s] == h0->prm.tn[s];
        if (!same) return rp::fail(RP_ERR_INVALID, "%s: the two handles are built on different encoders", name);
    }
    return RP_OK;
}
int nm_check(const rp_nlhe* h0, const rp_nlhe* h1, const rp_nlhe_match_args* a) {
    if (!h0) return rp::fail(RP_ERR_INVALID, "rp_nlhe_match: NULL handle");
    if (!a) return rp::fail(RP_ERR_INVALID, "rp_nlhe_match: NULL args");
    int rc = nm_args_check("rp_nlhe_match", a);
    return rc ? rc : nm_pair_check("rp_nlhe_match", h0, h1);
}
// what h1's stream has queued for its table comes before what is queued on st next
int nm_after(hipStream_t st, hipStream_t st1) {
    if (st1 == st) return RP_OK;
    hipEvent_t ev;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, st1);
    if (e == hipSuccess) e = hipStreamWaitEvent(st, ev, 0);
    (void)hipEventDestroy(ev);  // the wait already queued keeps what it needs
    HIP_TRY(e);
    return RP_OK;
}
NmArgs nm_args(const rp_nlhe_match_args* args, uint64_t at, uint32_t m, rp_aivat_hand* hands, int16_t* won, uint8_t* rejected, uint8_t* status) {
    NmArgs q{};
    q.deal_hash = rp_node_hash_step(args->seed, 0);
    q.play_hash = rp_node_hash_step(args->seed, 1);
    q.first_id = args->first_id + at;
    q.n = m;
    q.stacks[0] = args->stacks[0], q.stacks[1] = args->stacks[1];
    q.agent[0] = args->agent[0], q.agent[1] = args->agent[1];
    q.dealer = args->dealer, q.hero = args->hero, q.mirror = args->mirror, q.snap = args->snap, q.board_mode = args->board_mode;
    q.hands = rp::from(hands, at);
    q.won = rp::from(won, at);
    q.rejected = rp::from(rejected, at);
    q.status = rp::from(status, at);
    return q;
}
}  // namespace

extern "C" {

void rp_nlhe_match_args_default(rp_nlhe_match_args* out) {
    if (!out) return;
    *out = rp_nlhe_match_args{};
    out->dealer = 2;
    out->board_mode = 1;
}

int rp_nlhe_match_device(rp_nlhe* h0, rp_nlhe* h1, uint64_t n, const rp_nlhe_match_args* args, rp_aivat_hand* hands, int16_t* won,
                         uint8_t* rejected, uint8_t* status) {
    int rc = nm_check(h0, h1, args);
    if (rc || n == 0) return rc;
    if (!h1) h1 = h0;
    uint64_t chunk = 0;
    if ((rc = nr_chunk(&chunk))) return rc;
    HIP_TRY(hipSetDevice(h0->device));
    hipStream_t st = rp::profile_stream(h0->prof), st1 = rp::profile_stream(h1->prof);
    if ((rc = nm_after(st, st1))) return rc;
    return rp::chunks(n, chunk, [&](uint64_t at, uint32_t m) {
        const NmArgs q = nm_args(args, at, m, hands, won, rejected, status);
        hipLaunchKernelGGL(k_nl_match, dim3((m + NM_BLOCK - 1u) / NM_BLOCK), dim3(NM_BLOCK), 0, st, h0->tab, h1->tab, h0->prm, q);
    });
}

int rp_nlhe_match(rp_nlhe* h0, rp_nlhe* h1, uint64_t n, const rp_nlhe_match_args* args, rp_aivat_hand* hands, int16_t* won, uint8_t* rejected,
                  uint8_t* status) {
    int rc = nm_check(h0, h1, args);
    if (rc || n == 0) return rc;
    rp::Stage s(h0->device, rp::profile_stream(h0->prof));
    s.out(hands, n).out(won, n).out(rejected, n).out(status, n);
    if ((rc = s.up()) || (rc = rp_nlhe_match_device(h0, h1, n, args, hands, won, rejected, status))) return rc;
    return s.down();
}

int rp_match_summarize(uint64_t n, const int16_t* won, rp_match_summary* out) {
    if (!out) return rp::fail(RP_ERR_INVALID, "rp_match_summarize: NULL out");
    if (n > 0 && !won) return rp::fail(RP_ERR_INVALID, "rp_match_summarize: NULL won with n > 0");
    *out = rp_match_summary{};
    out->hands = n;
    if (n == 0) return RP_OK;
    const double nf = (double)n, bb = (double)NL_BBLIND;
    double total = 0.0;
    for (uint64_t i = 0; i < n; ++i) total = total + (double)won[i] / bb;
    out->total_bb = total;
    out->bb_per_100 = total / nf * 100.0;
    if (n >= 2) {
        const double mean = total / nf;
        double squares = 0.0;
        for (uint64_t i = 0; i < n; ++i) {
            const double d = (double)won[i] / bb - mean;
            squares = squares + d * d;
        }
        out->stddev = sqrt(squares / (double)(n - 1));
    }
    out->confidence = 1.96 * out->stddev / sqrt(nf) * 100.0;
    return RP_OK;
}

}  // extern "C"

// ---- translation (nlmc_translate.hpp): one lane per hand, at most NR_CHUNK hands per launch
namespace {
int nx_check(const rp_nlhe* h, uint64_t n, const rp_nlhe_translate_args* a, const void* hands) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_translate: NULL handle");
    if (!a) return rp::fail(RP_ERR_INVALID, "rp_nlhe_translate: NULL args");
    if (a->kind > (uint8_t)RP_TRANSLATE_PHARGMAX) return rp::fail(RP_ERR_INVALID, "rp_nlhe_translate: kind %u is no rp_translation_kind", a->kind);
    for (uint8_t r : a->reserved)
        if (r != 0u) return rp::fail(RP_ERR_INVALID, "rp_nlhe_translate: reserved must be 0");
    if (n == 0) return RP_OK;
    if (!hands) return rp::fail(RP_ERR_INVALID, "rp_nlhe_translate: NULL hands with n > 0");
    return RP_OK;
}
}  // namespace

extern "C" {

void rp_nlhe_translate_args_default(rp_nlhe_translate_args* out) {
    if (!out) return;
    *out = rp_nlhe_translate_args{};
    out->kind = (uint8_t)RP_TRANSLATE_SNAP;
}

int rp_nlhe_translate_device(rp_nlhe* h, uint64_t n, const rp_nlhe_translate_args* args, const rp_aivat_hand* hands, const uint8_t* pov,
                             const uint8_t* upto, rp_nlhe_recall* recalls, uint8_t* play_edges, uint64_t* past, uint32_t* present,
                             uint64_t* choices, uint8_t* n_choices, uint8_t* status) {
    int rc = nx_check(h, n, args, hands);
    if (rc || n == 0) return rc;
    uint64_t chunk = 0;
    if ((rc = nr_chunk(&chunk))) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = rp::profile_stream(h->prof);
    return rp::chunks(n, chunk, [&](uint64_t at, uint32_t m) {
        NxArgs q{};
        q.hands = hands + at;
        q.pov = rp::from(pov, at);
        q.upto = rp::from(upto, at);
        q.hash = rp_node_hash_step(args->seed, 3);
        q.first_id = args->first_id + at;
        q.n = m;
        q.kind = args->kind;
        q.recalls = rp::from(recalls, at);
        q.play_edges = rp::from(play_edges, at * RP_AIVAT_MAX_PLAYS);
        q.past = rp::from(past, at);
        q.present = rp::from(present, at);
        q.choices = rp::from(choices, at);
        q.n_choices = rp::from(n_choices, at);
        q.status = rp::from(status, at);
        hipLaunchKernelGGL(k_nl_translate, dim3((m + NX_BLOCK - 1u) / NX_BLOCK), dim3(NX_BLOCK), 0, st, h->prm, q);
    });
}

int rp_nlhe_translate(rp_nlhe* h, uint64_t n, const rp_nlhe_translate_args* args, const rp_aivat_hand* hands, const uint8_t* pov,
                      const uint8_t* upto, rp_nlhe_recall* recalls, uint8_t* play_edges, uint64_t* past, uint32_t* present, uint64_t* choices,
                      uint8_t* n_choices, uint8_t* status) {
    int rc = nx_check(h, n, args, hands);
    if (rc || n == 0) return rc;
    rp::Stage s(h->device, rp::profile_stream(h->prof));
    s.in(hands, n).in(pov, n).in(upto, n);
    s.out(recalls, n).out(play_edges, n * RP_AIVAT_MAX_PLAYS).out(past, n).out(present, n).out(choices, n).out(n_choices, n).out(status, n);
    if ((rc = s.up()) ||
        (rc = rp_nlhe_translate_device(h, n, args, hands, pov, upto, recalls, play_edges, past, present, choices, n_choices, status)))
        return rc;
    return s.down();
}

}  // extern "C"

// ---- search matches (nlmc_search.hpp): NSM_CHUNK hands in flight, played in rounds; one synchronisation per round
namespace {
constexpr uint32_t NSM_MAX_ROUNDS = RP_NLHE_SEARCH_MAX_SOLVES + 2u;  // a hand parks once per solve, and ends in the round after its last
int nsm_check(const rp_nlhe_search_args* a, const void* steps, uint32_t* rollouts) {
    const char* name = "rp_nlhe_search_match";
    if (!a) return rp::fail(RP_ERR_INVALID, "%s: NULL args", name);
    int rc = nm_args_check(name, &a->match);
    if (rc) return rc;
    for (int s = 0; s < 2; ++s)  // both seats' kinds before either seat's fish, as the header orders them
        if (a->search[s] > (uint8_t)RP_SEARCH_WORLD) return rp::fail(RP_ERR_INVALID, "%s: search %u of seat %d is no rp_search_kind", name, a->search[s], s);
    for (int s = 0; s < 2; ++s)
        if (a->search[s] != 0u && a->match.agent[s] == (uint8_t)RP_AGENT_FISH) return rp::fail(RP_ERR_INVALID, "%s: seat %d is a fish: it reads no table to search from", name, s);
    if (a->origin_mode > 1u) return rp::fail(RP_ERR_INVALID, "%s: origin_mode %u above 1", name, a->origin_mode);
    if (a->visit_threshold == 0u) return rp::fail(RP_ERR_INVALID, "%s: visit_threshold must be at least 1", name);
    rp_nlhe_subgame_args sub{};
    sub.iterations = a->iterations, sub.rollouts = a->rollouts, sub.bias = a->bias, sub.prior = a->prior;
    if ((rc = nd_args_check(name, &sub, rollouts))) return rc;
    for (uint8_t r : a->reserved0)
        if (r != 0u) return rp::fail(RP_ERR_INVALID, "%s: reserved must be 0", name);
    if (a->steps_cap > 0u && !steps) return rp::fail(RP_ERR_INVALID, "%s: NULL steps with steps_cap > 0", name);
    return RP_OK;
}
// the grow-only scratch of a chunk, carved 16-byte aligned
struct NsmScratch {
    NsHand* hands;
    NsmLists lists;
    uint8_t* hole_world;
    float* weights;
    uint8_t* belief_status;
    rp_nlhe_subgame_result* results;
    size_t bytes;
    explicit NsmScratch(unsigned char* base) {
        size_t at = 0;
        auto take = [&](size_t b) {
            unsigned char* p = base ? base + at : nullptr;
            at += (b + 15) & ~(size_t)15;
            return p;
        };
        hands = reinterpret_cast<NsHand*>(take(sizeof(NsHand) * NSM_CHUNK));
        lists.recalls = reinterpret_cast<rp_nlhe_recall*>(take(sizeof(rp_nlhe_recall) * NSM_CHUNK));
        lists.entries = reinterpret_cast<rp_nlhe_frontier*>(take(sizeof(rp_nlhe_frontier) * NSM_CHUNK));
        lists.ids = reinterpret_cast<uint64_t*>(take(sizeof(uint64_t) * NSM_CHUNK));
        lists.origin = reinterpret_cast<int8_t*>(take(NSM_CHUNK));
        hole_world = take((size_t)RP_NLHE_MAX_HOLES * NSM_CHUNK);
        weights = reinterpret_cast<float*>(take(sizeof(float) * RP_NLHE_WORLDS * NSM_CHUNK));
        belief_status = take(NSM_CHUNK);
        results = reinterpret_cast<rp_nlhe_subgame_result*>(take(sizeof(rp_nlhe_subgame_result) * NSM_CHUNK));
        bytes = at;
    }
};
static_assert(NSM_CHUNK <= NS_CHUNK && NSM_CHUNK <= NR_CHUNK, "a round's solves of one seat are one launch of each kernel");
}  // namespace

extern "C" {

void rp_nlhe_search_args_default(rp_nlhe_search_args* out) {
    if (!out) return;
    *out = rp_nlhe_search_args{};
    rp_nlhe_match_args_default(&out->match);
    rp_nlhe_subgame_args sub;
    rp_nlhe_subgame_args_default(&sub);
    out->iterations = sub.iterations, out->rollouts = sub.rollouts, out->bias = sub.bias, out->prior = sub.prior;
    out->visit_threshold = 1u << 18;  // SubgameHyperParams::default
}

int rp_nlhe_search_match_device(rp_nlhe* h0, rp_nlhe* h1, uint64_t n, const rp_nlhe_search_args* args, rp_aivat_hand* hands, int16_t* won,
                                uint8_t* rejected, uint8_t* status, uint8_t* searched, uint8_t* unsolved, rp_nlhe_search_step* steps) {
    uint32_t rollouts = 0;
    int rc = nsm_check(args, steps, &rollouts);
    if (rc || n == 0) return rc;
    if (!h0) return rp::fail(RP_ERR_INVALID, "rp_nlhe_search_match: NULL handle");
    if ((rc = nm_pair_check("rp_nlhe_search_match", h0, h1))) return rc;
    if (!h1) h1 = h0;
    HIP_TRY(hipSetDevice(h0->device));
    hipStream_t st = rp::profile_stream(h0->prof);
    if ((rc = nm_after(st, rp::profile_stream(h1->prof)))) return rc;
    if (!h0->search_post) {
        void *hp_ = nullptr, *dp_ = nullptr;
        if (hipHostMalloc(&hp_, sizeof(NsmPost), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostGetDevicePointer(&dp_, hp_, 0) != hipSuccess) {
            if (hp_) (void)hipHostFree(hp_);
            return rp::fail(RP_ERR_HIP, "rp_nlhe_search_match: no pinned host memory for the rounds' counts");
        }
        memset(hp_, 0, sizeof(NsmPost));
        h0->search_post = reinterpret_cast<NsmPost*>(hp_);
        h0->search_post_dev = reinterpret_cast<NsmPost*>(dp_);
    }
    if ((rc = rp::grow(h0->search_scratch, h0->search_scratch_bytes, NsmScratch(nullptr).bytes, st))) return rc;
    const NsmScratch sc(static_cast<unsigned char*>(h0->search_scratch));
    const bool any_search = args->search[0] != 0u || args->search[1] != 0u;
    if (any_search) {  // the overflow rows of one launch's solves, as rp_nlhe_subgame_solve_device sizes them
        const size_t need = (size_t)std::min<uint64_t>(NSM_CHUNK, n) * NS_ROWS_OVF * sizeof(NdRow);
        if ((rc = rp::grow(h0->subgame_rows, h0->subgame_rows_bytes, need, st))) return rc;
    }
    rp_nlhe* seat[2] = {h0, h1};
    for (uint64_t at = 0; at < n; at += NSM_CHUNK) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(NSM_CHUNK, n - at);
        NsmArgs q{};
        q.match = nm_args(&args->match, at, m, hands, won, rejected, status);
        q.search[0] = args->search[0], q.search[1] = args->search[1];
        q.origin_mode = args->origin_mode;
        q.visit_threshold = args->visit_threshold;
        q.steps_cap = steps ? args->steps_cap : 0u;
        q.hands = sc.hands;
        q.searched = rp::from(searched, at);
        q.unsolved = rp::from(unsolved, at);
        q.steps = q.steps_cap ? steps + at * args->steps_cap : nullptr;
        q.results = sc.results;
        q.belief_status = sc.belief_status;
        bool finished = false;
        for (uint32_t round = 0; round < NSM_MAX_ROUNDS && !finished; ++round) {
            q.first = round == 0u ? 1u : 0u;
            hipLaunchKernelGGL(k_nl_search_advance, dim3((m + NM_BLOCK - 1u) / NM_BLOCK), dim3(NM_BLOCK), 0, st, h0->tab, h1->tab, h0->prm, q);
            HIP_TRY(hipGetLastError());
            if (!any_search) {  // no hand can park
                finished = true;
                break;
            }
            hipLaunchKernelGGL(k_nl_search_compact, dim3(1), dim3(NSM_SCAN), 0, st, sc.hands, m, sc.lists, h0->search_post_dev);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(st));  // the one wait of the round: how many solves it asks for
            const uint32_t count[2] = {h0->search_post->count[0], h0->search_post->count[1]};
            if (count[0] + count[1] > m) return rp::fail(RP_ERR_HIP, "rp_nlhe_search_match: %u + %u solves posted for %u hands", count[0], count[1], m);
            if (count[0] + count[1] == 0u) {
                finished = true;
                break;
            }
            for (uint32_t s = 0, lo = 0; s < 2u; lo += count[s], ++s) {
                if (count[s] == 0u) continue;
                NwArgs w{};
                w.recalls = sc.lists.recalls + lo;
                w.weights = sc.weights + (size_t)lo * RP_NLHE_WORLDS;
                w.hole_world = sc.hole_world + (size_t)lo * RP_NLHE_MAX_HOLES;
                w.status = sc.belief_status + lo;
                hipLaunchKernelGGL(k_nl_world, dim3(count[s]), dim3(NW_BLOCK), 0, st, seat[s]->tab, seat[s]->prm, w);
                HIP_TRY(hipGetLastError());
                NsArgs v{};
                v.entries = sc.lists.entries + lo;
                v.hole_world = w.hole_world;
                v.weights = w.weights;
                v.origin = args->origin_mode ? sc.lists.origin + lo : nullptr;
                v.iterations = args->iterations;
                v.rollouts = rollouts;
                v.bias = args->bias;
                v.prior = args->prior;
                v.step_hash_rollout = rp_node_hash_step(args->search_seed, 0);
                v.step_hash_deal = rp_node_hash_step(args->search_seed, 1);
                v.step_hash_tree = rp_node_hash_step(args->search_seed, 2);
                v.ids = sc.lists.ids + lo;
                v.overflow = static_cast<NdRow*>(h0->subgame_rows);
                v.results = sc.results + lo;
                hipLaunchKernelGGL(k_nl_subgame, dim3(count[s]), dim3(NS_BLOCK), 0, st, seat[s]->tab, seat[s]->prm, v);
                HIP_TRY(hipGetLastError());
            }
        }
        if (!finished) return rp::fail(RP_ERR_HIP, "rp_nlhe_search_match: hands still waiting for solves after %u rounds", NSM_MAX_ROUNDS);
    }
    HIP_TRY(hipStreamSynchronize(st));
    return RP_OK;
}

int rp_nlhe_search_match(rp_nlhe* h0, rp_nlhe* h1, uint64_t n, const rp_nlhe_search_args* args, rp_aivat_hand* hands, int16_t* won, uint8_t* rejected,
                         uint8_t* status, uint8_t* searched, uint8_t* unsolved, rp_nlhe_search_step* steps) {
    uint32_t rollouts = 0;
    int rc = nsm_check(args, steps, &rollouts);
    if (rc || n == 0) return rc;
    if (!h0) return rp::fail(RP_ERR_INVALID, "rp_nlhe_search_match: NULL handle");
    if ((rc = nm_pair_check("rp_nlhe_search_match", h0, h1))) return rc;
    rp::Stage s(h0->device, rp::profile_stream(h0->prof));
    s.out(hands, n).out(won, n).out(rejected, n).out(status, n).out(searched, n).out(unsolved, n).out(steps, n * args->steps_cap);
    if ((rc = s.up()) || (rc = rp_nlhe_search_match_device(h0, h1, n, args, hands, won, rejected, status, searched, unsolved, steps))) return rc;
    return s.down();
}

}  // extern "C"

// ---- the blueprint census (nlmc_census.hpp): one workgroup of three wavefronts per segment of the table, then one fold of the partials
namespace {
// f64 sums over the cells of streets [s0, s1), street then code ascending; extremes over the non-empty ones
struct NcSums {
    uint64_t rows = 0, visits = 0;
    double regret = 0.0, weight = 0.0, payoff = 0.0;
    float max_regret = 0.0f, min_regret = 0.0f, max_weight = 0.0f, max_payoff = 0.0f, min_payoff = 0.0f;
    uint32_t max_visits = 0, min_visits = 0;
};
NcSums nc_sums(const rp_census* c, uint32_t s0, uint32_t s1) {
    NcSums t;
    for (uint32_t s = s0; s < s1; ++s)
        for (uint32_t e = 0; e < RP_NLHE_CENSUS_CODES; ++e) {
            const rp_census_cell& q = c->cell[s][e];
            t.regret = t.regret + q.regret;
            t.weight = t.weight + q.weight;
            t.payoff = t.payoff + q.payoff;
            if (q.rows == 0) continue;
            if (t.rows == 0) {
                t.max_regret = q.max_regret, t.min_regret = q.min_regret, t.max_weight = q.max_weight;
                t.max_payoff = q.max_payoff, t.min_payoff = q.min_payoff, t.max_visits = q.max_visits, t.min_visits = q.min_visits;
            } else {
                t.max_regret = std::max(t.max_regret, q.max_regret), t.min_regret = std::min(t.min_regret, q.min_regret);
                t.max_weight = std::max(t.max_weight, q.max_weight);
                t.max_payoff = std::max(t.max_payoff, q.max_payoff), t.min_payoff = std::min(t.min_payoff, q.min_payoff);
                t.max_visits = std::max(t.max_visits, q.max_visits), t.min_visits = std::min(t.min_visits, q.min_visits);
            }
            t.rows += q.rows;
            t.visits += q.visits;
        }
    return t;
}
}  // namespace

extern "C" {

int rp_nlhe_table_census_device(rp_nlhe* h, rp_census* out) {
    if (!h || !out) return rp::fail(RP_ERR_INVALID, "rp_nlhe_table_census: NULL argument");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = rp::profile_stream(h->prof);
    const uint64_t slots = 1ull << h->cap_log2;
    const uint32_t nseg = (uint32_t)((slots + RP_NLHE_CENSUS_SEGMENT - 1u) / RP_NLHE_CENSUS_SEGMENT);
    int rc = rp::grow(h->census_scratch, h->census_scratch_bytes, nc_partial_bytes(nseg), st);
    if (rc) return rc;
    const NcPartials part = nc_partials(h->census_scratch, nseg);
    hipLaunchKernelGGL(k_nl_census_scan, dim3(nseg), dim3(NC_SCAN_BLOCK), 0, st, h->tab, nseg, part);
    hipLaunchKernelGGL(k_nl_census_fold, dim3(5), dim3(64), 0, st, part, nseg, rp::profile_epoch(h->prof), slots, out);
    HIP_TRY(hipGetLastError());
    return RP_OK;
}

int rp_nlhe_table_census(rp_nlhe* h, rp_census* out) {
    if (!h || !out) return rp::fail(RP_ERR_INVALID, "rp_nlhe_table_census: NULL argument");
    rp::Stage s(h->device, rp::profile_stream(h->prof));
    s.out(out, 1);
    int rc;
    if ((rc = s.up()) || (rc = rp_nlhe_table_census_device(h, out))) return rc;
    return s.down();
}

int rp_census_stats(const rp_census* c, rp_census_totals* out) {
    if (!c || !out) return rp::fail(RP_ERR_INVALID, "rp_census_stats: NULL argument");
    *out = rp_census_totals{};
    for (uint32_t s = 0; s < RP_NLHE_CENSUS_STREETS; ++s) out->infosets += c->infosets[s];
    const NcSums t = nc_sums(c, 0, RP_NLHE_CENSUS_STREETS);
    out->edges = t.rows;
    if (t.rows == 0) return RP_OK;
    const double n = (double)t.rows;
    out->avg_regret = (float)(t.regret / n), out->max_regret = t.max_regret, out->min_regret = t.min_regret;
    out->avg_weight = (float)(t.weight / n), out->max_weight = t.max_weight;
    out->avg_payoff = (float)(t.payoff / n), out->max_payoff = t.max_payoff, out->min_payoff = t.min_payoff;
    out->avg_visits = (float)((double)t.visits / n), out->max_visits = t.max_visits, out->min_visits = t.min_visits;
    return RP_OK;
}

int rp_census_street_stats(const rp_census* c, rp_census_street* out) {
    if (!c || !out) return rp::fail(RP_ERR_INVALID, "rp_census_street_stats: NULL argument");
    for (uint32_t s = 0; s < RP_NLHE_CENSUS_STREETS; ++s) {
        out[s] = rp_census_street{};
        out[s].street = "PFTR?"[s];
        out[s].infosets = c->infosets[s];
        const NcSums t = nc_sums(c, s, s + 1u);
        out[s].edges = t.rows;
        if (t.rows == 0) continue;
        const double n = (double)t.rows;
        out[s].avg_regret = (float)(t.regret / n), out[s].avg_weight = (float)(t.weight / n);
        out[s].avg_payoff = (float)(t.payoff / n), out[s].avg_visits = (float)((double)t.visits / n);
    }
    return RP_OK;
}

int rp_census_saturation(const rp_census* c, rp_census_peaks* out) {
    if (!c || !out) return rp::fail(RP_ERR_INVALID, "rp_census_saturation: NULL argument");
    *out = rp_census_peaks{};
    const NcSums t = nc_sums(c, 0, RP_NLHE_CENSUS_STREETS);
    out->precision_f32 = std::numeric_limits<float>::max();
    out->max_weight = t.max_weight;
    out->max_regret = std::max(std::fabs(t.max_regret), std::fabs(t.min_regret));
    out->max_payoff = std::max(std::fabs(t.max_payoff), std::fabs(t.min_payoff));
    out->max_visits = t.max_visits;
    out->weight_pct = out->max_weight / out->precision_f32 * 100.0f;
    out->regret_pct = out->max_regret / out->precision_f32 * 100.0f;
    return RP_OK;
}

int rp_census_grid_usage(const rp_census* c, rp_census_grid* rows, uint32_t* n) {
    if (!c || !rows || !n) return rp::fail(RP_ERR_INVALID, "rp_census_grid_usage: NULL argument");
    uint32_t k = 0;
    bool rated[NC_CELLS];
    for (uint32_t s = 0; s < RP_NLHE_CENSUS_STREETS; ++s) {
        const uint32_t first = k;
        for (uint32_t e = 0; e < RP_NLHE_CENSUS_CODES; ++e) {
            const rp_census_cell& q = c->cell[s][e];
            if (q.rows == 0) continue;
            rp_census_grid g{};
            g.street = (uint8_t)s, g.edge = (uint8_t)e;
            g.avg_freq = q.rated ? (float)(q.ratio / (double)q.rated) : 0.0f;
            g.weighted_freq = q.total != 0.0 ? (float)(q.weight / q.total) : 0.0f;
            g.n_decisions_with_edge = q.rows, g.n_dominant = q.dominant;
            // insertion behind every row of the street that does not rank behind it (codes arrive ascending: ties keep code order)
            uint32_t at = k;
            while (at > first && ((q.rated != 0 && !rated[at - 1]) || (q.rated != 0 && rated[at - 1] && rows[at - 1].avg_freq < g.avg_freq))) {
                rows[at] = rows[at - 1];
                rated[at] = rated[at - 1];
                at -= 1;
            }
            rows[at] = g;
            rated[at] = q.rated != 0;
            k += 1;
        }
    }
    *n = k;
    return RP_OK;
}

}  // extern "C"

// ---- the table itself (nlmc_table.hpp): compaction, bulk insertion, rehash into another size, growth in front of a step
namespace {
int nl_keys(rp_nlhe* h, uint64_t* keys) {
    if (!h->keys_valid) {
        hipStream_t st = rp::profile_stream(h->prof);
        unsigned int k = 0;
        HIP_TRY(hipMemcpyAsync(&k, h->tab.n_keys, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        h->keys = k;
        h->keys_valid = true;
    }
    *keys = h->keys;
    return RP_OK;
}
// every key a step inserts belongs to a decision node it grew, and a step that stays within one pass grows at most the 1 536 nodes
// per tree the header names as its budget
uint64_t nl_default_headroom(const rp_nlhe* h) { return (uint64_t)h->batch * 1536u; }
uint32_t nt_blocks(const rp_nlhe* h, uint64_t lanes) {
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((lanes + NT_BLOCK - 1u) / NT_BLOCK, 1u), h->grid_cap);
}
// The handle moves onto a fresh table of 2^new_log2 slots.  Like rp::grow's regions, the old arrays may still be read by launches
// queued earlier, and the rehash itself reads them: they are freed only after the stream has passed the rehash.
int nl_resize(rp_nlhe* h, uint32_t new_log2) {
    if (new_log2 == h->cap_log2) return RP_OK;
    uint64_t keys = 0;
    int rc = nl_keys(h, &keys);
    if (rc) return rc;
    const uint64_t slots = 1ull << new_log2;
    if (2u * keys > slots)
        return rp::fail(RP_ERR_CAPACITY, "rp_nlhe_resize: %llu infosets do not fit 2^%u slots at a fill of one half", (unsigned long long)keys, new_log2);
    hipStream_t st = rp::profile_stream(h->prof);
    NlTable to{};
    to.mask = (uint32_t)(slots - 1u);
    void *p_slots = nullptr, *p_keys = nullptr, *p_rows = nullptr;
    const size_t row_bytes = (size_t)slots * 4u * NLMC_A * sizeof(float);
    hipError_t e = hipMalloc(&p_slots, (size_t)slots * sizeof(NlSlot));
    if (e == hipSuccess) e = hipMalloc(&p_keys, 8);  // the key count and, behind it, the rehash's error flags
    if (e == hipSuccess) e = hipMalloc(&p_rows, row_bytes);
    // a fresh table: empty slots, zero rows (the NLHE profile's default regrets are written by the insertion, not by the table)
    if (e == hipSuccess) e = hipMemsetAsync(p_slots, 0, (size_t)slots * sizeof(NlSlot), st);
    if (e == hipSuccess) e = hipMemsetAsync(p_keys, 0, 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(p_rows, 0, row_bytes, st);
    uint32_t err = 0;
    if (e == hipSuccess) {
        to.slots = static_cast<NlSlot*>(p_slots);
        to.n_keys = static_cast<unsigned int*>(p_keys);
        to.rows = static_cast<float*>(p_rows);
        hipLaunchKernelGGL(k_nl_table_rehash, dim3(nt_blocks(h, (uint64_t)h->tab.mask + 1u)), dim3(NT_BLOCK), 0, st, h->tab, to, to.n_keys + 1);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&err, to.n_keys + 1, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess || err) {  // the handle stays on its old table
        (void)hipStreamSynchronize(st);
        for (void* p : {p_slots, p_keys, p_rows})
            if (p) (void)hipFree(p);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return rp::fail(RP_ERR_HIP, "rp_nlhe_resize: %s (a table of 2^%u slots needs %llu bytes beside the one in use)", hipGetErrorString(e),
                            new_log2, (unsigned long long)(slots * 176u));
        }
        return rp::fail(RP_ERR_CAPACITY, "rp_nlhe_resize: the new table filled up (flags %u)", err);
    }
    void *old_slots = h->tab.slots, *old_keys = h->tab.n_keys;
    void* old_rows = rp::profile_swap_table(h->prof, to.rows, slots);
    h->allocs.erase(std::remove_if(h->allocs.begin(), h->allocs.end(), [&](void* p) { return p == old_slots || p == old_keys; }), h->allocs.end());
    h->allocs.push_back(p_slots);
    h->allocs.push_back(p_keys);
    h->tab = to;
    h->cap_log2 = new_log2;
    for (void* p : {old_slots, old_keys, old_rows}) (void)hipFree(p);  // the stream has passed the rehash (synchronised above)
    return RP_OK;
}
int nl_grow_table(rp_nlhe* h, uint64_t headroom) {
    if (!h->grow_max || h->cap_log2 >= h->grow_max) return RP_OK;
    uint64_t keys = 0;
    int rc = nl_keys(h, &keys);
    if (rc) return rc;
    uint32_t want = h->cap_log2;
    while (2u * (keys + headroom) > (1ull << want) && want < h->grow_max) want += 1;
    return nl_resize(h, want);  // the doublings in one rehash
}
}  // namespace

extern "C" {

int rp_nlhe_capacity(rp_nlhe* h, uint32_t* cap_log2, uint64_t* keys) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_capacity: NULL handle");
    if (cap_log2) *cap_log2 = h->cap_log2;
    if (!keys) return RP_OK;
    HIP_TRY(hipSetDevice(h->device));
    return nl_keys(h, keys);
}

int rp_nlhe_resize(rp_nlhe* h, uint32_t new_cap_log2) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_resize: NULL handle");
    if (new_cap_log2 < 8 || new_cap_log2 > 30) return rp::fail(RP_ERR_INVALID, "rp_nlhe_resize: cap_log2 %u outside 8..30", new_cap_log2);
    HIP_TRY(hipSetDevice(h->device));
    return nl_resize(h, new_cap_log2);
}

int rp_nlhe_set_growth(rp_nlhe* h, uint32_t max_cap_log2, uint64_t headroom) {
    if (!h) return rp::fail(RP_ERR_INVALID, "rp_nlhe_set_growth: NULL handle");
    if (max_cap_log2 != 0 && (max_cap_log2 < h->cap_log2 || max_cap_log2 > 30))
        return rp::fail(RP_ERR_INVALID, "rp_nlhe_set_growth: max_cap_log2 %u outside %u..30 (0 switches growth off)", max_cap_log2, h->cap_log2);
    h->grow_max = max_cap_log2;
    h->grow_headroom = headroom;
    return RP_OK;
}

int rp_nlhe_export_device(rp_nlhe* h, uint64_t cap, uint64_t* n, uint64_t* past_dev, uint32_t* present_dev, uint64_t* choices_dev,
                          rp_encounter* enc_dev) {
    if (!h || !n) return rp::fail(RP_ERR_INVALID, "rp_nlhe_export_device: NULL argument");
    if ((uintptr_t)enc_dev % 16u) return rp::fail(RP_ERR_INVALID, "rp_nlhe_export_device: enc_dev is not 16-byte aligned");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = rp::profile_stream(h->prof);
    const uint64_t slots = 1ull << h->cap_log2;
    const uint32_t nseg = (uint32_t)((slots + NT_SEGMENT - 1u) / NT_SEGMENT);
    // [counts nseg][offsets nseg][total, pad][the scan's scratch]
    const size_t words = (size_t)2 * nseg + 2;
    int rc = rp::grow(h->table_scratch, h->table_scratch_bytes, words * 4u + rp::ss::scan_scratch_bytes(nseg), st);
    if (rc) return rc;
    uint32_t* seg_count = static_cast<uint32_t*>(h->table_scratch);
    uint32_t *seg_off = seg_count + nseg, *total = seg_off + nseg;
    const dim3 grid(nt_blocks(h, (uint64_t)nseg * 64u));
    hipLaunchKernelGGL(k_nl_table_count, grid, dim3(NT_BLOCK), 0, st, h->tab, nseg, seg_count);
    HIP_TRY(rp::ss::exclusive_scan<uint32_t>(seg_count, seg_off, nseg, total + 2, st, total));
    if (cap && past_dev && present_dev && choices_dev && enc_dev)
        hipLaunchKernelGGL(k_nl_table_compact, grid, dim3(NT_BLOCK), 0, st, h->tab, nseg, seg_off, cap, past_dev, present_dev, choices_dev, enc_dev);
    HIP_TRY(hipGetLastError());
    uint32_t found = 0;
    HIP_TRY(hipMemcpyAsync(&found, total, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n = found;
    return RP_OK;
}

int rp_nlhe_import_device(rp_nlhe* h, uint64_t n, const uint64_t* past_dev, const uint32_t* present_dev, const uint64_t* choices_dev,
                          const rp_encounter* enc_dev, uint64_t epoch) {
    if (!h || (n && (!past_dev || !present_dev || !choices_dev || !enc_dev))) return rp::fail(RP_ERR_INVALID, "rp_nlhe_import_device: NULL argument");
    if ((uintptr_t)enc_dev % 16u) return rp::fail(RP_ERR_INVALID, "rp_nlhe_import_device: enc_dev is not 16-byte aligned");
    if (n == 0) return rp_profile_set_epoch(h->prof, epoch);
    HIP_TRY(hipSetDevice(h->device));
    int rc = h->grow_max ? nl_grow_table(h, n) : RP_OK;
    if (rc) return rc;
    hipStream_t st = rp::profile_stream(h->prof);
    // items per pair of launches: a claim is the item's index in its chunk + 1 in 32 bits.  RP_NLHE_IMPORT_CHUNK (tests): a smaller one.
    uint64_t chunk = 1ull << 26;
    if (const char* env = getenv("RP_NLHE_IMPORT_CHUNK")) chunk = (uint64_t)std::min(1 << 26, std::max(1, atoi(env)));
    chunk = std::min(chunk, n);
    if ((rc = rp::grow(h->table_scratch, h->table_scratch_bytes, (size_t)(chunk + 2u) * 4u, st))) return rc;
    uint32_t* rows = static_cast<uint32_t*>(h->table_scratch);
    uint32_t* flags = rows + chunk;  // [0] error flags, [1] unused
    HIP_TRY(hipMemsetAsync(flags, 0, 8, st));
    h->keys_valid = false;
    rc = rp::chunks(n, chunk, [&](uint64_t at, uint32_t m) {
        const dim3 grid(nt_blocks(h, m));
        hipLaunchKernelGGL(k_nl_table_find, grid, dim3(NT_BLOCK), 0, st, h->tab, m, past_dev + at, present_dev + at, choices_dev + at, rows, flags);
        hipLaunchKernelGGL(k_nl_table_write, grid, dim3(NT_BLOCK), 0, st, h->tab, m, rows, enc_dev + at * NLMC_A);
    });
    if (rc) return rc;
    uint32_t err = 0;
    unsigned int keys = 0;
    HIP_TRY(hipMemcpyAsync(&err, flags, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&keys, h->tab.n_keys, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    h->keys = keys;
    h->keys_valid = true;
    if (err) return rp::fail(RP_ERR_CAPACITY, "rp_nlhe_import_device: infoset table full (flags %u; the keys inserted before it stay)", err);
    return rp_profile_set_epoch(h->prof, epoch);
}

}  // extern "C"
