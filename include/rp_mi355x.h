/* rp_mi355x.h — C ABI of librp_mi355x.so: robopoker's two numeric hot paths on MI355X (gfx950).
 *
 * The reference (krukah/robopoker, Rust) has NO FFI seam for these paths: they sit behind
 * Rust traits with default methods.  This header IS the seam: every entry
 * point names the reference trait item it replaces so a thin Rust shim can implement
 * `mccfr::Solver` / `elkan::Elkan` / `monge::Coupling` by delegation (INTEGRATION.md shows
 * the binding).  Conventions kept from the reference: values are plain-old-data, the batch
 * (tree sampling + regret vectors) is pure w.r.t. the profile and the table mutation happens
 * afterwards in tree-id order; no Result on the hot path — here every call returns an
 * `rp_status` (0 = ok) and never unwinds across the boundary.
 *
 * All handles are opaque.  All buffers are caller-owned flat arrays.  `device` is a HIP
 * device ordinal; there is NO CPU fallback in this library: a call that needs the GPU on a
 * machine without one returns RP_ERR_NO_DEVICE.
 *
 * Arithmetic (exp/ln/pow, RNG, summation orders) is specified in rp_math.h and DESIGN.md.
 *
 * COMPILED LIMITS (a call outside them fails with RP_ERR_INVALID / RP_ERR_CAPACITY / RP_ERR_UNSUPPORTED, never silently):
 *   mccfr    max_actions <= 16 (RP_MAX_ACTIONS); a sampled tree has < 255 nodes (rp_game_table.max_tree_nodes) and each tree
 *            emits at most 255 Decisions.  Games with <= 62 nodes per sampled tree, depth <= 10, <= 32 internal nodes and
 *            <= 8191 infosets (Kuhn, Leduc, RPS, the wide Leduc) take the LDS-resident traversal; larger ones its HBM-scratch
 *            variant.  NLHE-sized trees (10^3-10^4 nodes) are NOT reachable through rp_game_table: see rp_nlhe_* below.
 *   profile  (rp_profile_*) max_actions <= 16, rows < 2^32, Decisions per batch < 2^31.
 *   nlhe     (rp_nlhe_*) 2 players, stacks of 200 chips; at most 9 choices per infoset; a batch's trees together may hold
 *            1 536 nodes per tree on average (92 B each) per PASS (a batch that needs more is split into passes automatically)
 *            and 160 Decisions per tree on average, one tree at most 48 levels,
 *            65 535 nodes and 2 048 walker nodes; the infoset table holds 2^cap_log2 rows (a full table fails the step).
 *   lloyd    K <= 256 and bins <= 256 (an Abstraction index is 8 bits, kicker/src/abstraction.rs:22-23), counts are u8
 *            (a point's mass per bin <= 255; the flop / turn layers have mass 47 / 46), N < 2^32.  The MFMA bound prunes
 *            points with 1..64 support bins; others go through the unpruned kernels.
 *   sampling Discounted / Asymmetric regret have a sign-dependent discount: ordered update only (composed, sharded and
 *            windowed steps return RP_ERR_UNSUPPORTED).
 */
#ifndef RP_MI355X_H
#define RP_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RP_API __attribute__((visibility("default")))

typedef enum rp_status {
    RP_OK = 0,
    RP_ERR_INVALID = 1,     /* bad argument / inconsistent table                */
    RP_ERR_NO_DEVICE = 2,   /* no HIP device (the product path has no CPU mode) */
    RP_ERR_HIP = 3,         /* a HIP runtime call failed (see rp_last_error)    */
    RP_ERR_UNSUPPORTED = 4, /* combination not implemented on the device path   */
    RP_ERR_CAPACITY = 5,    /* game exceeds the compiled per-tree limits        */
    RP_ERR_INTERNAL = 6     /* a self-check of the library failed (rp_last_error) */
} rp_status;

/* human-readable text of the last failure on the calling thread */
RP_API const char* rp_last_error(void);
/* Diagnostics — device self tests, HIP-event kernel clocks, traversal shape and census, the MFMA bound's intervals — are declared in
 * rp_mi355x_diag.h (same library, same conventions): what tests and bench.py call, nothing a drop-in caller needs. */
/* number of visible HIP devices (0 when there is none); never fails */
RP_API int rp_device_count(void);
/* library build info: "rp_mi355x <version> gfx950 hip <ver>" */
RP_API const char* rp_version(void);

/* ======================================================================= mccfr ==
 * crates/mccfr: Solver (solver/solver.rs:38-351), RefProf/MutProf/CfrSampling
 * (strategy/{profile.rs:12-29,storage.rs:9-18,training.rs:10-30}), schedules
 * (regret/mod.rs:18-29, policy/mod.rs:18-25), samplers (sample/mod.rs:53-65).
 */

/* RegretSchedule impls: regret/{summed,linear,discounted,floored,asymmetric}.rs */
typedef enum rp_regret_kind {
    RP_REGRET_SUMMED = 0,
    RP_REGRET_LINEAR = 1,
    RP_REGRET_DISCOUNTED = 2,
    RP_REGRET_FLOORED = 3,
    RP_REGRET_ASYMMETRIC = 4
} rp_regret_kind;

/* WeightSchedule impls: policy/{constant,linear,quadratic,exponential}.rs */
typedef enum rp_weight_kind {
    RP_WEIGHT_CONSTANT = 0,
    RP_WEIGHT_LINEAR = 1,
    RP_WEIGHT_QUADRATIC = 2,
    RP_WEIGHT_EXPONENTIAL = 3
} rp_weight_kind;

/* SamplingScheme impls: sample/{external,pruning,pluribus}.rs */
typedef enum rp_sampling_kind {
    RP_SAMPLING_EXTERNAL = 0,
    RP_SAMPLING_PRUNABLE = 1,
    RP_SAMPLING_PLURIBUS = 2
} rp_sampling_kind;

/* hyperparams/{sampling.rs:39-50, pruning.rs:36-53, training.rs:49-60}; rp_hyper_default() fills the
 * reference defaults {tau 1.0, beta 2.0, eps 0.05, threshold -3e5, explore 0.05, warmup 16384, regret_min -4e6}. */
typedef struct rp_hyper {
    float temperature;
    float smoothing;
    float curiosity;
    float prune_threshold;
    float prune_explore;
    uint64_t prune_warmup;
    float regret_min;
    uint32_t _pad;
} rp_hyper;
RP_API void rp_hyper_default(rp_hyper* out);

/* Encounter: solver/encounter.rs:22-27 (16-byte AoS at the boundary; SoA by field in HBM) */
typedef struct rp_encounter {
    float weight;
    float regret;
    float payoff;
    uint32_t visits;
} rp_encounter;

/* Flat description of an extensive-form game: the boundary's answer to "games are Rust generics"
 * (CfrGame/CfrTurn/CfrEdge/CfrInfo/CfrEncoder; kuhn/src/game.rs:115-167, leduc/src/game.rs:177-245).
 * A state is a node of the full game tree; children of a player state are listed in `choices()` order
 * (kuhn/src/info.rs:36-42, leduc/src/info.rs:29-35), children of a chance state in deal order. */
#define RP_TURN_CHANCE 254u
#define RP_TURN_TERMINAL 255u
#define RP_NO_INFO 0xffffffffu
typedef struct rp_state {
    uint8_t turn;       /* acting player 0..n_players-1, RP_TURN_CHANCE or RP_TURN_TERMINAL */
    uint8_t n_children; /* branching factor (0 for terminals), at most 16 (RP_MAX_ACTIONS) at player AND chance states: the
                           traversals keep the taken edge in 4 bits.  A wider deal is split into two chance levels, as the
                           built-in games deal their two private cards; rp_game_table_check answers RP_ERR_CAPACITY otherwise */
    uint16_t chance_info; /* chance states, reference-seed mode only: 1 + index of the node's info among rp_hash_streams.chance;
                             0 = this chance state has no counterpart in the reference's trees (the root deal, which the
                             reference takes from the thread RNG, kuhn/src/game.rs:115-123) and keeps the counter hash.
                             Was `reserved` before 0.4: a caller that builds its own rp_game_table MUST zero it unless it hands
                             hash streams to rp_mccfr_set_rng (a stray value in range selects the wrong chance stream)       */
    uint32_t info;      /* infoset id at player states, RP_NO_INFO otherwise                  */
    uint32_t offset;    /* player/chance: first child in children[]; terminal: row in payoffs */
} rp_state;

typedef struct rp_game_table {
    uint32_t n_states;
    uint32_t n_infos;
    uint32_t n_players;
    uint32_t max_actions;  /* A: row stride of the regret/strategy tables          */
    uint32_t n_children;   /* length of children[]                                  */
    uint32_t n_terminals;  /* rows of payoffs[]                                     */
    uint32_t train_root;   /* CfrGame::root(): chance over deals -> first decision  */
    uint32_t exploit_root; /* CfrGame::exploitability_root()                        */
    uint32_t max_depth;    /* longest root->leaf path (states) from either root; may be overstated, never understated */
    uint32_t max_tree_nodes; /* bound on nodes of one externally-sampled tree from train_root (walker states keep every
                                child, all others one; maximum over the walkers); may be overstated, never understated */
    const rp_state* states;
    const uint32_t* children;
    const float* payoffs;          /* [n_terminals][n_players]                       */
    const uint8_t* info_actions;   /* [n_infos] number of choices()                  */
    const uint8_t* info_player;    /* [n_infos] acting player                        */
    const float* default_regret;   /* [n_infos][max_actions] or NULL (= 0): CfrEdge::default_regret */
} rp_game_table;

/* Built-in game models (crates/kuhn, crates/leduc, crates/roshambo), owned by the library. */
/* RP_GAME_LEDUC_WIDE is synthetic (not a reference game): Leduc's rules over seven ranks, 616 infosets — it exists to
 * exercise the large-game kernels (more than 256 infosets) with a game the oracle can also play */
typedef enum rp_game_kind { RP_GAME_KUHN = 0, RP_GAME_LEDUC = 1, RP_GAME_RPS = 2, RP_GAME_LEDUC_WIDE = 3 } rp_game_kind;
typedef struct rp_game rp_game;
RP_API int rp_game_create(rp_game_kind kind, rp_game** out);
RP_API int rp_game_view(const rp_game* g, rp_game_table* out); /* pointers valid until destroy */
RP_API int rp_game_destroy(rp_game* g);
/* Named infoset lookup for the built-in games, e.g. "K|XB" (Kuhn: rank|history, kuhn/src/info.rs:58-66)
 * or "Q|K|XRC|R" (Leduc: rank|board|round1|round2). Returns RP_ERR_INVALID when unknown. */
RP_API int rp_game_info_id(const rp_game* g, const char* name, uint32_t* out);
RP_API int rp_game_info_name(const rp_game* g, uint32_t info, char* buf, size_t cap);
/* Validation of a caller-built table, on the host; rp_mccfr_create runs it first.  RP_ERR_INVALID: NULL fields, n_players
 * outside 1..8, max_actions outside 1..16, roots or offsets out of range, a child that does not follow its parent in states[],
 * a player state whose infoset is out of range or disagrees with it in acting player or action count, max_depth or
 * max_tree_nodes below what the table itself yields.  RP_ERR_CAPACITY: a state with more than 16 children (well formed, but
 * the kernels cannot hold it).  NOT checked: perfect recall — that an infoset never occurs twice on one root-to-leaf path is
 * the caller's to guarantee. */
RP_API int rp_game_table_check(const rp_game_table* t);

typedef struct rp_mccfr rp_mccfr;

/* ---- which generator draws the sampled branches ------------------------------------------------------------------------------
 * RP_RNG_COUNTER (default): one 64-bit counter hash per (seed, epoch, tree, infoset), include/rp_math.h rp_node_hash — the
 *   build's own definition, cheap on the device.
 * RP_RNG_REFERENCE ("reference-seed" mode): the reference's own chain, restated from the published algorithms in
 *   include/rp_refrng.h: DefaultHasher (SipHash-1-3, zero key) over t.hash(), info.hash(), node.seed().hash()
 *   (crates/mccfr/src/strategy/flow.rs:285-295) -> SmallRng::seed_from_u64 (xoshiro256++) -> one draw: WeightedIndex<f32> at an
 *   opponent node (sample/external.rs:41-64), random_range(0..n) at a chance node (sample/mod.rs:68-82), random::<f32>() for
 *   Pluribus' exploration coin (sample/pluribus.rs:91).  `t` = the epoch, node.seed() = the tree's index in the batch
 *   (solver.rs: the par_iter index), info.hash() = the byte stream the caller's `impl Hash for I` writes, handed over once as
 *   rp_hash_streams (INTEGRATION.md shows the ten-line recording Hasher that produces it from any CfrInfo).  The library's
 *   `seed` then only enters the root deal, which the reference leaves to the unseeded thread RNG. */
typedef enum rp_rng_kind { RP_RNG_COUNTER = 0, RP_RNG_REFERENCE = 1 } rp_rng_kind;
#define RP_HASH_STREAM_MAX 55u
typedef struct rp_hash_stream {
    uint8_t len;                       /* bytes written by I::hash                          */
    uint8_t bytes[RP_HASH_STREAM_MAX]; /* in write order                                    */
} rp_hash_stream;
typedef struct rp_hash_streams {
    uint32_t n_infos;              /* = rp_game_table.n_infos                                     */
    uint32_t n_chance;             /* distinct infos of in-tree chance nodes                      */
    const rp_hash_stream* infos;   /* [n_infos]                                                   */
    const rp_hash_stream* chance;  /* [n_chance], indexed by rp_state.chance_info - 1             */
} rp_hash_streams;
/* the streams of a built-in game (kuhn/src/info.rs:20-24,71; leduc/src/info.rs:11-17,85; roshambo/src/turn.rs:10-18) */
RP_API int rp_game_hash_streams(const rp_game* g, rp_hash_streams* out); /* pointers valid until destroy */
RP_API int rp_mccfr_set_rng(rp_mccfr* h, rp_rng_kind kind, const rp_hash_streams* streams /* NULL for RP_RNG_COUNTER */);

typedef enum rp_update_mode {
    RP_UPDATE_ORDERED = 0, /* per-key sequential application in tree-id order: solver.rs:96-105 exactly */
    RP_UPDATE_COMPOSED = 1 /* per-key composed (a,b,floor) maps; used for the multi-GPU exchange         */
} rp_update_mode;
/* WHICH MODE TO USE.  ORDERED is the reference's arithmetic bit for bit and the default of rp_mccfr_create (a drop-in caller
 * gets the reference's numbers); it is a serial chain per table cell: 0.35 G infoset-updates/s on Leduc.  COMPOSED re-associates
 * the same touches (tables within rtol 1e-4 per step of ORDERED, the "stated fp32 tolerance" of the build's north star), runs
 * 100x faster (36 G/s) and is the only mode that shards across GPUs — it is the mode bench.py's headline `value` is measured in
 * (`other_update_mode` in the same line quotes ORDERED).  Select it at creation with rp_mccfr_create_mode, or later with
 * rp_mccfr_set_update_mode.  Discounted / Asymmetric regret (sign-dependent discount) exist in ORDERED only. */

/* Composed update: a BLOCK is the set of Decisions of one infoset produced by one chunk of RP_COMPOSE_CHUNK
 * consecutive trees (of this rank); it is composed sequentially, in tree-id order, from the identity into a map
 * F(x) = max(a x + b, m) per table cell; the blocks of an infoset are then folded in chunk order and the result is
 * applied to the table (rank by rank in the multi-GPU exchange).  Exact in real arithmetic; in f32 it is a fixed
 * re-association of the reference's sequential update (tests state the tolerance). */
#define RP_COMPOSE_CHUNK 256u
/* The block maps of a cell are folded sequentially inside groups of RP_FOLD_GROUP consecutive blocks, the group maps
 * sequentially into the cell's map: a fixed two-level shape, so that the groups of a hot infoset (or hot row of the
 * sparse profile) fold in parallel on the device and the oracle can restate the association exactly. */
#define RP_FOLD_GROUP 64u

/* mccfr!(Prefix, Encoder, T, E, G, I, batch) + <R, W, S> (strategy/macros.rs:7-151): one solver instance.
 * `batch_size` = Solver::batch_size() (trees per step). */
RP_API int rp_mccfr_create(const rp_game_table* game, rp_regret_kind r, rp_weight_kind w, rp_sampling_kind s,
                           uint32_t batch_size, const rp_hyper* hp, uint64_t seed, int device, rp_mccfr** out);
RP_API int rp_mccfr_create_mode(const rp_game_table* game, rp_regret_kind r, rp_weight_kind w, rp_sampling_kind s,
                                uint32_t batch_size, const rp_hyper* hp, uint64_t seed, int device, rp_update_mode mode,
                                rp_mccfr** out);
RP_API int rp_mccfr_destroy(rp_mccfr* h);
/* Solver::step (solver.rs:96-105): batch() then update_{regret,weight,payoff,visits} then epoch += 1 */
RP_API int rp_mccfr_step(rp_mccfr* h);
/* Solver::solve (solver.rs:111-122): trees / batch_size steps */
RP_API int rp_mccfr_solve(rp_mccfr* h, uint64_t trees);
/* Solver::spend (solver.rs:130-137) */
RP_API int rp_mccfr_spend(rp_mccfr* h, double seconds, uint64_t* iterations, double* elapsed);
/* Trainer::train (crates/forge/src/trainer.rs:18-66) over this solver: loop { step; checkpoint; flush; interrupt? }.
 * A checkpoint fires when `log_interval` seconds passed since the last one (Metrics::checkpoint, mccfr/src/metrics/
 * mod.rs:67-80: rate = new infos / max(1, whole seconds)); its line is Checkpoint's Display (metrics/checkpoint.rs:
 * 39-50): "batch E", "nodes N", "infos I", "I/sec R.R", each left-aligned in 20 columns.  A flush event fires every
 * `flush_interval` seconds (TrainingHyperParams defaults: 60 s and 30 min, hyperparams/training.rs:50-54); the
 * callback may export the table there (rp_mccfr_export).  The loop ends when *interrupt becomes non-zero
 * (pokerkit::interrupted), after max_steps (0 = unbounded) or max_seconds (<= 0 = unbounded); `summary` receives
 * Progress::summary (progress.rs:24-26).  Counters are read from the device only when a checkpoint is due. */
typedef struct rp_checkpoint { uint64_t epoch, nodes, infos; double rate; } rp_checkpoint;
typedef enum rp_train_event { RP_TRAIN_CHECKPOINT = 0, RP_TRAIN_FLUSH = 1 } rp_train_event;
typedef void (*rp_train_event_fn)(int event, const rp_checkpoint* cp, const char* line, void* user);
RP_API int rp_mccfr_train(rp_mccfr* h, uint64_t max_steps, double max_seconds, double log_interval,
                          double flush_interval, rp_train_event_fn on_event, void* user,
                          const volatile int* interrupt, char* summary, size_t summary_cap);
/* enqueue `steps` steps on the stream without host synchronisation (FastSession::step loop shape) */
RP_API int rp_mccfr_step_async(rp_mccfr* h, uint32_t steps);
RP_API int rp_mccfr_sync(rp_mccfr* h);
/* RefProf::t (profile.rs:14) */
RP_API int rp_mccfr_epoch(rp_mccfr* h, uint64_t* epoch);
/* Metrics nodes / infos counters (metrics/mod.rs:21-80; infos = the "infoset-updates" unit, solver.rs:273) */
RP_API int rp_mccfr_counters(rp_mccfr* h, uint64_t* nodes, uint64_t* infos);
/* RefProf::cum_{weight,regret,payoff,visits} / MutProf::mut_* (profile.rs:16-23, storage.rs:9-18) */
RP_API int rp_mccfr_get(rp_mccfr* h, uint32_t info, uint32_t edge, rp_encounter* out);
RP_API int rp_mccfr_set(rp_mccfr* h, uint32_t info, uint32_t edge, const rp_encounter* in);
/* CfrData::encounters_ref / hydrate (book.rs:14-24, nlhe/src/profile.rs:97-163): rows[n_infos*max_actions] */
RP_API int rp_mccfr_export(rp_mccfr* h, rp_encounter* rows, uint64_t cap);
RP_API int rp_mccfr_import(rp_mccfr* h, const rp_encounter* rows, uint64_t n, uint64_t epoch);
typedef enum rp_dist_kind {
    RP_DIST_ITERATED = 0, /* RefProf::iterated_distribution (profile.rs:47-51) */
    RP_DIST_AVERAGED = 1, /* RefProf::averaged_distribution (profile.rs:40-44) */
    RP_DIST_SAMPLING = 2  /* CfrFlow::sampling_distribution (flow.rs:33-42)    */
} rp_dist_kind;
RP_API int rp_mccfr_policy(rp_mccfr* h, uint32_t info, rp_dist_kind kind, float* out, uint32_t* n);
/* Solver::exploitability (solver.rs:327-337) -> CfrNash::exploitability (nash.rs:31-38); host-side validation */
RP_API int rp_mccfr_exploitability(rp_mccfr* h, float* out);
/* ---- the same best response on the DEVICE (csrc/mccfr_nash.hpp): exploitability as a stopping rule -----------------------------
 * CfrNash::exploitability restated as kernels over the expanded tree from exploit_root; every result below is bit for bit what
 * rp_mccfr_exploitability computes on the host, which stays as the independent cross-check.  The expanded tree (one 16-byte record
 * per node, its kids, the nodes by depth level, every infoset's nodes) is built on the host by the FIRST of these calls on a handle,
 * uploaded once (that call synchronises) and kept until rp_mccfr_destroy: a handle that never asks pays nothing.  Limits: a tree of
 * more than 2^24 nodes, or one whose arrays the device cannot hold (28 bytes per node + 4 per node and player), is RP_ERR_CAPACITY.
 * Refused before a device is needed, rp_last_error naming the argument: NULL h, NULL out_dev / out, check_every == 0, a NaN target.
 * A sharded handle (world > 1) is served like any other: the tables are replicas. */
/* queued on the handle's stream, no host synchronisation; *out_dev (DEVICE memory) is written in stream order, so it reads the tables
 * as every earlier step on this stream left them */
RP_API int rp_mccfr_exploitability_device(rp_mccfr* h, float* out_dev);
/* the same computation with its parts, to HOST memory (synchronises); any output may be NULL:
 * values[n_players] = optimal_response_payoff per hero, choice[n_infos] = optimal_cfactual_choice (the action slot),
 * cfv[n_infos][max_actions] = optimal_cfactual_payoff (slots past the infoset's actions are 0) */
RP_API int rp_mccfr_best_response(rp_mccfr* h, float* exploitability, float* values, uint8_t* choice, float* cfv);
/* 0 = one launch, one workgroup per hero, LDS; 1 = one launch per level; same bits.  0 is chosen when
 * 4 * (tree nodes + 2 * n_infos * max_actions + n_infos) bytes are at most 64 KB (Leduc: 16 KB), 1 otherwise (wide Leduc: 249 KB);
 * RP_NASH_VARIANT=one|levels, read when the tree is built, forces one (tests; "one" past the limit works out of device scratch). */
RP_API int rp_mccfr_nash_variant(rp_mccfr* h, int* out);
/* loop { check_every x Solver::step; exploitability on the device } until the FIRST check with exploitability < target or until
 * max_steps (a multiple of check_every is not required: the last block is shorter and is checked too).  One 4-byte read of pinned
 * host memory per check is the only host<->device traffic.  *steps = steps taken, *exploitability = the last check's value,
 * *reached = 1 when it stopped on the target.  Uses the handle's current update mode and batch.  max_steps = 0 takes no step and
 * checks the tables as they stand; the kernels' capacity flags are read once, on return (rp_mccfr_sync reads them per call). */
RP_API int rp_mccfr_solve_to(rp_mccfr* h, float target, uint32_t check_every, uint64_t max_steps,
                             uint64_t* steps, float* exploitability, int* reached);
/* RefProf::sum_regret (book.rs:124-131), summed in (info, edge) order */
RP_API int rp_mccfr_sum_regret(rp_mccfr* h, float* out);
/* batch size may be changed between steps (no reference equivalent: batch_size is a const fn there) */
RP_API int rp_mccfr_set_batch(rp_mccfr* h, uint32_t batch_size);
RP_API int rp_mccfr_set_update_mode(rp_mccfr* h, rp_update_mode mode);
/* run on a caller-provided hipStream_t (NULL = the library's own stream) */
RP_API int rp_mccfr_set_stream(rp_mccfr* h, void* hip_stream);

/* ---- multi-GPU: trees sharded by rank, per-key composed maps exchanged -------------
 * rank r samples tree ids [r*B, (r+1)*B) of a world*B-tree batch.  step_local() runs the traversal and
 * reduces this rank's Decisions to one composed map per table cell; the caller all-gathers the
 * `summary_bytes` blobs (RCCL) and every rank folds them in rank order with step_apply(). */
RP_API int rp_mccfr_set_shard(rp_mccfr* h, uint32_t rank, uint32_t world);
RP_API int rp_mccfr_summary_bytes(rp_mccfr* h, size_t* bytes);
RP_API int rp_mccfr_step_local(rp_mccfr* h, void* summary_dev);
RP_API int rp_mccfr_step_apply(rp_mccfr* h, const void* gathered_dev, uint32_t world);
/* The PERIODIC exchange: window_local() is one local step against the table as it stood when the window began (the
 * table is not touched; the epoch — hence the sampled trees, the walker and the discounts — advances) whose composed
 * maps are folded into `window_dev` (summary_bytes; first != 0 starts a new window); after `S` such steps the caller
 * all-gathers the window summaries once and every rank applies them in rank order with window_apply() (no epoch
 * change).  S = 1 is step_local + step_apply.  Oracle: ora_mccfr_window_world. */
RP_API int rp_mccfr_window_local(rp_mccfr* h, void* window_dev, int first);
RP_API int rp_mccfr_window_apply(rp_mccfr* h, const void* gathered_dev, uint32_t world);

/* ---- rp_comm: the RCCL communicator of a one-process-per-GPU job, for hosts without torch.distributed (a Rust or C
 * trainer).  Rank 0 calls rp_comm_unique_id and ships the 128 bytes to the other ranks by its own means (MPI, a socket,
 * a file); every rank then calls rp_comm_create (ncclCommInitRank: collective, blocks until all ranks arrive).  A host that
 * already owns an ncclComm_t wraps it with rp_comm_adopt (not destroyed by rp_comm_destroy).  librccl is loaded on the
 * first rp_comm_* call.  SURVEY §8b: rp_mccfr_allreduce(h, rp_comm*). */
#define RP_COMM_ID_BYTES 128
typedef struct rp_comm rp_comm;
RP_API int rp_comm_unique_id(uint8_t* id /* [RP_COMM_ID_BYTES] */);
RP_API int rp_comm_create(const uint8_t* id, int rank, int world, int device, rp_comm** out);
RP_API int rp_comm_adopt(void* nccl_comm, int rank, int world, int device, rp_comm** out);
RP_API int rp_comm_destroy(rp_comm* c);
/* `steps` Solver::step's of a tree-sharded job (rank = the communicator's): exchange windows of `window` local steps
 * (rp_mccfr_window_local), ONE ncclAllGather of the window summaries per window on the solver's stream, then
 * rp_mccfr_window_apply — no host synchronisation inside; a trailing partial window is exchanged too.  Calls
 * rp_mccfr_set_shard(rank, world) itself.  Every rank must pass the same steps / window. */
RP_API int rp_mccfr_step_comm(rp_mccfr* h, rp_comm* c, uint32_t steps, uint32_t window);

/* which Solver::batch kernel this handle launches under its current sampling scheme: 0 = per-tree scratch in HBM (any
 * game), 1 = per-lane DFS with the tree in LDS (small games), 2 = instantiated over the game's compile-time action
 * skeleton (Kuhn / Leduc shapes, external sampling; csrc/traverse_static.hpp).  All three produce identical Decisions. */
RP_API int rp_mccfr_traversal_variant(rp_mccfr* h, int* out);
/* Variant 2 only: the size of the table of packed rows (one row of infoset ids, payoffs and draw keys per sequence of chance
 * outcomes) the traversal reads the game through; 0 when it follows the child records node by node instead (chance nodes of one
 * skeleton node with different numbers of outcomes, or RP_TRAV_NO_FLAT=1: the independent cross-check).  Same Decisions. */
RP_API int rp_mccfr_traversal_rows_bytes(rp_mccfr* h, size_t* out);
/* Composed update: how a step of the current batch size folds its group maps: 0 = in the launch that folds the block maps (the last
 * workgroup of a tile), 1 = in a launch of its own, one workgroup per infoset (batches of many groups; RP_FOLD_SPLIT=1 / 0 at creation
 * forces it always / never).  Same tables, counters and summary blobs. */
RP_API int rp_mccfr_fold_variant(rp_mccfr* h, int* out);
/* Which compile-time action skeleton a game table matches node for node, for every chance outcome (host only, no device
 * needed): 0 none (the generic traversal kernels), 1 Kuhn's, 2 Leduc's (any number of ranks). */
RP_API int rp_game_skeleton(const rp_game_table* game, int* out);

/* ---- safe subgame re-solve for table games (csrc/mccfr_subgame.hpp) ------------------------------------------------------------------
 * SubGameSolver::<_, 1, ..>::new(blueprint, external, belief, recall) with origin = None, step x iterations, Harvest::harvest
 * (subgame/src/solver.rs:47-49,146-229) over an rp_game_table game, with the handle's tables as the blueprint — what the reference's
 * own known-answer tests run (kuhn/src/solver.rs:280-517, leduc/src/solver.rs:153-285).  Both calls are READ-ONLY on the handle
 * exactly as rp_mccfr_policy is: tables, epoch and counters are unchanged, a sharded handle (world > 1) is served like any other (the
 * tables are replicas).  They queue on the handle's stream.  One wavefront per belief entry / per solve.  A table with n_players != 2
 * is RP_ERR_UNSUPPORTED (the reference's "two player game" expect).  The paragraphs named in capitals are those of the NLHE blocks
 * below (PARTITION, RESTRICT, TREE, DRAWS, PROFILE, VALUES, UPDATE, RESULT); only the deltas are stated here.
 *
 * BELIEF = Posterior, then Partition::partition::<W> (subgame/src/world/partition.rs:26-52).  Per entry: n_prior <= 16 candidates
 *   {root_state, secret < 16}, one shared path[n_path <= 16] of child slots, internal, mode, n_worlds = W in 1..4.  The mass of a
 *   candidate: mode 0 (`baseline`, kuhn/src/encoder.rs:74, leduc/src/encoder.rs:71-81) 1.0f; mode 1 (Solver::external_reach,
 *   mccfr/src/solver/solver.rs:198-210) the f32 product, from 1.0f in path order, of RP_DIST_AVERAGED(info)[slot] at the states on the
 *   path from root_state whose turn is the seat other than `internal`; chance states on the path are stepped through and contribute
 *   nothing.  The path is walked (and checked) in both modes.  Masses are added per secret in candidate order, from 0.0f
 *   (Posterior::add).  The entries of PARTITION are the secrets some candidate has, in ascending secret; 4 is W: total <= 0 gives
 *   world 0 to every entry and weights[w < W] = 1.0f / (float)W; otherwise segment = total / (float)W, the entries sorted by mass
 *   descending and stable (equal masses keep ascending secret), at most one advance per entry, index < W - 1.  world_of[s] =
 *   RP_WORLD_NONE for a secret no candidate has; weights are zero from W on.  Masses that are NaN are unspecified in value.
 *   Statuses (first that applies): RP_MSUB_SEAT internal > 1, RP_MSUB_MODE mode > 1, RP_MSUB_WORLDS, RP_MSUB_COUNT n_prior or n_path
 *   > 16, then per candidate in order RP_MSUB_SECRET, RP_MSUB_STATE, RP_MSUB_PATH (a slot >= n_children, which includes a terminal
 *   before the path ends): never an out-of-bounds read.  A failed entry answers every world_of RP_WORLD_NONE and zero weights.
 *
 * SOLVE, per solve i with id = first_id + i.  rp_mccfr_subgame_entry: observed = the state of recall.game(); external; candidate[] =
 *   the states the encoder's `restrict` enumerates (Card::ALL order, the other seat's card and the board excluded) with secret[];
 *   world_of[16], weights[4], n_worlds as BELIEF writes them; harvest_info (RP_NO_INFO = the info of the restricted entry state of the
 *   last iteration); harvest_order[16], whose first n_actions bytes are the slots of the harvest infoset in E's derived Ord (Harvest
 *   folds regret over BTreeMap<E, _> keys; Kuhn's Call < Fold is not slot order).  A world_of byte >= n_worlds reads as RP_WORLD_NONE.
 *   World of iteration t: the World rule of RESTRICT over weights[0 .. W) with h = rp_node_hash(seed, 1, id, t) (the reference uses
 *     the thread RNG: the counter contract applies; the construction-time draw of `build` is discarded by the first step).
 *   Restrict (leduc/src/encoder.rs:48-68, Kuhn's the same): if every world_of byte is RP_WORLD_NONE every candidate is remembered
 *     (Belief::remember's empty-members clause) and the first candidate wins; otherwise the first candidate with world_of[secret] ==
 *     world; if no candidate is chosen (n_candidates = 0 included) the entry state is `observed` and `fallbacks` counts it.
 *   TREE without frontiers and Pick edges: node 0 is the entry state; a decision state's branches are its children in slot order, a
 *     chance or terminal state has none (world/encoder.rs:100-107: a Leduc round-1 subgame ends at the board deal).  A node's infoset
 *     is (world_t, rp_state.info).  walker = t % 2 keeps every branch, the other seat one by the weighted draw of DRAWS with h(node) =
 *     rp_node_hash(seed, 2, id * RP_MCCFR_SUBGAME_MAX_ITERATIONS + t, node number), wrapping.  More than RP_MCCFR_SUBGAME_MAX_NODES
 *     nodes is RP_MSUB_TREE.
 *   PROFILE, VALUES, UPDATE word for word, "the blueprint row" being what rp_mccfr_get returns and "epoch" rp_mccfr_epoch: a local
 *     row shadows the blueprint for its world only; a miss reads max(blueprint, EPSILON) for weight and regret, the blueprint's value
 *     for payoff and visits; the first write warm-starts the row (mccfr/src/strategy/profile.rs:94-104); regret Summed, weight Linear
 *     at local t, sampling External whatever the handle's R / W / S; tau, beta, eps from the handle's rp_hyper.  A chance leaf is
 *     valued by cum_payoff(info, slot 0) of its parent's infoset — the local row of that world, else the blueprint (nash.rs:50-79).
 *     A chance or terminal entry state is a valid solve that updates nothing.
 *   RESULT with 4 = W: n_actions = the harvest infoset's (0 and info = RP_NO_INFO where the entry state is chance or terminal);
 *     refined[a] = the fold from 0.0f over w < W of p_w[a] / (float)W; visits[a] the wrapping sum over w; regret ONE fold of
 *     max(cum_regret, 0.0f), edges outer in harvest_order, worlds inner; sum_regret over the exported rows (slots ascending) divided by
 *     (float)max(t, 1); drawn[w], fallbacks, nodes, infosets (updated), n_rows.  rows[i][..] sorted by (world, info), zero past n_rows;
 *     n_rows is the true count even past rows_cap.  A failed solve yields a zero result with its status; the call is still RP_OK.
 *   Statuses (first that applies): RP_MSUB_SEAT external > 1, RP_MSUB_WORLDS n_worlds outside 1..4, RP_MSUB_COUNT n_candidates > 16,
 *     RP_MSUB_STATE observed or a candidate >= n_states, RP_MSUB_SECRET a candidate's secret >= 16, RP_MSUB_WEIGHT one of weights[0 ..
 *     W) negative, NaN or infinite, RP_MSUB_INFO harvest_info neither RP_NO_INFO nor an infoset; while solving RP_MSUB_TREE,
 *     RP_MSUB_ROWS (more than min(RP_MCCFR_SUBGAME_MAX_ROWS, 4 * n_infos) local rows); at the harvest RP_MSUB_ORDER (the first
 *     n_actions bytes of harvest_order are no permutation).  No input causes an out-of-bounds access or an unbounded loop.
 *   INVARIANCES.  A T-iteration solve is the first T iterations of a longer one; nothing depends on n, on the batch around a solve,
 *     on how a batch is split over calls with matching first_id, or on the launch segments below.
 * LAUNCHES.  A launch runs at most 8 192 iterations of every solve (RP_MCCFR_SUBGAME_SEGMENT = 1 .. 2^20 overrides; tests) and at
 *   most 2 048 solves; the solver state between the launches of one call — the local profile, its (world, info) -> row index, the
 *   counters — lives in a per-solve device region, allocated on first use, grown on demand, freed with the handle.  A table with more
 *   than RP_MCCFR_SUBGAME_MAX_INFOS infosets is RP_ERR_CAPACITY (the index keeps u16 row numbers, 4 x n_infos of them per solve).
 * Arguments.  solve: args first, without a device — NULL args, iterations outside 1 .. RP_MCCFR_SUBGAME_MAX_ITERATIONS, a prior not
 *   finite and positive, reserved != 0: RP_ERR_INVALID; then n = 0 is RP_OK without a launch; then a NULL handle, entries or results,
 *   or rows == NULL with rows_cap > 0: RP_ERR_INVALID; then n_players != 2: RP_ERR_UNSUPPORTED.  belief: n = 0 is RP_OK; a NULL handle,
 *   priors, world_of or weights is RP_ERR_INVALID (status may be NULL); then n_players != 2.  The host forms stage, launch and
 *   synchronise; the _device forms take every array in DEVICE memory (args on the host) and return without synchronising.
 *   rp_mccfr_subgame_solve writes 0 to the row's `kind` byte and to the result's `frontiers` word (both were padding before the
 *   depth-limited call below gave them a meaning).
 *
 * DEPTH-LIMITED: rp_mccfr_depth_solve = SubGameSolver::with_origin (subgame/src/solver.rs: build(.., Some(origin))) and, as one of its
 *   entries, DepthSolver (subgame/src/depth/solver.rs) over DepthEncoder / DepthGame (depth/encoder.rs, depth/game.rs) for table games.
 *   Every paragraph above applies word for word (RESTRICT, world draw, TREE numbering, DRAWS, PROFILE, VALUES, UPDATE, RESULT,
 *   INVARIANCES, LAUNCHES, the argument checks and their order); the deltas are the table-game form of rp_nlhe_depth_solve's
 *   paragraphs below, reproduced, not repaired.
 *   FRONTIER TABLES, on the handle (rp_mccfr_set_frontiers; host arrays, copied): depth[state] = CfrGame::depth(); for a chance state
 *     pick_info[state] < n_pick = the id of DepthInfo::Pick(inner), inner = resume(prefix ++ game edges, the chance game), and
 *     payoff_ref[state] names the D x D matrix DepthSampler::payoffs answers there ("the implementor decides what each index means"):
 *     an infoset id i < n_infos is Payoffs::uniform(the BLUEPRINT's cum_payoff(i, slot 0)) (frontier_payoff reads the blueprint, not the
 *     local profile), RP_NO_INFO is uniform(0.0f), 0x80000000u | m is matrices[m], row = internal's k, column = external's j.
 *     D = leaves in 1..4.  rp_mccfr_set_frontiers checks the struct's own fields first and needs no handle for them (leaves, reserved, a
 *     NULL array, n_pick > RP_MCCFR_SUBGAME_MAX_INFOS, a matrix entry that is not finite), then the handle (NULL: RP_ERR_INVALID), then
 *     against the handle's game table every chance state with depth > 0 (pick_info < n_pick) and every chance state's payoff_ref: all
 *     RP_ERR_INVALID with the field's name in rp_last_error, before the device is touched.  It synchronises the handle's stream,
 *     replaces any earlier tables (f = NULL clears them), and the tables are freed with the handle.  Read-only on the solver's tables,
 *     epoch and counters, like the solves.
 *     rp_game_frontiers (host only) answers the reference's values for the built-in games: Kuhn and RPS keep CfrGame::depth()'s
 *     default 0 everywhere and have no Pick infoset (n_pick = 0: no origin makes a frontier there); Leduc and wide Leduc answer 0 at
 *     Start, Dealt and R1(_), 1 everywhere else (leduc/src/game.rs:232-237), one Pick id per (seat 0's rank, round-1 spot) at the
 *     board-deal states — the chance game's info is (acting = false, seat 0's rank, board None, r1, None), leduc/src/encoder.rs:20-31,
 *     so frontier states that differ only in seat 1's card share one — numbered by the lowest-numbered state that carries them, and
 *     payoff_ref = RP_NO_INFO everywhere: leduc/src/solver.rs:7-25 asks blueprint.frontier_payoff(inner) for an infoset with acting =
 *     false, which training never writes, so unwrap_or_default makes Payoffs::uniform(0.0).  The three arrays are [n_states].
 *   ORIGIN, per solve: a value in 0 .. 253 is SubGameSolver::with_origin(origin); RP_MCCFR_ORIGIN_ENTRY (or origin == NULL for the whole
 *     batch) is depth[observed] (DepthSolver::new: origin = Some(entry.depth())); RP_MCCFR_ORIGIN_NONE is rp_mccfr_subgame_solve byte
 *     for byte.
 *   TREE.  A chance state with depth[state] > origin is a FRONTIER, at node 0 too (DepthGame::at_frontier).  It has D Pick(k) edges to
 *     Internal(k) nodes and, staying the chance node it was grown as, keeps ONE: k = rp_pick_uniform(h(node), D) — internal's
 *     continuation is never learnt.  The Internal(k) node's turn is the seat `external`; it has D Pick(j) edges to External(k, j)
 *     nodes, all kept when the walker is `external`, otherwise one by the weighted draw of DRAWS over the Pick infoset.  External(k, j)
 *     is a leaf.  Any other chance state stays the leaf it is above.  The node limit stays RP_MCCFR_SUBGAME_MAX_NODES.
 *   PROFILE.  A Pick infoset is (world, kind 1, pick id) and has D slots, slot c = continuation c.  Absent edges read weight 1.0f /
 *     (float)D, regret EPSILON, payoff 0.0f, visits 0 (DepthView); the first write creates all-zero encounters (Encounter::default()).
 *     The index grows to 4 x (n_infos + n_pick) and the row limit becomes min(RP_MCCFR_SUBGAME_MAX_ROWS, 4 * (n_infos + n_pick)).
 *   VALUES.  A frontier node multiplies neither rr nor sr and its edge is left out of the ancestor reach (a chance node);
 *     terminal_value at External(k, j) is +payoffs[k][j] for hero == 1 - external and the f32 negation otherwise, payoffs being the
 *     matrix payoff_ref of the frontier's state names, read from the handle's table, never from a local row.
 *   RESULT.  rp_mccfr_subgame_row.kind: 0 Game, 1 Pick; for a Pick row info = the pick id and n_actions = D; rows sort by (world,
 *     kind, info).  rp_mccfr_subgame_result.frontiers = the wrapping count of frontier nodes over all iterations.  A frontier entry
 *     state is a valid solve with n_actions = 0 that updates Pick rows.
 *   DEPTHSOLVER is not a second code path: DepthSolver::new(source, prefix, internal, entry) is the entry {observed = the entry state,
 *     external = 1 - internal, n_candidates = 0, n_worlds = 1, weights = {1}} with origin = RP_MCCFR_ORIGIN_ENTRY; world 0 is drawn
 *     every iteration, the entry state is `observed` every iteration and `fallbacks` counts every iteration.
 *   Statuses: those above, and RP_MSUB_FRONTIER for a frontier state whose tables are inconsistent at run time (a pick_info not below
 *     n_pick, a payoff_ref that names nothing) — unreachable after rp_mccfr_set_frontiers' validation, and checked all the same.
 *   Arguments: rp_mccfr_subgame_solve's checks in their order, then a handle without frontier tables: RP_ERR_INVALID.
 * OUT OF SCOPE: the reference-seed RNG for these draws, more than two players, tests/emul. */
#define RP_MCCFR_SUBGAME_MAX_ITERATIONS (1u << 20)
#define RP_MCCFR_SUBGAME_MAX_NODES 62u
#define RP_MCCFR_SUBGAME_MAX_ROWS 1024u
#define RP_MCCFR_SUBGAME_MAX_INFOS 8192u
#define RP_MCCFR_SUBGAME_MAX_CANDIDATES 16u
#ifndef RP_WORLD_NONE
#define RP_WORLD_NONE 0xffu
#endif
enum { RP_MSUB_OK = 0, RP_MSUB_SEAT = 1, RP_MSUB_MODE = 2, RP_MSUB_WORLDS = 3, RP_MSUB_COUNT = 4, RP_MSUB_STATE = 5, RP_MSUB_SECRET = 6,
       RP_MSUB_PATH = 7, RP_MSUB_WEIGHT = 8, RP_MSUB_INFO = 9, RP_MSUB_TREE = 10, RP_MSUB_ROWS = 11, RP_MSUB_ORDER = 12,
       RP_MSUB_FRONTIER = 13 };
typedef struct rp_mccfr_subgame_prior { /* one belief entry */
    uint32_t root_state[16];
    uint8_t secret[16];
    uint8_t path[16];
    uint8_t n_prior, n_path, internal, mode, n_worlds, pad[3];
} rp_mccfr_subgame_prior;  /* 104 bytes */
typedef struct rp_mccfr_subgame_entry { /* one solve */
    uint32_t observed, harvest_info;
    uint32_t candidate[16];
    uint8_t secret[16], world_of[16], harvest_order[16];
    float weights[4];
    uint8_t external, n_candidates, n_worlds, pad;
} rp_mccfr_subgame_entry;  /* 140 bytes */
typedef struct rp_mccfr_subgame_args { /* one per call */
    uint32_t iterations; /* 1 .. RP_MCCFR_SUBGAME_MAX_ITERATIONS */
    float prior;         /* WarmstartHyperParams::prior_strength as f32: finite, > 0 */
    uint64_t seed, first_id;
    uint32_t rows_cap;   /* local-profile rows exported per solve; 0 = none */
    uint32_t reserved;   /* 0 */
} rp_mccfr_subgame_args;   /* 32 bytes */
typedef struct rp_mccfr_subgame_result {
    uint32_t info;       /* the harvest infoset; RP_NO_INFO where there is none */
    uint8_t n_actions, status, pad[2];
    float refined[16];
    uint32_t visits[16];
    float regret, sum_regret;
    uint32_t iterations, n_rows;
    uint64_t nodes, infosets;
    uint32_t drawn[4];
    uint32_t fallbacks, frontiers; /* frontiers: 0 from rp_mccfr_subgame_solve */
} rp_mccfr_subgame_result; /* 192 bytes */
typedef struct rp_mccfr_subgame_row {
    uint8_t world, n_actions, kind /* 0 Game, 1 Pick */, pad;
    uint32_t info;
    rp_encounter enc[16]; /* zero from n_actions on */
} rp_mccfr_subgame_row;    /* 264 bytes */
/* 1 iteration, prior 2^14 (WarmstartHyperParams::default), seed 0, first_id 0, no rows */
RP_API void rp_mccfr_subgame_args_default(rp_mccfr_subgame_args* out);
RP_API int rp_mccfr_subgame_belief(rp_mccfr* h, uint64_t n, const rp_mccfr_subgame_prior* priors, uint8_t* world_of /* [n][16] */,
                                   float* weights /* [n][4] */, uint8_t* status /* [n] or NULL */);
RP_API int rp_mccfr_subgame_belief_device(rp_mccfr* h, uint64_t n, const rp_mccfr_subgame_prior* priors_dev, uint8_t* world_of_dev,
                                          float* weights_dev, uint8_t* status_dev);
RP_API int rp_mccfr_subgame_solve(rp_mccfr* h, uint64_t n, const rp_mccfr_subgame_entry* entries, const rp_mccfr_subgame_args* args,
                                  rp_mccfr_subgame_result* results, rp_mccfr_subgame_row* rows /* [n][rows_cap] or NULL */);
RP_API int rp_mccfr_subgame_solve_device(rp_mccfr* h, uint64_t n, const rp_mccfr_subgame_entry* entries_dev,
                                         const rp_mccfr_subgame_args* args /* host */, rp_mccfr_subgame_result* results_dev,
                                         rp_mccfr_subgame_row* rows_dev);
/* the depth-limited re-solve (DEPTH-LIMITED above) */
#define RP_MCCFR_ORIGIN_ENTRY 254u  /* origin = depth[observed]: DepthSolver::new */
#define RP_MCCFR_ORIGIN_NONE  255u  /* no frontier: rp_mccfr_subgame_solve, byte for byte */
typedef struct rp_mccfr_frontiers {   /* host struct, host arrays; copied */
    const uint8_t*  depth;      /* [n_states] CfrGame::depth() of every state */
    const uint32_t* pick_info;  /* [n_states] chance states: the Pick infoset, < n_pick; RP_NO_INFO elsewhere */
    const uint32_t* payoff_ref; /* [n_states] chance states: < n_infos: uniform(blueprint payoff of that infoset, slot 0);
                                   RP_NO_INFO: uniform(0.0f); 0x80000000u | m: matrices[m] */
    const float*    matrices;   /* [n_matrices][leaves][leaves], row = internal's k; NULL when n_matrices == 0 */
    uint32_t n_pick, n_matrices, leaves /* D, 1..4 */, reserved /* 0 */;
} rp_mccfr_frontiers;
RP_API int rp_mccfr_set_frontiers(rp_mccfr* h, const rp_mccfr_frontiers* f);  /* NULL f clears */
/* host only: the reference's depth / Pick infosets / payoffs of a built-in game, three arrays of [n_states] */
RP_API int rp_game_frontiers(const rp_game* g, uint8_t* depth, uint32_t* pick_info, uint32_t* payoff_ref, uint32_t* n_pick);
RP_API int rp_mccfr_depth_solve(rp_mccfr* h, uint64_t n, const rp_mccfr_subgame_entry* entries, const uint8_t* origin /* [n] or NULL = ENTRY */,
                                const rp_mccfr_subgame_args* args, rp_mccfr_subgame_result* results,
                                rp_mccfr_subgame_row* rows /* [n][rows_cap] or NULL */);
RP_API int rp_mccfr_depth_solve_device(rp_mccfr* h, uint64_t n, const rp_mccfr_subgame_entry* entries_dev, const uint8_t* origin_dev,
                                       const rp_mccfr_subgame_args* args /* host */, rp_mccfr_subgame_result* results_dev,
                                       rp_mccfr_subgame_row* rows_dev);

/* ============================================================= sparse profile ==
 * The update half of Solver::step (solver/solver.rs:96-105,143-192: update_regret, update_weight, update_payoff,
 * update_visits in batch order, then epoch += 1) for tables addressed by ROW INDEX: the NLHE-scale shape
 * (~2^27 infosets x <= 9 actions, crates/forge/README.md:175), where a per-infoset launch grid is impossible and the
 * Decisions come from a producer other than the built-in traversal (synthetic batches;
 * §8f f1: the on-device NLHE engine).  Rows are 16*max_actions contiguous bytes in HBM
 * {regret[A], weight[A], payoff[A], visits[A]} so that one touch reads and writes ONE contiguous row.
 *
 *   ORDERED   stable radix sort by row, then every row's touches applied sequentially in batch order:
 *             the reference loop, bit for bit.
 *   COMPOSED  per-row maps F(x) = max(a x + b, m) composed over blocks of RP_SPARSE_BLOCK consecutive touches,
 *             folded in block order (hot rows parallelise); the multi-GPU exchange uses the same entries:
 *             summarize -> all-gather -> fold in rank order.
 */
#define RP_SPARSE_BLOCK 64u
typedef struct rp_profile rp_profile;
typedef struct rp_decisions { /* one batch of Decisions in DEVICE memory, in application (tree-id) order */
    uint32_t n;
    const uint32_t* row;        /* [n] table row of the infoset                                   */
    const uint8_t* n_actions;   /* [n] |choices()| of the infoset (the same for every touch of a row) */
    const uint16_t* expanded;   /* [n] edges present in the regret vector (solver.rs:143-152)       */
    const float* regret;        /* [n][max_actions] regret_vector                                  */
    const float* policy;        /* [n][max_actions] policy_vector                                  */
    const float* payoff;        /* [n] infoset value                                               */
} rp_decisions;
/* default_regret: [max_actions] CfrEdge::default_regret per action slot (NULL = 0), book.rs:101-106 */
RP_API int rp_profile_create(int device, uint64_t n_rows, uint32_t max_actions, rp_regret_kind regret,
                             rp_weight_kind weight, const rp_hyper* hp, const float* default_regret,
                             uint32_t max_batch, rp_profile** out);
RP_API int rp_profile_destroy(rp_profile* h);
/* one Solver::step worth of updates: applies the batch (asynchronously on the profile's stream), epoch += 1 */
RP_API int rp_profile_apply(rp_profile* h, const rp_decisions* batch, rp_update_mode mode);
RP_API int rp_profile_sync(rp_profile* h);
RP_API int rp_profile_epoch(const rp_profile* h, uint64_t* epoch);
RP_API int rp_profile_set_epoch(rp_profile* h, uint64_t epoch);
/* out[i*max_actions + a] = Encounter of (rows[i], action a); rows is a HOST array */
RP_API int rp_profile_get_rows(rp_profile* h, uint64_t n, const uint32_t* rows, rp_encounter* out);
/* overwrite rows from the host (hydrate / resynchronisation): in[i*max_actions + a] -> (rows[i], action a) */
RP_API int rp_profile_set_rows(rp_profile* h, uint64_t n, const uint32_t* rows, const rp_encounter* in);
/* the three distributions of rp_nlhe_policy for n rows of this table, every pointer in DEVICE memory: rows_dev [n], n_actions_dev [n]
 * (clamped to max_actions), policy_dev [n][max_actions] (zero from slot n_actions on; a row >= n_rows reads as no actions).  One
 * launch queued on the profile's stream; rp_profile_sync waits. */
RP_API int rp_profile_policy(rp_profile* h, rp_dist_kind kind, uint64_t n, const uint32_t* rows_dev, const uint8_t* n_actions_dev,
                             float* policy_dev);
RP_API int rp_profile_set_stream(rp_profile* h, void* hip_stream);
/* multi-GPU: bytes of one summary entry (16 + 2*max_actions*16), and the two halves of a sharded step.
 * summarize: this rank's batch -> entries sorted by row in `entries_dev` (capacity >= batch->n entries);
 *            *n_entries is written on the host after a stream sync.
 * fold:      `n_entries` entries (all ranks' lists back to back, rank-major) -> stable sort by row -> per-row fold in
 *            rank order -> table; epoch += 1.  Every replica that folds the same list stays bit-identical. */
RP_API int rp_profile_entry_bytes(const rp_profile* h, size_t* bytes);
RP_API int rp_profile_summarize(rp_profile* h, const rp_decisions* batch, void* entries_dev, uint32_t* n_entries);
RP_API int rp_profile_fold(rp_profile* h, const void* entries_dev, uint32_t n_entries);

/* ===================================================================== nlhe ==
 * The blueprint trainer's solver: mccfr!(Nlhe, NlheEncoder, NlheTurn, NlheEdge, NlheGame, NlheInfo, 128)
 * (crates/nlhe/src/solver.rs:11) — external-sampling MCCFR over heads-up no-limit hold'em, the game generated on the
 * device (kicker::Game rules, the Pluribus action abstraction), infosets keyed by NlheInfo = (subgame Path, abstraction
 * bucket, choices Path) (nlhe/src/info.rs:145-160; columns past BIGINT, present SMALLINT, choices BIGINT of the blueprint
 * table, nlhe/src/profile.rs:20-31) and hashed to rows of an rp_profile table.  The encoder's isomorphism -> abstraction
 * map (NlheEncoder, nlhe/src/encoder.rs:30-36) is the four rp_lookup tables the clustering pipeline produces
 * (tables[street], street = 0 pref .. 3 river); tables = NULL selects a hash of the canonical observation (tests).
 * 2^cap_log2 table rows of 9 actions (144 B each) + one 32-byte key slot per row; batch = trees per step (0 = the
 * reference's 128).  2 players, stacks of 100 big blinds.  The batch is grown LEVEL-SYNCHRONOUSLY (all trees one level per
 * pair of launches, kernels sorted by node kind: robopoker_amd/csrc/nlmc_level.hpp) in 1 536 nodes of budget per tree
 * (92 B each); a batch that needs more is traversed in several passes over contiguous ranges of its trees (same Decisions).  Sampling scheme: ExternalSampling (the mccfr! macro's default) until rp_nlhe_set_sampling selects
 * PrunableSampling / PluribusSampling (Flagship, nlhe/src/lib.rs:86-90; thresholds from `hp`).
 * Device memory beside the table: 224 Decisions of buffer per tree (~120 B each) and the node arrays.  A batch of at most 2 048
 * trees (the reference runs 128) takes the one-tree-per-workgroup kernel and reserves a region of 8 192 nodes (92 + 192 B each: the
 * reference-order evaluation arrays are always allocated there) and 9 floats per walker slot PER TREE: 0.3 GB at 128 trees, 4.8 GB at
 * 2 048; the region is not released when a tree outgrows it and the handle falls back to the level-synchronous kernels.
 * Oracle: oracle/rp_oracle_nlmc.c. */
typedef struct rp_nlhe rp_nlhe;
typedef struct rp_lookup rp_lookup;
RP_API int rp_nlhe_create(int device, uint32_t cap_log2, rp_regret_kind regret, rp_weight_kind weight, const rp_hyper* hp,
                          uint64_t seed, uint32_t batch, const rp_lookup* const* tables, rp_nlhe** out);
RP_API int rp_nlhe_destroy(rp_nlhe* h);
/* SamplingScheme::sample at walker nodes (mccfr/src/sample/{external.rs:17-64, pruning.rs:44-66, pluribus.rs:72-101}) */
RP_API int rp_nlhe_set_sampling(rp_nlhe* h, rp_sampling_kind sampling);
/* rp_rng_kind for the NLHE trainer.  RP_RNG_REFERENCE: the opponent's WeightedIndex draw (sample/external.rs:41-64) and Pluribus'
 * exploration coin (sample/pluribus.rs:91) come from DefaultHasher(t, NlheInfo, tree id) -> SmallRng (flow.rs:285-295), NlheInfo's
 * Hash stream being subgame: Path(u64), choices: Path(u64), Abstraction(u16) (nlhe/src/{info.rs:41-42, public.rs:19-23,
 * secret.rs:10-11}) — the three fields of the infoset key this library already carries.  Hole cards and board cards stay on the
 * library's counter hash in both modes: the reference deals them from the unseeded thread RNG (kicker game.rs). */
RP_API int rp_nlhe_set_rng(rp_nlhe* h, rp_rng_kind kind);
/* The regret vectors' float order.  The reference values a leaf at rel / smp * payoff with the two reach products multiplied from the
 * walker node's CHILD down, and sums children in choices() order (CfrFlow::recursed_value / ancestor_reach, flow.rs:166-216).  A batch of
 * at most 2 048 trees (the reference's is 128) is ALWAYS evaluated that way (one tree per workgroup): Decisions and tables equal the
 * reference's arithmetic bit for bit.  Larger batches default to the factorised form D(node) = sum f(edge) D(child) (the same real
 * number; regret vectors within rtol 2e-4 / atol 2e-3); rp_nlhe_set_exact(h, 1) makes them carry the per-ancestor reach rows too
 * (192 B per node on top of 92: 77 GB at 262 144 trees) and equal the reference's order bit for bit as well. */
RP_API int rp_nlhe_set_exact(rp_nlhe* h, int on);
/* Solver::step (solver.rs:96-105): the batch's trees, their Decisions, the table update (ordered or composed), epoch += 1 */
RP_API int rp_nlhe_step(rp_nlhe* h, rp_update_mode mode);
/* Trainer::train (crates/forge/src/trainer.rs:18-66) over this solver — the loop forge runs on the Flagship type; the contract of
 * rp_mccfr_train (checkpoint / flush events, Checkpoint's display line, interrupt flag, Progress::summary) */
RP_API int rp_nlhe_train(rp_nlhe* h, rp_update_mode mode, uint64_t max_steps, double max_seconds, double log_interval,
                         double flush_interval, rp_train_event_fn on_event, void* user, const volatile int* interrupt,
                         char* summary, size_t summary_cap);
/* Solver::batch (solver.rs:225-250) alone, for inspection: the Decisions of the current epoch in tree order, each with
 * the infoset behind its row; *n = their number, at most `cap` are copied out; any output may be NULL.
 * regret / policy: [n][9]. */
RP_API int rp_nlhe_batch(rp_nlhe* h, uint32_t cap, uint32_t* n, uint32_t* tree, uint64_t* past, uint32_t* present, uint64_t* choices,
                         uint8_t* n_actions, uint16_t* expanded, float* regret, float* policy, float* payoff);
RP_API int rp_nlhe_epoch(rp_nlhe* h, uint64_t* epoch);
/* nodes / infos: Solver::inc_nodes / inc_infos (solver.rs:252-275); keys: infosets in the table */
RP_API int rp_nlhe_counters(rp_nlhe* h, uint64_t* nodes, uint64_t* infos, uint64_t* keys);
/* NlheProfile::rows (nlhe/src/profile.rs:144-163) without the edge expansion: every infoset with its 9 Encounters
 * (slot a = the a-th edge of `choices`); *n = infosets in the table, at most `cap` are copied */
RP_API int rp_nlhe_export(rp_nlhe* h, uint64_t cap, uint64_t* n, uint64_t* past, uint32_t* present, uint64_t* choices, rp_encounter* enc);
/* Hydrate (profile.rs:90-141): load Encounters by infoset; sets the epoch */
RP_API int rp_nlhe_import(rp_nlhe* h, uint64_t n, const uint64_t* past, const uint32_t* present, const uint64_t* choices,
                          const rp_encounter* enc, uint64_t epoch);

/* THE TABLE ITSELF ON THE DEVICE (csrc/nlmc_table.hpp): the reference's profile is a HashMap that grows by itself
 * (mccfr/src/strategy/macros.rs:13-16); here the table has 2^cap_log2 slots, and these five calls size it, grow it and move a blueprint
 * in and out of it without the host walking a slot.  Each answers RP_ERR_INVALID for a NULL handle before a device is touched.
 * rp_nlhe_export and rp_nlhe_import above stay what they are (host probing, their slot placement).
 * rp_nlhe_capacity: *cap_log2 = the table's size now, *keys = the infosets in it (rp_nlhe_counters' third value; read from the device
 *   only if something inserted without bringing the count to the host).  Either output may be NULL.
 * rp_nlhe_resize: the handle continues on a fresh table of 2^new_cap_log2 slots, new_cap_log2 in 8..30 (else RP_ERR_INVALID): new key
 *   slots, key count and profile rows; every infoset is rehashed on the device — its key to the new table's probe position, its
 *   144-byte row verbatim.  Epoch, counters, settings and every answer by key are unchanged; slot ORDER (rp_nlhe_export's order, row
 *   numbers of rp_nlhe_batch) is the new table's.  Shrinking is allowed while 2 * keys <= new slots, otherwise RP_ERR_CAPACITY before
 *   anything is allocated; the same size is RP_OK without work.  BOTH tables are resident during the call: 176 B x (old + new slots)
 *   of device memory; a failed allocation is RP_ERR_HIP and the handle stays on its old table.  The call synchronises the handle's
 *   stream (the old arrays are freed only after the rehash has run).
 * rp_nlhe_set_growth: off at creation.  With max_cap_log2 in cap_log2..30 (0 switches it off again; anything else RP_ERR_INVALID),
 *   rp_nlhe_step — and so rp_nlhe_train — and rp_nlhe_import_device resize the table before they run: to the smallest doubling, at
 *   most 2^max_cap_log2, with 2 * (keys + headroom) <= slots.  headroom = 0 selects batch x 1 536: every key a step inserts belongs
 *   to a decision node it grew, and 1 536 nodes per tree is the budget of one pass (a batch traversed in several passes may grow
 *   more).  rp_nlhe_import_device uses its n in place of headroom.  `keys` is the count the step before brought to the host with its
 *   own counts: no synchronisation per step is added.  A step that fills the table anyway fails as it always did (RP_ERR_CAPACITY,
 *   flag 32).  rp_nlhe_step_local / _apply / _comm do NOT grow: a sharded caller resizes every rank between steps.
 * rp_nlhe_export_device: rp_nlhe_export into DEVICE arrays — the same infosets in the same (slot) order with the same bytes: count per
 *   segment of 1 024 slots, scan, scatter.  *n (host) = the infosets in the table; the first min(cap, *n) are written; with cap = 0 or
 *   any of the four arrays NULL only *n is answered.  enc_dev: 16-byte aligned.  Ordered after earlier work on the handle's stream;
 *   synchronises it once, for *n.
 * rp_nlhe_import_device: rp_nlhe_import from DEVICE arrays: every key is found or inserted on the device (the table's own hash and
 *   linear probe; an inserted slot carries born = 0) and its row written whole from enc_dev[i][0..9).  A key named more than once
 *   keeps its LAST Encounters.  Maintains the key count, sets the epoch, synchronises once.  If the probe runs out of slots the call
 *   answers RP_ERR_CAPACITY and the epoch is unchanged; the keys inserted before that STAY, with their Encounters.  n = 0 sets the
 *   epoch without a launch. */
RP_API int rp_nlhe_capacity(rp_nlhe* h, uint32_t* cap_log2, uint64_t* keys);
RP_API int rp_nlhe_resize(rp_nlhe* h, uint32_t new_cap_log2);
RP_API int rp_nlhe_set_growth(rp_nlhe* h, uint32_t max_cap_log2, uint64_t headroom);
RP_API int rp_nlhe_export_device(rp_nlhe* h, uint64_t cap, uint64_t* n /* host */, uint64_t* past_dev, uint32_t* present_dev,
                                 uint64_t* choices_dev, rp_encounter* enc_dev /* [cap][9] */);
RP_API int rp_nlhe_import_device(rp_nlhe* h, uint64_t n, const uint64_t* past_dev, const uint32_t* present_dev,
                                 const uint64_t* choices_dev, const rp_encounter* enc_dev /* [n][9] */, uint64_t epoch);

/* What the blueprint says, asked BY KEY (Brain::policy, parlor/src/players/brain.rs:45-55; Source::strategy / Source::memory,
 * nlhe/src/source.rs:40-87): n infosets (past[i], present[i], choices[i]) against the device-resident table, read-only — nothing is
 * inserted, epoch / counters / keys are unchanged, and no query can fail a later step.
 * rp_nlhe_policy: RefProf::iterated_distribution / averaged_distribution (profile.rs:40-51) or CfrFlow::sampling_distribution
 * (flow.rs:24-42, temperature / smoothing / curiosity of the handle's rp_hyper).  policy [n][9]; edges [n][9] (edge code of slot a);
 * n_actions [n] = the consecutive non-zero 5-bit groups of `choices` from bit 0 (at most 9); found [n] (1: the infoset has a row).
 * edges / n_actions / found may be NULL.  An infoset without a row reads as default regret, zero weight (book.rs:93-122); slots
 * a >= n_actions are zero.  The arithmetic is rp_mccfr_policy's: f32, left folds in slot order, every operation rounded on its own.
 * The _device forms take every pointer in DEVICE memory, queue one launch on the handle's stream (rp_nlhe_set_stream) and return:
 * they are ordered after earlier steps and imports, rp_nlhe_sync waits.  The host forms stage, launch and synchronise.
 * n = 0 is RP_OK without a launch. */
RP_API int rp_nlhe_policy(rp_nlhe* h, rp_dist_kind kind, uint64_t n, const uint64_t* past, const uint32_t* present,
                          const uint64_t* choices, float* policy, uint8_t* edges, uint8_t* n_actions, uint8_t* found);
RP_API int rp_nlhe_policy_device(rp_nlhe* h, rp_dist_kind kind, uint64_t n, const uint64_t* past_dev, const uint32_t* present_dev,
                                 const uint64_t* choices_dev, float* policy_dev, uint8_t* edges_dev, uint8_t* n_actions_dev,
                                 uint8_t* found_dev);
/* Source::memory (nlhe/src/source.rs:40-65): the 9 Encounters of each infoset, enc [n][9]; an absent infoset's are
 * {weight 0, regret = the edge's default, payoff 0, visits 0}, slots a >= n_actions are zero */
RP_API int rp_nlhe_memory(rp_nlhe* h, uint64_t n, const uint64_t* past, const uint32_t* present, const uint64_t* choices,
                          rp_encounter* enc, uint8_t* n_actions, uint8_t* found);
RP_API int rp_nlhe_memory_device(rp_nlhe* h, uint64_t n, const uint64_t* past_dev, const uint32_t* present_dev,
                                 const uint64_t* choices_dev, rp_encounter* enc_dev, uint8_t* n_actions_dev, uint8_t* found_dev);

/* Ranges: what the blueprint says about every hole a seat could hold, given what the other seat has seen (Nlhe::reach,
 * opponent_reaches, opponent_range, opponent_observations, signalled_observations, signalled_reaches, normalize:
 * nlhe/src/solver.rs:137-260).  One recall is the edge-level content of a Witness (kicker/src/witness.rs:36-44) after
 * Recall::history(); translating actions to edges is the caller's (rp_nlhe_translate does it on the device).  Read-only exactly
 * as the key queries above: nothing is inserted, epoch / counters / keys are unchanged, no query can fail a later step.  One
 * workgroup per recall (csrc/nlmc_range.hpp).
 *
 * CANDIDATES, in HandIterator order (deuce/src/hand_iter.rs: ascending numeric value of the two-bit mask), count[r] of them.
 *   `board` = the union of draws[0 .. k), k = the larger of the number of Draw edges in the history (at most 3) and the street the
 *   replay ends on (the replay can deal a street no Draw edge names, see REPLAY).
 *   RP_REACH_OPPONENT  Observation::opponents (deuce/src/observation.rs:122-126): every mask disjoint from hole | board; the subject
 *                      (whose policy is multiplied) is the seat opposite `pov` and holds the candidate.
 *   RP_REACH_SIGNALLED signalled_reaches (solver.rs:227-240): every mask disjoint from board — hero's own cards are NOT removed;
 *                      the subject is `pov`, holding the candidate; the other seat's stub hole is inert.
 * REACH = 1.0f * p_1 * p_2 ..., multiplied left to right in f32, one rounding per multiply (Iterator::product, solver.rs:145-152);
 *   one factor per replay node whose turn, read BEFORE the edge is applied, is the subject (encoder.rs:72-84); an empty product
 *   is 1.0f.  The factor is averaged_distribution(info).density(edge): RP_DIST_AVERAGED's arithmetic as rp_nlhe_policy has it (an
 *   absent infoset reads as zero weights; the total is the left fold over all slots of the infoset), 0.0f when the edge is not
 *   among the infoset's choices.
 * REPLAY = CfrEncoder::replay over NlheGame::apply (nlhe/src/game.rs:50-70) from Game::from_start(dealer, stacks), with one
 *   deviation: where the reference's reveal() deals random cards, the recall's draws are dealt (street s deals draws[s]).  Corners
 *   as the reference has them: at a terminal state the remaining edges change nothing and contribute nothing; a choice edge met at a
 *   chance node first deals the pending streets (that node's turn was chance: no factor); a Draw edge met at a choice node leaves
 *   the game unchanged, is still appended to the path, and contributes factor 0 when the actor is the subject.
 * KEY of a node = resume(past, game) (nlhe/src/encoder.rs:59-67, info.rs:125-139): every edge so far is collected into a Path, which
 *   keeps only the FIRST 12 (kicker/src/path.rs:169-181, MAX_PATH_EDGES); the key's `past` is the trailing choice edges of that
 *   12-edge path, `choices` = game.choices(aggression of the same path), `present` = the bucket of (candidate, the game's board at
 *   that node).  From the 13th edge on the path no longer grows: that is the reference's behaviour for long histories and is
 *   reproduced, not repaired.
 * NORMALIZE (solver.rs:254-260): total = the f32 sum in candidate order, every reach divided by it; a total equal to zero (either
 *   sign) leaves the stream untouched.  normalize = 0: opponent_reaches / signalled_reaches; != 0: the two *_observations.
 * RANGE (rp_nlhe_opponent_range = opponent_range's Posterior<NlheSecret>): candidates and reaches of RP_REACH_OPPONENT; the bucket is
 *   abstraction(candidate, board); mass[r][b] = the f32 sum of the reaches of bucket index b in candidate order (Posterior::add,
 *   mccfr/src/strategy/posterior.rs:47-50), seen[r][b] = 1 where some candidate has that bucket (an entry of the map, mass 0.0 included).
 * STATUS per recall, rp_recall_status.  A malformed recall yields count 0, zero outputs and its status; the call is still RP_OK and
 *   the other recalls of the batch are answered.  No input causes an out-of-bounds access.
 * Outputs: count [n]; holes [n][RP_NLHE_MAX_HOLES] the candidates' masks; reach [n][RP_NLHE_MAX_HOLES]; status [n]; entries past
 * count[r] are zero; holes and status may be NULL.  mass [n][256] f32, seen [n][256].  The _device forms take every pointer in
 * DEVICE memory, queue one launch on the handle's stream and return, ordered exactly like rp_nlhe_policy_device; the host forms
 * stage, launch and synchronise.  n_recalls = 0 is RP_OK without a launch. */
#define RP_NLHE_MAX_HISTORY 48u
#define RP_NLHE_MAX_HOLES 1326u
typedef struct rp_nlhe_recall {
    uint64_t hole;       /* the point-of-view seat's two cards: bit c = card c, as everywhere in this library */
    uint64_t draws[3];   /* flop (3 bits), turn (1), river (1): the cards each Draw deals, in street order; 0 where not dealt */
    int16_t stacks[2];   /* 0,0 = the reference's STACK (200); otherwise both positive */
    uint8_t pov;         /* Witness::turn(): seat 0 or 1 */
    uint8_t dealer;      /* 0 in analysis mode */
    uint8_t n_edges;     /* <= RP_NLHE_MAX_HISTORY */
    uint8_t reserved;    /* 0 */
    uint8_t edges[RP_NLHE_MAX_HISTORY]; /* edge codes (Draw = 1 ...: kicker/src/edge.rs:101-120), Draw edges included */
} rp_nlhe_recall;
typedef enum { RP_REACH_OPPONENT = 0, RP_REACH_SIGNALLED = 1 } rp_reach_kind;
typedef enum {
    RP_RECALL_OK = 0,
    RP_RECALL_EDGE = 1,    /* an edge code that is no edge (0 or above 19) */
    RP_RECALL_ILLEGAL = 2, /* a snapped action the rules refuse (Game::is_allowed) */
    RP_RECALL_LENGTH = 3,  /* n_edges above RP_NLHE_MAX_HISTORY (a frontier: or n_prefix above RP_NLHE_MAX_PREFIX) */
    RP_RECALL_CARDS = 4,   /* hole not two cards; draws with wrong popcounts, overlapping each other or the hole, or out of street order */
    RP_RECALL_DRAW = 5,    /* a Draw (an edge, or a street the replay deals itself) that needs cards the recall does not carry */
    RP_RECALL_SEAT = 6,    /* pov > 1, dealer > 1, reserved != 0, or stacks neither 0,0 nor both positive */
    RP_RECALL_LOOKUP = 7   /* lookup-table encoder only: an observation the tables do not hold (the reference panics) */
} rp_recall_status;
RP_API int rp_nlhe_reaches(rp_nlhe* h, rp_reach_kind kind, int normalize, uint64_t n_recalls, const rp_nlhe_recall* recalls,
                           uint32_t* count, uint64_t* holes, float* reach, uint8_t* status);
RP_API int rp_nlhe_reaches_device(rp_nlhe* h, rp_reach_kind kind, int normalize, uint64_t n_recalls, const rp_nlhe_recall* recalls_dev,
                                  uint32_t* count_dev, uint64_t* holes_dev, float* reach_dev, uint8_t* status_dev);
RP_API int rp_nlhe_opponent_range(rp_nlhe* h, uint64_t n_recalls, const rp_nlhe_recall* recalls, float* mass, uint8_t* seen,
                                  uint8_t* status);
RP_API int rp_nlhe_opponent_range_device(rp_nlhe* h, uint64_t n_recalls, const rp_nlhe_recall* recalls_dev, float* mass_dev,
                                         uint8_t* seen_dev, uint8_t* status_dev);

/* Frontier payoffs: what the blueprint says a depth-limited leaf is worth (DepthSampler::payoffs, nlhe/src/solver.rs:39-67, called at
 * every frontier leaf the depth solver builds: subgame/src/depth/encoder.rs:96-98, subgame/src/encoder.rs:102-104).  For each of
 * the RP_NLHE_FRONTIER_LEAVES x RP_NLHE_FRONTIER_LEAVES pairs (k, j) of continuation strategies, `rollouts` games are played from
 * the frontier state to the end with NlheEncoder::biased_rollout (nlhe/src/encoder.rs:70-147) and their utilities averaged.  Read-only
 * exactly as the key queries above: nothing is inserted, epoch / counters / keys are unchanged, no query can fail a later step.
 * One workgroup per frontier (csrc/nlmc_frontier.hpp).
 *
 * FRONTIER STATE `game` = the state after `edges` has been replayed from Game::from_start(dealer, stacks) by the ranges' REPLAY rule,
 *   with the frontier's own draws and both seats holding their cards (holes[s] is seat s's).  RP_RECALL_DRAW where a street is needed
 *   and not carried.  `game` may be a chance node (the reference's case), a choice node, or terminal.
 * PREFIX.  The reference passes payoffs() the SOLVER's construction prefix (solver.rs:97-101: the current street's descents of the
 *   recall the solver was built from), not the path to the leaf: it is the same for every leaf of one solver.  So `prefix` is an
 *   input of its own, independent of `edges`, and the story of a rollout starts from it (Story::from(prefix), encoder.rs:91).  A
 *   Path keeps only its first 12 edges, so a longer prefix could never matter: n_prefix > 12 is RP_RECALL_LENGTH.
 * ROLLOUT = encoder.rs:89-115 over plain Game::apply: at a chance node ONE street is dealt (game.reveal()), at a choice node the edge
 *   sampled below is applied as game.apply(game.snap(game.actionize(edge))); every step pushes its edge (Draw, or the sampled edge)
 *   onto the story; a terminal node ends the rollout.
 * KEY at a decision = resume(story edges, game) (encoder.rs:59-67), the ranges' KEY rule applied to the story: the first 12 edges
 *   of prefix ++ rollout edges are the path, `past` its trailing choice edges, `choices` = game.choices(aggression of that path),
 *   `present` = the bucket of (the actor's hole, the board).  From the 13th story edge on the path is frozen; reproduced, not repaired.
 * POLICY = RP_DIST_AVERAGED in rp_nlhe_policy's arithmetic; an absent infoset, or a row of zero weights, is uniform.
 * SAMPLE_BIASED (encoder.rs:121-146), f32, one rounding per operation: w_a = p_a * m_a with m_a = bias when the actor's continuation
 *   is 1 and the edge is Fold, 2 and the edge is Check or Call, 3 and the edge is Open, Raise or Shove, and 1.0f otherwise
 *   (continuation 0 biases nothing); the actor's continuation is k for seat `internal`, j for the other seat.  total = the left fold
 *   of w from 0; threshold = u * total; the running sum starts from 0 and the first slot with threshold < sum wins, the last slot
 *   if there is none.
 * VALUE = (float)(reward - spent) of seat `internal` at the terminal state (Settlement::won, kicker/src/settlement.rs:30-32);
 *   payoffs[i][k][j] = the f32 left fold over r, divided by (float)rollouts.
 * RANDOM NUMBERS.  The reference uses the thread RNG here (rand::random, Deck::deal): there is nothing of the reference's to
 *   reproduce, and the library's counter contract is used (the one rp_nlhe_playouts has).  rollout_id = ((first_id + i) * 16 + 4 k + j)
 *   * rollouts + r, wrapping; draw c of a rollout is rp_node_hash(seed, 0, rollout_id, c), c counting from 0 in consumption order.  A
 *   chance step consumes one draw per card — rp_pick_uniform over the popcount of the deck picks the pick-th lowest card, which is
 *   then removed: 3 cards to the flop, then 1 and 1 — a decision one draw, u = rp_u01.  The deck is the 52 cards minus both holes and
 *   the board.  A frontier's answer depends on seed, first_id + i and its own record only, never on the batch around it.
 * TERMINATION.  The step loop of a rollout is bounded by a constant derived from the rules (chips are finite, every raise commits
 *   some: csrc/nlmc_frontier.hpp).  A rollout that reaches the bound, or a snapped action the rules refuse, gives the frontier the
 *   status RP_RECALL_ILLEGAL instead of a hang.
 * STATUS per frontier, rp_recall_status, by the ranges' rules: n_edges above RP_NLHE_MAX_HISTORY or n_prefix above 12 LENGTH;
 *   internal > 1, dealer > 1, reserved != 0 or bad stacks SEAT; a hole that is not two cards, or cards shared between the holes and
 *   the draws, CARDS; an edge code outside 1..19 in `edges` or `prefix` EDGE.  A malformed frontier yields zero outputs and its
 *   status; the call is still RP_OK and the rest of the batch is answered.  No input causes an out-of-bounds access or an unbounded loop.
 * Arguments: rollouts = 0 is treated as 1 (FrontierHyperParams::rollouts, subgame/src/depth/hyperparams.rs:29-31); rollouts > 4096,
 *   or a bias that is not finite and positive, is RP_ERR_INVALID.  payoffs [n][4][4]; won [n][16][rollouts] the utility of every
 *   rollout (may be NULL); status [n] (may be NULL).  The _device form takes every pointer in DEVICE memory, queues one launch on the
 *   handle's stream and returns, ordered exactly like rp_nlhe_policy_device; the host form stages, launches and synchronises.
 *   n = 0 is RP_OK without a launch. */
#define RP_NLHE_FRONTIER_LEAVES 4u
#define RP_NLHE_MAX_PREFIX 12u
typedef struct rp_nlhe_frontier {
    uint64_t holes[2];   /* the cards of seat 0 and seat 1 */
    uint64_t draws[3];   /* as in rp_nlhe_recall */
    int16_t stacks[2];   /* as in rp_nlhe_recall */
    uint8_t internal;    /* the seat whose utility is reported: 0 or 1 */
    uint8_t dealer;      /* as in rp_nlhe_recall */
    uint8_t n_edges;     /* <= RP_NLHE_MAX_HISTORY */
    uint8_t n_prefix;    /* <= RP_NLHE_MAX_PREFIX */
    uint8_t edges[RP_NLHE_MAX_HISTORY]; /* the history from Game::from_start to the frontier state, Draw edges included */
    uint8_t prefix[RP_NLHE_MAX_PREFIX]; /* the solver's construction prefix: the story starts from it; independent of `edges` */
    uint8_t reserved[4]; /* 0 */
} rp_nlhe_frontier;      /* 112 bytes */
RP_API int rp_nlhe_frontier_payoffs(rp_nlhe* h, uint64_t n, const rp_nlhe_frontier* frontiers, float bias, uint32_t rollouts,
                                    uint64_t seed, uint64_t first_id, float* payoffs, int16_t* won, uint8_t* status);
RP_API int rp_nlhe_frontier_payoffs_device(rp_nlhe* h, uint64_t n, const rp_nlhe_frontier* frontiers_dev, float bias,
                                           uint32_t rollouts, uint64_t seed, uint64_t first_id, float* payoffs_dev, int16_t* won_dev,
                                           uint8_t* status_dev);

/* Subgame worlds: the opponent's range cut into quantile worlds, and opponent holes dealt from a world (Nlhe::setup,
 * nlhe/src/solver.rs:129-136 = opponent_range(recall).partition(); the Belief<NlheSecret, 4> it yields is used on every iteration of
 * SubGameSolver::step / WorldSolver::new, subgame/src/solver.rs:94-100,149-153, world/solver.rs:49-50,66-72: a world is drawn from
 * belief.weights() and NlheEncoder::restrict, nlhe/src/encoder.rs:148-186, rejection-samples an opponent hole of that world).  The
 * outputs of rp_nlhe_restrict are what rp_nlhe_frontier.holes[external] wants.  Read-only exactly as the key queries above: nothing is
 * inserted, epoch / counters / keys are unchanged, no query can fail a later step.  One workgroup per recall (csrc/nlmc_world.hpp).
 *
 * PARTITION (Partition::partition::<4> for Posterior<NlheSecret>, subgame/src/world/partition.rs:26-52) of mass[256], seen[256].
 *   The entries are the buckets b with seen[b] != 0 in ascending b (the BTreeMap's order: an Abstraction is street << 8 | index and a
 *   recall has one street).  total = the f32 left fold of the entries' masses in that order.  total <= 0 (no entry at all included):
 *   every entry gets world 0 and weights = {0.25f, 0.25f, 0.25f, 0.25f}.  Otherwise the entries are sorted by mass, descending and
 *   stable — equal masses keep ascending b (sort_by with partial_cmp) — segment = total / 4.0f, index = 0, bucket = accumulated =
 *   0.0f, and for each entry in sorted order: bucket += m; accumulated += m; world[b] = index; then, if accumulated >= segment *
 *   (float)(index + 1) && index < 3: weights[index] = bucket / total; index += 1; bucket = 0.0f — an `if`, not a `while`: at most one
 *   advance per entry.  After the loop weights[index] = bucket / total.  A world never reached keeps weight 0.0f.  Every operation is
 *   rounded on its own, in f32.  world[b] = RP_WORLD_NONE where seen[b] == 0.  The range's masses are finite and >= +0; for the
 *   stand-alone entry an input outside that is unspecified in value, but no input causes an out-of-bounds access or an unbounded loop.
 * BELIEF of a recall = PARTITION applied to rp_nlhe_opponent_range's mass / seen of that recall: the same candidates
 *   (RP_REACH_OPPONENT, HandIterator order), the same REPLAY / KEY / REACH, the same statuses, RP_RECALL_LOOKUP exactly as there.
 *   hole_world[j] = world[bucket(candidate j, head board)]; entries past count are RP_WORLD_NONE.  A malformed recall is the empty
 *   row: every world RP_WORLD_NONE, weights 0.25f.
 * RESTRICT (NlheEncoder::restrict).  Recall r's deals d = 0 .. deals are answered each on its own:
 *   deal_id = (first_id + r) * deals + d, wrapping; draw c of a deal is rp_node_hash(seed, 1, deal_id, c) (epoch 1: the frontier's
 *   stream uses epoch 0).
 *   World.  A request 0..3 is that world.  A request RP_WORLD_NONE (or worlds == NULL) draws it: x = rp_u01(draw 0) * (the left fold
 *   of weights from 0.0f); the first world whose running f32 sum exceeds x wins (x < sum); if there is none — it cannot happen with
 *   u < 1, and is stated so that the rule is total — the highest world of non-zero weight, world 0 if every weight is zero.  Draw 0
 *   belongs to the world whether or not it is used.  A request in 4..254 is a malformed deal: hole 0, world_out RP_WORLD_NONE,
 *   attempts 0.
 *   Attempt a uses draws 1 + 2a and 2 + 2a.  The free cards are the 52 cards minus pov's hole and the head board (Observation::
 *   opponents' set, which equals deck | external's cards of encoder.rs:165).  First card: the rp_pick_uniform(h, n_free)-th lowest
 *   free card; second card: the rp_pick_uniform(h', n_free - 1)-th lowest of the rest.  The attempt is accepted iff hole_world[that
 *   hole] == world (Belief::remember; its empty-members clause cannot occur, a valid recall has candidates).
 *   The answer is the hole of the first accepted attempt a in [0, RP_NLHE_MAX_REJECTIONS), attempts = a; if there is none, the hole
 *   of attempt a = RP_NLHE_MAX_REJECTIONS whatever its world, attempts = RP_NLHE_MAX_REJECTIONS (the reference's fallback to an
 *   unconstrained hole).  world_out = the world asked for or drawn.  How the kernel finds the first accepted attempt is its own
 *   business (a world without a member goes straight to the fallback); the sequential rule defines the answer.
 *   RANDOM NUMBERS.  The reference uses the thread RNG here (Deck::from(available).hole(), and the caller's draw of the world): there
 *   is nothing of the reference's to reproduce, and the library's counter contract is used, as the frontier payoffs do.  Cards are
 *   picked as the frontier picks them — the pick-th lowest card, uniform — not by a bit-for-bit restatement of Deck::draw's loop
 *   (deuce/src/deck.rs:33-48): both are uniform over the ordered pairs of distinct free cards.
 *   A recall's answer depends on seed, first_id + r, deals and its own record only, never on the batch around it.  A malformed
 *   recall yields zero holes, RP_WORLD_NONE, zero attempts and its status; the call is still RP_OK.
 * Arguments: world [n][256] u8, weights [n][4] f32, hole_world [n][RP_NLHE_MAX_HOLES] u8 (may be NULL), status [n] (may be NULL);
 *   worlds [n][deals] u8 (may be NULL: every world is drawn), holes [n][deals] u64, world_out [n][deals] u8 (may be NULL), attempts
 *   [n][deals] u16 (may be NULL).  n = 0 or deals = 0 is RP_OK without a launch; deals > 4096, or a NULL required pointer, is
 *   RP_ERR_INVALID.  The _device forms take every pointer in DEVICE memory, queue one launch on the handle's stream and return,
 *   ordered exactly like rp_nlhe_policy_device; the host forms stage, launch and synchronise. */
#define RP_NLHE_WORLDS 4u             /* pokerkit::N_WORLDS */
#define RP_NLHE_MAX_REJECTIONS 10000u /* encoder.rs:162 */
#define RP_WORLD_NONE 0xffu           /* a bucket / hole that is no member; in a request: "draw the world" */
RP_API int rp_nlhe_partition(rp_nlhe* h, uint64_t n, const float* mass, const uint8_t* seen, uint8_t* world, float* weights);
RP_API int rp_nlhe_partition_device(rp_nlhe* h, uint64_t n, const float* mass_dev, const uint8_t* seen_dev, uint8_t* world_dev,
                                    float* weights_dev);
RP_API int rp_nlhe_belief(rp_nlhe* h, uint64_t n_recalls, const rp_nlhe_recall* recalls, uint8_t* world, float* weights,
                          uint8_t* hole_world, uint8_t* status);
RP_API int rp_nlhe_belief_device(rp_nlhe* h, uint64_t n_recalls, const rp_nlhe_recall* recalls_dev, uint8_t* world_dev,
                                 float* weights_dev, uint8_t* hole_world_dev, uint8_t* status_dev);
RP_API int rp_nlhe_restrict(rp_nlhe* h, uint64_t n_recalls, const rp_nlhe_recall* recalls, uint32_t deals, const uint8_t* worlds,
                            uint64_t seed, uint64_t first_id, uint64_t* holes, uint8_t* world_out, uint16_t* attempts,
                            uint8_t* status);
RP_API int rp_nlhe_restrict_device(rp_nlhe* h, uint64_t n_recalls, const rp_nlhe_recall* recalls_dev, uint32_t deals,
                                   const uint8_t* worlds_dev, uint64_t seed, uint64_t first_id, uint64_t* holes_dev,
                                   uint8_t* world_out_dev, uint16_t* attempts_dev, uint8_t* status_dev);

/* Depth-limited re-solve: DepthSolver::step x iterations and Harvest::harvest (subgame/src/depth/solver.rs:76-123), the solver
 * Nlhe::adapt_leaf builds (nlhe/src/solver.rs:97-102) and Solved::run drives (parlor/src/players/solved.rs:39-64).  One small tree
 * per iteration from the entry state, the local profile beside it, every frontier's rollouts in the same launch; many solves per call.
 * Read-only exactly as the queries above: nothing is inserted, epoch / counters / keys are unchanged, no solve can fail a later step.
 * One workgroup per solve (csrc/nlmc_depth.hpp).
 *
 * ENTRY = an rp_nlhe_frontier, validated and replayed by the frontier's rules with the frontier's statuses: `game` = the entry state,
 *   `internal` = the seat the solve is for (recall.turn()), `prefix` = the solver's construction prefix (the reference passes the
 *   trailing choice edges of the history, subgame_descents).  Both holes are required and distinct: the reference's `wipe` state
 *   (both seats holding the hero's cards, kicker/src/witness.rs:219-221) cannot be dealt from one deck and is RP_RECALL_CARDS here.
 * ORIGIN.  DepthGame::at_frontier (depth/game.rs:73-77) needs inner.depth() > origin at a chance node, and NlheGame::depth() is the
 *   street (nlhe/src/game.rs:72-74).  DepthSolver::new sets origin = the entry's street, so under adapt_leaf the chance node that closes
 *   the entry street (whose board is still the entry street's) is NOT a frontier: it is a leaf (depth/encoder.rs:109-110) valued by
 *   stored payoffs, and no rollout is played.  That is reproduced, not repaired, and origin is an input: origin[i] = the entry's street
 *   (or RP_NLHE_DEPTH_ORIGIN_ENTRY, or origin == NULL for the whole batch) is adapt_leaf bit for bit; origin[i] = street - 1 puts the
 *   4 x 4 continuation game at the next street boundary.  Any other value outside -1 .. 3 is RP_RECALL_SEAT.
 * PROFILE = DepthProfile over DepthView over this handle's table (depth/profile.rs, depth/view.rs), t = 0 at the start of a solve.  An
 *   infoset is (kind, past, present, choices), kind 0 Game / 1 Pick.  A local row shadows the blueprint.  Absent, cum_weight and
 *   cum_regret read max(blueprint, EPSILON), cum_payoff and cum_visits the blueprint's value; an infoset the blueprint does not hold
 *   reads as rp_nlhe_memory reads it (default regrets, zero weight, payoff, visits).  Pick edges read 0.25f, EPSILON, 0.0f, 0.  The
 *   first write of an edge creates it from warmstart (mccfr/src/strategy/profile.rs:94-104): weight = ((p * k) * (k + 1.0f)) / 2.0f
 *   with k = `prior` and p = RP_DIST_AVERAGED of the blueprint row, regret = blueprint regret * (k / (float)max(epoch, 1)), payoff 0,
 *   visits 0; Pick edges from Encounter::default() (all zero).  regret() = max(cum_regret, EPSILON), weight() likewise.  The
 *   warmstart's regret is stated for completeness and is unobservable: an edge is first written by update_regret (every slot of an
 *   updated infoset has a child at its head), which reads cum_regret before the edge exists and overwrites the warmstart's value.
 * ITERATION t = 0 .. iterations: walker = seat t % 2; one tree; the Decisions of every infoset whose head's turn is the walker, all
 *   computed on the profile as it stands, then applied in ascending head-node order; t += 1.
 * TREE = TreeBuilder with ExternalSampling over DepthEncoder (mccfr/src/solver/builder.rs, sample/external.rs, depth/encoder.rs).
 *   Node 0 is the entry state.  A node's branches are pushed in slot order onto one stack and the stack's top is grown next, so nodes
 *   are numbered in depth-first order, a node's LAST slot first; a node's edges are walked newest first (petgraph), which is slot
 *   order.  Branches of a node, by what it is:
 *     a chance node with street > origin (a FRONTIER; they are numbered f = 0, 1, .. in node order): the four Pick(k) edges, leading
 *       to Internal(k) nodes.  The node itself stays the chance node it was grown as (depth/encoder.rs:95-101 turns a copy into the
 *       Frontier phase), so ExternalSampling keeps ONE of the four, uniformly (`randomly`), its info is never read and internal's
 *       continuation is not learnt.
 *     an Internal(k) node (turn = the seat opposite `internal`): the four Pick(j) edges to External(k, j) nodes, which are terminal
 *       with payoff payoffs[k][j] for `internal`, -payoffs[k][j] for the other seat.  Its infoset is Pick(key of the chance node):
 *       past = the trailing choice edges of the 12-edge path, present = the bucket of the ticker's seat (sweat() at a chance node,
 *       kicker/src/game.rs:180-185, 656-658), choices = the one-edge Path [Draw] (game.choices at a chance node); four slots, slot c
 *       = continuation c.
 *     any other chance node, a terminal node: none (a leaf).
 *     a decision node: one per edge of its infoset's choices, the state after game.apply(game.snap(game.actionize(edge))).  Its
 *       infoset is Game(KEY), KEY = resume(prefix ++ the game edges from the entry, game) by the frontier's KEY rule (first 12 edges).
 *   Of a node whose turn is the walker every branch is kept; of any other decision or Internal node one, by the weighted draw.
 * DRAWS.  h(node) = rp_node_hash(seed, 2, (first_id + i) * RP_NLHE_DEPTH_MAX_ITERATIONS + t, the node's number), wrapping — epoch 2:
 *   the frontier's stream is epoch 0, the worlds' epoch 1; a function of seed, first_id + i, t and the node only.  Frontier node:
 *   rp_pick_uniform(h, 4).  Weighted draw (sample/external.rs:41-64 as the blueprint traversal draws it): w_a = max(q_a, EPSILON)
 *   with q = RP_DIST_SAMPLING of weight() under the handle's rp_hyper; total = the left fold of w; u = rp_u01(h) * total; the pick
 *   starts at slot 0 and moves on while the running sum up to and including it is <= u and a slot is left.
 * FRONTIER PAYOFFS of frontier f of tree t are, bit for bit, rp_nlhe_frontier_payoffs' answer for the record {holes, draws, stacks,
 *   internal, dealer, edges = the entry's edges ++ the game edges to the node, prefix} with the call's seed, bias and rollouts and
 *   first_id + i = ((first_id + i) * RP_NLHE_DEPTH_MAX_ITERATIONS + t) * RP_NLHE_DEPTH_MAX_FRONTIERS + f (wrapping).  So a
 *   T-iteration solve is the first T iterations of a longer one, and a batch split over calls with matching first_id answers the same.
 *   A frontier's status other than OK is the solve's; more than RP_NLHE_DEPTH_MAX_FRONTIERS frontiers in one tree is
 *   RP_DEPTH_FRONTIERS, a history past RP_NLHE_MAX_HISTORY RP_RECALL_LENGTH.
 * VALUES = CfrFlow::dfs (mccfr/src/strategy/flow.rs:64-86) per infoset, f32, one rounding per operation, every sum a left fold from
 *   0.0f in slot order.  rd = the fold of regret() over the head's choices.  For each node `root` of the span in node order:
 *     reach = cf / sm, both folded from 1.0f up the ancestors of root, nearest first, over the edges whose parent's turn is neither
 *       chance nor the walker: cf *= regret(edge) / (the parent's rd), sm *= the parent's q(edge);
 *     v_a = reach * recursed_value(child a, 1.0f, 1.0f) for each child; ev = the fold of (regret(a) / rd) * v_a; payoff += ev;
 *     delta_a += v_a - ev (from 0.0f).
 *   recursed_value(node, rr, sr) = (rr / sr) * terminal_value(node) at a node without children, else the fold over its children of
 *     recursed_value(child, rr' , sr'): rr' = rr * regret(edge) / rd unless the node is chance, sr' = sr * q(edge) where the node
 *     is neither chance nor the walker's.  terminal_value (nash.rs:66-79) for hero = root's turn: at a terminal state game.payoff(hero)
 *     = (float)(reward - spent), or +-payoffs[k][j] at an External node; at a chance leaf cum_payoff(info, first choice) of the nearest
 *     ancestor that is not chance — a stored payoff, from the local row if there is one, else the blueprint's.
 *   policy = RP_DIST_ITERATED of regret() (iterated_distribution).
 * UPDATE (mccfr/src/solver/solver.rs:143-192) of one infoset, edge by edge: regret = max(cum_regret + delta, -inf) (SummedRegret);
 *   weight = max(cum_weight + policy * (float)t, EPSILON) (LinearWeight, epoch t); payoff += (payoff_of_the_infoset - payoff) /
 *   (float)(cum_visits + 1); visits += 1 — in that order, so on an infoset's first update cum_regret is still max(blueprint,
 *   EPSILON) while cum_weight, payoff and visits are already the warmstart's.
 * RESULT = Harvest at Game(KEY of the entry state): the key, n_actions, refined = iterated_distribution, visits = cum_visits, regret =
 *   the fold of max(cum_regret, 0.0f); n_actions = 0 and a zero key where the entry state is chance or terminal (a valid solve).
 *   sum_regret = (the fold of max(regret, 0.0f) over the local rows in exported order, slots ascending) / (float)max(t, 1) — the
 *   reference folds a HashMap in no stated order.  Counters: nodes, infosets (updated), frontiers and rollouts (16 x rollouts each)
 *   over all iterations.  rows[i][..]: the local profile, sorted ascending by (kind, past, present, choices); n_rows is the true count
 *   even where it exceeds rows_cap.  A solve that fails yields a zero result (and no rows) with its status; the call is still RP_OK
 *   and the rest of the batch is answered.
 * BOUNDS.  Every loop is bounded; a tree of more than RP_NLHE_DEPTH_MAX_NODES nodes (or more than its share of distinct infosets or
 *   pending branches) ends the solve with RP_DEPTH_NODES, a local profile of more than RP_NLHE_DEPTH_MAX_ROWS rows with RP_DEPTH_ROWS.
 *   The first 64 rows of a solve live in LDS, the rest in a region of device memory the handle keeps for the call (168 bytes x 448 rows
 *   per solve of a launch, at most 4 096 solves per launch; allocated on first use, grown on demand, freed with the handle).
 * Arguments: NULL args, iterations outside 1 .. RP_NLHE_DEPTH_MAX_ITERATIONS, rollouts > 4096 (0 reads as 1), a bias or prior that is
 *   not finite and positive, or reserved != 0 is RP_ERR_INVALID whatever else is passed (args are checked first, without a device);
 *   then n = 0 is RP_OK without a launch; then a NULL handle, entries or results, or rows == NULL with rows_cap > 0, is RP_ERR_INVALID.  The _device form takes every array in DEVICE memory, queues its launches on
 *   the handle's stream and returns, ordered exactly like rp_nlhe_policy_device; the host form stages, launches and synchronises. */
#define RP_NLHE_DEPTH_MAX_ITERATIONS 4096u
#define RP_NLHE_DEPTH_MAX_FRONTIERS 32u
#define RP_NLHE_DEPTH_MAX_NODES 384u
#define RP_NLHE_DEPTH_MAX_ROWS 512u
#define RP_NLHE_DEPTH_ORIGIN_ENTRY 127 /* origin[i]: the entry's street */
enum { RP_DEPTH_NODES = 8, RP_DEPTH_ROWS = 9, RP_DEPTH_FRONTIERS = 10 }; /* statuses after RP_RECALL_LOOKUP */
typedef struct rp_nlhe_depth_args { /* one per call */
    uint32_t iterations; /* 1 .. RP_NLHE_DEPTH_MAX_ITERATIONS */
    uint32_t rollouts;   /* as rp_nlhe_frontier_payoffs: 0 reads as 1, > 4096 invalid */
    float bias;          /* finite, > 0 */
    float prior;         /* WarmstartHyperParams::prior_strength as f32: finite, > 0 */
    uint64_t seed, first_id;
    uint32_t rows_cap;   /* local-profile rows exported per solve; 0 = none */
    uint32_t reserved;   /* 0 */
} rp_nlhe_depth_args;    /* 40 bytes */
typedef struct rp_nlhe_depth_result {
    uint64_t past, choices; /* the key of the entry state's infoset */
    uint32_t present;
    uint8_t n_actions, status, pad[2];
    float refined[9];
    uint32_t visits[9];
    float regret, sum_regret;
    uint32_t iterations, n_rows;
    uint64_t nodes, infosets, frontiers, rollouts;
} rp_nlhe_depth_result;  /* 144 bytes */
typedef struct rp_nlhe_depth_row {
    uint8_t kind, n_actions, pad[2]; /* kind 0 Game, 1 Pick */
    uint32_t present;
    uint64_t past, choices;
    rp_encounter enc[9];             /* zero from n_actions on */
} rp_nlhe_depth_row;     /* 168 bytes */
/* bias 5, rollouts 16 (FrontierHyperParams::default), prior 2^14 (WarmstartHyperParams::default), 1 iteration, no rows */
RP_API void rp_nlhe_depth_args_default(rp_nlhe_depth_args* out);
RP_API int rp_nlhe_depth_solve(rp_nlhe* h, uint64_t n, const rp_nlhe_frontier* entries, const int8_t* origin,
                               const rp_nlhe_depth_args* args, rp_nlhe_depth_result* results,
                               rp_nlhe_depth_row* rows /* [n][rows_cap] or NULL */);
RP_API int rp_nlhe_depth_solve_device(rp_nlhe* h, uint64_t n, const rp_nlhe_frontier* entries_dev, const int8_t* origin_dev,
                                      const rp_nlhe_depth_args* args /* host */, rp_nlhe_depth_result* results_dev,
                                      rp_nlhe_depth_row* rows_dev);

/* Safe subgame re-solve: SubGameSolver::step x iterations and Harvest::harvest (subgame/src/solver.rs:146-229), the solver
 * Nlhe::adapt_full builds (nlhe/src/solver.rs:121-127), and — see ADAPT_SAFE — the one adapt_safe builds.  Many solves per call, one
 * workgroup per solve (csrc/nlmc_subgame.hpp), read-only exactly as the depth solve.  Everything the depth solve's block above states
 * holds here word for word — ENTRY's replay and statuses, TREE, DRAWS, FRONTIER PAYOFFS, VALUES, UPDATE, the counters — except for
 * the deltas below.
 *
 * WHERE THE TREE ENDS.  SubGameSolver::new passes origin = None (solver.rs:47-49), so DepthGame::at_frontier is false at every node
 *   (depth/game.rs:73-77) and SubGameEncoder::branches gives a chance or terminal node no branch (encoder.rs:115-116; WorldEncoder the
 *   same, world/encoder.rs:100-107).  The tree of adapt_full and of adapt_safe is therefore the rest of the ENTRY STREET, its chance
 *   leaves valued by stored payoffs — the depth block's adapt_leaf situation — whatever the reference's own comments say about trees
 *   "to the terminals" (nlhe/src/solver.rs:103-107, world/solver.rs:1-8).  Reproduced, not repaired.
 * ORIGIN, per solve.  RP_NLHE_SUBGAME_ORIGIN_NONE (or origin == NULL for the whole batch) is adapt_full as written: no node is a
 *   frontier, no rollout is played, `rollouts` and `bias` are not read.  A value in -1 .. 3 is SubGameSolver::with_origin: a chance
 *   node with street > origin is a FRONTIER exactly as in the depth block.  Anything else is RP_RECALL_SEAT.
 * ENTRY.  Only holes[internal] is read and validated; holes[1 - internal] may hold anything.  The draws are checked against
 *   internal's hole alone.  `internal` is the seat the solve is for, the seat opposite is dealt anew before every tree.
 * BELIEF, per solve, an input: hole_world[RP_NLHE_MAX_HOLES] u8 and weights[4] f32 exactly as rp_nlhe_belief(_device) writes them for
 *   the recall {pov = internal, hole = holes[internal], draws, edges, stacks, dealer}.  The free cards are the 52 minus internal's
 *   hole and the entry state's board, in ascending order; the candidate index of a hole is hi (hi - 1) / 2 + lo over the positions
 *   (hi > lo) of its cards among them; count = n_free (n_free - 1) / 2.  The belief is data: a hole_world byte in 4 .. 254, and any byte
 *   at or past count, reads as RP_WORLD_NONE.  A weight that is negative, NaN or infinite makes the solve RP_RECALL_CARDS (a belief
 *   that could not have been dealt from; no closer status exists).  All weights zero is legal: every iteration draws world 0.
 * DEAL of iteration t = deal d = t of recall first_id + i under rp_nlhe_restrict's rules with deals = RP_NLHE_DEPTH_MAX_ITERATIONS and
 *   no world requested: deal_id = (first_id + i) * RP_NLHE_DEPTH_MAX_ITERATIONS + t on epoch 1, World, Attempt, the fallback at
 *   RP_NLHE_MAX_REJECTIONS and RANDOM NUMBERS unchanged.  So rp_nlhe_restrict(deals = 4096) on that recall answers every deal of a
 *   solve, a T-iteration solve is the first T iterations of a longer one, and a split batch answers the same.  The hole dealt is the
 *   other seat's cards for the whole of tree t: its `present` buckets, the showdowns, and holes[1 - internal] of the record FRONTIER
 *   PAYOFFS names.  (SubGameSolver::build's construction-time deal is discarded by the first step and is not reproduced.)
 *   The workgroup finds the first accepted attempt with all 256 lanes (lane l tries l, l + 256, ..; the minimum accepted index wins
 *   after each round); a world none of whose candidates belongs to it goes straight to the fallback.
 * PROFILE = WorldProfile over DepthView (world/profile.rs, depth/view.rs).  An infoset is (world, kind, past, present, choices): every
 *   infoset of tree t carries world_t (WorldInfo, world/info.rs; subgame/src/encoder.rs:46-57).  A local row shadows the blueprint for
 *   its world only; a read that misses falls to the blueprint by the UNTAGGED key with the depth block's max(., EPSILON) rules
 *   (profile.rs:120-146); the first write warm-starts from the untagged blueprint row (profile.rs:67-109 through DepthView::warmstart).
 *   depth/view.rs was read for anything else: it forwards t, sum_regret, walker and the three sampling parameters to the blueprint
 *   and overrides nothing further, so the depth block's PROFILE rules with the tag added are the whole of it.  A chance leaf's stored
 *   payoff reads the local row of that world, else the blueprint.
 * RESULT = Harvest (solver.rs:184-229) at Game(KEY of the entry state); the entry state's cards are the last iteration's (only its
 *   `present` can depend on them, and only where the seat to act is not `internal`).  p_w = iterated_distribution at world w — from the
 *   local row of that world, else from max(blueprint, EPSILON).
 *     refined[a] = the f32 fold from 0.0f over w = 0 .. 3 of p_w[a] / 4.0f; Pick edges do not occur at a Game infoset.
 *     visits[a]  = the wrapping u32 sum over w of cum_visits.
 *     regret     = ONE f32 fold from 0.0f of max(cum_regret, 0.0f), edges outer, worlds inner.  The edges come from the keys of a
 *       BTreeMap<Edge, _>, i.e. in kicker::Edge's derived order (edge.rs:18-27): Fold < Check < Call < Open(n) ascending < Raise(Odds)
 *       by the pair (n, d) < Shove.  That is NOT slot order — slots run raises (grid order), Shove, Call, Fold, Check (game.rs:253-283)
 *       — and Odds compare as pairs, not as ratios: (1,1) (1,2) (1,3) (1,4) (2,1) (2,3) (3,1) (3,2) (3,4) (5,4).  refined and visits are
 *       per edge and are reported by slot.
 *     sum_regret as in the depth block, over the exported row order.  drawn[w] = the iterations dealt from world w (they sum to
 *       `iterations`), attempts = the sum of the deals' attempts, fallbacks = the deals that took the fallback.
 *   rows[i][..]: the local profile sorted ascending by (world, kind, past, present, choices).  deals[i][t], t < deals_cap: the deal of
 *   iteration t {hole, world, attempts}; zero past the iterations done.  A solve that fails yields a zero result, no rows and no deals.
 * ADAPT_SAFE.  WorldSolver (world/solver.rs) over NlheEncoder / NlheProfile was read against SubGameSolver with origin = None:
 *   WorldEncoder builds the same keys (prefix edges ++ path into NlheEncoder::resume) and stops at the same nodes (NlheGame keeps the
 *   default is_frontier() = false); WorldProfile<NlheProfile> reads and warm-starts exactly what WorldProfile<DepthView<..>> does for
 *   Game edges, and without a frontier there is no Pick edge; step and harvest are the same text.  So adapt_safe IS the
 *   RP_NLHE_SUBGAME_ORIGIN_NONE answer bit for bit and needs no field of its own.
 * BOUNDS.  As the depth block, with a local profile of up to RP_NLHE_SUBGAME_MAX_ROWS rows (RP_DEPTH_ROWS beyond): the tag splits the
 *   infosets of both seats by world.  The first 64 rows live in LDS, the rest in a region of this entry point's own (168 bytes x 1 984
 *   rows per solve of a launch, at most 1 024 solves per launch).  The deal's loop is bounded by RP_NLHE_MAX_REJECTIONS.  No input
 *   causes an out-of-bounds access or an unbounded loop.
 * Arguments: as the depth solve — args first, without a device (NULL args, iterations outside 1 .. RP_NLHE_DEPTH_MAX_ITERATIONS,
 *   rollouts > 4096, a bias or prior not finite and positive, reserved != 0: RP_ERR_INVALID); then n = 0 is RP_OK without a launch;
 *   then a NULL handle, entries, hole_world, weights or results, rows == NULL with rows_cap > 0 or deals == NULL with deals_cap > 0, is
 *   RP_ERR_INVALID.  The _device form takes every array in DEVICE memory and queues its launches on the handle's stream, so the
 *   outputs of rp_nlhe_belief_device feed it without a host copy. */
#define RP_NLHE_SUBGAME_MAX_ROWS 2048u
#define RP_NLHE_SUBGAME_ORIGIN_NONE 126 /* origin[i]: no frontier (adapt_full / adapt_safe as written) */
typedef struct rp_nlhe_subgame_args { /* one per call */
    uint32_t iterations; /* 1 .. RP_NLHE_DEPTH_MAX_ITERATIONS */
    uint32_t rollouts;   /* as rp_nlhe_depth_args */
    float bias;          /* finite, > 0 */
    float prior;         /* finite, > 0 */
    uint64_t seed, first_id;
    uint32_t rows_cap;   /* local-profile rows exported per solve; 0 = none */
    uint32_t deals_cap;  /* deals traced per solve; 0 = none */
    uint32_t reserved[2]; /* 0 */
} rp_nlhe_subgame_args;  /* 48 bytes */
typedef struct rp_nlhe_subgame_result {
    uint64_t past, choices; /* the key of the entry state's infoset */
    uint32_t present;
    uint8_t n_actions, status, pad[2];
    float refined[9];
    uint32_t visits[9];
    float regret, sum_regret;
    uint32_t iterations, n_rows;
    uint64_t nodes, infosets, frontiers, rollouts;
    uint32_t drawn[4];      /* iterations dealt from each world */
    uint64_t attempts;      /* summed over the deals */
    uint32_t fallbacks, pad2;
} rp_nlhe_subgame_result; /* 176 bytes */
typedef struct rp_nlhe_subgame_row {
    uint8_t kind, n_actions, world, pad; /* kind 0 Game, 1 Pick */
    uint32_t present;
    uint64_t past, choices;
    rp_encounter enc[9];                 /* zero from n_actions on */
} rp_nlhe_subgame_row;    /* 168 bytes */
typedef struct rp_nlhe_subgame_deal {
    uint64_t hole;
    uint8_t world, pad;
    uint16_t attempts;
    uint32_t pad2;
} rp_nlhe_subgame_deal;   /* 16 bytes */
/* rp_nlhe_depth_args_default's values; no rows, no deals */
RP_API void rp_nlhe_subgame_args_default(rp_nlhe_subgame_args* out);
RP_API int rp_nlhe_subgame_solve(rp_nlhe* h, uint64_t n, const rp_nlhe_frontier* entries, const uint8_t* hole_world /* [n][1326] */,
                                 const float* weights /* [n][4] */, const int8_t* origin, const rp_nlhe_subgame_args* args,
                                 rp_nlhe_subgame_result* results, rp_nlhe_subgame_row* rows /* [n][rows_cap] or NULL */,
                                 rp_nlhe_subgame_deal* deals /* [n][deals_cap] or NULL */);
RP_API int rp_nlhe_subgame_solve_device(rp_nlhe* h, uint64_t n, const rp_nlhe_frontier* entries_dev, const uint8_t* hole_world_dev,
                                        const float* weights_dev, const int8_t* origin_dev,
                                        const rp_nlhe_subgame_args* args /* host */, rp_nlhe_subgame_result* results_dev,
                                        rp_nlhe_subgame_row* rows_dev, rp_nlhe_subgame_deal* deals_dev);

/* AIVAT: blueprint control variates per played hand (Aivat::corrections / action_node_correction / chance_node_correction,
 * arena/src/aivat.rs:63-229; strategy_ev / observed_ev, arena/src/correction.rs:4-22; the queries eval_policy / eval_abstraction /
 * eval_chance_correction, arena/src/repository.rs:368-442) — the one consumer of the table's payoff column.  Heads-up.  One hand
 * is the two holes, the board as dealt, the walker's stacks and dealer, the hero seat and the hand's CHOICE plays in order (no
 * Blind, no Draw).  Read-only exactly as rp_nlhe_policy: nothing is inserted, epoch / counters / keys are unchanged, no query can
 * fail a later step.  One wavefront per hand (csrc/nlmc_aivat.hpp).
 *
 * TWO GAMES advance together.
 *   The WALKER (Replayer, arena/src/replay.rs:90-107) is Game::from_start(dealer, stacks) with both holes dealt; the real actions
 *   are applied to it (try_apply).  The WITNESS game is that of Witness::try_arrange(Choice(seat), arrangement, [])
 *   (kicker/src/witness.rs:193-213): stacks [STACK; 2] and dealer 0 WHATEVER THE HAND SAYS.  That difference is the reference's and
 *   is reproduced, not repaired.  The arrangement is the seat's hole plus ALL the board cards the hand carries, so seen().street()
 *   is the hand's last street from the first node on, and sprout (witness.rs:497-505) deals every pending street into the witness as
 *   soon as its head is a chance node below that street.  The reference keeps one witness per seat; they differ only in seen(), so
 *   one witness game serves both.
 * PER PLAY, in this order:  if the walker is terminal, stop (the remaining plays are ignored: no error).  While the walker is at a
 *   chance node: street s needs draws[s] (RP_RECALL_DRAW where it is 0); unless s is preflop, take the CHANCE correction; deal
 *   draws[s] into the walker.  If the walker's turn is `seat`, take the ACTION correction with that seat's hole and ADD it to hero; if
 *   it is the other seat, take it with the other hole and SUBTRACT it from villain.  Push the play onto the witness game (is_allowed,
 *   else the hand is refused: RP_AIVAT_WITNESS where the walker would have accepted the play, RP_RECALL_ILLEGAL where it refuses it
 *   as well), then sprout.  Apply the play to the walker (is_allowed, else RP_RECALL_ILLEGAL).  Streets the walker still has to
 *   deal when the plays run out (an all-in and a call) are not visited.
 * THREE AGGRESSION COUNTS, none of them another's:
 *   history()  (kicker/src/recall.rs:81-100) turns the witness's actions, Draws included, into edges with
 *              state.edgify(action, running.aggression()), where `running` is a Path of the edges so far: Path keeps its FIRST 12
 *              edges (MAX_PATH_EDGES), so from the 13th edge of the hand on that depth no longer changes.
 *   subgame()  (recall.rs:103-112) collects the history's edges since the last Draw into a Path: the FIRST 12 edges of the current
 *              street.  It is the key's `past`, and its aggression() (the raises / shoves among those 12) is the depth of the key's
 *              `choices` = witness head.choices(depth) (nlhe/src/info.rs:117-122); no choices where the head is no decision node.
 *   aggression() (recall.rs:63-70) counts the Raise / Shove ACTIONS since the last Draw, without a cut: the depth the OBSERVED edge is
 *              snapped with, on the WALKER: edge = walker.edgify(action, aggression()) (kicker/src/game.rs:754-766, 813-818: the grid
 *              edge of (street, depth) closest in chips on the walker's pot, the first of equally close ones, Shove where the grid is
 *              empty).
 * ACTION CORRECTION (aivat.rs:197-229).  present = the bucket of (the seat's hole, board): board_mode 0, the reference, takes EVERY
 *   board card the hand carries (the witness's seen()) — before the hand's last street that is a bucket of another street than the
 *   node's, and finds no row; board_mode 1 takes the walker's board at the node, the evaluator one would want.  The infoset
 *   (past, present, choices) is probed: no row, no slots, or Σ_slots weight <= 0 give None.  Otherwise total = Σ w,
 *   ev = Σ (w / total) · payoff, observed = payoff[idx] with idx the first slot whose edge is the observed edge, or ev where no slot
 *   is; the correction is ev - observed.  Slots are the infoset's n_actions; slots past them are never read into a result.
 * CHANCE CORRECTION (aivat.rs:151-195, repository.rs:397-442), at the walker's flop -> turn and turn -> river nodes.  The deals are
 *   the single cards outside hero | villain | board, ascending (HandIterator), 45 or 44.  The walker after a deal says who acts: the
 *   hero seat gives sign +, the other seat sign - and ITS hole as the pocket, anything else None.  past and choices are the witness's
 *   as above (it has sprouted already: past is empty).  Deal d's bucket is that of (pocket, board | d) on the next street; a bucket
 *   without a row DROPS the deal (the inner join), baseline = (Σ_slots w · payoff) / (Σ_slots w) is NULL where Σ_slots w == 0.
 *   avg = (float)((double)(Σ_deals baseline over the non-NULL joined deals) / (double)(number of joined deals, NULL ones included)),
 *   NULL where no joined deal has a value; obs = the observed deal's baseline; either NULL gives None; the correction is
 *   sign · (avg - obs).
 * ARITHMETIC, fixed here where the reference and SQL leave it open: every Σ is an f32 left fold from 0.0f, one rounding per
 *   operation (include/rp_math.h), Σ_slots in slot order, Σ_deals in deal order; w / total, (w / total) · v, w · v and the baseline's
 *   quotient are single f32 operations; avg is the one float8 division above, rounded to f32 — this is the definition whatever
 *   PostgreSQL does with real / bigint.  hero, villain and chance accumulate in f32 in play order; total = (hero + villain) + chance.
 *   NaN payloads are not part of the contract.
 * LOOKUP-TABLE ENCODER: an observation the tables do not hold drops that deal at a chance node (as the join does) and is None at an
 *   action node (as eval_abstraction is); it is never RP_RECALL_LOOKUP here.
 * STATUS per hand: rp_recall_status's values with their meanings, plus RP_AIVAT_WITNESS.  Checked before the replay, in this order:
 *   n_plays above RP_AIVAT_MAX_PLAYS LENGTH; seat > 1, dealer > 1, board_mode > 1, stacks neither 0,0 (= STACK) nor both positive
 *   SEAT; a hole that is not two cards, holes or draws that overlap, draws with wrong popcounts or out of street order CARDS; a kind
 *   that is no rp_aivat_play EDGE.  Then the first refusal of the replay in the order above.  A refused hand yields zero outputs and
 *   its status; the call is still RP_OK and the other hands are answered.  No input causes an out-of-bounds access.
 * Outputs: hero, villain, chance, total [n] f32; n_action, n_chance [n] u8, the nodes that contributed a correction that is not
 *   None; status [n]; n_action, n_chance and status may be NULL.  adjusted = won + total is the caller's (aivat.rs:33-42).
 *   The _device form takes every pointer in DEVICE memory, queues its launches on the handle's stream and returns, ordered exactly
 *   like rp_nlhe_policy_device; the host form stages, launches and synchronises.  n = 0 is RP_OK without a launch. */
#define RP_AIVAT_MAX_PLAYS 48u
typedef enum { RP_PLAY_FOLD = 1, RP_PLAY_CALL = 2, RP_PLAY_CHECK = 3, RP_PLAY_RAISE = 4, RP_PLAY_SHOVE = 5 } rp_aivat_play; /* action.rs:8-16 */
enum { RP_AIVAT_WITNESS = 11 }; /* the default-stack witness game refuses a play the walker accepts; after RP_DEPTH_FRONTIERS */
typedef struct rp_aivat_hand {
    uint64_t hole[2];      /* seat 0, seat 1 */
    uint64_t draws[3];     /* flop / turn / river as dealt; 0 where not dealt */
    int16_t  stacks[2];    /* the walker's starting stacks, both positive (0,0 = STACK) */
    int16_t  chips[RP_AIVAT_MAX_PLAYS]; /* Call / Raise / Shove: the chips the play adds; ignored for Fold / Check */
    uint8_t  kind[RP_AIVAT_MAX_PLAYS];  /* rp_aivat_play; the choice plays only: no Blind, no Draw */
    uint8_t  seat, dealer, n_plays, board_mode;
} rp_aivat_hand;           /* 192 bytes */
RP_API int rp_nlhe_aivat(rp_nlhe* h, uint64_t n, const rp_aivat_hand* hands, float* hero, float* villain, float* chance, float* total,
                         uint8_t* n_action, uint8_t* n_chance, uint8_t* status);
RP_API int rp_nlhe_aivat_device(rp_nlhe* h, uint64_t n, const rp_aivat_hand* hands_dev, float* hero_dev, float* villain_dev,
                                float* chance_dev, float* total_dev, uint8_t* n_action_dev, uint8_t* n_chance_dev, uint8_t* status_dev);
/* Aivat::summarize (aivat.rs:45-61) with ratio and erf of pokerkit/src/metrics.rs:102-119.  Host only, no handle, no device.
 *   n_f = (float)n; won = Σ adjusted; mean = ratio(won, n_f); variance = ratio(Σ (x - mean)(x - mean), n_f);
 *   stderr = ratio(sqrt(variance), sqrt(n_f)); raw = raw_stddev · raw_stddev; adj = (stderr · stderr) · n_f;
 *   reduction = adj > 0 ? raw / adj : 1; pvalue = stderr > 0 ? 2 · erf(-|mean| / stderr) : 1; ratio(a, b) = b > 0 ? a / b : 0.
 *   f32 left folds from 0.0f, every operation rounded on its own, sqrt correctly rounded, erf's exp through rp_glibc_expf
 *   (include/rp_libm_glibc.h).  n = 0 is RP_OK (all ratios 0, reduction 1, pvalue 1); adjusted may then be NULL. */
typedef struct rp_aivat_summary {
    float won, mean, stderr_, reduction, pvalue;
} rp_aivat_summary;
RP_API int rp_aivat_summarize(uint64_t n, const float* adjusted, float raw_stddev, rp_aivat_summary* out);

/* MATCHES: batches of heads-up hands played on the device between two agents, each reading a device-resident blueprint — the
 * producer of the hands rp_nlhe_aivat scores and of the winnings a bb/100 figure is made of.  Reference: the table of
 * parlor/src/engine.rs:48-68, 268-320 seating parlor/src/players/{agent,brain,blueprint,dirac,fish}.rs; the statistics of
 * spar/src/benchmark.rs:122-147.  One lane per hand (csrc/nlmc_match.hpp).  Seat s reads the table of handle hs; h1 == h0 or
 * h1 == NULL: one table serves both seats.  Both handles live on one device and share one encoder (the same lookup tables, or
 * both the hashed encoder).  Read-only on both tables exactly as rp_nlhe_policy: nothing is inserted, epoch / counters / keys are
 * unchanged, a queried table steps like one never queried.
 *
 * IDS AND RANDOM NUMBERS.  The reference deals and samples from the thread RNG: there is nothing of it to reproduce, so the
 *   library's counter contract (include/rp_math.h) is used, on two streams that never mix.  hand_id = first_id + i (wrapping);
 *   deal_id = mirror ? hand_id >> 1 : hand_id.  Card c of a deal is rp_node_hash(seed, 0, deal_id, c), c = 0..8: seat 0's two
 *   cards, seat 1's two, the flop's three, the turn, the river; each is rp_pick_uniform over the popcount of the remaining deck,
 *   the pick-th lowest card, which is then removed (the frontier rollouts' rule).  With mirror and an odd hand_id the two holes are
 *   swapped after dealing: hands 2m and 2m + 1 are one deal seen from both sides.  The board of a deal does not depend on the plays.
 *   Decision d of a hand, d counting from 0 over both seats, reads rp_node_hash(seed, 1, hand_id, d) WHETHER ITS AGENT USES IT OR
 *   NOT, so one seat's agent kind never shifts the other's draws.  A hand's outputs depend on seed, hand_id and the args only,
 *   never on the batch around it: a batch split into calls with matching first_id answers the same bytes.
 * THE GAME.  Game::from_start(dealer, stacks) with both holes; dealer 2 = hand_id & 1; stacks 0,0 = STACK.  At a chance node the
 *   deal's street is applied; the run-out after an all-in and a call is dealt to the end.  draws[s] of the record is street s as
 *   dealt, 0 for a street never reached.
 * THE KEY AT A DECISION is that of Brain::policy on the engine's witness (engine.rs:48-68: Witness::initial_with the real buy-ins
 *   and dealer, the actor's hole and the board dealt so far, the choice actions pushed) — the witness game IS the real game, so
 *   one game is kept.  past = subgame(), choices = head.choices(subgame().aggression()), with the two 12-edge cuts stated above
 *   rp_nlhe_aivat (history()'s running Path, subgame()'s Path); present = the bucket of (the actor's hole, the board at the node).
 * AGENTS (rp_agent_kind).
 *   RP_AGENT_BLUEPRINT (Agent<Blueprint>): RP_DIST_AVERAGED in rp_nlhe_policy's arithmetic, an absent row uniform; then sampled as
 *     WeightedIndex over the BTreeMap<Edge, _>, i.e. in Edge's DERIVED Ord, not in slot order: Draw < Fold < Check < Call <
 *     Open by chips < Raise by Odds' derived (numerator, denominator) tuple order < Shove (kicker/src/edge.rs:18-27,
 *     odds.rs:10-11).  RP_EDGE_ORD_RANKS below is the rank of every edge code in that order.  total = the f32 left fold of the
 *     probabilities from 0.0f in that order; threshold = rp_u01(draw) * total; the first edge with threshold < running sum (the
 *     same fold) is played, the last edge if there is none.
 *   RP_AGENT_DIRAC (Dirac<Blueprint>, nlhe::argmax, nlhe/src/strategy.rs:77-89): the LAST maximal edge in that same order
 *     (Iterator::max_by with ties Equal keeps the later one).
 *   RP_AGENT_FISH (fish.rs): reads no table.  Uniform, by rp_pick_uniform, over legal() in its own order (kicker/src/game.rs:
 *     253-280: raise, shove, call, fold, check) with the shove removed; the raise is Game::raise(), the minimum.
 *   A sampled edge becomes game.actionize(edge) (game.rs:741-751) on the real game.  Agent::sample's other arm (WeightedIndex
 *   failing) cannot be reached with a floored distribution and is not built.  NaN weights are not part of the contract.
 * A REFUSED PLAY.  snap = 0, the engine's rule (engine.rs:295-320): an action that is not is_allowed is rejected and the seat times
 *   out into passive(); the play recorded and applied is passive(), and rejected[i] counts it, saturating at 255.  snap = 1: the
 *   play is game.snap(game.actionize(edge)), as NlheGame::apply and the rollouts have it, and rejected stays 0; a snapped play the
 *   rules still refuse gives the hand RP_RECALL_ILLEGAL as a rollout would (the reference panics).
 * THE RECORD is an rp_aivat_hand rp_nlhe_aivat reads as it is: hole, draws, stacks (as given: 0,0 kept), dealer (the hand's, 0 or
 *   1), seat = hero, board_mode (copied), the choice plays in order — kind, and chips for Call / Raise / Shove, 0 for Fold / Check —
 *   n_plays, and zeros in the plays past n_plays.  won[i] = Settlement::won of seat `hero`, in chips.
 * STATUS per hand: RP_RECALL_OK; RP_RECALL_LOOKUP where the lookup tables do not hold an observation a blueprint or dirac agent
 *   asks for; RP_RECALL_LENGTH where the hand has more than RP_AIVAT_MAX_PLAYS plays — it is still played to its end, won and
 *   rejected are valid and the record holds the first 48 plays with n_plays = 48; RP_RECALL_ILLEGAL for the refused snapped play
 *   above, a decision without choices, or the step bound of the frontier rollouts (12 x 32 768 steps, the same derivation)
 *   reached.  LOOKUP and ILLEGAL give zero outputs: an all-zero record, won 0, rejected 0.  No input causes an out-of-bounds
 *   access or an unbounded loop.
 * THE CALL.  RP_ERR_INVALID, and nothing per hand: NULL h0 or args, agent above RP_AGENT_FISH, dealer > 2, hero > 1, mirror, snap or
 *   board_mode > 1, stacks neither 0,0 nor both positive, reserved != 0, handles on two devices or two encoders.  n = 0 is RP_OK
 *   without a launch.  hands, won, rejected and status may each be NULL.  The _device form takes every output pointer in DEVICE
 *   memory (args stay on the host), queues on h0's stream after an event recorded on h1's stream, and returns without
 *   synchronising; the host form stages, launches and synchronises. */
typedef enum { RP_AGENT_BLUEPRINT = 0, RP_AGENT_DIRAC = 1, RP_AGENT_FISH = 2 } rp_agent_kind;
/* rank of edge code e (kicker/src/edge.rs:101-120: 1 Draw, 2 Fold, 3 Check, 4 Call, 5 Shove, 6..9 Open(2,3,4,5), 10..19
 * Raise(1/4, 1/3, 1/2, 2/3, 3/4, 1/1, 5/4, 3/2, 2/1, 3/1)) in Edge's derived Ord; code 0 is no edge */
#define RP_EDGE_ORD_RANKS {31, 0, 1, 2, 3, 18, 4, 5, 6, 7, 11, 10, 9, 13, 16, 8, 17, 15, 12, 14}
typedef struct rp_nlhe_match_args {
    uint64_t seed, first_id;
    int16_t  stacks[2];     /* every hand starts from these; 0,0 = STACK; else both positive */
    uint8_t  agent[2];      /* rp_agent_kind of seat 0 / seat 1 */
    uint8_t  dealer;        /* 0, 1, or 2 = (hand id & 1) */
    uint8_t  hero;          /* the seat `won` and the record's `seat` speak of */
    uint8_t  mirror;        /* 1: hands 2m and 2m+1 are one deal with the holes swapped */
    uint8_t  snap;          /* 0: the engine's rule for a refused play; 1: game.snap(...) */
    uint8_t  board_mode;    /* copied into the records */
    uint8_t  reserved[5];   /* 0 */
} rp_nlhe_match_args;       /* 32 bytes */
/* seed 0, first_id 0, stacks 0,0, both agents RP_AGENT_BLUEPRINT, dealer 2, hero 0, mirror 0, snap 0, board_mode 1 */
RP_API void rp_nlhe_match_args_default(rp_nlhe_match_args* out);
RP_API int rp_nlhe_match(rp_nlhe* h0, rp_nlhe* h1, uint64_t n, const rp_nlhe_match_args* args /* host */, rp_aivat_hand* hands,
                         int16_t* won, uint8_t* rejected, uint8_t* status);
RP_API int rp_nlhe_match_device(rp_nlhe* h0, rp_nlhe* h1, uint64_t n, const rp_nlhe_match_args* args /* host */,
                                rp_aivat_hand* hands_dev, int16_t* won_dev, uint8_t* rejected_dev, uint8_t* status_dev);
/* The bb/100 statistics of spar/src/benchmark.rs:122-147.  Host only, no handle, no device, f64 as the reference:
 *   x_i = won[i] / (double)B_BLIND (2 chips); total_bb = Σ x, a left fold from 0.0; bb_per_100 = total_bb / n * 100;
 *   mean = total_bb / n; stddev = sqrt(Σ (x - mean)(x - mean) / (n - 1)), 0 with n < 2;
 *   confidence = 1.96 * stddev / sqrt(n) * 100, evaluated left to right.  n = 0: everything 0, won may then be NULL. */
typedef struct rp_match_summary {
    uint64_t hands;
    double   total_bb, bb_per_100, stddev, confidence;
} rp_match_summary;         /* 40 bytes */
RP_API int rp_match_summarize(uint64_t n, const int16_t* won, rp_match_summary* out);

/* TRANSLATION: played hands (chip amounts) to recalls (edges) — the step rp_nlhe_reaches leaves to the caller, on the device.  An
 * rp_aivat_hand exactly as rp_nlhe_match writes it and rp_nlhe_aivat reads it becomes the rp_nlhe_recall of seat pov[i] after the
 * first upto[i] plays, with the key of its head.  Reference: Recall::history() (kicker/src/recall.rs:81-100), which calls
 * Game::translate(action, past.aggression(), &translation, rng) (kicker/src/game.rs:778-811) under one of the three policies of
 * pokerkit/src/translation.rs and translate/lattice.rs; Size::translate (kicker/src/size.rs:48-92); the key of
 * NlheInfo::from((&recall, abstraction)) (nlhe/src/info.rs:117-122).  One lane per hand (csrc/nlmc_translate.hpp).  Read-only on the
 * table exactly as rp_nlhe_policy: nothing is inserted, epoch / counters / keys are unchanged.
 *
 * INPUT.  hole[pov] is two cards; the other seat's hole may be 0 (unknown, as in a hand that ended in a fold), and is checked as
 *   rp_nlhe_aivat checks it where it is not.  board_mode is ignored.  pov == NULL: pov[i] = hands[i].seat; upto == NULL:
 *   upto[i] = hands[i].n_plays.
 * THE REPLAY GAME is the hand's real game, Game::from_start(dealer, stacks) with 0,0 = STACK (Witness::initial_with,
 *   kicker/src/witness.rs:77) — rp_nlhe_aivat's walker, NOT its default-stack witness game.
 * PER PLAY j < upto, in this order:  while the game is at a chance node of street s: draws[s] == 0 gives RP_RECALL_DRAW, otherwise
 *   draws[s] is dealt and a Draw edge appended to the recall's edges and to the running path.  A play at a terminal state, or one
 *   is_allowed refuses, gives RP_RECALL_ILLEGAL.  depth = aggression() of the running path: the FIRST 12 edges of the whole history,
 *   Draws included (MAX_PATH_EDGES), its trailing choice edges that are aggressive (kicker/src/path.rs:32-38) — the `run` count
 *   stated above rp_nlhe_aivat.  edge = TRANSLATE(game before the play, play, depth); it is appended to the recall and to the running
 *   path, and to the street's first-12 path (subgame()).  The play is applied.  After the last included play, while the game is at a
 *   chance node whose street has cards in draws, that street is dealt and a Draw appended (an all-in run-out; the decision at the
 *   start of the next street).  More than RP_NLHE_MAX_HISTORY edges give RP_RECALL_LENGTH, and so does upto > n_plays.
 * TRANSLATE (game.rs:788-810, size.rs:48-92, lattice.rs:118-189).  Fold, Check, Call and Shove map to their edges.  Raise(chips): the
 *   grid is Edge::raises(street, depth); an empty grid (depth above MAX_RAISE_REPEATS) gives Shove.  The cell (preflop, depth 0) is
 *   the OPENING axis: x = (double)chips / 2.0, anchors (double)n over OPENS.  Every other cell is the POT-FRACTION axis:
 *   x = (double)chips / (double)pot, anchors (double)n / (double)d in the cell's ascending order.  f64, one rounding per operation,
 *   nothing contracted.
 *   RP_TRANSLATE_SNAP      the first anchor with minimal |a - x|.
 *   bracket                x <= the first anchor: (first, first); x >= the last: (last, last); otherwise hi = the first anchor not
 *                          < x and lo the one before it.  p = ((b - x) * (1.0 + a)) / ((b - a) * (1.0 + x)), a = lo, b = hi: the
 *                          pseudo-harmonic mapping of Ganzfried and Sandholm.
 *   RP_TRANSLATE_PHARGMAX  lo if the bracket is clamped or p >= 0.5, else hi.
 *   RP_TRANSLATE_HARMONIC  lo if the bracket is clamped or u < p, else hi.
 *   RP_TRANSLATE_SNAP is Translation::Snap, NOT edgify: edgify takes the grid edge nearest IN CHIPS, with Edge::into_chips' truncation.
 *   Dealer 0, stacks 200/200, Raise(5), Call(4), check, check, a turn pot of 12 and Raise(5): edgify answers edge 11 (1/3 pot: the
 *   chip distances tie at |4 - 5| = |6 - 5| and the first wins), Snap answers edge 12 (1/2 pot: 5/12 - 1/3 = 0.08333333333333337,
 *   1/2 - 5/12 = 0.08333333333333331).  rp_nlhe_aivat's and the matches' own histories keep edgify, as their contracts state.
 * RANDOM NUMBERS.  The reference draws from the thread RNG: there is nothing of it to reproduce, so the library's counter contract
 *   (include/rp_math.h) applies: u_j = (double)(rp_node_hash(seed, 3, first_id + i, j) >> 11) * 2^-53, j the index of the play in
 *   the hand, counted whether or not the play is a raise, so that a hand's draws do not depend on its content (rp_node_hash carries
 *   32 random bits, so u is a multiple of 2^-32).  Epoch 3 is a stream no other entry point names.  A hand's outputs depend on
 *   seed, first_id + i and the args only: a batch split into calls with matching first_id answers the same bytes.
 * OUTPUTS per hand, each pointer may be NULL.  recalls[i]: hole = hands[i].hole[pov], draws = the streets the replay dealt (0
 *   elsewhere), stacks, dealer as given, pov, n_edges and the translated edges, zeros past them.  play_edges[i][RP_AIVAT_MAX_PLAYS]:
 *   the edge of each included play without the Draws, 0 past upto.  The head's key: past = the street's first 12 edges;
 *   choices = head.choices(aggression of that path), n_choices their number, both 0 where the head is no decision node;
 *   present = the bucket of (hole, the head's board).
 * STATUS per hand, rp_recall_status.  Checked before the replay, in this order: n_plays above RP_AIVAT_MAX_PLAYS or upto above
 *   n_plays LENGTH; seat, dealer or pov above 1, stacks neither 0,0 nor both positive SEAT; hole[pov] not two cards, a non-zero other
 *   hole not two cards, holes or draws that overlap, draws with wrong popcounts or out of street order CARDS; a kind (of any of the
 *   n_plays plays) that is no rp_aivat_play EDGE.  Then the first refusal of the replay in the order above; last RP_RECALL_LOOKUP
 *   where the lookup-table encoder does not hold (hole, the head's board).  A refused hand yields zero outputs and its status; the
 *   call is still RP_OK and the other hands are answered.  No input causes an out-of-bounds access or an unbounded loop.
 * THE CALL.  RP_ERR_INVALID, and nothing per hand, checked before a device is touched: NULL h or args, kind above
 *   RP_TRANSLATE_PHARGMAX, reserved != 0; then, with n > 0, NULL hands.  n = 0 is RP_OK without a launch.  The _device form takes
 *   every array pointer in DEVICE memory (args stay on the host), queues its launches on the handle's stream and returns, ordered
 *   exactly like rp_nlhe_policy_device; the host form stages, launches and synchronises. */
typedef enum { RP_TRANSLATE_SNAP = 0, RP_TRANSLATE_HARMONIC = 1, RP_TRANSLATE_PHARGMAX = 2 } rp_translation_kind;
typedef struct rp_nlhe_translate_args {
    uint64_t seed, first_id;
    uint8_t  kind;          /* rp_translation_kind */
    uint8_t  reserved[7];   /* 0 */
} rp_nlhe_translate_args;   /* 24 bytes */
/* seed 0, first_id 0, RP_TRANSLATE_SNAP */
RP_API void rp_nlhe_translate_args_default(rp_nlhe_translate_args* out);
RP_API int rp_nlhe_translate(rp_nlhe* h, uint64_t n, const rp_nlhe_translate_args* args /* host */, const rp_aivat_hand* hands,
                             const uint8_t* pov /* [n] or NULL */, const uint8_t* upto /* [n] or NULL */, rp_nlhe_recall* recalls,
                             uint8_t* play_edges /* [n][RP_AIVAT_MAX_PLAYS] */, uint64_t* past, uint32_t* present, uint64_t* choices,
                             uint8_t* n_choices, uint8_t* status);
RP_API int rp_nlhe_translate_device(rp_nlhe* h, uint64_t n, const rp_nlhe_translate_args* args /* host */, const rp_aivat_hand* hands_dev,
                                    const uint8_t* pov_dev, const uint8_t* upto_dev, rp_nlhe_recall* recalls_dev, uint8_t* play_edges_dev,
                                    uint64_t* past_dev, uint32_t* present_dev, uint64_t* choices_dev, uint8_t* n_choices_dev,
                                    uint8_t* status_dev);

/* SEARCH MATCHES: rp_nlhe_match in which a seat may re-solve every postflop decision — Agent<World<Blueprint>>,
 * Agent<World<Depth<Blueprint>>> and their Dirac<..> forms (parlor/src/players/{brain,world,solved,dirac,agent}.rs) — on the device from
 * the deal to the settlement, written as the same rp_aivat_hand records.  It answers "how many bb/100 does search buy over the
 * blueprint".  Rounds of k_nl_search_advance / k_nl_search_compact / k_nl_world / k_nl_subgame (csrc/nlmc_search.hpp).
 *
 * EVERYTHING NOT ABOUT SEARCH IS rp_nlhe_match's CONTRACT, word for word: IDS AND RANDOM NUMBERS (the two counter streams of
 *   match.seed, the deal and the mirror), THE GAME, THE KEY AT A DECISION, AGENTS (the three kinds, Edge's derived order), A REFUSED
 *   PLAY, THE RECORD and the statuses.  Decision d of a hand reads rp_node_hash(match.seed, 1, hand_id, d) whatever its agent does
 *   with it.  With search = {RP_SEARCH_NONE, RP_SEARCH_NONE} the four outputs are the bytes rp_nlhe_match writes.
 * NO Depth<Blueprint>.  adapt_leaf solves from the witness's wipe state, in which both seats hold the hero's cards; the library
 *   refuses that entry (RP_RECALL_CARDS: ENTRY above), and handing the solver the opponent's true hole would make the
 *   agent clairvoyant.  World<Blueprint> (adapt_safe) and World<Depth<Blueprint>> (adapt_full) need no opponent hole and, by the
 *   ADAPT_SAFE paragraph above, answer the same bits: RP_SEARCH_WORLD is both.
 * A SEARCH SEAT.  search[s] = RP_SEARCH_WORLD with agent[s] = RP_AGENT_BLUEPRINT is Agent<World<..>>, with RP_AGENT_DIRAC
 *   Agent<Dirac<World<..>>>, with RP_AGENT_FISH RP_ERR_INVALID.  Before the flop the seat reads its blueprint exactly as
 *   rp_nlhe_match does (Brain::distrib, brain.rs:69-71).  At a postflop decision d of seat s, reading handle hs's table:
 *   1 RECALL = {pov = s, hole = s's cards, draws = the streets dealt so far (0 beyond), stacks and dealer as the hand has them
 *     (stacks as given: 0,0 kept), edges = the hand's whole history(): the edges the witness's counters are made of, Draws included}.
 *   2 BELIEF AND SOLVE.  The belief is what rp_nlhe_belief answers for that recall on hs.  The entry is the rp_nlhe_frontier of
 *     INTEGRATION.md's adapt_full: holes[s] only (the other 0), internal = s, draws, stacks, dealer and edges as the recall, prefix =
 *     the history's trailing choice edges, first 12.  The solve is what rp_nlhe_subgame_solve answers for that one entry with that
 *     belief, origin RP_NLHE_SUBGAME_ORIGIN_NONE (origin_mode 0, the reference as written) or the entry street - 1 (origin_mode 1),
 *     the call's iterations, rollouts, bias and prior, seed = search_seed, and first_id = solve_id = hand_id * 256 + (d & 255),
 *     wrapping — BIT FOR BIT: the search match answers what a caller composing the two public calls gets.
 *   3 FALLBACK to the blueprint's policy (Solved's solve -> None arm), counted in unsolved[i] and coded in the step, the first of:
 *     RP_SEARCH_FALLBACK_LENGTH (4) the history has more than RP_NLHE_MAX_HISTORY edges; RP_SEARCH_FALLBACK_CAP (5) the hand already
 *     asked for RP_NLHE_SEARCH_MAX_SOLVES solves, both seats together — neither asks for a solve; then RP_SEARCH_FALLBACK_BELIEF (1)
 *     the belief's status is not RP_RECALL_OK; RP_SEARCH_FALLBACK_SOLVE (2) the solve's status is not RP_RECALL_OK;
 *     RP_SEARCH_FALLBACK_KEY (3) the result's (past, present, choices) is not the real decision's key — the entry is a replay of
 *     edges and can part from the real chips after an off-grid play (the reference warns of this above subgame_descents).
 *     Codes 4 and 5 are guards no hand has been seen to reach: in 900 000 model hands between blueprint and Dirac seats, stacks up
 *     to 32 767, a seat that could search met at most 21 edges of history and a hand at most 14 such decisions (pot-fraction raises
 *     grow the pot geometrically and a street admits few); with a fish, whose minimum raises grow it linearly, 13 000 hands met at
 *     most 18 and 7, and no bound is claimed (tests/test_nlhe_search_model.py, test_every_case_occurs).
 *   4 BLEND (Solved::blend, solved.rs:133-152), per slot a of the infoset, f32, one rounding per operation, no contraction:
 *     v = (float)visits[a]; w = v / (v + (float)visit_threshold); raw = w * refined[a] + (1.0f - w) * bp[a]; total = max(the left
 *     fold of raw from 0.0f in Edge's derived order, RP_EPSILON); p[a] = raw / total.  bp is the match's RP_DIST_AVERAGED policy
 *     (an absent row uniform).
 *   5 CHOOSE from p by the blueprint agent's WeightedIndex rule in Edge order with the decision's draw, or by Dirac's last-maximal
 *     rule; then actionize, then snap or the rejection rule, as rp_nlhe_match.
 * ORDER INDEPENDENCE.  The pending solves of a round are compacted in an order that is the kernel's business; nothing a hand outputs
 *   depends on it, on n, or on the batch around it: only the explicit solve_id identifies a solve.  A batch split into calls with
 *   matching first_id answers the same bytes.
 * PINNED WHILE THE POT FITS AN int16.  match.stacks are admitted up to 32 767 each, but the CPU models this call is tested against keep
 *   chips in int16, as the reference does: at stacks of 24 000 and of 32 767 each their chips wrap in a solve's tree (a raise over a
 *   shove leaves a negative stack, the next node offers no edge) and they refuse, RP_RECALL_ILLEGAL, solves that this library answers
 *   RP_RECALL_OK and plays.  None of 360 model hands at stacks 600 to 16 384 differed.  Which side matches the reference where
 *   stacks[0] + stacks[1] passes 32 767 is undecided; nothing is tested there.
 * OUTPUTS.  hands, won, rejected, status as rp_nlhe_match; searched[i] = the postflop decisions of search seats, saturating at 255;
 *   unsolved[i] = those that fell back, likewise; both 0 for a hand without outputs.  steps[i][k], k < steps_cap: the hand's search
 *   decisions in decision order — solve_id, the recall and the rp_nlhe_subgame_result as solved (both zero for fallbacks 4 and 5),
 *   the belief's status, bp[9], p[9] (= bp after a fallback), seat, decision, the edge chosen from p, the fallback code — zero past
 *   the hand's search decisions and zero for a hand without outputs.  Any output may be NULL.
 * THE CALL.  The args are checked first, without a device and in this order: rp_nlhe_match's checks of `match`, search > 1, search
 *   on a fish, origin_mode > 1, visit_threshold = 0, rp_nlhe_subgame_solve's checks of iterations / rollouts / bias / prior,
 *   reserved0 != 0, steps == NULL with steps_cap > 0 — RP_ERR_INVALID; then n = 0 is RP_OK without a launch; then a NULL h0, or
 *   handles on two devices or two encoders, RP_ERR_INVALID.  BOTH forms return when the match is finished: unlike
 *   rp_nlhe_match_device, the _device form synchronises h0's stream — once per round, to read the round's count of solves — and only
 *   keeps the outputs in DEVICE memory (args stay on the host).  Hands are played in chunks of 1 024, each chunk in at most
 *   RP_NLHE_SEARCH_MAX_SOLVES + 2 rounds (every round but the last serves at least one solve of every unfinished hand; a chunk that
 *   needs more is RP_ERR_HIP, not a spin).  SCRATCH is bounded independently of n by the chunk: about 2.4 KB per hand in flight plus
 *   rp_nlhe_subgame_solve's overflow rows (168 bytes x 1 984 rows per solve of a launch), at most 345 MB; grow-only on h0, freed
 *   with it.  Read-only on both tables exactly as rp_nlhe_policy. */
typedef enum { RP_SEARCH_NONE = 0, RP_SEARCH_WORLD = 1 } rp_search_kind;
typedef enum {
    RP_SEARCH_SOLVED = 0, RP_SEARCH_FALLBACK_BELIEF = 1, RP_SEARCH_FALLBACK_SOLVE = 2, RP_SEARCH_FALLBACK_KEY = 3,
    RP_SEARCH_FALLBACK_LENGTH = 4, RP_SEARCH_FALLBACK_CAP = 5
} rp_search_fallback;
#define RP_NLHE_SEARCH_MAX_SOLVES 48u /* per hand, both seats together */
typedef struct rp_nlhe_search_args {
    rp_nlhe_match_args match; /* every field with rp_nlhe_match's meaning and checks */
    uint64_t search_seed;     /* the seed of every solve; never mixed with match.seed's two streams */
    uint32_t iterations;      /* 1 .. RP_NLHE_DEPTH_MAX_ITERATIONS: stands in for the reference's 5 s deadline */
    uint32_t rollouts;        /* as rp_nlhe_subgame_args */
    float    bias, prior;     /* as rp_nlhe_subgame_args */
    uint32_t visit_threshold; /* SubgameHyperParams::visit_threshold, >= 1 */
    uint32_t steps_cap;       /* traced search decisions per hand, 0 = none */
    uint8_t  search[2];       /* rp_search_kind of seat 0 / seat 1 */
    uint8_t  origin_mode;     /* 0: RP_NLHE_SUBGAME_ORIGIN_NONE; 1: origin = the entry street - 1 */
    uint8_t  reserved0[5];    /* 0 */
} rp_nlhe_search_args;        /* 72 bytes */
typedef struct rp_nlhe_search_step {
    uint64_t solve_id;
    rp_nlhe_recall recall;
    rp_nlhe_subgame_result result;
    float    bp[9], p[9];
    uint32_t decision;        /* d, counting from 0 over both seats */
    uint8_t  seat, edge, fallback /* rp_search_fallback */, belief_status;
} rp_nlhe_search_step;        /* 352 bytes */
/* rp_nlhe_match_args_default's match, no search seat, origin_mode 0, rp_nlhe_subgame_args_default's iterations / rollouts / bias /
 * prior, visit_threshold 1 << 18, no trace, search_seed 0 */
RP_API void rp_nlhe_search_args_default(rp_nlhe_search_args* out);
RP_API int rp_nlhe_search_match(rp_nlhe* h0, rp_nlhe* h1, uint64_t n, const rp_nlhe_search_args* args /* host */, rp_aivat_hand* hands,
                                int16_t* won, uint8_t* rejected, uint8_t* status, uint8_t* searched, uint8_t* unsolved,
                                rp_nlhe_search_step* steps /* [n][steps_cap] or NULL */);
RP_API int rp_nlhe_search_match_device(rp_nlhe* h0, rp_nlhe* h1, uint64_t n, const rp_nlhe_search_args* args /* host */,
                                       rp_aivat_hand* hands_dev, int16_t* won_dev, uint8_t* rejected_dev, uint8_t* status_dev,
                                       uint8_t* searched_dev, uint8_t* unsolved_dev, rp_nlhe_search_step* steps_dev);

/* THE BLUEPRINT CENSUS: what the table says AS A WHOLE — TrainingAPI::stats, street_stats, saturation, cold and hot
 * (crates/portal/src/training/api.rs:74-286) and StrategyAPI::grid_usage (crates/portal/src/strategy/api.rs:196-245), each a full scan
 * of the blueprint table with a GROUP BY in the reference.  One read-only scan of the device-resident table fills one rp_census
 * record (k_nl_census_scan / k_nl_census_fold, csrc/nlmc_census.hpp); pure host functions turn the record into the reference's
 * response shapes, as rp_match_summarize does for matches.
 * NAMES.  rp_nlhe_census (include/rp_mi355x_diag.h) is the profiled steps' node census and stays what it is: the scan is
 *   rp_nlhe_table_census, its record rp_census, and the summaries' output types are rp_census_totals / _street / _peaks / _grid.
 * A ROW of the SQL table is one (infoset, action a) pair, a < n_actions = the consecutive non-zero 5-bit groups of `choices`, at most
 *   9, as everywhere in this header; its edge is the 5-bit code of group a, its street min(present >> 8, 4) — index 4 collects what the
 *   reference prints as "unknown".  An infoset without actions has no row: it is in no count and in no list.
 * THE RECORD.  cell[street][edge code] (code 0 stays empty), infosets[street] = COUNT(DISTINCT (past, present, choices)), epoch, slots
 *   = the table's capacity, and two ranked lists of n_cold = n_hot = min(RP_NLHE_CENSUS_TOP, infosets) entries:
 *   cold: value MIN(visits) over the infoset's actions, ascending; hot: value MAX(regret), ordered by MAX(ABS(regret)) descending;
 *   ties in either by (past, present, choices) ascending as unsigned integers — total orders.  An entry carries past, choices, present,
 *   edges = n_actions and its value: `visits` in the cold list (regret 0), `regret` in the hot list (visits 0); entries past n are zero.
 *   Per cell: rows = COUNT(*); rated = rows whose decision total is not zero (the denominator of AVG, which skips NULLs); dominant =
 *   rated rows with ratio > 0.5f; visits = the exact sum; ratio, weight, total, regret, payoff = double sums; five f32 and two u32
 *   extremes.  A cell with rows == 0 is all zero.
 * THE ARITHMETIC, bit for bit (tests/nlhe_census_model.py follows it with explicit loops):
 *   Per infoset: dec_total = the f32 left fold of weight[0 .. n_actions) from 0.0f in action order (SUM(weight) OVER (PARTITION BY
 *     past, present, choices)); per action ratio = weight[a] / dec_total in f32, one rounding.  With dec_total == 0.0f (either sign)
 *     the row counts in rows, is not rated and adds nothing to ratio.  Row bytes at a >= n_actions reach no result.
 *   Float sums: every term is converted to f64 (exact) and added in f64.  Within a SEGMENT of RP_NLHE_CENSUS_SEGMENT consecutive
 *     slots: a left fold from +0.0 over the ready slots in ascending slot index and, within a slot, the actions in ascending a.  The
 *     table's sum: the left fold from +0.0 of the segment sums in ascending segment index.  A table of at most 65 536 slots is one
 *     plain left fold.  Two actions of one infoset with the same edge code (imported tables may hold such) both land in the cell,
 *     in action order.  `total` adds dec_total once per row, rated or not.
 *   Counts, visits, extremes and the lists do not depend on any order.  Extremes compare as values; the sign of a zero extreme is
 *     unspecified.  NaN is outside the contract, as for every NLHE call.
 * DEPARTURES FROM THE SQL.  Postgres accumulates SUM(real) in f32 in scan order, so weighted_freq and dec_total have no defined bits
 *   in the reference: here weighted_freq = (float)(weight / total) of the f64 sums.  AVG(visits::float4) rounds every row to f32: here
 *   the sum of visits is exact.  Postgres sorts NULL first under DESC: here a cell without a rated row sorts last in its street.
 * THE CALLS.  NULL h or out is RP_ERR_INVALID before any device work.  rp_nlhe_table_census stages, launches and synchronises;
 *   _device takes `out` in DEVICE memory, queues on the handle's stream — after every earlier step and import — and returns.  The scan
 *   reads 32 bytes per slot and 144 bytes per READY slot and writes only its own scratch (about 21 KB per segment, grow-only on the
 *   handle, freed with it) and the record, every byte of it: the table, epoch, counters and keys are unchanged.
 * THE SUMMARIES.  Host only, no handle, no device.  Sums over cells are f64 left folds from +0.0 over street then code ascending,
 *   averages one division in f64 and one cast to f32; a NULL argument is RP_ERR_INVALID.
 *   rp_census_stats (ApiBlueprintStats): infosets, edges = rows, avg = sum / edges, extremes over the non-empty cells; avg_visits =
 *     (float)((double)visits / edges); everything 0 with edges == 0.
 *   rp_census_street_stats (ApiStreetStats): five entries, street 'P' 'F' 'T' 'R' '?', the same per street; a street without rows zero.
 *   rp_census_saturation (ApiSaturation): max_weight, max_regret = MAX(ABS(regret)), max_payoff = MAX(ABS(payoff)), max_visits,
 *     precision_f32 = FLT_MAX, weight_pct = max_weight / precision_f32 * 100.0f and regret_pct likewise, in f32 left to right.
 *   rp_census_grid_usage (ApiGridUsage): the non-empty cells — avg_freq = (float)(ratio / rated), 0 with rated == 0; weighted_freq =
 *     (float)(weight / total), 0 with total == 0; n_decisions_with_edge = rows; n_dominant — ordered by street ascending, then cells
 *     with a rated row before those without, then avg_freq descending, then edge code ascending.  rows: room for 160; *n = written. */
#if defined(__cplusplus)
#define RP_STATIC_ASSERT(cond, name) static_assert(cond, #name)
#else
#define RP_STATIC_ASSERT(cond, name) _Static_assert(cond, #name)
#endif
#define RP_NLHE_CENSUS_TOP 64u
#define RP_NLHE_CENSUS_SEGMENT 65536u
#define RP_NLHE_CENSUS_STREETS 5u
#define RP_NLHE_CENSUS_CODES 32u
typedef struct rp_census_cell {
    uint64_t rows, rated, dominant, visits;
    double   ratio, weight, total, regret, payoff;
    float    max_regret, min_regret, max_weight, max_payoff, min_payoff;
    uint32_t max_visits, min_visits;
    uint32_t reserved;      /* 0 */
} rp_census_cell;           /* 104 bytes */
typedef struct rp_census_entry {
    uint64_t past, choices;
    uint32_t present, edges;
    uint32_t visits;        /* cold: MIN(visits) */
    float    regret;        /* hot: MAX(regret) */
} rp_census_entry;          /* 32 bytes */
typedef struct rp_census {
    rp_census_cell  cell[RP_NLHE_CENSUS_STREETS][RP_NLHE_CENSUS_CODES];
    uint64_t        infosets[RP_NLHE_CENSUS_STREETS];
    uint64_t        epoch, slots;
    uint32_t        n_cold, n_hot;
    rp_census_entry cold[RP_NLHE_CENSUS_TOP], hot[RP_NLHE_CENSUS_TOP];
} rp_census;                /* 20800 bytes */
typedef struct rp_census_totals {
    uint64_t infosets, edges;
    float    avg_regret, max_regret, min_regret, avg_weight, max_weight, avg_payoff, max_payoff, min_payoff, avg_visits;
    uint32_t max_visits, min_visits;
    uint32_t reserved;      /* 0 */
} rp_census_totals;         /* 64 bytes */
typedef struct rp_census_street {
    uint64_t infosets, edges;
    float    avg_regret, avg_weight, avg_payoff, avg_visits;
    char     street;        /* 'P' 'F' 'T' 'R' '?' */
    uint8_t  reserved[7];   /* 0 */
} rp_census_street;         /* 40 bytes */
typedef struct rp_census_peaks {
    float    max_weight, max_regret, max_payoff;
    uint32_t max_visits;
    float    precision_f32, weight_pct, regret_pct;
    uint32_t reserved;      /* 0 */
} rp_census_peaks;          /* 32 bytes */
typedef struct rp_census_grid {
    uint64_t n_decisions_with_edge, n_dominant;
    float    avg_freq, weighted_freq;
    uint8_t  street, edge;  /* 0..4, the 5-bit edge code */
    uint8_t  reserved[6];   /* 0 */
} rp_census_grid;           /* 32 bytes */
RP_STATIC_ASSERT(sizeof(rp_census_cell) == 104, rp_census_cell_is_104_bytes);
RP_STATIC_ASSERT(sizeof(rp_census_entry) == 32, rp_census_entry_is_32_bytes);
RP_STATIC_ASSERT(sizeof(rp_census) == 20800, rp_census_is_20800_bytes);
RP_STATIC_ASSERT(sizeof(rp_census_totals) == 64, rp_census_totals_is_64_bytes);
RP_STATIC_ASSERT(sizeof(rp_census_street) == 40, rp_census_street_is_40_bytes);
RP_STATIC_ASSERT(sizeof(rp_census_peaks) == 32, rp_census_peaks_is_32_bytes);
RP_STATIC_ASSERT(sizeof(rp_census_grid) == 32, rp_census_grid_is_32_bytes);
#undef RP_STATIC_ASSERT /* this header's own: not part of the API */
RP_API int rp_nlhe_table_census(rp_nlhe* h, rp_census* out);
RP_API int rp_nlhe_table_census_device(rp_nlhe* h, rp_census* out_dev);
RP_API int rp_census_stats(const rp_census* c, rp_census_totals* out);
RP_API int rp_census_street_stats(const rp_census* c, rp_census_street* out /* [5] */);
RP_API int rp_census_saturation(const rp_census* c, rp_census_peaks* out);
RP_API int rp_census_grid_usage(const rp_census* c, rp_census_grid* rows /* [160] */, uint32_t* n);

/* Multi-GPU (BASELINE configs[3]): trees sharded by rank (rank r samples tree ids [r*B, (r+1)*B) of a world*B-tree epoch
 * against a replicated table).  step_local: this rank's traversal reduced to one composed entry per infoset touched
 * (rp_profile_summarize's records, entry_bytes each, at most max_entries) plus the infoset KEY of every entry — each
 * rank's table assigns rows in its own insertion order, so the exchange is by key; the caller all-gathers entries and keys
 * (rank-major, packed); step_apply maps the keys to this table's rows (inserting unseen infosets with their default
 * regrets) and folds in rank order, epoch += 1.  Replicas stay identical as key -> Encounter maps.  Oracle:
 * ora_nlmc_step_world. */
RP_API int rp_nlhe_set_shard(rp_nlhe* h, uint32_t rank, uint32_t world);
RP_API int rp_nlhe_entry_bytes(rp_nlhe* h, size_t* bytes, uint32_t* max_entries);
RP_API int rp_nlhe_step_local(rp_nlhe* h, void* entries_dev, uint64_t* past_dev, uint32_t* present_dev, uint64_t* choices_dev,
                              uint32_t* n_entries);
RP_API int rp_nlhe_step_apply(rp_nlhe* h, void* entries_dev, const uint64_t* past_dev, const uint32_t* present_dev,
                              const uint64_t* choices_dev, uint32_t n_entries);
/* the whole sharded step over the library's own RCCL communicator (rp_comm, below): step_local, the ranks' entry counts
 * (the one host read of a step: ncclAllGather takes host-known sizes), entries + keys gathered padded to the longest list,
 * packed rank-major on the device, step_apply; `steps` times.  Sets the shard from the communicator's rank / world. */
RP_API int rp_nlhe_step_comm(rp_nlhe* h, rp_comm* c, uint32_t steps);
/* every rp_nlhe kernel runs on ONE stream (the profile's): hand it the stream the collectives run on and the exchange is
 * ordered without host synchronisation (NULL = back to a stream of the library's own); rp_nlhe_sync waits for it.
 * step_local returns with *n_entries valid and the key arrays QUEUED on that stream. */
RP_API int rp_nlhe_set_stream(rp_nlhe* h, void* hip_stream);
RP_API int rp_nlhe_sync(rp_nlhe* h);

/* ===================================================================== lloyd ==
 * crates/elkan: Elkan<K,N> (elkan.rs:27-207), Bounds (bounds.rs:19-120), Prior::tally (prior.rs:35-47)
 * crates/lloyd: Layer (layer.rs:23-273), Kmeans (kmeans.rs:29-111), Sinkhorn (sinkhorn.rs:62-230),
 *               Metric::emd (metric.rs:109-115), Equity::variation (equity.rs:41-53)
 * crates/monge: Coupling::{minimize, flow, cost} (coupling.rs:23-51)
 */
typedef enum rp_metric_kind {
    RP_METRIC_SINKHORN = 0, /* Histogram over Flop/Turn buckets -> Sinkhorn::divergence */
    RP_METRIC_VARIATION = 1 /* Histogram over river equity bins -> Equity::variation    */
} rp_metric_kind;

/* SinkhornHyperParams::DEFAULT {0.025, 128, 5e-4} (lloyd/src/hyperparams/sinkhorn.rs:17-23) */
typedef struct rp_sinkhorn_hp {
    float temperature;
    uint32_t iterations;
    float tolerance;
} rp_sinkhorn_hp;
RP_API void rp_sinkhorn_hp_default(rp_sinkhorn_hp* out);

/* Pair::merge (lloyd/src/pair.rs:58-65): triangular index of an unordered bin pair, i != j */
static inline uint32_t rp_tri_index(uint32_t i, uint32_t j) {
    uint32_t lo = i < j ? i : j, hi = i < j ? j : i;
    return hi == 0 ? 0 : hi * (hi - 1) / 2 + lo;
}

typedef struct rp_kmeans rp_kmeans;

/* Layer::build (layer.rs:250-272): K clusters over N points, each a dense histogram of `bins` u8 counts
 * (Bins<N>, bins.rs:30-37; reference stores usize counts, point mass <= 47 so u8 is lossless).
 * `tri_metric` is Metric's triangular table bins*(bins-1)/2 (metric.rs:26-55) for RP_METRIC_SINKHORN,
 * NULL for RP_METRIC_VARIATION.  `counts` is a host pointer; use the _device variant when the
 * histograms already live in HBM. */
RP_API int rp_kmeans_create(uint32_t K, uint64_t N, uint32_t bins, const uint8_t* counts, rp_metric_kind kind,
                            const float* tri_metric, const rp_sinkhorn_hp* hp, uint64_t seed, int device,
                            rp_kmeans** out);
RP_API int rp_kmeans_create_device(uint32_t K, uint64_t N, uint32_t bins, const void* counts_dev,
                                   rp_metric_kind kind, const float* tri_metric, const rp_sinkhorn_hp* hp,
                                   uint64_t seed, int device, rp_kmeans** out);
RP_API int rp_kmeans_destroy(rp_kmeans* h);
/* Elkan::init_centroids = k-means++ (layer.rs:140-181); chosen[] receives the K point indices (may be NULL) */
RP_API int rp_kmeans_init_centroids(rp_kmeans* h, uint64_t* chosen);
/* rp_rng_kind of rp_kmeans_init_centroids.  RP_RNG_REFERENCE = Layer::init_centroids' own chain (crates/lloyd/src/layer.rs:155-178):
 * DefaultHasher over the Street (`street` = its discriminant: 0 Pref, 1 Flop, 2 Turn, 3 Rive; deuce/src/street.rs:21-27) ->
 * SmallRng::seed_from_u64, ONE generator for the K picks, each pick WeightedIndex::<f32>::new(potentials).sample(rng): f32
 * running sums in index order (sequential by definition: one wavefront, ~4 ns per point), x = Uniform::new(0, total).sample,
 * partition_point (include/rp_refrng.h).  `seed` is not used in this mode.  The running sum is sequential, but between two powers
 * of two it is integer arithmetic (csrc/kpp_refpick.hpp), and a point-sharded layer continues it across ranks, per pick:
 *   1. rank 0: rp_kmeans_kpp_ref_walk(h, 0.0f, &end); rank r > 0 receives rank r-1's end, walks from it, hands its own end on
 *   2. the last rank's end is the reference's total_weight: broadcast it
 *   3. every rank: rp_kmeans_kpp_ref_draw(h, total, &x) (each rank's generator advances alike; K draws from ONE seed)
 *   4. the owner is the first rank whose end exceeds x (the last rank if none does: partition_point's fallback)
 *   5. the owner: rp_kmeans_kpp_ref_pick(h, x, &index); its point's histogram goes to every rank (rp_kmeans_get_point)
 *   6. every rank: rp_kmeans_set_centroid(h, k, histogram), rp_kmeans_kpp_update(h, k)
 * One f32 handed on per rank per pick; the picks are the single layer's bit for bit (tests/test_gpu_sharded_refdraw.py). */
RP_API int rp_kmeans_set_rng(rp_kmeans* h, rp_rng_kind kind, int street);
/* Which exp / ln the Sinkhorn distances compute with.
 *   RP_LIBM_CONTRACT  (default) include/rp_math.h's rp_expf / rp_logf: f32 only, packed and pipelined in the softmin loops,
 *                     <= 1 ulp from glibc's on the Sinkhorn's domain.
 *   RP_LIBM_GLIBC     glibc's expf / logf as a Rust build on Linux calls them (f32::exp / f32::ln, sinkhorn.rs:115,120-127,136;
 *                     phi.rs:36), restated in include/rp_libm_glibc.h (equal to glibc 2.35's on all 2^32 inputs) and evaluated in
 *                     double on the device: every distance, bound, drift and bucket is the reference's, bit for bit, at a few
 *                     times the cost (every kernel that evaluates exp / ln exists in both arithmetics: csrc/lloyd_kernels.hpp).
 * What the default's <= 1 ulp is worth is measured (costs within 7 ulps, no k-means++ pick and no bucket moves). */
typedef enum rp_libm_kind { RP_LIBM_CONTRACT = 0, RP_LIBM_GLIBC = 1 } rp_libm_kind;
/* a layer: call before the first centroid exists (recomputes the points' self costs).  One way only.  The three filters in front of
 * the bit-faithful solves — the k-means++ column bound, the k-means++ interval filter, the MFMA bound of the neighbor passes — stay
 * in place: their margins (4e-5 relative, 4e-6 absolute) sit three orders above the <= 7 ulps between the two arithmetics, and the
 * full flop layer has been audited in both (profiles/r05_glibc_audit.json, profiles/r03_mfma_audit.json: 0 of 1 286 792 points differ
 * from the unpruned search).  rp_kmeans_set_prune(h, 0) runs every distance through the bit-faithful kernel instead.
 * Host assumption of RP_LIBM_GLIBC ("bit for bit with a Rust build"): x86-64 glibc whose expf is the FMA variant (the ifunc every
 * AVX2 machine selects); rp_libm_glibc.h restates that one, and tests/test_libm_glibc.py compares it with the platform's libm. */
RP_API int rp_kmeans_set_libm(rp_kmeans* h, rp_libm_kind kind);
/* enable = 0: no filter in front of the exact solves (Elkan::neighbor / Layer::init_centroids as the reference loops them, every
 * (point, centroid) pair solved, every stale-bound refresh solved): the yardstick the filtered passes are audited against.  Before
 * the first centroid; a layer that gave its filters up does not get them back (enable = 1 on such a layer: RP_ERR_UNSUPPORTED).
 *
 * WHAT THE FILTERED PASSES GUARANTEE — read before relying on "bit-exact buckets" through them.  The four filters (k-means++ column
 * bound and interval filter, the MFMA bound of init_bounds / lookup, the interval-decided refresh of the Elkan iterations) replace a
 * bit-faithful solve by a scaling-domain INTERVAL that must contain the value the reference would compute.  The column bound is
 * rigorous, and so is the rule by which the MFMA bound skips cost evaluations inside a stopping window (round 6: a Lipschitz bound of
 * <P, C> in the coupling's L1 travel, exact arithmetic, applied only to columns that cannot be the argmin either way), and so is the
 * rule by which a far column (MFMA bound) or a far pair (k-means++ interval filter) LEAVES before its stopping window closes (round 6:
 * weak duality for a Kantorovich pair read off the iterate, f = T ln u with g = -T ln K^T u or f's c-transform, plus the L1 error of the
 * row marginals, which never grows; float slack only — csrc/sinkhorn_bound.hpp "THE DUAL EXIT").  The intervals of the columns that are
 * followed to the end are not proven: their margins (SbParams: kappa, rho, dc_abs 4e-6, dc_rel 4e-5) are a multiple of the worst
 * float noise MEASURED between the scaling-domain and the log-domain iteration, and the smallest slack observed on a sampled pair was
 * 0.88 of the margin (profiles/r05_glibc_audit.json), i.e. a safety factor of about 8 over the worst observed case, on synthetic
 * points.  The evidence that they hold: full-size audits in both arithmetics with 0 of 1 286 792 points differing from the unpruned
 * search on the synthetic layer (profiles/r05_glibc_audit.json, r05_kpp_audit*.json) and on the real flop layer (r03_mfma_audit.json),
 * 0 differences over 32 Elkan iterations with and without the refresh bound (profiles/r06_refresh_audit_*.json; all of them again
 * after the dual exits: profiles/r06p_*audit*.json, 0 of 2 573 584 audited points in each of the four), and a runtime
 * tripwire: every 521st point is searched again without the MFMA prune after every pruned pass (and every 521st point a k-means++ round's
 * interval filter drops is solved anyway and its bound compared with the exact distance), a mismatch makes the next call that
 * hands results out fail with RP_ERR_INTERNAL (never a silently different bucket).  That is a statistical claim with a tripwire, not a
 * bound: a caller that needs exactness BY CONSTRUCTION uses rp_kmeans_set_prune(h, 0), the only such mode (and RP_LLOYD_AUDIT=1 runs
 * the unpruned search behind every pruned pass and counts disagreements). */
RP_API int rp_kmeans_set_prune(rp_kmeans* h, int enable);
/* the three stand-alone operators (rp_sinkhorn_divergence / _cost / _flow): process-wide */
RP_API int rp_sinkhorn_set_libm(rp_libm_kind kind);
/* install centroids = copies of the given points (TestLayer-style explicit seeding, tests.rs:100-102) */
RP_API int rp_kmeans_set_centroids(rp_kmeans* h, const uint64_t* point_index);
/* install / read one centroid as an integer histogram (counts[bins] u32): resume, and the multi-GPU
 * k-means++ where the chosen point lives on another rank */
RP_API int rp_kmeans_set_centroid(rp_kmeans* h, uint32_t k, const uint32_t* counts);
RP_API int rp_kmeans_get_point(rp_kmeans* h, uint64_t index, uint32_t* counts);
/* k-means++ (layer.rs:140-181) one primitive at a time, so a point-sharded job can interleave collectives:
 *   kpp_begin   potentials <- 1, centroids cleared
 *   kpp_total   this shard's sum of quantised potentials (exact u64, rp_math.h rp_kpp_quant)
 *   kpp_pick    first local i whose inclusive quantised prefix exceeds r; its potential <- 0
 *   kpp_update  potentials <- min(potentials, distance(centroid k, point)^2)
 * rp_kmeans_init_centroids is exactly: for k in 0..K { total; r = mulhi64(rp_stream(seed,k), total); pick;
 * set_centroid(k, point); update(k) }. */
RP_API int rp_kmeans_kpp_begin(rp_kmeans* h);
RP_API int rp_kmeans_kpp_total(rp_kmeans* h, uint64_t* total);
RP_API int rp_kmeans_kpp_pick(rp_kmeans* h, uint64_t r, uint64_t* index);
RP_API int rp_kmeans_kpp_update(rp_kmeans* h, uint32_t k);
/* The same family after rp_kmeans_set_rng(h, RP_RNG_REFERENCE, street) and rp_kmeans_kpp_begin, which in that mode also seeds the
 * handle's SmallRng from the street exactly as rp_kmeans_init_centroids does (the protocol: at rp_kmeans_set_rng); without those
 * two calls RP_ERR_INVALID, the message names the missing one.
 * ref_walk: this shard's potentials walked in index order from the exact running sum in front of it (0.0f on the first shard) */
RP_API int rp_kmeans_kpp_ref_walk(rp_kmeans* h, float prefix_in, float* prefix_out);
/* every rank, once per pick, with the LAST shard's prefix_out: advances the handle's SmallRng by one u32 and returns
 * x = value0_1 * UniformFloat::new(0, total).scale + 0 (rp_refrng.h).  total == 0 (or not > 0): RP_ERR_INVALID ("the reference
 * panics here"), the generator still advanced identically on all ranks */
RP_API int rp_kmeans_kpp_ref_draw(rp_kmeans* h, float total, float* x);
/* after ref_walk with unchanged potentials: the first local index whose running sum exceeds x, its potential <- 0;
 * *index = N if none does (nothing written) */
RP_API int rp_kmeans_kpp_ref_pick(rp_kmeans* h, float x, uint64_t* index);
/* Elkan::init_bounds (elkan.rs:39-47) */
RP_API int rp_kmeans_init_bounds(rp_kmeans* h);
/* Kmeans::next (kmeans.rs:82-110): step_elkan (elkan.rs:153-168), install centroids, Prior::tally.
 * drift[K], sizes[K], reassigned may be NULL. */
RP_API int rp_kmeans_step(rp_kmeans* h, float* drift, uint64_t* sizes, double* reassigned);
/* Elkan::step_naive (elkan.rs:171-188) + install */
RP_API int rp_kmeans_step_naive(rp_kmeans* h);
/* Layer::lookup (layer.rs:62-82): fresh neighbor(i) for every point; bucket[N], distance[N] (may be NULL) */
RP_API int rp_kmeans_assign(rp_kmeans* h, uint8_t* bucket, float* distance);
/* current Elkan bounds: j[N] (u8), upper[N]; lower[N*K] may be NULL.  With the interval-decided refresh (the default for Sinkhorn
 * layers whose filters are on; csrc/refresh_bound.hpp) upper[i] may be the UPPER END of an interval around the reference's
 * Bounds::error and lower[i][j[i]] its lower end: rp_kmeans_upper_interval (rp_mi355x_diag.h) says where and returns the lower ends.
 * j[], and lower[i][k] for k != j[i], are the reference's bit for bit in every mode; after rp_kmeans_set_prune(h, 0) so is everything. */
RP_API int rp_kmeans_bounds(rp_kmeans* h, uint8_t* j, float* upper, float* lower);
/* centroids as integer sums: counts[K*bins] (u32), weight[K] (u64) (histogram.rs:286-294, bins.rs:75-82) */
RP_API int rp_kmeans_centroids(rp_kmeans* h, uint32_t* counts, uint64_t* weight);
/* Layer::metric (layer.rs:85-101) + Metric::from(BTreeMap) normalisation (metric.rs:127-141): tri[K*(K-1)/2] */
RP_API int rp_kmeans_metric(rp_kmeans* h, float* tri);
/* Elkan::rms (elkan.rs:191-200), summed in point order */
RP_API int rp_kmeans_rms(rp_kmeans* h, float* out);
/* number of distance evaluations so far (Sinkhorn/variation calls incl. self terms), for reporting */
RP_API int rp_kmeans_stats(rp_kmeans* h, uint64_t* distances, uint64_t* sinkhorn_iterations);
/* exp evaluations spent in Sinkhorn softmin / cost loops so far: sum over solves of (2*iterations + 1) * m * n */
RP_API int rp_kmeans_exp_evals(rp_kmeans* h, uint64_t* evals);
/* The MFMA Sinkhorn bound in front of the N x K neighbor passes of a Sinkhorn layer (init_bounds, assign, step_naive):
 * a scaling-domain iteration u = mu ./ (K v), v = nu ./ (K^T u), K = exp(-C/T), on v_mfma_f32_16x16x4_f32 gives every
 * (point, centroid) pair an interval that contains the value Sinkhorn::divergence (sinkhorn.rs:166-171) returns; the
 * centroids whose lower bound exceeds the smallest upper bound are discarded and the bit-faithful kernel runs on the
 * survivors only, in ascending centroid order — buckets, distances and tie-breaks are those of the unpruned loop
 * (elkan.rs:68-77).  Environment: RP_LLOYD_NO_MFMA_BOUND=1 switches it off; RP_LLOYD_AUDIT=1 also runs the unpruned
 * pass and counts the points on which the two disagree (audit_mismatches; must stay 0). */
typedef struct rp_prune_stats {
    uint32_t enabled;          /* 0: the layer runs every distance through the bit-faithful kernel */
    uint32_t reserved;
    uint64_t points;           /* points that went through the bound (all neighbor passes so far) */
    uint64_t candidates;       /* points * K */
    uint64_t survivors;        /* (point, centroid) pairs handed to the bit-faithful kernel */
    uint64_t block_iterations; /* MFMA work: iterations of a 16-centroid column block (each 2 * 16 * ceil(n/16) * 4 MFMAs of 2048 flop) */
    uint64_t cost_passes;      /* extra K.*C contractions for the cost of an iterate inside the stopping window */
    uint64_t mfma_instructions;/* v_mfma_f32_16x16x4_f32 issued per wavefront, summed (2048 flop each) */
    uint64_t audited_points;   /* RP_LLOYD_AUDIT: points compared with the unpruned pass */
    uint64_t audit_mismatches; /* ... and how many differed in bucket or distance bits */
    uint64_t sampled_points;   /* the production self-check: every 521st point is searched again WITHOUT the prune after every */
    uint64_t sample_mismatches;/* pruned pass; a mismatch fails the next call that hands results out (RP_ERR_INTERNAL) */
    /* the second k-means++ filter (csrc/kpp_bound.hpp; layer.rs:170-178 needs d(c_k, x) only where d^2 < potential): */
    uint64_t kpp_bound_pairs;      /* (new centroid, point) pairs the column-marginal bound let through and the interval examined */
    uint64_t kpp_bound_kept;       /* ... of which the bit-faithful solve was still run */
    uint64_t kpp_bound_iterations; /* scaling-domain iterations over all examined pairs */
    uint64_t kpp_bound_cost_passes;/* cost evaluations inside the stopping windows */
    uint64_t column_iterations;    /* MFMA bound: iterations summed over single centroid columns (a block of 16 runs until its slowest) */
    /* the reference-seed k-means++ draw (csrc/kpp_refpick.hpp; WeightedIndex<f32>'s sequential running sums, layer.rs:160-166): */
    uint64_t ref_pick_chunks;      /* 256-term chunks over the layer's K draws */
    uint64_t ref_pick_walked;      /* ... of which were walked term by term (first chunk, binade crossings, ties); the others are one exact add */
} rp_prune_stats;
RP_API int rp_kmeans_prune_stats(rp_kmeans* h, rp_prune_stats* out);
/* the same with the size of the CALLER's struct: a host compiled against an older (shorter) rp_prune_stats passes its own sizeof
 * and gets the fields it knows; bytes beyond this library's struct are zeroed.  Prefer this one from plain-C hosts. */
RP_API int rp_kmeans_prune_stats_sized(rp_kmeans* h, void* out, size_t out_bytes);
RP_API int rp_kmeans_set_stream(rp_kmeans* h, void* hip_stream);

/* ---- multi-GPU: points sharded by rank, integer centroid sums all-reduced ----------
 * step_local(): pairwise + bound refresh on this rank's points, then partial centroid sums into
 * partial_dev (K*bins u32 counts, K u64 weights, K u64 sizes: partial_bytes()).  After an
 * all-reduce(sum) over ranks, step_finish() installs the centroids, computes drift and updates bounds. */
RP_API int rp_kmeans_partial_bytes(rp_kmeans* h, size_t* bytes);
/* Kmeans::next of a point-sharded job over an rp_comm: step_local, ncclAllReduce(sum) of the integer centroid sums
 * (u32 block and u64 block of the partial, in place, on the layer's stream), step_finish. */
RP_API int rp_kmeans_step_comm(rp_kmeans* h, rp_comm* c, float* drift, uint64_t* sizes, double* reassigned);
RP_API int rp_kmeans_step_local(rp_kmeans* h, void* partial_dev);
RP_API int rp_kmeans_step_finish(rp_kmeans* h, const void* reduced_dev, float* drift, uint64_t* sizes,
                                 double* reassigned);

/* Sinkhorn::divergence (sinkhorn.rs:166-171) / Metric::emd for P independent pairs:
 * mu[P*bins], nu[P*bins] u32 counts (host), out[P].  One wavefront per pair. */
RP_API int rp_sinkhorn_divergence(uint32_t bins, uint64_t pairs, const uint32_t* mu, const uint32_t* nu,
                                  const float* tri_metric, const rp_sinkhorn_hp* hp, int device, float* out);
/* Coupling::minimize().cost() (sinkhorn.rs:194-218): raw entropic OT cost, and iterations used */
RP_API int rp_sinkhorn_cost(uint32_t bins, uint64_t pairs, const uint32_t* mu, const uint32_t* nu,
                            const float* tri_metric, const rp_sinkhorn_hp* hp, int device, float* out,
                            uint32_t* iterations);
/* the same with mu, nu, out and iterations (may be NULL) in DEVICE memory, used in place: the same kernels, the same bits.
 * tri_metric and hp stay host arguments.  Returns after the device finished. */
RP_API int rp_sinkhorn_cost_device(uint32_t bins, uint64_t pairs, const uint32_t* mu_dev, const uint32_t* nu_dev,
                                   const float* tri_metric, const rp_sinkhorn_hp* hp, int device, float* out_dev,
                                   uint32_t* iterations_dev);
/* impl Coupling for Sinkhorn (monge/src/coupling.rs:23-51; lloyd/src/sinkhorn.rs:194-218): minimize() one pair, then
 * flow(x, y) = coupling(x, y) * raw_distance(x, y) with coupling = exp(lhs(x) + rhs(y) - C/T) (sinkhorn.rs:114-116).
 * flow[bins*bins] row-major over (x, y), 0 outside supp(mu) x supp(nu); coupling (same shape) may be NULL.  The x-major
 * left fold of `flow` is cost() (sinkhorn.rs:206-217) bit for bit. */
RP_API int rp_sinkhorn_flow(uint32_t bins, const uint32_t* mu, const uint32_t* nu, const float* tri_metric,
                            const rp_sinkhorn_hp* hp, int device, float* flow, float* coupling);
/* Equity::variation (equity.rs:41-53) for P pairs of `bins`-bin histograms (bins = 101 on the turn layer) */
RP_API int rp_equity_variation(uint32_t bins, uint64_t pairs, const uint32_t* x, const uint32_t* y, int device,
                               float* out);

/* =================================================================================================
 * Abstraction inputs: what feeds the k-means layers above.
 *   crates/deuce/src — cards, hand strength, river equity, suit isomorphism and its iterator;
 *   crates/lloyd/src/lookup.rs — the (isomorphism -> abstraction) table and its projection onto the
 *   previous street's histograms (the k-means points).
 * Encodings are the reference's: card = rank * 4 + suit (card.rs:16-20; rank 0 = Two .. 12 = Ace, suit
 * c, d, h, s = 0..3); Hand = u64 bit set of cards (hand.rs:7); Observation as i64 = one byte
 * (card + 1) per card, public cards then pocket cards, each ascending, first card most significant
 * (observation.rs:132-165) — the `obs BIGINT` column of the reference's tables.
 * `*_dev` arguments are DEVICE pointers the caller has finished writing; calls return after the
 * device finished.  Bulk work shards across GPUs by pocket range / observation slice, no exchange.
 * ================================================================================================= */
typedef enum rp_street { RP_STREET_PREF = 0, RP_STREET_FLOP = 1, RP_STREET_TURN = 2, RP_STREET_RIVE = 3 } rp_street;

/* Strength::from(Hand) (strength.rs:18-32 = Evaluator::find_ranking + find_kickers, evaluator.rs:38-72) for n
 * hands of 5..7 cards (host arrays).  key = variant << 21 | rank1 << 17 | rank2 << 13 | kickers, variant in the
 * default build's Ranking order (ranking.rs:17-29: HighCard 0 .. StraightFlush 8; Flush above FullHouse as
 * declared there): integer order of keys == the reference's derived Ord on Strength. */
RP_API int rp_hand_strength(int device, uint64_t n, const uint64_t* hands, uint32_t* keys);
/* i64::from(Isomorphism::from(Observation::from(obs))) (isomorphism.rs:8-14, permutation.rs:9-71), host arrays */
RP_API int rp_obs_canonical(int device, uint64_t n, const int64_t* obs, int64_t* canon);
/* IsomorphismIterator::from(street) (isomorphism_iter.rs:7-26 over observation_iter.rs:13-104), restricted to the
 * pockets numbered [pocket_lo, pocket_hi) of the 1326 two-card hands in ascending bit-set order (the iterator's outer
 * loop).  Writes the canonical observations, in the iterator's order, to obs_dev[0..min(*n, cap)) and the number
 * there are to *n; obs_dev may be NULL to count.  All pockets: 169 / 1 286 792 / 13 960 050 / 123 156 254
 * (street.rs:120-127). */
RP_API int rp_isomorphisms(int device, int street, uint32_t pocket_lo, uint32_t pocket_hi, int64_t* obs_dev,
                           uint64_t cap, uint64_t* n);
/* Observation::equity (observation.rs:45-63) of n river observations: wins / (wins + losses) over the 990 opposing
 * holes, 0.5 when every showdown ties; bucket = Abstraction::from(Probability)'s index (kicker/src/abstraction.rs:
 * 61-63,93-99: round(p * 100)) = Lookup::grow(Street::Rive) (lookup.rs:172-178).  Either output may be NULL. */
RP_API int rp_river_equity(int device, uint64_t n, const int64_t* obs_dev, float* equity_dev, uint8_t* bucket_dev);

/* Lookup (lookup.rs:9-25): `n` isomorphisms of one street with their abstraction indices, in
 * IsomorphismIterator order (checked).  The table is copied. */
typedef struct rp_lookup rp_lookup;
RP_API int rp_lookup_create(int device, int street, uint64_t n, const int64_t* obs_dev, const uint8_t* abs_dev,
                            rp_lookup** out);
RP_API int rp_lookup_destroy(rp_lookup* h);
/* Lookup::lookup(&Isomorphism::from(obs)) for n observations of the table's street (any suit labelling).  A miss
 * is RP_ERR_INVALID (the reference panics, lookup.rs:24). */
RP_API int rp_lookup_get(rp_lookup* h, uint64_t n, const int64_t* obs_dev, uint8_t* abs_dev);
/* Lookup::projections / future (lookup.rs:27-45): for each of n observations of the PREVIOUS street, the histogram
 * of the table's abstractions over its children (Observation::children, observation.rs:35-40: 47 turns of a flop,
 * 46 rivers of a turn), Histogram::from(Vec<Abstraction>) (histogram.rs:207-212).  hist_dev[n][bins] u8 — the
 * `counts` layout of rp_kmeans_create_device. */
RP_API int rp_lookup_project(rp_lookup* h, uint64_t n, const int64_t* obs_dev, uint32_t bins, uint8_t* hist_dev);
/* device time of the calling thread's last call in this section, from HIP events around its launches */
RP_API int rp_deuce_kernel_ms(double* ms);

/* =================================================================================================
 * Abstraction atlas: the reference's derived tables over one street's Lookup, and the batched queries of its abstraction
 * explorer, answered from device memory.
 *   crates/daybook/src/schema.rs:78-173 — the `abstraction` table (population, equity via get_equity);
 *   crates/lloyd/src/lookup.rs:86-119   — isomorphism.position = ROW_NUMBER() OVER (PARTITION BY abs ORDER BY obs) - 1;
 *   crates/portal/src/topology/api.rs   — TopologyAPI (obs_to_abs, *_equity, *_population, abs_distance, *_histogram,
 *                                         exp_wrt_*, *_nearby, *_similar, nbr_*_wrt_abs, knn_ / kfn_ / kgn_wrt_abs).
 * One handle per street.  Derived once at create, on the device:
 *   population[k]  rows with abs == k
 *   position[i]    rows j with abs[j] == abs[i] and obs[j] < obs[i], compared as signed 64-bit (the BIGINT order; the table's
 *                  own IsomorphismIterator order is NOT that order)
 *   offset[K + 1], members[n]   members[offset[k] + p] = the row of bucket k at position p: the (abs, position) index
 *   equity[k]      river: (float)k / 100.0f.  Elsewhere get_equity (schema.rs:100-107) in f32, one rounding per operation:
 *                  over the bucket's transition rows (bins with a count, dx = (float)count / (float)weight), the left fold
 *                  from 0.0f of dx * next.equity[bin] divided by the left fold from 0.0f of dx; 0.0f for a bucket without
 *                  rows or with a zero divisor.
 * Three things SQL leaves open and this library fixes:
 *   fold order   PostgreSQL's SUM(REAL) folds in REAL in an unspecified row order; here the order is the one
 *                rp_artifact_write_transitions writes: dx descending, stable over the ascending bin.
 *   ties         neighbours at equal distance go to the smaller bucket index, nearest and farthest alike.
 *   draws        a RANDOM() is a caller-supplied uint64 `draw`: u = (double)(draw >> 11) * 2^-53,
 *                i = (uint32)floor(u * (double)population).  The library draws nothing itself.
 * The reference's *_similar predicate (position < LEAST(6, population) AND position >= FLOOR(RANDOM() *
 * GREATEST(population - 6, 1))) is a caller's choice of `start` for rp_atlas_members; it is not built in.
 * Every query is batched and fills a per-answer status; the plain forms take host arrays, the _device forms device arrays
 * the caller has finished writing, and return after the device finished.
 * ================================================================================================= */
typedef struct rp_atlas rp_atlas;
typedef struct rp_atlas_sample {
    int64_t obs;         /* the table's (canonical) observation; 0 where there is none */
    float equity;        /* equity[k] of the record's bucket */
    float density;       /* (float)population / (float)n_observations(street) from describe (api.rs:266), / n_isomorphisms(street)
                            from pick and neighbours (api.rs:299) */
    float distance;      /* tri[Pair::merge(abs, wrt)], 0 without a wrt */
    uint32_t position;
    uint32_t population;
    int16_t abs;         /* street << 8 | k */
    uint8_t reserved[2];
} rp_atlas_sample; /* 32 bytes */
#if defined(__cplusplus)
static_assert(sizeof(rp_atlas_sample) == 32, "rp_atlas_sample is 32 bytes");
#else
_Static_assert(sizeof(rp_atlas_sample) == 32, "rp_atlas_sample is 32 bytes");
#endif
typedef enum rp_atlas_status {
    RP_ATLAS_OK = 0,
    RP_ATLAS_MISS = 1,  /* the observation is not one of the street, or not in the table: a zero record */
    RP_ATLAS_SAME = 2,  /* describe: wrt is the observation's own bucket, distance 0 */
    RP_ATLAS_EMPTY = 3, /* the bucket has no member (pick, neighbours with draws) or no transition row (obs_equity, histograms) */
    RP_ATLAS_RANGE = 4  /* a bucket index >= K: a zero record */
} rp_atlas_status;
typedef enum rp_atlas_hist_kind { RP_ATLAS_HIST_ABS = 0, RP_ATLAS_HIST_OBS = 1 } rp_atlas_hist_kind;
#define RP_ATLAS_MAX_K 256u
#define RP_ATLAS_MAX_ROWS (1ull << 27) /* sortscan's row indices are 27 bits; the river's 123 156 254 fit */
#define RP_ATLAS_MAX_NEIGHBORS 16u
#define RP_ATLAS_MAX_WINDOW 16u
/* (obs_dev, abs_dev): what rp_lookup_create takes, under the same check (a prefix of a street's list is a valid table); K <= 256 and
 * every abs < K, else RP_ERR_INVALID; n > 2^27: RP_ERR_UNSUPPORTED.  future_counts [K][bins] / future_weight [K] (host) are what
 * rp_kmeans_centroids returns, tri [K (K - 1) / 2] (host) what rp_kmeans_metric returns; bins must equal next's K, next must be the
 * atlas of street + 1 on the same device (it is read at create only).  River: future_*, tri and next are NULL, bins 0; row_equity_dev
 * [n] may be rp_river_equity's equities (the isomorphism.equity column), it is copied.  Elsewhere future_* and next are required;
 * tri may be NULL (neighbours, distance and describe-with-wrt then answer RP_ERR_UNSUPPORTED). */
RP_API int rp_atlas_create(int device, int street, uint64_t n, const int64_t* obs_dev, const uint8_t* abs_dev, uint32_t K,
                           const uint32_t* future_counts, const uint64_t* future_weight, uint32_t bins, const float* tri,
                           const float* row_equity_dev, const rp_atlas* next, rp_atlas** out);
RP_API int rp_atlas_destroy(rp_atlas* h);
/* n, K, bins, street of the handle; any output may be NULL */
RP_API int rp_atlas_shape(const rp_atlas* h, uint64_t* n, uint32_t* K, uint32_t* bins, int* street);
/* the derived tables, copied to host OR device memory (any may be NULL): population[K], offset[K + 1], equity[K],
 * position[n], members[n] */
RP_API int rp_atlas_tables(rp_atlas* h, uint32_t* population, uint32_t* offset, float* equity, uint32_t* position, uint32_t* members);
/* device time of this handle's create: the (abs, obs) sort, and everything else (histogram, scan, positions, equity) */
RP_API int rp_atlas_create_ms(const rp_atlas* h, double* sort_ms, double* rest_ms);
/* obs_to_abs, obs_population, exp_wrt_obs, nbr_obs_wrt_abs, kgn_wrt_abs: the record of each observation (any suit labelling);
 * wrt u8[n] or NULL: distance = tri[Pair(abs, wrt)], status SAME and distance 0 when wrt is the observation's own bucket */
RP_API int rp_atlas_describe(rp_atlas* h, uint64_t n, const int64_t* obs, const uint8_t* wrt, rp_atlas_sample* out, uint8_t* status);
RP_API int rp_atlas_describe_device(rp_atlas* h, uint64_t n, const int64_t* obs, const uint8_t* wrt, rp_atlas_sample* out, uint8_t* status);
/* obs_equity (api.rs:91-115).  River: the row's row_equity (RP_ERR_UNSUPPORTED if none was given).  Elsewhere the un-normalised
 * left fold of dx * next.equity over the rows of the observation's bucket (no division), 0 with status EMPTY if it has none */
RP_API int rp_atlas_obs_equity(rp_atlas* h, uint64_t n, const int64_t* obs, float* out, uint8_t* status);
RP_API int rp_atlas_obs_equity_device(rp_atlas* h, uint64_t n, const int64_t* obs, float* out, uint8_t* status);
/* exp_wrt_abs, replace_obs, nbr_abs_wrt_abs, hst_wrt_abs_on_river: the member of bucket abs[q] at the position draw[q] selects;
 * population 0: status EMPTY (abs, equity and zeros) */
RP_API int rp_atlas_pick(rp_atlas* h, uint64_t n, const uint8_t* abs, const uint64_t* draw, rp_atlas_sample* out, uint8_t* status);
RP_API int rp_atlas_pick_device(rp_atlas* h, uint64_t n, const uint8_t* abs, const uint64_t* draw, rp_atlas_sample* out, uint8_t* status);
/* abs_nearby, knn_wrt_abs, kfn_wrt_abs: the k <= min(K - 1, 16) other buckets of the street by tri ascending (farthest != 0:
 * descending), ties to the smaller index; out / status [n][k].  draws [n][k] or NULL: slot j comes with the member draws[q][j]
 * selects; an empty neighbour keeps its slot with status EMPTY (the reference drops it after the LIMIT).  Without draws obs and
 * position are 0. */
RP_API int rp_atlas_neighbors(rp_atlas* h, uint64_t n, const uint8_t* wrt, uint32_t k, int farthest, const uint64_t* draws,
                              rp_atlas_sample* out, uint8_t* status);
RP_API int rp_atlas_neighbors_device(rp_atlas* h, uint64_t n, const uint8_t* wrt, uint32_t k, int farthest, const uint64_t* draws,
                                     rp_atlas_sample* out, uint8_t* status);
/* abs_distance: 0 for a == b, else tri[Pair::merge(a, b)]; NaN where an index is >= K */
RP_API int rp_atlas_distance(rp_atlas* h, uint64_t n, const uint8_t* a, const uint8_t* b, float* out);
RP_API int rp_atlas_distance_device(rp_atlas* h, uint64_t n, const uint8_t* a, const uint8_t* b, float* out);
/* abs_histogram (kind ABS, ids u8[n]): count = (uint32)(dx * 1000.0f), truncated (api.rs:207); obs_histogram (kind OBS, ids i64[n]):
 * count = roundf(dx * (float)n_children(street)) of the observation's bucket (api.rs:227-237; 19 600 / 47 / 46).  counts [n][bins];
 * a bucket without transition rows: zeros with status EMPTY.  River atlases: RP_ERR_UNSUPPORTED */
RP_API int rp_atlas_histograms(rp_atlas* h, uint64_t n, int kind, const void* ids, uint32_t* counts, uint8_t* status);
RP_API int rp_atlas_histograms_device(rp_atlas* h, uint64_t n, int kind, const void* ids, uint32_t* counts, uint8_t* status);
/* the window [start, start + count) ∩ [0, population) of bucket abs[q] in position order: out i64 [n][count] (0 beyond the window),
 * got[q] = observations written; count <= 16 */
RP_API int rp_atlas_members(rp_atlas* h, uint64_t n, const uint8_t* abs, const uint32_t* start, uint32_t count, int64_t* out, uint8_t* got);
RP_API int rp_atlas_members_device(rp_atlas* h, uint64_t n, const uint8_t* abs, const uint32_t* start, uint32_t count, int64_t* out,
                                   uint8_t* got);

/* =================================================================================================
 * Artifact files: what the reference streams to PostgreSQL, written as files in the same
 * byte format — daybook::Streamable::stream (daybook/src/traits/streamable.rs:36-46) over
 * tokio_postgres::binary_copy::BinaryCopyInWriter, i.e. PostgreSQL's binary COPY format: load with
 *     COPY isomorphism (obs, abs) FROM '<file>' (FORMAT binary)       etc.
 * Host code, host arrays.
 * ================================================================================================= */
/* Generic writer / reader, struct-of-arrays.  `types`: one character per column — 'h' int2, 'i' int4, 'q' int8,
 * 'f' float4 (the shapes of daybook/src/traits/row.rs:21-57 are "qh", "if", "hhf", "qhqqfffi").  columns[c] points
 * at n_rows values of column c.  read(): fills up to `cap` rows (columns may be NULL to count) and reports *n_rows.
 * read() takes an SQL NULL (field length -1) in an 'f' column and stores the NaN with the bits RP_PGCOPY_NULL_F32; a NULL in any
 * other column is RP_ERR_INVALID as before.  write() writes no NULLs. */
#define RP_PGCOPY_NULL_F32 0xffffffffu
RP_API int rp_pgcopy_write(const char* path, const char* types, uint64_t n_rows, const void* const* columns);
RP_API int rp_pgcopy_read(const char* path, const char* types, uint64_t cap, void* const* columns, uint64_t* n_rows);
/* Lookup rows (lloyd/src/lookup.rs:141-147): (obs i64, abs i16 = street << 8 | index) in table order */
RP_API int rp_artifact_write_lookup(const char* path, int street, uint64_t n, const int64_t* obs,
                                    const uint8_t* abs_index);
/* Metric rows (lloyd/src/metric.rs:219-226, distances.rs:69-84): (tri i32 = street << 30 | t, dx f32), t ascending;
 * tri[] as rp_kmeans_metric returns it */
RP_API int rp_artifact_write_metric(const char* path, int street, uint32_t K, const float* tri);
/* Future rows (lloyd/src/future.rs:99-111): per abstraction, its centroid's distribution() (bins.rs:113-117: density
 * descending, stable) as (prev i16, next i16, dx f32); counts/weight as rp_kmeans_centroids returns them */
RP_API int rp_artifact_write_transitions(const char* path, int street, uint32_t K, uint32_t bins,
                                         const uint32_t* counts, const uint64_t* weight);
/* The derived `abstraction` table (daybook/src/schema.rs:87-92): rows (abs i16 = street << 8 | k, street i16, population i32,
 * equity f32), k ascending; population / equity as rp_atlas_tables returns them.  Read back with rp_pgcopy_read(path, "hhif", ...). */
RP_API int rp_artifact_write_abstraction(const char* path, int street, uint32_t K, const uint32_t* population, const float* equity);
/* The `isomorphism` table with its derived columns (lloyd/src/lookup.rs:91-96): rows (obs i64, abs i16, equity f32, position i32) in
 * table order; equity NULL writes SQL NULL in every row (the column is the river's).  Read back with rp_pgcopy_read(path, "qhfi", ...). */
RP_API int rp_artifact_write_isomorphism(const char* path, int street, uint64_t n, const int64_t* obs, const uint8_t* abs_index,
                                         const float* equity, const uint32_t* position);
/* NlheProfile::rows (nlhe/src/profile.rs:144-163) as the blueprint table's COPY file: columns (past BIGINT, present SMALLINT,
 * choices BIGINT, edge BIGINT, weight REAL, regret REAL, payoff REAL, visits INTEGER) (profile.rs:20-31), one row per
 * (infoset, edge of its choices); edge = From<Edge> for u64 (kicker/src/edge.rs:122-160).  Input: rp_nlhe_export's arrays.
 * Read back with rp_pgcopy_read(path, "qhqqfffi", ...) and rp_nlhe_import (Hydrate, profile.rs:90-141). */
RP_API int rp_artifact_write_blueprint(const char* path, uint64_t n_infosets, const uint64_t* past, const uint32_t* present,
                                       const uint64_t* choices, const rp_encounter* enc, int only_visited, uint64_t* rows_written);

/* =================================================================================================
 * The NLHE rules engine on the device (first device step).  The betting state machine of
 * kicker::GameN<P> (crates/kicker/src/game.rs), the action abstraction (edge.rs, size.rs: Pluribus grids) with
 * NlheGame::apply's actionize + snap (crates/nlhe/src/game.rs:33-53) and Showdown::settle (showdown.rs) run as
 * device functions; this entry point plays `n_games` random abstract hands of `n_players` (2..10, 200-chip stacks,
 * blinds 1 / 2, dealer = game % n_players), one lane per game: deals and choices from rp_node_hash(seed, 0, game,
 * counter) (rp_math.h).  payoffs_dev[game][seat] = NlheGame::payoff (settlement.won()), digests_dev[game] folds every
 * intermediate state, steps_dev[game] = actions taken (0xffffffff if the hand did not finish in max_steps).  The
 * MCCFR traversal over this engine is not built yet.
 * ================================================================================================= */
RP_API int rp_nlhe_playouts(int device, uint32_t n_players, uint64_t n_games, uint64_t seed, uint32_t max_steps,
                            float* payoffs_dev, uint64_t* digests_dev, uint32_t* steps_dev);

#ifdef __cplusplus
}
#endif
#endif /* RP_MI355X_H */
