// rp_internal.h — shared host-side helpers of librp_mi355x.so (not part of the ABI).
#ifndef RP_INTERNAL_H
#define RP_INTERNAL_H

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>

#include "../../include/rp_mi355x.h"
#include "../../include/rp_mi355x_diag.h"

#define RP_MAX_ACTIONS 16u   // widest infoset row the device kernels are compiled for (NLHE needs 9..14)
#define RP_MAX_PLAYERS 8u
#define RP_STR2(x) #x
#define RP_STR(x) RP_STR2(x)

struct ihipStream_t;

namespace rp {

// records the message for rp_last_error() and returns the code
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
// Checkpoint's display line / Progress::format (metrics/checkpoint.rs:39-50, progress.rs:8-18)
void format_progress(char* buf, size_t cap, uint64_t epoch, uint64_t nodes, uint64_t infos, double rate);

// Trainer::train (crates/forge/src/trainer.rs:18-66), the loop behind rp_mccfr_train and rp_nlhe_train: loop { step; checkpoint;
// flush; interrupt? }, then Progress::summary.  step runs one step and may update the counts; refresh brings nodes and infos up
// to date and is called at each checkpoint and once before the summary.  A flush reports the counts as last known.
struct TrainCounts {
    uint64_t epoch, nodes, infos;
};
int train_loop(const std::function<int(TrainCounts&)>& step, const std::function<int(TrainCounts&)>& refresh, uint64_t max_steps,
               double max_seconds, double log_interval, double flush_interval, rp_train_event_fn on_event, void* user,
               const volatile int* interrupt, char* summary, size_t summary_cap);

// What one table says about the trees below `root` (games.cpp).  Walker states keep every child, all other states one
// (external sampling); each sampled-tree figure is the maximum over the walkers 0..n_players-1, saturating at UINT32_MAX.
// Needs children[] entries in range and behind their parents (rp_game_table_check verifies that first).
struct TableBounds {
    uint32_t depth;      // states on the longest root-to-leaf path
    uint32_t nodes;      // nodes of the largest sampled tree
    uint32_t decisions;  // walker nodes of a sampled tree
    uint32_t stack;      // pending leaves of the traversal: a walker node pushes all children, one is popped and explored first
    uint32_t internal;   // expanded (non-terminal) nodes of a sampled tree
};
TableBounds table_bounds(const rp_game_table& t, uint32_t root);

}  // namespace rp

// sparse.hip / deuce.hip: what nlmc.hip needs of the profile and of the encoder tables
struct rp_profile;
struct rp_lookup;
namespace rp {
float* profile_table(rp_profile* h);
float* profile_swap_table(rp_profile* h, float* tab, uint64_t n_rows);
ihipStream_t* profile_stream(rp_profile* h);
uint64_t profile_epoch(const rp_profile* h);
unsigned char* profile_entries(rp_profile* h);
int lookup_view(const rp_lookup* t, const uint64_t** keys, const uint8_t** abs_, uint64_t* n, int* street);
}  // namespace rp

// comm.cpp: the collectives behind rp_comm, enqueued on the caller's HIP stream
struct rp_comm;
namespace rp {
int comm_world(const rp_comm* c);
int comm_rank(const rp_comm* c);
int comm_all_gather(rp_comm* c, const void* send, void* recv, size_t bytes, ihipStream_t* stream);
int comm_all_reduce_sum(rp_comm* c, void* buf, size_t count, int kind /* 0 = i32, 1 = i64 */, ihipStream_t* stream);
}  // namespace rp

#endif
