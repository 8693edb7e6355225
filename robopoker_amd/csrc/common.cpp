// common.cpp — error reporting, the training loop, version and device probing for librp_mi355x.so
#include "rp_internal.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <hip/hip_runtime_api.h>

namespace rp {

static thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// Checkpoint's Display / Progress::format (metrics/checkpoint.rs:39-50, progress.rs:8-18): four 20-column fields
void format_progress(char* buf, size_t cap, uint64_t epoch, uint64_t nodes, uint64_t infos, double rate) {
    char f[4][48];
    snprintf(f[0], sizeof f[0], "batch %llu", (unsigned long long)epoch);
    snprintf(f[1], sizeof f[1], "nodes %llu", (unsigned long long)nodes);
    snprintf(f[2], sizeof f[2], "infos %llu", (unsigned long long)infos);
    snprintf(f[3], sizeof f[3], "I/sec %.1f", rate);
    snprintf(buf, cap, "%-20s%-20s%-20s%-20s", f[0], f[1], f[2], f[3]);
}

int train_loop(const std::function<int(TrainCounts&)>& step, const std::function<int(TrainCounts&)>& refresh, uint64_t max_steps,
               double max_seconds, double log_interval, double flush_interval, rp_train_event_fn on_event, void* user,
               const volatile int* interrupt, char* summary, size_t summary_cap) {
    using clock = std::chrono::steady_clock;
    const auto start = clock::now();
    auto prior = start, flushed = start;
    uint64_t prior_infos = 0, steps = 0;
    TrainCounts c{0, 0, 0};
    auto secs_since = [](clock::time_point t) { return std::chrono::duration<double>(clock::now() - t).count(); };
    int rc;
    for (;;) {
        if ((rc = step(c))) return rc;  // Trainer::train: step, then checkpoint, then flush, then the interrupt test
        steps += 1;
        if (secs_since(prior) >= log_interval) {  // Metrics::checkpoint (metrics/mod.rs:67-80)
            if ((rc = refresh(c))) return rc;
            const double secs = std::max(1.0, std::floor(secs_since(prior)));  // elapsed().as_secs().max(1)
            rp_checkpoint cp{c.epoch, c.nodes, c.infos, (double)(c.infos - prior_infos) / secs};
            prior = clock::now();
            prior_infos = c.infos;
            if (on_event) {
                char line[96];
                format_progress(line, sizeof line, cp.epoch, cp.nodes, cp.infos, cp.rate);
                on_event(RP_TRAIN_CHECKPOINT, &cp, line, user);
            }
        }
        if (secs_since(flushed) >= flush_interval) {  // FastSession::flush cadence (forge/src/fast.rs:97-125)
            flushed = clock::now();
            if (on_event) {
                rp_checkpoint cp{c.epoch, c.nodes, c.infos, 0.0};
                on_event(RP_TRAIN_FLUSH, &cp, "", user);
            }
        }
        const bool stop = (interrupt && *interrupt) || (max_steps && steps >= max_steps) ||
                          (max_seconds > 0.0 && secs_since(start) >= max_seconds);
        if (stop) break;
    }
    if ((rc = refresh(c))) return rc;
    if (summary && summary_cap) {  // Progress::summary (progress.rs:24-26): rate over the whole run
        char line[96];
        const double secs = std::max(1.0, std::floor(secs_since(start)));
        format_progress(line, sizeof line, c.epoch, c.nodes, c.infos, (double)c.infos / secs);
        snprintf(summary, summary_cap, "training stopped\n%s", line);
    }
    return RP_OK;
}

}  // namespace rp

extern "C" {

const char* rp_last_error(void) { return rp::g_err; }

int rp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

const char* rp_version(void) { return "rp_mi355x 0.3.0 gfx950 hip " RP_STR(HIP_VERSION_MAJOR) "." RP_STR(HIP_VERSION_MINOR); }

void rp_hyper_default(rp_hyper* out) {
    if (!out) return;
    memset(out, 0, sizeof(*out));
    out->temperature = 1.0f;
    out->smoothing = 2.0f;
    out->curiosity = 0.05f;
    out->prune_threshold = -3e5f;
    out->prune_explore = 0.05f;
    out->prune_warmup = 16384;
    out->regret_min = -4e6f;
}

void rp_sinkhorn_hp_default(rp_sinkhorn_hp* out) {
    if (!out) return;
    out->temperature = 0.025f;
    out->iterations = 128;
    out->tolerance = 0.0005f;
}

}  // extern "C"
