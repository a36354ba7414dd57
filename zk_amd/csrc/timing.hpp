// timing.hpp -- how the zk_bench_* measurement hooks take their times: a span between the context's two events (timed_span), an owner
// of N events with per-phase sums (PhaseEvents) and a wall-clock-per-call loop (wall_clock_each).  Host-only, beside the owners of
// host_core.hpp; no kernel is defined here.
//
// The warm-up policy of every hook (the ALU-bound kernels follow the shader clock, which keeps climbing for ~20 ms after idle; the
// streaming ones only need their pool blocks and plans to exist):
//
//   hook                  | unit   | untimed calls                      | wait after | what is timed
//   ----------------------+--------+------------------------------------+------------+-----------------------------------------------
//   fold                  | capi   | 0                                  | no         | reps launches, ev0..ev1, average
//   fold_samples          | capi   | 0                                  | no         | reps launches, one event per `group` of them
//   prove_partial         | capi   | 0                                  | (each rep) | wall clock around each zk_sumcheck_prove
//   evaluate              | capi   | 0                                  | (each rep) | wall clock around each zk_mle_evaluate
//   evaluate_device       | capi   | 1                                  | yes        | reps enqueues, ev0..ev1, average
//   modmul                | capi   | 1 launch of 8 iterations (its own) | no         | one launch of `iters` iterations, ev0..ev1
//   copy                  | capi   | 1 launch (its own)                 | no         | reps launches, ev0..ev1, GB/s
//   ntt                   | ntt    | reps + 1                           | no         | reps transforms, ev0..ev1, average
//   upoly_interp          | ntt    | 0                                  | (each rep) | each rep and its 4 phases, events of its own
//   upoly_evaluate_many   | ntt    | 1, marked like a timed one         | (each rep) | each rep and its 5 phases (tree path)
//   upoly_divrem          | ntt    | 1, marked like a timed one         | (each rep) | each rep and its 3 phases (Newton path)
//   cmle                  | cmle   | 1                                  | yes        | reps enqueues, ev0..ev1, average
//   cmle_algebra          | cmle   | 1                                  | yes        | reps calls, ev0..ev1, average
//   batch_inverse         | inv    | reps                               | no         | reps calls, ev0..ev1, average
//   merkle                | merkle | reps                               | no         | reps builds, ev0..ev1, average
//   fri_fold              | fri    | reps                               | no         | reps folds, ev0..ev1, average
//   deep_quotient         | pcs    | reps                               | no         | reps quotients, ev0..ev1, average
//   gprod                 | gprod  | reps                               | no         | reps trees / whole proofs, ev0..ev1, average
//   fsum                  | fsum   | reps                               | no         | reps trees / proofs / multiplicity counts, ev0..ev1, average
//   mlbatch               | mlbatch| reps                               | no         | reps openings' device work / first folds / rounds, ev0..ev1, average
//
// "(each rep)": the host waits for every rep before the next starts (the last event of a phase-timed rep, the stream before a
// wall-clock one).  Every helper leaves by the same rule on a failure: the stream is drained before the caller's blocks go back, what
// was created is destroyed, and the first failing status is returned (nothing is written to the output then).
#pragma once
#include <chrono>

#include "host_core.hpp"

enum class AfterWarm { kNoWait, kWait };

// `warm` untimed calls of once(), a stream wait if asked for, then `reps` calls between the context's ev0 and ev1: *out_ms = average
// ms per call.  once() enqueues on c->stream and returns a status.
template <class Once>
inline int32_t timed_span(zk_ctx *c, int32_t warm, AfterWarm after, int32_t reps, Once &&once, double *out_ms) {
    DrainOnExit drain(c);   // a failed call waits for what it enqueued before the caller's blocks go back
    for (int32_t i = 0; i < warm; ++i) ZKCHK(once());
    if (after == AfterWarm::kWait) HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    for (int32_t i = 0; i < reps; ++i) ZKCHK(once());
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    HIPCHK(hipEventSynchronize(c->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    drain.armed = false;   // ev1 has been waited for
    *out_ms = (double)ms / reps;
    return ZK_OK;
}

// Move-only owner of a sequence of events on the context's stream: begin() records the first, mark(i) the i-th of the inner ones (what
// the product code calls through its optional pointer), end() records the last and waits for it.  run() times whole calls with it:
// per rep the span first..last and, where asked for, the span between every two consecutive events, summed and averaged.
// (comm.hip's shard_run uses the owner alone, for the phases of the sharded prover: push() and record() as its loop goes.)
struct PhaseEvents {
    hipStream_t stream;
    std::vector<hipEvent_t> ev;
    explicit PhaseEvents(const zk_ctx *c) : stream(c->stream) {}
    PhaseEvents(PhaseEvents &&o) noexcept : stream(o.stream), ev(std::move(o.ev)) { o.ev.clear(); }
    PhaseEvents &operator=(PhaseEvents &&) = delete;
    PhaseEvents(const PhaseEvents &) = delete;
    PhaseEvents &operator=(const PhaseEvents &) = delete;
    ~PhaseEvents() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    // first and last event plus n_marks inner ones
    int32_t create(size_t n_marks) {
        ev.reserve(n_marks + 2);
        while (ev.size() < n_marks + 2) ZKCHK(push());
        return ZK_OK;
    }
    // one more event at the end of the sequence (for a caller that learns the number of its marks as it goes)
    int32_t push() {
        hipEvent_t e = nullptr;
        HIPCHK(hipEventCreate(&e));
        ev.push_back(e);
        return ZK_OK;
    }
    size_t count() const { return ev.size(); }
    int32_t record(size_t i) const {
        HIPCHK(hipEventRecord(ev[i], stream));
        return ZK_OK;
    }
    int32_t begin() const { return record(0); }
    int32_t mark(size_t i) const { return record(i + 1); }
    int32_t end() const {
        ZKCHK(record(ev.size() - 1));
        HIPCHK(hipEventSynchronize(ev.back()));
        return ZK_OK;
    }
    // ms between event i and event j, both recorded and complete
    int32_t span_ms(size_t i, size_t j, double *out) const {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ev[i], ev[j]));
        *out = ms;
        return ZK_OK;
    }
    // `warm` untimed and `reps` timed calls of once(), each between begin() and end(): out_ms[0] = average ms of the call,
    // out_ms[1 .. count()) = of its phases, or zeros when `phases` is false (a path that records no inner mark)
    template <class Once>
    int32_t run(zk_ctx *c, int32_t warm, int32_t reps, bool phases, Once &&once, double *out_ms) const {
        DrainOnExit drain(c);   // a failed call waits for what it enqueued before the caller's blocks go back
        std::vector<double> acc(ev.size(), 0.0);
        for (int32_t r = -warm; r < reps; ++r) {
            ZKCHK(begin());
            ZKCHK(once());
            ZKCHK(end());
            if (r < 0) continue;
            double ms = 0.0;
            ZKCHK(span_ms(0, ev.size() - 1, &ms));
            acc[0] += ms;
            for (size_t q = 0; phases && q + 1 < ev.size(); ++q) {
                ZKCHK(span_ms(q, q + 1, &ms));
                acc[q + 1] += ms;
            }
        }
        drain.armed = false;   // the last event of the last rep has been waited for
        for (size_t q = 0; q < ev.size(); ++q) out_ms[q] = acc[q] / reps;
        return ZK_OK;
    }
};

// Wall clock of each of `reps` calls of once(), which waits for its own results: the stream is waited for before every stamp, so a
// call never pays for its predecessor's tail.  out_ms_each[reps].
template <class Once>
inline int32_t wall_clock_each(zk_ctx *c, int32_t reps, Once &&once, double *out_ms_each) {
    DrainOnExit drain(c);
    for (int32_t i = 0; i < reps; ++i) {
        HIPCHK(hipStreamSynchronize(c->stream));
        const auto t0 = std::chrono::steady_clock::now();
        ZKCHK(once());
        out_ms_each[i] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    drain.armed = false;   // every call has waited for its own results
    return ZK_OK;
}
