// comm.hip -- the exchange steps of the sharded paths.
//
// The reference (sumcheck/src/prover.rs:44-68, fft/src/lib.rs:4-19) is single-process; this is the multi-GPU form's
// communication: ONE all-reduce of (D+1)*8 uint64 lanes per sumcheck round, one all-gather for the prover's tail, one
// all-to-all per sharded NTT.  Transport is RCCL over xGMI (one process per GPU), enqueued on the context's stream so the
// whole round loop runs without a host synchronisation; a host-callback transport with the same control flow exists for
// tests and for hosts that bring their own channel.  librccl.so.1 is loaded on first use (dlopen): a process that already
// maps a copy (PyTorch-ROCm bundles one under the same SONAME) gets that copy -- one RCCL, one HIP runtime per process.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "../../include/zk_amd.h"
#include "host_core.hpp"
#include "timing.hpp"
#include "env.hpp"
#include "prover_state.hpp"

#include <dlfcn.h>
#include <rccl/rccl.h>

namespace {
struct RcclApi {
    bool ok = false;
    std::string err;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclAllToAll) AllToAll = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;   // optional: absent -> a failed rank cannot release its peers
    decltype(&ncclGetVersion) GetVersion = nullptr;        // optional (zk_comm_info)
    decltype(&ncclCommCount) CommCount = nullptr;          // optional
    decltype(&ncclCommUserRank) CommUserRank = nullptr;    // optional
};
RcclApi load_rccl() {
    RcclApi a;
    void *h = nullptr;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (h) break;
    }
    if (!h) {
        const char *e = dlerror();
        a.err = std::string("dlopen librccl.so.1: ") + (e ? e : "not found");
        return a;
    }
#define ZK_RCCL_SYM(field, sym)                                   \
    a.field = reinterpret_cast<decltype(a.field)>(dlsym(h, sym)); \
    if (!a.field) {                                               \
        a.err = std::string("librccl lacks ") + sym;              \
        return a;                                                 \
    }
    ZK_RCCL_SYM(GetUniqueId, "ncclGetUniqueId")
    ZK_RCCL_SYM(CommInitRank, "ncclCommInitRank")
    ZK_RCCL_SYM(CommDestroy, "ncclCommDestroy")
    ZK_RCCL_SYM(AllReduce, "ncclAllReduce")
    ZK_RCCL_SYM(AllGather, "ncclAllGather")
    ZK_RCCL_SYM(AllToAll, "ncclAllToAll")
    ZK_RCCL_SYM(GetErrorString, "ncclGetErrorString")
#undef ZK_RCCL_SYM
    a.CommAbort = reinterpret_cast<decltype(a.CommAbort)>(dlsym(h, "ncclCommAbort"));
    a.GetVersion = reinterpret_cast<decltype(a.GetVersion)>(dlsym(h, "ncclGetVersion"));
    a.CommCount = reinterpret_cast<decltype(a.CommCount)>(dlsym(h, "ncclCommCount"));
    a.CommUserRank = reinterpret_cast<decltype(a.CommUserRank)>(dlsym(h, "ncclCommUserRank"));
    a.ok = true;
    return a;
}
RcclApi &rccl() {
    static RcclApi a = load_rccl();
    return a;
}
}  // namespace

struct zk_comm {
    zk_ctx *ctx;
    uint32_t world, rank;
    ncclComm_t nccl;      // RCCL transport (null: host callbacks)
    bool own_nccl;
    zk_host_allreduce_fn h_allreduce;
    zk_host_allgather_fn h_allgather;
    zk_host_alltoall_fn h_alltoall;
    void *user;
    uint64_t *h_send, *h_recv;   // pinned staging of the host transport, grown on demand
    size_t h_send_bytes, h_recv_bytes;
    bool dead;                   // a collective or a step between two collectives failed: every later call returns ZK_ERR_COMM
};
// A rank that fails BETWEEN two collectives (an allocation, a launch) would leave its peers blocked inside the next collective
// for ever.  The failing rank therefore aborts a communicator it owns (ncclCommAbort: the peers' pending collectives return
// with an error instead of hanging) and the zk_comm is dead from then on.  A wrapped communicator belongs to the host: it is
// only marked dead here, aborting it is the host's call.
static int32_t comm_fail(zk_comm *cm, int32_t rc) {
    if (rc == ZK_OK || cm->dead) return rc;
    cm->dead = true;
    if (cm->nccl && cm->own_nccl && rccl().CommAbort) {
        (void)rccl().CommAbort(cm->nccl);
        cm->nccl = nullptr;
        cm->own_nccl = false;
    }
    return rc;
}
static int32_t comm_alive(zk_comm *cm) {
    if (!cm->dead) return ZK_OK;
    g_hip_err = "communicator is dead after an earlier failure (zk_comm_destroy it and create a new one)";
    return ZK_ERR_COMM;
}

static int32_t rccl_check(ncclResult_t r, const char *what) {
    if (r == ncclSuccess) return ZK_OK;
    g_hip_err = std::string(what) + ": " + rccl().GetErrorString(r);
    return ZK_ERR_COMM;
}
static void comm_delete(zk_comm *cm) { delete cm; }
static int32_t comm_new(zk_ctx *c, uint32_t world, uint32_t rank, zk_comm **out) {
    if (!c || !out) return ZK_ERR_BAD_ARG;
    if (world == 0 || (world & (world - 1)) || world > 65536 || rank >= world) return ZK_ERR_BAD_ARG;
    zk_comm *cm = new (std::nothrow) zk_comm();
    if (!cm) return ZK_ERR_ALLOC;
    *cm = {};
    cm->ctx = c;
    cm->world = world;
    cm->rank = rank;
    *out = cm;
    return ZK_OK;
}
extern "C" int32_t zk_comm_unique_id(uint8_t out[128]) {
    if (!out) return ZK_ERR_BAD_ARG;
    static_assert(sizeof(ncclUniqueId) == 128, "include/zk_amd.h says 128 bytes");
    if (!rccl().ok) {
        g_hip_err = rccl().err;
        return ZK_ERR_COMM;
    }
    ncclUniqueId id;
    ZKCHK(rccl_check(rccl().GetUniqueId(&id), "ncclGetUniqueId"));
    memcpy(out, &id, sizeof id);
    return ZK_OK;
}
extern "C" int32_t zk_comm_create_rccl(zk_ctx *c, const uint8_t id_bytes[128], uint32_t world, uint32_t rank, zk_comm **out) {
    if (!id_bytes) return ZK_ERR_BAD_ARG;
    if (!rccl().ok) {
        g_hip_err = rccl().err;
        return ZK_ERR_COMM;
    }
    zk_comm *cm = nullptr;
    ZKCHK(comm_new(c, world, rank, &cm));
    Scoped<zk_comm, comm_delete> owner(cm);
    ZKCHK(use_device(c));   // ncclCommInitRank binds the communicator to the current device
    ncclUniqueId id;
    memcpy(&id, id_bytes, sizeof id);
    ZKCHK(rccl_check(rccl().CommInitRank(&cm->nccl, (int)world, id, (int)rank), "ncclCommInitRank"));
    cm->own_nccl = true;
    *out = owner.release();
    return ZK_OK;
}
extern "C" int32_t zk_comm_wrap_rccl(zk_ctx *c, void *nccl_comm, uint32_t world, uint32_t rank, zk_comm **out) {
    if (!nccl_comm) return ZK_ERR_BAD_ARG;
    if (!rccl().ok) {
        g_hip_err = rccl().err;
        return ZK_ERR_COMM;
    }
    zk_comm *cm = nullptr;
    ZKCHK(comm_new(c, world, rank, &cm));
    cm->nccl = (ncclComm_t)nccl_comm;
    cm->own_nccl = false;
    *out = cm;
    return ZK_OK;
}
extern "C" int32_t zk_comm_create_host(zk_ctx *c, uint32_t world, uint32_t rank, zk_host_allreduce_fn ar, zk_host_allgather_fn ag,
                                       zk_host_alltoall_fn a2a, void *user, zk_comm **out) {
    if (!ar || !ag) return ZK_ERR_BAD_ARG;   // alltoall is only needed by zk_ntt_sharded
    zk_comm *cm = nullptr;
    ZKCHK(comm_new(c, world, rank, &cm));
    cm->h_allreduce = ar;
    cm->h_allgather = ag;
    cm->h_alltoall = a2a;
    cm->user = user;
    *out = cm;
    return ZK_OK;
}
// What the transport itself reports (bench.py prints it so that a multi-GPU record shows N real RCCL ranks): RCCL's version
// (ncclGetVersion; 0 for the host-callback transport), and the communicator's own rank count / rank (ncclCommCount,
// ncclCommUserRank -- for the host transport the numbers the comm was created with).
extern "C" int32_t zk_comm_info(zk_comm *cm, int32_t *out_rccl_version, uint32_t *out_ranks, uint32_t *out_rank) {
    if (!cm) return ZK_ERR_BAD_ARG;
    int version = 0, count = (int)cm->world, urank = (int)cm->rank;
    if (cm->nccl) {
        ZKCHK(comm_alive(cm));
        if (rccl().GetVersion) ZKCHK(rccl_check(rccl().GetVersion(&version), "ncclGetVersion"));
        if (rccl().CommCount) ZKCHK(rccl_check(rccl().CommCount(cm->nccl, &count), "ncclCommCount"));
        if (rccl().CommUserRank) ZKCHK(rccl_check(rccl().CommUserRank(cm->nccl, &urank), "ncclCommUserRank"));
    }
    if (out_rccl_version) *out_rccl_version = version;
    if (out_ranks) *out_ranks = (uint32_t)count;
    if (out_rank) *out_rank = (uint32_t)urank;
    return ZK_OK;
}
extern "C" int32_t zk_comm_destroy(zk_comm *cm) {
    if (!cm) return ZK_OK;
    (void)hipSetDevice(cm->ctx->device);
    (void)hipStreamSynchronize(cm->ctx->stream);
    if (cm->nccl && cm->own_nccl) (void)rccl().CommDestroy(cm->nccl);
    if (cm->h_send) (void)hipHostFree(cm->h_send);
    if (cm->h_recv) (void)hipHostFree(cm->h_recv);
    delete cm;
    return ZK_OK;
}

// ---- host transport: device -> pinned, synchronise, callback, pinned -> device ------------------------------------------
static int32_t comm_stage(uint64_t **buf, size_t *cap, size_t bytes) {
    if (*cap >= bytes) return ZK_OK;
    if (*buf) (void)hipHostFree(*buf);
    *buf = nullptr;
    *cap = 0;
    size_t want = 4096;
    while (want < bytes) want <<= 1;
    HIPCHK(hipHostMalloc((void **)buf, want, hipHostMallocDefault));
    *cap = want;
    return ZK_OK;
}
static int32_t comm_host_call(zk_comm *cm, const uint64_t *d_send, size_t send_u64, uint64_t *d_recv, size_t recv_u64, int kind,
                              uint64_t n) {
    zk_ctx *c = cm->ctx;
    ZKCHK(comm_stage(&cm->h_send, &cm->h_send_bytes, send_u64 * 8));
    ZKCHK(comm_stage(&cm->h_recv, &cm->h_recv_bytes, recv_u64 * 8));
    HIPCHK(hipMemcpyAsync(cm->h_send, d_send, send_u64 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int32_t cb = 0;
    if (kind == 0) {
        cb = cm->h_allreduce(cm->user, cm->h_send, n);
        memcpy(cm->h_recv, cm->h_send, send_u64 * 8);
    } else if (kind == 1) {
        cb = cm->h_allgather(cm->user, cm->h_send, n, cm->h_recv);
    } else {
        cb = cm->h_alltoall(cm->user, cm->h_send, cm->h_recv, n);
    }
    if (cb != 0) {
        g_hip_err = "host transport callback returned " + std::to_string(cb);
        return ZK_ERR_COMM;
    }
    HIPCHK(hipMemcpyAsync(d_recv, cm->h_recv, recv_u64 * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // the staging buffer is reused by the next call
    return ZK_OK;
}
// lanes[i] <- sum over ranks, n uint64 lanes, in place
static int32_t comm_allreduce(zk_comm *cm, uint64_t *d_lanes, uint64_t n) {
    ZKCHK(comm_alive(cm));
    if (cm->nccl) return rccl_check(rccl().AllReduce(d_lanes, d_lanes, n, ncclUint64, ncclSum, cm->nccl, cm->ctx->stream), "ncclAllReduce");
    return comm_host_call(cm, d_lanes, n, d_lanes, n, 0, n);
}
// d_recv[r*n ..] <- rank r's d_send (n uint64 each)
static int32_t comm_allgather(zk_comm *cm, const uint64_t *d_send, uint64_t n, uint64_t *d_recv) {
    ZKCHK(comm_alive(cm));
    if (cm->nccl) return rccl_check(rccl().AllGather(d_send, d_recv, n, ncclUint64, cm->nccl, cm->ctx->stream), "ncclAllGather");
    return comm_host_call(cm, d_send, n, d_recv, n * cm->world, 1, n);
}
// d_recv[r*n ..] <- rank r's d_send[me*n ..] (n uint64 per peer)
static int32_t comm_alltoall(zk_comm *cm, const uint64_t *d_send, uint64_t *d_recv, uint64_t n) {
    ZKCHK(comm_alive(cm));
    if (cm->nccl) return rccl_check(rccl().AllToAll(d_send, d_recv, n, ncclUint64, cm->nccl, cm->ctx->stream), "ncclAllToAll");
    if (!cm->h_alltoall) return ZK_ERR_BAD_ARG;
    return comm_host_call(cm, d_send, n * cm->world, d_recv, n * cm->world, 2, n);
}

// ---- the sharded prover's whole loop (prove_partial on a table sharded by index mod world) ------------------------------
// phases (optional, 4 doubles, ms on the stream by HIP events -- each record stalls the stream ~4 us, so a run with phases is
// a breakdown, not a timing): [0] local kernels of the exchanging rounds ((fold +) sums -> lanes, lanes -> transcript step),
// [1] the per-round all-reduces, [2] pending fold + all-gather of the shard tails, [3] the replicated tail rounds.
// ZK_SHARD_FAKE_ALLREDUCE_US: a stand-in for a multi-rank all-reduce's latency on a one-rank communicator (measurements: every all-reduce
// of the loop is followed by a spin of this many microseconds on the stream)
static uint32_t shard_fake_allreduce_us() {
    static const uint32_t v = (uint32_t)env_u64("ZK_SHARD_FAKE_ALLREDUCE_US", 0, 0, 1000);
    return v;
}
static int32_t shard_run(zk_shard_prover *sp, zk_comm *cm, uint32_t gather_below, double *phases) {
    RoundState &st = sp->st;
    zk_ctx *c = st.c;
    const uint64_t n_lanes = (uint64_t)(st.D + 1) * 8;
    PhaseEvents ev(c);   // one event per mark, made as the loop goes
    auto mark = [&]() -> int32_t {
        if (!phases) return ZK_OK;
        ZKCHK(ev.push());
        return ev.record(ev.count() - 1);
    };
    // an rc chain: a failure between two collectives must reach comm_fail below (the peers would wait for ever)
    int32_t rc = mark();
    uint64_t exchanged = 0;
    while (rc == ZK_OK && sp->local_rounds - st.round > gather_below) {       // prover.rs:44-68, one collective per round
        rc = zk_shard_prover_round_begin(sp);                                  // (fold +) local sums -> digit lanes
        if (rc == ZK_OK) rc = mark();
        if (rc == ZK_OK) rc = comm_allreduce(cm, sp->lanes.as(), n_lanes);        // "the three partial sums", exact integer lane sums
        if (rc == ZK_OK && shard_fake_allreduce_us() && launch_spin_us(c->stream, shard_fake_allreduce_us()) != kLaunchOk) {
            g_hip_err = "spin kernel launch failed";
            rc = ZK_ERR_HIP;
        }
        if (rc == ZK_OK) rc = mark();
        if (rc == ZK_OK) rc = zk_shard_prover_round_finish(sp);                // mod p, absorb, squeeze: same challenge on every rank
        if (rc == ZK_OK) rc = mark();
        ++exchanged;
    }
    void *tail = nullptr;
    uint64_t elems = 0;
    if (rc == ZK_OK) rc = zk_shard_prover_tail_ptr(sp, &tail, &elems);
    if (rc == ZK_OK && !sp->gathered) rc = sp->gathered.alloc(c, (size_t)elems * 32 * sp->world);
    if (rc == ZK_OK) rc = comm_allgather(cm, (const uint64_t *)tail, elems * 4, sp->gathered.as());
    if (rc == ZK_OK) rc = mark();
    if (rc != ZK_OK) rc = comm_fail(cm, rc);     // the peers may be inside a collective this rank will never join
    if (rc == ZK_OK) rc = zk_shard_prover_tail_rounds(sp, sp->gathered.p);   // no collective after this point
    if (rc == ZK_OK) rc = mark();
    if (phases && rc == ZK_OK) {
        rc = hipStreamSynchronize(c->stream) == hipSuccess ? ZK_OK : ZK_ERR_HIP;
        auto span = [&](size_t a, size_t b) {
            double ms = 0.0;
            (void)ev.span_ms(a, b, &ms);
            return ms;
        };
        phases[0] = phases[1] = phases[2] = phases[3] = 0.0;
        if (rc == ZK_OK && ev.count() == 3 + 3 * exchanged) {
            for (uint64_t r = 0; r < exchanged; ++r) {
                phases[0] += span(3 * r, 3 * r + 1) + span(3 * r + 2, 3 * r + 3);
                phases[1] += span(3 * r + 1, 3 * r + 2);
            }
            phases[2] = span(3 * exchanged, 3 * exchanged + 1);
            phases[3] = span(3 * exchanged + 1, 3 * exchanged + 2);
        }
    }
    return rc;
}
static int32_t shard_run_args(zk_shard_prover *sp, zk_comm *cm) {
    if (!sp || !cm) return ZK_ERR_BAD_ARG;
    if (cm->ctx != sp->st.c) return ZK_ERR_CONTEXT_MISMATCH;
    if (cm->world != sp->world || sp->st.round != 0 || sp->tail_done) return ZK_ERR_BAD_ARG;   // a fresh prover, same world
    ZKCHK(comm_alive(cm));
    return use_device(sp->st.c);
}
extern "C" int32_t zk_shard_prover_run(zk_shard_prover *sp, zk_comm *cm, uint32_t gather_below) {
    ZKCHK(shard_run_args(sp, cm));
    return shard_run(sp, cm, gather_below, nullptr);
}
extern "C" int32_t zk_shard_prover_run_phases(zk_shard_prover *sp, zk_comm *cm, uint32_t gather_below, double out_ms[4]) {
    if (!out_ms) return ZK_ERR_BAD_ARG;
    ZKCHK(shard_run_args(sp, cm));
    return shard_run(sp, cm, gather_below, out_ms);
}

// ---- four-step NTT across the ranks (the layouts are documented at ShardedNtt in zk_amd/distributed.py) ----
//   X[k1 + M*k2] = sum_r w_W^(r*k2) * ( w_N^(r*k1) * NTT_M(shard r)[k1] ),  N = W*M, input x[r + W*j] on rank r
extern "C" int32_t zk_ntt_sharded(zk_ctx *c, zk_comm *cm, const zk_mle *shard, int32_t inverse, zk_mle *out) {
    if (!c || !cm || !shard || !out) return ZK_ERR_BAD_ARG;
    if (cm->ctx != c || shard->ctx != c || out->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    if (shard->n_vars != out->n_vars || shard->d == out->d) return ZK_ERR_BAD_ARG;
    ZKCHK(comm_alive(cm));
    uint32_t lw = 0;
    while ((1u << lw) < cm->world) ++lw;
    const uint64_t m = shard->n_vars;
    if (m < lw || lw > 10) return ZK_ERR_BAD_ARG;
    const FieldParams &P = c->fi->P;
    Fe w_n;
    if (!field_root_of_unity(*c->fi, (uint32_t)(m + lw), w_n)) return ZK_ERR_FFT_NO_ROOT;   // fft/src/lib.rs:6
    if (inverse) w_n = fe_inverse(w_n, P);                                                  // :14
    uint64_t tw[4], scale[4];
    fe_to_u64limbs(fe_pow_u64(w_n, cm->rank, P), tw);                                       // w_N^rank: the base of this rank's twiddles
    Fe sc = fe_one(P);
    if (inverse) {                                                                          // :17 -- 1/N = (1/M from the local ifft) * 1/W
        const uint64_t wl[4] = {cm->world, 0, 0, 0};
        sc = fe_inverse(fe_from_canonical(fe_from_u64limbs(wl), P), P);
    }
    fe_to_u64limbs(sc, scale);
    ZKCHK(use_device(c));
    MleHolder a;   // stream-ordered reuse when the call returns
    ZKCHK(mle_alloc(c, m, a.put()));
    const uint64_t per_peer = ((uint64_t)4 << m) / cm->world;   // uint64 words each pair of ranks exchanges
    int32_t rc;   // a chain: a failure before the exchange must reach comm_fail
    bool exchanged = false;   // the one collective has been enqueued / completed: a later failure is local and strands no peer
    if (!inverse) {   // shard -NTT-> out -twiddle-> out =all-to-all=> a -across-> out
        rc = zk_ntt(c, shard, 0, out);
        if (rc == ZK_OK) rc = zk_mle_mul_powers(c, out, tw, scale);
        if (rc == ZK_OK) rc = comm_alltoall(cm, out->d, a->d, per_peer);
        exchanged = rc == ZK_OK;
        if (rc == ZK_OK) rc = zk_dft_across(c, a.get(), out, lw, 0);
    } else {          // shard -across-> out =all-to-all=> a -twiddle-> a -iNTT-> out
        rc = zk_dft_across(c, shard, out, lw, 1);
        if (rc == ZK_OK) rc = comm_alltoall(cm, out->d, a->d, per_peer);
        exchanged = rc == ZK_OK;
        if (rc == ZK_OK) rc = zk_mle_mul_powers(c, a.get(), tw, scale);
        if (rc == ZK_OK) rc = zk_ntt(c, a.get(), 1, out);
    }
    // a rank that failed before / in the all-to-all must not leave its peers waiting in it; a failure AFTER the exchange is this
    // rank's own and leaves the communicator usable
    return exchanged ? rc : comm_fail(cm, rc);
}

// ---- the sharded layout back to the natural order on every rank: one all-gather of the shards (rank-major) + the interleave ----
extern "C" int32_t zk_mle_unshard(zk_ctx *c, zk_comm *cm, const zk_mle *shard, zk_mle **out) {
    if (!c || !cm || !shard || !out) return ZK_ERR_BAD_ARG;
    if (cm->ctx != c || shard->ctx != c) return ZK_ERR_CONTEXT_MISMATCH;
    ZKCHK(comm_alive(cm));
    const uint64_t m = shard->n_vars;
    if (m + log2_world(cm->world) > kMaxVars) return ZK_ERR_UNSUPPORTED;
    ZKCHK(use_device(c));
    PoolBlock d_all;   // stream-ordered reuse when the call returns
    // a chain: a failure before the one collective must reach comm_fail
    int32_t rc = d_all.alloc(c, ((size_t)32 << m) * cm->world);
    if (rc == ZK_OK) rc = comm_allgather(cm, shard->d, (uint64_t)4 << m, d_all.as());   // [world][2^m], rank-major
    if (rc != ZK_OK) return comm_fail(cm, rc);
    return shard_interleave(c, {}, d_all.as(), cm->world, m, out);   // after the collective a failure is this rank's own
}
