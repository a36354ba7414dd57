// prover_state.hpp -- the state of one sumcheck prover between its launches: owned by the prover in sumcheck.hip, which alone steps it; comm.hip's
// run loop reads the sharded prover's round counters and exchange buffers, gkr.hip sizes the E-partial block of a DeviceChain.
#pragma once
#include "host_core.hpp"

constexpr size_t kChalWords = kChallengeBytes / 8;                                   // one challenge record, in u64
constexpr size_t kEpartBytes = (size_t)(kPipeMaxWorkBlocks + 2) * 16 * 32;         // E partials of one pipelined round (+ total + counter)
constexpr size_t kChalBlockBytes = 2 * kChallengeBytes + 32;   // two challenge records + the claim element
constexpr size_t kEpartBlockBytes = 2 * kEpartBytes + 16;      // two E-partial buffers + their two last-block-done counters
struct ProverScratch {
    WordSponge *d_sponge;
    uint64_t *d_challenge;   // TWO challenge records (round s uses slot s & 1): a pipelined launch reads r_{s-2} while r_{s-1} is written
    uint64_t *d_claim;       // one element behind them: the claim S_prev(r_prev) a SKIP1 round kernel parks for its tail (ClaimJob).  Per
                             // PROVER, not per context: the sharded prover keeps it live from round_begin to round_finish, across API
                             // calls in which other provers of the same context may run their own SKIP1 rounds
    uint64_t *d_epart;       // two E-partial buffers (pipelined rounds), same alternation
    uint64_t *d_rp;          // rounds * (D+1) elements
    uint64_t *d_ch;          // rounds elements
    uint64_t *d_final;       // kMaxFactors elements (same block as d_rp, d_ch)
    size_t rp_bytes, ch_bytes;
    bool external;           // sponge and the three outputs belong to a DeviceChain (not allocated / freed here)
    // the owners behind the pointers above; with a DeviceChain only the challenge block is owned
    PoolBlock sponge_block, chal_block, epart_block, proof_block;
    size_t proof_block_bytes() const { return rp_bytes + ch_bytes + kMaxFactors * 32; }
};
// A caller that keeps ONE transcript on the device across several sumchecks (the GKR driver): the sponge already holds
// everything absorbed so far INCLUDING this sumcheck's claimed sum; round polynomials, challenges and the factor values at
// the point are written straight to the caller's device buffers; nothing is copied to the host and nothing waits.
struct DeviceChain {
    WordSponge *d_sponge;
    uint64_t *d_rp, *d_ch, *d_final;
    uint64_t *d_epart;   // E-partial buffers + counters shared by the chain's sumchecks (counters zero between launches)
};
// the initial sponge of a single proof, not stored yet: the first classic tail takes it as an argument (k_round_tail_init); any other
// first consumer stores it first (flush_pending_sponge)
struct PendingSponge {
    WordSponge w;
    WordSponge *dst;
    uint64_t *zero2;
    bool valid;
};
// (a default-constructed state is the empty state: round_state_init sets what depends on its arguments)
struct RoundState {
    zk_ctx *c = nullptr;
    uint64_t k = 0;
    uint64_t vars_left = 0;           // variables of the tables in `cur` (before any pending fold)
    uint64_t round = 0;               // rounds completed
    uint32_t D = 0;
    bool pending_fold = false;        // the last challenge has not been applied to `cur` yet (it is fused into the next round)
    bool first_out_of_place = false;  // next fold must leave `cur` intact (caller keeps the inputs): write to scratch
    uint64_t *cur[kMaxFactors] = {};  // current tables (device)
    PoolBlock scratch[kMaxFactors];   // owned tables
    ProverScratch ps = {};
    TermSpec terms = {};              // how the k flat factors group into products (one term = ProductPoly)
    uint64_t *d_final = nullptr;      // optional (= ps.d_final when requested): the factors at the challenge point
    TailDerive dv = {};               // Lagrange weights on 0..D (prev_rp is set per round)
    // pipelined rounds (pipe_kernels.cuh): the E partials of round `round` already exist (computed from `cur`, the table of
    // round - 1, before its challenge was known); `cur` still awaits that fold (pending_fold is true)
    bool pipe_active = false;
    uint32_t pipe_blocks = 0;         // work blocks that wrote them
    bool pipe_total = true;           // slot 0 of their buffer holds the total (k_round_pipe: the block that finishes last adds them up);
                                      // false: the next launch's transcript block (or the finisher) adds the pipe_blocks partials up
    PendingSponge init = {};          // valid: the initial sponge is still on the host side of the launch queue (prove_core)
    FinishPublish pub = {};           // flag != null: the pipelined finisher, being the call's last launch, publishes the proof block itself
    bool published = false;           // ... and has been enqueued with that job
};
struct zk_shard_prover {
    RoundState st;
    uint32_t world = 0;
    uint64_t local_rounds = 0, total_rounds = 0;
    PoolBlock lanes;         // (D+1)*8 u64 lanes
    TailDerive lanes_dv = {};   // what round_finish derives from the all-reduced lanes (set by round_begin)
    PoolBlock tail;          // k * 2^tail_s elements: this rank's shard tables at the moment of the gather
    uint32_t tail_s = 0;     // variables left in the local tables when gathered
    bool tail_done = false;
    PoolBlock gathered;      // zk_shard_prover_run: the all-gathered tails [world][k][2^tail_s]
};
