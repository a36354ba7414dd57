// ntt_plan.hpp -- the pass plan of one transform size (built by ntt.hip, read by the kernels of ntt_kernels.cuh, cached in the context).
#pragma once
#include <stdint.h>

namespace zk {

// Twiddles are stored ready for the carry-free multiplier (field.cuh fe_mul29): every multiplication of the transform
// has a table value as one operand, so the tables hold omega^e * 2^5 mod p -- the low table already split into nine
// 29-bit limbs (Mul29, 64-byte records), the high table as a plain element so that two levels compose with one more
// fe_mul29:  hi' (x) lo' = (w_hi 2^5)(w_lo 2^5) 2^-261 = (w_hi w_lo) 2^5, again a prepared value.
constexpr int kTw29Words = 16;   // record stride of a stored Mul29 (9 words used)
struct NttPlan {
    uint32_t log_n;
    uint32_t n_pass;
    uint32_t l[4];          // log2 radix of each pass
    uint32_t lo_bits;       // two-level table: w_lo[i] ~ omega^i (i < 2^lo_bits), w_hi[i] ~ omega^(i << lo_bits)
    const uint32_t *w_lo;   // Mul29 records of omega^i
    const uint64_t *w_hi;   // elements omega^(i << lo_bits) * 2^5 mod p
    // optional full inter-pass twiddle table of pass p < P: element (k, i) at [k * I_p + i] = omega^(O_p * i * k) * 2^5 mod p,
    // R_p * I_p = n / O_p entries (the whole vector for pass 0, n / R_1 for pass 1, ...).  Trades the compose multiply
    // for a 32-byte read in a pass that is bound by VALU issue, not HBM.  Null: compose from the two-level table.
    const uint64_t *w_full[4];
};

}  // namespace zk
