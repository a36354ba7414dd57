// env.hpp -- the library's ZK_* environment switches, parsed in one place.
//
// Every switch is a tuning / A-B / debug override read ONCE per process (function-local statics at the call sites); none of
// them selects a different implementation of the arithmetic -- only thresholds and kernel choices that all produce the same
// bits (tests/skip1_check.py, tests/test_gpu_parity.py, tests/test_gpu_forced_paths.py and their neighbours force each of them in
// child processes; tests/test_switch_coverage.py fails when a switch other than the debug / timing ones is named by no test).  The
// list with defaults and accepted ranges is in INTEGRATION.md section 7 and at the end of include/zk_amd.h.
//
// zk_upoly_evaluate_many reads ZK_UPOLY_EVALMANY_DIRECT_MAX (0 .. 2^40; unset: a cost model): shapes with n * len(p) at most this
// take the direct kernel, the others the transposed tree, 0 meaning the tree wherever its length rule allows it; and
// zk_upoly_interpolate_xy reads ZK_UPOLY_INTERP_XY_TREE_MIN (1 .. 2^40): from that many points on its weights' denominators come from
// that tree path instead of the O(nx m) kernel (ntt.hip; tests/test_gpu_upoly_evalmany.py forces both ends of both).
//
// zk_upoly_divrem reads ZK_UPOLY_DIVREM_DIRECT_MAX (0 .. 2^40, values above the kernel's 2048 count as 2048; default 1023, below the smallest measured size at which Newton wins): dividends
// of at most this many coefficients take the one-workgroup schoolbook kernel, 0 meaning never; and ZK_UPOLY_DIVREM_LINEAR (default 1):
// 0 sends divisors of two coefficients to the other paths instead of the affine scan (ntt.hip; tests/test_gpu_upoly_divrem.py forces
// the direct kernel, the Newton path and the scan in child processes).
//
// zk_mle_batch_inverse / zk_upoly_batch_inverse / zk_batch_inverse_host read ZK_BATCH_INV_ONE_LAUNCH_MAX (0 .. 2048, default 2048 = one
// chunk): lengths up to it run in one launch of one workgroup, longer ones in three launches, 0 meaning always three (inv.hip;
// tests/test_gpu_batch_inverse.py forces both in child processes).
//
// zk_merkle_commit reads ZK_MERKLE_FUSE_LEVELS (0 .. 10): 0 builds the tree with one launch per level, s > 0 with fused stages in which a
// workgroup climbs s levels over a tile of 2^s digests in LDS (merkle.hip; tests/test_gpu_merkle.py forces 0, 3, 10 and the default in
// child processes).
//
// zk_fri_fold / zk_fri_prove read ZK_FRI_FUSED_FOLD (0 .. 1, default 1): 1 folds a layer by 2^a in one launch of k_fri_fold<a>, 0 in a
// launches of k_fri_fold<1> through intermediate layers (fri.hip; tests/test_gpu_fri.py forces 0, 1 and the default in child processes).
//
// zk_mlpcs_open reads ZK_MLPCS_ROUND (0 .. 1): 1 runs the sumcheck side of an opening on the fused round kernel (no eq table, the fold of
// T joined to the round's sums), 0 on zk_eq_table with the two-table round sums and two folds per round (mlpcs.hip;
// tests/test_gpu_mlpcs.py forces 0, 1 and the default in child processes).
//
// zk_mlbatch_open reads ZK_MLBATCH_FUSE_FOLD (0 .. 1, default 1): 1 combines the k committed codewords and folds them in one pass
// (k_ml_combine_fold: the combined layer 0 is never written), 0 writes it with k_ml_lincomb and folds it with FRI's kernel (mlbatch.hip;
// tests/test_gpu_mlbatch.py forces 0, 1 and the default in child processes).
//
// zk_mle_product_tree / zk_gprod_prove read ZK_GPROD_TREE_FUSE (0 .. 3, 0 = the default): the levels of the product tree one launch of
// k_ptree takes above the one-workgroup LDS stage (gprod.hip; tests/test_gpu_gprod.py forces 1, 2, 3 and the default in child processes).
//
// zk_mle_fraction_tree / zk_fsum_prove read ZK_FSUM_TREE_FUSE (0 .. 2, 0 = the default): the levels of the fraction tree one launch of
// k_ftree takes above the one-workgroup LDS stage (fsum.hip; tests/test_gpu_fsum.py forces 1, 2 and the default in child processes).
//
// zk_perm_prove reads ZK_PERM_FUSE (0 .. 1, default 0): 0 writes the fingerprint table with k_perm_leaves and runs the product tree over
// it, 1 writes it and the tree's first levels in one launch of k_perm_tree (at most two levels; the arity follows ZK_GPROD_TREE_FUSE);
// and ZK_PERM_MAX_GRID (1 .. 16384): the cap of that launch's grid, above which its waves loop (perm.hip; tests/test_gpu_perm.py forces
// both routes, every arity and a grid of one workgroup in child processes).
//
// A value that does not parse as a whole decimal number, or lies outside the accepted range, is IGNORED (the default
// applies) and reported once on stderr: a mistyped switch must not silently change the kernel selection.
#pragma once
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

namespace zk {

inline uint64_t env_u64(const char *name, uint64_t dflt, uint64_t lo, uint64_t hi) {
    const char *e = getenv(name);
    if (!e) return dflt;
    char *end = nullptr;
    errno = 0;
    const unsigned long long v = strtoull(e, &end, 10);
    const bool numeric = *e != '\0' && *e != '-' && *e != '+' && end && *end == '\0' && errno == 0;
    if (!numeric || v < lo || v > hi) {
        fprintf(stderr, "zk_amd: %s=\"%s\" ignored (accepted: whole numbers %llu..%llu; default %llu applies)\n", name, e,
                (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)dflt);
        return dflt;
    }
    return (uint64_t)v;
}
// set (to anything but "0" or the empty string) = on
inline bool env_flag(const char *name) {
    const char *e = getenv(name);
    return e && e[0] != '\0' && !(e[0] == '0' && e[1] == '\0');
}

}  // namespace zk
