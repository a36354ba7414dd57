"""The sumcheck and evaluate kernels on worst-case Montgomery limbs (tests/extreme_tables.py; tests/test_extreme_tables_host.py pins the
builders and says why a table of the value p - 1 is not the worst case).  The round kernels accumulate up to kMaxLazy = 32 unreduced
products of stored limbs per lane (wide_mac / redc_wide), 63 products per 29-bit column between normalisations (dot29_mac), 8 rows x 5
products per column (eval_mac): these tables put the largest representation M = p - 1, the all-ones representation O and exact zeros
through every kernel that relies on such a bound, and compare bit for bit with the CPU oracle and with closed forms in Python integers.

One child process per kernel-selecting switch set (tests/extreme_tables_check.py; the library reads its ZK_* switches once per
process), started as tests/test_gpu_parity.py starts its sweeps: the oracle answers once, on CPU-only workers, then the children four
at a time, each under its own time limit, nothing retried.  The switch sets are that file's (SKIP1_RUNS) and
tests/test_gpu_forced_paths.py's (FINISHER_SETTINGS); ZK_ROUND_MIN_BLOCKS=1 gives the round kernels as few workgroups as the lazy
limit allows, so that a lane holds 32 products at n = 15.

The pipeline never takes round 0 (sumcheck.hip, pipe_wants_next: it prepares round r + 1), so its first round has 2^(n - 2) pairs: the cap
kPipeMaxWorkBlocks * 16 * kMaxLazy = 2^17 pairs, 32 products per lane, is reached at n = 19, not 18 (at n = 18 a lane holds 16, and
redc_wide without its top-word term still passes on BN254 there).

Cuts for time: n = 19 runs on BN254 and BLS12-381 only; the (3, 3) shape at n >= 16 on BN254 only."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import zk_amd
from zk_amd import MultiLinearPolynomial as MLE
from zk_amd import ProductPoly

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extreme_tables as et  # noqa: E402
import extreme_tables_check as check  # noqa: E402
from test_gpu_forced_paths import FINISHER_SETTINGS  # noqa: E402
from test_gpu_parity import _SWEEP_ENV_KEYS, SKIP1_RUNS  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "extreme_tables_check.py")
FIELDS = [zk_amd.BN254_FR, zk_amd.BLS12_381_FR, zk_amd.BLS12_377_FR]
FIELD_IDS = ["bn254", "bls12_381", "bls12_377"]
_ENV_KEYS = _SWEEP_ENV_KEYS + ("ZK_ROUND_MIN_BLOCKS", "ZK_FINISH_PIPE", "ZK_EVAL_STREAM_MIN", "ZK_EVAL_STREAM_LEAVE", "ZK_EVAL_WEIGHT",
                               "ZK_ORACLE_CACHE")
FEW_BLOCKS = dict(ZK_ROUND_MIN_BLOCKS="1")


def _set(name, sizes, fields=3, **more):
    switches = {k: v for k, v in SKIP1_RUNS[name].items() if k not in ("ZK_CHECK_SIZES", "ZK_CHECK_FIELDS")} if name else {}
    return dict(switches, ZK_CHECK_SIZES=sizes, ZK_CHECK_FIELDS=str(fields), **more)


# name -> environment of the child: the kernels it reaches, and what a lane accumulates
RUNS = {
    # quad, pipe, finishers, k_round_kd at the shipped thresholds
    "defaults": _set(None, "3,7,11,13,14,16"),
    # k_round0_dot29, LEAD / SKIP1 k_round_kd: 32 products per lane from n = 15
    "lead_skip1_classic": _set("lead_skip1_classic", "7,13,15,16", **FEW_BLOCKS),
    # k_round_kd<2,2,sums only,LEAD> in round 0: 32 products per lane at n = 15
    "round0_wide": _set("round0_wide", "9,15", **FEW_BLOCKS),
    # k_round0_dot29<1> (the two-term shape): 32 pair indices per lane at n = 15
    "round0_dot29_terms": _set("round0_dot29_terms", "9,14,15", **FEW_BLOCKS),
    # k_round0_glds<0/1>, k_round_fused_glds<3,0> and <2,1>, cached and nontemporal: 32 runs per wave at n = 15
    "glds_classic_tails": _set("glds_classic_tails", "7,8,9,13,15", **FEW_BLOCKS),
    # the LDS-DMA kernels, then the pipeline
    "glds_then_pipe": _set("glds_then_pipe", "12,13"),
    # k_round_quad<2,2,0>, <3,3,0>, <2,2,1> and the batched twins
    "quad_classic_tails": _set("quad_classic_tails", "7,11,13,15"),
    # k_round_pipe, k_finish_pipe; at n = 19 round 1 has 2^17 pairs = kPipeMaxWorkBlocks * 16 * kMaxLazy: 32 products per lane
    "pipe_from_2p17_after_skip1": _set("pipe_from_2p17_after_skip1", "12,17,18"),
    "pipe_from_2p17_after_skip1_n19": _set("pipe_from_2p17_after_skip1", "19", fields=2),
    # k_finish, k_finish_terms
    "classic_finisher": dict(FINISHER_SETTINGS["classic_finisher"], ZK_CHECK_SIZES="3,7,11", ZK_CHECK_FIELDS="3"),
}


def _base_env():
    return {k: v for k, v in os.environ.items() if k not in _ENV_KEYS}


def _sizes(extra):
    return tuple(int(x) for x in extra["ZK_CHECK_SIZES"].split(","))


@pytest.fixture(scope="module")
def sweeps(tmp_path_factory):
    """prefill the oracle cache for the union of the runs' grids, then start every child (four at a time); -> {name: Future}"""
    from concurrent.futures import ThreadPoolExecutor

    import oracle_cache

    cache = str(tmp_path_factory.mktemp("extreme_oracle_cache"))
    base = dict(_base_env(), ZK_ORACLE_CACHE=cache)
    spec = []
    for extra in RUNS.values():
        spec += check.spec(_sizes(extra), int(extra["ZK_CHECK_FIELDS"]))
    os.environ["ZK_ORACLE_CACHE"] = cache
    try:
        oracle_cache.prefill(spec, workers=min(12, max(2, (os.cpu_count() or 4) - 2)))
    finally:
        del os.environ["ZK_ORACLE_CACHE"]

    def child(extra):
        return subprocess.run([sys.executable, CHECK], env=dict(base, **extra), capture_output=True, text=True, timeout=600, cwd=ROOT)

    pool = ThreadPoolExecutor(max_workers=4)
    # the longest first
    order = sorted(RUNS, key=lambda name: -max(_sizes(RUNS[name])))
    futures = {name: pool.submit(child, RUNS[name]) for name in order}
    yield futures
    pool.shutdown(wait=True)


@pytest.mark.parametrize("name", list(RUNS))
def test_rounds_and_proofs_on_extreme_tables(sweeps, name):
    """round_sums, prove_partial (right and wrong claim, kept and consumed tables), prove_partial_batch, the two-term shape, prod_reduce
    and partial_evaluate of every family at every size of the switch set, on all its fields.  A failure names its switch set, and the
    child's assertion the family, shape and size."""
    r = sweeps[name].result()
    assert r.returncode == 0, f"{RUNS[name]} exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    m = re.search(r"^extreme ok: (\d+) checks", r.stdout, re.M)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) == check.expected_checks(_sizes(RUNS[name]), int(RUNS[name]["ZK_CHECK_FIELDS"]))


@pytest.mark.parametrize("n", [6, 9, 12, 16])
@pytest.mark.parametrize("field", FIELDS, ids=FIELD_IDS)
def test_evaluate_on_extreme_tables(field, n):
    """MLE.evaluate and ProductPoly.evaluate (k_eval_sum, k_eval_low, k_evaluate_tail) of const(M), const(O), step(Z,O) and stripe(O,Z) at
    a point of M / O representations, a random point, all zeros and all ones: oracle and closed form"""
    ctx = zk_amd.Context(field, 0)
    try:
        assert check.check_evaluate(ctx, field, n) == 2 * 4 * len(check.EVAL_TABLES)
    finally:
        ctx.close()


@pytest.mark.parametrize("weight", [None, "0"], ids=["weighted", "unweighted"])
def test_streaming_evaluate_on_all_ones_halves(weight):
    """k_eval_stream (half an element per lane, 8 rows x 5 products per 29-bit column, the 13-column -> 16-word repack) forced from 19
    variables: n = 19 (L = 10) and n = 20 on all three fields, tables whose 128-bit halves are all ones; with its outputs weighted
    (shipped) and with ZK_EVAL_WEIGHT=0"""
    env = dict(_base_env(), ZK_EVAL_STREAM_MIN="19", ZK_CHECK_SIZES="19,20", ZK_CHECK_FIELDS="3")
    if weight is not None:
        env["ZK_EVAL_WEIGHT"] = weight
    r = subprocess.run([sys.executable, CHECK, "eval"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert f"extreme evaluate ok: {3 * 2 * 2 * 4 * len(check.EVAL_TABLES)} evaluations (ZK_EVAL_STREAM_MIN=19" in r.stdout, r.stdout[-2000:]


@pytest.fixture(scope="module")
def all_ones_2p24():
    """const(O) on 2^24 BN254 elements and its closed form as both factors of a product"""
    field = zk_amd.BN254_FR
    tabs, closed = et.family(field, "const(O)", 24, 2)
    return field, tabs[0], closed


def test_round0_glds_beyond_one_flush_at_2p24(all_ones_2p24):
    """round_sums(2) of const(O) x const(O) at n = 24 (one handle listed twice): k_round0_glds<0> is capped at 512 workgroups, so a wave
    runs 64 runs -- the smallest size at which the lazy == kMaxLazy flush happens before the last run -- with every 29-bit column sum
    at its maximum.  The closed form 2^23 v(O)^2 is the check."""
    field, tab, closed = all_ones_2p24
    ctx = zk_amd.Context(field, 0)
    try:
        t = MLE.new(ctx, 24, tab)
        got = ProductPoly.new([t, t]).round_sums(2)
        t.free()
    finally:
        ctx.close()
    assert np.array_equal(got, et.elems(field, closed.round_sums(2)))


def test_quad_rounds_at_32_products_per_lane_at_2p24(all_ones_2p24):
    """k_round_quad<2,2,0> at its limit (a child: the switches are read once per process).  A fused round folds before it sums, so at
    n = 24 round 1 has 2^22 pairs; ZK_QUAD_MAX_PAIRS=2^22 admits it to the quad kernel, whose grid is capped at 2048 workgroups of 64
    pair indices: 32 products per lane.  launch_round tries the LEAD + SKIP1 k_round_kd first, from 2^16 pairs by default, so
    ZK_LEAD_MIN_PAIRS and ZK_SKIP1_MIN_PAIRS are put out of reach; ZK_PIPE_MAX_PAIRS=0 keeps the quad kernel for the small rounds too.
    const(O) (the table of the test above) and const(M), the only fill whose 32 products reach a non-zero top word on BN254: all 24
    round polynomials of each against the closed form, the challenges against pyref's verifier replaying the transcript."""
    field, tab, closed = all_ones_2p24
    assert np.array_equal(tab[:4], et.family(field, "const(O)", 2, 2)[0][0])   # the child builds the same rows
    env = dict(_base_env(), ZK_QUAD_MAX_PAIRS=str(1 << 22), ZK_PIPE_MAX_PAIRS="0", ZK_LEAD_MIN_PAIRS=str(1 << 40), ZK_SKIP1_MIN_PAIRS=str(1 << 40))
    r = subprocess.run([sys.executable, CHECK, "quad24"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert ("extreme quad24 ok: 2 x 24 rounds (ZK_QUAD_MAX_PAIRS=4194304 ZK_PIPE_MAX_PAIRS=0 ZK_LEAD_MIN_PAIRS=1099511627776 "
            "ZK_SKIP1_MIN_PAIRS=1099511627776)") in r.stdout, r.stdout[-2000:]
