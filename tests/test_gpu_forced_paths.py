"""Shipped kernel paths that the default thresholds keep out of the suite, forced by their switches.  The library reads every ZK_*
switch once per process, so each setting is a child process (tests/forced_paths_check.py, tests/skip1_check.py, or the neighbouring
tests themselves under the switch); every comparison is bit for bit against the oracle the neighbouring tests use.

  ZK_NTT_FULL_TABLE_MAX_LOG   0: every inter-pass twiddle composed (ntt_twiddle: w_lo x w_hi by fe_mul29) -- also what runs when a
                              table allocation fails; 12: a three-pass transform (lg = 17) with pass 0 composed and pass 1 from a table
  ZK_FINISH_PIPE=0            the classic finisher where the pipelined one takes over by default
  ZK_PUBLISH_IN_FINISHER=0    publication by k_publish_host, single proofs and batches
  ZK_UPOLY_INTERP_DIRECT_LOG  8: k_interp_tree_direct<8> (256 threads)"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "forced_paths_check.py")
SWITCHES = ("ZK_NTT_FULL_TABLE_MAX_LOG", "ZK_FINISH_PIPE", "ZK_PUBLISH_IN_FINISHER", "ZK_UPOLY_INTERP_DIRECT_LOG")


def _env(**extra):
    return dict({k: v for k, v in os.environ.items() if k not in SWITCHES}, **extra)


def _child(args, env, timeout):
    """one child under its own time limit; nothing is retried"""
    r = subprocess.run([sys.executable] + args, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, f"{args} exit {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}"
    return r.stdout


@pytest.mark.parametrize("max_log", ["0", "12"])
def test_ntt_with_composed_twiddles(max_log):
    out = _child([CHECK, "ntt"], _env(ZK_NTT_FULL_TABLE_MAX_LOG=max_log), 600)
    print(out)
    assert "forced ntt ok" in out
    plan17 = [ln for ln in out.splitlines() if ln.startswith("plan lg=17:")][0]
    if max_log == "12":   # one pass with a table and one without, in the same transform
        assert "pass 0: 2^17 composed" in plan17 and "pass 1: 2^11 table" in plan17, plan17
    else:
        assert "table" not in plan17, plan17


FINISHER_SETTINGS = {
    "classic_finisher": dict(ZK_FINISH_PIPE="0"),
    "publish_by_its_own_kernel": dict(ZK_PUBLISH_IN_FINISHER="0"),
    "classic_finisher_and_publish_by_its_own_kernel": dict(ZK_FINISH_PIPE="0", ZK_PUBLISH_IN_FINISHER="0"),
}


@pytest.mark.parametrize("name", list(FINISHER_SETTINGS))
def test_finisher_and_publication_paths_match_the_oracle(name):
    """zk_sumcheck_prove over the (k, D, n) grid of test_sumcheck_matches_oracle with and without absorbed tables (that test itself,
    run under the switches), then tests/skip1_check.py: n = 2, 3 (the edge of finish_pipe_applies), 7, 11, 13 with right and wrong
    claims, a zk_sumcheck_prove_batch of three proofs per shape, and the two-term shape with its final evaluations requested --
    every transcript against the oracle's."""
    env = _env(**FINISHER_SETTINGS[name])
    out = _child(["-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join("tests", "test_gpu_parity.py"), "-k",
                  "test_sumcheck_matches_oracle"], env, 900)
    assert " passed" in out and "failed" not in out and "skipped" not in out, out[-2000:]
    out = _child([os.path.join(ROOT, "tests", "skip1_check.py")], dict(env, ZK_CHECK_SIZES="2,3,7,11,13"), 900)
    assert "skip1 ok" in out, out[-2000:]


def test_interp_direct_level_of_256_threads():
    """ZK_UPOLY_INTERP_DIRECT_LOG=8 (k_interp_tree_direct<8>): the small-size restatement and the 2^16 +- 1 Schwartz-Zippel cases of
    tests/test_gpu_upoly_interp.py under the switch, and the coefficients byte-identical to the default setting's"""
    env8 = _env(ZK_UPOLY_INTERP_DIRECT_LOG="8")
    out = _child(["-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join("tests", "test_gpu_upoly_interp.py"), "-k",
                  "test_interpolate_small_sizes_against_restatement or (test_random_ys_schwartz_zippel and not 1048576)"], env8, 900)
    assert "9 passed" in out and "failed" not in out and "skipped" not in out, out[-2000:]
    digests = {}
    for name, env in (("default", _env()), ("8", env8)):
        out = _child([CHECK, "interp"], env, 600)
        assert "forced interp ok" in out
        digests[name] = [ln for ln in out.splitlines() if ln.startswith("DIGEST")]
    assert digests["default"] == digests["8"] and len(digests["8"]) == 3 * 53
