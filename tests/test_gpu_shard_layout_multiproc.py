"""Sharding by index mod world across processes: every rank builds its shard from the same natural-order host table with
MultiLinearPolynomial.new_shard (zk_mle_upload_shard), proves with zk_shard_prover_run, and gets the natural order back with
zk_amd.distributed.unshard (zk_mle_unshard: all-gather + interleave), also after the sharded inverse NTT.  Fresh child processes
on cuda:0 exchange over gloo through HostComm, as in tests/test_gpu_multiproc.py; unshard over RCCL runs at world 1 in-process."""
import datetime
import json
import os
import socket
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch.distributed as dist

    # a rank that fails leaves the others inside a collective: bound that wait
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))
    report = {"rank": rank, "cases": 0, "errors": []}
    try:
        import zk_amd
        from oracle import binding as orc
        from zk_amd import MultiLinearPolynomial as MLE
        from zk_amd import ProductPoly
        from zk_amd.distributed import GpuShardBackend, HostComm, ntt_sharded, sliced_shard_of, unshard

        lw = world.bit_length() - 1
        for field in (zk_amd.BN254_FR, zk_amd.BLS12_381_FR):
            ctx = zk_amd.Context(field, 0)
            comm = HostComm(ctx)
            for n, k, D in ((12, 2, 2), (15, 3, 3), (16, 2, 2)):
                tabs = [orc.fill_random(field, 8100 + 16 * n + f, 1 << n) for f in range(k)]
                claimed = orc.sum_elems(field, orc.prod_reduce(field, n, tabs))   # iter().sum::<F>()
                want_rp, want_ch = orc.sumcheck_prove(field, n, tabs, D, claimed, False)
                shards = [MLE.new_shard(ctx, n, t, world, rank) for t in tabs]
                for f, s in enumerate(shards):   # before the prover consumes them: every rank gets the whole table back
                    report["cases"] += 1
                    if not np.array_equal(unshard(comm, s).evaluation_slice(), tabs[f]):
                        report["errors"].append(f"unshard field={field} n={n} factor={f}")
                backend = GpuShardBackend(ProductPoly.new(shards), D, claimed, world)
                rp, ch = backend.run(comm, 10)
                report["cases"] += 1
                if not (np.array_equal(rp, want_rp) and np.array_equal(ch, want_ch)):
                    report["errors"].append(f"prover field={field} n={n}")
                backend.close()
            # the sharded inverse NTT returns the strided layout; unshard puts it back in natural order
            for log_n in (10, 13):
                x = orc.fill_random(field, 4500 + log_n, 1 << log_n)
                X = orc.ntt_fast(field, x, False)
                Xs = MLE.new(ctx, log_n - lw, sliced_shard_of(X, rank, world))
                report["cases"] += 2
                if not np.array_equal(unshard(comm, ntt_sharded(comm, Xs, True)).evaluation_slice(), x):
                    report["errors"].append(f"unshard of the inverse ntt field={field} log_n={log_n}")
                fwd = ntt_sharded(comm, MLE.new_shard(ctx, log_n, x, world, rank), False)
                if not np.array_equal(fwd.evaluation_slice(), sliced_shard_of(X, rank, world)):
                    report["errors"].append(f"forward ntt of new_shard field={field} log_n={log_n}")
            ctx.use_own_stream()
            comm.close()
            ctx.close()
    except Exception as e:   # reported, not raised: the other ranks must not be left waiting in a collective forever
        import traceback

        report["errors"].append("exception: " + repr(e) + "\n" + traceback.format_exc())
    finally:
        with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
            json.dump(report, f)
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_multiprocess_new_shard_prove_and_unshard(tmp_path, world):
    import torch.multiprocessing as mp

    port = _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        rep = json.load(open(os.path.join(str(tmp_path), f"rank{r}.json")))
        assert rep["errors"] == [], f"rank {r}: {rep['errors']}"
        assert rep["cases"] == 2 * ((2 + 1) + (3 + 1) + (2 + 1) + 2 * 2), rep


def test_rccl_world1_unshard():
    """unshard over the RCCL transport (ncclAllGather enqueued on the context's stream) at world 1: the table itself"""
    import numpy as np

    import zk_amd
    from oracle import binding as orc
    from zk_amd import MultiLinearPolynomial as MLE
    from zk_amd.distributed import RcclComm, unshard

    field = zk_amd.BN254_FR
    ctx = zk_amd.Context(field, 0)
    comm = RcclComm(ctx)
    assert (comm.world, comm.rank) == (1, 0)
    for n in (0, 7, 18):
        host = orc.fill_random(field, 60 + n, 1 << n)
        got = unshard(comm, MLE.new_shard(ctx, n, host, 1, 0))
        assert got.n_vars() == n
        assert np.array_equal(got.evaluation_slice(), host), n
    comm.close()
    ctx.close()
