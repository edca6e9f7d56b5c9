"""The RCCL ("nccl" backend) code path of the posterior pooling on one GPU.

The multi-GPU runs (bench.py under torchrun, N = 2..8) pool posterior blocks with
``all_gather_into_tensor`` on device tensors and reduce ``rawstats`` sufficient
statistics with ``all_reduce``; the CPU tests cover the same functions over gloo.  Two
ranks cannot share one GPU under RCCL, so this runs a world-size-1 RCCL group in a child
process: the device engine's sharded MH, the RCCL all-gather and the pooled rawstats
must equal the single-process results exactly.
"""
import os
import socket
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = textwrap.dedent(r"""
    import os, sys
    import numpy as np
    import torch
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(os.environ["ROOT"], "tests"))
    sys.path.insert(0, os.environ["ROOT"])
    from helpers import product_model
    from odelib_amd.distributed import allgather_walkers, pooled_rawstats, sharded_mh
    from odelib_amd.Framework import rawstats
    import pandas as pd

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        assert dist.get_backend() == "nccl"
        m = product_model("two_i", method="rk4")
        eng = m.engine()
        P = len(m.get_pnames())
        W = 333
        theta = np.repeat(np.array([float(m.parameters[p].val) for p in m.get_pnames()])[:, None], W, axis=1)
        theta = theta * np.exp(0.02 * np.random.RandomState(3).standard_normal(theta.shape))
        y0 = np.repeat(np.asarray(m.get_inits(), float)[:, None], W, axis=1)
        th = torch.as_tensor(theta, device=dev)
        yy = torch.as_tensor(y0, device=dev)
        walk = np.ones(P, np.uint8)
        pooled, r = sharded_mh(eng, th, yy, nits=12, burnin=4, walk_mask=walk, seed=5)
        ref = eng.mh_run(th, yy, nits=12, burnin=4, walk_mask=walk, rng="philox", seed=5)
        assert pooled.device.type == "cuda"
        assert torch.equal(pooled, ref["samples"])
        # the all-gather itself, with a ragged walker axis
        blk = torch.arange(W, dtype=torch.float64, device=dev).repeat(2, 1)
        assert torch.equal(allgather_walkers(blk, W), blk)
        # the same pooling through the C-ABI's own RCCL communicator (oe_allgather_samples)
        from odelib_amd.distributed import native_allgather_walkers, native_comm
        comm = native_comm(0)
        got = native_allgather_walkers(ref["samples"], W, comm)
        assert got.device.type == "cuda" and torch.equal(got, ref["samples"])
        assert torch.equal(native_allgather_walkers(blk, W, comm), blk)
        comm.close()
        # pooled rawstats over RCCL == rawstats of the same posterior (Framework.py:11-17)
        med, std = pooled_rawstats(ref["samples"], P)
        s = ref["samples"].cpu().numpy()
        for j in range(P):
            rm, rs = rawstats(pd.Series(s[:, j, :].ravel()))
            np.testing.assert_allclose(med[j], rm, rtol=1e-12)
            np.testing.assert_allclose(std[j], rs, rtol=1e-9)
        print("NCCL OK")
    finally:
        dist.destroy_process_group()
""")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


CABI_CHILD = textwrap.dedent(r"""
    # the ODElib-side binding of INTEGRATION.md §4, without torch.distributed: ctypes
    # only, one rank; the block is an MH posterior [kept][P+5][W] from oe_mh_run
    import ctypes as C, os, sys
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(os.environ["ROOT"], "tests"))
    sys.path.insert(0, os.environ["ROOT"])
    from helpers import product_model
    from odelib_amd import _native as N
    m = product_model("two_i", method="rk4")
    eng = m.engine()
    W = 301
    theta = np.repeat(np.array([float(m.parameters[p].val) for p in m.get_pnames()])[:, None], W, axis=1)
    y0 = np.repeat(np.asarray(m.get_inits(), float)[:, None], W, axis=1)
    r = eng.mh_run(theta, y0, nits=9, burnin=3, walk_mask=np.ones(5, np.uint8), rng="philox", seed=2)
    blk = r["samples"].contiguous()
    rows = blk.numel() // W
    lib = N.load_library()
    uid = (C.c_uint8 * 128)()
    assert lib.oe_comm_unique_id(C.cast(uid, C.c_void_p), 128) == 0
    h = C.c_void_p()
    assert lib.oe_comm_init(0, 1, 0, C.cast(uid, C.c_void_p), 128, C.byref(h)) == 0, lib.oe_comm_last_error(None)
    out = torch.full_like(blk, float("nan"))
    counts = np.array([W], np.int64)
    rc = lib.oe_allgather_samples(h, rows, C.c_void_p(blk.data_ptr()), C.c_void_p(counts.ctypes.data),
                                  C.c_void_p(out.data_ptr()), 0)
    assert rc == 0, lib.oe_comm_last_error(h)
    assert torch.equal(out, blk)
    assert lib.oe_allgather_samples(h, -1, None, C.c_void_p(counts.ctypes.data), None, 0) == N.OE_ERR_ARG
    assert lib.oe_allgather_samples(h, rows, None, C.c_void_p(counts.ctypes.data), C.c_void_p(out.data_ptr()),
                                    N.OE_HOST_PTRS) == N.OE_ERR_ARG
    lib.oe_comm_destroy(h)
    print("CABI OK")
""")


@pytest.mark.gpu
def test_rccl_world1_allgather_through_the_c_abi():
    """oe_comm_unique_id / oe_comm_init / oe_allgather_samples bound with ctypes alone (no
    torch.distributed): a world-size-1 RCCL communicator pools the MH posterior block."""
    env = dict(os.environ, ROOT=ROOT)
    r = subprocess.run([sys.executable, "-c", CABI_CHILD], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=100)
    assert r.returncode == 0 and "CABI OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


@pytest.mark.gpu
def test_rccl_world1_pooling_equals_single_process():
    env = dict(os.environ, ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=100)
    assert r.returncode == 0 and "NCCL OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


GLOO2_CHILD = textwrap.dedent(r"""
    # one of two gloo ranks sharing GPU 0: the DEVICE engine runs this rank's shard
    # (Philox keyed by the global walker id), the posterior is pooled over gloo
    import os, sys
    import numpy as np
    import torch
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(os.environ["ROOT"], "tests"))
    sys.path.insert(0, os.environ["ROOT"])
    from helpers import product_model
    from odelib_amd.distributed import pooled_rawstats, shard, sharded_mh
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # every MH chain is integrated on its own (RK4; DOPRI5 and BDF with their own step
        # sizes per chain), so the shards reproduce one launch whatever their boundaries
        method = os.environ["OE_METHOD"]
        m = product_model("two_i", method=method)
        eng = m.engine()
        W = 301  # ragged: 151 + 150 walkers
        theta = np.repeat(np.array([float(m.parameters[p].val) for p in m.get_pnames()])[:, None], W, axis=1)
        theta = theta * np.exp(0.02 * np.random.RandomState(3).standard_normal(theta.shape))
        if method == "auto":  # stiff chains in both shards: handed to BDF at their own times
            for w, tau in ((7, 1e5), (150, 1e4), (151, 3e4), (300, 1e5)):
                theta[4, w] = tau
            theta[1, [20, 200]] = 1.5e-5
        y0 = np.repeat(np.asarray(m.get_inits(), float)[:, None], W, axis=1)
        walk = np.ones(5, np.uint8)
        pooled, mine = sharded_mh(eng, theta, y0, nits=10, burnin=3, walk_mask=walk, seed=8)
        off, cnt = shard(W, rank, world)
        med, sd = pooled_rawstats(mine["samples"].cpu(), 5)
        if rank == 0:
            ref = eng.mh_run(theta, y0, nits=10, burnin=3, walk_mask=walk, rng="philox", seed=8)
            assert torch.equal(pooled.cpu(), ref["samples"].cpu()), "pooled shards differ from one launch"
            if method == "auto":
                assert (ref["status"].cpu().numpy() & 8).any(), "no chain was handed to BDF"
            import pandas as pd
            from odelib_amd.Framework import rawstats
            s = ref["samples"].cpu().numpy()
            for j in range(5):  # rawstats of the whole posterior (Framework.py:11-17), one process
                rm, rs = rawstats(pd.Series(s[:, j, :].ravel()))
                np.testing.assert_allclose(med[j], rm, rtol=1e-12)
                np.testing.assert_allclose(sd[j], rs, rtol=1e-9)
            print("GLOO2 OK")
    finally:
        dist.destroy_process_group()
""")


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["rk4", "auto"])
def test_two_gloo_ranks_device_engine_pool_equals_one_launch(method):
    """World size 2 with the DEVICE engine (verdict r2: the CPU world-2 test drives the C
    restatement): two ranks on one GPU (gloo; RCCL refuses two ranks per device), each
    running its shard through oe_mh_run (in speculative rounds: sharded_mh's default, 151
    chains leave the device idle), pooled by the all-gather and the rawstats all-reduces —
    equal to one sequential 301-walker launch bit for bit.  'auto' (the drop-in default)
    with stiff chains in both shards: the chains handed to BDF are bitwise too."""
    port = str(_free_port())
    procs = []
    for r in range(2):
        env = dict(os.environ, ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(r), WORLD_SIZE="2",
                   LOCAL_RANK=str(r), OE_METHOD=method)
        procs.append(subprocess.Popen([sys.executable, "-c", GLOO2_CHILD], cwd=ROOT, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=150) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-2000:] for o in outs]
    assert "GLOO2 OK" in outs[0][0]


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("n", [2, 8])
def test_bench_multi_rank_rehearsal(n):
    """bench.py's multi-rank path as the driver launches it (torchrun child launch from
    --gpus N), rehearsed on one GPU over gloo for N = 2 and for the driver's N = 8
    (Framework.py:779-780's chain pool, :1037's concat): the line reports N GPUs, the
    headline counts every rank's walkers, and the C4 leg shards 1 048 576 walkers into N
    contiguous shards (131 072 per rank at N = 8) and pools the 4.11 GB posterior."""
    import json
    env = dict(os.environ, ODELIB_BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "3", "--warmup", "1",
                        "--full", "--warmup-ms", "5", "--no-extra-configs", "--no-pmc", "--mcmc-iters", "5", "--c4-steps", "2"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=840)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == n and line["config"]["walkers_total"] == n * 65536
    c4 = line["other_configs"]["C4"]
    assert c4["walkers_total"] == 1 << 20 and c4["walkers_per_gpu"] == (1 << 20) // n and c4["n_gpus"] == n
    assert c4["allgather"]["bytes_gathered"] == 49 * 10 * (1 << 20) * 8
    assert c4["allgather"]["world_size"] == n
    assert c4["integrate"]["chi_finite"]


@pytest.mark.gpu
@pytest.mark.parametrize("counts", [[5, 3], [4, 4, 1], [7, 0, 7, 6, 7, 7, 2, 7], [131072, 131071]])
def test_pool_pad_and_relayout_n_ranks_on_one_gpu(counts):
    """The data movement oe_allgather_samples does around the RCCL collective for n > 1 ranks
    (comm.hip: pad each rank's [rows][count] block to [rows][cmax]; lay the rank-major
    [n][rows][cmax] result out as [rows][sum(counts)] in global walker order), driven through
    the C-ABI on one GPU with a synthetic gathered buffer — the path an 8-GPU pooling takes,
    checked against a numpy re-layout for n = 2, 3, 8, ragged counts (one rank empty) and the
    C4 shard size."""
    import numpy as np
    import torch
    from odelib_amd import _native as N
    dev = torch.device("cuda", 0)
    n, rows = len(counts), 7
    cmax = max(counts)
    rs = np.random.RandomState(len(counts))
    blocks = [rs.standard_normal((rows, c)) for c in counts]
    # each rank pads its block (oe_pool_pad) into its slot of the rank-major buffer, as the
    # collective would deliver it
    gathered = torch.full((n, rows, cmax), np.nan, dtype=torch.float64, device=dev)
    for r, b in enumerate(blocks):
        tb = torch.as_tensor(b, device=dev).contiguous()
        N.pool_pad(rows, tb.data_ptr() if b.size else None, counts[r], cmax, gathered[r].data_ptr())
    g = gathered.cpu().numpy()
    for r, b in enumerate(blocks):
        assert np.array_equal(g[r, :, :counts[r]], b) and not g[r, :, counts[r]:].any()
    out = torch.full((rows, sum(counts)), np.nan, dtype=torch.float64, device=dev)
    N.pool_relayout(counts, rows, gathered.data_ptr(), out.data_ptr())
    want = np.concatenate(blocks, axis=1)
    assert np.array_equal(out.cpu().numpy(), want)
