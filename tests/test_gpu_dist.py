"""GPU, world_size 2 on ONE device (gloo moves device tensors; RCCL refuses two ranks on one GPU): the member-sharded
ensemble's real exchange step -- values_amd.dist.ensemble_uncertainty_sharded's sum-reduce of sufficient statistics --
and the map gather, with the HIP kernels on both ranks.  On a node with at least two GPUs the same exchange runs on the
`nccl` backend (= RCCL over xGMI), one rank per device (skipped on the 1-GPU boxes of the build pool)."""
import os

import numpy as np
import pytest
import torch

from tests.test_dist_cpu import _run_world2

pytestmark = pytest.mark.gpu


def _worker_sharded(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        from tests.test_gpu_unet3d import KEYS, make_model
        from values_amd import predict_uncertainty
        from values_amd.dist import ensemble_uncertainty_sharded, gather_maps, shard_range
        from tests.formula import formula_volume
        models = [make_model(seed_tag=s, do_dropout=False) for s in range(3)]
        x = torch.from_numpy(np.concatenate([formula_volume((1, 1, 16, 16, 16), tag=70 + i) for i in range(3)], 0)).float().cuda()
        sh = ensemble_uncertainty_sharded(models, x, world=world, rank=rank, n_pred=1)
        ok = True
        if rank == 0:
            one = predict_uncertainty(models, x, n_pred=1)
            ok = all((sh[k] - one[k]).abs().max().item() < 2e-6 for k in KEYS + ("mean_softmax",))
            ok = ok and torch.equal(sh["pred_seg_mean"], one["pred_seg_mean"])
        else:
            ok = sh is None
        # volume-sharded MC-dropout + gather: rank r runs its shard, rank 0 ends up with every volume's maps
        drop = make_model(do_dropout=True)
        lo, hi = shard_range(3, world, rank)
        mine = predict_uncertainty([drop], x[lo:hi], n_pred=4, seeds=[11 + rank])
        allm = gather_maps(mine, world, rank)
        if rank == 0:
            for r in range(world):
                l2, h2 = shard_range(3, world, r)
                ref = predict_uncertainty([drop], x[l2:h2], n_pred=4, seeds=[11 + r])
                ok = ok and all(torch.equal(allm[k][l2:h2], ref[k]) for k in KEYS + ("softmax_variance", "mean_softmax", "pred_seg_mean"))
        else:
            ok = ok and allm is None
        torch.cuda.synchronize()
        q.put(bool(ok))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_member_sharded_ensemble_reduce_and_map_gather_world2():
    assert all(_run_world2(_worker_sharded))


def _worker_nccl(rank, world, port, q):
    """one rank per GPU, backend nccl (RCCL): member-sharded ensemble (sum-reduce) + the overlapped map gather of
    bench.py --gpus N against the single-GPU results computed on rank 0"""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(rank)
    dev = torch.device("cuda", rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    try:
        from tests.test_gpu_unet3d import KEYS, make_model
        from values_amd import predict_uncertainty
        from values_amd.dist import MapGatherPipeline, ensemble_uncertainty_sharded, shard_range
        from tests.formula import formula_volume
        assert dist.get_world_size() == world and str(dist.get_backend()).lower() == "nccl"
        models = [make_model(seed_tag=s, do_dropout=False) for s in range(3)]
        x = torch.from_numpy(np.concatenate([formula_volume((1, 1, 16, 16, 16), tag=70 + i) for i in range(4)], 0)).float().to(dev)
        sh = ensemble_uncertainty_sharded(models, x, world=world, rank=rank, n_pred=1)
        ok = True
        if rank == 0:
            one = predict_uncertainty(models, x, n_pred=1)
            ok = all((sh[k] - one[k]).abs().max().item() < 2e-6 for k in KEYS + ("mean_softmax",))
            ok = ok and torch.equal(sh["pred_seg_mean"], one["pred_seg_mean"])
        else:
            ok = sh is None
        # volume shards + MapGatherPipeline (async gathers, buffer reuse, flush): bit for bit the single-GPU maps
        drop = make_model(do_dropout=True)
        lo, hi = shard_range(4, world, rank)
        pipe = MapGatherPipeline(world, rank, depth=2)
        got = []
        for step in range(5):
            r = pipe.submit(predict_uncertainty([drop], x[lo:hi], n_pred=4, seeds=[100 * step + rank]))
            if r is not None:
                got.append({k: v.clone() for k, v in r.items()})
        got += [{k: v.clone() for k, v in r.items()} for r in pipe.flush() if r is not None]
        if rank == 0:
            ok = ok and len(got) == 5
            for step, res in enumerate(got):
                for r in range(world):
                    l2, h2 = shard_range(4, world, r)
                    ref = predict_uncertainty([drop], x[l2:h2], n_pred=4, seeds=[100 * step + r])
                    ok = ok and all(torch.equal(res[k][l2:h2], ref[k])
                                    for k in KEYS + ("softmax_variance", "mean_softmax", "pred_seg_mean"))
        else:
            ok = ok and len(got) == 0
        torch.cuda.synchronize()
        q.put(bool(ok))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_nccl_backend_two_gpus_sharded_ensemble_and_gather_pipeline():
    """SURVEY section 4, pyramid level 4: the RCCL paths themselves (dist.reduce / async dist.gather on `nccl`)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs on one node (the build pool's boxes have one); covered under gloo above")
    assert all(_run_world2(_worker_nccl))


@pytest.mark.parametrize("extra,world,units,workload", [(["--volumes", "4"], 2, 8.0, "C2"), (["--volumes", "2"], 4, 8.0, "C2"),
                                                        (["--config", "C3", "--volumes", "2"], 2, 4.0, "C3"),
                                                        (["--config", "C5", "--volumes", "1"], 2, 2.0, "C5"),
                                                        (["--config", "C4", "--volumes", "1"], 2, 2.0, "C4")])
def test_bench_ranks_emulated_on_one_gpu(extra, world, units, workload):
    """The whole `bench.py --gpus N` path, end to end, on a 1-GPU box (VX_BENCH_EMULATE_RANKS=1: both ranks on the visible GPU, gloo
    instead of RCCL): the parent that never touches a GPU runtime spawns torch.distributed.run, the ranks shard the volumes, every
    step's maps are gathered on rank 0 INSIDE the timed region (MapGatherPipeline), region times are the max over ranks, rank 0
    prints one JSON line with the contract's fields.  The round-5 verdict's gap is a run over xGMI, which no box of the pool can
    give; this is what CAN be checked before the driver's 8-GPU run: that nothing on that path fails to start, deadlocks or
    miscounts -- for C2 at two and four ranks, the member-sharded C3 (one RCCL-style sum-reduce), the sliding-window C5 and the 2D C4.  The line
    says "emulated": its value is not a measurement."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VX_BENCH_EMULATE_RANKS="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", str(world), "--full"] + extra + ["--steps", "2", "--warmup", "1", "--repeats", "1",
           "--min-gpu-seconds", "0", "--no-cpu-baseline", "--no-roofline", "--no-latency", "--no-batch64", "--no-storage16"]
    p = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == world and d["ranks_joined"] == world and d["emulated"] is True
    assert d["scaling"] == "weak" and d["higher_is_better"] is True and d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and d["unit"] in ("volumes/s", "images/s") and d["config"]["workload"].startswith(workload)
    # value = the units of ALL ranks per max-over-ranks time (C2: volumes per GPU x ranks; the other configs likewise)
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - units) < 0.05 * units, (d["value"], d["ms_per_step"], units)
    if workload == "C2":
        assert "no_gather" in json.dumps(d)       # the side number that leaves the maps on their ranks
