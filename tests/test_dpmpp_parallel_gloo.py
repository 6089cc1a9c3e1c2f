"""Tile-parallel TiledRestoreDPMPP2MSampler on two gloo ranks (CPU): tile groups dealt round robin, x_next and old_next stacked into ONE
all-reduce per step, rank 0's start latent and per-step noise broadcast.  Both ranks must land on what one process computes."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_parallel_gloo import _free_port


def _dpmpp_tile_worker(rank, world, port, q, tile_batch):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from supir_amd.modules import sampling as S
    from tests.helpers import synth_tensor

    def fake_net(xin, tt, cc, cs):
        return torch.tanh(xin * 0.7 + cc["control"] * 0.1) * (1.0 + 0.001 * tt.view(-1, 1, 1, 1).float()) * cs

    big = (1, 4, 24, 40)
    lqb = synth_tensor("lq_big", big)
    ctx, y = synth_tensor("context", (2, 77, 2048)), synth_tensor("vector", (2, 2816))
    c = {"crossattn": ctx[:1], "vector": y[:1], "control": lqb}
    uc = {"crossattn": ctx[1:], "vector": y[1:], "control": lqb}
    den = S.DiscreteDenoiserWithControl()
    counts = {"broadcast": 0, "all_reduce": 0}
    orig = {name: getattr(dist, name) for name in counts}

    def counting(name):
        def fn(t, *a, **k):
            counts[name] += 1
            return orig[name](t, *a, **k)
        return fn

    def run(parallel, seed, x0):
        # the default (Brownian-tree) noise source: each rank's own stream, seeded differently below
        smp = S.TiledRestoreDPMPP2MSampler(tile_size=16, tile_stride=8, num_steps=4, s_noise=1.003, eta=1.0, device="cpu",
                                           guider_config=S.LinearCFG(1.0, 4.0), tile_batch=tile_batch, tile_parallel=parallel)
        torch.manual_seed(seed)
        return smp(lambda i, s, cc, cs: den(fake_net, i, s, cc, cs), x0.clone(), cond=dict(c), uc=dict(uc), control_scale=1.0)

    x0 = synth_tensor("noised_big", big)
    serial = run(False, 123, x0)                                   # what one process computes from rank 0's start latent / seed
    for name in counts:
        setattr(dist, name, counting(name))
    try:
        # rank 1 starts from a DIFFERENT latent and seed: the broadcasts must pull it onto rank 0's trajectory
        par = run(True, 123 if rank == 0 else 999, x0 if rank == 0 else x0 * 0.5 + 1.0)
    finally:
        for name, fn in orig.items():
            setattr(dist, name, fn)
    err = ((par - serial).norm() / serial.norm()).item()
    q.put((rank, err, bool(torch.isfinite(par).all()), dict(counts)))
    dist.barrier()
    dist.destroy_process_group()


def _run(tile_batch):
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dpmpp_tile_worker, args=(r, world, port, q, tile_batch)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return res


def test_tile_parallel_dpmpp_sampler_matches_single_process():
    """tile_batch 1 and 2, on every rank, within the fp32 summation order of overlapping tiles; 4 steps = 1 start-latent broadcast +
    2 noise broadcasts (steps 1 and 2: the first and the last step take no noise) and exactly one all-reduce per step."""
    for tile_batch in (1, 2):
        for rank, err, finite, counts in _run(tile_batch):
            assert finite and err <= 2e-6, (tile_batch, rank, err)
            assert counts == {"broadcast": 3, "all_reduce": 4}, (tile_batch, rank, counts)
