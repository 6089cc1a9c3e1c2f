"""Per-tile prompts with tile batching on two gloo ranks (CPU), `tile_parallel=True`: the tile groups -- each stacking ITS tiles' prompts
-- are dealt round robin, one all-reduce per step assembles the canvas, and both ranks land on what one process computes (as
tests/test_dpmpp_parallel_gloo.py checks for a global prompt)."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_parallel_gloo import _free_port


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from supir_amd.modules import sampling as S
    from tests.helpers import synth_tensor
    from tests.test_host_logic import _prompt_net

    big = (1, 4, 24, 40)
    lqb = synth_tensor("lq_big", big)
    n_tiles = len(S._sliding_windows(24, 40, 16, 8))
    local = [{"crossattn": synth_tensor(f"local.ctx{j}", (1, 77, 2048)), "vector": synth_tensor(f"local.vec{j}", (1, 2816)), "control": lqb}
             for j in range(n_tiles)]
    uc = {"crossattn": synth_tensor("context", (2, 77, 2048))[1:], "vector": synth_tensor("vector", (2, 2816))[1:], "control": lqb}
    den = S.DiscreteDenoiserWithControl()
    xc = synth_tensor("xc_big", big)
    res = []
    for name, tile_batch in (("edm", 3), ("dpmpp", 3), ("dpmpp", 2)):
        batches = []

        def net(xin, tt, cc, cs):
            batches.append(xin.shape[0])
            return _prompt_net(xin, tt, cc, cs)

        def run(parallel, seed, x0):
            kw = dict(tile_size=16, tile_stride=8, device="cpu", guider_config=S.LinearCFG(1.0, 4.0), tile_batch=tile_batch,
                      tile_batch_local_prompts=True, tile_parallel=parallel)
            torch.manual_seed(seed)
            d = lambda i, s, cc, cs: den(net, i, s, cc, cs)  # noqa: E731
            if name == "edm":
                smp = S.TiledRestoreEDMSampler(num_steps=3, s_churn=5, s_noise=1.01, restore_cfg=4.0, **kw)
                return smp(d, x0.clone(), cond=[dict(cj) for cj in local], uc=dict(uc), x_center=xc, control_scale=0.9)
            smp = S.TiledRestoreDPMPP2MSampler(num_steps=4, s_noise=1.003, eta=1.0, **kw)
            return smp(d, x0.clone(), cond=[dict(cj) for cj in local], uc=dict(uc), control_scale=1.0)

        x0 = synth_tensor("noised_big", big)
        serial = run(False, 123, x0)
        del batches[:]
        # rank 1 starts from ANOTHER latent and seed: the broadcasts must pull it onto rank 0's trajectory
        par = run(True, 123 if rank == 0 else 999, x0 if rank == 0 else x0 * 0.5 + 1.0)
        err = ((par - serial).norm() / serial.norm()).item()
        res.append((name, tile_batch, err, bool(torch.isfinite(par).all()), list(batches)))
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_with_batched_local_prompts_match_one_process():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, res in got:
        for name, tile_batch, err, finite, batches in res:
            # the bound of tests/test_dpmpp_parallel_gloo.py: the fp32 summation order of overlapping tiles
            assert finite and err <= 2e-6, (rank, name, tile_batch, err)
            steps = 3 if name == "edm" else 4
            sizes = [2 * min(tile_batch, 8 - j0) for j0 in range(0, 8, tile_batch)]
            assert batches == [b for gi, b in enumerate(sizes) if gi % 2 == rank] * steps, (rank, name, tile_batch, batches)
