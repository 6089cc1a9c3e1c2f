"""World-2 gloo run of the tiled VAE's fast mode on CPU (kernels served by tests/tilevae_fast_support.py): tile_parallel=True equals the
serial hook on every rank, and fast mode issues ONE collective -- the canvas -- where the non-fast path issues one per GroupNorm more."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_parallel_gloo import _free_port, _tiny_vae


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from supir_amd.utils.tilevae import VAEHook
    from tests import tilevae_fast_support as S
    from tests.helpers import synth_tensor
    calls = []
    inner = dist.all_reduce

    def counted(*a, **k):
        calls.append(1)
        return inner(*a, **k)

    res = {}
    with S.installed(fp32=True), torch.no_grad():
        vae = _tiny_vae()
        for net in (vae.denoise_encoder, vae.decoder):
            net.original_forward = net.forward
        img, z = synth_tensor("img_tiled", (2, 3, 192, 160), scale=0.5), synth_tensor("z_tiled", (2, 4, 40, 32))
        for name, net, size, dec, x, kw in (("enc", vae.denoise_encoder, 64, False, img, dict(fast_encoder=True)),
                                            ("dec", vae.decoder, 8, True, z, dict(fast_decoder=True)),
                                            ("dec_chunk", vae.decoder, 8, True, z, dict(fast_decoder=True, tile_chunk=2)),
                                            ("enc_cf", vae.denoise_encoder, 64, False, img, dict(fast_encoder=True, color_fix=True)),
                                            ("enc_nonfast", vae.denoise_encoder, 64, False, img, {})):
            serial = VAEHook(net, size, is_decoder=dec, **kw)(x)
            del calls[:]
            dist.all_reduce = counted
            try:
                par = VAEHook(net, size, is_decoder=dec, tile_parallel=True, **kw)(x)
            finally:
                dist.all_reduce = inner
            res[name] = (((par - serial).norm() / serial.norm()).item(), len(calls))
    q.put((rank, res))
    dist.barrier()
    dist.destroy_process_group()


def test_fast_mode_tile_parallel_matches_serial_with_one_collective():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=900) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, r in res:
        for name, (err, n) in r.items():
            assert err <= 2e-6, (rank, name, err)           # the bound of tests/test_parallel_gloo.py for the non-fast tiled VAE
        assert r["enc"][1] == r["dec"][1] == r["dec_chunk"][1] == 1, (rank, r)
        # color_fix keeps a pooled all-reduce for every GroupNorm after the first down-sampling, the non-fast path for all of them
        assert 1 < r["enc_cf"][1] < r["enc_nonfast"][1], (rank, r)
