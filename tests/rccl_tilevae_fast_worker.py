"""Worker of tests/test_tilevae_fast_gpu.py::test_fast_mode_tile_parallel_under_a_one_rank_nccl_group (a subprocess: a wedged
collective must not take the test session with it).  One rank, backend "nccl" (= RCCL on ROCm), supir_amd.parallel.FORCE_COLLECTIVES
on: the tiled VAE in fast mode with tile_parallel=True issues its collectives through RCCL on device tensors and must be bitwise
the serial result; every dist.all_reduce is counted.  Prints one JSON line."""
import json
import os
import sys

import torch


def main():
    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from supir_amd import parallel
    from tests import tilevae_fast_support as S
    from tests.helpers import build_vae
    dev = "cuda"
    vae = build_vae(dev)
    runs = {"dec": ("dec_40x32_t8", {}), "enc": ("enc_192x160_t64", {}), "enc_cf": ("enc_cf_192x160_t64", {}),
            "dec_chunk": ("dec_40x32_t8", dict(tile_chunk=2))}

    def run(case, **kw):
        hook, x = S.make_hook(vae, case, dev, **kw)
        with torch.no_grad():
            return hook(x).clone()

    serial = {k: run(case, **kw) for k, (case, kw) in runs.items()}
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 2000))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    parallel.FORCE_COLLECTIVES = True
    res = {"backend": dist.get_backend()}
    calls = []
    inner = dist.all_reduce

    def counted(*a, **k):
        calls.append(1)
        return inner(*a, **k)

    dist.all_reduce = counted
    for k, (case, kw) in runs.items():
        del calls[:]
        out = run(case, tile_parallel=True, **kw)
        res[k + "_equal"], res[k + "_collectives"] = bool(torch.equal(out, serial[k])), len(calls)
    dist.all_reduce = inner
    hook, x = S.make_hook(vae, "enc_cf_192x160_t64", dev)
    with torch.no_grad():
        n_est = len(hook.estimate_group_norm(x.float().contiguous()))
        n_all = len(S.make_hook(vae, "enc_192x160_t64", dev)[0].estimate_group_norm(x.float().contiguous()))
    res["enc_cf_pooled_norms"] = n_all - n_est
    dist.barrier()
    torch.cuda.synchronize()
    dist.destroy_process_group()
    print("RCCL_RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
