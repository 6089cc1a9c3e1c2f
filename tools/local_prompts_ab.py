"""Per-tile prompts on the tiled samplers, whole images at 4096 x 4096 (49 latent tiles of 128 / 64, tiled VAE) with 49 distinct synthetic
prompts, in one process:
  bank A/B   the per-image bank of text K / V^T + one supir_gather_segments launch per call (wrappers.CONTEXT_BANK) against recomputing
             them before every replay, alternating, --reps each: config 3 geometry (EDM, 50 steps, bf16, tile batch 4) and config 6
             geometry (DPM++ 2M, 8 steps, fp16, tile batch 1 and 4);
  paths      config 3 geometry: the generic loop with one tile per call (what a list `cond` ran before it reached the fused path), the fused
             path at tile batch 1 (the default: tile_batch_local_prompts=False) and at tile batch 4.
Usage: python tools/local_prompts_ab.py [--reps 3] [--edm-steps 50] [--lightning-steps 8] [--res 4096] [--out local_prompts_ab.json]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from supir_amd.configs import supir_v0_config  # noqa: E402
from supir_amd.modules import sampling, wrappers  # noqa: E402
from supir_amd.plugin import instantiate_from_config  # noqa: E402
from supir_amd.synth import synth_param, synth_tensor  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--edm-steps", type=int, default=50)
ap.add_argument("--lightning-steps", type=int, default=8)
ap.add_argument("--res", type=int, default=4096)
ap.add_argument("--skip", default="")            # comma list of: edm, lightning, paths
ap.add_argument("--out", default="local_prompts_ab.json")
args = ap.parse_args()
skip = set(args.skip.split(","))
dev = "cuda"
R = args.res
lat = R // 8
n_tiles = (math.ceil((lat - 128) / 64) + 1) ** 2

cfg = supir_v0_config(sampler="RestoreEDMSampler", sampler_device="cuda")
with torch.device(dev):
    m = instantiate_from_config(cfg)
with torch.no_grad():
    for k, t in m.state_dict().items():
        if t.is_floating_point() and k != "denoiser.sigmas":
            t.copy_(synth_param(k, t.shape, device=dev))
m.model.enable_graph(True)
m.init_tile_vae(encoder_tile_size=512, decoder_tile_size=64)
x = synth_tensor(f"img{R}", (1, 3, R, R), scale=0.5).clamp(-1, 1).to(dev)
local = [{"crossattn": synth_tensor(f"lp.c{j}", (1, 77, 2048)).to(dev), "vector": synth_tensor(f"lp.v{j}", (1, 2816)).to(dev)}
         for j in range(n_tiles)]
uc = {"crossattn": synth_tensor("bench.uc", (1, 77, 2048)).to(dev), "vector": synth_tensor("bench.uv", (1, 2816)).to(dev)}
res = {"device": torch.cuda.get_device_name(0), "resolution": R, "latent_tiles": n_tiles, "prompts": f"{n_tiles} distinct synthetic"}


def save():
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


def image(steps, **kw):
    torch.cuda.synchronize()
    t0 = time.time()
    out = m.batchify_sample(x, num_steps=steps, cond=(local, uc), **kw)
    torch.cuda.synchronize()
    return time.time() - t0, bool(torch.isfinite(out).all())


def bank_ab(steps, kw):
    """bank on / off alternating, args.reps each: seconds per image, medians, the spread of each arm and the verdict of the rule
    'lower median by more than the spread of the runs'."""
    t = {True: [], False: []}
    stats = {}
    for _ in range(args.reps):
        for on in (True, False):
            wrappers.CONTEXT_BANK = on
            m.model.enable_graph(True)           # resets the call counters (graphs of a shape are kept)
            s, ok = image(steps, **kw)
            assert ok
            t[on].append(round(s, 4))
            stats[on] = m.model.graph_stats()
    wrappers.CONTEXT_BANK = True
    med = {on: statistics.median(v) for on, v in t.items()}
    spread = max(max(v) - min(v) for v in t.values())
    return dict(s_per_image_bank=t[True], s_per_image_recompute=t[False], median_bank=med[True], median_recompute=med[False],
                spread_of_runs=round(spread, 4), gain_s=round(med[False] - med[True], 4),
                gain_pct=round(100 * (med[False] - med[True]) / med[False], 2), bank_pays=bool(med[False] - med[True] > spread),
                graph_stats_bank=stats[True], graph_stats_recompute=stats[False])


def params(target, tile_batch, local_batch, **more):
    m.sampler_config["target"] = "sgm.modules.diffusionmodules.sampling." + target
    p = m.sampler_config["params"]
    p.pop("eta", None)
    p.update(tile_size=128, tile_stride=64, tile_batch=tile_batch, tile_batch_local_prompts=local_batch, **more)


kw3 = dict(restoration_scale=-1, s_churn=5, s_noise=1.01, cfg_scale=4.0, seed=1234, color_fix_type="Wavelet", use_linear_CFG=True,
           cfg_scale_start=1.0)
kw6 = dict(restoration_scale=-1, s_churn=0, s_noise=1.003, cfg_scale=4.0, cfg_scale_start=7.5, use_linear_CFG=True, seed=1234,
           color_fix_type="Wavelet")
if "edm" not in skip:
    params("TiledRestoreEDMSampler", 4, True)
    t_first = image(2, **kw3)[0]                 # warm-up: autotune, graph capture
    res[f"config3_geometry_edm_{args.edm_steps}steps_bf16_tile_batch4"] = dict(bank_ab(args.edm_steps, kw3), s_warmup_call_2_steps=round(t_first, 1),
                                                                                peak_mem_GB=round(torch.cuda.max_memory_allocated() / 1e9, 1))
    save()
if "paths" not in skip:
    out = {}
    params("TiledRestoreEDMSampler", 4, False)   # the default: one tile per call, now on the fused step
    image(2, **kw3)
    out["fused_tile_batch1_s_per_image"] = round(image(args.edm_steps, **kw3)[0], 4)
    out["fused_tile_batch1_graph_stats"] = m.model.graph_stats()
    sampling.FUSED_EDM_STEP = False              # the generic torch-op loop, one tile per call: a list `cond` before this change
    image(2, **kw3)
    m.model.enable_graph(True)
    out["generic_loop_one_tile_per_call_s_per_image"] = round(image(args.edm_steps, **kw3)[0], 4)
    out["generic_loop_graph_stats"] = m.model.graph_stats()
    sampling.FUSED_EDM_STEP = True
    res[f"config3_geometry_edm_{args.edm_steps}steps_bf16_paths"] = out
    save()
if "lightning" not in skip:
    m.model.dtype = torch.float16
    for tb in (1, 4):
        params("TiledRestoreDPMPP2MSampler", tb, True, eta=1.0)
        t_first = image(2, **kw6)[0]
        res[f"config6_geometry_dpmpp2m_{args.lightning_steps}steps_fp16_tile_batch{tb}"] = dict(bank_ab(args.lightning_steps, kw6),
                                                                                               s_warmup_call_2_steps=round(t_first, 1))
        save()
    m.model.dtype = torch.bfloat16
