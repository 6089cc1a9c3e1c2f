"""In-process A/B of the fused ZeroSFT launch (ops.zerosft_conv, SUPIR_ZSFT_FUSED) on one CFG-doubled UNet+control step at 1024^2
(latent 128^2, B = 2) under hipGraph replay: the switch alternates 0 / 1, each setting re-captures the graph and is timed `reps` times
(never compare numbers from two calls: box-to-box spread is ~5 %).  Prints per-repetition ms/step, medians, spreads and the distance
between the two outputs, and writes them as JSON when a path is given.
Usage: python tools/zsft_ab.py [reps=6] [out.json] [control_scale=1.0]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from supir_amd import ops
from tests.helpers import build_unet, synth_tensor

dev = "cuda"
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 6
out_path = sys.argv[2] if len(sys.argv) > 2 else None
cscale = float(sys.argv[3]) if len(sys.argv) > 3 else 1.0
wrap = build_unet(device=dev)
B, lat = 2, 128
x = synth_tensor("x", (B, 4, lat, lat)).to(dev)
cond = {"crossattn": synth_tensor("ctx", (B, 77, 2048)).to(dev), "vector": synth_tensor("y", (B, 2816)).to(dev),
        "control": synth_tensor("lq", (B, 4, lat, lat)).to(dev)}
t = torch.full((B,), 500, dtype=torch.int64, device=dev)

res, outs, launches = {0: [], 1: []}, {}, {}
with torch.no_grad():
    for rep in range(reps + 1):             # repetition 0 tunes both settings and is not counted
        for fused in (0, 1):
            ops.USE_ZSFT_FUSED = bool(fused)
            wrap.enable_graph(False)
            if rep == 0:
                for _ in range(2):
                    wrap(x, t, cond, cscale)    # eager: autotune
                tr = ops.start_trace()
                wrap(x, t, cond, cscale)
                ops.stop_trace()
                kinds = {}
                for r in tr:
                    kinds[r["kernel"]] = kinds.get(r["kernel"], 0) + 1
                launches[fused] = dict(sorted(kinds.items()), all=len(tr))
            wrap.enable_graph(True)
            for _ in range(3):
                o = wrap(x, t, cond, cscale)
            torch.cuda.synchronize()
            n = 20
            t0 = time.time()
            for _ in range(n):
                o = wrap(x, t, cond, cscale)
            torch.cuda.synchronize()
            ms = (time.time() - t0) / n * 1e3
            outs[fused] = o.float().clone()
            if rep:
                res[fused].append(round(ms, 3))
            print(f"rep{rep} SUPIR_ZSFT_FUSED={fused}: {ms:.3f} ms/step", flush=True)
    wrap.enable_graph(False)
summary = {"what": "one 1024^2 CFG-doubled step under graph replay, 20 replays per timing, settings alternated in one process",
           "control_scale": cscale, "ms_per_step": {"two_launch": res[0], "fused": res[1]},
           "median": {"two_launch": statistics.median(res[0]), "fused": statistics.median(res[1])},
           "spread": {"two_launch": round(max(res[0]) - min(res[0]), 3), "fused": round(max(res[1]) - min(res[1]), 3)},
           "launches_per_step": {"two_launch": launches[0], "fused": launches[1]},
           "zsft_tiles": {str(k[1:]): v for k, v in ops._TUNE.items() if k[0] == "zsft"},
           "rel_l2_fused_vs_two_launch": ((outs[1] - outs[0]).norm() / outs[0].norm()).item()}
print(json.dumps(summary))
if out_path:
    with open(out_path, "w") as f:
        json.dump(summary, f, indent=1)
