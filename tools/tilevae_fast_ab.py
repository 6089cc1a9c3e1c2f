"""A/B of the tiled VAE's fast mode on BASELINE config 3's VAE legs (bf16): 4096^2 encode at tile 512 and 512^2-latent decode at tile
64, non-fast vs fast vs fast with tile_chunk=8 -- interleaved, 5 repetitions each, median of event pairs around the whole hook call,
plus the peak memory of each form.  The non-fast form is the code path the hook has always run (the flags default to off).

    python tools/tilevae_fast_ab.py [--out profiles/tilevae_fast/ab.json] [--small]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/tilevae_fast_ab.py --only fast --leg dec --reps 1     # launch counts per form

Reported, not asserted: the result is written as it comes out."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = {"nonfast": dict(), "fast": dict(fast=True), "fast_chunk8": dict(fast=True, tile_chunk=8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, choices=list(FORMS))
    ap.add_argument("--leg", default=None, choices=["enc", "dec"])
    ap.add_argument("--small", action="store_true", help="2048^2 / 256^2 latent instead of 4096^2 / 512^2")
    a = ap.parse_args()
    from supir_amd import _lib
    from supir_amd.utils.tilevae import VAEHook
    from tests.helpers import build_vae, synth_tensor
    _lib.load()
    dev = "cuda"
    vae = build_vae(dev)
    px, lat = (2048, 256) if a.small else (4096, 512)
    legs = {"enc": (vae.denoise_encoder, 512, False, synth_tensor("ab.img", (1, 3, px, px), scale=0.5).to(dev)),
            "dec": (vae.decoder, 64, True, synth_tensor("ab.z", (1, 4, lat, lat)).to(dev))}
    for net, _, _, _ in legs.values():
        net.original_forward = net.forward
    forms = {k: v for k, v in FORMS.items() if a.only in (None, k)}
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "pixels": px, "latent": lat, "legs": {}}
    for leg, (net, tile, dec, x) in legs.items():
        if a.leg not in (None, leg):
            continue
        hooks = {}
        for name, f in forms.items():
            kw = dict(fast_decoder=bool(f.get("fast")) and dec, fast_encoder=bool(f.get("fast")) and not dec, tile_chunk=f.get("tile_chunk"))
            hooks[name] = VAEHook(net, tile, is_decoder=dec, **kw)
        times, peak = {k: [] for k in hooks}, {}
        with torch.no_grad():
            for name, h in hooks.items():             # warm-up: autotune, workspaces, derived weights
                h(x)
            torch.cuda.synchronize()
            for name, h in hooks.items():
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                h(x)
                torch.cuda.synchronize()
                peak[name] = torch.cuda.max_memory_allocated() / 2 ** 20
            for _ in range(a.reps):
                for name, h in hooks.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    h(x)
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1))
        res["legs"][leg] = {name: dict(median_ms=statistics.median(t), all_ms=t, peak_mib=peak[name]) for name, t in times.items()}
        for name, t in times.items():
            print(f"[tilevae_fast_ab] {leg} {name}: median {statistics.median(t):.1f} ms  (min {min(t):.1f}, max {max(t):.1f})  peak {peak[name]:.0f} MiB",
                  flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print("AB_RESULT " + json.dumps(res))


if __name__ == "__main__":
    main()
