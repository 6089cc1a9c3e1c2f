"""Measurements for soft region weights (supir_xattn_q_d64_regions_soft), written as one JSON file:

(1) the kernel at the two text cross-attention shapes of an untiled 2048^2 step -- (B 2, H 10, T 16384, C 640) and (B 2, H 20, T 4096,
    C 1280), Tk 77 -- with R = 4 and R = 9 regions: the hard form (supir_xattn_q_d64_regions; R = 4: quadrants, R = 9:
    regions_from_tiles(256, 256, 128, 64)), the soft form on the same maps as one-hot weights, and the soft form on Gaussian tile
    weights (region_weights_from_tiles: R = 4 windows of 192 at stride 64, R = 9 windows of 128 at stride 64, so up to four prompts per
    pixel); batch row 0 is the unconditional one, all on entry 0; interleaved with the plain supir_xattn_q_d64.  With --parent-lib PATH
    also the plain and the hard kernel of this build against the parent's library, bitwise and in time (the existing instantiations
    must not have moved);
(2) with --step: sampling steps at a 2048^2 input (latent 256^2) on the full-depth model under graph replay, interleaved -- the untiled
    EDM sampler with 9 prompts on soft Gaussian tile weights, on the hard nearest-centre map, and with a single prompt; ms per step =
    one sampler call of STEPS steps / STEPS, the call a pure replay (an untimed call of the same alternative runs right before it;
    captures inside timed calls are counted and must be 0).

Kernel timings: a captured graph of ITERS launches, replayed; ROUNDS interleaved rounds per alternative; median, min and max.
Usage: python tools/soft_regions_ab.py out.json [--parent-lib PATH] [--step] [--depth 1,2,10]"""
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from supir_amd import _lib, ops
from supir_amd.modules import sampling as S
from supir_amd.modules.attention import level_region_ids, level_region_weights

BF, dev = torch.bfloat16, "cuda"
args = sys.argv[1:]
out_path = args[0] if args and not args[0].startswith("--") else "soft_regions_ab.json"
parent_path = args[args.index("--parent-lib") + 1] if "--parent-lib" in args else None
depth = tuple(int(v) for v in args[args.index("--depth") + 1].split(",")) if "--depth" in args else (1, 2, 10)
ROUNDS, ITERS, STEPS = 9, 20, 4
SHAPES = [(2, 10, 16384, 640), (2, 20, 4096, 1280)]          # (B, H, T, C)


def graph_of(fn, iters=ITERS):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    return g


def ab(fns, iters=ITERS):
    graphs = {k: graph_of(f, iters) for k, f in fns.items()}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) / iters * 1e3)
    return {k: {"us_median": round(statistics.median(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)} for k, v in ts.items()}


def hard_maps():
    """R -> [256, 256] map of region indices on the latent grid."""
    return {4: S.regions_from_tiles(256, 256, 128, 128), 9: S.regions_from_tiles(256, 256, 128, 64)}


def gaussian_weights():
    """R -> [R, 256, 256] Gaussian tile weights on the latent grid."""
    return {4: S.region_weights_from_tiles(256, 256, 192, 64), 9: S.region_weights_from_tiles(256, 256, 128, 64)}


def doubled(w):
    """Region weights [R, h, w] -> [2, 1 + R, h, w]: the unconditional row on entry 0, the conditional row on entries 1 + r."""
    out = torch.zeros((2, 1 + w.shape[0]) + tuple(w.shape[1:]))
    out[0, 0] = 1.0
    out[1, 1:] = w
    return out.to(dev)


res = {"rounds": ROUNDS, "launches_per_replay": ITERS, "device": torch.cuda.get_device_name(0)}
lib = _lib.load()
parent = None
if parent_path:
    parent = ctypes.CDLL(parent_path)
    for name in ("supir_xattn_q_d64", "supir_xattn_q_d64_regions"):
        getattr(parent, name).argtypes = _lib.SIGNATURES[name]
        getattr(parent, name).restype = ctypes.c_int
rows = []
for (B, H, T, C) in SHAPES:
    N, Tk = H * 64, 77
    g = torch.Generator(device="cpu").manual_seed(B + H + T + C)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    x, wq = r(B, T, C).to(BF), (r(N, C) * C ** -0.5).to(BF)
    kb = r(10, Tk, N).to(BF)
    vtb = torch.zeros(10, N, 128, device=dev, dtype=BF)
    vtb[:, :, :Tk] = r(10, N, Tk).to(BF)
    k2, vt2 = kb[:2].contiguous(), vtb[:2].contiguous()
    side = int(T ** 0.5)
    row = {"shape": [B, H, T, Tk, C]}
    new = lambda: torch.empty(B, T, N, device=dev, dtype=BF)  # noqa: E731
    o_plain = new()
    fns = {"plain": lambda: ops.xattn_q(x, wq, None, k2, vt2, B, H, T, Tk, out=o_plain)}
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    ids9 = None
    outs = {}
    for R, m in hard_maps().items():
        lat = torch.stack([torch.zeros_like(m), m + 1]).to(torch.uint8).to(dev)
        ids = level_region_ids(lat, side, side)
        if R == 9:
            ids9 = ids
        one = torch.zeros(2, 1 + R, 256, 256, device=dev).scatter_(1, lat.long()[:, None], 1.0)
        for kind, w in (("onehot", one), ("gauss", doubled(gaussian_weights()[R]))):
            wts, span = level_region_weights(w, side, side)
            outs[kind, R] = new()
            fns[f"soft_{kind}_R{R}"] = (lambda wts=wts, span=span, R=R, kind=kind: ops.xattn_q_regions_soft(
                x, wq, None, kb[:R + 1], vtb[:R + 1], wts, span, B, H, T, Tk, out=outs[kind, R]))
            row[f"soft_{kind}_R{R}_entries_walked_per_block_mean"] = round(float((span[..., 1].float() - span[..., 0].float() + 1).mean()), 3)
        outs["hard", R] = new()
        fns[f"hard_R{R}"] = (lambda ids=ids, R=R: ops.xattn_q_regions(x, wq, None, kb[:R + 1], vtb[:R + 1], ids, B, H, T, Tk, out=outs["hard", R]))
    if parent is not None:
        o_old, o_old_reg = new(), new()

        def old():
            rc = parent.supir_xattn_q_d64(x.data_ptr(), wq.data_ptr(), None, k2.data_ptr(), vt2.data_ptr(), o_old.data_ptr(), B, H, T, Tk, C, C,
                                          N, 128, N, None, 0, 0, None, 1e-5, 0.125, None, stream())
            assert rc == 0, rc

        def old_reg():
            rc = parent.supir_xattn_q_d64_regions(x.data_ptr(), wq.data_ptr(), None, kb.data_ptr(), vtb.data_ptr(), ids9.data_ptr(), 10,
                                                  o_old_reg.data_ptr(), B, H, T, Tk, C, C, N, 128, N, None, 0, 0, None, 1e-5, 0.125, None, stream())
            assert rc == 0, rc
        fns["plain_parent_lib"] = old
        fns["hard_R9_parent_lib"] = old_reg
        fns["plain_again"] = fns["plain"]         # A/A: the spread a difference has to exceed
    row.update(ab(fns))
    torch.cuda.synchronize()
    if parent is not None:
        row["plain_bitwise_equal_to_parent_lib"] = bool(torch.equal(o_plain, o_old))
        row["regions_bitwise_equal_to_parent_lib"] = bool(torch.equal(outs["hard", 9], o_old_reg))
    for R in (4, 9):
        row[f"soft_onehot_R{R}_bitwise_equal_to_hard"] = bool(torch.equal(outs["onehot", R], outs["hard", R]))
        for kind in ("onehot", "gauss"):
            row[f"soft_{kind}_R{R}_over_hard_R{R}"] = round(row[f"soft_{kind}_R{R}"]["us_median"] / row[f"hard_R{R}"]["us_median"], 3)
    rows.append(row)
    print(json.dumps(row), flush=True)
res["kernel"] = rows

if "--step" in args:
    from tests.helpers import build_unet, synth_tensor
    wrap = build_unet(depth=depth, device=dev)
    den = S.DiscreteDenoiserWithControl().to(dev)
    LAT = 256
    T_ = lambda name, shape: synth_tensor(name, shape).to(dev)  # noqa: E731
    lq, xc = T_("rp.lq", (1, 4, LAT, LAT)), T_("rp.xc", (1, 4, LAT, LAT))
    local = [{"crossattn": T_(f"rp.ctx{j}", (1, 77, 2048)), "vector": T_("rp.vec", (1, 2816)), "control": lq} for j in range(9)]
    uc = {"crossattn": T_("rp.uctx", (1, 77, 2048)), "vector": T_("rp.uvec", (1, 2816)), "control": lq}
    m9 = S.regions_from_tiles(LAT, LAT, 128, 64)
    w9 = S.region_weights_from_tiles(LAT, LAT, 128, 64)

    def denoiser(i, s, cc, cs):
        return den(wrap, i, s, cc, cs)
    denoiser.fused = (den, wrap)
    kw = dict(num_steps=STEPS, s_churn=0, s_noise=1.003, restore_cfg=4.0, guider_config=S.LinearCFG(7.5, 4.0), device=dev)
    smp = S.RestoreEDMSampler(**kw)
    x0 = T_("rp.x0", (1, 4, LAT, LAT))
    runs = {"untiled_9_prompts_soft_gaussian_weights": lambda: smp(denoiser, x0.clone(), cond=[dict(c) for c in local], uc=dict(uc), x_center=xc,
                                                                   region_weights=w9),
            "untiled_9_prompts_hard_map": lambda: smp(denoiser, x0.clone(), cond=[dict(c) for c in local], uc=dict(uc), x_center=xc, regions=m9),
            "untiled_single_prompt": lambda: smp(denoiser, x0.clone(), cond=dict(local[0]), uc=dict(uc), x_center=xc)}
    wrap.enable_graph(True)
    ts = {k: [] for k in runs}
    with torch.no_grad():
        for k, f in runs.items():           # warm-up: autotune, captures
            t0 = time.time()
            f()
            torch.cuda.synchronize()
            print(f"warm-up {k}: {time.time() - t0:.1f} s", flush=True)
        captured = 0
        for _ in range(3):
            for k, f in runs.items():
                f()                         # untimed: another alternative ran in between (other embedding-schedule tables), so this
                torch.cuda.synchronize()    # call may re-capture its graphs; the timed call right behind it only replays
                c0 = wrap.graph_stats()["captures"]
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) / STEPS * 1e3)
                captured += wrap.graph_stats()["captures"] - c0
    res["step_captures_inside_timed_calls"] = captured
    step = {k: {"ms_per_step_median": round(statistics.median(v), 2), "ms_min": round(min(v), 2), "ms_max": round(max(v), 2)} for k, v in ts.items()}
    step["soft_over_hard"] = round(step["untiled_9_prompts_soft_gaussian_weights"]["ms_per_step_median"]
                                   / step["untiled_9_prompts_hard_map"]["ms_per_step_median"], 4)
    res["step_2048px_full_depth" if depth == (1, 2, 10) else f"step_2048px_depth_{depth}"] = step
    res["step_graph_stats"] = wrap.graph_stats()
    wrap.enable_graph(False)
    print(json.dumps(step), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
print("wrote", out_path)
