"""Measurements for regional prompts (supir_xattn_q_d64_regions), written as one JSON file:

(1) the kernel at the two text cross-attention shapes of an untiled 2048^2 step -- (B 2, H 10, T 16384, C 640) and (B 2, H 20, T 4096,
    C 1280), Tk 77 -- with R = 1 / 4 / 9 regions (R = 4: quadrants; R = 9: regions_from_tiles(256, 256, 128, 64); batch row 0 is the
    unconditional one, all on entry 0) against the plain supir_xattn_q_d64 on the same shape, interleaved; with --parent-lib PATH also
    the plain kernel of this build against the parent's library (the existing instantiation must not have moved);
(2) with --step: sampling steps at a 2048^2 input (latent 256^2) on the full-depth model under graph replay, interleaved -- the untiled
    EDM sampler with 9 regional prompts, the untiled sampler with a single prompt, and TiledRestoreEDMSampler (tile 128, stride 64,
    tile_batch 4) with 9 per-tile prompts, all three on THIS build (not the parent commit); ms per step = one sampler call of STEPS steps / STEPS, the call a pure replay
    (an untimed call of the same alternative runs right before it; captures inside timed calls are counted and must be 0).

Kernel timings: a captured graph of ITERS launches, replayed; ROUNDS interleaved rounds per alternative; median, min and max.
Usage: python tools/regional_prompts_ab.py out.json [--parent-lib PATH] [--step] [--depth 1,2,10]"""
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

BF, dev = torch.bfloat16, "cuda"
args = sys.argv[1:]
out_path = args[0] if args and not args[0].startswith("--") else "regional_prompts_ab.json"
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


def region_maps():
    """R -> [256, 256] map of region indices on the latent grid."""
    return {1: torch.zeros(256, 256, dtype=torch.int64), 4: S.regions_from_tiles(256, 256, 128, 128), 9: S.regions_from_tiles(256, 256, 128, 64)}


res = {"rounds": ROUNDS, "launches_per_replay": ITERS, "device": torch.cuda.get_device_name(0)}
lib = _lib.load()
parent = None
if parent_path:
    parent = ctypes.CDLL(parent_path)
    parent.supir_xattn_q_d64.argtypes = _lib.SIGNATURES["supir_xattn_q_d64"]
    parent.supir_xattn_q_d64.restype = ctypes.c_int
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
    o_plain = torch.empty(B, T, N, device=dev, dtype=BF)
    fns = {"plain": lambda: ops.xattn_q(x, wq, None, k2, vt2, B, H, T, Tk, out=o_plain)}
    if parent is not None:
        o_old = torch.empty(B, T, N, device=dev, dtype=BF)

        def old():
            rc = parent.supir_xattn_q_d64(x.data_ptr(), wq.data_ptr(), None, k2.data_ptr(), vt2.data_ptr(), o_old.data_ptr(), B, H, T, Tk, C, C,
                                          N, 128, N, None, 0, 0, None, 1e-5, 0.125, None, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc
        fns["plain_parent_lib"] = old
        fns["plain_again"] = fns["plain"]         # A/A: the spread a difference has to exceed
    outs = {}
    for R, m in region_maps().items():
        from supir_amd.modules.attention import level_region_ids
        lat = torch.stack([torch.zeros_like(m), m + 1]).to(torch.uint8).to(dev)
        ids = level_region_ids(lat, side, side)
        outs[R] = torch.empty(B, T, N, device=dev, dtype=BF)
        fns[f"regions_R{R}"] = (lambda ids=ids, R=R: ops.xattn_q_regions(x, wq, None, kb[:R + 1], vtb[:R + 1], ids, B, H, T, Tk, out=outs[R]))
    row.update(ab(fns))
    torch.cuda.synchronize()
    if parent is not None:
        row["plain_bitwise_equal_to_parent_lib"] = bool(torch.equal(o_plain, o_old))
    row["R1_bitwise_equal_to_plain"] = bool(torch.equal(outs[1], o_plain))
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

    def denoiser(i, s, cc, cs):
        return den(wrap, i, s, cc, cs)
    denoiser.fused = (den, wrap)
    kw = dict(num_steps=STEPS, s_churn=0, s_noise=1.003, restore_cfg=4.0, guider_config=S.LinearCFG(7.5, 4.0), device=dev)
    plain_smp = S.RestoreEDMSampler(**kw)
    tiled_smp = S.TiledRestoreEDMSampler(128, 64, tile_batch=4, tile_batch_local_prompts=True, **kw)
    x0 = T_("rp.x0", (1, 4, LAT, LAT))
    runs = {"untiled_9_regional_prompts": lambda: plain_smp(denoiser, x0.clone(), cond=[dict(c) for c in local], uc=dict(uc), x_center=xc, regions=m9),
            "untiled_single_prompt": lambda: plain_smp(denoiser, x0.clone(), cond=dict(local[0]), uc=dict(uc), x_center=xc),
            "tiled_tile_batch4_9_local_prompts": lambda: tiled_smp(denoiser, x0.clone(), cond=[dict(c) for c in local], uc=dict(uc), x_center=xc)}
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
    res["step_2048px_full_depth" if depth == (1, 2, 10) else f"step_2048px_depth_{depth}"] = {
        k: {"ms_per_step_median": round(statistics.median(v), 2), "ms_min": round(min(v), 2), "ms_max": round(max(v), 2)} for k, v in ts.items()}
    res["step_graph_stats"] = wrap.graph_stats()
    wrap.enable_graph(False)
    print(json.dumps(res[[k for k in res if k.startswith("step_2048px")][0]]), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
print("wrote", out_path)
