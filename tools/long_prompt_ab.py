"""Measurements for long prompts (supir_xattn_q_d64 over any number of key tiles), written as one JSON file:

(1) with --parent-lib PATH (a libsupir_hip.so built from the parent commit): supir_xattn_q_d64 at 77 tokens, this build against the
    parent's library, interleaved in one process -- the kernel's one- and two-tile path must not have moved;
(2) fused (one launch) against two-launch (to_q GEMM + flash attention) at Tk = 77 / 154 / 231, and the pick ops.choose makes;
(3) with --step: one CFG-doubled network call of the reduced-depth model at latent 128^2 with a 154-token context against a
    77-token one (graph replay).

Each timing is a captured graph of ITERS launches, replayed; ROUNDS interleaved rounds per alternative; median, min and max reported
(the spread of the rounds is the yardstick a difference is read against).
Usage: python tools/long_prompt_ab.py out.json [--parent-lib PATH] [--step]"""
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from supir_amd import _lib, ops

BF, dev = torch.bfloat16, "cuda"
args = sys.argv[1:]
out_path = args[0] if args and not args[0].startswith("--") else "long_prompt_ab.json"
parent_path = args[args.index("--parent-lib") + 1] if "--parent-lib" in args else None
ROUNDS, ITERS = 9, 50
SHAPES = [(2, 20, 1024, 1280), (2, 10, 4096, 640)]          # (B, H, T, C): the two text cross-attention shapes of a 1024^2 step


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


class _Loop:
    """fn called `iters` times per replay(): for callables that replay a graph of their own."""

    def __init__(self, fn, iters):
        self.fn, self.iters = fn, iters

    def replay(self):
        for _ in range(self.iters):
            self.fn()


def ab(fns, iters=ITERS, capture=True):
    graphs = {k: (graph_of(f, iters) if capture else _Loop(f, iters)) for k, f in fns.items()}
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


def operands(B, H, T, Tk, C):
    N = H * 64
    g = torch.Generator(device="cpu").manual_seed(B + H + T + Tk + C)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    x = r(B, T, C).to(BF)
    wq = (r(N, C) * C ** -0.5).to(BF)
    k = r(B, Tk, N).to(BF)
    vt = torch.zeros(B, N, (Tk + 63) // 64 * 64, device=dev, dtype=BF)
    vt[:, :, :Tk] = r(B, N, Tk).to(BF)
    return x, wq, k, vt


def direct(lib, x, wq, k, vt, out, B, H, T, Tk, C):
    N = H * 64

    def call():
        rc = lib.supir_xattn_q_d64(x.data_ptr(), wq.data_ptr(), None, k.data_ptr(), vt.data_ptr(), out.data_ptr(), B, H, T, Tk, C, C, N,
                                   vt.shape[-1], N, None, 0, 0, None, 1e-5, 0.125, None, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    return call


res = {"rounds": ROUNDS, "launches_per_replay": ITERS, "device": torch.cuda.get_device_name(0)}
lib = _lib.load()
if parent_path:
    parent = ctypes.CDLL(parent_path)
    parent.supir_xattn_q_d64.argtypes = _lib.SIGNATURES["supir_xattn_q_d64"]
    parent.supir_xattn_q_d64.restype = ctypes.c_int
    rows = []
    for (B, H, T, C) in SHAPES:
        x, wq, k, vt = operands(B, H, T, 77, C)
        o_new, o_old = torch.empty(B, T, H * 64, device=dev, dtype=BF), torch.empty(B, T, H * 64, device=dev, dtype=BF)
        f_new, f_old = direct(lib, x, wq, k, vt, o_new, B, H, T, 77, C), direct(parent, x, wq, k, vt, o_old, B, H, T, 77, C)
        row = {"shape": [B, H, T, 77, C]}
        # A/A first: the same library twice gives the spread a difference has to exceed
        row.update({("aa_" + n): v for n, v in ab({"this_a": f_new, "this_b": f_new}).items()})
        row.update(ab({"this": f_new, "parent": f_old}))
        torch.cuda.synchronize()
        row["bitwise_equal"] = bool(torch.equal(o_new, o_old))
        rows.append(row)
        print(json.dumps(row), flush=True)
    res["tk77_this_vs_parent"] = rows

rows = []
for (B, H, T, C) in SHAPES:
    for Tk in (77, 154, 231):
        x, wq, k, vt = operands(B, H, T, Tk, C)
        assert ops.xattn_q_supported(B, T, C, H, Tk)
        o1, o2, q = (torch.empty(B, T, H * 64, device=dev, dtype=BF) for _ in range(3))
        ops.gemm(x, wq, out=q)          # autotune the projection's tile outside the capture

        def two():
            ops.flash_attn(ops.gemm(x, wq, out=q), k, vt, B, H, T, Tk, out=o2)

        def fused():
            ops.xattn_q(x, wq, None, k, vt, B, H, T, Tk, out=o1)

        row = {"shape": [B, H, T, Tk, C]}
        row.update(ab({"fused": fused, "two_launch": two}))
        ops._CHOICE.pop(("xattn_ab", B, T, C, H, Tk), None)
        row["choose_picks"] = ["two_launch", "fused"][ops.choose(("xattn_ab", B, T, C, H, Tk), (two, fused), prefer=1)]
        row["rel_l2_fused_vs_two"] = float(((o1.float() - o2.float()).norm() / o2.float().norm()).item())
        rows.append(row)
        print(json.dumps(row), flush=True)
res["fused_vs_two_launch"] = rows

if "--step" in args:
    from tests.helpers import build_unet, synth_tensor
    wrap = build_unet(depth=(1, 1, 2), device=dev)
    B, lat = 2, 128
    x, lq = synth_tensor("xt128", (B, 4, lat, lat)).to(dev), synth_tensor("lq128", (B, 4, lat, lat)).to(dev)
    t = torch.tensor([500, 37], dtype=torch.int64, device=dev)
    conds = {Tk: {"crossattn": synth_tensor(f"ctx{Tk}", (B, Tk, 2048)).to(dev), "vector": synth_tensor("vector", (B, 2816)).to(dev),
                  "control": lq} for Tk in (77, 154)}
    with torch.no_grad():
        for c in conds.values():      # eager first: autotune and ops.choose run outside capture
            wrap(x, t, c, 1.0)
        wrap.enable_graph(True)       # the wrapper's own captured graph per context shape, replayed by each call
        res["network_call_reduced_depth_latent128"] = ab({f"tk{Tk}": (lambda c=c: wrap(x, t, c, 1.0)) for Tk, c in conds.items()}, iters=8,
                                                         capture=False)
        res["network_call_graph_stats"] = wrap.graph_stats()
        wrap.enable_graph(False)
        res["network_call_xattn_picks"] = {str(k_): ["two_launch", "fused"][v] for k_, v in ops._CHOICE.items() if k_[0] == "xattn"}
    print(json.dumps(res["network_call_reduced_depth_latent128"]), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
json.dump(res, open(out_path, "w"), indent=1)
print("wrote", out_path)
