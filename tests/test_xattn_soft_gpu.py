"""supir_xattn_q_d64_regions_soft: the fused to_q + text cross-attention with SOFT region weights (csrc/xattn.hip), through the C ABI and ops.

Shapes as in test_xattn_regions_gpu.py: (B 2, H 2, T 256, C 192) -- three K steps, the kernel's minimum, and four 128-row blocks --, a
bank of NR = 4 entries, key counts 77 / 154 / 231 (two, three and four key tiles per entry, so streamed tiles occur), with and without the
LayerNorm fold, on the bf16 library and once on the fp16 one.  `span` comes from attention.region_span, the helper the modules use.

Three yardsticks:
 1. one-hot weights: the output equals (==) ops.xattn_q_regions with the ids the weights encode;
 2. power-of-two weights over a bank that holds ONE prompt in every entry: the mix is exact in fp32, so the output equals (==) the
    unchanged supir_xattn_q_d64 on that prompt (a state not reset between entries, a missed finalisation or a contribution of a
    zero-weight lane all break this);
 3. general weights against float64: sum_e w softmax(q K_e^T / 8) V_e from the same 16-bit operands.  The cap is measured in the test:
    (a) the plain kernel's max-abs error against float64 over all entries, (b) the error of "plain kernel per entry, weighted sum in
    fp32, one cast" (both the parent's code); the soft kernel may take 1.05 x the larger -- a convex mix of per-entry results cannot err
    more than the worst entry before the final rounding.  All three figures go to profiles/soft_regions/kernel_error.json."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from supir_amd import _lib, ops  # noqa: E402
from supir_amd.modules.attention import region_span  # noqa: E402

DEV = "cuda"
B, H, T, C, NR = 2, 2, 256, 192, 4
N = H * 64
RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "soft_regions", "kernel_error.json")


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def record(key, **values):
    """Merge one entry into the JSON record (best effort: a read-only checkout still runs the assertions)."""
    try:
        os.makedirs(os.path.dirname(RECORD), exist_ok=True)
        data = {}
        if os.path.exists(RECORD):
            with open(RECORD) as f:
                data = json.load(f)
        data[key] = values
        with open(RECORD, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


def id_patterns():
    """name -> ids [B, T] (int64, cpu).  A workgroup is 128 consecutive rows of one batch element, a wave 32 of them."""
    t = torch.arange(T)
    out = {}
    for e in range(NR):                                                  # constant per entry
        out[f"a_all_{e}"] = torch.full((B, T), e)
    out["b_block_uniform"] = torch.tensor([0, 3, 2, 1]).repeat_interleave(128).reshape(B, T)     # another entry per 128-row block
    out["c_alternating"] = torch.stack([(t + b) % NR for b in range(B)])                          # changes inside every wave
    d = torch.zeros(B, T, dtype=torch.int64)                             # rows of entry 3 that never use entries 0 .. 2: a late first own
    d[0, 100:] = 3                                                       # tile; the switch at row 100 splits a wave
    d[1, :30] = 3
    out["d_late_first_tile"] = d
    e1 = torch.zeros(B, T, dtype=torch.int64)                            # one entry used by exactly one token
    e1[1, 200] = 2
    out["e_single_token"] = e1
    out["f_middle_unused"] = torch.stack([3 * ((t + b) % 2) for b in range(B)])                    # entries 0 and 3, never 1 or 2
    g = torch.ones(B, T, dtype=torch.int64)                              # the walk starts above entry 0
    g[:, 64:] = 2
    out["g_entry0_unused"] = g
    return out


def one_hot(ids):
    """ids [B, T] -> wts [B, NR, T] float32."""
    return torch.zeros(B, NR, ids.shape[1]).scatter_(1, ids[:, None], 1.0).contiguous()


def pow2_weights():
    """[B, NR, T]: every token has (1/2, 1/2), (1/4, 1/4, 1/2) or (1/4, 1/4, 1/4, 1/4), placed on entries that vary with the token."""
    w = torch.zeros(B, NR, T)
    for b in range(B):
        for t in range(T):
            kind, rot = (t + b) % 3, (t // 3 + b) % NR
            vals = [(0.5, 0.5), (0.25, 0.25, 0.5), (0.25, 0.25, 0.25, 0.25)][kind]
            if kind == 0 and t % 2:
                ent = [rot, (rot + 2) % NR]                               # two entries that are not neighbours: the one between is skipped
            else:
                ent = [(rot + i) % NR for i in range(len(vals))]
            for e, v in zip(ent, vals):
                w[b, e, t] = v
    assert (w.sum(1) == 1).all()
    return w.contiguous()


def general_patterns():
    """name -> wts [B, NR, T] float32 (cpu), >= 0, summing to 1 over the entries within fp32 rounding."""
    g = torch.Generator(device="cpu").manual_seed(77)
    t = torch.arange(T, dtype=torch.float32)

    def dirichlet():
        d = -torch.log(torch.rand(B, NR, T, generator=g).clamp_min(1e-6))
        return d / d.sum(1, keepdim=True)

    out = {"dirichlet": dirichlet()}
    r = torch.zeros(B, NR, T)                                            # a linear ramp between entries 1 and 2 across the token axis
    r[:, 2] = t / (T - 1)
    r[:, 1] = 1.0 - r[:, 2]
    out["ramp_1_2"] = r
    u = torch.rand(B, T, generator=g) * 0.98 + 0.01                      # entries {0, 2} only: every wave skips entry 1
    s = torch.zeros(B, NR, T)
    s[:, 0], s[:, 2] = u, 1.0 - u
    out["entries_0_2"] = s
    tiny = torch.zeros(B, NR, T)                                         # one token with 1e-6 on a third entry
    tiny[:, 0], tiny[:, 1] = 0.5, 0.5
    tiny[1, :, 200] = torch.tensor([0.5, 0.5 - 1e-6, 0.0, 1e-6])
    out["tiny_third_entry"] = tiny
    sb = dirichlet()                                                     # a block whose span is a single entry
    sb[0, :, :128] = 0.0
    sb[0, 3, :128] = 1.0
    out["single_entry_block"] = sb
    z = dirichlet()                                                      # tokens whose weight on the first walked entry is 0
    z[:, 0, 1::2] = 0.0
    out["zero_on_first_entry"] = z / z.sum(1, keepdim=True)
    return {k: v.float().contiguous() for k, v in out.items()}


def operands(Tk, dt, ln, same_prompt=False):
    from supir_amd.weights import compute_dtype, fold_layernorm
    x = (rnd(B, T, C) * 1.5 + 0.3).to(dt)
    kb = rnd(NR, Tk, N, seed=1).to(dt)
    kb[:, 0] *= 3.0
    kb[:, Tk - 1] *= 3.0
    v = rnd(NR, Tk, N, seed=2).to(dt)
    if same_prompt:
        kb = kb[1:2].expand(NR, -1, -1).contiguous()
        v = v[1:2].expand(NR, -1, -1).contiguous()
    vtb = torch.zeros(NR, N, (Tk + 63) // 64 * 64, dtype=dt, device=DEV)
    vtb[:, :, :Tk] = v.permute(0, 2, 1)
    w = rnd(N, C, scale=C ** -0.5, seed=6)
    if not ln:
        wd = w.to(dt)
        return dict(x=x, w=wd, b=None, kb=kb, vtb=vtb, v=v, ln=None, cs=None, q64=x.double() @ wd.double().T)
    wp = rnd(C, C, scale=C ** -0.5, seed=9).to(dt)
    xs, st = ops.gemm_ln(x.view(B * T, C), wp, None, residual=x.view(B * T, C), emit_stats=True)      # statistics as a producer leaves them
    xs = xs.view(B, T, C)
    gamma, beta = rnd(C, seed=4) * 0.2 + 1.0, rnd(C, seed=5) * 0.2
    with compute_dtype(dt):
        wf, cs, bf_ = fold_layernorm(w, None, gamma, beta)
    q64 = torch.nn.functional.layer_norm(xs.double(), (C,), gamma.double(), beta.double(), 1e-5) @ w.to(dt).double().T
    return dict(x=xs, w=wf, b=bf_, kb=kb, vtb=vtb, v=v, ln=st, cs=cs, q64=q64)


def per_entry_f64(q64, kb, v):
    """[NR, B, T, N]: float64 softmax(q k_e^T / 8) v_e of every token against every entry."""
    q = q64.reshape(B, -1, H, 64).permute(0, 2, 1, 3)
    out = []
    for e in range(kb.shape[0]):
        ke = kb[e].double().reshape(-1, H, 64).permute(1, 0, 2)
        ve = v[e].double().reshape(-1, H, 64).permute(1, 0, 2)
        p = torch.softmax(q @ ke.transpose(-1, -2) / 8.0, dim=-1)
        out.append((p @ ve).permute(0, 2, 1, 3).reshape(B, -1, N))
    return torch.stack(out)


def plain_per_entry(op, Tk):
    """[NR, B, T, N]: the unchanged supir_xattn_q_d64, once per entry, that entry's K / V^T given to every batch row."""
    return torch.stack([ops.xattn_q(op["x"], op["w"], op["b"], op["kb"][e:e + 1].expand(B, -1, -1).contiguous(),
                                    op["vtb"][e:e + 1].expand(B, -1, -1).contiguous(), B, H, T, Tk, ln=op["ln"], colsum=op["cs"])
                        for e in range(NR)])


def mix(per_entry, wts, dtype):
    """sum_e wts[b, e, t] per_entry[e, b, t, :] in `dtype`: per_entry [NR, B, T, N], wts [B, NR, T]."""
    return (per_entry.to(dtype) * wts.to(dtype).permute(1, 0, 2)[..., None]).sum(0)


def soft(op, wts, Tk, T_=T, span="derive"):
    wts = wts.to(DEV)
    sp = region_span(wts) if span == "derive" else span
    return ops.xattn_q_regions_soft(op["x"], op["w"], op["b"], op["kb"], op["vtb"], wts, sp, B, H, T_, Tk, ln=op["ln"], colsum=op["cs"])


CONFIGS = [(77, torch.bfloat16, False), (77, torch.bfloat16, True), (154, torch.bfloat16, False), (154, torch.bfloat16, True),
           (231, torch.bfloat16, False), (231, torch.bfloat16, True), (154, torch.float16, True)]
IDS = [f"Tk{c[0]}-{'fp16' if c[1] == torch.float16 else 'bf16'}-{'ln' if c[2] else 'plain'}" for c in CONFIGS]


@pytest.mark.parametrize("Tk,dt,ln", CONFIGS, ids=IDS)
def test_one_hot_weights_equal_the_hard_regional_kernel(Tk, dt, ln):
    op = operands(Tk, dt, ln)
    assert ops.xattn_q_regions_soft_supported(B, T, C, H, Tk, NR)
    for name, ids in id_patterns().items():
        want = ops.xattn_q_regions(op["x"], op["w"], op["b"], op["kb"], op["vtb"], ids.to(torch.uint8).contiguous().to(DEV), B, H, T, Tk,
                                   ln=op["ln"], colsum=op["cs"])
        out = soft(op, one_hot(ids), Tk)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), f"{name}: NaN / Inf"
        bad = (out != want).any(-1)
        assert not bad.any(), f"{name}: {int(bad.sum())} token rows differ from the hard regional kernel, first {bad.nonzero()[:4].tolist()}"


@pytest.mark.parametrize("Tk,dt,ln", CONFIGS, ids=IDS)
def test_power_of_two_mix_of_one_prompt_equals_the_plain_kernel(Tk, dt, ln):
    op = operands(Tk, dt, ln, same_prompt=True)
    want = ops.xattn_q(op["x"], op["w"], op["b"], op["kb"][:1].expand(B, -1, -1).contiguous(), op["vtb"][:1].expand(B, -1, -1).contiguous(),
                       B, H, T, Tk, ln=op["ln"], colsum=op["cs"])
    out = soft(op, pow2_weights(), Tk)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    bad = (out != want).any(-1)
    assert not bad.any(), f"{int(bad.sum())} token rows differ from the plain kernel on the one prompt, first {bad.nonzero()[:4].tolist()}"


def caps(op, Tk, wts, ref64, plain=None):
    """(a) the plain kernel's error over all entries, (b) the error of its per-entry outputs mixed in fp32 and cast once."""
    plain = plain_per_entry(op, Tk) if plain is None else plain
    a = (plain.double() - ref64).abs().max().item()
    comp = mix(plain, wts.to(DEV), torch.float32).to(plain.dtype)
    b = (comp.double() - mix(ref64, wts.to(DEV), torch.float64)).abs().max().item()
    return a, b


@pytest.mark.parametrize("Tk,dt,ln", CONFIGS, ids=IDS)
def test_general_weights_against_float64(Tk, dt, ln):
    op = operands(Tk, dt, ln)
    plain = plain_per_entry(op, Tk)
    ref64 = per_entry_f64(op["q64"], op["kb"], op["v"])
    assert torch.isfinite(plain).all()
    fig = {}
    failed = []
    for name, wts in general_patterns().items():
        a, b = caps(op, Tk, wts, ref64, plain)
        out = soft(op, wts, Tk)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), f"{name}: NaN / Inf"
        err = (out.double() - mix(ref64, wts.to(DEV), torch.float64)).abs().max().item()
        print(f"[xattn soft Tk{Tk} {dt} ln={ln}] {name}: soft {err:.4e}  (a) plain kernel {a:.4e}  (b) composition {b:.4e}")
        fig[name] = dict(a_plain_kernel=a, b_composition=b, soft_kernel=err)
        if not err <= 1.05 * max(a, b):
            failed.append((name, err, a, b))
    key = f"Tk{Tk}_{'fp16' if dt == torch.float16 else 'bf16'}_{'ln' if ln else 'plain'}"
    record(key, shape=dict(B=B, H=H, T=T, C=C, Tk=Tk, NR=NR), max_abs_vs_float64=fig)
    assert not failed, failed


def test_ops_slow_path_on_a_shape_the_kernel_refuses():
    """T = 192 is no multiple of the 128-row block: ops.xattn_q_regions_soft projects, runs the existing attention once per entry and mixes
    in fp32.  Same operands (the first 192 tokens of each batch row), same float64 evaluation, the cap of the kernel test."""
    Tk, dt, T2 = 154, torch.bfloat16, 192
    op = operands(Tk, dt, False)
    wts = general_patterns()["dirichlet"]
    ref64 = per_entry_f64(op["q64"], op["kb"], op["v"])
    a, b = caps(op, Tk, wts, ref64)
    cap = 1.05 * max(a, b)
    assert not ops.xattn_q_regions_soft_supported(B, T2, C, H, Tk, NR)
    op2 = dict(op, x=op["x"][:, :T2].contiguous())
    w2 = wts[:, :, :T2].contiguous()
    out = soft(op2, w2, Tk, T_=T2, span=None)
    ref = mix(ref64[:, :, :T2], w2.to(DEV), torch.float64)
    err = (out.double() - ref).abs().max().item()
    print(f"[xattn soft] ops slow path T=192: max-abs vs float64 {err:.4e}, (a) {a:.4e} (b) {b:.4e} cap {cap:.4e}")
    record("slow_path_T192_Tk154_bf16", max_abs_vs_float64=err, a_plain_kernel=a, b_composition=b, cap=cap)
    assert out.shape == (B, T2, N) and torch.isfinite(out).all()
    assert err <= cap, (err, cap)


def test_refusals_return_status_codes_and_launch_nothing():
    lib = _lib.load()
    Tk = 77
    op = operands(Tk, torch.bfloat16, False)
    wts = general_patterns()["dirichlet"].to(DEV)
    span = region_span(wts)
    o = torch.full((B, T, N), 7.0, dtype=torch.bfloat16, device=DEV)

    def call(T_=T, NR_=NR, wts_=wts.data_ptr(), span_=span.data_ptr(), k_=op["kb"].data_ptr(), vt_=op["vtb"].data_ptr()):
        return lib.supir_xattn_q_d64_regions_soft(op["x"].data_ptr(), op["w"].data_ptr(), None, k_, vt_, wts_, span_, NR_, o.data_ptr(),
                                                  B, H, T_, Tk, C, C, N, op["vtb"].shape[-1], N, None, 0, 0, None, 1e-5, 0.125, None, None)

    assert call(T_=192) == -2          # SUPIR_ERR_SHAPE
    assert call(NR_=0) == -2
    assert call(NR_=256) == -2
    assert call(wts_=None) == -1       # SUPIR_ERR_ARG
    assert call(span_=None) == -1
    assert call(k_=None) == -1
    assert call(vt_=None) == -1
    torch.cuda.synchronize()
    assert (o == 7.0).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(o).all() and not (o == 7.0).all()
