"""supir_xattn_q_d64_regions: the fused to_q + text cross-attention with a prompt per region (csrc/xattn.hip), through the C ABI and ops.

Shapes (B 2, H 2, T 256, C 192): three K steps -- the kernel's minimum --, four workgroup row blocks of 128 tokens, key counts 77 / 154 /
231 (two, three and four key tiles per entry: the third and every later tile of the walk is a streamed one), a bank of NR = 3 entries,
with and without the LayerNorm fold, on the bf16 library and once on the fp16 one.

The yardstick is exact: a token's output row must equal, bit for bit, the row the UNCHANGED supir_xattn_q_d64 produces when it is given
that token's entry as its K / V^T.  Next to it a float64 evaluation of the per-token masked softmax, whose cap is not fixed in advance:
the existing kernel's own error against float64 is measured on the same operands in the same test and the regional kernel may take
1.05 x that (the bitwise check says equal; both figures go to profiles/regional_prompts/kernel_error.json)."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from supir_amd import _lib, ops  # noqa: E402

DEV = "cuda"
B, H, T, C, NR = 2, 2, 256, 192, 3
N = H * 64
RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "regional_prompts", "kernel_error.json")


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


def patterns():
    """name -> ids [B, T] (uint8).  A workgroup is 128 consecutive rows of one batch element, a wave 32 of them."""
    t = torch.arange(T)
    out = {}
    for e in range(NR):                                                  # (a) every token on one entry
        out[f"a_all_{e}"] = torch.full((B, T), e)
    out["b_block_uniform"] = torch.tensor([0, 1, 2, 1]).repeat_interleave(128).reshape(B, T)     # (b) another entry per 128-row block
    out["c_alternating"] = torch.stack([(t + b) % NR for b in range(B)])                          # (c) changes inside every wave
    d = torch.zeros(B, T, dtype=torch.int64)                             # (d) rows of entry 2 that never use entry 0 or 1: their first own
    d[0, 100:] = 2                                                       #     tile comes after masked ones (running max still -inf); the
    d[1, :30] = 2                                                        #     switch at row 100 splits a wave
    out["d_late_first_tile"] = d
    e1 = torch.zeros(B, T, dtype=torch.int64)                            # (e) one entry used by exactly one token
    e1[1, 200] = 2
    out["e_single_token"] = e1
    out["f_middle_unused"] = torch.stack([2 * ((t + b) % 2) for b in range(B)])                    # (f) entries 0 and 2, never 1
    g = torch.ones(B, T, dtype=torch.int64)                              # the walk starts above entry 0 (e_lo = 1)
    g[:, 64:] = 2
    out["g_entry0_unused"] = g
    return {k: v.to(torch.uint8).contiguous().to(DEV) for k, v in out.items()}


def operands(Tk, dt, ln):
    from supir_amd.weights import compute_dtype, fold_layernorm
    x = (rnd(B, T, C) * 1.5 + 0.3).to(dt)
    kb = rnd(NR, Tk, N, seed=1).to(dt)
    kb[:, 0] *= 3.0
    kb[:, Tk - 1] *= 3.0
    v = rnd(NR, Tk, N, seed=2).to(dt)
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
    q = q64.reshape(B, T, H, 64).permute(0, 2, 1, 3)
    out = []
    for e in range(kb.shape[0]):
        ke = kb[e].double().reshape(-1, H, 64).permute(1, 0, 2)
        ve = v[e].double().reshape(-1, H, 64).permute(1, 0, 2)
        p = torch.softmax(q @ ke.transpose(-1, -2) / 8.0, dim=-1)
        out.append((p @ ve).permute(0, 2, 1, 3).reshape(B, T, N))
    return torch.stack(out)


def select(per_entry, ids):
    """per_entry [NR, B, T, N], ids [B, T] -> [B, T, N]: every token's row of its own entry."""
    return torch.gather(per_entry, 0, ids.long()[None, :, :, None].expand(1, B, ids.shape[1], N))[0]


@pytest.fixture(scope="module")
def plain_error():
    return {}


CONFIGS = [(77, torch.bfloat16, False), (77, torch.bfloat16, True), (154, torch.bfloat16, False), (154, torch.bfloat16, True),
           (231, torch.bfloat16, False), (231, torch.bfloat16, True), (154, torch.float16, True)]


@pytest.mark.parametrize("Tk,dt,ln", CONFIGS, ids=[f"Tk{c[0]}-{'fp16' if c[1] == torch.float16 else 'bf16'}-{'ln' if c[2] else 'plain'}" for c in CONFIGS])
def test_regions_kernel_is_bitwise_the_plain_kernel_on_each_tokens_entry(Tk, dt, ln, plain_error):
    op = operands(Tk, dt, ln)
    assert ops.xattn_q_regions_supported(B, T, C, H, Tk, NR)
    # the yardstick: the existing kernel, once per entry, that entry's K / V^T given to every batch row
    plain = torch.stack([ops.xattn_q(op["x"], op["w"], op["b"], op["kb"][e:e + 1].expand(B, -1, -1).contiguous(),
                                     op["vtb"][e:e + 1].expand(B, -1, -1).contiguous(), B, H, T, Tk, ln=op["ln"], colsum=op["cs"])
                         for e in range(NR)])
    ref64 = per_entry_f64(op["q64"], op["kb"], op["v"])
    assert torch.isfinite(plain).all()
    err_plain = (plain.double() - ref64).abs().max().item()
    worst = 0.0
    for name, ids in patterns().items():
        out = ops.xattn_q_regions(op["x"], op["w"], op["b"], op["kb"], op["vtb"], ids, B, H, T, Tk, ln=op["ln"], colsum=op["cs"])
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), f"{name}: NaN / Inf"
        want = select(plain, ids)
        bad = (out != want).any(-1)
        assert not bad.any(), f"{name}: {int(bad.sum())} token rows differ from the plain kernel on their entry, first {bad.nonzero()[:4].tolist()}"
        err = (out.double() - select(ref64, ids)).abs().max().item()
        worst = max(worst, err)
        print(f"[xattn regions Tk{Tk} {dt} ln={ln}] {name}: max-abs vs float64 {err:.4e} (plain kernel {err_plain:.4e})")
        assert err <= 1.05 * err_plain, (name, err, err_plain)
    key = f"Tk{Tk}_{'fp16' if dt == torch.float16 else 'bf16'}_{'ln' if ln else 'plain'}"
    plain_error[key] = err_plain
    record(key, shape=dict(B=B, H=H, T=T, C=C, Tk=Tk, NR=NR), max_abs_vs_float64_plain_kernel=err_plain,
           max_abs_vs_float64_regions_kernel_worst_pattern=worst)


def test_ops_slow_path_on_a_shape_the_kernel_refuses(plain_error):
    """T = 192 is no multiple of the 128-row block: ops.xattn_q_regions projects, runs the existing attention once per entry and selects.
    Same operands (the first 192 tokens of each batch row), same float64 evaluation, the cap of the kernel test."""
    Tk, dt = 154, torch.bfloat16
    op = operands(Tk, dt, False)
    if "Tk154_bf16_plain" not in plain_error:        # run alone: measure the existing kernel here
        plain = torch.stack([ops.xattn_q(op["x"], op["w"], None, op["kb"][e:e + 1].expand(B, -1, -1).contiguous(),
                                         op["vtb"][e:e + 1].expand(B, -1, -1).contiguous(), B, H, T, Tk) for e in range(NR)])
        plain_error["Tk154_bf16_plain"] = (plain.double() - per_entry_f64(op["q64"], op["kb"], op["v"])).abs().max().item()
    cap = 1.05 * plain_error["Tk154_bf16_plain"]
    T2 = 192
    assert not ops.xattn_q_regions_supported(B, T2, C, H, Tk, NR)
    x2 = op["x"][:, :T2].contiguous()
    ids = patterns()["c_alternating"][:, :T2].contiguous()
    out = ops.xattn_q_regions(x2, op["w"], None, op["kb"], op["vtb"], ids, B, H, T2, Tk)
    ref = select(per_entry_f64(op["q64"], op["kb"], op["v"])[:, :, :T2], ids)
    err = (out.double() - ref).abs().max().item()
    print(f"[xattn regions] ops slow path T=192: max-abs vs float64 {err:.4e}, cap {cap:.4e}")
    record("slow_path_T192_Tk154_bf16", max_abs_vs_float64=err, cap=cap)
    assert out.shape == (B, T2, N) and torch.isfinite(out).all()
    assert err <= cap, (err, cap)


def test_refusals_return_status_codes_and_launch_nothing():
    lib = _lib.load()
    Tk = 77
    op = operands(Tk, torch.bfloat16, False)
    ids = patterns()["c_alternating"]
    o = torch.full((B, T, N), 7.0, dtype=torch.bfloat16, device=DEV)

    def call(T_=T, NR_=NR, ids_=ids.data_ptr(), k_=op["kb"].data_ptr()):
        return lib.supir_xattn_q_d64_regions(op["x"].data_ptr(), op["w"].data_ptr(), None, k_, op["vtb"].data_ptr(), ids_, NR_, o.data_ptr(),
                                             B, H, T_, Tk, C, C, N, op["vtb"].shape[-1], N, None, 0, 0, None, 1e-5, 0.125, None, None)

    assert call(T_=192) == -2          # SUPIR_ERR_SHAPE
    assert call(NR_=0) == -2
    assert call(NR_=256) == -2
    assert call(ids_=None) == -1       # SUPIR_ERR_ARG
    assert call(k_=None) == -1
    torch.cuda.synchronize()
    assert (o == 7.0).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.isfinite(o).all() and not (o == 7.0).all()
