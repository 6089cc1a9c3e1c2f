"""Tile 37 (csrc/gemm_big.hip, 256 x 320, v_mfma_f32_16x16x32) against an fp32 value * gelu(gate) reference at the two production GEGLU
shapes of a 1024^2 step, for both GELU codes (fitted and erf), with the LayerNorm fold on and off and the bias on and off.
Tolerances are the ones tests/test_kernels_gpu.py states for the GEMM family (rel-L2 4e-3, 8e-3 with the LayerNorm fold)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from supir_amd import ops  # noqa: E402
from supir_amd.weights import fold_layernorm, interleave_geglu  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def check(out, ref, rel, name):
    out, ref = out.float(), ref.float()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{name}: non-finite output"
    err = ((out - ref).norm() / (ref.norm() + 1e-12)).item()
    mx = (out - ref).abs().max().item()
    bound = 2.0 ** -7 * ref.abs().max().item() + 1e-3
    assert err <= rel, f"{name}: rel-L2 {err:.3e} > {rel} (max-abs {mx:.3e})"
    assert mx <= bound * 1.5, f"{name}: max-abs {mx:.3e} > {bound * 1.5:.3e}"


@pytest.mark.parametrize("exact", [False, True], ids=["fitted", "erf"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("M,N2,K", [(2048, 10240, 1280), (8192, 5120, 640)])
def test_geglu_tile37_vs_fp32(M, N2, K, with_bias, exact, monkeypatch):
    monkeypatch.setattr(ops, "EXACT_GELU", exact)
    a = rnd(M, K).to(BF)
    w = rnd(N2, K, scale=K ** -0.5, seed=1).to(BF)
    bias = rnd(N2, seed=2) if with_bias else None
    w16, b16 = interleave_geglu(w, bias, 16)
    tag = f"{(M, N2, K)} {'erf' if exact else 'fitted'} bias={with_bias}"

    # LayerNorm fold off
    out = ops.gemm(a, w16, b16, act=2, tile=37)
    y = a.float() @ w.float().T + (bias if with_bias else 0.0)
    v, g = y.chunk(2, dim=-1)
    check(out, v * F.gelu(g), rel=4e-3, name=f"geglu {tag}")
    assert torch.equal(out, ops.gemm(a, w16, b16, act=2, tile=37))   # bitwise repeatable
    # the 256 x 160 tile of gemm16.hip runs the same MFMA shape and epilogue arithmetic: equal to rounding
    check(out, ops.gemm(a, w16, b16, act=2, tile=34).float(), rel=3e-3, name=f"tile 37 vs tile 34 {tag}")

    # LayerNorm fold on: statistics as the producer GEMM leaves them (partial per tile column) and finalised
    C = K
    wp = rnd(C, C, scale=C ** -0.5, seed=5).to(BF)
    x, st = ops.gemm_ln(a, wp, None, emit_stats=True)
    # without a bias the LayerNorm has no shift either, so the launch gets no bias vector at all
    gamma = rnd(C, seed=6) * 0.2 + 1.0
    beta = rnd(C, seed=7) * 0.2 if with_bias else torch.zeros(C, device=DEV)
    wf, cs, bf_ = fold_layernorm(w.float(), bias, gamma, beta)
    wf16, bf16_ = interleave_geglu(wf, bf_ if with_bias else None, 16)
    _, cs16 = interleave_geglu(wf, cs, 16)
    yr = F.layer_norm(x.float(), (C,), gamma, beta, 1e-5) @ w.float().T + (bias if with_bias else 0.0)
    vr, gr = yr.chunk(2, dim=-1)
    ref = vr * F.gelu(gr)
    check(ops.gemm_ln(x, wf16, bf16_, act=2, ln=st, colsum=cs16, tile=37), ref, rel=8e-3, name=f"ln-fold {tag}")
    fin = ops.rowstats_finalize(st, C, 1e-5)
    check(ops.gemm_ln(x, wf16, bf16_, act=2, ln=fin, colsum=cs16, tile=37), ref, rel=8e-3, name=f"ln-fold finalised {tag}")
