"""supir_xattn_q_d64 over more than two key tiles: the contexts of chunked long prompts (154, 231, ... text tokens).

Key tile t lives in ring buffer (kv0 + t) % 3 of the kernel: tiles 0 / 1 arrive with the projection's last two K steps, tile 2 goes to
the third buffer, and from tile 3 on a tile re-uses a buffer an earlier tile was read from.  The cases walk that ladder -- a third
tile holding one key, three full tiles, the first re-use (193 keys), a second lap of the ring (321 keys) -- next to the token
counts real prompts give (154 = two chunks, 231 = three).  Operands as tests/test_kernels_gpu.py::_xattn_operands builds them,
with one spiked key at each END of the key axis: the first tile sets a large running maximum every later tile is scaled against,
and the last tile has to rescale everything accumulated before it.  Bounds are the ones the project already holds this kernel to
against the same two references (test_xattn_q_with_layernorm_fold): rel-L2 8e-3 vs fp32 LayerNorm -> Linear -> SDPA and vs the
two-launch HIP path (they differ by q's single 16-bit rounding), 2e-3 between raw and finalised row statistics.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from supir_amd import ops  # noqa: E402

DEV = "cuda"
CASES = [(1, 2, 128, 129, 192),     # third tile holding one key
         (2, 3, 256, 154, 256),     # two chunks
         (1, 2, 128, 192, 192),     # three full tiles
         (1, 2, 128, 193, 192),     # first reuse of a ring buffer
         (1, 5, 384, 231, 320),     # three chunks
         (1, 2, 256, 321, 256)]     # second lap of the ring
DTYPES = [torch.bfloat16, torch.float16]


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def check(out, ref, rel, name=""):
    out, ref = out.float(), ref.float()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert torch.isfinite(out).all(), f"{name}: non-finite output"
    err = ((out - ref).norm() / (ref.norm() + 1e-12)).item()
    mx = (out - ref).abs().max().item()
    bound = 2.0 ** -7 * ref.abs().max().item() + 1e-3
    print(f"{name}: rel-L2 {err:.3e} (bound {rel}), max-abs {mx:.3e} (bound {bound * 1.5:.3e})")
    assert err <= rel, f"{name}: rel-L2 {err:.3e} > {rel} (max-abs {mx:.3e})"
    assert mx <= bound * 1.5, f"{name}: max-abs {mx:.3e} > {bound * 1.5:.3e}"


def _operands(B, H, T, Tk, C, dt):
    N = H * 64
    x = (rnd(B, T, C) * 1.5 + 0.3).to(dt)
    k = rnd(B, Tk, N, seed=1).to(dt)
    k[:, 0] *= 3.0
    k[:, Tk - 1] *= 3.0
    v = rnd(B, Tk, N, seed=2).to(dt)
    Tp = (Tk + 63) // 64 * 64
    vt = torch.zeros(B, N, Tp, dtype=dt, device=DEV)
    vt[:, :, :Tk] = v.permute(0, 2, 1)
    w = rnd(N, C, scale=C ** -0.5, seed=6)
    return x, k, v, vt, w


def _attn_ref(q, k, v, B, H):
    qf, kf, vf = (t.float().reshape(B, -1, H, 64).permute(0, 2, 1, 3) for t in (q, k, v))
    return F.scaled_dot_product_attention(qf, kf, vf).permute(0, 2, 1, 3).reshape(B, -1, H * 64)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,H,T,Tk,C", CASES)
def test_xattn_q_long_context_with_layernorm_fold(B, H, T, Tk, C, dt):
    from supir_amd.weights import compute_dtype, fold_layernorm
    x, k, v, vt, w = _operands(B, H, T, Tk, C, dt)
    assert ops.xattn_q_supported(B, T, C, H, Tk)
    wp = rnd(C, C, scale=C ** -0.5, seed=9).to(dt)
    xs, st = ops.gemm_ln(x.view(B * T, C), wp, None, residual=x.view(B * T, C), emit_stats=True)      # statistics as a producer leaves them
    xs = xs.view(B, T, C)
    gamma, beta = rnd(C, seed=4) * 0.2 + 1.0, rnd(C, seed=5) * 0.2
    with compute_dtype(dt):         # the folded weight in the element type of the library that runs it
        wf, cs, bf_ = fold_layernorm(w, None, gamma, beta)
    out = ops.xattn_q(xs, wf, bf_, k, vt, B, H, T, Tk, ln=st, colsum=cs)
    q_ref = F.layer_norm(xs.float(), (C,), gamma, beta, 1e-5) @ w.to(dt).float().T
    check(out, _attn_ref(q_ref, k, v, B, H), rel=8e-3, name=f"xattn-long-ln {(B, H, T, Tk, C)}")
    two = ops.flash_attn(ops.gemm_ln(xs, wf, bf_, ln=st, colsum=cs), k, vt, B, H, T, Tk)
    check(out, two, rel=8e-3, name=f"xattn-long-vs-two-launches {(B, H, T, Tk, C)}")
    if Tk == 231:    # finalised statistics (slots == 0) take the other branch of the kernel's prologue
        out_f = ops.xattn_q(xs, wf, bf_, k, vt, B, H, T, Tk, ln=ops.rowstats_finalize(st, C, 1e-5), colsum=cs)
        check(out_f, out, rel=2e-3, name="xattn-long-finalised-stats")


def test_xattn_q_long_context_with_a_next_weight_hint():
    """The hint's loads share the wave's load counter with the streamed key tiles and land 4 KB above the tile in the third buffer:
    same bits with and without it, and the hinted matrix is only read."""
    from supir_amd import _lib
    B, H, T, Tk, C = 1, 2, 128, 193, 192
    dt = torch.bfloat16
    N = H * 64
    x, k, v, vt, w = _operands(B, H, T, Tk, C, dt)
    wb = w.to(dt)
    out = ops.xattn_q(x, wb, None, k, vt, B, H, T, Tk)
    check(out, _attn_ref(x.float() @ wb.float().T, k, v, B, H), rel=8e-3, name="xattn-long-plain")
    lib = _lib.load()
    nxt = rnd(1280, 1280, seed=3).to(dt)
    nxt_copy = nxt.clone()
    hints = _lib.LaunchHints(next_weight=nxt.data_ptr(), next_weight_bytes=nxt.numel() * 2, gn_partials_out=None)
    o2 = torch.empty(B, T, N, dtype=dt, device=DEV)
    rc = lib.supir_xattn_q_d64(x.data_ptr(), wb.data_ptr(), None, k.data_ptr(), vt.data_ptr(), o2.data_ptr(), B, H, T, Tk, C, C, N,
                               vt.shape[-1], N, None, 0, 0, None, 1e-5, 0.125, ctypes.byref(hints), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(o2, out) and torch.equal(nxt, nxt_copy)


def test_xattn_q_refuses_a_vt_narrower_than_the_keys():
    """Tk = 154 needs three 64-key columns blocks of V^T; on a 128-wide one the entry returns SUPIR_ERR_SHAPE and launches nothing."""
    from supir_amd import _lib
    lib = _lib.load()
    B, H, T, Tk, C = 1, 2, 128, 154, 256
    x, k, v, vt, w = _operands(B, H, T, Tk, C, torch.bfloat16)
    wb = w.to(torch.bfloat16)
    narrow = vt[:, :, :128].contiguous()
    o = torch.full((B, T, H * 64), 7.0, dtype=torch.bfloat16, device=DEV)

    def call(vt_):
        return lib.supir_xattn_q_d64(x.data_ptr(), wb.data_ptr(), None, k.data_ptr(), vt_.data_ptr(), o.data_ptr(), B, H, T, Tk, C, C,
                                     H * 64, vt_.shape[-1], H * 64, None, 0, 0, None, 1e-5, 0.125, None, None)
    assert call(narrow) == -2
    torch.cuda.synchronize()
    assert (o == 7.0).all()
    assert call(vt) == 0
    torch.cuda.synchronize()
    check(o, _attn_ref(x.float() @ wb.float().T, k, v, B, H), rel=8e-3, name="xattn-long-direct")
