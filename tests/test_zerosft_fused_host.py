"""Host side of the fused ZeroSFT launch (ops.zerosft_conv): the interleaved gamma|beta weight layout against its index formula, and the
module taking today's two-call path whenever the real GPU entry points are not in place (the CPU stand-ins of tests/torch_ops.py and
tests/fake_ops.py swap named entry points of supir_amd.ops and do not know the fused op)."""
import torch

from supir_amd import ops
from supir_amd import weights as Wt
from tests import fake_ops, torch_ops


def test_interleaved_layout_matches_the_index_formula():
    C, Cin = 320, 8
    w_mul = torch.arange(C * 9 * Cin, dtype=torch.float32).reshape(C, 3, 3, Cin)
    w_add = -w_mul - 1.0
    b_mul, b_add = torch.arange(C, dtype=torch.float32), -torch.arange(C, dtype=torch.float32) - 1.0
    wi, bi = Wt.interleave_zerosft(w_mul, w_add, b_mul, b_add)
    assert wi.shape == (2 * C, 3, 3, Cin) and bi.shape == (2 * C,) and wi.is_contiguous() and bi.is_contiguous()
    for n in range(2 * C):
        blk, r = divmod(n, 32)
        src_w, src_b = (w_mul, b_mul) if r < 16 else (w_add, b_add)
        row = 16 * blk + (r & 15)
        assert torch.equal(wi[n], src_w[row]) and bi[n] == src_b[row], n
    # a 160-column tile [160 t, 160 t + 160) of the fused convolution = the modulation maps of output channels [80 t, 80 t + 80)
    t = 3
    rows = [16 * (n // 32) + (n & 15) for n in range(160 * t, 160 * t + 160)]
    assert sorted(set(rows)) == list(range(80 * t, 80 * t + 80))


def test_predicate_conditions_without_a_gpu():
    bf = torch.bfloat16
    ok = dict(B=2, H=32, W=32, Cin=128, C=1920, C1=640, dtype=bf, static=True)
    assert ops.USE_ZSFT_FUSED and ops.zerosft_conv_supported(**ok)
    for C in (640, 960, 1280, 1920, 2560):                      # every adapter width of the model: whole 160-column tiles, 10-channel units
        assert ops.zerosft_conv_supported(**dict(ok, C=C, C1=C)) and (2 * C) % 160 == 0 and (C // 32) % 10 == 0
    assert not ops.zerosft_conv_supported(**dict(ok, dtype=torch.float32))          # the fp32 service
    assert not ops.zerosft_conv_supported(**dict(ok, C=480, C1=480))
    assert not ops.zerosft_conv_supported(**dict(ok, C1=600))
    assert not ops.zerosft_conv_supported(**dict(ok, H=6, W=10))                    # tile latents whose maps are no whole tile rows fall back
    assert not ops.zerosft_conv_supported(**dict(ok, static=False))                 # no producer partials
    saved = ops.USE_ZSFT_FUSED
    try:
        ops.USE_ZSFT_FUSED = False
        assert not ops.zerosft_conv_supported(**ok)
    finally:
        ops.USE_ZSFT_FUSED = saved


def test_module_takes_the_two_call_path_under_the_cpu_stand_ins(monkeypatch):
    from supir_amd.modules.supir_v0 import ZeroSFT
    from tests.helpers import fill_module, synth_tensor

    def refuse(*a, **k):
        raise AssertionError("the fused op must not be reached under a CPU stand-in")

    monkeypatch.setattr(ops, "zerosft_conv", refuse)
    with torch_ops.installed(fp32=True):
        assert not ops.zerosft_conv_supported(2, 16, 16, 128, 640, 320, torch.bfloat16, static=True)
        assert not ops.zerosft_conv_supported(2, 16, 16, 128, 640, 320, torch.float32, static=True)
        m = ZeroSFT(320, 320, concat_channels=320)
        fill_module(m, "model.diffusion_model.project_modules.8.", "cpu")
        c, h, ho = synth_tensor("zf.c", (2, 320, 16, 16)), synth_tensor("zf.hh", (2, 320, 16, 16)), synth_tensor("zf.ho", (2, 320, 16, 16))
        with torch.no_grad():
            side = m.control_side(c)
            assert side.shape[-1] == 2 * 640                      # the gamma|beta maps, as before
            out = m(c, h, ho, control_scale=0.6, pre=side)
            # SUPIR_v0.py:91-113 in plain torch
            F = torch.nn.functional
            actv = F.silu(F.conv2d(c, m.mlp_shared[0].weight, m.mlp_shared[0].bias, padding=1))
            gamma, beta = F.conv2d(actv, m.zero_mul.weight, m.zero_mul.bias, padding=1), F.conv2d(actv, m.zero_add.weight, m.zero_add.bias, padding=1)
            hz = h + F.conv2d(c, m.zero_conv.weight.reshape(320, 320, 1, 1), m.zero_conv.bias)
            n = m.param_free_norm
            ref = F.group_norm(torch.cat([ho, hz], 1), 32, n.weight, n.bias, n.eps) * (gamma + 1) + beta
            ref = ref * 0.6 + torch.cat([ho, h], 1) * 0.4
        assert out.shape == ref.shape and (out.float() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()
    assert ops.conv3x3 is ops._REAL_CONV3X3 and ops.groupnorm is ops._REAL_GROUPNORM      # the stand-in scope restored the real entry points
    undo = fake_ops.install()
    try:
        from supir_amd.utils import tilevae
        assert tilevae.ops is fake_ops and not hasattr(fake_ops, "zerosft_conv")     # the tiled VAE's backend has no fused op to reach
        assert not ops.zerosft_conv_supported(1, 16, 16, 128, 640, 320, tilevae.cdt(), static=True)
    finally:
        undo()
