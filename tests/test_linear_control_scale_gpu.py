"""Dynamic control scale on the GPU: the ZeroSFT GroupNorm and ZeroCrossAttn GEMM forms that read the scale from a device cell
against their float forms (bitwise), and linear Stage-2 guidance (`use_linear_control_scale`, sampling.py:557-559) replayed from ONE
captured graph per shape, bitwise what the float-scale path computes (SUPIR_DYNAMIC_CONTROL_SCALE=0)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from supir_amd import ops  # noqa: E402
from tests.helpers import build_unet, synth_tensor  # noqa: E402

DEV = "cuda"
SCALES = (0.0, 0.37, 0.8, 1.0)


def T(name, shape, dt=torch.float32, **kw):
    return synth_tensor(name, shape, **kw).to(DEV, dt)


def _cell(v):
    return torch.full((1,), v, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("c1,c2", [(640, 320), (1280, 1280), (0, 1280)])   # ZeroSFT concat forms [h_ori | h] and the plain form
@pytest.mark.parametrize("parts", [False, True])
def test_zerosft_groupnorm_dynamic_vs_float(dt, c1, c2, parts):
    B, H, W = 2, 16, 16
    M = B * H * W
    C = c1 + c2
    h = T("dcs.h", (M, 256), dt)
    gamma, beta = T("dcs.g", (C,), scale=0.2) + 1.0, T("dcs.b", (C,), scale=0.2)
    gb = T("dcs.gb", (B, H, W, 2 * C), dt, scale=0.3)
    # the producers: h + zero_conv(c) (and h_ori) as GEMMs that may leave GroupNorm partials behind
    # tile 34 (256 x 160) emits the partials supir_groupnorm_nhwc_parts reads
    w2, raw2 = T("dcs.w2", (c2, 256), dt, scale=0.05), T("dcs.r2", (M, c2), dt)
    hz, pz = ops.gemm(h, w2, residual=raw2, rows_per_batch=H * W, gn_part=True, tile=34)
    pz = pz if parts else None
    if c1:
        w1 = T("dcs.w1", (c1, 256), dt, scale=0.05)
        ho, po = ops.gemm(h, w1, rows_per_batch=H * W, gn_part=True, tile=34)
        po = po if parts else None
    if parts:
        assert pz is not None and (not c1 or po is not None)

    def run(cs, dyn):
        raw = raw2.view(B, H, W, c2) if (dyn or cs != 1.0) else None
        scale = _cell(cs) if dyn else cs
        if c1:
            return ops.groupnorm(ho.view(B, H, W, c1), gamma, beta, 1e-5, x2=hz.view(B, H, W, c2), mod_g=gb[..., :C], mod_b=gb[..., C:],
                                 control_scale=scale, x2raw=raw, part=po, part2=pz)
        return ops.groupnorm(hz.view(B, H, W, c2), gamma, beta, 1e-5, mod_g=gb[..., :C], mod_b=gb[..., C:], control_scale=scale,
                             x1raw=raw, part=pz)

    outs = []
    for cs in SCALES:
        a, b = run(cs, False), run(cs, True)
        assert torch.equal(a, b), (cs, (a.float() - b.float()).abs().max())
        outs.append(b)
    assert not torch.equal(outs[0], outs[-1])


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("M,C", [(2048, 1280), (8192, 640), (128, 1280), (512, 640)])   # ZeroCrossAttn.to_out at 128^2 / 32^2 latents
def test_zerocrossattn_gemm_dynamic_vs_float_every_tile(dt, M, C):
    a, w, bias = T("dcs.o", (M, C), dt), T("dcs.wo", (C, C), dt, scale=0.03), T("dcs.bo", (C,))
    res = T("dcs.x", (M, C), dt)
    tiles = ops._gemm_candidates(M, C, C, 0, 0, C)
    assert any(t >= 32 for t in tiles) and any(t < 32 for t in tiles)
    for t in tiles:
        for cs in SCALES:
            ref = ops.gemm(a, w, bias, residual=res, alpha=cs, tile=t)
            got = ops.gemm(a, w, bias, residual=res, alpha=_cell(cs), tile=t)
            torch.cuda.synchronize()
            assert torch.equal(ref, got), (t, cs)


def _setup(h, w, names):
    from supir_amd.modules.sampling import DiscreteDenoiserWithControl
    mini = build_unet(depth=(1, 1, 2), device=DEV)
    den = DiscreteDenoiserWithControl().to(DEV)
    ctx, y = T("context", (2, 77, 2048)), T("vector", (2, 2816))
    lq, xc = T(names[0], (1, 4, h, w)), T(names[1], (1, 4, h, w))
    c = {"crossattn": ctx[:1], "vector": y[:1], "control": lq}
    uc = {"crossattn": ctx[1:], "vector": y[1:], "control": lq}

    def denoiser(i, s, cc, cs):
        return den(mini, i, s, cc, cs)

    denoiser.fused = (den, mini)
    return mini, denoiser, c, uc, xc


def test_untiled_linear_control_scale_replays_one_graph(monkeypatch):
    """8 steps with churn, linear CFG and a linear control scale: one capture and eight replays with the dynamic cell, bitwise the
    float-scale run (which captures the first two steps' graphs and runs the other six eagerly)."""
    from supir_amd.modules import sampling
    from supir_amd.modules.sampling import LinearCFG, RestoreEDMSampler
    h = w = 32
    mini, denoiser, c, uc, xc = _setup(h, w, ("lq_tiled", "fs.center"))
    monkeypatch.setattr(sampling, "FUSED_EDM_STEP", True)
    monkeypatch.setattr(sampling, "EMB_SCHEDULE", True)
    smp = RestoreEDMSampler(num_steps=8, s_churn=5, s_noise=1.01, restore_cfg=4.0, guider_config=LinearCFG(1.0, 4.0), device=DEV)
    for cs, cs0 in ((1.0, 0.0), (0.8, 0.3)):
        res, stats = {}, {}
        for dyn in (False, True):
            monkeypatch.setattr(sampling, "DYNAMIC_CONTROL_SCALE", dyn)
            mini.enable_graph(True)
            try:
                torch.manual_seed(77)
                with torch.no_grad():
                    res[dyn] = smp(denoiser, T("fs.x0", (1, 4, h, w)).clone(), cond=dict(c), uc=dict(uc), x_center=xc, control_scale=cs,
                                   use_linear_control_scale=True, control_scale_start=cs0).float().clone()
                stats[dyn] = mini.graph_stats()
            finally:
                mini.enable_graph(False)
            assert mini._sched is None and mini._cs_table is None
        print(f"[linear cs {cs} from {cs0}] graph stats: dynamic {stats[True]}, float {stats[False]}")
        assert stats[True] == {"captures": 1, "replays": 8, "eager": 0}
        assert stats[False]["captures"] == 2 and stats[False]["eager"] == 6
        assert torch.equal(res[True], res[False])


def test_tiled_linear_control_scale_captures_once_per_group_shape(monkeypatch):
    """Latent 48 x 64 as 32^2 tiles (6 tiles: groups of 4 and 2), tile batch 4, 3 steps: 2 captures over the whole image, bitwise
    the float-scale run."""
    from supir_amd.modules import sampling
    from supir_amd.modules.sampling import LinearCFG, TiledRestoreEDMSampler
    h, w = 48, 64
    mini, denoiser, c, uc, xc = _setup(h, w, ("lq_tiled2", "fs.center2"))
    monkeypatch.setattr(sampling, "FUSED_EDM_STEP", True)
    monkeypatch.setattr(sampling, "EMB_SCHEDULE", True)
    res, stats = {}, {}
    for dyn in (False, True):
        monkeypatch.setattr(sampling, "DYNAMIC_CONTROL_SCALE", dyn)
        smp = TiledRestoreEDMSampler(32, 16, num_steps=3, s_churn=5, s_noise=1.01, restore_cfg=4.0, guider_config=LinearCFG(1.0, 4.0),
                                     device=DEV, tile_batch=4)
        mini.enable_graph(True)
        try:
            torch.manual_seed(321)
            with torch.no_grad():
                res[dyn] = smp(denoiser, T("fs.x0t0", (1, 4, h, w)).clone(), cond=dict(c), uc=dict(uc), x_center=xc, control_scale=0.8,
                               use_linear_control_scale=True, control_scale_start=0.3).float().clone()
            stats[dyn] = mini.graph_stats()
        finally:
            mini.enable_graph(False)
    print(f"[tiled linear cs] graph stats: dynamic {stats[True]}, float {stats[False]}")
    assert stats[True] == {"captures": 2, "replays": 6, "eager": 0}
    assert torch.equal(res[True], res[False])


def test_full_depth_call_dynamic_cell_is_bitwise_the_float_scale():
    """One CFG-doubled call of the full-depth network at latent 128^2: a cell holding v gives bitwise the float-v output."""
    wrap = build_unet(device=DEV)
    x = T("xt", (2, 4, 128, 128))
    cond = {"crossattn": T("context", (2, 77, 2048)), "vector": T("vector", (2, 2816)), "control": T("lq", (2, 4, 128, 128))}
    t = torch.tensor([500, 37], dtype=torch.int64, device=DEV)
    with torch.no_grad():
        for v in (0.6, 1.0):
            a = wrap(x, t, cond, v).clone()
            b = wrap(x, t, cond, _cell(v)).clone()
            assert torch.equal(a, b), v
