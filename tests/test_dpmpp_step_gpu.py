"""supir_dpmpp2m_step_post / _tiles (csrc/sampler.hip): the post half of RestoreDPMPP2MSampler.sampler_step
(sgm/modules/diffusionmodules/sampling.py:429-483) against the torch expressions it replaces, and both DPM++ samplers on the fused
step (supir_edm_step_pre + network + the post kernel, host-side scalars, per-image embedding schedule, hipGraph replay) against
their generic torch-op path with the real reduced-depth network.  Same bars as tests/test_sampler_fused_gpu.py for EDM."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from supir_amd import ops  # noqa: E402
from tests.helpers import build_unet, rel_l2, synth_tensor  # noqa: E402

DEV = "cuda"
SC = dict(c_out=-3.7125, c_skip=1.0, cfg=5.13, m1=0.8312, m2=-0.2247, m3=1.4376, m4=0.4376, noise_mul=0.6021, s_noise=1.003)


def T(name, shape, **kw):
    return synth_tensor(name, shape, **kw).to(DEV)


def _ref(net_out, x, old, eps, reps, c_out, c_skip, cfg, m1, m2, m3, m4, noise_mul, s_noise):
    """sampler_step's torch expressions (the port's operation order, supir_amd/modules/sampling.py) with scalar factors."""
    dens = [h * c_out + x * c_skip for h in net_out.chunk(reps)]
    den = dens[0] + cfg * (dens[1] - dens[0]) if reps == 2 else dens[0]
    if old is None:
        return m1 * x - m2 * den, den
    dd = m3 * den - m4 * old
    xn = m1 * x - m2 * dd
    if eps is not None:
        xn = xn + (eps * noise_mul) * s_noise
    return xn, den


def _close(a, b):
    assert torch.allclose(a, b, rtol=1e-6, atol=1e-6), (a - b).abs().max()


@pytest.mark.parametrize("shape", [(1, 4, 128, 128), (2, 4, 64, 64), (3, 4, 9, 7), (1, 1, 1, 3), (1, 3, 5, 7)])
@pytest.mark.parametrize("reps", [2, 1])
def test_dpmpp_post_kernel_vs_torch(shape, reps):
    n = 1
    for d in shape:
        n *= d
    if reps == 2 and n % 4:
        pytest.skip("CFG doubling needs n % 4 == 0 (latents have 4 channels)")
    x, old, eps = T("dp.x", shape), T("dp.old", shape), T("dp.eps", shape)
    net_out = T("dp.n", (reps * shape[0],) + shape[1:])
    for o, e in ((None, None), (old, None), (old, eps)):
        xn, den = ops.dpmpp2m_step_post(net_out, x, o, e, *SC.values(), reps)
        rx, rd = _ref(net_out, x, o, e, reps, **SC)
        _close(xn, rx)
        _close(den, rd)
    # eps without old (a first step that was handed noise) is ignored, as sampler_step ignores it
    xn, _ = ops.dpmpp2m_step_post(net_out, x, None, eps, *SC.values(), reps)
    _close(xn, _ref(net_out, x, None, None, reps, **SC)[0])


@pytest.mark.parametrize("geom", [(1, 4, 96, 96, 32, 16, 4), (2, 4, 80, 100, 32, 24, 3), (1, 4, 33, 35, 32, 16, 4), (1, 4, 64, 64, 64, 32, 1)])
@pytest.mark.parametrize("reps", [2, 1])
def test_dpmpp_post_tiles_kernel_vs_torch(geom, reps):
    """Overlapping tiles, last windows shifted to the canvas edge (odd origins), several samples, groups of k tiles; old / eps read
    through the windows of the canvases; the results blended with supir_tile_blend equal the reference's slice-adds."""
    from supir_amd.modules.sampling import _sliding_windows, _stack, gaussian_weights
    b, C, Hc, Wc, Tt, stride, k = geom
    tiles = _sliding_windows(Hc, Wc, Tt, stride)
    x, old, eps = T("dpt.x", (b, C, Hc, Wc)), T("dpt.old", (b, C, Hc, Wc)), T("dpt.eps", (b, C, Hc, Wc))
    w = gaussian_weights(Tt, Tt, 1, device=DEV)
    x_next, ref_next = torch.zeros_like(x), torch.zeros_like(x)
    for j0 in range(0, len(tiles), k):
        grp = tiles[j0:j0 + k]
        x_t, _ = ops.edm_step_pre_tiles(x, None, grp, Tt, 1.0, 0.0, 0.25, reps)
        assert torch.equal(x_t, _stack(x, grp))
        net_out = T(f"dpt.n{j0}", (reps * len(grp) * b, C, Tt, Tt))
        for o, e in ((None, None), (old, None), (old, eps)):
            xn, den = ops.dpmpp2m_step_post_tiles(net_out, x_t, o, e, grp, *SC.values(), reps)
            rx, rd = _ref(net_out, x_t, None if o is None else _stack(o, grp), None if e is None else _stack(e, grp), reps, **SC)
            _close(xn, rx)
            _close(den, rd)
        ops.tile_blend(xn, w[0, 0].contiguous(), x_next, grp, Tt)
        for (hi, he, wi, we), t in zip(grp, rx.chunk(len(grp), 0)):
            ref_next[:, :, hi:he, wi:we] += t * w.repeat(b, 1, 1, 1)
    assert torch.allclose(x_next, ref_next, rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------------------------------------ samplers
def _setup(h, w):
    from supir_amd.modules.sampling import DiscreteDenoiserWithControl
    mini = build_unet(depth=(1, 1, 2), device=DEV)
    den = DiscreteDenoiserWithControl().to(DEV)
    ctx, y = T("context", (2, 77, 2048)), T("vector", (2, 2816))
    lq = T("dpg.lq", (1, 4, h, w))
    c = {"crossattn": ctx[:1], "vector": y[:1], "control": lq}
    uc = {"crossattn": ctx[1:], "vector": y[1:], "control": lq}

    def denoiser(i, s, cc, cs):
        return den(mini, i, s, cc, cs)

    return mini, den, denoiser, c, uc


def _recording_noise(queries):
    from supir_amd.modules.sampling import default_noise_sampler_cls

    class Recording(default_noise_sampler_cls()):
        def __call__(self, sigma, sigma_next):
            queries.append((float(sigma.reshape(-1)[0]), float(sigma_next.reshape(-1)[0])))
            return super().__call__(sigma, sigma_next)

    return Recording


def _modes(monkeypatch, mini, den, denoiser, make, run):
    """generic / fused / fused+graph, two images in a row each; returns {mode: (outputs, next RNG draws, noise queries)}."""
    from supir_amd.modules import sampling
    res = {}
    for mode in ("generic", "fused", "fused+graph"):
        if mode == "generic":
            denoiser.__dict__.pop("fused", None)
        else:
            denoiser.fused = (den, mini)
        monkeypatch.setattr(sampling, "FUSED_EDM_STEP", mode != "generic")
        mini.enable_graph(mode == "fused+graph")
        queries, outs, draws = [], [], []
        smp = make(_recording_noise(queries))
        assert (smp._fused_ctx(denoiser, torch.zeros(1, device=DEV)) is not None) == (mode != "generic")
        try:
            for img in range(2):
                torch.manual_seed(321 + img)
                with torch.no_grad():
                    outs.append(run(smp, img).float().clone())
                draws.append(torch.randn(4, device=DEV))   # equal iff both paths consumed the same number of values
        finally:
            mini.enable_graph(False)
        assert mini._sched is None and not mini._scheds
        res[mode] = (outs, draws, queries)
    return res


def _check_modes(res, tag):
    g_outs, g_draws, g_q = res["generic"]
    assert len(g_q) > 0
    for mode in ("fused", "fused+graph"):
        outs, draws, q = res[mode]
        for i in range(2):
            e = rel_l2(outs[i], g_outs[i])
            print(f"[{tag} {mode}] image {i}: rel-L2 vs generic {e:.3e}")
            assert e <= 1e-2, (mode, i, e)
            assert torch.equal(draws[i], g_draws[i])
        assert q == g_q
    for i in range(2):
        assert torch.equal(res["fused"][0][i], res["fused+graph"][0][i])      # graph == eager


@pytest.mark.parametrize("steps", [4, 8])
def test_dpmpp_sampler_fused_vs_generic(monkeypatch, steps):
    from supir_amd.modules.sampling import LinearCFG, RestoreDPMPP2MSampler
    h = w = 32
    mini, den, denoiser, c, uc = _setup(h, w)

    def make(ns):
        return RestoreDPMPP2MSampler(num_steps=steps, s_noise=1.003, eta=1.0, restore_cfg=4.0, guider_config=LinearCFG(7.5, 4.0),
                                     device=DEV, noise_sampler_cls=ns)

    def run(smp, img):
        return smp(denoiser, T(f"dpg.x0_{img}", (1, 4, h, w)).clone(), cond=dict(c), uc=dict(uc), control_scale=1.0)

    _check_modes(_modes(monkeypatch, mini, den, denoiser, make, run), f"dpmpp {steps} steps")


@pytest.mark.parametrize("steps", [4, 8])
def test_tiled_dpmpp_sampler_fused_vs_generic(monkeypatch, steps):
    """Latent 48 x 64 as 32 x 32 tiles (stride 16: 6 tiles), tile_batch 4: a full group of 4 and a remainder group of 2 -- two batch
    sizes, two embedding schedules, two graphs."""
    from supir_amd.modules.sampling import LinearCFG, TiledRestoreDPMPP2MSampler
    h, w = 48, 64
    mini, den, denoiser, c, uc = _setup(h, w)

    def make(ns):
        return TiledRestoreDPMPP2MSampler(32, 16, num_steps=steps, s_noise=1.003, eta=1.0, restore_cfg=4.0,
                                          guider_config=LinearCFG(7.5, 4.0), device=DEV, noise_sampler_cls=ns, tile_batch=4)

    def run(smp, img):
        return smp(denoiser, T(f"dpg.x0t_{img}", (1, 4, h, w)).clone(), cond=dict(c), uc=dict(uc), control_scale=1.0)

    _check_modes(_modes(monkeypatch, mini, den, denoiser, make, run), f"tiled dpmpp {steps} steps")


def test_dpmpp_fused_step_fp16_network_vs_fp32_oracle(monkeypatch):
    """BASELINE config 5's sampler on the FUSED step driving the fp16 network vs the generic sampler driving the fp32 oracle network,
    scripted noise, 4 and 8 steps: the bar of tests/test_fp16_gpu.py::test_dpmpp2m_config5_sampler_fp16 (1e-3)."""
    from oracle import supir_oracle as O
    from supir_amd.modules import sampling, wrappers
    from supir_amd.modules.sampling import LinearCFG, RestoreDPMPP2MSampler
    monkeypatch.setattr(wrappers, "FP16_NATIVE", True)
    monkeypatch.setattr(sampling, "FUSED_EDM_STEP", True)
    h = w = 32
    mini, den, denoiser, c, uc = _setup(h, w)
    sd = {}
    for pfx, mod in (("model.diffusion_model.", mini.diffusion_model), ("model.control_model.", mini.control_model)):
        for k, v in mod.state_dict().items():
            sd[pfx + k] = v
    x0 = T("dpm.gpu.x0", (1, 4, h, w))

    class Scripted:
        def __init__(self, x, *a, **k):
            self.i = 0

        def __call__(self, s, sn):
            self.i += 1
            return T(f"dpm.gpu.eps{self.i}", (1, 4, h, w))

    def oracle(i, s, cc, cs):
        return den(lambda a, b_, ccc, s_: O.control_wrapper(sd, a, b_, ccc, s_), i, s, cc, cs)

    denoiser.fused = (den, mini)
    res = {}
    mini.dtype = torch.float16
    try:
        for steps in (8, 4):
            outs = []
            for dn in (denoiser, oracle):
                smp = RestoreDPMPP2MSampler(num_steps=steps, s_noise=1.0, eta=1.0, restore_cfg=4.0, guider_config=LinearCFG(2.0, 2.0),
                                            device=DEV, noise_sampler_cls=Scripted)
                assert (smp._fused_ctx(dn, x0) is not None) == (dn is denoiser)
                with torch.no_grad():
                    outs.append(smp(dn, x0.clone(), cond=dict(c), uc=dict(uc), control_scale=1.0).float())
            res[steps] = rel_l2(outs[0], outs[1])
            assert torch.isfinite(outs[0]).all()
    finally:
        mini.dtype = torch.bfloat16
    print(f"[dpmpp fused fp16] rel-L2 vs fp32 oracle: {res}")
    assert max(res.values()) <= 1e-3, res
