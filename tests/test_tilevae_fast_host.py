"""Fast mode / color_fix / tile_chunk of supir_amd/utils/tilevae.py on a box without a GPU: the host logic (index rule, estimate,
per-GroupNorm choice between estimated and pooled statistics, chunked execution, fall-back) with the kernels served by plain torch
(tests/tilevae_fast_support.py), held to what the reference's own VAEHook computed (tests/golden/golden_tilevae_fast.pt.*)."""
import math
import warnings

import pytest
import torch
import torch.nn.functional as F

from tests import tilevae_fast_support as S
from tests.helpers import build_vae, golden, rel_l2

TOL = 1e-4     # the tolerance tests/test_host_path_cpu.py::test_tiled_vae_vs_reference_golden holds the non-fast fixtures to


@pytest.fixture(scope="module")
def backend():
    with S.installed(fp32=True) as be:
        yield be


@pytest.fixture(scope="module")
def vae(backend):
    return build_vae("cpu")


def _index_cases():
    cases = [(4096, 4096, 512), (512, 512, 64), (2048, 2048, 512), (1088, 1920, 512), (1920, 1088, 512), (136, 240, 64), (40, 32, 8),
             (192, 160, 64), (44, 36, 8), (352, 288, 64)]
    g = torch.Generator().manual_seed(7)
    while len(cases) < 240:
        t = int(torch.randint(4, 97, (1,), generator=g))
        h, w = (int(v) for v in torch.randint(t + 1, 12 * t + 64, (2,), generator=g))
        cases.append((h, w, t))
    return cases


def test_index_rule_is_interpolate_nearest_exact_with_the_given_scale():
    """A: nearest_exact_index == the pixels F.interpolate(scale_factor=s, mode="nearest-exact") picks, sizes included; exact."""
    from supir_amd.utils.tilevae import nearest_exact_index
    cases = _index_cases()
    assert len(cases) >= 200
    differs_from_size_rule = 0
    for h, w, t in cases:
        s = t / max(h, w)
        ramp = torch.arange(h * w, dtype=torch.float32).view(1, 1, h, w)
        want = F.interpolate(ramp, scale_factor=s, mode="nearest-exact")
        iy, ix = nearest_exact_index(h, s), nearest_exact_index(w, s)
        assert (iy.numel(), ix.numel()) == tuple(want.shape[2:]) == (math.floor(h * s), math.floor(w * s)), (h, w, t)
        assert iy.dtype == torch.int32 and int(iy.min()) >= 0 and int(iy.max()) < h and int(ix.min()) >= 0 and int(ix.max()) < w
        got = ramp[:, :, iy.long()][:, :, :, ix.long()]
        assert torch.equal(got, want), (h, w, t)
        differs_from_size_rule += int(not torch.equal(want, F.interpolate(ramp, size=tuple(want.shape[2:]), mode="nearest-exact")))
    assert differs_from_size_rule > 0      # the cases do tell the given scale from in / out


def _stats_close(got, want):
    """gnstats_*: per entry <= 1e-4 relative on mean (1e-5 absolute near zero) and on variance."""
    assert len(got) == want.shape[0], (len(got), want.shape)
    worst_m = worst_v = 0.0
    for g, w in zip(got, want):
        assert g.shape == w.shape
        dm = (g[..., 0] - w[..., 0]).abs()
        worst_m = max(worst_m, float((dm / w[..., 0].abs().clamp_min(1e-20)).where(dm > 1e-5, torch.zeros(())).max()))
        worst_v = max(worst_v, float(((g[..., 1] - w[..., 1]).abs() / w[..., 1].abs().clamp_min(1e-20)).max()))
    return worst_m, worst_v


@pytest.mark.parametrize("case", list(S.CASES))
def test_fast_modes_vs_reference_fixture(vae, case):
    """B: the down-sampled and repaired input, the statistics the estimate records and the hook's output, per case."""
    fx = S.load_fixture()
    hook, x = S.make_hook(vae, case)
    with torch.no_grad():
        small = hook.downsample_for_estimate(x.float().contiguous())
        stats = hook.estimate_group_norm(x.float().contiguous())
        out = hook(x)
    e_small = rel_l2(small, fx["small_" + case])
    wm, wv = _stats_close(stats, fx["gnstats_" + case])
    e_out = rel_l2(out, fx["fast_" + case])
    print(f"{case}: small {e_small:.3e}  gnstats mean {wm:.3e} var {wv:.3e}  output {e_out:.3e}")
    assert small.shape == fx["small_" + case].shape and e_small <= 1e-5
    assert wm <= 1e-4 and wv <= 1e-4
    assert e_out <= TOL


def test_modes_are_told_apart_on_the_host_too(vae):
    """The fixture's own distances: fast is far from non-fast, color_fix far from plain fast (what makes the comparisons above mean
    something), and the hooks with all flags off still give the non-fast goldens."""
    fx, g = S.load_fixture(), golden()
    d = fx["meta"]["rel_l2"]
    assert d["dec_fast_vs_nonfast"] > 0.1 and d["enc_fast_vs_nonfast"] > 0.1 and d["enc_cf_vs_fast"] > 0.1
    hook, x = S.make_hook(vae, "dec_40x32_t8", fast_decoder=False)
    with torch.no_grad():
        assert rel_l2(hook(x), g["tiled_dec_40x32_t8"]) <= TOL


@pytest.mark.parametrize("case", ["dec_40x32_t8", "enc_192x160_t64", "dec_n2_44x36_t8"])
def test_tile_chunk_does_not_change_the_result(vae, case):
    """C: tile_chunk 1 / 3 / everything == all tiles at once.  A chunk that keeps every stack whole only reorders the launches: bitwise.
    Smaller chunks change the batch size of the stand-in's convolutions, and torch's CPU convolution picks its algorithm (and with it
    its fp32 summation order) by batch size, so there equality holds up to that: 2e-5, the bound tests/test_host_path_cpu.py puts on
    "a different association of the same arithmetic" -- five orders below the distance between the modes."""
    hook, x = S.make_hook(vae, case)
    with torch.no_grad():
        want = hook(x)
        assert torch.equal(S.make_hook(vae, case, tile_chunk=10 ** 6)[0](x), want)
        for k in (1, 3):
            got = S.make_hook(vae, case, tile_chunk=k)[0](x)
            err = rel_l2(got, want)
            print(f"{case}: tile_chunk={k} vs all tiles at once {err:.3e}")
            assert err <= 2e-5, (case, k, err)


def test_tile_chunk_needs_independent_tiles(vae):
    from supir_amd.utils.tilevae import VAEHook
    with pytest.raises(ValueError):
        VAEHook(vae.decoder, 8, is_decoder=True, tile_chunk=2)                                        # fast mode off
    with pytest.raises(ValueError):
        VAEHook(vae.denoise_encoder, 64, is_decoder=False, fast_encoder=True, color_fix=True, tile_chunk=2)
    with pytest.raises(ValueError):
        VAEHook(vae.decoder, 8, is_decoder=True, fast_encoder=True, tile_chunk=2)                      # the encoder's flag on a decoder
    with pytest.raises(ValueError):
        VAEHook(vae.decoder, 8, is_decoder=True, fast_decoder=True, tile_chunk=0)
    h = VAEHook(vae.decoder, 8, is_decoder=True, fast_decoder=True, color_fix=True, tile_chunk=2)     # color_fix is encoder-only
    assert h.fast_mode and not h.color_fix and h.tile_chunk == 2


@pytest.mark.parametrize("case,key", [("dec_40x32_t8", "tiled_dec_40x32_t8"), ("enc_192x160_t64", "tiled_enc_192x160_t64")])
def test_non_finite_estimate_falls_back_to_the_pooled_path(vae, case, key):
    """C: an inf among the recorded statistics -> one warning, and the call is the non-fast path (tile_chunk ignored for it)."""
    hook, x = S.make_hook(vae, case, tile_chunk=2)
    inner = hook.estimate_group_norm

    def poisoned(z):
        rec = inner(z)
        rec[len(rec) // 2] = rec[len(rec) // 2].clone()
        rec[len(rec) // 2][0, 3, 1] = float("inf")
        return rec

    hook.estimate_group_norm = poisoned
    with torch.no_grad(), warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = hook(x)
        nonfast = S.make_hook(vae, case, fast_decoder=False, fast_encoder=False)[0](x)
    assert sum("non-finite" in str(m.message) for m in w) == 1
    assert torch.equal(out, nonfast) and rel_l2(out, golden()[key]) <= TOL


def test_init_tile_vae_defaults_keep_every_flag_off(vae):
    """E: SUPIRModel.init_tile_vae() without keywords installs what it always did; the new keywords reach the hooks."""
    import types
    from supir_amd.models.supir_model import SUPIRModel
    from supir_amd.utils.tilevae import VAEHook

    def nets():
        import torch.nn as nn
        fs = types.SimpleNamespace(denoise_encoder=nn.Identity(), encoder=nn.Identity(), decoder=nn.Identity())
        return types.SimpleNamespace(first_stage_model=fs), fs

    m, fs = nets()
    SUPIRModel.init_tile_vae(m)
    for net, size, dec in ((fs.denoise_encoder, 512, False), (fs.encoder, 512, False), (fs.decoder, 64, True)):
        h = net.forward
        assert isinstance(h, VAEHook) and (h.tile_size, h.is_decoder) == (size, dec)
        assert not h.fast_mode and not h.color_fix and h.tile_chunk is None and not h.tile_parallel
    m, fs = nets()
    SUPIRModel.init_tile_vae(m, 256, 32, fast_encoder=True, fast_decoder=True, color_fix=True, tile_chunk=4)
    e, d = fs.encoder.forward, fs.decoder.forward
    assert e.fast_mode and e.color_fix and e.tile_chunk is None and e.tile_size == 256      # pooled norms remain: no chunking
    assert d.fast_mode and not d.color_fix and d.tile_chunk == 4 and d.tile_size == 32
    m, fs = nets()
    SUPIRModel.init_tile_vae(m, fast_encoder=True, tile_chunk=2)
    assert fs.denoise_encoder.forward.tile_chunk == 2 and fs.decoder.forward.tile_chunk is None and not fs.decoder.forward.fast_mode
