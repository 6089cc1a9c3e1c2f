"""Fast mode / color_fix / tile_chunk of the tiled VAE on the HIP kernels, against what the reference's own VAEHook computed on the
same inputs (tests/golden/golden_tilevae_fast.pt.*, CPU fp32; tools/gen_golden_tilevae_fast.py).  Reads tests/golden only."""
import json
import os
import subprocess
import sys

import pytest
import torch

from supir_amd import ops
from supir_amd import weights as Wt
from tests import tilevae_fast_support as S
from tests.helpers import build_vae, golden, rel_l2, synth_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONFAST = {"dec_40x32_t8": "tiled_dec_40x32_t8", "enc_192x160_t64": "tiled_enc_192x160_t64"}


@pytest.fixture(scope="module")
def vae():
    return build_vae(DEV)


def _bar(fx, case):
    """F's bar: 1.5 x the reference's OWN bf16-autocast distance from its fp32 result on this input (50 % for the different accumulation
    order of the HIP kernels) -- the construction of tests/test_parity_production_gpu.py."""
    return 1.5 * rel_l2(fx["bf16_" + case], fx["fast_" + case])


def _gnstats_report(hook, x, want):
    """Distance per GroupNorm of the estimate's statistics from the reference's (printed when an output misses its bar)."""
    with torch.no_grad():
        got = hook.estimate_group_norm(x.float().contiguous())
    return [f"gn{i}: mean {float((g[..., 0].cpu() - w[..., 0]).abs().max()):.2e} var rel {rel_l2(g[..., 1], w[..., 1]):.2e}"
            for i, (g, w) in enumerate(zip(got, want))]


@pytest.fixture(scope="module")
def bf16_outputs(vae):
    out = {}
    with torch.no_grad():
        for case in ("dec_40x32_t8", "enc_192x160_t64", "enc_cf_192x160_t64"):
            hook, x = S.make_hook(vae, case, DEV)
            out[case] = hook(x).float().cpu()
    return out


@pytest.mark.parametrize("case", ["dec_40x32_t8", "enc_192x160_t64", "enc_cf_192x160_t64"])
def test_bf16_fast_modes_vs_reference_fixture(vae, bf16_outputs, case):
    """F: the bf16 HIP path vs the reference's fp32 result, within 1.5 x the reference's own bf16 distance."""
    fx = S.load_fixture()
    err, bar = rel_l2(bf16_outputs[case], fx["fast_" + case]), _bar(fx, case)
    print(f"[tilevae_fast] F {case}: rel-L2 {err:.3e}  bar {bar:.3e}  (reference bf16 autocast {bar / 1.5:.3e})")
    if err > bar:
        hook, x = S.make_hook(vae, case, DEV)
        print("\n".join(_gnstats_report(hook, x, fx["gnstats_" + case])))
    assert bf16_outputs[case].shape == fx["fast_" + case].shape and torch.isfinite(bf16_outputs[case]).all()
    assert err <= bar, (case, err, bar)


def test_bf16_modes_are_told_apart(bf16_outputs):
    """G: fast decoder / encoder farther than 3 x their bar from the NON-fast goldens, color_fix farther than 3 x its bar from plain fast."""
    fx, g = S.load_fixture(), golden()
    for case, key in NONFAST.items():
        d, bar = rel_l2(bf16_outputs[case], g[key]), _bar(fx, case)
        print(f"[tilevae_fast] G {case} vs non-fast golden: {d:.3e}  (3 x bar = {3 * bar:.3e})")
        assert d > 3 * bar, (case, d, bar)
    d, bar = rel_l2(bf16_outputs["enc_cf_192x160_t64"], fx["fast_enc_192x160_t64"]), _bar(fx, "enc_cf_192x160_t64")
    print(f"[tilevae_fast] G enc_cf vs plain fast fixture: {d:.3e}  (3 x bar = {3 * bar:.3e})")
    assert d > 3 * bar, (d, bar)


@pytest.mark.parametrize("case", ["dec_40x32_t8", "enc_192x160_t64", "enc_cf_192x160_t64", "dec_n2_44x36_t8"])
def test_fp32_service_fast_modes_vs_reference_fixture(vae, case):
    """H: `--ae_dtype fp32` -- at the bar tests/test_fp32_gpu.py::test_tiled_vae_fp32_vs_oracle holds the non-fast tiled VAE to (1e-5)."""
    fx = S.load_fixture()
    hook, x = S.make_hook(vae, case, DEV)
    with torch.no_grad(), Wt.compute_dtype(torch.float32):
        out = hook(x)
    err = rel_l2(out, fx["fast_" + case])
    print(f"[tilevae_fast] H fp32 {case}: rel-L2 {err:.3e}")
    assert out.dtype == torch.float32 and err <= 1e-5, (case, err)


def test_moments_and_downsample_kernels_vs_torch():
    """I: supir_image_moments vs torch in float64 (<= 1e-6 relative), supir_downsample_nearest_exact_affine vs the torch expression of
    tilevae.py:860-872 (<= 1e-6 relative; the gathered pixels exact) on a (2, 3, 1088, 1920) image at tile 512."""
    import torch.nn.functional as F
    from supir_amd.utils.tilevae import nearest_exact_index
    x = (synth_tensor("fast.img", (2, 3, 1088, 1920), scale=0.5) + torch.tensor([0.3, -0.2, 0.05]).view(1, 3, 1, 1)).to(DEV).contiguous()
    s = 512 / 1920
    iy, ix = nearest_exact_index(1088, s), nearest_exact_index(1920, s)
    mo, mn = ops.image_moments(x), ops.image_moments(x, iy, ix)
    small = F.interpolate(x, scale_factor=s, mode="nearest-exact")
    assert tuple(small.shape[2:]) == (iy.numel(), ix.numel())
    worst = 0.0
    for m, ref in ((mo, x), (mn, small)):
        r, n = ref.double(), ref.numel() // 3
        std, mean = torch.std_mean(r, dim=[0, 2, 3])
        got_mean = m[:, 0] / n
        got_std = torch.sqrt((m[:, 1] - m[:, 0] * got_mean) / (n - 1))
        worst = max(worst, float(((got_mean - mean).abs() / mean.abs()).max()), float(((got_std - std).abs() / std).max()))
        assert float(m[:, 2].min()) == float(r.min()) and float(m[:, 3].max()) == float(r.max())
        assert torch.equal(m[:, 2], r.amin(dim=(0, 2, 3))) and torch.equal(m[:, 3], r.amax(dim=(0, 2, 3)))
    print(f"[tilevae_fast] I moments: worst relative error of mean / std {worst:.3e}")
    assert worst <= 1e-6
    out = ops.downsample_nearest_exact_affine(x, iy, ix, mo, mn)
    std_old, mean_old = torch.std_mean(x, dim=[0, 2, 3], keepdim=True)
    std_new, mean_new = torch.std_mean(small, dim=[0, 2, 3], keepdim=True)
    ref = torch.clamp((small - mean_new) / std_new * std_old + mean_old, min=x.min(), max=x.max())
    err = rel_l2(out, ref)
    print(f"[tilevae_fast] I down-sample + repair: rel-L2 {err:.3e}")
    assert out.shape == ref.shape and err <= 1e-6
    # indices exact: on channels holding their own row / column number a wrong source pixel is off by >= 1 x (std_old / std_new ~ 1),
    # the arithmetic by ~1e-4
    yy = torch.arange(1088, dtype=torch.float32, device=DEV).view(1, 1, 1088, 1).expand(1, 1, 1088, 1920)
    xx = torch.arange(1920, dtype=torch.float32, device=DEV).view(1, 1, 1, 1920).expand(1, 1, 1088, 1920)
    pos = torch.cat([yy, xx], dim=1).contiguous()
    picked = ops.downsample_nearest_exact_affine(pos, iy, ix, ops.image_moments(pos), ops.image_moments(pos, iy, ix))
    psmall = F.interpolate(pos, scale_factor=s, mode="nearest-exact")
    assert torch.equal(psmall[0, 0, :, 0].to(torch.int32).cpu(), iy) and torch.equal(psmall[0, 1, 0].to(torch.int32).cpu(), ix)
    so, mo_ = torch.std_mean(pos, dim=[0, 2, 3], keepdim=True)
    sn, mn_ = torch.std_mean(psmall, dim=[0, 2, 3], keepdim=True)
    worst_px = float((picked - torch.clamp((psmall - mn_) / sn * so + mo_, min=pos.min(), max=pos.max())).abs().max())
    print(f"[tilevae_fast] I position channels: worst pixel error {worst_px:.3e}")
    assert worst_px < 0.25


@pytest.mark.parametrize("which", ["enc_2048", "dec_256"])
def test_tile_chunk_bounds_memory_and_keeps_the_result(vae, which, monkeypatch):
    """J: tile_chunk 1 / 4 / all.  With the tile picks frozen (no autotune) a chunk that keeps every stack whole is bitwise the
    un-chunked run.  Smaller chunks change the batch of each launch, and the convolution / attention kernels choose their tile and key
    split by the size of the launch (another fp32 accumulation order under the same bf16 rounding), so there equality is up to that
    rounding: half the reference's own bf16 distance on the fixture of the same net -- the share the F bar grants to "a different
    accumulation order".  Peak memory with tile_chunk=1 must be strictly below the un-chunked run: that is what the option is for."""
    from supir_amd.utils.tilevae import VAEHook
    # frozen picks = the packaged ones every process starts from, nothing an earlier test of this session happened to time (with
    # those left in, the chunked decoder came out at 1.04e-2 run on its own and 1.16e-2 after the rest of the suite; bound 1.08e-2)
    ops._check_packaged_tune()
    monkeypatch.setattr(ops, "AUTOTUNE", False)
    monkeypatch.setattr(ops, "_TUNE", {k: v for k, v in ops._TUNE.items() if k in ops._PACKAGED[0]})
    monkeypatch.setattr(ops, "_CHOICE", {k: v for k, v in ops._CHOICE.items() if k in ops._PACKAGED[1]})
    fx = S.load_fixture()
    if which == "enc_2048":
        net, tile, dec, kw = vae.denoise_encoder, 512, False, dict(fast_encoder=True)
        x = synth_tensor("fast.img2048", (1, 3, 2048, 2048), scale=0.5).to(DEV)
        bound = 0.5 * rel_l2(fx["bf16_enc_192x160_t64"], fx["fast_enc_192x160_t64"])
    else:
        net, tile, dec, kw = vae.decoder, 64, True, dict(fast_decoder=True)
        x = synth_tensor("fast.z256", (1, 4, 256, 256)).to(DEV)
        bound = 0.5 * rel_l2(fx["bf16_dec_40x32_t8"], fx["fast_dec_40x32_t8"])
    if not hasattr(net, "original_forward"):
        net.original_forward = net.forward

    def run(chunk):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        with torch.no_grad():
            out = VAEHook(net, tile, is_decoder=dec, tile_chunk=chunk, **kw)(x)
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated()

    run(None)                                   # warm: workspaces and derived weights exist before anything is measured
    want, peak_all = run(None)
    whole, _ = run(10 ** 6)
    assert torch.isfinite(want).all() and torch.equal(whole, want)
    for k in (1, 4):
        got, peak = run(k)
        err = rel_l2(got, want)
        print(f"[tilevae_fast] J {which}: tile_chunk={k} rel-L2 vs all tiles {err:.3e} (bound {bound:.3e}), peak {peak / 2**20:.0f} MiB vs {peak_all / 2**20:.0f} MiB")
        assert err <= bound, (which, k, err, bound)
        if k == 1:
            assert peak < peak_all, (peak, peak_all)


def test_fast_mode_tile_parallel_under_a_one_rank_nccl_group():
    """K: fast mode with tile_parallel=True through RCCL (one rank, collectives forced) is bitwise the serial result; plain fast mode
    issues ONE collective (the canvas), color_fix additionally one per pooled GroupNorm."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rccl_tilevae_fast_worker.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RCCL_RESULT ")]
    assert p.returncode == 0 and line, p.stdout[-2000:] + "\n" + p.stderr[-4000:]
    r = json.loads(line[-1][len("RCCL_RESULT "):])
    print(r)
    assert r["backend"] == "nccl"
    assert r["dec_equal"] and r["enc_equal"] and r["enc_cf_equal"] and r["dec_chunk_equal"]
    assert r["dec_collectives"] == 1 and r["enc_collectives"] == 1 and r["dec_chunk_collectives"] == 1
    assert r["enc_cf_collectives"] == 1 + r["enc_cf_pooled_norms"] and r["enc_cf_pooled_norms"] > 0
