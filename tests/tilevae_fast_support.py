"""TEST-ONLY support for the fast mode of the tiled VAE: the fixture loader (tests/golden/golden_tilevae_fast.pt.NN, recorded from the
reference by tools/gen_golden_tilevae_fast.py) and plain-torch stand-ins for the ops fast mode adds (ops.image_moments,
ops.downsample_nearest_exact_affine, ops.groupnorm_mean_var) on top of tests/torch_ops.py, so the HOST logic of
supir_amd/utils/tilevae.py runs on a CPU.  Never imported by the product."""
import contextlib
import glob
import io
import os

import torch

from tests.helpers import GOLDEN_DIR

_fix = {}


def load_fixture():
    """The torch.save stream is committed in pieces below the per-file size limit; joined here."""
    if "f" not in _fix:
        parts = sorted(glob.glob(os.path.join(GOLDEN_DIR, "golden_tilevae_fast.pt.*")))
        assert parts, "tests/golden/golden_tilevae_fast.pt.* missing"
        data = b"".join(open(p, "rb").read() for p in parts)
        _fix["f"] = torch.load(io.BytesIO(data), map_location="cpu", weights_only=False)
    return _fix["f"]


CASES = {"dec_40x32_t8": dict(net="decoder", tile=8, input=("z_tiled", (1, 4, 40, 32), 1.0), is_decoder=True, fast_decoder=True),
         "enc_192x160_t64": dict(net="denoise_encoder", tile=64, input=("img_tiled", (1, 3, 192, 160), 0.5), is_decoder=False,
                                 fast_encoder=True),
         "enc_cf_192x160_t64": dict(net="denoise_encoder", tile=64, input=("img_tiled", (1, 3, 192, 160), 0.5), is_decoder=False,
                                    fast_encoder=True, color_fix=True),
         "dec_n2_44x36_t8": dict(net="decoder", tile=8, input=("z_tiled_n2", (2, 4, 44, 36), 1.0), is_decoder=True, fast_decoder=True)}


def make_hook(vae, case, device="cpu", **extra):
    """(VAEHook of the case, its input) on `device`."""
    from supir_amd.utils.tilevae import VAEHook
    from tests.helpers import synth_tensor
    c = CASES[case]
    net = getattr(vae, c["net"])
    if not hasattr(net, "original_forward"):
        net.original_forward = net.forward
    name, shape, scale = c["input"]
    kw = {k: c[k] for k in ("fast_decoder", "fast_encoder", "color_fix") if k in c}
    kw.update(extra)
    return VAEHook(net, c["tile"], is_decoder=c["is_decoder"], **kw), synth_tensor(name, shape, scale=scale).to(device)


# ------------------------------------------------------------------------------------------------ torch stand-ins
def image_moments(x, iy=None, ix=None):
    v = x.double()
    if iy is not None:
        v = v[:, :, torch.as_tensor(iy).long()][:, :, :, torch.as_tensor(ix).long()]
    return torch.stack([v.sum(dim=(0, 2, 3)), (v * v).sum(dim=(0, 2, 3)), v.amin(dim=(0, 2, 3)), v.amax(dim=(0, 2, 3))], dim=-1)


def _mean_std(mom, n):
    mean = mom[:, 0] / n
    return mean.float(), torch.sqrt((mom[:, 1] - mom[:, 0] * mean).clamp_min(0.0) / (n - 1)).float()


def downsample_nearest_exact_affine(x, iy, ix, mom_old, mom_new):
    g = x[:, :, torch.as_tensor(iy).long()][:, :, :, torch.as_tensor(ix).long()]
    mo, so = _mean_std(mom_old, x.numel() // x.shape[1])
    mn, sn = _mean_std(mom_new, g.numel() // g.shape[1])
    v = lambda t: t.view(1, -1, 1, 1)
    out = (g - v(mn)) / v(sn) * v(so) + v(mo)
    return out.clamp_(min=float(mom_old[:, 2].min()), max=float(mom_old[:, 3].max()))


def groupnorm_mean_var(x):
    B, C = x.shape[0], x.shape[-1]
    n = float(x[0].numel() // 32)
    g = x.double().reshape(B, -1, 32, C // 32)
    s = torch.stack([g.sum(dim=(1, 3)), (g * g).sum(dim=(1, 3))], dim=-1)
    mean = s[..., 0] / n
    return torch.stack([mean, (s[..., 1] / n - mean * mean).clamp_min(0.0)], dim=-1).float()


@contextlib.contextmanager
def installed(fp32=True):
    """tests/torch_ops.installed() with the three fast-mode entry points swapped in as well."""
    from supir_amd import ops as real_ops
    from tests import torch_ops
    names = ("image_moments", "downsample_nearest_exact_affine", "groupnorm_mean_var")
    saved = {n: getattr(real_ops, n) for n in names}
    with torch_ops.installed(fp32=fp32) as be:
        try:
            for n in names:
                setattr(real_ops, n, globals()[n])
            yield be
        finally:
            for n, v in saved.items():
                setattr(real_ops, n, v)
