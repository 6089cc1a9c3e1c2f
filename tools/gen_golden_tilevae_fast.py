"""Record tests/golden/golden_tilevae_fast.pt: the REFERENCE's own VAEHook (SUPIR/utils/tilevae.py) in fast mode, CPU fp32, on
supir_amd.synth weights and inputs -- what tests/test_tilevae_fast_*.py hold supir_amd/utils/tilevae.py to.

Needs the reference checkout (oracle/ref_import.py finds it); nothing of it is copied, only what its programs compute is stored:

  fast_dec_40x32_t8        decoder, tile 8, fast_decoder=True, synth "z_tiled" (1, 4, 40, 32)
  fast_enc_192x160_t64     denoise encoder, tile 64, fast_encoder=True, synth "img_tiled" (1, 3, 192, 160) * 0.5
  fast_enc_cf_192x160_t64  the same with color_fix=True
  fast_dec_n2_44x36_t8     decoder, tile 8, synth "z_tiled_n2" (2, 4, 44, 36): batch of two, ragged tile grid
  small_<case>             the repaired down-sampled tensor the estimate ran on (argument of estimate_group_norm)
  gnstats_<case>           [n_groupnorms, N, 32, 2] = (mean, biased variance) the estimate recorded, in network order (the defaults
                           of the `apply_norm` closures it left in the task queue)
  bf16_<case>              the first three outputs with the reference under torch.autocast("cpu", torch.bfloat16)
  meta                     relative L2 distances between the modes (what the GPU tests derive their bars from), torch version

No committed file may exceed 1 MiB, so the torch.save stream is written in pieces golden_tilevae_fast.pt.00, .01, ...;
tests/tilevae_fast_support.py::load_fixture() joins them.

    python tools/gen_golden_tilevae_fast.py
"""
import glob
import io
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import as R  # noqa: E402
from supir_amd.synth import fill_state_dict_, synth_tensor  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
NAME = "golden_tilevae_fast.pt"
PIECE = 960 * 1024


def rel_l2(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-20)).item()


def fill(module, prefix):
    fill_state_dict_({prefix + k: v for k, v in module.state_dict().items()})
    return module


def prepare_reference():
    """The reference's tiled VAE on CPU: an SDPA-backed `xformers`, its device module pointed at the CPU."""
    ns = R.load_reference()
    xf = types.ModuleType("xformers")
    xf.ops = types.ModuleType("xformers.ops")

    def mea(q, k, v, attn_bias=None, op=None):     # [B * heads, T, D]: what xformers' memory_efficient_attention computes
        return torch.nn.functional.scaled_dot_product_attention(q[:, None], k[:, None], v[:, None])[:, 0]

    xf.ops.memory_efficient_attention = mea
    sys.modules["xformers"], sys.modules["xformers.ops"] = xf, xf.ops
    from SUPIR.utils import devices
    devices.device = torch.device("cpu")
    devices.get_optimal_device = lambda: torch.device("cpu")
    from SUPIR.utils import tilevae as TV
    TV.xformers = xf
    TV.devices.device = torch.device("cpu")
    _, _, vae = R.unet_params()
    with R.quiet():
        denc = ns.Encoder(**vae).eval()
        dec = ns.Decoder(**vae).eval()
    fill(denc, "first_stage_model.denoise_encoder.")
    fill(dec, "first_stage_model.decoder.")
    for net in (denc, dec):
        net.original_forward = net.forward
        net.mid.attn_1.attention_op = None
    return TV, denc, dec


def run(TV, net, tile, x, *, is_decoder, fast, color_fix=False, autocast=False):
    """One hook call; returns (output, small, gnstats) -- the last two None when fast mode is off."""
    hook = TV.VAEHook(net, tile, is_decoder=is_decoder, fast_decoder=fast and is_decoder, fast_encoder=fast and not is_decoder,
                      color_fix=color_fix, to_gpu=False)
    seen = {}
    inner = hook.estimate_group_norm

    def spy(z, task_queue, color_fix):
        seen["small"] = z.detach().clone()
        ok = inner(z, task_queue, color_fix=color_fix)
        stats = []
        for task in task_queue:
            if task[0] == "apply_norm":
                mean, var = task[1].__defaults__[:2]
                n = z.shape[0]
                stats.append(torch.stack([mean.float().reshape(n, 32), var.float().reshape(n, 32)], dim=-1))
        seen["gnstats"], seen["ok"] = torch.stack(stats), ok
        return ok

    hook.estimate_group_norm = spy
    with R.quiet(), torch.no_grad(), torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        out = hook(x).clone()
    if fast:
        assert seen["ok"], "the reference's estimate fell back to the non-fast path"
    return out.float(), seen.get("small"), seen.get("gnstats")


def main():
    torch.manual_seed(0)
    TV, denc, dec = prepare_reference()
    z_t = synth_tensor("z_tiled", (1, 4, 40, 32), scale=1.0)
    img_t = synth_tensor("img_tiled", (1, 3, 192, 160), scale=0.5)
    z_n2 = synth_tensor("z_tiled_n2", (2, 4, 44, 36), scale=1.0)
    cases = {"dec_40x32_t8": (dec, 8, z_t, dict(is_decoder=True)),
             "enc_192x160_t64": (denc, 64, img_t, dict(is_decoder=False)),
             "enc_cf_192x160_t64": (denc, 64, img_t, dict(is_decoder=False, color_fix=True)),
             "dec_n2_44x36_t8": (dec, 8, z_n2, dict(is_decoder=True))}
    gold = {}
    for name, (net, tile, x, kw) in cases.items():
        out, small, stats = run(TV, net, tile, x, fast=True, **kw)
        gold["fast_" + name], gold["small_" + name], gold["gnstats_" + name] = out, small, stats
        print(name, tuple(out.shape), "small", tuple(small.shape), "groupnorms", stats.shape[0], flush=True)
        if name != "dec_n2_44x36_t8":
            b, _, _ = run(TV, net, tile, x, fast=True, autocast=True, **kw)
            # the canvas is fp32 but what is pasted into it came out of a bf16 convolution: bf16 storage is lossless then
            gold["bf16_" + name] = b.bfloat16() if torch.equal(b.bfloat16().float(), b) else b
    nonfast_dec, _, _ = run(TV, dec, 8, z_t, is_decoder=True, fast=False)
    nonfast_enc, _, _ = run(TV, denc, 64, img_t, is_decoder=False, fast=False)
    mini = torch.load(os.path.join(OUT, "golden_mini.pt"), map_location="cpu", weights_only=False)
    assert rel_l2(nonfast_dec, mini["tiled_dec_40x32_t8"]) <= 1e-6 and rel_l2(nonfast_enc, mini["tiled_enc_192x160_t64"]) <= 1e-6
    gold["meta"] = dict(
        torch=torch.__version__,
        note="the reference's VAEHook in fast mode (CPU fp32) on supir_amd.synth inputs / weights; rel_l2(a, b) = |a - b| / |b|",
        rel_l2={"dec_fast_vs_nonfast": rel_l2(gold["fast_dec_40x32_t8"], nonfast_dec),
                "enc_fast_vs_nonfast": rel_l2(gold["fast_enc_192x160_t64"], nonfast_enc),
                "enc_cf_vs_nonfast": rel_l2(gold["fast_enc_cf_192x160_t64"], nonfast_enc),
                "enc_cf_vs_fast": rel_l2(gold["fast_enc_cf_192x160_t64"], gold["fast_enc_192x160_t64"]),
                "bf16_dec_40x32_t8": rel_l2(gold["bf16_dec_40x32_t8"], gold["fast_dec_40x32_t8"]),
                "bf16_enc_192x160_t64": rel_l2(gold["bf16_enc_192x160_t64"], gold["fast_enc_192x160_t64"]),
                "bf16_enc_cf_192x160_t64": rel_l2(gold["bf16_enc_cf_192x160_t64"], gold["fast_enc_cf_192x160_t64"])})
    for k, v in gold["meta"]["rel_l2"].items():
        print(f"  {k}: {v:.3e}")
    buf = io.BytesIO()
    torch.save(gold, buf)
    data = buf.getvalue()
    for old in glob.glob(os.path.join(OUT, NAME + ".*")):
        os.remove(old)
    for i in range(0, len(data), PIECE):
        with open(os.path.join(OUT, f"{NAME}.{i // PIECE:02d}"), "wb") as f:
            f.write(data[i:i + PIECE])
    print("wrote", NAME, len(data) / 1e6, "MB in", (len(data) + PIECE - 1) // PIECE, "pieces")


if __name__ == "__main__":
    main()
