"""SUPIRModel: the unit of work of the metric (`batchify_sample`), same constructor kwargs / methods / attribute protocol
as SUPIR/models/SUPIR_model.py:12-179 (+ the DiffusionEngine constructor subset it relies on, sgm/models/diffusion.py:23-83).

The text conditioner (CLIP-L + OpenCLIP-bigG, once per image) is built from `conditioner_config` like the
reference does (supir_amd/modules/conditioner.py: both towers on the HIP kernels).  `conditioner_config` may also be None:
`batchify_sample(..., cond=(c, uc))` takes prepared `crossattn [N,77,2048]` / `vector [N,2816]` tensors directly (what bench.py
does: synthetic conditioning, no tokeniser vocabulary files in this image), or a `conditioner` object with the reference's
`get_unconditional_conditioning(batch, batch_uc)` method can be attached.
"""
import contextlib
import copy
import os
import random

import torch
import torch.nn as nn

from .. import weights as Wt
from ..modules.vae import DiagonalGaussianDistribution
from ..plugin import get_obj_from_str, instantiate_from_config

_DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def seed_everything(seed):
    """pytorch_lightning.seed_everything: python / numpy / torch global RNGs (SUPIR_model.py:115)."""
    import numpy as np
    random.seed(seed)
    np.random.seed(seed % (2 ** 32))
    torch.manual_seed(seed)
    return seed


def _cfg_set(cfg, path, value):
    node = cfg
    for k in path[:-1]:
        node = node[k]
    node[path[-1]] = value


class SUPIRModel(nn.Module):
    def __init__(self, control_stage_config, network_config, denoiser_config, first_stage_config, sampler_config,
                 conditioner_config=None, ae_dtype="fp32", diffusion_dtype="fp32", p_p="", n_p="", scale_factor=1.0,
                 disable_first_stage_autocast=False, network_wrapper=None, **kwargs):
        super().__init__()
        net = instantiate_from_config(network_config)
        wrapper = get_obj_from_str(network_wrapper or "sgm.modules.diffusionmodules.wrappers.ControlWrapper")
        self.model = wrapper(net)
        self.denoiser = instantiate_from_config(denoiser_config)
        self.sampler = instantiate_from_config(sampler_config) if sampler_config is not None else None
        self.conditioner = instantiate_from_config(conditioner_config) if conditioner_config is not None else None
        self.first_stage_model = instantiate_from_config(first_stage_config).eval()
        self.scale_factor = scale_factor
        self.model.load_control_model(instantiate_from_config(control_stage_config))
        self.first_stage_model.denoise_encoder = copy.deepcopy(self.first_stage_model.encoder)
        self.sampler_config = copy.deepcopy(sampler_config)
        assert ae_dtype in _DT and diffusion_dtype in _DT
        if ae_dtype == "fp16":
            raise RuntimeError("fp16 cause NaN in AE")  # SUPIR_model.py:23-24
        self.ae_dtype = _DT[ae_dtype]
        self.model.dtype = _DT[diffusion_dtype]
        self.p_p, self.n_p = p_p, n_p
        # long prompts (modules/conditioner.py): at most this many 75-token chunks per prompt; 1 = the reference's truncation at 77
        # tokens.  SUPIR_PROMPT_CHUNKS sets the default for callers that cannot pass the keyword (the reference's own test.py).
        self.prompt_chunks = int(os.environ.get("SUPIR_PROMPT_CHUNKS", "1"))
        if self.prompt_chunks < 1:
            raise ValueError(f"SUPIR_PROMPT_CHUNKS must be >= 1, got {self.prompt_chunks}")
        self._ae_dtype_noted = None

    # ------------------------------------------------------------------ first stage
    @contextlib.contextmanager
    def _ae_scope(self):
        """The reference runs the three VAE entry points under `torch.autocast("cuda", dtype=self.ae_dtype)` (SUPIR_model.py:41-69;
        `model.ae_dtype = ...` is part of test.py's attribute protocol, test.py:67).  Here `ae_dtype` selects the element type of
        the VAE kernels for the call: torch.bfloat16 (test.py's default) -> bf16, the reference's own arithmetic for that request.
        torch.float32 (`--ae_dtype fp32`) is computed by the reference in TRUE fp32 (autocast disables itself for float32) -> the fp32
        service (libsupir_hip_f32.so, supir_amd/ops_f32.py); with weights.FP32_NATIVE off (SUPIR_FP32_NATIVE=0) it is served in bf16 --
        said once per request with a RuntimeWarning, a RuntimeError under SUPIR_STRICT_DTYPE=1.  torch.float16 is refused like the
        reference's constructor refuses it (SUPIR_model.py:23-24)."""
        dt = self.ae_dtype
        if dt == torch.float16:
            raise RuntimeError("fp16 cause NaN in AE")
        served = Wt.as_compute_dtype(dt)
        if served != dt and dt != torch.bfloat16 and self._ae_dtype_noted != dt:
            self._ae_dtype_noted = dt
            Wt.note_downgrade("SUPIRModel.ae_dtype", f"{dt} (test.py --ae_dtype fp32)", "torch.bfloat16",
                              "the reference computes this request in true fp32 (torch.autocast disables itself for float32, "
                              "SUPIR/models/SUPIR_model.py:41-69); SUPIR_FP32_NATIVE=0 keeps fp32 requests off the fp32 service "
                              "(decoder rel-L2 vs fp32 ~1e-2 at 512 px).", stacklevel=5)
        with Wt.compute_dtype(served):
            yield

    @torch.no_grad()
    def encode_first_stage(self, x, noise=None):
        fs = self.first_stage_model
        with self._ae_scope():
            post = DiagonalGaussianDistribution(fs.quant_conv(fs.encoder(x)))
            return self.scale_factor * post.sample(noise)

    @torch.no_grad()
    def encode_first_stage_with_denoise(self, x, use_sample=True, is_stage1=False, noise=None):
        fs = self.first_stage_model
        with self._ae_scope():
            h = fs.denoise_encoder_s1(x) if is_stage1 else fs.denoise_encoder(x)
            post = DiagonalGaussianDistribution(fs.quant_conv(h))
            z = post.sample(noise) if use_sample else post.mode()
            return self.scale_factor * z

    @torch.no_grad()
    def decode_first_stage(self, z):
        fs = self.first_stage_model
        with self._ae_scope():
            return fs.decoder(fs.post_quant_conv(z, in_scale=1.0 / self.scale_factor)).float()

    @torch.no_grad()
    def batchify_denoise(self, x, is_stage1=False):
        return self.decode_first_stage(self.encode_first_stage_with_denoise(x, use_sample=False, is_stage1=is_stage1))

    # ------------------------------------------------------------------ the unit of work
    @torch.no_grad()
    def batchify_sample(self, x, p=None, p_p="default", n_p="default", num_steps=100, restoration_scale=4.0, s_churn=0,
                        s_noise=1.003, cfg_scale=4.0, seed=-1, num_samples=1, control_scale=1, color_fix_type="None",
                        use_linear_CFG=False, use_linear_control_scale=False, cfg_scale_start=1.0,
                        control_scale_start=0.0, cond=None, noises=None, return_intermediates=False, prompt_chunks=None,
                        regions=None, region_weights=None, region_feather=None, **kwargs):
        """SUPIR_model.py:80-136.  `cond=(c, uc)` bypasses the text conditioner (a `crossattn` longer than 77 tokens, e.g. the
        [N, 154, 2048] of a two-chunk prompt, needs nothing else: every layer below takes the token count from the tensor);
        `prompt_chunks` (None: self.prompt_chunks) lets prompts use up to that many 75-token chunks instead of being cut at 77 tokens
        (prepare_condition); prompts are strings or token-id tensors [N, 77 n]; `noises` (dict with optional
        'posterior', 'init', 'steps') injects the RNG draws for parity runs (otherwise the sampler's churn noise comes from
        torch.randn_like on the device generator exactly like the reference).

        `regions` (untiled samplers): a prompt per REGION of one image, in one untiled network call -- `p = [[p_0 ... p_{R-1}]]` (the
        local-prompt form, batch size 1 as in the reference; num_samples > 1 repeats the map) or `cond=([c_0 ... c_{R-1}], uc)`, and
        `regions` an integer map [h, w] on the latent grid with values in [0, R), or R latent boxes (h0, h1, w0, w1), later boxes over
        earlier ones, covering every pixel (sampling.region_map; sampling.regions_from_tiles gives the partition that matches the tiled
        samplers' windows).  Every text cross-attention restricts each token to its region's prompt; the pooled `vector`, the control
        hint and the scales are global and come from region 0's conditioning.

        Soft region weights (same prompts, same samplers, still one network call): `region_weights` = a float tensor / array [R, h, w]
        on the latent grid, >= 0, normalised per pixel (sampling.region_weights; sampling.region_weights_from_tiles gives the tiled
        samplers' Gaussian blend weights), used WITHOUT `regions`; or `regions=map_or_boxes, region_feather=k`, the (2k + 1)^2 box
        filter over the hard map (sampling.feather_regions; k = 0: the hard map as one-hot weights).  Every text cross-attention then
        outputs the weighted sum over the regions of the token's attention to each region's prompt."""
        assert color_fix_type in ["Wavelet", "AdaIn", "None"]
        N = len(x)
        if num_samples > 1:
            assert N == 1
            N = num_samples
            x = x.repeat(N, 1, 1, 1)
            if p is not None and regions is None and region_weights is None:
                p = p.repeat(N, 1) if torch.is_tensor(p) else p * N
        p_p = self.p_p if p_p == "default" else p_p
        n_p = self.n_p if n_p == "default" else n_p
        sc = self.sampler_config
        _cfg_set(sc, ("params", "num_steps"), num_steps)
        _cfg_set(sc, ("params", "guider_config", "params", "scale_min"), cfg_scale)
        _cfg_set(sc, ("params", "guider_config", "params", "scale"), cfg_scale_start if use_linear_CFG else cfg_scale)
        _cfg_set(sc, ("params", "restore_cfg"), restoration_scale)
        _cfg_set(sc, ("params", "s_churn"), s_churn)
        _cfg_set(sc, ("params", "s_noise"), s_noise)
        self.sampler = instantiate_from_config(sc)
        if seed == -1:
            seed = random.randint(0, 65535)
        seed_everything(seed)
        noises = noises or {}
        _z = self.encode_first_stage_with_denoise(x, use_sample=False)
        x_stage1 = self.decode_first_stage(_z)
        z_stage1 = self.encode_first_stage(x_stage1, noise=noises.get("posterior"))
        if region_feather is not None and regions is None:
            raise ValueError("`region_feather` softens a hard map: it needs `regions`")
        if region_weights is not None and regions is not None:
            raise ValueError("regional prompts take `regions` (with `region_feather` to soften them) or `region_weights`, not both")
        if region_feather is not None and int(region_feather) < 0:
            raise ValueError(f"`region_feather` is {region_feather}: the radius cannot be negative")
        regional = regions is not None or region_weights is not None
        if cond is None and not regional:
            assert len(x) == len(p)   # SUPIR_model.py:95
        if regional:
            # a prompt per region, one untiled network call (see the docstring)
            c, uc, regions, region_weights = self._regional_condition(_z, p, p_p, n_p, N, cond, regions, prompt_chunks, region_weights,
                                                                      region_feather)
        elif cond is not None:
            # (c a list: per-tile conditionings, as prepare_condition returns them for local prompts)
            c = [dict(cj, control=_z) for cj in cond[0]] if isinstance(cond[0], (list, tuple)) else dict(cond[0], control=_z)
            uc = dict(cond[1], control=_z)
        else:
            c, uc = self.prepare_condition(_z, p, p_p, n_p, N, prompt_chunks=prompt_chunks)
        denoiser = lambda inp, sigma, cc, cs: self.denoiser(self.model, inp, sigma, cc, cs, **kwargs)
        if not kwargs:   # lets RestoreEDMSampler fuse the elementwise halves of a step around the network call (sampling.py)
            denoiser.fused = (self.denoiser, self.model)
        noised_z = noises["init"].to(_z).clone() if "init" in noises else torch.randn_like(_z)
        if "steps" in noises:   # parity runs: per-step churn noise instead of torch.randn_like (RestoreEDMSampler only)
            self.sampler.injected_step_noises = list(noises["steps"])
        _samples = self.sampler(denoiser, noised_z, cond=c, uc=uc, x_center=z_stage1, control_scale=control_scale,
                                use_linear_control_scale=use_linear_control_scale, control_scale_start=control_scale_start,
                                **({} if regions is None else {"regions": regions}),
                                **({} if region_weights is None else {"region_weights": region_weights}))
        samples = self.decode_first_stage(_samples)
        if color_fix_type == "Wavelet":
            from ..utils.colorfix import wavelet_reconstruction
            samples = wavelet_reconstruction(samples, x_stage1)
        elif color_fix_type == "AdaIn":
            from ..utils.colorfix import adaptive_instance_normalization
            samples = adaptive_instance_normalization(samples, x_stage1)
        if return_intermediates:
            return samples, dict(z=_z, x_stage1=x_stage1, z_stage1=z_stage1, samples=_samples)
        return samples

    def _regional_condition(self, _z, p, p_p, n_p, N, cond, regions, prompt_chunks, region_weights=None, region_feather=None):
        """batchify_sample(regions=...): the per-region conditionings (c_0 ... c_{R-1}), uc, the checked [h, w] map and None -- or, with
        `region_weights` or `region_feather`, None and the checked soft weights [R, h, w].  The prompts are those of ONE image
        (`p = [[...]]` or `cond=([...], uc)`); with num_samples = N their rows are repeated N times."""
        from ..modules import sampling
        if isinstance(self.sampler, sampling._TileGroups):
            raise ValueError("the tiled samplers take per-tile prompts (their windows are the regions), not `regions`")

        def rows(t):
            return t if (not torch.is_tensor(t) or t.shape[0] == N) else t[:1].repeat(N, *([1] * (t.dim() - 1)))

        if cond is not None:
            if not isinstance(cond[0], (list, tuple)):
                raise ValueError("`regions` needs cond=([c_0 ... c_{R-1}], uc): one conditioning per region")
            c, uc = [dict(cj) for cj in cond[0]], dict(cond[1])
        else:
            if p is None or torch.is_tensor(p) or len(p) != 1 or not isinstance(p[0], (list, tuple)):
                raise ValueError("`regions` needs p = [[p_0 ... p_{R-1}]]: the prompts of the regions of one image")
            if not 1 <= len(p[0]) <= sampling.MAX_REGIONS:
                raise ValueError(f"regional prompts take 1 .. {sampling.MAX_REGIONS} regions, got {len(p[0])}")
            c, uc = self.prepare_condition(_z[:1], [list(p[0])], p_p, n_p, 1, prompt_chunks=prompt_chunks)
        m = wts = None
        if region_weights is not None:
            wts = sampling.region_weights(region_weights, len(c), _z.shape[-2], _z.shape[-1])
        else:
            m = sampling.region_map(regions, len(c), _z.shape[-2], _z.shape[-1])
            if region_feather is not None:
                m, wts = None, sampling.feather_regions(m, len(c), int(region_feather))
        c = [dict({k: rows(v) for k, v in cj.items()}, control=_z) for cj in c]
        uc = dict({k: rows(v) for k, v in uc.items()}, control=_z)
        return c, uc, m, wts

    def init_tile_vae(self, encoder_tile_size=512, decoder_tile_size=64, fast_encoder=False, fast_decoder=False, color_fix=False,
                      tile_chunk=None):
        """SUPIR_model.py:138-150: route the three VAE nets through the tiled forward (test.py --use_tile_vae).  The reference installs
        the hook with fast modes and color_fix off, and so do the defaults; the keywords are the hook's own (utils/tilevae.py).
        tile_chunk bounds the tiles in flight of the nets that run in fast mode without color_fix (the others take all tiles at once)."""
        from ..utils.tilevae import VAEHook
        fs = self.first_stage_model
        for net, size, dec in ((fs.denoise_encoder, encoder_tile_size, False), (fs.encoder, encoder_tile_size, False),
                               (fs.decoder, decoder_tile_size, True)):
            net.original_forward = net.forward
            independent = fast_decoder if dec else (fast_encoder and not color_fix)
            net.forward = VAEHook(net, size, is_decoder=dec, fast_decoder=fast_decoder, fast_encoder=fast_encoder, color_fix=color_fix,
                                  to_gpu=True, tile_chunk=tile_chunk if independent else None)

    def prepare_condition(self, _z, p, p_p, n_p, N, prompt_chunks=None):
        """SUPIR_model.py:152-180.  prompt_chunks (None: self.prompt_chunks, 1 unless SUPIR_PROMPT_CHUNKS says otherwise): a prompt
        (caption + p_p) may fill up to that many 75-token chunks, each encoded as its own 77-token sequence; c and uc -- and with
        per-tile prompts every tile's c -- come back with the same token count 77 n, n = the most any of them needs (at most
        prompt_chunks), the shorter ones ending in empty chunks.  `p` / `n_p` may be token-id tensors ([N, 77 n] / [77 m] or [N, 77 m],
        taken as they are: p_p is text and is not appended to ids)."""
        if self.conditioner is None:
            raise RuntimeError("no text conditioner attached (conditioner_config was None); pass cond=(c, uc) with "
                               "crossattn [N,77,2048] / vector [N,2816], or attach a conditioner object")
        chunks = getattr(self, "prompt_chunks", 1) if prompt_chunks is None else int(prompt_chunks)
        if chunks < 1:
            raise ValueError(f"prompt_chunks must be >= 1, got {chunks}")
        batch = {"original_size_as_tuple": torch.tensor([1024, 1024]).repeat(N, 1).to(_z.device),
                 "crop_coords_top_left": torch.tensor([0, 0]).repeat(N, 1).to(_z.device),
                 "target_size_as_tuple": torch.tensor([1024, 1024]).repeat(N, 1).to(_z.device),
                 "aesthetic_score": torch.tensor([9.0]).repeat(N, 1).to(_z.device), "control": _z}
        batch_uc = copy.deepcopy(batch)
        batch_uc["txt"] = (n_p if n_p.dim() == 2 else n_p[None].repeat(len(p), 1)) if torch.is_tensor(n_p) else [n_p for _ in p]
        cond = self.conditioner
        chunked = hasattr(cond, "prompt_chunks")
        if not chunked and chunks != 1:
            raise RuntimeError(f"prompt_chunks={chunks}: the attached conditioner ({type(cond).__name__}) does not chunk prompts")
        saved = cond.prompt_chunks if chunked else None
        if chunked:
            cond.prompt_chunks = chunks
        try:
            # the reference runs the conditioner under autocast(ae_dtype) (SUPIR_model.py:165,174): the text towers follow the VAE's
            # request -- bf16 by test.py's default, true fp32 for `--ae_dtype fp32`
            if torch.is_tensor(p) or not isinstance(p[0], list):
                batch["txt"] = p if torch.is_tensor(p) else ["".join([_p, p_p]) for _p in p]
                with self._ae_scope():
                    return cond.get_unconditional_conditioning(batch, batch_uc)
            # local (per-tile) prompts, SUPIR_model.py:168-178: one cond per tile, a single uc (the tiled samplers' `cond` list)
            assert len(p) == 1, "Support bs=1 only for local prompt conditioning."
            tiles = [dict(batch, txt=p_tile[None] if torch.is_tensor(p_tile) else ["".join([p_tile, p_p])]) for p_tile in p[0]]
            # the context bank of the tiled samplers holds one shape: every tile and the uc share one chunk count
            pad = {"pad_to": cond.chunks_for(batch_uc, *tiles)} if chunked and hasattr(cond, "chunks_for") else {}
            if pad and pad["pad_to"] == 1:
                pad = {}
            c, uc = [], None
            for i, tile in enumerate(tiles):
                with self._ae_scope():
                    if i == 0:
                        _c, uc = cond.get_unconditional_conditioning(tile, batch_uc, **pad)
                    else:
                        _c, _ = cond.get_unconditional_conditioning(tile, None, **pad)
                c.append(_c)
            return c, uc
        finally:
            if chunked:
                cond.prompt_chunks = saved
