"""Prompts longer than 77 tokens on the GPU: the text towers on two chunks, one network call with a 154-token context on the fused
to_q + cross-attention kernel, batchify_sample(prompt_chunks=2) end to end, and the tiled sampler with per-tile 154-token contexts.
Fixtures, sizes and bounds are those of the 77-token tests each case extends (named at each test)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cond_oracle as CO  # noqa: E402
from supir_amd import ops  # noqa: E402
from tests.helpers import build_unet, rel_l2, synth_tensor  # noqa: E402

DEV = "cuda"
BOS, EOS = 49406, 49407


def T(name, shape, **kw):
    return synth_tensor(name, shape, **kw).to(DEV)


def _tokens(n, chunks, seed, pos=(76, 20, 9, 50)):
    """[n, 77 chunks] ids, every chunk [BOS] ids [EOS] 0 ... with its own EOS position."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(1000, 40000, (n, chunks, 77), generator=g)
    t[:, :, 0] = BOS
    for i in range(n):
        for j in range(chunks):
            e = pos[(2 * i + j) % len(pos)]
            t[i, j, e] = EOS
            t[i, j, e + 1:] = 0
    return t.reshape(n, chunks * 77)


@pytest.fixture(scope="module")
def model():
    """The reduced-depth model with the full-size text conditioner of tests/test_testpy_flow_gpu.py (reference-style config, synthetic
    checkpoint), built with SUPIR_PROMPT_CHUNKS set: the constructor takes its default from it."""
    import os
    from supir_amd.plugin import instantiate_from_config
    from tests.test_reference_test_py import synthetic_checkpoint
    from tests.test_testpy_flow_gpu import _config
    old = os.environ.get("SUPIR_PROMPT_CHUNKS")
    os.environ["SUPIR_PROMPT_CHUNKS"] = "3"
    try:
        m = instantiate_from_config(_config()).cpu()
    finally:
        if old is None:
            del os.environ["SUPIR_PROMPT_CHUNKS"]
        else:
            os.environ["SUPIR_PROMPT_CHUNKS"] = old
    assert m.prompt_chunks == 3
    m.prompt_chunks = 1
    assert not m.load_state_dict(synthetic_checkpoint(), strict=False).unexpected_keys
    m.ae_dtype = torch.bfloat16
    m.model.dtype = torch.bfloat16
    return m.to(DEV)


def _oracle_chunked(cond_sd, batch, tokens):
    """oracle/cond_oracle.py once per 77-token chunk: crossattn joined along the token axis, vector (pooled | sizes) from chunk 0."""
    outs = [CO.general_conditioner_with_control(cond_sd, batch, tokens[:, j:j + 77], tokens[:, j:j + 77]) for j in range(0, tokens.shape[1], 77)]
    return {"crossattn": torch.cat([o["crossattn"] for o in outs], 1), "vector": outs[0]["vector"]}


def test_text_towers_on_two_chunks_vs_oracle(model):
    """tests/test_conditioner.py::test_text_towers_on_gpu_vs_oracle on [2, 154] ids, the oracle run per chunk; its tolerances."""
    cl, g = model.conditioner.embedders[0], model.conditioner.embedders[1]
    tok = _tokens(2, 2, seed=3)
    with torch.no_grad():
        z = cl(tok)
        pen, pooled = g(tok)
        per_z = [CO.clip_l_hidden(cl.state_dict(), tok[:, j:j + 77].to(DEV), p="transformer.text_model.") for j in (0, 77)]
        per_g = [CO.openclip_g_penultimate_pooled(g.state_dict(), tok[:, j:j + 77].to(DEV), p="model.") for j in (0, 77)]
    e = dict(clip_l_hidden11=rel_l2(z, torch.cat(per_z, 1)), bigg_penultimate=rel_l2(pen, torch.cat([p[0] for p in per_g], 1)),
             bigg_pooled=rel_l2(pooled, per_g[0][1]))
    print("[parity] text towers, two chunks:", {k: f"{v:.3e}" for k, v in e.items()})
    assert z.shape == (2, 154, 768) and pen.shape == (2, 154, 1280) and pooled.shape == (2, 1280)
    assert e["clip_l_hidden11"] <= 1.5e-2 and e["bigg_penultimate"] <= 2e-2 and e["bigg_pooled"] <= 2.5e-2
    assert rel_l2(pooled, per_g[1][1]) > 0.1           # chunk 0's pooled vector, not chunk 1's
    with pytest.raises(ValueError):
        cl(tok[:, :100])


def test_network_call_with_a_154_token_context_runs_the_fused_kernel(monkeypatch):
    """tests/test_model_gpu.py::test_wrapper_vs_oracle_with_measured_bf16_floor with crossattn [2, 154, 2048] -- same network
    (build_unet depth (1, 1, 2)), same synthetic inputs by name, same bound max(2e-2, 1.5 x the ATen-bf16 floor) -- at latent 32^2
    instead of 16^2: the fused kernel takes whole 128-token row blocks, and 32^2 is the smallest latent whose attention levels have
    one (16 x 16 = 256 tokens at 640 channels; 8 x 8 = 64 tokens stay on the two-launch form).  The pick between the fused and the
    two-launch form is forced to the fused one and read back from the launch trace."""
    from tests.test_model_gpu import _bf16_floor, _oracle_sd
    wrap = build_unet(depth=(1, 1, 2), device=DEV)
    B = 2
    x, lq = T("xt32", (B, 4, 32, 32)), T("lq32", (B, 4, 32, 32))
    cond = {"crossattn": T("context154", (B, 154, 2048)), "vector": T("vector", (B, 2816)), "control": lq}
    t = torch.tensor([500, 37], dtype=torch.int64, device=DEV)
    real_choose = ops.choose
    monkeypatch.setattr(ops, "choose", lambda key, fns, **kw: 1 if key[0] == "xattn" else real_choose(key, fns, **kw))
    ref, floor = _bf16_floor(_oracle_sd(wrap), x, t, cond)
    ops.start_trace()
    try:
        with torch.no_grad():
            out = wrap(x, t, cond, 1.0)
    finally:
        trace = ops.stop_trace()
    fused = [r for r in trace if r["kernel"] == "xattn_q"]
    assert fused and all(r["Tk"] == 154 for r in fused), [r["kernel"] for r in trace][:20]
    assert {(r["T"], r["C"]) for r in fused} == {(256, 640)}
    e = rel_l2(out, ref)
    print(f"mini wrapper, 154-token context: HIP bf16 vs fp32 oracle {e:.3e}; ATen-autocast bf16 floor {floor:.3e}; "
          f"{len(fused)} fused xattn launches")
    assert torch.isfinite(out).all() and e <= max(2e-2, 1.5 * floor)


def test_batchify_sample_with_two_prompt_chunks_vs_oracle_conditioning(model):
    """batchify_sample(prompt_chunks=2) on token-id prompts (positive: two chunks; negative: one, padded with an empty chunk) at the
    256 px / latent 32^2 of tests/test_testpy_flow_gpu.py, 2 steps, every RNG draw injected -- against the same call given cond=(c, uc)
    from the fp32 oracle conditioner run per chunk.  The two runs differ by the towers' bf16 arithmetic only; bound: the 5e-3 the
    config-1 test (tests/test_parity_production_gpu.py) caps the final latent's distance between product and oracle at."""
    lat, steps = 32, 2
    x = T("lp.img", (1, 3, 256, 256), scale=0.5).clamp(-1, 1)
    pos, neg = _tokens(1, 2, seed=7), _tokens(1, 1, seed=8, pos=(30,))
    noises = lambda: {"posterior": T("lp.post", (1, 4, lat, lat)), "init": T("lp.init", (1, 4, lat, lat)),  # noqa: E731
                      "steps": [T(f"lp.eps{i}", (1, 4, lat, lat)) for i in range(steps)]}
    kw = dict(num_steps=steps, restoration_scale=-1, s_churn=5, s_noise=1.01, cfg_scale=4.0, control_scale=1.0, seed=1234,
              use_linear_CFG=True, cfg_scale_start=1.0, return_intermediates=True)
    model.model.enable_graph(False)
    seen = []
    hook = model.model.register_forward_pre_hook(lambda mod, args: seen.append(tuple(args[2]["crossattn"].shape)))
    try:
        with torch.no_grad():
            out, mid = model.batchify_sample(x, pos, n_p=neg[0], noises=noises(), prompt_chunks=2, **kw)
            one, one_mid = model.batchify_sample(x, pos[:, :77], n_p=neg[0], noises=noises(), **kw)   # the default: one chunk
    finally:
        hook.remove()
    assert seen and set(seen[:len(seen) // 2]) == {(2, 154, 2048)} and set(seen[len(seen) // 2:]) == {(2, 77, 2048)}, set(seen)
    assert model.conditioner.prompt_chunks == 1 and model.prompt_chunks == 1
    sd = {k: v.float() for k, v in model.conditioner.state_dict().items()}
    z = mid["z"]
    batch = {"original_size_as_tuple": torch.tensor([[1024, 1024]], device=DEV), "crop_coords_top_left": torch.tensor([[0, 0]], device=DEV),
             "target_size_as_tuple": torch.tensor([[1024, 1024]], device=DEV), "control": z}
    empty = torch.tensor([[BOS, EOS] + [0] * 75])
    with torch.no_grad():
        c = _oracle_chunked(sd, batch, pos.to(DEV))
        # the oracle takes one id tensor per tower: the empty chunk's padding (EOS for CLIP-L, 0 for bigG) sits after the EOS, where
        # CLIP-L's causal rows up to the EOS do not see it -- but its later rows do, so each tower gets its own convention
        neg2 = torch.cat([neg, empty], 1).to(DEV)
        neg2_l = neg2.clone()
        neg2_l[:, 77 + 2:] = EOS
        u0 = CO.general_conditioner_with_control(sd, batch, neg2_l[:, :77], neg2[:, :77])
        u1 = CO.general_conditioner_with_control(sd, batch, neg2_l[:, 77:], neg2[:, 77:])
        uc = {"crossattn": torch.cat([u0["crossattn"], u1["crossattn"]], 1), "vector": u0["vector"]}
        ref, rmid = model.batchify_sample(x, cond=(c, uc), noises=noises(), **kw)
    e_lat, e_img = rel_l2(mid["samples"], rmid["samples"]), rel_l2(out, ref)
    d_one = rel_l2(mid["samples"], one_mid["samples"])
    print(f"[long prompt e2e] product vs oracle conditioning, two chunks: latent rel-L2 {e_lat:.3e}, image {e_img:.3e}; "
          f"two chunks vs the first chunk alone: latent {d_one:.3e}")
    assert torch.isfinite(out).all() and out.shape == (1, 3, 256, 256)
    assert e_lat <= 5e-3, e_lat
    assert d_one > e_lat            # the second chunk reaches the result: dropping it moves the latent further than the towers' rounding


def test_tiled_sampler_with_per_tile_154_token_contexts(monkeypatch):
    """tests/test_local_prompt_tiles_gpu.py's comparison -- the fused, graph-replayed tiled EDM sampler over per-tile prompts against
    the generic one-tile-per-call loop, latent 48 x 64 in 32 x 32 tiles, bar 1e-2, same RNG consumption -- with 154-token contexts
    and tile batch 2: the per-image bank of text K / V^T, its gather tables and the captured graph are keyed on the context's shape."""
    from supir_amd.modules import sampling
    from supir_amd.modules.sampling import DiscreteDenoiserWithControl
    from tests.test_local_prompt_tiles_gpu import H, W, N_TILES, _run, _sampler
    mini = build_unet(depth=(1, 1, 2), device=DEV)
    den = DiscreteDenoiserWithControl().to(DEV)
    lq, xc = T("lq_tiled2", (1, 4, H, W)), T("fs.center2", (1, 4, H, W))
    local = [{"crossattn": T(f"lp154.ctx{j}", (1, 154, 2048)), "vector": T(f"lp.vec{j}", (1, 2816)), "control": lq} for j in range(N_TILES)]
    uc = {"crossattn": T("lp154.uc", (1, 154, 2048)), "vector": T("vector", (2, 2816))[1:], "control": lq}

    def denoiser(i, s, cc, cs):
        return den(mini, i, s, cc, cs)

    monkeypatch.setattr(sampling, "EMB_SCHEDULE", True)
    monkeypatch.setattr(sampling, "FUSED_EDM_STEP", False)
    generic = _run("edm", _sampler("edm", tile_batch=2), denoiser, local, uc, xc)
    denoiser.fused = (den, mini)
    monkeypatch.setattr(sampling, "FUSED_EDM_STEP", True)
    banks = []
    real_bank = mini.prepare_context_bank

    def bank(*a, **k):
        ok = real_bank(*a, **k)
        banks.append((ok, [tuple(s_) for s_ in mini._bank["shapes"]] if ok else None))
        return ok

    monkeypatch.setattr(mini, "prepare_context_bank", bank)
    mini.enable_graph(True)
    try:
        fused = _run("edm", _sampler("edm", tile_batch=2, tile_batch_local_prompts=True), denoiser, local, uc, xc)
        stats = mini.graph_stats()
    finally:
        mini.enable_graph(False)
    e = rel_l2(fused[0], generic[0])
    print(f"[long prompt tiles] fused + graph vs generic loop, 154-token per-tile contexts: rel-L2 {e:.3e}; {stats}; bank {banks}")
    assert banks and banks[0][0] and len(banks[0][1]) == 1 and 154 in banks[0][1][0]
    assert stats["eager"] == 0 and stats["captures"] == 1 and stats["replays"] == 3 * 3          # 3 steps x 3 groups of 2 tiles
    assert e <= 1e-2 and torch.equal(fused[1], generic[1])
