"""Text conditioner (sgm/modules/encoders/modules.py:193-243, 445-609, 1027-1043).

CPU tier: the oracle restatement (oracle/cond_oracle.py) is pinned against the real transformers.CLIPTextModel (the class the
reference instantiates for CLIP-L) and, block-wise, against torch.nn.MultiheadAttention (what open_clip's ResidualAttentionBlock
wraps; open_clip itself is not installed), and the bigG tower -- the fixtures' and the oracle's -- against
transformers.CLIPTextModelWithProjection, an independent implementation of the same architecture; state-dict keys of the product classes against the
transformers / open_clip naming; the conditioner's key routing / concatenation.
GPU tier: the HIP towers at full size (CLIP-L 12 x 768, bigG 32 x 1280) against the oracle on synthetic weights.
"""
import pytest
import torch
import torch.nn as nn

from oracle import cond_oracle as CO
from supir_amd.synth import synth_param


def _tokens(n, seed=0, eot_pos=(20, 76)):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(1000, 40000, (n, 77), generator=g)
    t[:, 0] = 49406
    for i in range(n):
        e = eot_pos[i % len(eot_pos)]
        t[i, e] = 49407
        t[i, e + 1:] = 0
    return t


def test_clip_l_restatement_vs_transformers_cliptextmodel():
    from transformers import CLIPTextConfig, CLIPTextModel
    cfg = CLIPTextConfig(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                         max_position_embeddings=77, hidden_act="quick_gelu")
    torch.manual_seed(0)
    hf = CLIPTextModel(cfg).eval()
    sd = {}
    for k, v in hf.state_dict().items():
        k = k if k.startswith("text_model.") else "text_model." + k     # transformers >= 5 dropped the wrapper level
        sd["transformer." + k] = v.float()
    tok = _tokens(2)
    tok_hf = tok.clone()
    tok_hf[tok_hf == 0] = 49407      # HF pads with eot; hidden_states before the eot position do not depend on the padding (causal)
    with torch.no_grad():
        ref = hf(input_ids=tok_hf, output_hidden_states=True).hidden_states[11]
        got = CO.clip_l_hidden(sd, tok_hf)
    assert ((got - ref).norm() / ref.norm()).item() <= 2e-5
    with torch.no_grad():
        got0 = CO.clip_l_hidden(sd, tok)
    assert torch.allclose(got0[0, :21], got[0, :21], atol=1e-5)       # causal: rows up to the eot are padding independent


def test_openclip_block_restatement_vs_torch_multihead_attention():
    d, heads, n = 128, 2, 77
    torch.manual_seed(1)
    mha = nn.MultiheadAttention(d, heads, batch_first=True)
    ln1, ln2 = nn.LayerNorm(d), nn.LayerNorm(d)
    fc, proj = nn.Linear(d, 4 * d), nn.Linear(4 * d, d)
    sd = {"b.ln_1.weight": ln1.weight, "b.ln_1.bias": ln1.bias, "b.ln_2.weight": ln2.weight, "b.ln_2.bias": ln2.bias,
          "b.attn.in_proj_weight": mha.in_proj_weight, "b.attn.in_proj_bias": mha.in_proj_bias,
          "b.attn.out_proj.weight": mha.out_proj.weight, "b.attn.out_proj.bias": mha.out_proj.bias,
          "b.mlp.c_fc.weight": fc.weight, "b.mlp.c_fc.bias": fc.bias, "b.mlp.c_proj.weight": proj.weight, "b.mlp.c_proj.bias": proj.bias}
    x = torch.randn(2, n, d)
    mask = CO.causal_mask(n, "cpu")
    with torch.no_grad():
        h = ln1(x)
        y = x + mha(h, h, h, need_weights=False, attn_mask=mask)[0]
        ref = y + proj(torch.nn.functional.gelu(fc(ln2(y))))
        got = CO.openclip_block({k: v.detach() for k, v in sd.items()}, "b.", x, heads)
    assert ((got - ref).norm() / ref.norm()).item() <= 2e-5


def _cond_golden():
    import os
    return torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_cond.pt"), map_location="cpu")


def test_oracle_vs_the_references_own_conditioner_classes():
    """oracle/cond_oracle.py against outputs of the reference's GeneralConditionerWithControl + FrozenCLIPEmbedder +
    FrozenOpenCLIPEmbedder2 + ConcatTimestepEmbedderND (tests/golden/golden_cond.pt, written by oracle/gen_golden_cond.py from
    /root/reference: c and uc of get_unconditional_conditioning as SUPIR_model.py:166 calls it, force_uc_zero_embeddings, and the
    legacy branch of the OpenCLIP embedder).  Pins dim-keyed concatenation order, penultimate-layer selection, argmax-EOT pooling,
    the hidden_states[11] choice, force-zero by input key and control passthrough."""
    from oracle import gen_golden_cond as G
    gold = _cond_golden()
    # the synthetic state dict the generator loaded into the reference classes, rebuilt from key names + shapes alone
    shapes = {}
    with torch.device("meta"):
        from transformers import CLIPTextConfig, CLIPTextModel
        hf = CLIPTextModel(CLIPTextConfig(vocab_size=G.VOCAB, hidden_size=G.L_WIDTH, intermediate_size=4 * G.L_WIDTH, num_hidden_layers=G.L_LAYERS,
                                          num_attention_heads=G.L_HEADS, max_position_embeddings=77, hidden_act="quick_gelu"))
        oc = G._FakeOpenClipModel()
    for k, v in hf.state_dict().items():
        shapes[G.canonical_key("embedders.0.transformer." + k)] = tuple(v.shape)
    for k, v in oc.state_dict().items():
        shapes["embedders.1.model." + k] = tuple(v.shape)
    sd = {k: synth_param("conditioner." + k, shp) for k, shp in shapes.items() if "position_ids" not in k}
    c_b, uc_b = G.batches()
    tok = lambda texts: torch.stack([gold["texts"][t] for t in texts])  # noqa: E731
    rel = lambda a, b: ((a - b).norm() / (b.norm() + 1e-20)).item()  # noqa: E731
    with torch.no_grad():
        c = CO.general_conditioner_with_control(sd, c_b, tok(c_b["txt"]), tok(c_b["txt"]), heads_l=G.L_HEADS, heads_g=G.G_HEADS)
        uc = CO.general_conditioner_with_control(sd, uc_b, tok(uc_b["txt"]), tok(uc_b["txt"]), heads_l=G.L_HEADS, heads_g=G.G_HEADS)
        uc0 = CO.general_conditioner_with_control(sd, uc_b, tok(uc_b["txt"]), tok(uc_b["txt"]), force_zero_embeddings=["txt"],
                                                  heads_l=G.L_HEADS, heads_g=G.G_HEADS)
        gsd = {k[len("embedders.1."):]: v for k, v in sd.items() if k.startswith("embedders.1.")}
        leg = {layer: CO.openclip_g_legacy(gsd, tok(c_b["txt"]), layer, heads=G.G_HEADS) for layer in ("last", "penultimate")}
    for name, got in (("c", c), ("uc", uc)):
        assert got["crossattn"].shape == gold[f"{name}.crossattn"].shape == (2, 77, G.L_WIDTH + G.G_WIDTH)
        assert rel(got["crossattn"], gold[f"{name}.crossattn"]) <= 2e-5, name
        assert rel(got["vector"], gold[f"{name}.vector"]) <= 2e-5, name
        assert torch.equal(got["control"], gold[f"{name}.control"])
    assert torch.equal(uc0["crossattn"], gold["uc_force_zero_txt.crossattn"]) and uc0["crossattn"].abs().sum() == 0
    assert rel(uc0["vector"], gold["uc_force_zero_txt.vector"]) <= 2e-5 and uc0["vector"][:, :G.G_PROJ].abs().sum() == 0
    for layer in ("last", "penultimate"):
        assert rel(leg[layer], gold[f"g_legacy_{layer}"]) <= 2e-5, layer
    # c and uc differ (different prompts), the size embeddings are prompt independent
    assert rel(c["crossattn"], uc["crossattn"]) > 0.1 and torch.equal(c["vector"][:, G.G_PROJ:], uc["vector"][:, G.G_PROJ:])


def test_conditioner_fixture_reproduces_from_the_live_reference():
    """With /root/reference mounted (the build container): re-run the generator and require the committed fixture bit for bit."""
    from oracle import ref_import
    if not ref_import.available():
        pytest.skip("reference checkout not mounted")
    # in a fresh interpreter: other tests of this session call plugin.install(), which re-points the reference's module attributes
    # at this package's classes -- the generator must see the genuine reference
    import os
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "cond.pt")
        subprocess.run([sys.executable, "-m", "oracle.gen_golden_cond", "--out", path], cwd=root, check=True, capture_output=True, timeout=600)
        live = torch.load(path, map_location="cpu")
    gold = _cond_golden()
    assert set(live) == set(gold)
    for k, v in gold.items():
        if torch.is_tensor(v):
            assert torch.equal(live[k], v), k


def test_product_state_dict_keys_follow_transformers_and_open_clip():
    from transformers import CLIPTextConfig, CLIPTextModel
    from supir_amd.modules import conditioner as C
    with torch.device("meta"):
        ours = C.FrozenCLIPEmbedder(layer="hidden", layer_idx=11)
        hf = CLIPTextModel(CLIPTextConfig(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                                          num_attention_heads=12, max_position_embeddings=77, hidden_act="quick_gelu"))
        g = C.FrozenOpenCLIPEmbedder2(arch="ViT-bigG-14", layer="penultimate", always_return_pooled=True, legacy=False)
    want = {("transformer." + (k if k.startswith("text_model.") else "text_model." + k)): tuple(v.shape) for k, v in hf.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in ours.state_dict().items()} == want
    gk = {k: tuple(v.shape) for k, v in g.state_dict().items()}
    assert gk["model.positional_embedding"] == (77, 1280) and gk["model.text_projection"] == (1280, 1280)
    assert gk["model.token_embedding.weight"] == (49408, 1280) and gk["model.ln_final.weight"] == (1280,)
    for i in (0, 31):
        p = f"model.transformer.resblocks.{i}."
        assert gk[p + "attn.in_proj_weight"] == (3840, 1280) and gk[p + "attn.out_proj.weight"] == (1280, 1280)
        assert gk[p + "mlp.c_fc.weight"] == (5120, 1280) and gk[p + "mlp.c_proj.weight"] == (1280, 5120)
        assert gk[p + "ln_1.weight"] == gk[p + "ln_2.bias"] == (1280,)
    assert len(gk) == 4 + 2 + 32 * 12          # open_clip's text-side key count for ViT-bigG-14 (visual tower deleted, modules.py:538)


def test_conditioner_routing_concat_and_control_passthrough():
    """GeneralConditionerWithControl: 3-D outputs concatenate on dim 2 into crossattn, 2-D on dim 1 into vector, tuple outputs are
    routed element-wise, force_zero_embeddings zeroes by input key, `control` is passed through (modules.py:193-243)."""
    from supir_amd.modules import conditioner as C

    class A(C.AbstractEmbModel):
        def forward(self, txt):
            return torch.ones(len(txt), 77, 3)

    class B(C.AbstractEmbModel):
        def forward(self, txt):
            return torch.full((len(txt), 77, 5), 2.0), torch.full((len(txt), 7), 3.0)

    C._test_A, C._test_B = A, B
    cfgs = [{"target": "supir_amd.modules.conditioner._test_A", "input_key": "txt"},
            {"target": "supir_amd.modules.conditioner._test_B", "input_key": "txt"},
            {"target": "supir_amd.modules.conditioner.ConcatTimestepEmbedderND", "params": {"outdim": 256},
             "input_key": "original_size_as_tuple"}]
    cond = C.GeneralConditionerWithControl(cfgs)
    batch = {"txt": ["a", "b"], "original_size_as_tuple": torch.tensor([[1024, 1024], [512, 768]]), "control": torch.zeros(2, 4, 8, 8)}
    out = cond(batch)
    assert out["crossattn"].shape == (2, 77, 8) and out["vector"].shape == (2, 7 + 512) and out["control"] is batch["control"]
    assert torch.equal(out["vector"][:, 7:], CO.concat_timestep_embedder_nd(batch["original_size_as_tuple"]))
    c, uc = cond.get_unconditional_conditioning(batch, dict(batch, txt=["", ""]), force_uc_zero_embeddings=["txt"])
    assert c["crossattn"].abs().sum() > 0 and uc["crossattn"].abs().sum() == 0 and uc["vector"][:, :7].abs().sum() == 0
    assert uc["vector"][:, 7:].abs().sum() > 0
    # a config carrying training-time rates still serves inference: get_unconditional_conditioning zeroes the rates for its two
    # encodes and restores them (modules.py:177-191); legacy_ucg_value alone (rate 0) is a no-op; a direct forward with a live rate
    # is refused (conditioning dropout is not on this path)
    cfgs[0] = dict(cfgs[0], ucg_rate=0.2, legacy_ucg_value="")
    cfgs[1] = dict(cfgs[1], legacy_ucg_value="")
    cond2 = C.GeneralConditionerWithControl(cfgs)
    c2, uc2 = cond2.get_unconditional_conditioning(batch, dict(batch, txt=["", ""]), force_uc_zero_embeddings=["txt"])
    assert torch.equal(c2["crossattn"], c["crossattn"]) and torch.equal(uc2["vector"], uc["vector"])
    assert [e.ucg_rate for e in cond2.embedders] == [0.2, 0.0, 0.0]
    with pytest.raises(NotImplementedError):
        cond2(batch)


def _fill(module, prefix, dev):
    with torch.no_grad():
        for k, t in module.state_dict().items():
            if t.is_floating_point():
                t.copy_(synth_param(prefix + k, t.shape, device=dev))
    return module


@pytest.mark.gpu
def test_text_towers_on_gpu_vs_oracle():
    from supir_amd.modules import conditioner as C
    dev = "cuda"
    tok = _tokens(2, seed=3)
    with torch.device(dev):
        cl = C.FrozenCLIPEmbedder(layer="hidden", layer_idx=11)
        g = C.FrozenOpenCLIPEmbedder2(arch="ViT-bigG-14", layer="penultimate", always_return_pooled=True, legacy=False)
    _fill(cl, "conditioner.embedders.0.", dev)
    _fill(g, "conditioner.embedders.1.", dev)
    with torch.no_grad():
        z = cl(tok)
        pen, pooled = g(tok)
        ref_z = CO.clip_l_hidden(cl.state_dict(), tok.to(dev), p="transformer.text_model.")
        ref_pen, ref_pool = CO.openclip_g_penultimate_pooled(g.state_dict(), tok.to(dev), p="model.")
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()
    e = dict(clip_l_hidden11=rel(z, ref_z), bigg_penultimate=rel(pen, ref_pen), bigg_pooled=rel(pooled, ref_pool))
    print("[parity] text towers:", {k: f"{v:.3e}" for k, v in e.items()})
    assert z.shape == (2, 77, 768) and pen.shape == (2, 77, 1280) and pooled.shape == (2, 1280)
    assert e["clip_l_hidden11"] <= 1.5e-2 and e["bigg_penultimate"] <= 2e-2 and e["bigg_pooled"] <= 2.5e-2
    # causal mask: changing tokens AFTER position p leaves rows <= p unchanged bit for bit
    tok2 = tok.clone()
    tok2[:, 40:] = torch.randint(1000, 40000, (2, 37))
    with torch.no_grad():
        z2 = cl(tok2)
    assert torch.equal(z[:, :40], z2[:, :40]) and not torch.equal(z[:, 40:], z2[:, 40:])


@pytest.mark.gpu
def test_general_conditioner_with_control_on_gpu_vs_oracle():
    """The embedder list of options/SUPIR_v0.yaml:66-106 through the plugin: crossattn [N,77,2048], vector [N,2816], control."""
    from supir_amd.plugin import instantiate_from_config
    dev = "cuda"
    P = "sgm.modules.encoders.modules."
    cfg = {"target": "sgm.modules.GeneralConditionerWithControl", "params": {"emb_models": [
        {"is_trainable": False, "input_key": "txt", "target": P + "FrozenCLIPEmbedder", "params": {"layer": "hidden", "layer_idx": 11}},
        {"is_trainable": False, "input_key": "txt", "target": P + "FrozenOpenCLIPEmbedder2",
         "params": {"arch": "ViT-bigG-14", "version": "laion2b_s39b_b160k", "freeze": True, "layer": "penultimate",
                    "always_return_pooled": True, "legacy": False}},
        {"is_trainable": False, "input_key": "original_size_as_tuple", "target": P + "ConcatTimestepEmbedderND", "params": {"outdim": 256}},
        {"is_trainable": False, "input_key": "crop_coords_top_left", "target": P + "ConcatTimestepEmbedderND", "params": {"outdim": 256}},
        {"is_trainable": False, "input_key": "target_size_as_tuple", "target": P + "ConcatTimestepEmbedderND", "params": {"outdim": 256}}]}}
    with torch.device(dev):
        cond = instantiate_from_config(cfg)
    _fill(cond, "conditioner.", dev)
    tok = _tokens(2, seed=5)
    z4 = torch.zeros(2, 4, 16, 16, device=dev)
    batch = {"txt": tok, "original_size_as_tuple": torch.tensor([1024, 1024]).repeat(2, 1).to(dev),
             "crop_coords_top_left": torch.tensor([0, 0]).repeat(2, 1).to(dev),
             "target_size_as_tuple": torch.tensor([1024, 1024]).repeat(2, 1).to(dev), "control": z4}
    with torch.no_grad():
        c, uc = cond.get_unconditional_conditioning(batch, dict(batch, txt=_tokens(2, seed=6)))
        ref = CO.general_conditioner_with_control(cond.state_dict(), batch, tok.to(dev), tok.to(dev))
    assert c["crossattn"].shape == (2, 77, 2048) and c["vector"].shape == (2, 2816) and c["control"] is z4
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm()).item()
    assert rel(c["crossattn"], ref["crossattn"]) <= 2e-2 and rel(c["vector"], ref["vector"]) <= 2e-2
    assert not torch.equal(c["crossattn"], uc["crossattn"])


def test_bigg_tower_vs_transformers_cliptextmodelwithprojection():
    """open_clip is not installable here, so the bigG tower of the fixtures (tests/golden/golden_cond.pt: the REFERENCE'S
    FrozenOpenCLIPEmbedder2, sgm/modules/encoders/modules.py:513-609, run over a stand-in open_clip text tower) is held against a second,
    independently written implementation of the same published architecture: transformers.CLIPTextModelWithProjection -- the class
    diffusers loads SDXL's second text encoder (the same OpenCLIP ViT-bigG-14 checkpoint, converted) into.  Weights are the fixtures'
    (supir_amd.synth by reference key name) re-keyed open_clip -> transformers: in_proj_weight split into q / k / v, c_fc / c_proj -> fc1 /
    fc2, text_projection transposed into a bias-free Linear.  Compared: the penultimate hidden state (hidden_states[-2], no final
    LayerNorm: modules.py:583-597 `penultimate`) and the pooled, projected eot row (modules.py:575-581) -- i.e. the block arithmetic
    (pre-LN residual block, packed-QKV multi-head attention with the causal mask, erf-GELU MLP) that the stand-in restates, and with it the
    oracle's and the product's towers, which the other tests hold to these fixtures."""
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    gold = _cond_golden()
    D, LAYERS, HEADS, PROJ, L_WIDTH = 320, 6, 20, 320, 192          # oracle/gen_golden_cond.py: the reduced "bigG" of the fixtures
    cfg = CLIPTextConfig(vocab_size=49408, hidden_size=D, intermediate_size=4 * D, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                         max_position_embeddings=77, hidden_act="gelu", projection_dim=PROJ, eos_token_id=2)   # 2: pooled row = argmax(ids)
    hf = CLIPTextModelWithProjection(cfg).eval()
    P = "conditioner.embedders.1.model."
    syn = lambda name, shape: synth_param(P + name, shape)  # noqa: E731
    new = {}
    for k, t in hf.state_dict().items():
        kk = k[len("text_model."):] if k.startswith("text_model.") else k
        if kk == "embeddings.token_embedding.weight":
            v = syn("token_embedding.weight", t.shape)
        elif kk == "embeddings.position_embedding.weight":
            v = syn("positional_embedding", t.shape)
        elif kk.startswith("final_layer_norm."):
            v = syn("ln_final." + kk.split(".")[-1], t.shape)
        elif kk == "text_projection.weight":
            v = syn("text_projection", (D, PROJ)).t()                   # open_clip: x @ text_projection; HF: Linear(weight = its transpose)
        elif kk.startswith("encoder.layers."):
            _, _, i, *rest = kk.split(".")
            B = f"transformer.resblocks.{i}."
            rest = ".".join(rest)
            wb = rest.split(".")[-1]
            if rest.startswith("self_attn.") and rest.split(".")[1] in ("q_proj", "k_proj", "v_proj"):
                j = ("q_proj", "k_proj", "v_proj").index(rest.split(".")[1])
                full = syn(B + "attn.in_proj_" + wb, (3 * D, D) if wb == "weight" else (3 * D,))
                v = full[j * D:(j + 1) * D]
            else:
                name = {"self_attn.out_proj": "attn.out_proj", "layer_norm1": "ln_1", "layer_norm2": "ln_2", "mlp.fc1": "mlp.c_fc",
                        "mlp.fc2": "mlp.c_proj"}[rest.rsplit(".", 1)[0]]
                v = syn(B + name + "." + wb, t.shape)
        else:
            continue                                                     # position_ids buffer
        assert v.shape == t.shape, (k, v.shape, t.shape)
        new[k] = v.contiguous()
    missing = [k for k, t in hf.state_dict().items() if t.is_floating_point() and k not in new]
    assert not missing, missing
    hf.load_state_dict(new, strict=False)
    texts = ["a photo of a cat", "cinematic, high detail, 8k"]          # gen_golden_cond.batches(): the `c` batch
    ids = torch.stack([gold["texts"][t] for t in texts])
    with torch.no_grad():
        out = hf(input_ids=ids, output_hidden_states=True)
    pen_ref = gold["c.crossattn"][:, :, L_WIDTH:]                        # crossattn = CLIP-L hidden[11] | bigG penultimate
    pooled_ref = gold["c.vector"][:, :PROJ]                              # vector = bigG pooled | 3 x sincos
    pen, pooled = out.hidden_states[-2], out.text_embeds
    d_pen, d_pool = ((pen - pen_ref).norm() / pen_ref.norm()).item(), ((pooled - pooled_ref).norm() / pooled_ref.norm()).item()
    print(f"bigG tower, reference-over-stand-in vs transformers: penultimate {d_pen:.2e}, pooled {d_pool:.2e}")
    assert d_pen <= 2e-5 and d_pool <= 2e-5
    # and the legacy branch (modules.py:565-568): ln_final of the last layer == HF's last_hidden_state
    assert ((out.last_hidden_state - gold["g_legacy_last"]).norm() / gold["g_legacy_last"].norm()).item() <= 2e-5


def test_bigg_restatement_vs_transformers_at_the_real_head_geometry():
    """The oracle's own bigG restatement (oracle/cond_oracle.py: openclip_g_penultimate_pooled / openclip_g_legacy) against
    transformers.CLIPTextModelWithProjection at ViT-bigG-14's real width and head geometry (1280 wide, 20 heads of 64, MLP 5120,
    projection 1280; 3 of the 32 layers to keep the CPU tier short), HF's own random initialisation re-keyed to open_clip's names."""
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    D, LAYERS, HEADS = 1280, 3, 20
    cfg = CLIPTextConfig(vocab_size=49408, hidden_size=D, intermediate_size=4 * D, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                         max_position_embeddings=77, hidden_act="gelu", projection_dim=D, eos_token_id=2)
    torch.manual_seed(3)
    hf = CLIPTextModelWithProjection(cfg).eval()
    with torch.no_grad():
        for n_, p_ in hf.named_parameters():          # HF initialises biases / LayerNorm to 0 / 1: make every term of the arithmetic count
            if p_.ndim == 1:
                p_.add_(0.1 * torch.randn_like(p_))
    h = {(k[len("text_model."):] if k.startswith("text_model.") else k): v.float() for k, v in hf.state_dict().items()}
    sd = {"model.token_embedding.weight": h["embeddings.token_embedding.weight"],
          "model.positional_embedding": h["embeddings.position_embedding.weight"],
          "model.ln_final.weight": h["final_layer_norm.weight"], "model.ln_final.bias": h["final_layer_norm.bias"],
          "model.text_projection": h["text_projection.weight"].t().contiguous()}
    for i in range(LAYERS):
        s, q = f"encoder.layers.{i}.", f"model.transformer.resblocks.{i}."
        sd[q + "attn.in_proj_weight"] = torch.cat([h[s + f"self_attn.{n}_proj.weight"] for n in "qkv"])
        sd[q + "attn.in_proj_bias"] = torch.cat([h[s + f"self_attn.{n}_proj.bias"] for n in "qkv"])
        for a, b in (("self_attn.out_proj", "attn.out_proj"), ("layer_norm1", "ln_1"), ("layer_norm2", "ln_2"), ("mlp.fc1", "mlp.c_fc"),
                     ("mlp.fc2", "mlp.c_proj")):
            sd[q + b + ".weight"], sd[q + b + ".bias"] = h[s + a + ".weight"], h[s + a + ".bias"]
    tok = _tokens(2, seed=5, eot_pos=(9, 76))
    with torch.no_grad():
        out = hf(input_ids=tok, output_hidden_states=True)
        pen, pooled = CO.openclip_g_penultimate_pooled(sd, tok, p="model.", heads=HEADS)
        last = CO.openclip_g_legacy(sd, tok, "last", p="model.", heads=HEADS)
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()  # noqa: E731
    # rows after the eot see padding tokens (id 0) in both implementations alike (causal mask only, no padding mask: modules.py:571)
    assert rel(pen, out.hidden_states[-2]) <= 2e-5
    assert rel(pooled, out.text_embeds) <= 2e-5
    assert rel(last, out.last_hidden_state) <= 2e-5
