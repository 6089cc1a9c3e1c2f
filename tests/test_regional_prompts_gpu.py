"""Regional prompts on the GPU above the kernel: one SpatialTransformer level against an fp32 torch composition, batchify_sample on
both untiled samplers (bitwise against the single-prompt call where the prompts agree), graph replay against the eager fused path with
one captured graph serving another map and another region count, and num_samples = 2.  Networks: the reduced-depth ones the other GPU
tests build.  The pick between the fused and the two-launch text attention of a PLAIN call is forced to the fused form, so that plain
and regional calls run the same arithmetic (the regional branch always takes the fused kernel where its shape allows)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from supir_amd import ops  # noqa: E402
from supir_amd import weights as Wt  # noqa: E402
from supir_amd.modules import sampling as S  # noqa: E402
from supir_amd.modules.attention import RegionalContext, SpatialTransformer  # noqa: E402
from tests.helpers import fill_module, rel_l2, synth_tensor  # noqa: E402

DEV = "cuda"
RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "regional_prompts", "kernel_error.json")


def T(name, shape, **kw):
    return synth_tensor(name, shape, **kw).to(DEV)


def record(key, **values):
    try:
        os.makedirs(os.path.dirname(RECORD), exist_ok=True)
        data = {}
        if os.path.exists(RECORD):
            with open(RECORD) as f:
                data = json.load(f)
        data[key] = values
        with open(RECORD, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


@pytest.fixture(autouse=True)
def fused_text_attention(monkeypatch):
    real = ops.choose
    monkeypatch.setattr(ops, "choose", lambda key, fns, **kw: 1 if key[0] == "xattn" else real(key, fns, **kw))


# ------------------------------------------------------------------------------------------------ one transformer level
def _heads(t, H):
    return t.reshape(t.shape[0], t.shape[1], H, 64).permute(0, 2, 1, 3)


def _attn32(a, n, contexts, ids):
    """CrossAttention in fp32: contexts None = self-attention; else [NR, Tk, D] with every token attending to entry ids[b, t]."""
    H = a.heads
    q = _heads(F.linear(n, a.to_q.weight), H)
    if contexts is None:
        o = F.scaled_dot_product_attention(q, _heads(F.linear(n, a.to_k.weight), H), _heads(F.linear(n, a.to_v.weight), H))
    else:
        per = []
        for e in range(contexts.shape[0]):                  # full attention per entry, then the per-token select
            c = contexts[e:e + 1].expand(n.shape[0], -1, -1)
            per.append(F.scaled_dot_product_attention(q, _heads(F.linear(c, a.to_k.weight), H), _heads(F.linear(c, a.to_v.weight), H)))
        per = torch.stack(per)                              # [NR, B, H, T, 64]
        o = torch.gather(per, 0, ids[None, :, None, :, None].expand(1, -1, H, -1, 64))[0]
    o = o.permute(0, 2, 1, 3).reshape(n.shape[0], n.shape[1], H * 64)
    return F.linear(o, a.to_out[0].weight, a.to_out[0].bias)


def _st32(st, x, contexts, ids):
    """SpatialTransformer.forward in fp32 torch ops (sgm/modules/attention.py:614-635 with use_linear)."""
    B, C, Hh, Ww = x.shape
    t = F.group_norm(x, 32, st.norm.weight, st.norm.bias, 1e-6).permute(0, 2, 3, 1).reshape(B, Hh * Ww, C)
    t = F.linear(t, st.proj_in.weight, st.proj_in.bias)
    for blk in st.transformer_blocks:
        D = t.shape[-1]
        t = t + _attn32(blk.attn1, F.layer_norm(t, (D,), blk.norm1.weight, blk.norm1.bias, 1e-5), None, None)
        t = t + _attn32(blk.attn2, F.layer_norm(t, (D,), blk.norm2.weight, blk.norm2.bias, 1e-5), contexts, ids)
        g = F.linear(F.layer_norm(t, (D,), blk.norm3.weight, blk.norm3.bias, 1e-5), blk.ff.net[0].proj.weight, blk.ff.net[0].proj.bias)
        a, gate = g.chunk(2, dim=-1)
        t = t + F.linear(a * F.gelu(gate), blk.ff.net[2].weight, blk.ff.net[2].bias)
    t = F.linear(t, st.proj_out.weight, st.proj_out.bias)
    return t.reshape(B, Hh, Ww, C).permute(0, 3, 1, 2) + x


def test_one_transformer_level_with_a_left_right_map():
    """Depth 2, 640 channels, a 64 x 32 token grid (2048 tokens: sixteen row blocks of the kernel per image), latent map 128 x 64 read
    at ds = 2.  Cap: 1.5 x the same module's measured single-prompt error against its fp32 counterpart on the same inputs -- K / V of
    two prompts instead of one is the only new rounding source."""
    B, C, Hh, Ww, NR = 2, 640, 64, 32, 3
    with torch.device(DEV):
        st = SpatialTransformer(C, C // 64, 64, depth=2, context_dim=2048, use_linear=True)
    fill_module(st, "model.diffusion_model.input_blocks.4.1.", DEV)
    x = T("rp.st.x", (B, C, Hh, Ww))
    bank = T("rp.st.bank", (NR, 77, 2048))
    lat = torch.ones(B, 2 * Hh, 2 * Ww, dtype=torch.uint8, device=DEV)
    lat[:, :, Ww:] = 2                                      # left half region 1, right half region 2 (latent columns Ww .. 2 Ww - 1)
    lat[0] = lat[0].flip(-1)                                # the other way round on batch row 0
    reg = RegionalContext(bank, lat)
    with torch.no_grad(), Wt.compute_dtype(torch.bfloat16):
        ops.start_trace()
        try:
            out = st(x, reg).float()
        finally:
            trace = ops.stop_trace()
        fused = [r for r in trace if r["kernel"] == "xattn_q_regions"]      # one launch per text cross-attention: depth 2
        assert len(fused) == 2 and all((r["T"], r["C"], r["NR"]) == (Hh * Ww, C, NR) for r in fused), [r["kernel"] for r in trace]
        ids = reg.level_ids(Hh, Ww)
        assert reg.level_ids(Hh, Ww) is ids and ids.shape == (B, Hh * Ww)
        assert torch.equal(ids.view(B, Hh, Ww), lat[:, 1::2, 1::2])
        plain = {r: st(x, bank[r:r + 1].expand(B, -1, -1).contiguous()).float() for r in (1, 2)}
        const = {r: st(x, RegionalContext(bank, torch.full_like(lat, r))).float() for r in (1, 2)}
        ref = _st32(st, x, bank, ids.long())
        ref1 = _st32(st, x, bank, torch.ones_like(ids).long())
    assert torch.isfinite(out).all()
    for r in (1, 2):
        assert torch.equal(const[r], plain[r]), f"map constant at {r} differs from the plain call with prompt {r}"
    e_reg, e_one = rel_l2(out, ref), rel_l2(plain[1], ref1)
    print(f"[regional level] rel-L2 vs fp32: two regions {e_reg:.4e}, single prompt {e_one:.4e} (cap 1.5 x)")
    record("spatial_transformer_depth2_64x32_C640", rel_l2_vs_fp32_two_regions=e_reg, rel_l2_vs_fp32_single_prompt=e_one)
    assert e_reg <= 1.5 * e_one, (e_reg, e_one)
    assert not torch.equal(out, plain[1]) and not torch.equal(out, plain[2])
    # the halves follow their prompts: where the map says r, the result is nearer the plain call with prompt r than the other one
    half = out[1, :, :, :Ww // 2]
    assert rel_l2(half, plain[1][1, :, :, :Ww // 2]) < rel_l2(half, plain[2][1, :, :, :Ww // 2])


@pytest.mark.parametrize("how", ["fp32_service", "no_layernorm_fold"])
def test_one_transformer_level_on_the_plain_path(how, monkeypatch):
    """The paths without the fused kernel -- the fp32 service, and bf16 with FOLD_LAYERNORM off -- project, run the existing attention
    once per entry and select (ops.attn_regions).  16 x 16 tokens, depth 1, three regions in stripes.  Bounds: fp32 against the fp32
    composition 1e-5 (what smoke() holds the fp32 service to on a whole network call); bf16 1.5 x the single-prompt error of the same
    path, as in the test above."""
    from supir_amd.modules import attention as A
    B, C, Hh, Ww, NR = 2, 640, 16, 16, 4
    with torch.device(DEV):
        st = SpatialTransformer(C, C // 64, 64, depth=1, context_dim=2048, use_linear=True)
    fill_module(st, "model.diffusion_model.input_blocks.5.1.", DEV)
    x, bank = T("rp.st.x16", (B, C, Hh, Ww)), T("rp.st.bank4", (NR, 77, 2048))
    lat = (1 + (torch.arange(2 * Ww, device=DEV) * 3 // (2 * Ww))).to(torch.uint8)[None, None, :].expand(B, 2 * Hh, -1).contiguous()
    reg = RegionalContext(bank, lat)
    dt = torch.float32 if how == "fp32_service" else torch.bfloat16
    if how == "no_layernorm_fold":
        monkeypatch.setattr(A, "FOLD_LAYERNORM", False)
    with torch.no_grad(), Wt.compute_dtype(dt):
        ops.start_trace()
        try:
            out = st(x, reg).float()
        finally:
            trace = ops.stop_trace()
        assert not [r for r in trace if r["kernel"] == "xattn_q_regions"]
        one = st(x, bank[1:2].expand(B, -1, -1).contiguous()).float()
        ids = reg.level_ids(Hh, Ww).long()
        ref, ref1 = _st32(st, x, bank, ids), _st32(st, x, bank, torch.ones_like(ids))
    e, e1 = rel_l2(out, ref), rel_l2(one, ref1)
    print(f"[regional level, {how}] rel-L2 vs fp32: three regions {e:.4e}, single prompt {e1:.4e}")
    assert torch.isfinite(out).all() and set(ids.unique().tolist()) == {1, 2, 3}
    assert e <= (1e-5 if how == "fp32_service" else 1.5 * e1), (e, e1)


# ------------------------------------------------------------------------------------------------ whole model
LAT, STEPS = 32, 2


@pytest.fixture(scope="module")
def model():
    """SUPIRModel as bench.py builds it (supir_v0_config through the plugin) at transformer depth [1, 1, 2], synthetic weights."""
    from supir_amd.configs import supir_v0_config
    from supir_amd.plugin import instantiate_from_config
    from supir_amd.synth import synth_param
    with torch.device(DEV):
        m = instantiate_from_config(supir_v0_config(transformer_depth=[1, 1, 2], sampler_device=DEV))
    with torch.no_grad():
        for k, t in m.state_dict().items():
            if t.is_floating_point() and k != "denoiser.sigmas":
                t.copy_(synth_param(k, t.shape, device=DEV))
    return m


def _use(model, kind):
    from supir_amd.configs import supir_v0_config
    name = "RestoreEDMSampler" if kind == "edm" else "RestoreDPMPP2MSampler"
    model.sampler_config = supir_v0_config(sampler=name, sampler_device=DEV)["params"]["sampler_config"]


def _conds(n, ns=1):
    cs = [{"crossattn": T(f"rp.ctx{j}", (1, 77, 2048)).repeat(ns, 1, 1), "vector": T("rp.vec", (1, 2816)).repeat(ns, 1)} for j in range(n)]
    uc = {"crossattn": T("rp.uctx", (1, 77, 2048)).repeat(ns, 1, 1), "vector": T("rp.uvec", (1, 2816)).repeat(ns, 1)}
    return cs, uc


def _sample(model, kind, cond, regions=None, ns=1, img="rp.img"):
    x = T(img, (1, 3, 8 * LAT, 8 * LAT), scale=0.5).clamp(-1, 1)
    noises = {"posterior": T("rp.post", (ns, 4, LAT, LAT)), "init": T("rp.init", (ns, 4, LAT, LAT))}
    if kind == "edm":
        noises["steps"] = [T(f"rp.eps{i}", (ns, 4, LAT, LAT)) for i in range(STEPS)]
    kw = dict(num_steps=STEPS, restoration_scale=4.0, s_churn=5, s_noise=1.01, cfg_scale=4.0, control_scale=1.0, seed=1234,
              use_linear_CFG=True, cfg_scale_start=1.0, return_intermediates=True, num_samples=ns)
    if regions is not None:
        kw["regions"] = regions
    with torch.no_grad():
        out, mid = model.batchify_sample(x, cond=cond, noises=noises, **kw)
    assert torch.isfinite(out).all()
    return mid["samples"].clone()


def _left_right(R=2):
    m = torch.zeros(LAT, LAT, dtype=torch.int64)
    for r in range(1, R):
        m[:, r * LAT // R:] = r
    return m


@pytest.mark.parametrize("kind", ["edm", "dpmpp"])
def test_batchify_sample_with_regions(model, kind, monkeypatch):
    """Three identical prompts on any map = the single-prompt call, bitwise; two different prompts on a left / right map differ from
    both single-prompt results.  Eager fused path (graphs off)."""
    monkeypatch.setattr(S, "FUSED_EDM_STEP", True)
    monkeypatch.setattr(S, "EMB_SCHEDULE", True)
    _use(model, kind)
    model.model.enable_graph(False)
    cs, uc = _conds(2)
    single = {j: _sample(model, kind, (cs[j], uc)) for j in (0, 1)}
    same = _sample(model, kind, ([cs[0], cs[0], cs[0]], uc), regions=_left_right(3))
    assert torch.equal(same, single[0])
    two = _sample(model, kind, ([cs[0], cs[1]], uc), regions=[(0, LAT, 0, LAT), (0, LAT, LAT // 2, LAT)])
    assert not torch.equal(two, single[0]) and not torch.equal(two, single[1])
    d0, d1 = rel_l2(two, single[0]), rel_l2(two, single[1])
    print(f"[regional e2e {kind}] left / right prompts vs the single-prompt runs: rel-L2 {d0:.3e} / {d1:.3e}; "
          f"the two single-prompt runs apart: {rel_l2(single[0], single[1]):.3e}")
    assert d0 > 0 and d1 > 0


@pytest.mark.parametrize("order", ["fewer_regions_second", "more_regions_second"])
@pytest.mark.parametrize("kind", ["edm", "dpmpp"])
def test_graph_replay_equals_eager_and_one_graph_serves_another_map(model, kind, order, monkeypatch):
    """Two images with three and with two regions (both inside the bank's capacity of 4 entries), other maps, other pictures, in
    either order.  Under graph replay the second re-uses the first's graph (the wrapper's capture counter does not move), and both
    equal their own eager fused runs bitwise -- also at the 8 x 8 = 64-token level, which runs the per-entry attention loop whose
    launches were captured on the first image."""
    monkeypatch.setattr(S, "FUSED_EDM_STEP", True)
    monkeypatch.setattr(S, "EMB_SCHEDULE", True)
    _use(model, kind)
    cs, uc = _conds(3)
    map_a = _left_right(3)
    map_b = _left_right(2).t().contiguous()                  # top / bottom
    calls = {"a": dict(cond=([cs[0], cs[1], cs[2]], uc), regions=map_a, img="rp.img"),
             "b": dict(cond=([cs[2], cs[0]], uc), regions=map_b, img="rp.img2")}
    if order == "more_regions_second":
        calls = {"a": calls["b"], "b": calls["a"]}
    model.model._region_slots.clear()          # the capacity is decided by the first image of this test
    model.model.enable_graph(True)
    try:
        ga = _sample(model, kind, **calls["a"])
        after_a = model.model.graph_stats()
        gb = _sample(model, kind, **calls["b"])
        after_b = model.model.graph_stats()
    finally:
        model.model.enable_graph(False)
    print(f"[regional graph {kind}] graph stats after image A {after_a}, after image B {after_b}")
    assert after_a["captures"] == 1 and after_a["eager"] == 0 and after_a["replays"] == STEPS
    assert after_b["captures"] == after_a["captures"] and after_b["eager"] == 0 and after_b["replays"] == 2 * STEPS
    ea = _sample(model, kind, **calls["a"])
    eb = _sample(model, kind, **calls["b"])
    assert torch.equal(ga, ea) and torch.equal(gb, eb)
    assert not torch.equal(ga, gb)


def test_num_samples_two_rows_see_the_same_map(model, monkeypatch):
    """num_samples = 2: both rows of the conditional half carry the same map (1 + region), the unconditional rows entry 0.  With identical
    per-sample noise the two samples then agree to the bar the project holds two evaluation orders of one trajectory to (1e-2,
    tests/test_sampler_fused_gpu.py): they ran the same prompts on the same regions."""
    monkeypatch.setattr(S, "FUSED_EDM_STEP", True)
    monkeypatch.setattr(S, "EMB_SCHEDULE", True)
    _use(model, "edm")
    model.model.enable_graph(False)
    cs, uc = _conds(2)
    seen = []
    hook = model.model.register_forward_pre_hook(lambda mod, args: seen.append(args[2]["regions"].ids.clone()))
    try:
        with torch.no_grad():
            x = T("rp.img", (1, 3, 8 * LAT, 8 * LAT), scale=0.5).clamp(-1, 1)
            rep = lambda name: T(name, (1, 4, LAT, LAT)).repeat(2, 1, 1, 1)   # noqa: E731
            noises = {"posterior": rep("rp.post"), "init": rep("rp.init"), "steps": [rep(f"rp.eps{i}") for i in range(STEPS)]}
            out, mid = model.batchify_sample(x, cond=([cs[0], cs[1]], uc), noises=noises, num_steps=STEPS, restoration_scale=4.0, s_churn=5,
                                             s_noise=1.01, cfg_scale=4.0, seed=1234, use_linear_CFG=True, cfg_scale_start=1.0,
                                             return_intermediates=True, num_samples=2, regions=_left_right(2))
    finally:
        hook.remove()
    ids = seen[0]
    want = (_left_right(2) + 1).to(torch.uint8).to(DEV)
    assert tuple(ids.shape) == (4, LAT, LAT) and ids[:2].eq(0).all() and torch.equal(ids[2], want) and torch.equal(ids[3], want)
    assert out.shape[0] == 2 and torch.isfinite(out).all()
    e = rel_l2(mid["samples"][0:1], mid["samples"][1:2])
    print(f"[regional num_samples=2] sample 0 vs sample 1: rel-L2 {e:.3e}")
    assert e <= 1e-2
