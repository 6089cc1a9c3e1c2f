"""Soft region weights on the GPU above the kernel: one SpatialTransformer level (one-hot weights against the hard RegionalContext,
bitwise; a feathered map against an fp32 torch composition), batchify_sample on both untiled samplers (region_feather=0 and one-hot
region_weights bitwise against the `regions=` call, a (1/2, 1/2) mix of two identical prompts bitwise against the single-prompt call,
num_samples = 2) and graph replay against the eager fused path with one captured graph serving another weight map and another region
count.  Networks, inputs and the ops.choose pin: those of test_regional_prompts_gpu.py."""
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
RECORD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "soft_regions", "kernel_error.json")


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


def _attn32(a, n, contexts, wts):
    """CrossAttention in fp32: contexts None = self-attention; else [NR, Tk, D] and wts [B, NR, T]: sum_e wts[b, e, t] * (token (b, t)'s
    full attention to entry e)."""
    H = a.heads
    q = _heads(F.linear(n, a.to_q.weight), H)
    if contexts is None:
        o = F.scaled_dot_product_attention(q, _heads(F.linear(n, a.to_k.weight), H), _heads(F.linear(n, a.to_v.weight), H))
    else:
        o = 0
        for e in range(contexts.shape[0]):
            c = contexts[e:e + 1].expand(n.shape[0], -1, -1)
            pe = F.scaled_dot_product_attention(q, _heads(F.linear(c, a.to_k.weight), H), _heads(F.linear(c, a.to_v.weight), H))
            o = o + pe * wts[:, e, None, :, None]
    o = o.permute(0, 2, 1, 3).reshape(n.shape[0], n.shape[1], H * 64)
    return F.linear(o, a.to_out[0].weight, a.to_out[0].bias)


def _st32(st, x, contexts, wts):
    """SpatialTransformer.forward in fp32 torch ops (sgm/modules/attention.py:614-635 with use_linear)."""
    B, C, Hh, Ww = x.shape
    t = F.group_norm(x, 32, st.norm.weight, st.norm.bias, 1e-6).permute(0, 2, 3, 1).reshape(B, Hh * Ww, C)
    t = F.linear(t, st.proj_in.weight, st.proj_in.bias)
    for blk in st.transformer_blocks:
        D = t.shape[-1]
        t = t + _attn32(blk.attn1, F.layer_norm(t, (D,), blk.norm1.weight, blk.norm1.bias, 1e-5), None, None)
        t = t + _attn32(blk.attn2, F.layer_norm(t, (D,), blk.norm2.weight, blk.norm2.bias, 1e-5), contexts, wts)
        g = F.linear(F.layer_norm(t, (D,), blk.norm3.weight, blk.norm3.bias, 1e-5), blk.ff.net[0].proj.weight, blk.ff.net[0].proj.bias)
        a, gate = g.chunk(2, dim=-1)
        t = t + F.linear(a * F.gelu(gate), blk.ff.net[2].weight, blk.ff.net[2].bias)
    t = F.linear(t, st.proj_out.weight, st.proj_out.bias)
    return t.reshape(B, Hh, Ww, C).permute(0, 3, 1, 2) + x


def _one_hot(ids, NR):
    """ids [B, h, w] uint8 -> [B, NR, h, w] float32."""
    return torch.zeros((ids.shape[0], NR) + tuple(ids.shape[1:]), device=ids.device).scatter_(1, ids.long()[:, None], 1.0)


def test_one_transformer_level_with_soft_weights():
    """Depth 2, 640 channels, a 64 x 32 token grid (sixteen row blocks of the kernel per image), latent weights 128 x 64 read at ds = 2.
    One-hot weights: the hard RegionalContext's result, bitwise.  A left / right map feathered with radius 6 (the other way round on
    batch row 0): against the fp32 composition, cap 1.5 x the same module's measured single-prompt error against its fp32 counterpart
    on the same inputs (the existing level test's rule)."""
    B, C, Hh, Ww, NR = 2, 640, 64, 32, 3
    with torch.device(DEV):
        st = SpatialTransformer(C, C // 64, 64, depth=2, context_dim=2048, use_linear=True)
    fill_module(st, "model.diffusion_model.input_blocks.4.1.", DEV)
    x = T("rp.st.x", (B, C, Hh, Ww))
    bank = T("rp.st.bank", (NR, 77, 2048))
    lat = torch.ones(B, 2 * Hh, 2 * Ww, dtype=torch.uint8, device=DEV)
    lat[:, :, Ww:] = 2
    lat[0] = lat[0].flip(-1)
    soft = torch.zeros(B, NR, 2 * Hh, 2 * Ww, device=DEV)
    for b in range(B):
        soft[b, 1:] = S.feather_regions((lat[b] - 1).cpu(), 2, 6).to(DEV)
    assert (soft.sum(1) - 1).abs().max() < 1e-6
    with torch.no_grad(), Wt.compute_dtype(torch.bfloat16):
        hard = st(x, RegionalContext(bank, lat)).float()
        reg1 = RegionalContext(bank, lat, weights=_one_hot(lat, NR))
        ops.start_trace()
        try:
            one = st(x, reg1).float()
        finally:
            trace = ops.stop_trace()
        fused = [r for r in trace if r["kernel"] == "xattn_q_regions_soft"]      # one launch per text cross-attention: depth 2
        assert len(fused) == 2 and all((r["T"], r["C"], r["NR"]) == (Hh * Ww, C, NR) for r in fused), [r["kernel"] for r in trace]
        assert not [r for r in trace if r["kernel"] in ("xattn_q_regions", "xattn_q", "attn") and r.get("Tk") == 77]
        assert torch.equal(one, hard), "one-hot weights differ from the hard map"
        reg = RegionalContext(bank, soft.argmax(1).to(torch.uint8), weights=soft)
        out = st(x, reg).float()
        wts, span = reg.level_weights(Hh, Ww)
        assert reg.level_weights(Hh, Ww)[0] is wts and wts.shape == (B, NR, Hh * Ww) and span.shape == (B, Hh * Ww // 128, 2)
        assert torch.equal(wts.view(B, NR, Hh, Ww), soft[:, :, 1::2, 1::2])
        plain = st(x, bank[1:2].expand(B, -1, -1).contiguous()).float()
        ref = _st32(st, x, bank, wts)
        ref1 = _st32(st, x, bank, _one_hot(torch.ones_like(lat), NR)[:, :, 1::2, 1::2].reshape(B, NR, Hh * Ww))
    assert torch.isfinite(out).all()
    e_soft, e_one = rel_l2(out, ref), rel_l2(plain, ref1)
    print(f"[soft level] rel-L2 vs fp32: feathered two regions {e_soft:.4e}, single prompt {e_one:.4e} (cap 1.5 x)")
    record("spatial_transformer_depth2_64x32_C640", rel_l2_vs_fp32_feathered=e_soft, rel_l2_vs_fp32_single_prompt=e_one)
    assert e_soft <= 1.5 * e_one, (e_soft, e_one)
    assert not torch.equal(out, hard)


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


def _sample(model, kind, cond, ns=1, img="rp.img", **regional):
    x = T(img, (1, 3, 8 * LAT, 8 * LAT), scale=0.5).clamp(-1, 1)
    rep = lambda name: T(name, (1, 4, LAT, LAT)).repeat(ns, 1, 1, 1)   # noqa: E731
    noises = {"posterior": rep("rp.post"), "init": rep("rp.init")}
    if kind == "edm":
        noises["steps"] = [rep(f"rp.eps{i}") for i in range(STEPS)]
    kw = dict(num_steps=STEPS, restoration_scale=4.0, s_churn=5, s_noise=1.01, cfg_scale=4.0, control_scale=1.0, seed=1234,
              use_linear_CFG=True, cfg_scale_start=1.0, return_intermediates=True, num_samples=ns)
    with torch.no_grad():
        out, mid = model.batchify_sample(x, cond=cond, noises=noises, **kw, **regional)
    assert torch.isfinite(out).all()
    return mid["samples"].clone()


def _left_right(R=2):
    m = torch.zeros(LAT, LAT, dtype=torch.int64)
    for r in range(1, R):
        m[:, r * LAT // R:] = r
    return m


@pytest.mark.parametrize("kind", ["edm", "dpmpp"])
def test_batchify_sample_with_soft_weights(model, kind, monkeypatch):
    """Eager fused path (graphs off).  region_feather=0 and one-hot region_weights = the `regions=` call, bitwise; (1/2, 1/2) over two
    identical prompts = the single-prompt call, bitwise (the mix is exact); a feathered map differs from the hard one."""
    monkeypatch.setattr(S, "FUSED_EDM_STEP", True)
    monkeypatch.setattr(S, "EMB_SCHEDULE", True)
    _use(model, kind)
    model.model.enable_graph(False)
    cs, uc = _conds(2)
    m = _left_right(2)
    hard = _sample(model, kind, ([cs[0], cs[1]], uc), regions=m)
    assert torch.equal(_sample(model, kind, ([cs[0], cs[1]], uc), regions=m, region_feather=0), hard)
    assert torch.equal(_sample(model, kind, ([cs[0], cs[1]], uc), region_weights=S.feather_regions(m, 2, 0)), hard)
    single = _sample(model, kind, (cs[0], uc))
    half = _sample(model, kind, ([cs[0], cs[0]], uc), region_weights=torch.full((2, LAT, LAT), 0.5))
    assert torch.equal(half, single)
    soft = _sample(model, kind, ([cs[0], cs[1]], uc), regions=m, region_feather=3)
    d = rel_l2(soft, hard)
    print(f"[soft e2e {kind}] feather 3 vs the hard map: rel-L2 {d:.3e}")
    assert d > 0


def test_num_samples_two_rows_carry_the_same_weights(model, monkeypatch):
    """num_samples = 2: the unconditional rows have weight 1 on entry 0, both conditional rows the region weights on entries 1 + r."""
    monkeypatch.setattr(S, "FUSED_EDM_STEP", True)
    monkeypatch.setattr(S, "EMB_SCHEDULE", True)
    _use(model, "edm")
    model.model.enable_graph(False)
    cs, uc = _conds(2)
    w = S.feather_regions(_left_right(2), 2, 2)
    seen = []
    hook = model.model.register_forward_pre_hook(lambda mod, args: seen.append(args[2]["regions"].weights.clone()))
    try:
        out = _sample(model, "edm", ([cs[0], cs[1]], uc), ns=2, region_weights=w)
    finally:
        hook.remove()
    wts = seen[0]
    assert tuple(wts.shape) == (4, 3, LAT, LAT)
    assert wts[:2, 0].eq(1).all() and wts[:2, 1:].eq(0).all() and wts[2:, 0].eq(0).all()
    assert torch.equal(wts[2, 1:], w.to(DEV)) and torch.equal(wts[3, 1:], w.to(DEV))
    assert out.shape[0] == 2
    e = rel_l2(out[0:1], out[1:2])
    print(f"[soft num_samples=2] sample 0 vs sample 1: rel-L2 {e:.3e}")
    assert e <= 1e-2          # identical noise, prompts and weights on both rows (the bar of the hard test)


@pytest.mark.parametrize("kind", ["edm", "dpmpp"])
def test_graph_replay_equals_eager_and_one_graph_serves_other_weights(model, kind, monkeypatch):
    """Two images with three and with two regions (both inside the bank's capacity of 4 entries), other weight maps, other pictures.
    Under graph replay the second re-uses the first's graph (the capture counter does not move), and both equal their own eager
    fused runs bitwise -- also at the 8 x 8 = 64-token level, which runs the per-entry loop whose launches were captured on image A."""
    monkeypatch.setattr(S, "FUSED_EDM_STEP", True)
    monkeypatch.setattr(S, "EMB_SCHEDULE", True)
    _use(model, kind)
    cs, uc = _conds(3)
    w4 = S.region_weights_from_tiles(LAT, LAT, 24, 8)        # 2 x 2 windows: the left and the right column of tiles as two regions
    calls = {"a": dict(cond=([cs[0], cs[1], cs[2]], uc), region_weights=S.feather_regions(_left_right(3), 3, 2), img="rp.img"),
             "b": dict(cond=([cs[2], cs[0]], uc), region_weights=torch.stack([w4[0] + w4[2], w4[1] + w4[3]]), img="rp.img2")}
    model.model._region_slots.clear()          # the capacity is decided by the first image of this test
    model.model.enable_graph(True)
    try:
        ga = _sample(model, kind, **calls["a"])
        after_a = model.model.graph_stats()
        gb = _sample(model, kind, **calls["b"])
        after_b = model.model.graph_stats()
    finally:
        model.model.enable_graph(False)
    print(f"[soft graph {kind}] graph stats after image A {after_a}, after image B {after_b}")
    assert after_a["captures"] == 1 and after_a["eager"] == 0 and after_a["replays"] == STEPS
    assert after_b["captures"] == after_a["captures"] and after_b["eager"] == 0 and after_b["replays"] == 2 * STEPS
    ea = _sample(model, kind, **calls["a"])
    eb = _sample(model, kind, **calls["b"])
    assert torch.equal(ga, ea) and torch.equal(gb, eb)
    assert not torch.equal(ga, gb)
