"""Soft region weights on the untiled samplers, host side (no GPU): the weight helpers (region_weights, feather_regions,
region_weights_from_tiles), the level tables and spans, the guiders' row layout, the refusals, the modules' routing with CPU stand-ins
for the new op (they live here and are monkeypatched in), and batchify_sample's routing with stand-in networks."""
import numpy as np
import pytest
import torch

from supir_amd import ops
from supir_amd.modules import sampling as S
from supir_amd.modules.attention import RegionalContext, SpatialTransformer, level_region_ids, level_region_weights, region_span


def one_hot(m, R):
    return torch.zeros(R, *m.shape).scatter_(0, m.long()[None], 1.0)


# ------------------------------------------------------------------------------------------------ weights
def test_region_weights_normalises_and_keeps_one_hot_exact():
    g = torch.Generator().manual_seed(3)
    raw = torch.rand(3, 6, 5, generator=g) * 7.0
    w = S.region_weights(raw, 3, 6, 5)
    assert w.dtype == torch.float32 and tuple(w.shape) == (3, 6, 5) and w.is_contiguous()
    assert torch.allclose(w.double(), raw.double() / raw.double().sum(0, keepdim=True), atol=1e-7) and (w.sum(0) - 1).abs().max() < 1e-6
    assert torch.equal(S.region_weights(raw.numpy(), 3, 6, 5), w)                 # arrays too
    m = (torch.arange(30).reshape(6, 5) * 7) % 3
    oh = one_hot(m, 3)
    assert torch.equal(S.region_weights(oh, 3, 6, 5), oh)                         # exactly one-hot, not 0.99999
    assert torch.equal(S.region_weights(oh * 5.0, 3, 6, 5), oh)


def test_region_weights_checks():
    ok = torch.ones(2, 4, 4)
    for bad, R in [(torch.ones(4, 4), 2), (torch.ones(2, 4, 5), 2), (torch.ones(1, 2, 4, 4), 2),      # rank / size
                   (torch.ones(3, 4, 4), 2),                                                            # R not the prompts'
                   (ok * float("nan"), 2), (ok * float("inf"), 2), (-ok, 2),                            # non-finite, negative
                   (torch.zeros(2, 4, 4), 2),                                                           # a pixel without weight
                   ([[1.0]], 1)]:                                                                       # not a tensor or array
        with pytest.raises(ValueError):
            S.region_weights(bad, R, 4, 4)
    z = ok.clone()
    z[:, 2, 3] = 0.0
    with pytest.raises(ValueError, match="no weight"):
        S.region_weights(z, 2, 4, 4)
    with pytest.raises(ValueError, match="254"):
        S.region_weights(torch.ones(255, 2, 2), 255, 2, 2)
    assert S.region_weights(torch.ones(254, 2, 2), 254, 2, 2).shape == (254, 2, 2)


def test_feather_regions():
    m = torch.zeros(16, 20, dtype=torch.int64)
    m[:, 10:] = 1                                            # a straight vertical border between columns 9 and 10
    assert torch.equal(S.feather_regions(m, 2, 0), one_hot(m, 2))
    for radius in (1, 3):
        w = S.feather_regions(m, 2, radius)
        assert w.dtype == torch.float32 and tuple(w.shape) == (2, 16, 20)
        assert (w.sum(0) - 1).abs().max() < 1e-6 and w.min() >= 0
        assert torch.equal(w[0], w[1].flip(-1))              # symmetric across the border
        k = 2 * radius + 1
        for x in range(20):                                  # the box filter: the share of the window's columns (replicated at the edge) left of the border
            cols = np.clip(np.arange(x - radius, x + radius + 1), 0, 19)
            assert abs(float(w[0, 5, x]) - float((cols < 10).sum()) / k) < 1e-6
        assert torch.equal(w[:, :, :10 - radius], one_hot(m, 2)[:, :, :10 - radius])      # unchanged away from the border
        assert torch.equal(w[:, :, 10 + radius:], one_hot(m, 2)[:, :, 10 + radius:])
    # a radius larger than the grid is still a distribution; three regions, a corner
    m3 = torch.zeros(6, 6, dtype=torch.int64)
    m3[3:, :] = 1
    m3[4:, 4:] = 2
    w = S.feather_regions(m3, 3, 9)
    assert (w.sum(0) - 1).abs().max() < 1e-6 and (w > 0).all()
    with pytest.raises(ValueError):
        S.feather_regions(m, 2, -1)
    with pytest.raises(ValueError):
        S.feather_regions(m.float(), 2, 1)                   # region_map's rules: integer maps
    with pytest.raises(ValueError):
        S.feather_regions(m, 1, 1)                           # the map names more regions than R


SIZES = [(h, w) for h in range(128, 321, 32) for w in range(128, 321, 32)]


@pytest.mark.parametrize("h,w,tile,stride", [(h, w, 128, 64) for h, w in SIZES] + [(96, 200, 64, 48)])
def test_region_weights_from_tiles_are_the_tiled_samplers_blend_weights(h, w, tile, stride):
    tiles = S._sliding_windows(h, w, tile, stride)
    wt = S.region_weights_from_tiles(h, w, tile, stride)
    assert wt.dtype == torch.float32 and tuple(wt.shape) == (len(tiles), h, w)
    assert (wt.sum(0) - 1).abs().max() < 1e-6 and wt.min() >= 0
    g = S.gaussian_weights(tile, tile, 1, device="cpu")                          # [1, 4, tile, tile] float64
    count = S._TileGroups._count_canvas(torch.zeros(1, 4, h, w, dtype=torch.float64), tiles, g)
    for j, (a, b, c, d) in enumerate(tiles):
        outside = torch.ones(h, w, dtype=torch.bool)
        outside[a:b, c:d] = False
        assert wt[j][outside].eq(0).all()                                        # no weight outside its window
        want = g[0, 0] / count[0, 0, a:b, c:d]                                   # the share of tile j in the blended canvas
        assert torch.allclose(wt[j, a:b, c:d].double(), want, rtol=0, atol=1e-7)
    assert torch.equal(S.region_weights(wt, len(tiles), h, w).argmax(0), wt.argmax(0))       # accepted as region_weights as it is


# ------------------------------------------------------------------------------------------------ level tables
def _weights8(B=2, cap=4, n=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(B, cap, 8, 16, generator=g)
    w[:, n:] = 0.0                                           # capacity padding: entries >= n carry no weight
    w[0, 0, :, :8] = 0.0                                     # batch row 0: entry 0 unused in the left half
    w[1, 1:, 4:, :] = 0.0                                    # batch row 1: only entry 0 in the lower half
    return (w / w.sum(1, keepdim=True)).contiguous()


@pytest.mark.parametrize("ds", [1, 2, 4])
def test_level_weights_follow_the_centre_pixel_rule_of_the_ids(ds):
    w = _weights8()
    H, W = 8 // ds, 16 // ds
    wts, span = level_region_weights(w, H, W)
    assert wts.dtype == torch.float32 and wts.shape == (2, 4, H * W) and wts.is_contiguous()
    for b in range(2):
        for y in range(H):
            for x in range(W):
                assert torch.equal(wts[b, :, y * W + x], w[b, :, y * ds + ds // 2, x * ds + ds // 2])
    assert (span is None) == ((H * W) % 128 != 0)
    # one-hot weights mean what the hard ids mean, at every level
    ids = w.argmax(1).to(torch.uint8)
    oh = torch.zeros_like(w).scatter_(1, ids.long()[:, None], 1.0)
    assert torch.equal(level_region_weights(oh, H, W)[0].argmax(1).to(torch.uint8), level_region_ids(ids, H, W))
    with pytest.raises(ValueError):
        level_region_weights(w, 3, 3)


def test_span_against_a_brute_force_loop():
    g = torch.Generator().manual_seed(5)
    B, NR, Tn = 2, 6, 512
    w = torch.rand(B, NR, Tn, generator=g)
    w[:, 4:] = 0.0                                           # capacity padding
    w[0, :2, :128] = 0.0                                     # block 0 of row 0 starts at entry 2
    w[0, 1:, 128:256] = 0.0                                  # block 1: entry 0 alone
    w[1, 1:3, 256:384] = 0.0                                 # block 2 of row 1: entries 0 and 3, a hole between
    w[1, :, 384:] = 0.0
    w[1, 3, 400] = 1e-6                                      # block 3: one token, one entry
    span = region_span(w)
    assert span.dtype == torch.uint8 and span.shape == (B, Tn // 128, 2) and span.is_contiguous()
    for b in range(B):
        for blk in range(Tn // 128):
            used = [e for e in range(NR) if bool((w[b, e, blk * 128:(blk + 1) * 128] > 0).any())]
            assert span[b, blk].tolist() == [min(used), max(used)], (b, blk)
    assert region_span(torch.zeros(1, 3, 128)).tolist() == [[[0, 0]]]            # no weight at all: a valid single entry


def test_regional_context_keeps_its_weight_tables_and_refreshes_them_in_place():
    w = _weights8(cap=4, n=3)
    w16 = w.repeat(1, 1, 2, 1)                               # 16 x 16 latent: the 16 x 16 level has 256 tokens (a span), the 8 x 8 level none
    rc = RegionalContext(torch.zeros(4, 77, 8), w16.argmax(1).to(torch.uint8), n=3, weights=w16)
    wts, span = rc.level_weights(16, 16)
    wts8, span8 = rc.level_weights(8, 8)
    assert rc.level_weights(16, 16)[0] is wts and rc.level_weights(16, 16)[1] is span and span8 is None and span is not None
    assert torch.equal(span, region_span(wts)) and wts[:, 3].eq(0).all()
    o = _weights8(cap=2, n=2, seed=9).repeat(1, 1, 2, 1)
    other = RegionalContext(torch.ones(2, 77, 8), o.argmax(1).to(torch.uint8), weights=o)
    ptrs = (wts.data_ptr(), span.data_ptr(), wts8.data_ptr(), rc.weights.data_ptr(), rc.bank.data_ptr())
    rc.load(other)
    assert rc.level_weights(16, 16)[0] is wts and rc.level_weights(16, 16)[1] is span and rc.level_weights(8, 8)[0] is wts8
    assert (wts.data_ptr(), span.data_ptr(), wts8.data_ptr(), rc.weights.data_ptr(), rc.bank.data_ptr()) == ptrs and rc.n == 2
    assert torch.equal(rc.weights[:, :2], o) and rc.weights[:, 2:].eq(0).all()   # capacity padding stays zero
    want, want_span = level_region_weights(rc.weights, 16, 16)
    assert torch.equal(wts, want) and torch.equal(span, want_span) and int(span.max()) <= 1
    assert torch.equal(wts8, level_region_weights(rc.weights, 8, 8)[0])
    v = rc.weights._version
    rc.load(other)                                           # unchanged source: nothing is written
    assert rc.weights._version == v
    with pytest.raises(ValueError):                          # a soft context does not take a hard one, nor the other way round
        rc.load(RegionalContext(torch.ones(2, 77, 8), o.argmax(1).to(torch.uint8)))
    with pytest.raises(ValueError):
        RegionalContext(torch.ones(2, 77, 8), o.argmax(1).to(torch.uint8)).load(other)
    with pytest.raises(ValueError):                          # weights of another capacity than the bank
        RegionalContext(torch.ones(3, 77, 8), o.argmax(1).to(torch.uint8), weights=o)
    with pytest.raises(ValueError):
        RegionalContext(torch.ones(2, 77, 8), o.argmax(1).to(torch.uint8), weights=o.double())


def test_wrapper_slot_keys_hard_and_soft_apart():
    from supir_amd.modules.wrappers import ControlWrapper
    wrap = ControlWrapper.__new__(ControlWrapper)
    wrap._region_slots = {}
    w = _weights8(cap=3, n=3)
    ids = w.argmax(1).to(torch.uint8)
    hard, soft = RegionalContext(torch.ones(3, 77, 8), ids), RegionalContext(torch.ones(3, 77, 8), ids, weights=w)
    sh, ss = wrap._regions_slot(hard), wrap._regions_slot(soft)
    assert sh is not ss and sh.weights is None and ss.weights is not None and len(wrap._region_slots) == 2
    assert ss.cap == 4 and tuple(ss.weights.shape) == (2, 4, 8, 16)
    assert torch.equal(ss.weights[:, :3], w) and ss.weights[:, 3].eq(0).all()
    assert wrap._regions_slot(soft) is ss and wrap._regions_slot(hard) is sh
    w2 = _weights8(cap=2, n=2, seed=4)
    assert wrap._regions_slot(RegionalContext(torch.ones(2, 77, 8), ids.clamp(max=1), weights=w2)) is ss      # fewer regions: the same slot
    assert ss.n == 2 and torch.equal(ss.weights[:, :2], w2) and ss.weights[:, 2:].eq(0).all()


# ------------------------------------------------------------------------------------------------ guiders
def _spec(R=2, ns=1, h=4, w=4):
    g = torch.Generator().manual_seed(R)
    wt = S.region_weights(torch.rand(R, h, w, generator=g) + 0.1, R, h, w)
    c = {"crossattn": torch.full((ns, 77, 8), 1.0), "vector": torch.zeros(ns, 4),
         "regions": S.RegionSpec([torch.full((1, 77, 8), float(r + 1)) for r in range(R)], wt.argmax(0).to(torch.uint8), wt)}
    uc = {"crossattn": torch.full((ns, 77, 8), -1.0), "vector": torch.ones(ns, 4)}
    return c, uc, wt


@pytest.mark.parametrize("ns", [1, 2])
def test_prepare_cond_row_layout_with_cfg(ns):
    c, uc, wt = _spec(R=3, ns=ns)
    reg = S.LinearCFG(1.0, 4.0).prepare_cond(c, uc)["regions"]
    assert isinstance(reg, RegionalContext) and reg.n == reg.cap == 4 and reg.weights.dtype == torch.float32
    assert reg.bank[:, 0, 0].tolist() == [-1.0, 1.0, 2.0, 3.0]
    assert tuple(reg.weights.shape) == (2 * ns, 4, 4, 4)
    assert reg.weights[:ns, 0].eq(1).all() and reg.weights[:ns, 1:].eq(0).all()  # unconditional rows: weight 1 on entry 0
    for r in range(ns):
        assert reg.weights[ns + r, 0].eq(0).all() and torch.equal(reg.weights[ns + r, 1:], wt)
    assert torch.equal(reg.ids[ns], wt.argmax(0).to(torch.uint8) + 1) and reg.ids[:ns].eq(0).all()


def test_prepare_cond_row_layout_with_identity_guider():
    c, uc, wt = _spec(R=2, ns=2)
    reg = S.IdentityGuider().prepare_cond(c, uc)["regions"]
    assert tuple(reg.weights.shape) == (2, 3, 4, 4) and reg.weights[:, 0].eq(0).all()
    assert torch.equal(reg.weights[0, 1:], wt) and torch.equal(reg.weights[1, 1:], wt)


# ------------------------------------------------------------------------------------------------ modules (CPU stand-ins)
def soft_standin(calls):
    """CPU stand-in for ops.xattn_q_regions_soft: the projection (with the LayerNorm fold) and the per-entry composition, recorded."""
    def xattn_q_regions_soft(x, wq, bias, k_bank, vt_bank, wts, span, B, H, T, Tk, *, ln=None, colsum=None, ln_eps=1e-5, out=None, entries=None):
        calls.append(dict(wts=wts, span=span, NR=k_bank.shape[0], T=T))
        q = ops.gemm_ln(x, wq, bias, ln=ln, colsum=colsum, ln_eps=ln_eps) if ln is not None else ops.gemm(x, wq, bias)
        return ops.attn_regions_soft(q.view(B, T, H * 64), k_bank, vt_bank, wts, B, H, T, Tk)
    return xattn_q_regions_soft


def hard_standin(x, wq, bias, k_bank, vt_bank, ids, B, H, T, Tk, *, ln=None, colsum=None, ln_eps=1e-5, out=None, entries=None):
    q = ops.gemm_ln(x, wq, bias, ln=ln, colsum=colsum, ln_eps=ln_eps) if ln is not None else ops.gemm(x, wq, bias)
    return ops.attn_regions(q.view(B, T, H * 64), k_bank, vt_bank, ids, B, H, T, Tk)


@pytest.mark.parametrize("how", ["fused", "no_layernorm_fold"])
def test_spatial_transformer_hands_the_level_weights_to_the_op(how, monkeypatch):
    """A 16 x 8 token grid (128 tokens: a span) under a 32 x 16 latent map.  The fused path calls ops.xattn_q_regions_soft once per
    block with the level's own (wts, span) objects; the plain path composes ops.attn_regions_soft.  One-hot weights equal the hard
    context; a (1/4, 3/4) mix of ONE prompt equals the plain call with that prompt up to the rounding of the fp32 mix."""
    from supir_amd.modules import attention as A
    from tests import torch_ops
    from tests.helpers import fill_module, synth_tensor
    B, C, Hh, Ww, NR = 2, 128, 16, 8, 3
    calls = []
    if how == "no_layernorm_fold":
        monkeypatch.setattr(A, "FOLD_LAYERNORM", False)
    with torch_ops.installed(fp32=True):
        monkeypatch.setattr(ops, "xattn_q_regions_soft", soft_standin(calls))
        monkeypatch.setattr(ops, "xattn_q_regions", hard_standin)
        st = SpatialTransformer(C, C // 64, 64, depth=2, context_dim=32, use_linear=True)
        fill_module(st, "model.diffusion_model.input_blocks.4.1.", "cpu")
        x = synth_tensor("soft.st.x", (B, C, Hh, Ww))
        bank = synth_tensor("soft.st.bank", (NR, 77, 32))
        lat = (1 + (torch.arange(2 * Ww) >= Ww).to(torch.uint8))[None, None, :].expand(B, 2 * Hh, -1).contiguous()
        with torch.no_grad():
            hard = st(x, RegionalContext(bank, lat)).float()
            oh = torch.zeros(B, NR, 2 * Hh, 2 * Ww).scatter_(1, lat.long()[:, None], 1.0)
            reg = RegionalContext(bank, lat, weights=oh)
            one = st(x, reg).float()
            same = bank[1:2].expand(NR, -1, -1).contiguous()
            mixw = torch.zeros(B, NR, 2 * Hh, 2 * Ww)
            mixw[:, 0], mixw[:, 2] = 0.25, 0.75
            mixed = st(x, RegionalContext(same, lat, weights=mixw)).float()
            plain = st(x, same[:1].expand(B, -1, -1).contiguous()).float()
    assert torch.equal(one, hard)
    assert torch.allclose(mixed, plain, rtol=0, atol=1e-5 * float(plain.abs().max()))
    if how == "no_layernorm_fold":
        assert not calls                                     # the unfused blocks compose the existing attention (ops.attn_regions_soft)
    else:
        assert len(calls) == 4 and all(c["NR"] == NR and c["T"] == Hh * Ww for c in calls)
        wts, span = reg.level_weights(Hh, Ww)
        assert calls[0]["wts"] is wts and calls[0]["span"] is span and calls[1]["wts"] is wts
        assert span.shape == (B, 1, 2) and span[0, 0].tolist() == [1, 2]


def test_attn_regions_soft_is_the_weighted_sum_of_the_per_entry_attention(monkeypatch):
    from tests import torch_ops
    monkeypatch.setattr(ops, "flash_attn", torch_ops.flash_attn)
    g = torch.Generator().manual_seed(2)
    B, H, Tn, Tk, NR = 2, 1, 24, 5, 3
    q, kb = torch.randn(B, Tn, 64, generator=g), torch.randn(NR, Tk, 64, generator=g)
    v = torch.randn(NR, Tk, 64, generator=g)
    vtb = torch.zeros(NR, 64, 64)
    vtb[:, :, :Tk] = v.transpose(1, 2)
    w = torch.rand(B, NR, Tn, generator=g)
    w[:, 1, ::2] = 0.0
    w = w / w.sum(1, keepdim=True)
    out = ops.attn_regions_soft(q, kb, vtb, w, B, H, Tn, Tk)
    want = sum(w[:, e, :, None] * (torch.softmax(q @ kb[e].T / 8.0, -1) @ v[e]) for e in range(NR))
    assert torch.allclose(out, want, atol=1e-5)


# ------------------------------------------------------------------------------------------------ samplers
class _Net(torch.nn.Module):
    """Stand-in network: records the conditioning of every call."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def forward(self, x, t, c, control_scale=1.0, **kw):
        self.seen.append(c)
        return x * 0.5


def _cond(R, h=8, w=8, ns=1):
    lq = torch.zeros(ns, 4, h, w)
    cs = [{"crossattn": torch.full((ns, 77, 8), float(r + 1)), "vector": torch.zeros(ns, 4), "control": lq} for r in range(R)]
    uc = {"crossattn": torch.full((ns, 77, 8), -1.0), "vector": torch.zeros(ns, 4), "control": lq}
    return cs, uc


def _samplers():
    g = lambda: S.LinearCFG(1.0, 4.0)   # noqa: E731
    return [("edm", S.RestoreEDMSampler(num_steps=2, s_churn=0, restore_cfg=-1.0, device="cpu", guider_config=g())),
            ("dpmpp", S.RestoreDPMPP2MSampler(num_steps=2, eta=0.0, restore_cfg=-1.0, device="cpu", guider_config=g()))]


def _lr8():
    m = torch.zeros(8, 8, dtype=torch.int64)
    m[:, 4:] = 1
    return m


@pytest.mark.parametrize("kind", ["edm", "dpmpp"])
def test_untiled_samplers_hand_the_network_a_soft_context(kind):
    smp = dict(_samplers())[kind]
    net, den = _Net(), S.DiscreteDenoiserWithControl()
    cs, uc = _cond(2)
    w = S.feather_regions(_lr8(), 2, 1)
    x0 = torch.ones(1, 4, 8, 8)
    smp(lambda i, s, cc, c_: den(net, i, s, cc, c_), x0, cond=cs, uc=uc, x_center=torch.zeros(1, 4, 8, 8), region_weights=w * 3.0)
    assert len(net.seen) == 2
    reg = net.seen[0]["regions"]
    assert all(c["regions"] is reg for c in net.seen)                    # built once per image, not per step
    assert isinstance(reg, RegionalContext) and reg.n == 3 and tuple(reg.weights.shape) == (2, 3, 8, 8)
    assert reg.weights[0, 0].eq(1).all() and reg.weights[0, 1:].eq(0).all() and torch.equal(reg.weights[1, 1:], w)     # normalised
    assert torch.equal(reg.ids[1], (_lr8() + 1).to(torch.uint8))
    for kw in [dict(region_weights=w, regions=_lr8()),                   # both forms at once
               dict(region_weights=w[:1]),                               # R not the prompts'
               dict(region_weights=w[:, :6]),                            # another size than the latent's
               dict(region_weights=-w), dict(region_weights=w * 0)]:
        with pytest.raises(ValueError):
            smp(lambda *a: None, x0, cond=cs, uc=uc, **kw)
    with pytest.raises(ValueError):                                       # weights without a list of conditionings
        smp(lambda *a: None, x0, cond=cs[0], uc=uc, region_weights=w)


@pytest.mark.parametrize("cls", [S.TiledRestoreEDMSampler, S.TiledRestoreDPMPP2MSampler])
def test_tiled_samplers_refuse_region_weights(cls):
    smp = cls(8, 4, num_steps=2, device="cpu", guider_config=S.LinearCFG(1.0, 4.0))
    cs, uc = _cond(1)
    with pytest.raises(ValueError, match="tiled samplers take per-tile prompts"):
        smp(lambda *a: None, torch.ones(1, 4, 8, 8), cond=cs[0], uc=uc, x_center=torch.zeros(1, 4, 8, 8), region_weights=torch.ones(1, 8, 8))


# ------------------------------------------------------------------------------------------------ batchify_sample
def _model(monkeypatch, sampler="RestoreEDMSampler"):
    """SUPIRModel.batchify_sample around stand-ins: identity 'VAE' on a 4-channel 'image', the recording network."""
    from supir_amd.models.supir_model import SUPIRModel
    m = SUPIRModel.__new__(SUPIRModel)
    torch.nn.Module.__init__(m)
    ddpm = {"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"}
    extra = {"tile_size": 8, "tile_stride": 4} if sampler.startswith("Tiled") else {}
    m.sampler_config = {"target": f"sgm.modules.diffusionmodules.sampling.{sampler}",
                        "params": dict(num_steps=2, restore_cfg=-1.0, s_churn=0, s_noise=1.0, device="cpu", discretization_config=ddpm,
                                       guider_config={"target": "sgm.modules.diffusionmodules.guiders.LinearCFG",
                                                      "params": {"scale": 7.5, "scale_min": 4.0}}, **extra)}
    m.p_p, m.n_p = "", ""
    m.denoiser = S.DiscreteDenoiserWithControl()
    m.model = _Net()
    m.conditioner = None
    monkeypatch.setattr(m, "encode_first_stage_with_denoise", lambda x, use_sample=True, is_stage1=False, noise=None: x.clone())
    monkeypatch.setattr(m, "decode_first_stage", lambda z: z.clone())
    monkeypatch.setattr(m, "encode_first_stage", lambda x, noise=None: x.clone())
    return m


def _strip(d):
    return {k: v for k, v in d.items() if k != "control"}


def _run(m, cs, uc, **kw):
    return m.batchify_sample(torch.ones(1, 4, 8, 8), cond=([_strip(c) for c in cs], _strip(uc)), num_steps=2, restoration_scale=-1, seed=3, **kw)


def test_batchify_sample_with_both_keywords_none_is_the_parents_call(monkeypatch):
    """region_weights=None, region_feather=None: the regional branch is never entered, the sampler gets no new keyword, and the
    conditioning dicts the network sees hold the keys they held before (no "regions")."""
    m = _model(monkeypatch)

    def boom(*a, **k):
        raise AssertionError("the regional branch was entered")

    for name in ("_regional_cond", "_regional_context", "region_weights", "feather_regions", "region_map"):
        monkeypatch.setattr(S, name, boom)
    monkeypatch.setattr(m, "_regional_condition", boom)
    seen_kw = []
    real_call = S.RestoreEDMSampler.__call__
    monkeypatch.setattr(S.RestoreEDMSampler, "__call__", lambda self, *a, **k: (seen_kw.append(sorted(k)), real_call(self, *a, **k))[1])
    cs, uc = _cond(1)
    out = m.batchify_sample(torch.ones(1, 4, 8, 8), cond=(_strip(cs[0]), _strip(uc)), num_steps=2, restoration_scale=-1, seed=3,
                            region_weights=None, region_feather=None)
    assert out.shape == (1, 4, 8, 8) and len(m.model.seen) == 2
    assert seen_kw == [["cond", "control_scale", "control_scale_start", "uc", "use_linear_control_scale", "x_center"]]
    assert all(sorted(cc) == ["control", "crossattn", "vector"] for cc in m.model.seen)
    assert m.model.seen[0]["crossattn"].shape == (2, 77, 8)


@pytest.mark.parametrize("sampler", ["RestoreEDMSampler", "RestoreDPMPP2MSampler"])
def test_batchify_sample_routes_weights_and_feather(monkeypatch, sampler):
    cs, uc = _cond(2)
    w = S.feather_regions(_lr8(), 2, 2)
    seen = {}
    for name, kw in [("weights", dict(region_weights=w)), ("feather", dict(regions=_lr8(), region_feather=2)),
                     ("boxes", dict(regions=[(0, 8, 0, 8), (0, 8, 4, 8)], region_feather=2)),
                     ("feather0", dict(regions=_lr8(), region_feather=0)), ("hard", dict(regions=_lr8()))]:
        m = _model(monkeypatch, sampler)
        assert _run(m, cs, uc, num_samples=2, **kw).shape == (2, 4, 8, 8)
        seen[name] = m.model.seen[0]["regions"]
    for name in ("weights", "feather", "boxes"):
        reg = seen[name]
        assert tuple(reg.weights.shape) == (4, 3, 8, 8) and reg.weights[:2, 0].eq(1).all() and reg.weights[:2, 1:].eq(0).all()
        assert torch.equal(reg.weights[2, 1:], w) and torch.equal(reg.weights[3, 1:], w)      # num_samples repeats the weights
        assert reg.bank[:, 0, 0].tolist() == [-1.0, 1.0, 2.0]
    assert seen["hard"].weights is None                                                       # `regions` alone is untouched
    assert torch.equal(seen["feather0"].weights[2, 1:], one_hot(_lr8(), 2)) and torch.equal(seen["feather0"].ids, seen["hard"].ids)
    m = _model(monkeypatch, sampler)
    for kw in [dict(region_weights=w, regions=_lr8()),                   # both
               dict(region_feather=2),                                   # a radius without a map
               dict(regions=_lr8(), region_feather=-1),                  # a negative radius
               dict(regions=w),                                          # a float tensor as `regions` keeps raising
               dict(region_weights=w[:1]), dict(region_weights=torch.ones(2, 4, 4)), dict(region_weights=w * float("nan"))]:
        with pytest.raises(ValueError):
            _run(m, cs, uc, **kw)
    with pytest.raises(ValueError):                                       # one conditioning, not a list of them
        m.batchify_sample(torch.ones(1, 4, 8, 8), cond=(_strip(cs[0]), _strip(uc)), num_steps=2, restoration_scale=-1, seed=3,
                          region_weights=w)
    with pytest.raises(ValueError, match="254"):
        m.batchify_sample(torch.ones(1, 4, 8, 8), p=[["x"] * 255], num_steps=2, restoration_scale=-1, seed=3,
                          region_weights=torch.ones(255, 8, 8))


def test_batchify_sample_refuses_region_weights_on_a_tiled_sampler(monkeypatch):
    m = _model(monkeypatch, "TiledRestoreEDMSampler")
    cs, uc = _cond(2)
    with pytest.raises(ValueError, match="tiled"):
        _run(m, cs, uc, region_weights=torch.ones(2, 8, 8))
    with pytest.raises(ValueError, match="tiled"):
        _run(m, cs, uc, regions=_lr8(), region_feather=1)
