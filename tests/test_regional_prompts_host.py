"""Regional prompts on the untiled samplers, host side (no GPU): the region maps (regions_from_tiles, box lists, checks), the id tables
of the transformer levels, the guiders' row layout, the refusals, and batchify_sample's routing with stand-in networks."""
import pytest
import torch

from supir_amd.modules import sampling as S
from supir_amd.modules.attention import RegionalContext, level_region_ids


# ------------------------------------------------------------------------------------------------ maps
SIZES = [(h, w) for h in range(128, 321, 32) for w in range(128, 321, 32)]


@pytest.mark.parametrize("h,w,tile,stride", [(h, w, 128, 64) for h, w in SIZES] + [(96, 200, 64, 48)])
def test_regions_from_tiles_is_a_partition_with_a_region_per_tile(h, w, tile, stride):
    tiles = S._sliding_windows(h, w, tile, stride)
    m = S.regions_from_tiles(h, w, tile, stride)
    assert tuple(m.shape) == (h, w) and not m.is_floating_point()
    assert int(m.min()) >= 0 and int(m.max()) < len(tiles)              # every pixel exactly one id (a map has no other way) ...
    assert sorted(m.unique().tolist()) == list(range(len(tiles)))       # ... and every tile a non-empty region
    for j, (a, b, c, d) in enumerate(tiles):
        assert bool((m[a:b, c:d] == j).any())                           # inside its own window
        assert int(m[(a + b - 1) // 2, (c + d - 1) // 2]) == j          # around its own centre


def test_regions_from_tiles_takes_the_nearest_centre_and_the_lower_index_on_ties():
    # 128 x 192, tile 128, stride 64: two tiles with centres at x = 63.5 and 127.5; x = 95 and 96 are 31.5 / 32.5 and 32.5 / 31.5 away
    m = S.regions_from_tiles(128, 192, 128, 64)
    assert m[:, :96].eq(0).all() and m[:, 96:].eq(1).all()
    # tile 2 x 2, stride 1 on a 2 x 3 grid: centres at x = 0.5 and 1.5; the column x = 1 is 0.5 from both -> the lower index
    m = S.regions_from_tiles(2, 3, 2, 1)
    assert m.tolist() == [[0, 0, 1], [0, 0, 1]]


def test_box_lists_paint_in_order_and_must_cover_the_grid():
    m = S.region_map([(0, 8, 0, 8), (2, 6, 4, 8), (4, 8, 0, 6)], 3, 8, 8)
    want = torch.zeros(8, 8, dtype=torch.uint8)
    want[2:6, 4:8] = 1
    want[4:8, 0:6] = 2                       # the later box wins where it overlaps box 1
    assert m.dtype == torch.uint8 and torch.equal(m, want)
    with pytest.raises(ValueError, match="covered by no region"):
        S.region_map([(0, 8, 0, 4), (0, 7, 4, 8)], 2, 8, 8)
    with pytest.raises(ValueError):
        S.region_map([(0, 9, 0, 8)], 1, 8, 8)                          # outside the grid
    with pytest.raises(ValueError):
        S.region_map([(0, 8, 0, 8)], 2, 8, 8)                          # one box, two prompts


def test_region_map_checks():
    ok = torch.tensor([[0, 1], [2, 1]])
    assert S.region_map(ok, 3, 2, 2).tolist() == ok.tolist()
    assert S.region_map(ok.numpy(), 3, 2, 2).tolist() == ok.tolist()
    with pytest.raises(ValueError, match="there are 2 prompts"):
        S.region_map(ok, 2, 2, 2)                                       # mismatched R
    with pytest.raises(ValueError, match="latent grid"):
        S.region_map(ok, 3, 2, 4)                                       # a map of the wrong size
    with pytest.raises(ValueError):
        S.region_map(ok.float(), 3, 2, 2)
    with pytest.raises(ValueError):
        S.region_map(-ok, 3, 2, 2)
    with pytest.raises(ValueError, match="254"):
        S.region_map(torch.zeros(2, 2, dtype=torch.int64), 255, 2, 2)  # more than 254 regions
    assert S.region_map(torch.zeros(2, 2, dtype=torch.int64), 254, 2, 2).shape == (2, 2)


# ------------------------------------------------------------------------------------------------ level ids
MAP8 = torch.tensor([[0, 0, 0, 1, 1, 1, 1, 1],
                     [0, 0, 0, 1, 1, 1, 1, 1],
                     [0, 0, 2, 2, 2, 1, 1, 1],
                     [3, 3, 2, 2, 2, 2, 4, 4],
                     [3, 3, 2, 2, 2, 2, 4, 4],
                     [3, 3, 3, 5, 5, 5, 4, 4],
                     [6, 6, 6, 5, 5, 5, 7, 7],
                     [6, 6, 6, 6, 5, 7, 7, 8]], dtype=torch.uint8)


@pytest.mark.parametrize("ds", [1, 2, 4])
def test_level_ids_follow_the_centre_pixel_rule(ds):
    ids = torch.stack([MAP8, MAP8.flip(0)])
    n = 8 // ds
    got = level_region_ids(ids, n, n)
    assert got.dtype == torch.uint8 and got.shape == (2, n * n) and got.is_contiguous()
    for b in range(2):
        for y in range(n):
            for x in range(n):
                assert int(got[b, y * n + x]) == int(ids[b, y * ds + ds // 2, x * ds + ds // 2])
    with pytest.raises(ValueError):
        level_region_ids(ids, 3, 3)
    with pytest.raises(ValueError):
        level_region_ids(ids, 4, 2)


def test_regional_context_keeps_its_level_tables_and_refreshes_them_in_place():
    bank = torch.zeros(4, 77, 8)
    rc = RegionalContext(bank, torch.stack([MAP8 % 3]), n=3)
    a = rc.level_ids(4, 4)
    assert rc.level_ids(4, 4) is a and rc.cap == 4 and rc.n == 3
    other = RegionalContext(torch.ones(2, 77, 8), torch.stack([(MAP8 + 1) % 2]))
    ptr, bank_ptr = a.data_ptr(), rc.bank.data_ptr()
    rc.load(other)
    assert rc.level_ids(4, 4).data_ptr() == ptr and rc.bank.data_ptr() == bank_ptr and rc.n == 2
    assert torch.equal(rc.level_ids(4, 4), level_region_ids(other.ids, 4, 4)) and torch.equal(rc.ids, other.ids)
    assert rc.bank[:2].eq(1).all() and rc.bank[2:].eq(0).all()
    v = rc.bank._version
    rc.load(other)                                   # unchanged source: nothing is written
    assert rc.bank._version == v
    with pytest.raises(ValueError):
        rc.load(RegionalContext(torch.ones(5, 77, 8), torch.stack([MAP8 % 5])))      # more entries than the bank holds
    with pytest.raises(ValueError):
        RegionalContext(torch.zeros(256, 1, 8), torch.zeros(1, 2, 2, dtype=torch.uint8))
    with pytest.raises(ValueError):
        RegionalContext(bank, torch.zeros(1, 2, 2, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ guiders
def _spec(R=2, ns=1, h=4, w=4):
    m = S.region_map((torch.arange(h * w).reshape(h, w) % R), R, h, w)
    c = {"crossattn": torch.full((ns, 77, 8), 1.0), "vector": torch.zeros(ns, 4),
         "regions": S.RegionSpec([torch.full((1, 77, 8), float(r + 1)) for r in range(R)], m)}
    uc = {"crossattn": torch.full((ns, 77, 8), -1.0), "vector": torch.ones(ns, 4)}
    return c, uc, m


@pytest.mark.parametrize("ns", [1, 2])
def test_prepare_cond_row_layout_with_cfg(ns):
    c, uc, m = _spec(R=3, ns=ns)
    out = S.LinearCFG(1.0, 4.0).prepare_cond(c, uc)
    reg = out["regions"]
    assert isinstance(reg, RegionalContext) and reg.n == reg.cap == 4 and reg.ids.dtype == torch.uint8
    assert reg.bank[:, 0, 0].tolist() == [-1.0, 1.0, 2.0, 3.0]           # entry 0 = uc, entries 1 .. R = the regions' prompts
    assert tuple(reg.ids.shape) == (2 * ns, 4, 4)
    assert reg.ids[:ns].eq(0).all()                                      # unconditional rows: entry 0 everywhere
    for r in range(ns):
        assert torch.equal(reg.ids[ns + r], m + 1)                       # every conditional row the same map, 1 + region
    assert out["crossattn"].shape == (2 * ns, 77, 8) and out["vector"].shape == (2 * ns, 4)


def test_prepare_cond_row_layout_with_identity_guider():
    c, uc, m = _spec(R=2, ns=2)
    g = S.IdentityGuider()
    out = g.prepare_cond(c, uc)
    reg = out["regions"]
    assert tuple(reg.ids.shape) == (2, 4, 4) and torch.equal(reg.ids[0], m + 1) and torch.equal(reg.ids[1], m + 1)
    assert reg.bank[:, 0, 0].tolist() == [-1.0, 1.0, 2.0]
    assert g.prepare_inputs(torch.zeros(2, 4, 4, 4), torch.ones(2), c, uc)[2]["regions"].ids.shape == (2, 4, 4)
    plain = {"crossattn": torch.zeros(1, 77, 8)}
    assert g.prepare_cond(plain, None) == plain


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


@pytest.mark.parametrize("kind", ["edm", "dpmpp"])
def test_untiled_samplers_hand_the_network_a_regional_context(kind):
    smp = dict(_samplers())[kind]
    net, den = _Net(), S.DiscreteDenoiserWithControl()
    cs, uc = _cond(2)
    m = torch.zeros(8, 8, dtype=torch.int64)
    m[:, 4:] = 1
    smp(lambda i, s, cc, c_: den(net, i, s, cc, c_), torch.ones(1, 4, 8, 8), cond=cs, uc=uc, x_center=torch.zeros(1, 4, 8, 8),
        regions=m)
    assert len(net.seen) == 2
    reg = net.seen[0]["regions"]
    assert all(c["regions"] is reg for c in net.seen)                    # built once per image, not per step
    assert isinstance(reg, RegionalContext) and reg.n == 3
    assert reg.ids[0].eq(0).all() and torch.equal(reg.ids[1], (m + 1).to(torch.uint8))
    assert net.seen[0]["crossattn"].shape == (2, 77, 8)                  # region 0's conditioning is the global one
    with pytest.raises(ValueError):                                       # a list without a map: that is the tiled samplers' form
        smp(lambda *a: None, torch.ones(1, 4, 8, 8), cond=cs, uc=uc)
    with pytest.raises(ValueError):                                       # a map without a list
        smp(lambda *a: None, torch.ones(1, 4, 8, 8), cond=cs[0], uc=uc, regions=m)
    with pytest.raises(ValueError):                                       # mismatched R
        smp(lambda *a: None, torch.ones(1, 4, 8, 8), cond=cs, uc=uc, regions=m + 1)
    with pytest.raises(ValueError):                                       # a map of the wrong size
        smp(lambda *a: None, torch.ones(1, 4, 8, 8), cond=cs, uc=uc, regions=m[:, :6])
    with pytest.raises(ValueError):                                       # one token count per bank
        bad = [cs[0], dict(cs[1], crossattn=torch.zeros(1, 154, 8))]
        smp(lambda *a: None, torch.ones(1, 4, 8, 8), cond=bad, uc=uc, regions=m)


@pytest.mark.parametrize("cls", [S.TiledRestoreEDMSampler, S.TiledRestoreDPMPP2MSampler])
def test_tiled_samplers_refuse_regions(cls):
    smp = cls(8, 4, num_steps=2, device="cpu", guider_config=S.LinearCFG(1.0, 4.0))
    cs, uc = _cond(1)
    with pytest.raises(ValueError, match="tiled"):
        smp(lambda *a: None, torch.ones(1, 4, 8, 8), cond=cs[0], uc=uc, x_center=torch.zeros(1, 4, 8, 8),
            regions=torch.zeros(8, 8, dtype=torch.int64))


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


def test_batchify_sample_without_regions_never_enters_the_regional_branch(monkeypatch):
    m = _model(monkeypatch)

    def boom(*a, **k):
        raise AssertionError("the regional branch was entered")

    monkeypatch.setattr(m, "_regional_condition", boom)
    monkeypatch.setattr(S, "_regional_cond", boom)
    monkeypatch.setattr(S, "_regional_context", boom)
    cs, uc = _cond(1)
    c = {k: v for k, v in cs[0].items() if k != "control"}
    u = {k: v for k, v in uc.items() if k != "control"}
    out = m.batchify_sample(torch.ones(1, 4, 8, 8), cond=(c, u), num_steps=2, restoration_scale=-1, seed=3)
    assert out.shape == (1, 4, 8, 8) and len(m.model.seen) == 2
    assert all("regions" not in cc for cc in m.model.seen)
    assert m.model.seen[0]["crossattn"].shape == (2, 77, 8)


@pytest.mark.parametrize("sampler", ["RestoreEDMSampler", "RestoreDPMPP2MSampler"])
def test_batchify_sample_with_regions_and_num_samples(monkeypatch, sampler):
    m = _model(monkeypatch, sampler)
    cs, uc = _cond(3)
    strip = lambda d: {k: v for k, v in d.items() if k != "control"}   # noqa: E731
    boxes = [(0, 8, 0, 8), (0, 8, 4, 8), (6, 8, 0, 8)]
    out = m.batchify_sample(torch.ones(1, 4, 8, 8), cond=([strip(c) for c in cs], strip(uc)), num_steps=2, restoration_scale=-1, seed=3,
                            num_samples=2, regions=boxes)
    assert out.shape == (2, 4, 8, 8)
    reg = m.model.seen[0]["regions"]
    want = S.region_map(boxes, 3, 8, 8) + 1
    assert tuple(reg.ids.shape) == (4, 8, 8) and reg.ids[:2].eq(0).all()
    assert torch.equal(reg.ids[2], want) and torch.equal(reg.ids[3], want)        # rows 0 and 1 of the conditional half: the same map
    assert reg.bank[:, 0, 0].tolist() == [-1.0, 1.0, 2.0, 3.0]
    assert m.model.seen[0]["vector"].shape == (4, 4) and m.model.seen[0]["control"].shape == (4, 4, 8, 8)
    for bad, kw in [(ValueError, dict(regions=boxes[:2])),                                       # mismatched R
                    (ValueError, dict(regions=torch.zeros(4, 4, dtype=torch.int64))),           # a map of the wrong size
                    (ValueError, dict(regions=[(0, 4, 0, 8), (0, 4, 0, 8), (4, 8, 0, 7)]))]:     # uncovered pixels
        with pytest.raises(bad):
            m.batchify_sample(torch.ones(1, 4, 8, 8), cond=([strip(c) for c in cs], strip(uc)), num_steps=2, restoration_scale=-1,
                              seed=3, **kw)
    with pytest.raises(ValueError):                                                              # one conditioning, not a list of them
        m.batchify_sample(torch.ones(1, 4, 8, 8), cond=(strip(cs[0]), strip(uc)), num_steps=2, restoration_scale=-1, seed=3,
                          regions=boxes)
    with pytest.raises(ValueError, match="254"):                                                 # more than 254 regions
        m.batchify_sample(torch.ones(1, 4, 8, 8), p=[["x"] * 255], num_steps=2, restoration_scale=-1, seed=3,
                          regions=torch.zeros(8, 8, dtype=torch.int64))


def test_batchify_sample_refuses_regions_on_a_tiled_sampler(monkeypatch):
    m = _model(monkeypatch, "TiledRestoreEDMSampler")
    cs, uc = _cond(2)
    strip = lambda d: {k: v for k, v in d.items() if k != "control"}   # noqa: E731
    with pytest.raises(ValueError, match="tiled"):
        m.batchify_sample(torch.ones(1, 4, 8, 8), cond=([strip(c) for c in cs], strip(uc)), num_steps=2, restoration_scale=-1, seed=3,
                          regions=torch.zeros(8, 8, dtype=torch.int64))
