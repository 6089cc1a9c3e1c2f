"""TiledRestoreDPMPP2MSampler with tile batching (`tile_batch`: k tiles stacked into one denoiser call) on the host path, against the
goldens the unbatched sampler is pinned to (reference classes, oracle/gen_golden*.py): stacking tiles changes no per-tile arithmetic,
so every group split -- full groups, a remainder group (3 + 3 + 2), one group of all 8 tiles -- must land on the same image."""
import os

import pytest
import torch

from supir_amd.modules import sampling as S
from tests.helpers import GOLDEN_DIR, golden, rel_l2, synth_tensor
from tests.test_host_logic import _ScriptedNoise, _fake_net, _io, _prompt_net

BIG = (1, 4, 24, 40)      # 16 / 8 tiles: 2 x 4 = 8 tiles


@pytest.fixture(scope="module")
def g():
    return golden()


@pytest.fixture(scope="module")
def ge():
    return torch.load(os.path.join(GOLDEN_DIR, "golden_extra.pt"), map_location="cpu", weights_only=False)


def _cond():
    c, uc = _io()
    lqb = synth_tensor("lq_big", BIG)
    return dict(c, control=lqb), dict(uc, control=lqb)


def _sampler(tile_batch, **kw):
    return S.TiledRestoreDPMPP2MSampler(tile_size=16, tile_stride=8, num_steps=4, s_noise=1.003, eta=1.0, device="cpu",
                                        guider_config=S.LinearCFG(1.0, 4.0), tile_batch=tile_batch, **kw)


def test_tile_geometry_of_the_fixture():
    tiles = S._sliding_windows(BIG[2], BIG[3], 16, 8)
    assert len(tiles) == 8
    groups, mine = S._TileGroups._tile_groups(tiles, 3, 1, 0)
    assert [len(gr) for gr in groups] == [3, 3, 2] and mine == [0, 1, 2]
    assert S._TileGroups._tile_groups(tiles, 3, 2, 1)[1] == [1]           # round robin over two ranks


@pytest.mark.parametrize("tile_batch", [2, 3, 8])
def test_tile_batch_with_scripted_noise_matches_the_reference(g, tile_batch):
    c, uc = _cond()
    den = S.DiscreteDenoiserWithControl()
    smp = _sampler(tile_batch, noise_sampler_cls=_ScriptedNoise)
    calls = []

    def net(xin, tt, cc, cs):
        calls.append(xin.shape[0])
        return _fake_net(xin, tt, cc, cs)

    out = smp(lambda i, s, cc, cs: den(net, i, s, cc, cs), synth_tensor("noised_big", BIG), cond=c, uc=uc, control_scale=1.0)
    assert rel_l2(out, g["sampler_dpmpp_tiled_4"]) <= 5e-5
    per_step = [2 * len(gr) for gr in S._TileGroups._tile_groups(S._sliding_windows(24, 40, 16, 8), tile_batch, 1, 0)[0]]
    assert calls == per_step * 4          # k tiles (x 2 for CFG) per network call, every step


@pytest.mark.parametrize("tile_batch", [2, 3, 8])
def test_tile_batch_with_the_default_brownian_noise_matches_the_reference(ge, tile_batch):
    c, uc = _cond()
    den = S.DiscreteDenoiserWithControl()
    smp = _sampler(tile_batch)
    torch.manual_seed(4321)
    out = smp(lambda i, s, cc, cs: den(_fake_net, i, s, cc, cs), synth_tensor("noised_big", BIG), cond=c, uc=uc, control_scale=1.0)
    assert rel_l2(out, ge["sampler_dpmpp_brownian_tiled_4"]) <= 5e-5


def test_local_prompts_force_one_tile_per_call(ge):
    """Per-tile prompts cannot share a call: tile_batch 4 still runs one tile per call and matches the local-prompt golden."""
    _, uc = _io()
    lqb = synth_tensor("lq_big", BIG)
    n_tiles = len(S._sliding_windows(24, 40, 16, 8))
    local = [{"crossattn": synth_tensor(f"local.ctx{j}", (1, 77, 2048)), "vector": synth_tensor(f"local.vec{j}", (1, 2816)), "control": lqb}
             for j in range(n_tiles)]
    uc = dict(uc, control=lqb)
    den = S.DiscreteDenoiserWithControl()
    calls = []

    def net(xin, tt, cc, cs):
        calls.append(xin.shape[0])
        return _prompt_net(xin, tt, cc, cs)

    torch.manual_seed(777)
    out = _sampler(4)(lambda i, s, cc, cs: den(net, i, s, cc, cs), synth_tensor("noised_big", BIG), cond=[dict(cj) for cj in local],
                      uc=dict(uc), control_scale=1.0)
    assert rel_l2(out, ge["sampler_dpmpp_tiled_local_prompts"]) <= 5e-5
    assert set(calls) == {2}


def test_new_kwargs_are_stored():
    smp = _sampler(5, tile_parallel=True, process_group=None)
    assert smp.tile_batch == 5 and smp.tile_parallel is True and smp.process_group is None
    assert _sampler(0).tile_batch == 1
