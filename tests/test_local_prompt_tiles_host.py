"""Per-tile ("local") prompts on the batched tiled samplers, host side (no GPU): `cond` as a list (SUPIR_model.py:168-178 ->
sampling.py:609-616, 636-643, 671-680, 705-708) with `tile_batch_local_prompts=True` stacks k tiles -- each with ITS prompt -- into one
network call and lands on the goldens recorded from the reference classes; the per-group embedding schedule addresses row g * S + i;
supir_gather_segments is declared, exported and validates its arguments before any HIP call."""
import math
import os

import pytest
import torch

from supir_amd import _lib, ops
from supir_amd.modules import sampling as S
from supir_amd.modules.wrappers import ControlWrapper
from tests.helpers import GOLDEN_DIR, rel_l2, synth_tensor
from tests.test_abi import _header_functions
from tests.test_host_logic import _Noise, _io, _prompt_net

BIG = (1, 4, 24, 40)      # tiles of 16 with stride 8: 2 x 4 = 8 tiles
N_TILES = 8
FAKE = 0x10000            # never dereferenced: validation comes first
ERR_ARG = -1


@pytest.fixture(scope="module")
def ge():
    return torch.load(os.path.join(GOLDEN_DIR, "golden_extra.pt"), map_location="cpu", weights_only=False)


def _local():
    """The inputs of tests/test_host_logic.py::test_tiled_samplers_with_local_prompts_vs_reference."""
    _, uc = _io()
    lqb = synth_tensor("lq_big", BIG)
    assert len(S._sliding_windows(BIG[2], BIG[3], 16, 8)) == N_TILES
    local = [{"crossattn": synth_tensor(f"local.ctx{j}", (1, 77, 2048)), "vector": synth_tensor(f"local.vec{j}", (1, 2816)), "control": lqb}
             for j in range(N_TILES)]
    return local, dict(uc, control=lqb)


def _recording_net(calls):
    def net(xin, tt, cc, cs):
        calls.append((xin.shape[0], cc["crossattn"].clone(), cc["vector"].clone()))
        return _prompt_net(xin, tt, cc, cs)
    return net


def _edm(tile_batch, **kw):
    return S.TiledRestoreEDMSampler(tile_size=16, tile_stride=8, num_steps=3, s_churn=5, s_noise=1.01, restore_cfg=4.0, device="cpu",
                                    guider_config=S.LinearCFG(1.0, 4.0), tile_batch=tile_batch, **kw)


def _dpmpp(tile_batch, **kw):
    return S.TiledRestoreDPMPP2MSampler(tile_size=16, tile_stride=8, num_steps=4, s_noise=1.003, eta=1.0, device="cpu",
                                        guider_config=S.LinearCFG(1.0, 4.0), tile_batch=tile_batch, **kw)


def _run_edm(smp, net):
    local, uc = _local()
    den = S.DiscreteDenoiserWithControl()
    with _Noise([synth_tensor(f"local.eps{i}", BIG) for i in range(3)]):
        return smp(lambda i, s, cc, cs: den(net, i, s, cc, cs), synth_tensor("noised_big", BIG), cond=[dict(cj) for cj in local],
                   uc=dict(uc), x_center=synth_tensor("xc_big", BIG), control_scale=0.9)


def _run_dpmpp(smp, net):
    local, uc = _local()
    den = S.DiscreteDenoiserWithControl()
    torch.manual_seed(777)
    return smp(lambda i, s, cc, cs: den(net, i, s, cc, cs), synth_tensor("noised_big", BIG), cond=[dict(cj) for cj in local], uc=dict(uc),
               control_scale=1.0)


def _check_calls(calls, tile_batch, steps):
    """ceil(n_tiles / tile_batch) calls per step with batches 2 k; a call's crossattn / vector rows are [uc] * k, then its tiles' in order."""
    local, uc = _local()
    sizes = [min(tile_batch, N_TILES - j0) for j0 in range(0, N_TILES, tile_batch)]
    assert len(sizes) == math.ceil(N_TILES / tile_batch)
    assert [c[0] for c in calls] == [2 * k for k in sizes] * steps
    for n, (_, ctx, vec) in enumerate(calls):
        gi = n % len(sizes)
        j0, k = gi * tile_batch, sizes[gi]
        assert tuple(ctx.shape) == (2 * k, 77, 2048) and tuple(vec.shape) == (2 * k, 2816)
        for r in range(k):
            assert torch.equal(ctx[r], uc["crossattn"][0]) and torch.equal(vec[r], uc["vector"][0])
            assert torch.equal(ctx[k + r], local[j0 + r]["crossattn"][0]) and torch.equal(vec[k + r], local[j0 + r]["vector"][0])


@pytest.mark.parametrize("tile_batch", [4, 2, 3, 8, 16])
def test_edm_batches_tiles_with_their_own_prompts(ge, tile_batch):
    calls = []
    out = _run_edm(_edm(tile_batch, tile_batch_local_prompts=True), _recording_net(calls))
    assert rel_l2(out, ge["sampler_tiled_local_prompts"]) <= 5e-5
    _check_calls(calls, tile_batch, 3)


@pytest.mark.parametrize("tile_batch", [4, 2, 3, 8, 16])
def test_dpmpp_batches_tiles_with_their_own_prompts(ge, tile_batch):
    calls = []
    out = _run_dpmpp(_dpmpp(tile_batch, tile_batch_local_prompts=True), _recording_net(calls))
    assert rel_l2(out, ge["sampler_dpmpp_tiled_local_prompts"]) <= 5e-5
    _check_calls(calls, tile_batch, 4)


def test_default_keeps_one_tile_per_call(ge):
    """Without the kwarg a list `cond` runs one tile per call whatever tile_batch says (tests/test_dpmpp_tiled_host.py pins it)."""
    for make, run, name, steps in ((_edm, _run_edm, "sampler_tiled_local_prompts", 3), (_dpmpp, _run_dpmpp, "sampler_dpmpp_tiled_local_prompts", 4)):
        smp = make(4)
        assert smp.tile_batch_local_prompts is False and make(4, tile_batch_local_prompts=1).tile_batch_local_prompts is True
        calls = []
        out = run(smp, _recording_net(calls))
        assert rel_l2(out, ge[name]) <= 5e-5
        assert [c[0] for c in calls] == [2] * (N_TILES * steps)


def test_group_conditioning_tensors_are_built_once_per_image():
    """The network's caches and captured graphs key on tensor identity: every step must pass the group's very same tensors."""
    seen = []

    def net(xin, tt, cc, cs):
        seen.append((id(cc["crossattn"]), id(cc["vector"])))
        return _prompt_net(xin, tt, cc, cs)

    _run_edm(_edm(3, tile_batch_local_prompts=True), net)
    assert len(seen) == 9 and seen[:3] == seen[3:6] == seen[6:] and len(set(seen[:3])) == 3


# ------------------------------------------------------------------------------------------------ per-group embedding schedule
class _TableNet(torch.nn.Module):
    """Stands in for a UNet: records what ControlWrapper.prepare_schedule hands down."""

    def __init__(self):
        super().__init__()
        self.got = []

    def prepare_schedule(self, t_values, y, row, control=None):
        self.got.append((list(t_values), y, row))
        return 1

    def end_schedule(self):
        pass


def test_select_step_addresses_row_g_times_s_plus_i():
    w = ControlWrapper(_TableNet(), dtype=torch.bfloat16)
    w.load_control_model(_TableNet())
    S_, G = 50, 13                                   # 13 groups x 50 steps = 650 rows: more than the 64-row table floor
    vecs4 = [torch.full((8, 16), float(g)) for g in range(G)]
    w.prepare_schedule(list(range(S_)), vecs4)
    w.prepare_schedule(list(range(S_)), [torch.zeros(2, 16)])             # the remainder group's batch size: one group
    t_values, y, row = w.diffusion_model.got[0]
    assert len(t_values) == S_ and isinstance(y, list) and len(y) == G and all(a is b for a, b in zip(y, vecs4))
    assert row is w._emb_row and w.control_model.got[0][1] is y
    assert w._sched_groups == {8: G, 2: 1} and w._scheds[8][1:3] == w._scheds[2][1:3]     # the graph key's part: no group in it
    for i, g in ((0, 0), (49, 0), (0, 1), (7, 5), (49, 12)):
        w.select_step(i, group=g, batch=8)
        assert int(w._emb_row) == g * S_ + i
        w._sched_armed = False
    w.select_step(3, expect_t=3)                     # callers that pass no group: row i of the schedule prepared last
    assert int(w._emb_row) == 3
    for bad in (13, -1, 100):
        with pytest.raises(IndexError):
            w.select_step(0, group=bad, batch=8)
    with pytest.raises(IndexError):
        w.select_step(0, group=1, batch=2)           # the batch-2 schedule has one group
    with pytest.raises(IndexError):
        w.select_step(0, group=0, batch=6)           # no schedule for that batch
    with pytest.raises(IndexError):
        w.select_step(50, group=0, batch=8)
    w.select_step(2, group=12, batch=8)              # announced for the batch-8 table, then called with batch 2: refused at the call
    with pytest.raises(IndexError):
        w._use_schedule({}, 2)
    with pytest.raises(ValueError):
        w.prepare_schedule([1, 2], [torch.zeros(2, 16)], control=torch.zeros(2, 4, 8, 8))
    w.end_schedule()
    assert w._sched is None and not w._scheds


def test_1200_rows_fit():
    """49 groups x 50 steps (tile batch 1 on the 4096^2 canvas) is past the 1024 row indices the wrapper used to keep."""
    w = ControlWrapper(_TableNet(), dtype=torch.bfloat16)
    w.load_control_model(_TableNet())
    w.prepare_schedule(list(range(50)), [torch.zeros(2, 16) for _ in range(49)])
    w.select_step(49, group=48)
    assert int(w._emb_row) == 48 * 50 + 49


def test_sampler_prepares_one_table_per_group_size_and_announces_groups(monkeypatch):
    """The fused loop with per-tile prompts: 8 tiles in groups of 3 + 3 + 2 -> two prepare_schedule calls (batch 6 with two vectors, batch 4
    with one), every call announced with its group's block."""
    monkeypatch.setattr(S, "EMB_SCHEDULE", True)
    monkeypatch.setattr(ops, "tile_blend", lambda *a, **k: None)
    prepared, selected, banks = [], [], []

    class Net:
        def prepare_schedule(self, t_values, vector, control=None, control_scales=None):
            prepared.append([tuple(v.shape) for v in vector])

        def select_step(self, i, expect_t=None, group=None, batch=None):
            selected.append((i, group, batch))

        def prepare_context_bank(self, contexts, groups, reps):
            banks.append((len(contexts), [(tuple(c.shape), idx) for c, _, idx in groups], reps))

        def end_schedule(self):
            pass

    den = S.DiscreteDenoiserWithControl()
    smp = _edm(3, tile_batch_local_prompts=True)
    smp._fused_ctx = lambda d, x: (den, Net())

    def fused_step(ctx, *a, sched_row=None, tiles=None, sched_group=None, **k):
        ctx[1].select_step(sched_row, None, group=sched_group, batch=2 * len(tiles[0]))
        return torch.zeros(len(tiles[0]), 4, 16, 16)

    smp._fused_step = fused_step
    local, uc = _local()
    smp(None, synth_tensor("noised_big", BIG), cond=[dict(cj) for cj in local], uc=dict(uc), x_center=synth_tensor("xc_big", BIG))
    assert prepared == [[(6, 2816)] * 2, [(4, 2816)]]
    assert selected == [(i, g, b) for i in range(3) for g, b in ((0, 6), (1, 6), (0, 4))]
    assert banks == [(8, [((6, 77, 2048), [0, 1, 2]), ((6, 77, 2048), [3, 4, 5]), ((4, 77, 2048), [6, 7])], 2)]


# ------------------------------------------------------------------------------------------------ supir_gather_segments: the ABI
def test_gather_segments_declared_mirrored_and_exported():
    fns = _header_functions()
    assert fns["supir_gather_segments"] == 4 == len(_lib.SIGNATURES["supir_gather_segments"])
    for lib in (_lib.load(), _lib.load(torch.float16)):
        assert hasattr(lib, "supir_gather_segments")
        assert lib.supir_abi_version() == 2
    assert not hasattr(_lib.load_f32(), "supir_gather_segments")


def test_gather_segments_rejects_bad_arguments_without_a_gpu():
    for lib in (_lib.load(), _lib.load(torch.float16)):
        assert lib.supir_gather_segments(None, 4, 4096, None) == ERR_ARG           # NULL table
        assert lib.supir_gather_segments(FAKE, 0, 4096, None) == ERR_ARG           # no segments
        assert lib.supir_gather_segments(FAKE, -3, 4096, None) == ERR_ARG
        assert lib.supir_gather_segments(FAKE, 4, 0, None) == ERR_ARG              # empty segments
        assert lib.supir_gather_segments(FAKE, 4, 4100, None) == ERR_ARG           # not a multiple of 16 bytes
        assert lib.supir_gather_segments(FAKE, 4, 8, None) == ERR_ARG
        assert lib.supir_gather_segments(FAKE + 4, 4, 4096, None) == ERR_ARG       # a table of pointers is 8-byte aligned
        assert lib.supir_gather_segments(FAKE, 70000, 4096, None) == ERR_ARG       # one grid row per segment: at most 65535


def test_segment_table_checks_its_segments_on_the_host():
    """ops.SegmentTable refuses what the kernel could not copy safely: misaligned or unequal segments, overlapping destinations."""
    buf, src = torch.zeros(64, dtype=torch.bfloat16), torch.ones(64, dtype=torch.bfloat16)
    assert not (buf.data_ptr() | src.data_ptr()) & 15          # torch's host allocator aligns to 64 bytes
    t = ops.SegmentTable([(buf[:16], src[:16]), (buf[16:48], src[16:48])])
    assert t.n == 2 and t.max_bytes == 64 and t.table.dtype == torch.int64
    assert t.table.tolist() == [[buf.data_ptr(), src.data_ptr(), 32], [buf.data_ptr() + 32, src.data_ptr() + 32, 64]]
    for pairs in ([], [(buf[:16], src[:8])], [(buf[:4], src[:4])], [(buf[4:12], src[:8])], [(buf[:8], src[4:12])],
                  [(buf[:16], src[:16]), (buf[8:24], src[16:32])], [(buf[:16], buf[8:24])], [(buf[:32:2], src[:16])]):
        with pytest.raises(_lib.SupirHipError):
            ops.SegmentTable(pairs)
