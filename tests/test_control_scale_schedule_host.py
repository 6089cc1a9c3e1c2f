"""Dynamic control scale, host side (no GPU): the per-step table the Restore-EDM samplers hand to the network under
`use_linear_control_scale` (sampling.py:557-559), the ControlWrapper's argument checks, and the three new C entry points
(supir_groupnorm_nhwc_dyn, supir_groupnorm_nhwc_parts_dyn, supir_gemm_bf16_ex_dyn)."""
import ctypes

import numpy as np
import pytest
import torch

from supir_amd import _lib, ops
from supir_amd.modules import sampling
from supir_amd.modules.sampling import SIGMA_MAX, DiscreteDenoiserWithControl, LinearCFG, RestoreEDMSampler, TiledRestoreEDMSampler
from supir_amd.modules.wrappers import ControlWrapper
from tests.test_abi import _header_functions

NEW = ("supir_groupnorm_nhwc_dyn", "supir_groupnorm_nhwc_parts_dyn", "supir_gemm_bf16_ex_dyn")


class _Net:
    """Stands in for ControlWrapper: records what the sampler prepares."""

    def __init__(self):
        self.prepared = []

    def prepare_schedule(self, t_values, vector, control=None, control_scales=None):
        self.prepared.append((list(t_values), control_scales))

    def select_step(self, i, expect_t=None):
        pass

    def end_schedule(self):
        pass


def _expected(steps, cs, cs0):
    """The reference's per-step expression (sampling.py:557-559) on the host sigmas, rounded as a ctypes float argument rounds it."""
    sig = sampling.LegacyDDPMDiscretization()(steps, device="cpu")
    return [ctypes.c_float((float(s) / SIGMA_MAX) * (cs0 - cs) + cs).value for s in list(sig)[:-1]]


def _run(monkeypatch, tiled, steps, cs, cs0, flag=True):
    monkeypatch.setattr(sampling, "DYNAMIC_CONTROL_SCALE", flag)
    monkeypatch.setattr(sampling, "EMB_SCHEDULE", True)
    monkeypatch.setattr(ops, "tile_blend", lambda *a, **k: None)
    net, den = _Net(), DiscreteDenoiserWithControl()
    kw = dict(num_steps=steps, s_churn=5, s_noise=1.01, restore_cfg=4.0, guider_config=LinearCFG(1.0, 4.0), device="cpu")
    smp = TiledRestoreEDMSampler(tile_size=8, tile_stride=4, tile_batch=4, **kw) if tiled else RestoreEDMSampler(**kw)
    smp._fused_ctx = lambda d, x: (den, net)
    seen = []

    def fused_step(ctx, sigma_f, next_sigma_f, x, gamma, x_center, eps_noise, control_scale, use_linear, start, cond_cat, sched_row=None,
                   tiles=None):
        seen.append(smp._linear_control_scale(sigma_f, control_scale, start) if use_linear else control_scale)
        return x if tiles is None else torch.zeros(len(tiles[0]), 4, 8, 8)

    smp._fused_step = fused_step
    h, w = (12, 16) if tiled else (8, 8)
    c = {"crossattn": torch.zeros(1, 77, 8), "vector": torch.zeros(1, 16), "control": torch.zeros(1, 4, h, w)}
    uc = {"crossattn": torch.ones(1, 77, 8), "vector": torch.ones(1, 16), "control": torch.zeros(1, 4, h, w)}
    smp(None, torch.zeros(1, 4, h, w), cond=c, uc=uc, x_center=torch.zeros(1, 4, h, w), control_scale=cs,
        use_linear_control_scale=True, control_scale_start=cs0)
    return net.prepared, seen


@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("steps", [12, 50])
@pytest.mark.parametrize("cs,cs0", [(1.0, 0.0), (0.8, 0.3)], ids=["lin_cs_12", "lin_cs_8"])
def test_sampler_table_is_the_fp32_of_the_per_step_expression(monkeypatch, tiled, steps, cs, cs0):
    prepared, seen = _run(monkeypatch, tiled, steps, cs, cs0)
    want = _expected(steps, cs, cs0)
    assert len(prepared) == (2 if tiled else 1)          # tiled: a group of 4 tiles and a remainder group of 2, one table each
    for t_values, table in prepared:
        assert len(table) == len(t_values) == steps
        assert [ctypes.c_float(v).value for v in table] == want
        assert np.array_equal(np.asarray(table, dtype=np.float64).astype(np.float32), np.asarray(want, dtype=np.float32))
    # and each step's call computes the same value the table holds for it
    per_step = seen if not tiled else seen[::2]
    assert [ctypes.c_float(v).value for v in per_step] == want


def test_flag_off_and_constant_scale_prepare_no_table(monkeypatch):
    for flag, lin in ((False, True), (True, False)):
        monkeypatch.setattr(sampling, "DYNAMIC_CONTROL_SCALE", flag)
        smp = RestoreEDMSampler(num_steps=4, device="cpu")
        assert smp._control_scales([3.0, 2.0, 1.0, 0.5, 0.0], 5, 1.0, lin, 0.0) is None
    prepared, _ = _run(monkeypatch, False, 12, 1.0, 0.0, flag=False)
    assert prepared[0][1] is None


def test_wrapper_table_and_length_check():
    class Stub(torch.nn.Module):
        def prepare_schedule(self, t_values, y, row, control=None):
            return 1

        def end_schedule(self):
            pass

    w = ControlWrapper(Stub(), dtype=torch.bfloat16)
    w.load_control_model(Stub())
    with pytest.raises(ValueError):
        w.prepare_schedule([900, 500, 100], torch.zeros(2, 16), control_scales=[1.0, 0.5])
    assert w._cs_table is None and w._sched is None      # rejected before anything was prepared
    vals = _expected(12, 0.8, 0.3)
    dbl = [(float(s) / SIGMA_MAX) * (0.3 - 0.8) + 0.8 for s in list(sampling.LegacyDDPMDiscretization()(12, device="cpu"))[:-1]]
    w.prepare_schedule(list(range(12)), torch.zeros(2, 16), control_scales=dbl)
    assert torch.equal(w._cs_table, torch.tensor(vals, dtype=torch.float32)) and w._cs_table.dtype == torch.float32
    w.select_step(5)
    assert float(w._cs_cell) == vals[5] and w._cs_row == 5
    assert w.graph_stats() == {"captures": 0, "replays": 0, "eager": 0}
    w.end_schedule()
    assert w._cs_table is None and w._cs_row is None


def test_new_entries_declared_exported_and_bound():
    fns = _header_functions()
    lib, lib16, lib32 = _lib.load(), _lib.load(torch.float16), _lib.load(torch.float32)
    for name, base, i in (("supir_groupnorm_nhwc_dyn", "supir_groupnorm_nhwc", 17),
                          ("supir_groupnorm_nhwc_parts_dyn", "supir_groupnorm_nhwc_parts", 17),
                          ("supir_gemm_bf16_ex_dyn", "supir_gemm_bf16_ex", 16)):
        assert fns[name] == fns[base] == len(_lib.SIGNATURES[name])
        sig, bsig = _lib.SIGNATURES[name], _lib.SIGNATURES[base]
        assert bsig[i] is ctypes.c_float and sig[i] is ctypes.c_void_p and sig[:i] == bsig[:i] and sig[i + 1:] == bsig[i + 1:]
        assert hasattr(lib, name) and hasattr(lib16, name), name
        assert not hasattr(lib32, name), name              # the fp32 service never captures graphs
    assert lib.supir_abi_version() == lib16.supir_abi_version() == _lib.ABI_VERSION == 2


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_null_cell_is_rejected_before_any_hip_call(dt):
    lib = _lib.load(dt)
    fake = 0x10000
    # supir_gemm_bf16_ex_dyn: everything valid but the cell
    assert lib.supir_gemm_bf16_ex_dyn(fake, fake, fake, 128, 640, 640, 640, 640, None, None, 0, 0, fake, 640, 0, 0, None, -1, None,
                                      None) == -1
    ws = 2 * 1024 * 64 * 4
    assert lib.supir_groupnorm_nhwc_dyn(fake, None, fake, None, 2, 64, 640, 640, 640, 0, fake, fake, 1e-5, 0, fake, fake, 640, None,
                                        fake, 640, fake, ws, None, None) == -1
    assert lib.supir_groupnorm_nhwc_parts_dyn(fake, None, fake, None, 2, 64, 640, 640, 640, 0, fake, fake, 1e-5, 0, fake, fake, 640,
                                              None, fake, 640, fake, 1, None, 0, None) == -1
    # a cell without the ZeroSFT modulation maps is not a form the dynamic entries have
    assert lib.supir_groupnorm_nhwc_dyn(fake, None, None, None, 2, 64, 640, 640, 640, 0, fake, fake, 1e-5, 0, None, None, 0, fake,
                                        fake, 640, fake, ws, None, None) == -1


def test_ops_rejects_a_malformed_cell():
    with pytest.raises(_lib.SupirHipError):
        ops._dyn_cell(torch.ones(2), torch.device("cpu"))
    with pytest.raises(_lib.SupirHipError):
        ops._dyn_cell(torch.ones(1, dtype=torch.float64), torch.device("cpu"))
    assert ops._dyn_cell(torch.ones(1), torch.device("cpu")) is True and ops._dyn_cell(0.5, torch.device("cpu")) is False
    x = torch.zeros(1, 4, 4, 32)
    with pytest.raises(_lib.SupirHipError):    # the fp32 service takes a float scale only
        ops.groupnorm(x.float(), torch.ones(32), torch.zeros(32), 1e-5, mod_g=x, mod_b=x, control_scale=torch.ones(1))
