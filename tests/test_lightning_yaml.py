"""Boundary proof for BASELINE config 5: the reference's own `create_SUPIR_model` (SUPIR/util.py:34-51) on the reference's
`options/SUPIR_v0_Juggernautv9_lightning.yaml` builds THIS package's DPM++(2M) sampler with the YAML's parameters, and the same YAML
with the target swapped to the tiled class carries `tile_batch` / `tile_parallel` through its `params`.

CPU tier; needs the reference checkout (absent on the GPU box -> skipped there), like tests/test_boundary_reference_yaml.py."""
import pytest
import torch
import yaml

from oracle import ref_import
from tests.test_boundary_reference_yaml import _yaml_without_checkpoints, ref_util  # noqa: F401  (ref_util: fixture)

pytestmark = pytest.mark.skipif(not ref_import.available(), reason="reference checkout not mounted")

NAME = "SUPIR_v0_Juggernautv9_lightning.yaml"


def _build(ref_util, path):
    with ref_import.quiet():
        return ref_util.create_SUPIR_model(path, SUPIR_sign=None)


def test_lightning_yaml_builds_the_dpmpp_sampler(ref_util, tmp_path):  # noqa: F811
    import supir_amd.models.supir_model as M
    import supir_amd.modules.sampling as S
    path, cfg = _yaml_without_checkpoints(tmp_path, NAME)
    assert cfg["model"]["params"]["sampler_config"]["target"] == "sgm.modules.diffusionmodules.sampling.RestoreDPMPP2MSampler"
    model = _build(ref_util, path)
    assert type(model) is M.SUPIRModel and type(model.denoiser) is S.DiscreteDenoiserWithControl
    smp = model.sampler
    assert type(smp) is S.RestoreDPMPP2MSampler
    assert smp.s_noise == 1.003 and smp.eta == 1.0 and smp.num_steps == 100
    assert type(smp.guider) is S.LinearCFG and smp.guider.scale == 7.5 and smp.guider.scale_min == 4.0
    assert isinstance(smp.discretization, S.LegacyDDPMDiscretization)
    assert model.model.dtype == torch.float16 and model.ae_dtype == torch.bfloat16


@pytest.mark.parametrize("tile_batch,tile_parallel", [(4, False), (2, True)])
def test_lightning_yaml_with_the_tiled_sampler_carries_the_tile_kwargs(ref_util, tmp_path, tile_batch, tile_parallel):  # noqa: F811
    import supir_amd.modules.sampling as S
    path, _ = _yaml_without_checkpoints(tmp_path, NAME)
    cfg = yaml.safe_load(open(path))
    sc = cfg["model"]["params"]["sampler_config"]
    sc["target"] = "sgm.modules.diffusionmodules.sampling.TiledRestoreDPMPP2MSampler"
    sc["params"].update(tile_size=128, tile_stride=64, tile_batch=tile_batch, tile_parallel=tile_parallel)
    yaml.safe_dump(cfg, open(path, "w"))
    smp = _build(ref_util, path).sampler
    assert type(smp) is S.TiledRestoreDPMPP2MSampler
    assert smp.tile_size == 128 and smp.tile_stride == 64 and smp.tile_batch == tile_batch and smp.tile_parallel is tile_parallel
    assert smp.s_noise == 1.003 and smp.eta == 1.0 and smp.guider.scale == 7.5 and smp.guider.scale_min == 4.0
