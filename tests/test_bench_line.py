"""The bench contract's stdout line stays small enough for the driver to parse (a 20 KB line -> `parsed: null`)."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _fake_full(n_kernels=60, shapes=12, text=3000):
    pmc = {"shape": "M2048 N1280 K1280", "algorithmic_bytes": 19005440.0, "fetch_bytes": 29089792.0, "write_bytes": 5242880.0,
           "fetch_plus_write_over_algorithmic": 1.81, "mfma_busy_over_sq_busy": 7.83, "mfma_busy_frac": 0.245}
    roof = {"kernel": "gemm16_kernel<128,80,2k,s3>", "bound": "mfma", "achieved": 487.9123456, "peak": 2500.0, "unit": "TFLOP/s",
            "frac": 0.19523456, "traffic": 56073625, "traffic_unit": "x" * 200, "traffic_over_algorithmic": 2.088,
            "traffic_launches_covered": "293 of 300", "launches_per_unet_step": 300, "avg_launch_us": 26.14,
            "algorithmic_gflop_per_launch": 12.756, "algorithmic_mb_per_launch": 21.433, "share_of_step_time": 0.226,
            "frac_graph_replay": 0.242, "avg_launch_us_graph_replay": 21.08, "graph_replay_source": "y" * 300,
            "shapes": [dict(pmc, traffic=dict(pmc)) for _ in range(shapes)]}
    cpu = {"unit": "images/s", "cores": 16, "kind": "port", "host_threads_available": 256, "thread_scan_seconds_per_256px_call": {16: 1.0, 32: 2.0},
           "unet_step_1024px_cfg_doubled_s": 17.24, "unet_step_1024px_tflops": 1.177, "config1_end_to_end_s": 14.33,
           "value": 0.0011259663365091042, "sample": "s" * text, "seconds_sample": 31.57082772254944}
    return {"metric": "1024px 50-step EDM denoise images/sec", "value": 0.6786874323244236, "unit": "images/s", "n_gpus": 1, "steps": 20,
            "warmup": 5, "ms_per_step": 1473.4323229989968, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
            "data": "synthetic", "config": {"workload": "w" * text, "edm_steps": 50, "resolution": 1024, "images_per_gpu_per_step": 1,
                                            "parallelism": "dp1", "hip_graph": True, "two_stream_overlap": True},
            "roofline": roof, "cpu_baseline": cpu, "output_finite": True, "end_to_end_tflops_per_gpu": 709.1,
            "kernel_breakdown_unet_step": {f"k{i}": {"launches": 3, "ms": 0.1, "tflops": 1.0} for i in range(n_kernels)},
            "roofline_by_kernel": [dict(roof) for _ in range(10)], "kernel_picks": {"mode": "box"}, "ms_per_unet_step": 28.74024353027344,
            "ms_per_unet_step_inside_the_sampler": 28.618, "unet_step_tflops": 705.66,
            "kernel_breakdown_vae_colorfix": {"wall_ms_eager": 36.9, "kernels": {f"k{i}": {"ms": 1.0} for i in range(20)}},
            "batched": {"images_per_call": 4, "images_per_s": 0.8655122154173842, "s_per_call": 4.62154078099411}}


def test_line_fits_and_round_trips():
    full = _fake_full()
    assert len(json.dumps(full)) > 20000          # the record that broke the driver's parse in round 5
    out = bench.compact_line(full, "gpurun_out/bench_details.json")
    assert "\n" not in out and len(out.encode()) <= bench.LINE_MAX_BYTES <= 4096
    line = json.loads(out)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["value"] == round(full["value"], 6) and line["steps"] == 20 and line["warmup"] == 5 and line["vs_baseline"] is None
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(line["roofline"])
    assert abs(line["roofline"]["frac"] - line["roofline"]["achieved"] / line["roofline"]["peak"]) < 1e-3
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(line["cpu_baseline"])
    assert "workload" in line["config"] and "model" not in line["config"]
    assert not any(isinstance(v, list) for v in line["roofline"].values())      # per-shape arrays live in the side file only
    assert line["details"] == "gpurun_out/bench_details.json"


def test_line_without_optional_legs():
    full = _fake_full()
    full.update(roofline=None, cpu_baseline=None)
    for k in ("batched", "kernel_breakdown_vae_colorfix", "ms_per_unet_step"):
        full.pop(k)
    line = json.loads(bench.compact_line(full))
    assert line["roofline"] is None and line["cpu_baseline"] is None and "details" not in line


def test_main_prints_the_compact_line_last():
    """bench.main's only stdout write is the compact line, and it is the final statement that writes to either stream on rank 0."""
    src = open(bench.__file__).read()
    body = src[src.index("def main():"):]
    assert body.count("print(") == 1 and "print(compact_line(full, details), flush=True)" in body
    after = body[body.index("print(compact_line"):]
    assert "log(" not in after


def test_only_the_line_reaches_stdout_even_when_a_library_writes_to_fd_1():
    """RCCL prints a version banner on fd 1 when its first communicator is created (five lines in front of the bench line under
    torch.distributed.run); bench.StdoutForTheLine sends every such write to stderr and hands the real stdout back for the line only."""
    code = ("import os, sys; sys.path.insert(0, %r); import bench\n"
            "g = bench.StdoutForTheLine()\n"
            "os.write(1, b'RCCL version : banner\\n'); print('python-level noise', flush=True)\n"
            "with g:\n    print('{\"the\": \"line\"}', flush=True)\n"
            "os.write(1, b'late noise\\n')\n") % os.path.dirname(os.path.abspath(bench.__file__))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    assert r.stdout == '{"the": "line"}\n', r.stdout
    assert "banner" in r.stderr and "python-level noise" in r.stderr and "late noise" in r.stderr


def test_replay_profile_kernel_names_match_the_kernels_template_arity():
    """bench.py finds the dominant kernel in the rocprofv3 CSV by a PREFIX of its demangled name.  The prefix must be a prefix of what the
    compiler prints for the instantiation the library actually contains (a template parameter appended to gemm16_kernel in round 6 silently
    cost one bench run its frac_graph_replay): check against the symbols of the built library."""
    import re
    import subprocess
    from supir_amd import _lib
    syms = subprocess.run(["nm", "-C", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    host_stubs = [l.split(" ", 2)[2] for l in syms.splitlines() if "gemm16_kernel<" in l or "geglu_big_kernel<" in l]
    norm = [re.sub(r"\s+", " ", s) for s in host_stubs]
    for trace_name in ("gemm16_kernel<128,80,2k,s3>", "gemm16_kernel<256,128,1k,s3,qkv>", "geglu_big_kernel<256,320,4x2>"):
        want = bench._rocprof_kernel_name(trace_name)
        assert want is not None
        if norm:
            assert any(want in s for s in norm), (trace_name, want)


def test_dump_outputs_writes_float32_and_samples_under_the_cap(tmp_path):
    """--dump-outputs: small outputs land whole as float32; larger ones become the same seeded sample on every run, under the cap."""
    import numpy as np
    import torch
    small = torch.linspace(-1, 1, 3 * 8 * 8, dtype=torch.bfloat16).reshape(1, 3, 8, 8)
    p = bench.dump_outputs({"samples": small}, str(tmp_path / "a"))
    got = np.load(p["samples"])
    assert got.dtype == np.float32 and got.shape == (1, 3, 8, 8) and np.array_equal(got, small.float().numpy())

    big = {"x": torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)), "y": torch.randn(5000, dtype=torch.float64)}
    cap = 40_000
    p1 = bench.dump_outputs(big, str(tmp_path / "b"), max_bytes=cap)
    p2 = bench.dump_outputs(big, str(tmp_path / "c"), max_bytes=cap)
    assert sum(os.path.getsize(f) for f in p1.values()) <= cap
    for name, t in big.items():
        a, b = np.load(p1[name]), np.load(p2[name])
        assert a.dtype == np.float32 and a.ndim == 1 and 0 < a.size < t.numel() and np.array_equal(a, b)
        assert np.isin(a, t.float().reshape(-1).numpy()).all()


@pytest.mark.gpu
def test_a_plain_run_only_times_dumps_and_prints(tmp_path):
    """Without --full bench.py sets up, warms up, times the steps, writes --dump-outputs and prints the line: none of the supplementary
    legs (ms per UNet step, kernel profiles, rocprofv3 replay, batched, CPU baseline) runs, and no side file is written."""
    import numpy as np
    cmd = [sys.executable, bench.__file__, "--steps", "1", "--warmup", "1", "--edm-steps", "2", "--res", "512", "--tune", "file",
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout)
    assert line["metric"] == "1024px 50-step EDM denoise images/sec" and line["unit"] == "images/s" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["steps"] == 1 and line["warmup"] == 1 and line["output_finite"] is True
    assert line["value"] > 0 and abs(line["ms_per_step"] - 1e3 / line["value"]) < 1e-3 * line["ms_per_step"]
    assert line["roofline"] is None and line["cpu_baseline"] is None
    for k in ("details", "ms_per_unet_step", "ms_per_unet_step_inside_the_sampler", "unet_step_tflops", "batched", "vae_colorfix_tail_ms"):
        assert k not in line, k
    samples = np.load(tmp_path / "out" / "samples.npy")
    assert samples.dtype == np.float32 and samples.shape == (1, 3, 512, 512) and np.isfinite(samples).all()
