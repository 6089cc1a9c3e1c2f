"""Per-tile ("local") prompts on the fused, batched tiled samplers, on the GPU: supir_gather_segments against torch copies (bitwise),
and both tiled samplers with a list `cond` (SUPIR_model.py:168-178 -> sampling.py:609-616, 671-680), `tile_batch_local_prompts=True` and
tile batch 4 on the reduced-depth network -- one captured graph per group shape, the per-group embedding schedule, the per-image bank of
text K / V^T -- against the generic loop, under graph replay and eagerly."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from supir_amd import _lib, ops  # noqa: E402
from tests.helpers import build_unet, rel_l2, synth_tensor  # noqa: E402

DEV = "cuda"
H, W = 48, 64             # 32 x 32 tiles, stride 16: 6 tiles -> a group of 4 and a remainder group of 2 (two group shapes)
N_TILES = 6


def T(name, shape, dt=torch.float32, **kw):
    return synth_tensor(name, shape, **kw).to(DEV, dt)


# ------------------------------------------------------------------------------------------------ the gather kernel
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("sizes", [[16], [16, 48, 16], [4 << 20, 16, (4 << 20) + 16, 98560, 163840, 32, 2 << 20],
                                   [98560] * 33 + [163840] * 34])
def test_gather_segments_is_bitwise_the_torch_copies(dt, sizes):
    """Odd segment counts, 16-byte to multi-MB segments, through the bf16 and the fp16 library: the bytes torch's own copies move, and
    nothing outside the destinations."""
    lib = _lib.load(dt)
    total = sum(sizes)
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (total // 4 + 64,), dtype=torch.int32, device=DEV)
    dst = torch.full((total // 4 + 2 * len(sizes) * 4 + 64,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    want = dst.clone()
    pairs, so, do = [], 0, 4
    for nb in reversed(sizes):                 # destinations in another order than the sources, 16 guard bytes between them
        pairs.append((dst[do:do + nb // 4], src[so:so + nb // 4]))
        want[do:do + nb // 4] = src[so:so + nb // 4]
        so += nb // 4
        do += nb // 4 + 4
    table = ops.SegmentTable(pairs)
    assert table.n == len(sizes) and table.max_bytes == max(sizes)
    rc = lib.supir_gather_segments(table.table.data_ptr(), table.n, table.max_bytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(dst, want)
    dst.fill_(0)
    ops.gather_segments(table)                 # the wrapper (bf16 library), and a second launch of the same table
    # a max_segment_bytes below the longest segment only shrinks the grid
    assert lib.supir_gather_segments(table.table.data_ptr(), table.n, 16, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for d, s in pairs:
        assert torch.equal(d, s)


# ------------------------------------------------------------------------------------------------ samplers
def _setup():
    from supir_amd.modules.sampling import DiscreteDenoiserWithControl
    mini = build_unet(depth=(1, 1, 2), device=DEV)
    den = DiscreteDenoiserWithControl().to(DEV)
    ctx, y = T("context", (2, 77, 2048)), T("vector", (2, 2816))
    lq, xc = T("lq_tiled2", (1, 4, H, W)), T("fs.center2", (1, 4, H, W))
    local = [{"crossattn": T(f"lp.ctx{j}", (1, 77, 2048)), "vector": T(f"lp.vec{j}", (1, 2816)), "control": lq} for j in range(N_TILES)]
    uc = {"crossattn": ctx[1:], "vector": y[1:], "control": lq}

    def denoiser(i, s, cc, cs):
        return den(mini, i, s, cc, cs)

    return mini, den, denoiser, local, uc, xc


def _sampler(kind, **kw):
    from supir_amd.modules.sampling import LinearCFG, TiledRestoreDPMPP2MSampler, TiledRestoreEDMSampler
    if kind == "edm":
        return TiledRestoreEDMSampler(32, 16, num_steps=3, s_churn=5, s_noise=1.01, restore_cfg=4.0, guider_config=LinearCFG(1.0, 4.0),
                                      device=DEV, **kw)
    return TiledRestoreDPMPP2MSampler(32, 16, num_steps=4, s_noise=1.003, eta=1.0, restore_cfg=4.0, guider_config=LinearCFG(7.5, 4.0),
                                      device=DEV, **kw)


def _run(kind, smp, denoiser, cond, uc, xc, seed=321, x0="fs.x0t0"):
    torch.manual_seed(seed)
    kw = {"x_center": xc} if kind == "edm" else {}
    cond = [dict(cj) for cj in cond] if isinstance(cond, list) else dict(cond)
    with torch.no_grad():
        out = smp(denoiser, T(x0, (1, 4, H, W)).clone(), cond=cond, uc=dict(uc), control_scale=1.0, **kw).float().clone()
    return out, torch.randn(4, device=DEV)


def _modes(monkeypatch, kind, mini, den, denoiser, local, uc, xc, images=2):
    """generic (the torch-op loop, default kwarg: one tile per call) / fused / fused+graph with tile batch 4 over the prompts."""
    from supir_amd.modules import sampling
    res, stats = {}, None
    for mode in ("generic", "fused", "fused+graph"):
        if mode == "generic":
            denoiser.__dict__.pop("fused", None)
        else:
            denoiser.fused = (den, mini)
        monkeypatch.setattr(sampling, "FUSED_EDM_STEP", mode != "generic")
        monkeypatch.setattr(sampling, "EMB_SCHEDULE", True)
        smp = _sampler(kind, tile_batch=4) if mode == "generic" else _sampler(kind, tile_batch=4, tile_batch_local_prompts=True)
        mini.enable_graph(mode == "fused+graph")
        try:
            res[mode] = [_run(kind, smp, denoiser, local, uc, xc, 321 + img, f"fs.x0t{img}") for img in range(images)]
            if mode == "fused+graph":
                stats = mini.graph_stats()
        finally:
            mini.enable_graph(False)
        assert mini._sched is None and not mini._scheds and mini._bank is None
    return res, stats


@pytest.mark.parametrize("kind,steps", [("edm", 3), ("dpmpp", 4)])
def test_batched_local_prompts_replay_one_graph_per_group_shape_and_match_the_generic_loop(monkeypatch, kind, steps):
    """Two images in a row: captures <= the two group shapes, replays = steps x groups per image, nothing eager (without the feature a
    list `cond` never reaches the fused path: steps x tiles network calls of batch 2).  Against the generic loop with the default kwarg
    on the same seeds: the bars of tests/test_sampler_fused_gpu.py / tests/test_dpmpp_step_gpu.py for a global prompt (1e-2, same RNG
    consumption), and graph replay bitwise the eager fused path."""
    mini, den, denoiser, local, uc, xc = _setup()
    res, stats = _modes(monkeypatch, kind, mini, den, denoiser, local, uc, xc)
    print(f"[local prompts {kind}] graph stats over two images: {stats}")
    assert stats["captures"] <= 2 and stats["eager"] == 0 and stats["replays"] == 2 * steps * 2
    for mode in ("fused", "fused+graph"):
        for img in range(2):
            e = rel_l2(res[mode][img][0], res["generic"][img][0])
            print(f"[local prompts {kind} {mode}] image {img}: rel-L2 vs generic {e:.3e}")
            assert e <= 1e-2, (mode, img, e)
            assert torch.equal(res[mode][img][1], res["generic"][img][1])          # same RNG consumption
    for img in range(2):
        assert torch.equal(res["fused"][img][0], res["fused+graph"][img][0])       # graph == eager


@pytest.mark.parametrize("kind", ["edm", "dpmpp"])
def test_prompts_reach_their_tiles(monkeypatch, kind):
    """Swapping the prompts of tiles 0 and 5 (opposite corners: their windows do not overlap) changes the result inside both windows.
    One prompt given as a list of six reproduces the global-prompt fused result of the same build: the text K / V^T then come out of
    the bank's launch over all tiles instead of the stacked launch of a call.  MEASURED_SAME_PROMPT below is that distance as measured
    on the MI355X (profiles/local_prompts/); the bar is twice it, capped by the fused-vs-generic bar 1e-2.  Measured: 0.0 for both samplers -- the GEMMs give a row
    the same bits in either launch -- so the bar is 0: bitwise."""
    from supir_amd.modules import sampling
    mini, den, denoiser, local, uc, xc = _setup()
    denoiser.fused = (den, mini)
    monkeypatch.setattr(sampling, "FUSED_EDM_STEP", True)
    monkeypatch.setattr(sampling, "EMB_SCHEDULE", True)
    swapped = [local[5]] + local[1:5] + [local[0]]
    same = [dict(local[2]) for _ in range(N_TILES)]
    mini.enable_graph(True)
    try:
        base = _run(kind, _sampler(kind, tile_batch=4, tile_batch_local_prompts=True), denoiser, local, uc, xc)[0]
        swap = _run(kind, _sampler(kind, tile_batch=4, tile_batch_local_prompts=True), denoiser, swapped, uc, xc)[0]
        as_list = _run(kind, _sampler(kind, tile_batch=4, tile_batch_local_prompts=True), denoiser, same, uc, xc)[0]
        glob = _run(kind, _sampler(kind, tile_batch=4), denoiser, local[2], uc, xc)[0]
    finally:
        mini.enable_graph(False)
    tiles = sampling._sliding_windows(H, W, 32, 16)
    for j in (0, 5):
        hi, he, wi, we = tiles[j]
        d = rel_l2(swap[:, :, hi:he, wi:we], base[:, :, hi:he, wi:we])
        print(f"[local prompts {kind}] prompts of tiles 0 and 5 swapped: rel-L2 inside tile {j} = {d:.3e}")
        assert d > 0 and not torch.equal(swap[:, :, hi:he, wi:we], base[:, :, hi:he, wi:we]), (j, d)
    e = rel_l2(as_list, glob)
    print(f"[local prompts {kind}] one prompt as a list vs the global prompt: rel-L2 {e:.3e}")
    bar = min(2 * MEASURED_SAME_PROMPT[kind], 1e-2)
    assert e <= bar, (e, bar)


# one prompt as a list vs the same global prompt, fused + graph, tile batch 4 (rel-L2 measured on the MI355X, see the test above)
MEASURED_SAME_PROMPT = {"edm": 0.0, "dpmpp": 0.0}


@pytest.mark.parametrize("kind,steps", [("edm", 3), ("dpmpp", 4)])
@pytest.mark.parametrize("graph", [True, False])
def test_bank_serves_every_call_without_recomputing_text_kv(monkeypatch, kind, steps, graph):
    """Tile batch 2: three groups of ONE shape, so consecutive calls find another group's rows in the buffers.  After the per-image bank
    is built, refresh_static_conditioning is not called during the steps (without the bank: twice per network call), one gather launch
    serves every call, and after a call the resident K / V^T rows of EVERY text cross-attention layer equal the bank entries of that
    group's tiles bitwise."""
    from supir_amd.modules import sampling
    mini, den, denoiser, local, uc, xc = _setup()
    denoiser.fused = (den, mini)
    monkeypatch.setattr(sampling, "FUSED_EDM_STEP", True)
    monkeypatch.setattr(sampling, "EMB_SCHEDULE", True)
    count = {"refresh": 0, "at_bank": None, "checked": 0, "gathers": 0}
    for net in (mini.control_model, mini.diffusion_model):
        real = net.refresh_static_conditioning

        def counted(ctx, y, real=real):
            count["refresh"] += 1
            return real(ctx, y)

        monkeypatch.setattr(net, "refresh_static_conditioning", counted)
    real_bank = mini.prepare_context_bank

    def bank(*a, **k):
        ok = real_bank(*a, **k)
        count["at_bank"] = count["refresh"]
        assert ok and len(mini._bank["tables"]) == 3 and len(mini._bank["shapes"]) == 1
        assert len(mini._bank["layers"]) == len(mini.control_model.text_attentions()) + len(mini.diffusion_model.text_attentions()) > 0
        return ok

    monkeypatch.setattr(mini, "prepare_context_bank", bank)

    def after_call(mod, args, out):
        table = mod._bank["tables"][id(args[2]["crossattn"])][4]
        assert table.n == 2 * len(mod._bank["layers"])          # consecutive tiles: one segment per layer and operand
        for dst, src in zip(table.keep[0::2], table.keep[1::2]):
            assert torch.equal(dst, src)
        count["checked"] += 1
        count["gathers"] = mod._bank["gathers"]

    hook = mini.register_forward_hook(after_call)
    mini.enable_graph(graph)
    try:
        _run(kind, _sampler(kind, tile_batch=2, tile_batch_local_prompts=True), denoiser, local, uc, xc)
        stats = mini.graph_stats()
    finally:
        mini.enable_graph(False)
        hook.remove()
    assert count["at_bank"] == 2                    # once per network and group shape while the bank is built: the unconditional rows
    assert count["refresh"] == count["at_bank"]     # and never during the steps
    assert count["checked"] == count["gathers"] == 3 * steps
    if graph:
        assert stats == {"captures": 1, "replays": 3 * steps, "eager": 0}
    # the switch off: every call recomputes (what the bank is measured against)
    monkeypatch.setattr("supir_amd.modules.wrappers.CONTEXT_BANK", False)
    monkeypatch.setattr(mini, "prepare_context_bank", real_bank)
    count["refresh"] = 0
    mini.enable_graph(True)
    try:
        _run(kind, _sampler(kind, tile_batch=2, tile_batch_local_prompts=True), denoiser, local, uc, xc)
    finally:
        mini.enable_graph(False)
    # (the first call captures: its warm-up fills the buffers through the layers' own caches)
    assert mini._bank is None and count["refresh"] == 2 * (3 * steps - 1)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_group_schedule_rows_are_the_per_step_embeddings(dt):
    """UNetModel.prepare_schedule with a LIST of label vectors: row g * S + i of the table is bitwise what the single-vector schedule of
    group g holds at row i (same GEMMs, more rows)."""
    from supir_amd import weights as Wt
    mini = build_unet(depth=(1, 1, 2), device=DEV)
    mini.dtype = dt
    net = mini.diffusion_model
    t_values = [999, 750, 500, 250, 1]
    ys = [T(f"lp.sched.y{g}", (4, 2816)) for g in range(3)]
    row = torch.zeros(1, dtype=torch.int64, device=DEV)
    with torch.no_grad(), Wt.compute_dtype(mini.effective_dtype):
        net.prepare_schedule(t_values, ys, row)
        sch = net._schedule
        proj, raw = sch["proj"][:15].clone(), sch["raw"][:15].clone()
        assert sch["proj"].shape[0] >= 64
        for g, y in enumerate(ys):
            net.prepare_schedule(t_values, y, row)
            one = net._schedule
            assert torch.equal(one["proj"][:5], proj[5 * g:5 * g + 5]) and torch.equal(one["raw"][:5], raw[5 * g:5 * g + 5])
        net.end_schedule()
    assert not torch.equal(proj[:5], proj[5:10])
