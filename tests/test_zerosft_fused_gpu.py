"""ops.zerosft_conv (supir_conv3x3_zerosft: the gamma|beta convolution of a ZeroSFT adapter with the GroupNorm + modulation + control-scale
lerp as its epilogue, SUPIR/modules/SUPIR_v0.py:62-113) against the two launches it replaces, against fp32 torch, its emitted GroupNorm
partials, graph replay and the refusal of operands outside its shapes.

Shapes: B = 2, a 16 x 16 map (256 tokens per batch element: one 256-row tile or two 128-row tiles), 128 conv input channels.
  Ccat 320            single source, 10-channel groups (a tile's 80 channels touch eight groups)
  Ccat 320 + 320      the concat boundary on a tile boundary
  Ccat 640 + 320      30-channel groups, one of them (channels 630..659) straddling the two sources
The producers of the two sources run on different tiles (128 / 256 rows), so their partial buffers have different numbers of tile rows."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from supir_amd import _lib, ops  # noqa: E402
from supir_amd import weights as Wt  # noqa: E402
from tests.helpers import synth_tensor  # noqa: E402

DEV = "cuda"
B, H, W, CIN = 2, 16, 16, 128
CASES = {"single320": (0, 320), "cat320+320": (320, 320), "cat640+320": (640, 320)}
TILES = (33, 34)
EPS = 1e-5
_CACHE = {}


def T(name, shape, dt=torch.float32, **kw):
    return synth_tensor(name, shape, **kw).to(DEV, dt)


def _cell(v):
    return torch.full((1,), v, dtype=torch.float32, device=DEV)


def _operands(case, dt):
    """Everything a case needs, built once and left unchanged: operands, the two-launch results and the fp32 reference per scale."""
    key = (case, dt)
    if key in _CACHE:
        return _CACHE[key]
    c1, c2 = CASES[case]
    C, M = c1 + c2, B * H * W
    o = dict(C=C, c1=c1, c2=c2)
    o["actv"] = T("zf.actv", (B, H, W, CIN), dt)
    w_mul, w_add = T("zf.wm", (C, 3, 3, CIN), dt, scale=0.03), T("zf.wa", (C, 3, 3, CIN), dt, scale=0.03)
    b_mul, b_add = T("zf.bm", (C,), scale=0.1), T("zf.ba", (C,), scale=0.1)
    o["w_cat"], o["b_cat"] = torch.cat([w_mul, w_add], 0).contiguous(), torch.cat([b_mul, b_add], 0).contiguous()
    o["w_il"], o["b_il"] = Wt.interleave_zerosft(w_mul, w_add, b_mul, b_add)
    o["gamma"], o["beta"] = T("zf.g", (C,), scale=0.2) + 1.0, T("zf.b", (C,), scale=0.2)
    h = T("zf.h", (M, 256), dt)
    # the producers: GEMMs that leave the GroupNorm partials of what they store (tile 34: one 256-row tile row per batch; 33: two)
    o["raw2"] = T("zf.r2", (M, c2), dt).view(B, H, W, c2)
    hz, o["pz"] = ops.gemm(h, T("zf.w2", (c2, 256), dt, scale=0.05), residual=o["raw2"].view(M, c2), rows_per_batch=H * W, gn_part=True, tile=34)
    o["hz"] = hz.view(B, H, W, c2)
    if c1:
        ho, o["po"] = ops.gemm(h, T("zf.w1", (c1, 256), dt, scale=0.05), rows_per_batch=H * W, gn_part=True, tile=33)
        o["ho"] = ho.view(B, H, W, c1)
        assert o["po"] is not None and o["po"].nchunk == 2
    assert o["pz"] is not None and o["pz"].nchunk == 1
    # fp32 torch on the same 16-bit operands: maps unrounded, statistics over the tensor (on the host: no second GPU library involved)
    x = torch.cat(([o["ho"]] if c1 else []) + [o["hz"]], -1).float().cpu()
    raw = torch.cat(([o["ho"]] if c1 else []) + [o["raw2"]], -1).float().cpu()
    gb = torch.nn.functional.conv2d(o["actv"].float().cpu().permute(0, 3, 1, 2), o["w_cat"].float().cpu().permute(0, 3, 1, 2),
                                    o["b_cat"].cpu(), padding=1).permute(0, 2, 3, 1)
    xn = torch.nn.functional.group_norm(x.permute(0, 3, 1, 2), 32, o["gamma"].cpu(), o["beta"].cpu(), EPS).permute(0, 2, 3, 1)
    y = xn * (gb[..., :C] + 1.0) + gb[..., C:]
    o["ref32"] = {cs: (y * cs + raw * (1.0 - cs)) if cs != 1.0 else y for cs in (1.0, 0.6)}
    o["two"] = {}
    torch.cuda.synchronize()
    _CACHE[key] = o
    return o


def _two_launch(o, cs, tile):
    """conv3x3 (concatenated weights) + groupnorm(mod_g, mod_b): the path the fused launch replaces.  cs: float or device cell.
    tile: the convolution's tile.  33 / 34 walk K in the order the fused launch on that tile does (two K groups / one), so the fp32
    accumulators -- and with them the rounded gamma|beta maps -- are identical and only the epilogue's contraction order can differ.
    -1 = whatever the autotuner picks: another K order moves an accumulator by ~1e-7 relative, which flips the 16-bit rounding of a map
    element now and then (a few per 100 000), and where the output is a near-cancellation that one flip is many ulps of the OUTPUT:
    printed, not asserted."""
    k = ("cell" if torch.is_tensor(cs) else cs, tile)
    if k not in o["two"]:
        C = o["C"]
        gb = ops.conv3x3(o["actv"], o["w_cat"], o["b_cat"], tile=tile)
        raw = o["raw2"] if (torch.is_tensor(cs) or cs != 1.0) else None
        if o["c1"]:
            out = ops.groupnorm(o["ho"], o["gamma"], o["beta"], EPS, x2=o["hz"], mod_g=gb[..., :C], mod_b=gb[..., C:], control_scale=cs,
                                x2raw=raw, part=o["po"], part2=o["pz"])
        else:
            out = ops.groupnorm(o["hz"], o["gamma"], o["beta"], EPS, mod_g=gb[..., :C], mod_b=gb[..., C:], control_scale=cs, x1raw=raw,
                                part=o["pz"])
        o["two"][k] = out
    return o["two"][k]


def _fused(o, cs, tile, out=None):
    raw = o["raw2"] if (torch.is_tensor(cs) or cs != 1.0) else None
    if o["c1"]:
        return ops.zerosft_conv(o["actv"], o["w_il"], o["b_il"], o["ho"], o["gamma"], o["beta"], EPS, x2=o["hz"], control_scale=cs, x2raw=raw,
                                part=o["po"], part2=o["pz"], tile=tile, out=out)
    return ops.zerosft_conv(o["actv"], o["w_il"], o["b_il"], o["hz"], o["gamma"], o["beta"], EPS, control_scale=cs, x1raw=raw, part=o["pz"],
                            tile=tile, out=out)


def _ordinal(t):
    """16-bit floats as integers that count representable values in order (one step = one ulp, across zero too)."""
    i = t.contiguous().view(torch.int16).int()
    return torch.where(i < 0, -(i & 0x7fff), i)


def _ulp_at(v, dt):
    """Spacing of the 16-bit type at magnitude v: the rounding of ONE output moves it by at most this."""
    return 2.0 ** (math.floor(math.log2(v)) - (7 if dt == torch.bfloat16 else 10))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", list(CASES))
def test_fused_vs_two_launches_fp32_and_partials(case, dt):
    o = _operands(case, dt)
    C = o["C"]
    assert ops.zerosft_conv_supported(B, H, W, CIN, C, o["c1"] or C, dt, o.get("po", o["pz"]), o["pz"] if o["c1"] else None)
    fails = []

    def chk(ok, *what):          # every tile / scale is measured and printed before the test fails
        if not ok:
            fails.append(what)

    for tile in TILES:
        for cs_name, cs in (("1.0", 1.0), ("0.6", 0.6), ("cell 0.6", _cell(0.6))):
            csf = 0.6 if torch.is_tensor(cs) else cs
            two, two_auto = _two_launch(o, cs, tile), _two_launch(o, cs, -1)
            out, part = _fused(o, cs, tile)
            torch.cuda.synchronize()
            d_auto = (_ordinal(out) - _ordinal(two_auto)).abs()
            print(f"{case} {dt} tile {tile} cs {cs_name}: vs the two launches with the AUTOTUNED convolution tile: {(d_auto != 0).float().mean().item():.2e} "
                  f"of the elements differ, worst {int(d_auto.max())} ulp, worst |difference| {(out.float() - two_auto.float()).abs().max().item():.3e}")
            # ---- the two-launch path: the same fp32 expression from identical 16-bit inputs, only contraction order can differ
            d = (_ordinal(out) - _ordinal(two)).abs()
            frac = (d != 0).float().mean().item()
            print(f"{case} {dt} tile {tile} cs {cs_name}: {frac:.2e} of the elements differ from the two-launch path, worst {int(d.max())} ulp")
            if int(d.max()) > 1:
                idx = (d > 1).nonzero()[:8]
                print("    beyond one ulp (index, fused, two-launch):", [(tuple(i.tolist()), out[tuple(i)].item(), two[tuple(i)].item()) for i in idx])
            chk(bool(torch.isfinite(out.float()).all()) and int(d.max()) <= 1, tile, cs_name, 'ulp', int(d.max()))
            if cs_name == "1.0":       # without the lerp the two paths are bitwise equal in every case, tile and element type (measured): held to that.
                # (With it, 2e-5 .. 2e-4 of the elements differ by one ulp: the lerp's two products contract differently in the two kernels.)
                chk(int(d.max()) == 0, tile, cs_name, 'bitwise', int(d.max()))
            # ---- fp32 torch: no further from it than the two launches, up to the rounding of one output
            ref = o["ref32"][csf].to(DEV)
            e_f, e_t = (out.float() - ref).abs().max().item(), (two.float() - ref).abs().max().item()
            bound = _ulp_at(ref.abs().max().item(), dt)
            print(f"    max |error| vs fp32 torch: fused {e_f:.3e}, two launches {e_t:.3e} (one output's rounding {bound:.3e})")
            chk(e_f <= e_t + bound, tile, cs_name, 'fp32', e_f, e_t)
            # ---- emitted partials: group statistics against fp64 sums over the tensor as stored (the bound of the producer-partials test
            # of tests/test_model_gpu.py: rstd to 1e-6 relative, mean to 1e-6 standard deviations)
            assert part is not None and part.C == C and part.unit == 10 and part.nchunk == (H * W) // (128 if tile == 33 else 256)
            assert tuple(part.buf.shape) == (B, part.nchunk, C // 10, 2)
            cpg = C // 32
            sums = part.buf.double().sum(1).reshape(B, 32, cpg // 10, 2).sum(2)
            n = H * W * cpg
            mean_p = sums[..., 0] / n
            var_p = (sums[..., 1] / n - mean_p * mean_p).clamp_min(0)
            gx = out.double().reshape(B, H * W, 32, cpg)
            mean_t = gx.mean(dim=(1, 3))
            var_t = ((gx * gx).mean(dim=(1, 3)) - mean_t * mean_t).clamp_min(0)
            r_p, r_t = 1.0 / torch.sqrt(var_p + EPS), 1.0 / torch.sqrt(var_t + EPS)
            e_r, e_m = ((r_p - r_t).abs() / r_t).max().item(), ((mean_p - mean_t).abs() / var_t.sqrt()).max().item()
            print(f"    emitted partials: worst rstd error {e_r:.2e}, worst mean error {e_m:.2e} std")
            chk(e_r <= 1e-6 and e_m <= 1e-6, tile, cs_name, 'partials', e_r, e_m)
            # each unit's (sum, sum of squares) itself, against fp64 over its 10 channels of its tile row: a value passes through at most
            # 16 (block rows) + 2 (blocks of a wave) + 8 (waves) + 10 (channels) fp32 additions, 36 x 2^-24 = 2.1e-6 of the sum of magnitudes
            ux = out.double().reshape(B, part.nchunk, (H * W) // part.nchunk, C // 10, 10)
            t_sum, t_sq = ux.sum(dim=(2, 4)), (ux * ux).sum(dim=(2, 4))
            scale = (ux.abs().sum(dim=(2, 4)) + 1.0)
            chk(((part.buf[..., 0].double() - t_sum).abs() / scale).max().item() <= 1e-5, tile, cs_name, 'unit sums')
            chk(((part.buf[..., 1].double() - t_sq).abs() / (t_sq + 1.0)).max().item() <= 1e-5, tile, cs_name, 'unit sums of squares')
    assert not fails, fails


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", list(CASES))
def test_graph_replay_and_device_cell(case, dt):
    """A captured launch replays bitwise what the eager launch computed; the device-cell form, captured ONCE, replayed with two cell values
    equals the two float-scale results."""
    o = _operands(case, dt)
    for tile in TILES:
        eager = {cs: _fused(o, cs, tile)[0] for cs in (1.0, 0.6)}
        cell = _cell(1.0)
        buf_f, buf_c = torch.empty_like(eager[1.0]), torch.empty_like(eager[1.0])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _fused(o, 0.6, tile, out=buf_f)
            _fused(o, cell, tile, out=buf_c)
        for v in (1.0, 0.6):
            cell.fill_(v)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(buf_f, eager[0.6]), (tile, v)
            assert torch.equal(buf_c, eager[v]), (tile, v)
        assert not torch.equal(eager[1.0], eager[0.6])


def test_ineligible_operands_are_refused():
    """An odd multiple of the channel unit, a tile without the epilogue and the fp32 dtype: the predicate says no, and the ABI entry returns an
    error code before any launch (fake pointers: a launch would fault)."""
    dt = torch.bfloat16
    o = _operands("cat640+320", dt)
    C, c1 = o["C"], o["c1"]
    assert ops.zerosft_conv_supported(B, H, W, CIN, C, c1, dt, o["po"], o["pz"])
    assert not ops.zerosft_conv_supported(B, H, W, CIN, C, c1, torch.float32, o["po"], o["pz"])
    assert not ops.zerosft_conv_supported(B, H, W, CIN, 480, 480, dt, static=True)          # 15-channel groups: no whole 10-channel units
    assert not ops.zerosft_conv_supported(B, H, W, CIN, 1120, 480, dt, static=True)         # 35-channel groups
    assert not ops.zerosft_conv_supported(B, H, W, CIN, 960, 600, dt, static=True)          # a tile would straddle the two sources
    assert not ops.zerosft_conv_supported(B, 8, 12, CIN, C, c1, dt, static=True)            # 96 tokens: no whole tile rows
    assert not ops.zerosft_conv_supported(B, H, W, CIN, C, c1, dt, None, o["pz"])           # a producer left no partials
    lib = _lib.load(dt)
    fake, st = 0x10000, torch.cuda.current_stream().cuda_stream

    def abi(C_=C, c1_=c1, tile=34, h=H, part1=fake):
        return lib.supir_conv3x3_zerosft(fake, fake, fake, fake, B, h, W, CIN, CIN, C_, C_, fake, fake, None, None, c1_, c1_, C_ - c1_, fake, fake,
                                         EPS, part1, 1, fake, 1, 1.0, None, tile, None, st)

    assert abi(C_=480, c1_=480) == -2
    assert abi(C_=1120, c1_=480) == -2
    assert abi(c1_=600) == -2
    for tile in (32, 35, 38, 42, 49, 50, -1):
        assert abi(tile=tile) == -2, tile
    assert abi(h=6) == -2
    assert abi(part1=None) == -1
    with pytest.raises(_lib.SupirHipError):
        _fused(o, 1.0, 32)
    torch.cuda.synchronize()
