"""Prompts longer than 77 tokens, host side (no GPU): chunked tokenisation, chunked encoding of the two text towers against the
conditioner oracle run once per 77-token chunk, and the routing that keeps c and uc at one token count.

The towers run on tests/torch_ops.py in fp32 (the CPU stand-in of the kernels), at the real widths and head geometry of their
attention (CLIP-L 768 / 12 heads; an OpenCLIP tower of 128 / 2 heads) but two / three layers deep: chunking is a reshape around the
tower, not a property of its depth.  Tolerance: the 2e-5 of the fp32 one-chunk tower comparisons in tests/test_conditioner.py.
"""
import os

import pytest
import torch
import torch.nn as nn

from oracle import cond_oracle as CO
from tests.test_reference_test_py import write_byte_level_clip_vocab

BOS, EOS = 49406, 49407
LONG = "".join(chr(ord("a") + i % 26) for i in range(160))       # 160 bytes = 160 ids in the byte-level vocabulary: needs 3 chunks


@pytest.fixture(scope="module")
def vocab(tmp_path_factory):
    old = os.environ.get("SUPIR_CLIP_TOKENIZER")
    os.environ["SUPIR_CLIP_TOKENIZER"] = write_byte_level_clip_vocab(str(tmp_path_factory.mktemp("clip_vocab")))
    yield
    if old is None:
        del os.environ["SUPIR_CLIP_TOKENIZER"]
    else:
        os.environ["SUPIR_CLIP_TOKENIZER"] = old


def _todays_tokenize(texts, pad_zero):
    """The one-chunk tokenisation as it was before chunks existed (the reference's: truncate at 77, pad to 77)."""
    from transformers import CLIPTokenizer
    tok = CLIPTokenizer.from_pretrained(os.environ["SUPIR_CLIP_TOKENIZER"])
    ids = tok(list(texts), truncation=True, max_length=77, padding="max_length", return_tensors="pt")["input_ids"]
    if pad_zero:
        eot = ids.argmax(dim=-1)
        ids = ids * (torch.arange(77)[None] <= eot[:, None])
    return ids


# ------------------------------------------------------------------------------------------------ tokenisation
@pytest.mark.parametrize("pad_zero", [False, True])
def test_one_chunk_is_todays_tokenisation(vocab, pad_zero):
    from supir_amd.modules.conditioner import _tokenize
    texts = ["", "a cat", LONG]
    want = _todays_tokenize(texts, pad_zero)
    assert torch.equal(_tokenize(texts, pad_zero), want) and torch.equal(_tokenize(texts, pad_zero, chunks=1), want)
    assert want.shape == (3, 77) and want[2, 76] == EOS          # the over-long text is cut at 75 ids


@pytest.mark.parametrize("pad_zero", [False, True])
def test_chunked_tokenisation(vocab, pad_zero):
    from supir_amd.modules.conditioner import _tokenize
    pad = 0 if pad_zero else EOS
    # the prompt's own ids, from an untruncated call of the tokeniser without special tokens
    from transformers import CLIPTokenizer
    full = CLIPTokenizer.from_pretrained(os.environ["SUPIR_CLIP_TOKENIZER"])([LONG], add_special_tokens=False)["input_ids"][0]
    assert len(full) == 160 and full[:75] == _todays_tokenize([LONG], False)[0, 1:76].tolist()
    t3 = _tokenize([LONG], pad_zero, chunks=3)
    assert t3.shape == (1, 231) and t3.dtype == torch.int64
    want = ([BOS] + full[:75] + [EOS]) + ([BOS] + full[75:150] + [EOS]) + ([BOS] + full[150:] + [EOS] + [pad] * 65)
    assert t3[0].tolist() == want
    for j in range(3):
        assert t3[0, 77 * j] == BOS
    assert t3[0, 76] == EOS and t3[0, 153] == EOS and t3[0, 154 + 11] == EOS and (t3[0, 154 + 12:] == pad).all()
    # more chunks allowed than needed: still 3
    assert torch.equal(_tokenize([LONG], pad_zero, chunks=8), t3)
    # the cap: ids beyond 75 n are dropped, as truncation drops them at n = 1
    t2 = _tokenize([LONG], pad_zero, chunks=2)
    assert t2.shape == (1, 154) and torch.equal(t2, t3[:, :154])
    # a short and a long text in one call share n; the short one ends in empty chunks
    both = _tokenize(["a cat", LONG], pad_zero, chunks=3)
    assert both.shape == (2, 231) and torch.equal(both[1:], t3)
    assert torch.equal(both[0, :77], _todays_tokenize(["a cat"], pad_zero)[0])      # chunk 0 of a short prompt: what one chunk gives today
    empty = [BOS, EOS] + [pad] * 75
    assert both[0, 77:154].tolist() == empty and both[0, 154:].tolist() == empty
    # only short texts: one chunk, whatever the cap
    assert torch.equal(_tokenize(["a cat", ""], pad_zero, chunks=3), _todays_tokenize(["a cat", ""], pad_zero))


# ------------------------------------------------------------------------------------------------ towers
def _towers():
    """CLIP-L with 2 of its layers (hidden_states[2]) and a 3-layer OpenCLIP tower of width 128, random weights, on the CPU."""
    from supir_amd.modules import conditioner as C
    g_ = torch.Generator().manual_seed(11)
    with torch.device("meta"):
        cl = C.FrozenCLIPEmbedder(layer="hidden", layer_idx=2)
    enc = cl.transformer.text_model.encoder
    enc.layers = nn.ModuleList(list(enc.layers)[:2])
    cl = cl.to_empty(device="cpu")
    C._OC_ARCH["test-tiny"] = dict(vocab=49408, d=128, inner=512, layers=3, out_dim=96, heads=2)
    try:
        g = C.FrozenOpenCLIPEmbedder2(arch="test-tiny", layer="penultimate", always_return_pooled=True, legacy=False)
    finally:
        del C._OC_ARCH["test-tiny"]
    with torch.no_grad():
        for m in (cl, g):
            for k, t in m.state_dict().items():
                if not t.is_floating_point():
                    continue
                r = torch.randn(t.shape, generator=g_)
                if t.ndim == 0:
                    t.fill_(1.0)
                elif t.ndim == 1:
                    t.copy_(1.0 + 0.1 * r if k.endswith("weight") else 0.1 * r)          # LayerNorm scales near 1, biases small
                elif "embedding" in k:
                    t.copy_(0.5 * r)
                else:
                    t.copy_(r * t.shape[-1] ** -0.5)
    return cl.eval(), g.eval()


@pytest.fixture(scope="module")
def towers():
    return _towers()


def _tokens(n, chunks, seed):
    """[n, 77 chunks] ids: every chunk [BOS] ids [EOS] 0...; the EOS position differs per chunk and row (76 = a full chunk included)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(1000, 40000, (n, chunks, 77), generator=g)
    t[:, :, 0] = BOS
    pos = [76, 20, 1, 50]
    for i in range(n):
        for j in range(chunks):
            e = pos[(2 * i + j) % len(pos)]
            t[i, j, e] = EOS
            t[i, j, e + 1:] = 0
    return t.reshape(n, chunks * 77)


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def test_chunked_encode_vs_oracle_per_chunk(towers):
    from tests import torch_ops
    cl, g = towers
    tok = _tokens(2, 2, seed=3)
    with torch_ops.installed(fp32=True), torch.no_grad():
        z = cl(tok)
        pen, pooled = g(tok)
        z1 = cl(tok[:, :77])
    sd_l = {k: v.float() for k, v in cl.state_dict().items()}
    sd_g = {k: v.float() for k, v in g.state_dict().items()}
    with torch.no_grad():
        ref_z = torch.cat([CO.clip_l_hidden(sd_l, tok[:, 77 * j:77 * (j + 1)], layer_idx=2) for j in range(2)], 1)
        per = [CO.openclip_g_penultimate_pooled(sd_g, tok[:, 77 * j:77 * (j + 1)], heads=2) for j in range(2)]
    ref_pen = torch.cat([p[0] for p in per], 1)
    assert z.shape == (2, 154, 768) and pen.shape == (2, 154, 128) and pooled.shape == (2, 96)
    e = dict(clip=_rel(z, ref_z), pen=_rel(pen, ref_pen), pooled=_rel(pooled, per[0][1]))
    print("chunked towers vs per-chunk oracle:", {k: f"{v:.2e}" for k, v in e.items()})
    assert max(e.values()) <= 2e-5, e
    assert _rel(pooled, per[1][1]) > 0.1                 # the pooled output is chunk 0's, and chunk 1's is a different vector
    assert _rel(z[:, :77], z1) <= 1e-5                   # chunk 0 of a long prompt is what the one-chunk call gives
    assert _rel(z[:, 77:], z[:, :77]) > 0.1              # each chunk saw its own tokens at positions 0..76


def test_token_width_must_be_whole_chunks(towers):
    from tests import torch_ops
    cl, g = towers
    bad = _tokens(1, 2, seed=1)[:, :100]
    with torch_ops.installed(fp32=True):
        for tower in (cl, g):
            with pytest.raises(ValueError, match="77"):
                tower(bad)
            with pytest.raises(ValueError, match="77"):
                tower.encode_tokens(bad)


# ------------------------------------------------------------------------------------------------ routing
def _conditioner(towers):
    from supir_amd.modules import conditioner as C
    cond = C.GeneralConditionerWithControl([])
    cl, g = towers
    nd = C.ConcatTimestepEmbedderND(256)
    for e, key in ((cl, "txt"), (g, "txt"), (nd, "original_size_as_tuple")):
        e.input_key, e.ucg_rate = key, 0.0
    cond.embedders = nn.ModuleList([cl, g, nd])
    return cond


def test_c_and_uc_share_their_token_count(vocab, towers):
    from tests import torch_ops
    cond = _conditioner(towers)
    assert cond.prompt_chunks == 1
    batch = {"txt": [LONG, "a cat"], "original_size_as_tuple": torch.tensor([[1024, 1024], [512, 768]]), "control": torch.zeros(2, 4, 8, 8)}
    batch_uc = dict(batch, txt=["blurry", "blurry"])
    with torch_ops.installed(fp32=True):
        c1, uc1 = cond.get_unconditional_conditioning(batch, batch_uc)
        # "the attribute never existed": today's tokenisation straight into the towers, concatenated by hand
        cl, g = towers
        for b, got in ((batch, c1), (batch_uc, uc1)):
            pen, pooled = g.encode_tokens(_todays_tokenize(b["txt"], True))
            want_x = torch.cat([cl.encode_tokens(_todays_tokenize(b["txt"], False)), pen], 2)
            want_v = torch.cat([pooled, CO.concat_timestep_embedder_nd(b["original_size_as_tuple"])], 1)
            assert torch.equal(got["crossattn"], want_x) and torch.equal(got["vector"], want_v) and got["control"] is b["control"]
        assert c1["crossattn"].shape == (2, 77, 768 + 128)
        cond.prompt_chunks = 3
        c3, uc3 = cond.get_unconditional_conditioning(batch, batch_uc)
        cond.prompt_chunks = 2
        c2, uc2 = cond.get_unconditional_conditioning(batch, batch_uc)
        _, uc_only = cond.get_unconditional_conditioning(batch_uc, None)      # all short: one chunk whatever the cap
        # token tensors: taken as they are, the narrower side padded
        tk = _tokens(2, 2, seed=5)
        ct, uct = cond.get_unconditional_conditioning(dict(batch, txt=tk), dict(batch, txt=tk[:, :77]))
    assert c3["crossattn"].shape == uc3["crossattn"].shape == (2, 231, 768 + 128)
    assert c2["crossattn"].shape == uc2["crossattn"].shape == (2, 154, 768 + 128)
    assert c3["vector"].shape == uc3["vector"].shape == c1["vector"].shape
    assert uc_only["crossattn"].shape == (2, 77, 768 + 128)
    # chunk 0 of the short negative prompt is the one-chunk encoding; its other chunks are the encoding of an empty prompt, all alike
    # (the same rows in a taller batch: equal up to the GEMM's blocking, not bit for bit)
    same = lambda a, b: _rel(a, b) <= 1e-5  # noqa: E731
    assert same(uc3["crossattn"][:, :77], uc1["crossattn"]) and same(uc3["vector"], uc1["vector"])
    assert same(uc3["crossattn"][:, 77:154], uc3["crossattn"][:, 154:]) and not same(uc3["crossattn"][:, 77:154], uc3["crossattn"][:, :77])
    assert same(c3["crossattn"][1, :77], c1["crossattn"][1]) and same(c2["crossattn"], c3["crossattn"][:, :154])   # the cap drops chunks
    assert not same(c3["crossattn"][0, 77:154], c3["crossattn"][0, :77])
    assert ct["crossattn"].shape == uct["crossattn"].shape == (2, 154, 768 + 128)
    assert same(uct["crossattn"][0, 77:, :768], uct["crossattn"][1, 77:, :768])      # CLIP-L's empty chunk: [BOS] [EOS] EOS ...
    assert cond.prompt_chunks == 2


def test_prepare_condition_takes_prompt_chunks_by_name(vocab, towers):
    """SUPIRModel.prepare_condition on a stand-in `self`: the keyword (or model.prompt_chunks) reaches the conditioner for the call
    and is put back; per-tile prompts and the single uc share one chunk count."""
    import contextlib
    import inspect
    import types
    from tests import torch_ops
    from supir_amd.models.supir_model import SUPIRModel
    for fn in (SUPIRModel.prepare_condition, SUPIRModel.batchify_sample):
        assert inspect.signature(fn).parameters["prompt_chunks"].default is None
    cond = _conditioner(towers)
    cond.embedders = nn.ModuleList(list(cond.embedders)[:2])
    stub = types.SimpleNamespace(conditioner=cond, prompt_chunks=1, _ae_scope=contextlib.nullcontext)
    z = torch.zeros(1, 4, 8, 8)
    with torch_ops.installed(fp32=True):
        c, uc = SUPIRModel.prepare_condition(stub, z, [LONG[:100]], ", " + LONG[:40], "blurry", 1)
        assert c["crossattn"].shape == uc["crossattn"].shape == (1, 77, 896)
        c, uc = SUPIRModel.prepare_condition(stub, z, [LONG[:100]], ", " + LONG[:40], "blurry", 1, prompt_chunks=4)
        assert c["crossattn"].shape == uc["crossattn"].shape == (1, 154, 896) and cond.prompt_chunks == 1
        stub.prompt_chunks = 2
        cs, uc = SUPIRModel.prepare_condition(stub, z, [["short tile", LONG, "another"]], "", "blurry", 1)
        assert [ci["crossattn"].shape for ci in cs] == [(1, 154, 896)] * 3 and uc["crossattn"].shape == (1, 154, 896)
        assert cond.prompt_chunks == 1
