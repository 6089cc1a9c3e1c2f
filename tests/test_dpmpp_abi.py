"""The DPM++(2M) step entries of the C ABI (supir_dpmpp2m_step_post / _tiles): declared in include/supir_hip.h, mirrored in
_lib.SIGNATURES with the header's argument counts, exported by both 16-bit builds (not by the fp32 library, whose export set is pinned),
and argument errors reported before any launch -- no GPU needed."""
import ctypes

import torch

from supir_amd import _lib
from tests.test_abi import _header_functions

NEW = ("supir_dpmpp2m_step_post", "supir_dpmpp2m_step_post_tiles")
FAKE = 0x10000          # never dereferenced: validation comes first
ERR_ARG, ERR_SHAPE = -1, -2


def test_declared_mirrored_and_exported():
    fns = _header_functions()
    for name in NEW:
        assert name in fns and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name]) == fns[name], (name, fns[name])
    assert fns["supir_dpmpp2m_step_post"] == 18 and fns["supir_dpmpp2m_step_post_tiles"] == 24
    for lib in (_lib.load(), _lib.load(torch.float16)):
        for name in NEW:
            assert hasattr(lib, name), name
        assert lib.supir_abi_version() == 2
    lib32 = _lib.load_f32()
    assert not any(hasattr(lib32, name) for name in NEW)


def _post(lib, net_out=FAKE, x=FAKE, old=None, eps=None, x_next=FAKE, den=FAKE, n=4096, reps=2):
    return lib.supir_dpmpp2m_step_post(net_out, x, old, eps, -1.5, 1.0, 4.0, 0.9, -0.1, 1.5, 0.5, 0.3, 1.003, x_next, den, n, reps, None)


def _tiles(lib, hw, k=None, b=1, C=4, Hc=64, Wc=64, T=32, reps=2, net_out=FAKE):
    arr = (ctypes.c_int * max(2, len(hw)))(*hw)
    k = len(hw) // 2 if k is None else k
    return lib.supir_dpmpp2m_step_post_tiles(net_out, FAKE, FAKE, None, -1.5, 1.0, 4.0, 0.9, -0.1, 1.5, 0.5, 0.3, 1.003, FAKE, FAKE, arr, k,
                                             b, C, Hc, Wc, T, reps, None)


def test_bad_arguments_return_error_codes_without_a_gpu():
    for lib in (_lib.load(), _lib.load(torch.float16)):
        # whole-batch entry
        assert _post(lib, net_out=None) == ERR_ARG and _post(lib, den=None) == ERR_ARG and _post(lib, x_next=None) == ERR_ARG
        assert _post(lib, n=0) == ERR_ARG and _post(lib, n=-4) == ERR_ARG
        assert _post(lib, reps=3) == ERR_ARG and _post(lib, reps=0) == ERR_ARG
        assert _post(lib, x=FAKE + 4) == ERR_SHAPE                       # misaligned (16-byte rule)
        assert _post(lib, old=FAKE + 8) == ERR_SHAPE and _post(lib, eps=FAKE + 12) == ERR_SHAPE
        assert _post(lib, n=4094) == ERR_SHAPE                           # CFG doubling needs n % 4 == 0
        # tile entry
        assert _tiles(lib, [0, 0], k=0) == ERR_ARG
        assert _tiles(lib, [0, 0] * 65) == ERR_ARG                       # k > 64
        assert _tiles(lib, [0, 0], reps=3) == ERR_ARG
        assert _tiles(lib, [0, 0], net_out=None) == ERR_ARG
        assert _tiles(lib, [0, 40]) == ERR_SHAPE                         # window past the right edge
        assert _tiles(lib, [0, 0, 33, 0]) == ERR_SHAPE                   # second window past the bottom edge
        assert _tiles(lib, [-1, 0]) == ERR_SHAPE
        assert _tiles(lib, [0, 0], b=70000, C=1) == ERR_SHAPE             # b * C over the grid limit
