"""The rANS encoder's C boundary without a GPU: the three entries exist, refuse bad arguments before the device
is touched (fake non-null pointers, as tests/test_cabi_cpu.py does) and size a workspace only for arguments they accept."""
import ctypes

import pytest

INVALID, UNSUPPORTED = -1, -2
P = ctypes.c_void_p(16)            # non-null, 16-byte aligned, never dereferenced: every call below is refused on the host
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    from neuroquant_amd import _lib
    for name in ("nq_rans_encode_ws_bytes", "nq_rans_table", "nq_rans_encode"):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
    assert _lib.lib().nq_abi_version() == 7
    return _lib.lib()


def _encode(lib, levels=P, n=1000, n_bits=4, chunk=64, freq=P, states=P, offsets=P, words=P, ws=P, ws_bytes=BIG):
    return lib.nq_rans_encode(levels, n, n_bits, chunk, freq, states, offsets, words, ws, ws_bytes, None)


def _table(lib, levels=P, n=1000, n_bits=4, freq=P, ws=P, ws_bytes=BIG):
    return lib.nq_rans_table(levels, n, n_bits, freq, ws, ws_bytes, None)


@pytest.mark.parametrize("bad,code", [
    (dict(levels=None), INVALID), (dict(freq=None), INVALID), (dict(states=None), INVALID), (dict(offsets=None), INVALID),
    (dict(words=None), INVALID), (dict(ws=None), INVALID), (dict(n=0), INVALID), (dict(n=-5), INVALID),
    (dict(n_bits=0), INVALID), (dict(n_bits=9), INVALID), (dict(chunk=0), INVALID), (dict(chunk=-64), INVALID),
    (dict(chunk=100), INVALID), (dict(ws_bytes=0), INVALID), (dict(ws=ctypes.c_void_p(8)), INVALID),
    (dict(n=1 << 32), UNSUPPORTED), (dict(n=(1 << 32) + 7, chunk=4096), UNSUPPORTED),
])
def test_encode_refuses_before_the_device(lib, bad, code):
    assert _encode(lib, **bad) == code
    if not {"chunk", "states", "offsets", "words"} & set(bad):       # what the table entry takes as well
        assert _table(lib, **bad) == code


def test_workspace_size():
    from neuroquant_amd import _lib
    ws = _lib.lib().nq_rans_encode_ws_bytes
    for n, b, chunk in [(0, 4, 64), (-1, 4, 64), (1000, 0, 64), (1000, 9, 64), (1000, 4, 0), (1000, 4, 96), (1000, 4, -64),
                        (1 << 32, 4, 64)]:
        assert ws(n, b, chunk) == 0, (n, b, chunk)
    # partial histograms (one per 4096 levels, at most 1024), one count per chunk, a region of `chunk` words per chunk
    assert ws(1000, 4, 64) == 16 * 4 + 16 * 4 + 16 * 64 * 2
    assert ws(1000, 4, 4096) == 16 * 4 + 16 + 1024 * 2              # one chunk longer than the tensor: 1000 -> 1024 words
    assert ws(2642003, 6, 32768) == 646 * 64 * 4 + 336 + 81 * 32768 * 2
    assert ws((1 << 32) - 1, 8, 64) > 2 * ((1 << 32) - 1)
