"""The four entry points of csrc/lpips.hip as return codes, without a GPU (like tests/test_shadow_abi.py): the check order of
DESIGN.md section 10 -- a bad argument is MPMHIP_ERR_INVALID whatever the device, a device that does not exist is
MPMHIP_ERR_NO_DEVICE -- the workspace query as host arithmetic, and nothing written on MPMHIP_ERR_INVALID.  Every call names device
-1, so nothing is launched on any machine; the pointers are addresses of a host buffer nothing reads before the return."""
import ctypes as C
import os

import pytest

from mpmavatar_amd import _lib as L
from mpmavatar_amd import build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpmhip_lpips_prepare_weights", "mpmhip_lpips_workspace_bytes", "mpmhip_lpips_forward", "mpmhip_lpips_backward")


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return L.load()


@pytest.fixture()
def buf():
    return C.create_string_buffer(b"\x5a" * 256, 256)


def _desc(p, n=1, h=16, w=16, **change):
    """a valid request with every pointer `p`"""
    d = L.LpipsDesc()
    d.n, d.h, d.w = n, h, w
    for i in range(13):
        d.weight[i] = d.bias[i] = d.weight_bwd[i] = p
    for i in range(5):
        d.tap_weight[i] = p
    for c, (m, s) in enumerate(zip((-.030, -.088, -.188), (.458, .448, .450))):
        d.mean[c], d.std[c] = m, s
    for k, v in change.items():
        getattr(d, k)[v[0]] = v[1]
    return d


def _bytes(lib, d, keep=1):
    ws = C.c_int64(-1)
    return lib.mpmhip_lpips_workspace_bytes(-1, None, C.byref(d), keep, C.byref(ws)), ws.value


def test_the_library_was_built_from_lpips_hip_and_the_header_declares_all_four(lib):
    assert "lpips.hip" in hipbuild.SOURCES and "lpips_math.hpp" in hipbuild.HEADERS
    header = open(os.path.join(ROOT, "include", "mpmhip.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.SIGNATURES and f"int {n}(" in header
    assert "} mpmhip_lpips_desc;" in header and "#define MPMHIP_LPIPS_LAYERS 13" in header and "#define MPMHIP_LPIPS_TAPS 5" in header
    body = header[header.rindex("typedef struct {", 0, header.index("} mpmhip_lpips_desc;")):header.index("} mpmhip_lpips_desc;")]
    at = -1
    for f, _ in L.LpipsDesc._fields_:                       # the ctypes mirror names the header's fields in the header's order
        nxt = body.find(f, at + 1)
        assert nxt > at, f
        at = nxt
    assert C.sizeof(L.LpipsDesc) == 4 * 4 + (3 * 13 + 5) * 8 + 6 * 4
    assert [len(L.SIGNATURES[n][1]) for n in NAMES] == [3, 5, 9, 7]


def test_workspace_bytes_is_host_arithmetic(lib, buf):
    """it answers without a device, grows with n h w, is smaller when nothing is kept, and refuses h < 16"""
    p = C.addressof(buf)
    rc, base = _bytes(lib, _desc(p))
    assert rc == L.ERR_NO_DEVICE and base > 0                 # written although the device does not exist
    assert _bytes(lib, _desc(None))[1] == base                # the pointers are not read
    sizes = [_bytes(lib, _desc(p, n, h, w))[1] for n, h, w in ((1, 16, 16), (1, 32, 16), (1, 32, 32), (2, 32, 32), (2, 35, 22), (1, 72, 40))]
    assert sizes[0] < sizes[1] < sizes[2] < sizes[3]
    assert 0 < _bytes(lib, _desc(p), keep=0)[1] < base
    at_1024 = _bytes(lib, _desc(p, 1, 1024, 1024))[1]
    assert 3.0e9 < at_1024 < 3.4e9                            # 1.1 GB of x, 0.5 of y's taps, 0.5 of tap gradients, 1.1 of alternating buffers
    for bad in (dict(h=15), dict(w=15), dict(n=-1), dict(n=1025), dict(h=8193)):
        assert _bytes(lib, _desc(p, **bad)) == (L.ERR_INVALID, -1), bad
    assert lib.mpmhip_lpips_workspace_bytes(-1, None, C.byref(_desc(p)), 2, C.byref(C.c_int64())) == L.ERR_INVALID
    assert lib.mpmhip_lpips_workspace_bytes(-1, None, C.byref(_desc(p)), 1, None) == L.ERR_INVALID
    assert lib.mpmhip_lpips_workspace_bytes(-1, None, None, 1, C.byref(C.c_int64())) == L.ERR_INVALID


def test_arguments_then_device(lib, buf):
    p = C.addressof(buf)
    _, nbytes = _bytes(lib, _desc(p))
    fwd = lambda d, x=p, y=p, keep=1, ws=p, size=nbytes, out=p: lib.mpmhip_lpips_forward(-1, None, C.byref(d), x, y, keep, ws, size, out)
    bwd = lambda d, g=p, ws=p, size=nbytes, dx=p: lib.mpmhip_lpips_backward(-1, None, C.byref(d), g, ws, size, dx)
    assert fwd(_desc(p)) == bwd(_desc(p)) == lib.mpmhip_lpips_prepare_weights(-1, None, C.byref(_desc(p))) == L.ERR_NO_DEVICE
    assert fwd(_desc(p, n=0)) == L.ERR_NO_DEVICE              # a request for nothing still names a device
    assert fwd(_desc(p, weight_bwd=(3, None)), keep=0) == L.ERR_NO_DEVICE    # the backward layouts are not needed when nothing is kept
    for bad in (dict(weight=(0, None)), dict(bias=(12, None)), dict(tap_weight=(4, None)), dict(weight_bwd=(3, None)), dict(std=(1, 0.0)),
                dict(mean=(2, float("nan"))), dict(h=15)):
        assert fwd(_desc(p, **bad)) == L.ERR_INVALID, bad
    for bad in (dict(weight_bwd=(0, None)), dict(std=(0, float("inf"))), dict(w=8)):
        assert bwd(_desc(p, **bad)) == L.ERR_INVALID, bad
    assert fwd(_desc(p), x=None) == fwd(_desc(p), y=None) == fwd(_desc(p), out=None) == fwd(_desc(p), ws=None) == L.ERR_INVALID
    assert fwd(_desc(p), size=nbytes - 4) == fwd(_desc(p), keep=2) == L.ERR_INVALID
    assert bwd(_desc(p), g=None) == bwd(_desc(p), dx=None) == bwd(_desc(p), ws=None) == bwd(_desc(p), size=nbytes - 4) == L.ERR_INVALID
    assert bwd(_desc(p), size=_bytes(lib, _desc(p), keep=0)[1]) == L.ERR_INVALID     # a workspace that kept nothing
    assert lib.mpmhip_lpips_prepare_weights(-1, None, None) == L.ERR_INVALID
    assert lib.mpmhip_lpips_prepare_weights(-1, None, C.byref(_desc(p, weight_bwd=(7, None)))) == L.ERR_INVALID
    assert buf.raw == b"\x5a" * 256                           # nothing was written
