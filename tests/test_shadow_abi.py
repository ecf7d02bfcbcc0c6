"""The three entry points of csrc/shadow.hip as return codes, without a GPU (like tests/test_shade_abi.py): the check order of
DESIGN.md section 10 -- a bad argument is MPMHIP_ERR_INVALID whatever the device, a device that does not exist is
MPMHIP_ERR_NO_DEVICE even for a request for nothing -- and nothing is written on MPMHIP_ERR_INVALID.  Every call names device -1, so
nothing is launched on any machine; the pointers are addresses of a host buffer nothing reads before the return."""
import ctypes as C
import os

import pytest

from mpmavatar_amd import _lib as L
from mpmavatar_amd import build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpmhip_shadow_workspace_bytes", "mpmhip_shadow_forward", "mpmhip_shadow_backward")


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return L.load()


@pytest.fixture()
def buf():
    return C.create_string_buffer(b"\x5a" * 256, 256)


def _desc(p, **change):
    """a valid request: one 33 x 33 map, shadow_size 20, uv_size 24, four channels, every pointer `p`"""
    d = L.ShadowDesc()
    d.n, d.in_h, d.in_w, d.shadow_size, d.uv_size, d.n_dims, d.lrelu_slope, d.beta = 1, 33, 33, 20, 24, 4, 0.2, 1.0
    d.ao_mean = d.tables = p
    for layer in range(9):
        for field in ("weight_v", "weight_g", "bias", "d_weight_v", "d_weight_g", "d_bias"):
            getattr(d, field)[layer] = p
    for k, v in change.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


def _sizes(lib, d):
    ws, tb = C.c_int64(-1), C.c_int64(-1)
    rc = lib.mpmhip_shadow_workspace_bytes(-1, None, C.byref(d), C.byref(ws), C.byref(tb), None)
    return rc, ws.value, tb.value


def test_the_library_was_built_from_shadow_hip_and_the_header_declares_all_three(lib):
    assert "shadow.hip" in hipbuild.SOURCES and "shadow_math.hpp" in hipbuild.HEADERS
    header = open(os.path.join(ROOT, "include", "mpmhip.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.SIGNATURES and f"int {n}(" in header
    assert "scene/shadow.py:14-181" in header and "train_appearance.py:120" in header and "shadow.py:135-181" in header
    assert "} mpmhip_shadow_desc;" in header and "#define MPMHIP_SHADOW_LAYERS 9" in header
    fields = [f for f, _ in L.ShadowDesc._fields_]
    body = header[header.rindex("typedef struct {", 0, header.index("} mpmhip_shadow_desc;")):header.index("} mpmhip_shadow_desc;")]
    at = -1
    for f in fields:                                        # the ctypes mirror names the header's fields in the header's order
        nxt = body.find(f, at + 1)
        assert nxt > at, f
        at = nxt
    assert C.sizeof(L.ShadowDesc) == 8 * 4 + 2 * 4 + 2 * 8 + 6 * 9 * 8
    assert [len(L.SIGNATURES[n][1]) for n in NAMES] == [6, 9, 9]


def test_workspace_bytes_is_host_arithmetic(lib, buf):
    p = C.addressof(buf)
    rc, ws, tb = _sizes(lib, _desc(p))
    assert rc == L.ERR_NO_DEVICE and ws > 0 and tb > 0 and ws % 16 == 0           # written whatever the device
    # the activations alone: 4 channels at 20, 10, 5, 2 and back up, plus the input gradients of the backward pass
    assert ws >= 4 * 4 * 2 * (400 + 100 + 25 + 4)
    assert tb == 4 * (2 * 20 + sum(7 * o + i + 1 for i, o in [(20, 10), (10, 5), (5, 2), (2, 5), (5, 10), (10, 20), (20, 24)]))
    assert _sizes(lib, _desc(p, n=3))[1] > ws and _sizes(lib, _desc(p, n_dims=8))[1] > ws
    assert _sizes(lib, _desc(p, uv_size=20))[2] < tb
    null = _desc(None)                                                              # the pointers of the descriptor are not read
    assert _sizes(lib, null) == (rc, ws, tb)
    for change in (dict(n=-1), dict(n=65536), dict(in_h=0), dict(in_w=8193), dict(shadow_size=7), dict(shadow_size=8193), dict(uv_size=0),
                   dict(n_dims=5), dict(n_dims=64), dict(untied_head_bias=2)):
        assert _sizes(lib, _desc(p, **change)) == (L.ERR_INVALID, -1, -1), change
    ws64, tb64 = C.c_int64(0), C.c_int64(0)
    assert lib.mpmhip_shadow_workspace_bytes(-1, None, None, C.byref(ws64), C.byref(tb64), None) == L.ERR_INVALID
    assert lib.mpmhip_shadow_workspace_bytes(-1, None, C.byref(_desc(p)), None, C.byref(tb64), None) == L.ERR_INVALID
    assert lib.mpmhip_shadow_workspace_bytes(-1, None, C.byref(_desc(p)), C.byref(ws64), None, None) == L.ERR_INVALID
    assert lib.mpmhip_shadow_workspace_bytes(-1, None, C.byref(_desc(p, n=0)), C.byref(ws64), C.byref(tb64), None) == L.ERR_NO_DEVICE


@pytest.mark.parametrize("name", NAMES[1:])
def test_invalid_then_no_device_then_empty(lib, buf, name):
    f, p = getattr(lib, name), C.addressof(buf)
    before = buf.raw
    _, ws, _ = _sizes(lib, _desc(p))

    def run(d, ws_bytes=ws, **change):
        if name == NAMES[1]:
            a = dict(ao=p, ws=p, out_ao=p, low=p, smap=p)
            a.update(change)
            return f(-1, None, C.byref(d), a["ao"], a["ws"], ws_bytes, a["out_ao"], a["low"], a["smap"])
        a = dict(ao=p, low=p, g_map=p, g_low=p, ws=p)
        a.update(change)
        return f(-1, None, C.byref(d), a["ao"], a["low"], a["g_map"], a["g_low"], a["ws"], ws_bytes)

    assert run(_desc(p)) == L.ERR_NO_DEVICE
    bad = [dict(n=-1), dict(in_h=0), dict(shadow_size=7), dict(uv_size=0), dict(n_dims=6), dict(untied_head_bias=-1), dict(lrelu_slope=-0.1),
           dict(lrelu_slope=float("nan")), dict(beta=float("inf")), dict(ao_mean=None), dict(tables=None), dict(weight_v=(0, None)),
           dict(weight_g=(8, None)), dict(bias=(4, None))]
    for change in bad:
        assert run(_desc(p, **change)) == L.ERR_INVALID, change
    assert f(-1, None, None, *([p] * 2 + [ws] + [p] * 3 if name == NAMES[1] else [p] * 5 + [ws])) == L.ERR_INVALID
    assert run(_desc(p), ws_bytes=ws - 4) == L.ERR_INVALID                          # a workspace that is too small
    assert run(_desc(p), ws=None) == L.ERR_INVALID and run(_desc(p), ao=None) == L.ERR_INVALID and run(_desc(p), low=None) == L.ERR_INVALID
    if name == NAMES[1]:
        assert run(_desc(p), smap=None) == L.ERR_INVALID
        assert run(_desc(p), out_ao=None) == L.ERR_NO_DEVICE                        # the resized input is optional
    else:
        assert run(_desc(p), g_map=None) == L.ERR_NO_DEVICE and run(_desc(p), g_low=None, g_map=None) == L.ERR_NO_DEVICE   # NULL = zero
        nothing = _desc(p)
        for layer in range(9):
            nothing.d_weight_v[layer] = nothing.d_weight_g[layer] = nothing.d_bias[layer] = None
        assert run(nothing) == L.ERR_NO_DEVICE                                      # nothing wanted is still a checked call
    # an argument error wins over the device, and over an empty request
    assert run(_desc(p, n=0, n_dims=5)) == L.ERR_INVALID
    assert run(_desc(p, n=0)) == L.ERR_NO_DEVICE
    assert run(_desc(p, untied_head_bias=1, n_dims=8, uv_size=20), ws_bytes=_sizes(lib, _desc(p, n_dims=8))[1]) == L.ERR_NO_DEVICE
    assert buf.raw == before                                                        # nothing was written through any pointer
