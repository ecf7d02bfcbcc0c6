"""The entry points of csrc/densify.hip as return codes, without a GPU (like tests/test_reg_abi.py): the check order of DESIGN.md
section 10 -- a bad argument is MPMHIP_ERR_INVALID whatever the device, a device that does not exist is MPMHIP_ERR_NO_DEVICE even
for a request for nothing -- and nothing is written on MPMHIP_ERR_INVALID.  Every call names device -1, so nothing is launched on
any machine; the pointers are addresses of host buffers nothing reads before the return."""
import ctypes as C
import os
import re

import pytest

from mpmavatar_amd import _lib as L
from mpmavatar_amd import build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpmhip_densify_stats_add", "mpmhip_densify_scratch_bytes", "mpmhip_densify_plan", "mpmhip_densify_emit", "mpmhip_reset_opacity")
# positions behind (device, stream)
S_N, S_GRAD, S_RADII, S_VISIBLE, S_ACCUM, S_DENOM, S_MAX = range(7)                                                  # stats_add
P_N, P_FACES, P_SCALING, P_OPACITY, P_BINDING, P_FS, P_ACCUM, P_DENOM = range(8)                                     # plan
P_SCRATCH, P_BYTES, P_COUNTS = 13, 14, 15
E_N, E_FACES, E_OUT, E_XYZ, E_SCALING, E_ROTATION, E_BINDING, E_FS, E_NOISE, E_SCRATCH, E_BYTES, E_TENSORS = range(12)  # emit
E_IN, E_OUTS, E_WIDTHS, E_MODES, E_SRC, E_KIND, E_OBINDING, E_COUNTER = range(12, 20)


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return L.load()


@pytest.fixture()
def buf():
    return C.create_string_buffer(b"\x5a" * 256, 256)


def _table(p, widths=(3, 3), modes=(2, 3)):
    k = len(widths)
    return (C.c_void_p * k)(*[p] * k), (C.c_void_p * k)(*[p] * k), (C.c_int32 * k)(*widths), (C.c_int32 * k)(*modes)


def _args(name, p, table=None, **change):
    """a valid request for one Gaussian on one face, every pointer `p`"""
    if name == NAMES[0]:
        a = [1, p, p, None, p, p, p]
    elif name == NAMES[2]:
        a = [1, 1, p, p, p, p, p, p, 2.0 ** -12, 0.02, 0.005, 0.2, 1, p, 1 << 20, p]
    else:
        ins, outs, widths, modes = table
        a = [1, 1, 1, p, p, p, p, p, p, p, 1 << 20, len(widths), C.addressof(ins), C.addressof(outs), C.addressof(widths), C.addressof(modes), p, p, p, p]
    for k, v in change.items():
        a[globals()[k]] = v
    return a


def test_the_library_was_built_from_densify_hip_and_the_header_declares_all_five(lib):
    assert "densify.hip" in hipbuild.SOURCES and "densify_math.hpp" in hipbuild.HEADERS
    header = open(os.path.join(ROOT, "include", "mpmhip.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.SIGNATURES and f"int {n}(" in header
        declared = re.search(r"int %s\((.*?)\);" % n, header, re.S).group(1).count(",") + 1
        assert declared == len(L.SIGNATURES[n][1]), n
    for cite in ("scene/gaussian_model.py:378-526", "train_appearance.py:245-257", "utils/general_utils.py:116-137"):
        assert cite in header, cite
    from mpmavatar_amd import densify
    assert f"#define MPMHIP_DENSIFY_COUNTS {densify._N_COUNTS}" in header and f"#define MPMHIP_DENSIFY_MAX_TENSORS {densify._MAX_TENSORS}" in header


def test_stats_add_invalid_then_no_device_then_empty(lib, buf):
    f, p, name = lib.mpmhip_densify_stats_add, C.addressof(buf), NAMES[0]
    before = buf.raw
    assert f(-1, None, *_args(name, p)) == L.ERR_NO_DEVICE
    assert f(-1, None, *_args(name, p, S_RADII=None, S_VISIBLE=p)) == L.ERR_NO_DEVICE          # the byte mask instead of the radii
    for change in (dict(S_N=-1), dict(S_GRAD=None), dict(S_RADII=None), dict(S_VISIBLE=p), dict(S_ACCUM=None), dict(S_DENOM=None), dict(S_MAX=None)):
        assert f(-1, None, *_args(name, p, **change)) == L.ERR_INVALID, change
    assert f(-1, None, *_args(name, p, S_N=0, S_RADII=None)) == L.ERR_INVALID                  # an argument error wins over an empty request
    assert f(-1, None, *_args(name, p, S_N=0, S_GRAD=None, S_ACCUM=None, S_DENOM=None, S_MAX=None)) == L.ERR_NO_DEVICE
    assert buf.raw == before


def test_plan_and_scratch_bytes_invalid_then_no_device(lib, buf):
    f, p, name = lib.mpmhip_densify_plan, C.addressof(buf), NAMES[2]
    before = buf.raw
    assert f(-1, None, *_args(name, p)) == L.ERR_NO_DEVICE
    bad = [dict(P_N=-1), dict(P_FACES=-1), dict(P_N=2 ** 31 // 3 + 1), dict(P_SCRATCH=None), dict(P_COUNTS=None)]
    bad += [{k: None} for k in ("P_SCALING", "P_OPACITY", "P_BINDING", "P_FS", "P_ACCUM", "P_DENOM")]
    for change in bad:
        assert f(-1, None, *_args(name, p, **change)) == L.ERR_INVALID, change
    empty = dict(P_N=0, P_SCALING=None, P_OPACITY=None, P_BINDING=None, P_FS=None, P_ACCUM=None, P_DENOM=None)
    assert f(-1, None, *_args(name, p, **empty)) == L.ERR_NO_DEVICE                              # no Gaussians: no row pointers needed
    out = C.c_int64(-7)
    assert lib.mpmhip_densify_scratch_bytes(-1, 1, 1, C.byref(out)) == L.ERR_NO_DEVICE
    assert lib.mpmhip_densify_scratch_bytes(-1, -1, 1, C.byref(out)) == L.ERR_INVALID
    assert lib.mpmhip_densify_scratch_bytes(-1, 1, 1, None) == L.ERR_INVALID
    assert out.value == -7 and buf.raw == before


def test_emit_invalid_then_no_device(lib, buf):
    f, p, name = lib.mpmhip_densify_emit, C.addressof(buf), NAMES[3]
    before = buf.raw
    assert f(-1, None, *_args(name, p, _table(p))) == L.ERR_NO_DEVICE
    assert f(-1, None, *_args(name, p, _table(p), E_TENSORS=0, E_IN=None, E_OUTS=None, E_WIDTHS=None, E_MODES=None)) == L.ERR_NO_DEVICE
    bad = [dict(E_N=-1), dict(E_FACES=-1), dict(E_OUT=-1), dict(E_TENSORS=-1), dict(E_TENSORS=25), dict(E_SCRATCH=None), dict(E_IN=None),
           dict(E_WIDTHS=None), dict(E_SRC=None), dict(E_KIND=None), dict(E_OBINDING=None), dict(E_COUNTER=None)]
    bad += [{k: None} for k in ("E_XYZ", "E_SCALING", "E_ROTATION", "E_BINDING", "E_FS", "E_NOISE")]
    for change in bad:
        assert f(-1, None, *_args(name, p, _table(p), **change)) == L.ERR_INVALID, change
    for table in (_table(p, widths=(3, 0)), _table(p, modes=(2, 4)), _table(p, widths=(4, 3)), _table(None)):   # a width, a mode, xyz of width 4, NULL rows
        assert f(-1, None, *_args(name, p, table)) == L.ERR_INVALID
    assert buf.raw == before


def test_reset_opacity_invalid_then_no_device_then_empty(lib, buf):
    f, p = lib.mpmhip_reset_opacity, C.addressof(buf)
    before = buf.raw
    assert f(-1, None, 1, p, p) == L.ERR_NO_DEVICE and f(-1, None, 0, None, None) == L.ERR_NO_DEVICE
    for a in ((-1, p, p), (1, None, p), (1, p, None)):
        assert f(-1, None, *a) == L.ERR_INVALID, a
    assert buf.raw == before
