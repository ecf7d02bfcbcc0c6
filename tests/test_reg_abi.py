"""The four entry points of csrc/reg.hip as return codes, without a GPU (like tests/test_shade_abi.py): the check order of DESIGN.md
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
MESH = ("mpmhip_mesh_reg_forward", "mpmhip_mesh_reg_backward")
GAUSS = ("mpmhip_gauss_reg_forward", "mpmhip_gauss_reg_backward")
# positions behind (device, stream)
VERTS, N_VERTS, FACES, N_FACES, NB, ND, NW = range(7)
SCRATCH, TERMS, STATS, SQ_DIST = range(7, 11)                                  # mesh forward
B_STATS, B_G, V_START, V_ITEMS, D_STENCIL, D_VERTS = range(7, 13)              # mesh backward
N, OPACITY, XYZ, SCALING, RADII, VISIBLE, T_XYZ, T_SCALE = range(8)
G_SCRATCH, G_TERMS, N_VISIBLE = range(8, 11)                                   # Gaussian forward
B_N_VISIBLE, G_G, D_OPACITY, D_XYZ, D_SCALING = range(8, 13)                   # Gaussian backward


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return L.load()


@pytest.fixture()
def buf():
    return C.create_string_buffer(b"\x5a" * 256, 256)


def _args(name, p, **change):
    """a valid request: 1 face on 3 vertices / 1 Gaussian named by radii, every pointer `p`"""
    if name in MESH:
        a = [p, 3, p, 1, p, p, p] + [p] * (4 if name == MESH[0] else 6)
    else:
        a = [1, p, p, p, p, None, 1.0, 0.6] + [p] * (3 if name == GAUSS[0] else 5)
    for k, v in change.items():
        a[globals()[k]] = v
    return a


def test_the_library_was_built_from_reg_hip_and_the_header_declares_all_four(lib):
    assert "reg.hip" in hipbuild.SOURCES and "reg_math.hpp" in hipbuild.HEADERS
    assert "frames_math.hpp" in hipbuild.HEADERS        # the shared 3-vector and the binding's forward: a change rebuilds the objects
    header = open(os.path.join(ROOT, "include", "mpmhip.h")).read()
    for n in MESH + GAUSS:
        assert hasattr(lib, n) and n in L.SIGNATURES and f"int {n}(" in header
        declared = re.search(r"int %s\((.*?)\);" % n, header, re.S).group(1).count(",") + 1
        assert declared == len(L.SIGNATURES[n][1]), n
    for cite in ("train_appearance.py:136-150", "scene/mesh_gaussian_model.py:203-246", "scene/mesh_gaussian_model.py:88-98",
                 "utils/general_utils.py:286-316", "train_appearance.py:138,147,148", "scene/gaussian_model.py:158"):
        assert cite in header, cite
    assert "MPMHIP_MESH_REG_SCRATCH" in header and "MPMHIP_GAUSS_REG_SCRATCH" in header


@pytest.mark.parametrize("name", MESH)
def test_mesh_invalid_then_no_device_then_empty(lib, buf, name):
    f, p = getattr(lib, name), C.addressof(buf)
    before = buf.raw
    assert f(-1, None, *_args(name, p)) == L.ERR_NO_DEVICE
    bad = [dict(N_VERTS=-1), dict(N_FACES=-1), dict(N_FACES=2 ** 31 // 36 + 1), dict(VERTS=None), dict(FACES=None), dict(NB=None), dict(ND=None),
           dict(NW=None)]
    bad += [dict(SCRATCH=None), dict(TERMS=None), dict(STATS=None)] if name == MESH[0] else \
        [dict(B_STATS=None), dict(B_G=None), dict(V_START=None), dict(V_ITEMS=None), dict(D_STENCIL=None)]
    for change in bad:
        assert f(-1, None, *_args(name, p, **change)) == L.ERR_INVALID, change
    assert f(-1, None, *_args(name, p, N_FACES=0, N_VERTS=-1)) == L.ERR_INVALID       # an argument error wins over an empty request
    # valid forms reach the device check: no faces (no row pointers needed), and the optional pointers NULL
    empty = dict(N_FACES=0, VERTS=None, FACES=None, NB=None, ND=None, NW=None)
    if name == MESH[1]:
        empty.update(V_ITEMS=None, D_STENCIL=None)
    assert f(-1, None, *_args(name, p, **empty)) == L.ERR_NO_DEVICE
    optional = dict(SQ_DIST=None) if name == MESH[0] else dict(D_VERTS=None)
    assert f(-1, None, *_args(name, p, **optional)) == L.ERR_NO_DEVICE
    assert buf.raw == before                                                   # nothing was written through any pointer


@pytest.mark.parametrize("name", GAUSS)
def test_gauss_invalid_then_no_device_then_empty(lib, buf, name):
    f, p = getattr(lib, name), C.addressof(buf)
    before = buf.raw
    assert f(-1, None, *_args(name, p)) == L.ERR_NO_DEVICE
    assert f(-1, None, *_args(name, p, RADII=None, VISIBLE=p)) == L.ERR_NO_DEVICE      # the byte mask instead of the radii
    bad = [dict(N=-1), dict(OPACITY=None), dict(XYZ=None), dict(SCALING=None), dict(RADII=None), dict(VISIBLE=p)]   # neither, both
    bad += [dict(G_SCRATCH=None), dict(G_TERMS=None), dict(N_VISIBLE=None)] if name == GAUSS[0] else [dict(B_N_VISIBLE=None), dict(G_G=None)]
    for change in bad:
        assert f(-1, None, *_args(name, p, **change)) == L.ERR_INVALID, change
    assert f(-1, None, *_args(name, p, N=0, RADII=None)) == L.ERR_INVALID              # an argument error wins over an empty request
    assert f(-1, None, *_args(name, p, N=0, OPACITY=None, XYZ=None, SCALING=None)) == L.ERR_NO_DEVICE
    if name == GAUSS[1]:
        assert f(-1, None, *_args(name, p, D_OPACITY=None, D_XYZ=None, D_SCALING=None)) == L.ERR_NO_DEVICE       # nothing wanted
    assert buf.raw == before
