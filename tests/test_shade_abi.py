"""The two entry points of csrc/shade.hip as return codes, without a GPU (like tests/test_abi.py): the check order of DESIGN.md
section 10 -- a bad argument is MPMHIP_ERR_INVALID whatever the device, a device that does not exist is MPMHIP_ERR_NO_DEVICE even
for a request for nothing -- and nothing is written on MPMHIP_ERR_INVALID.  Every call names device -1, so nothing is launched on
any machine; the pointers are addresses of host buffers nothing reads before the return."""
import ctypes as C
import os

import pytest

from mpmavatar_amd import _lib as L
from mpmavatar_amd import build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpmhip_shade_colors", "mpmhip_shade_colors_backward")
# positions behind (device, stream)
N, N_FACES, BINDING, MEANS, CAMPOS, DEG, K, DC, REST, MAP, MAP_H, MAP_W, UV = range(13)
OUT = 13                                                                        # forward: out_colors
G, D_DC, D_REST, D_MEANS, F_START, F_ITEMS, T_START, T_ITEMS, D_MAP, SCRATCH = range(13, 23)


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return L.load()


@pytest.fixture()
def buf():
    b = C.create_string_buffer(b"\x5a" * 256, 256)
    return b


def _args(name, p, **change):
    """a valid request: 1 Gaussian, 1 face, degree 3 with 16 coefficients, a 2 x 2 map, every pointer `p`"""
    a = [1, 1, p, p, p, 3, 16, p, p, p, 2, 2, p] + [p] * (1 if name == NAMES[0] else 10)
    for k, v in change.items():
        a[globals()[k]] = v
    return a


def test_the_library_was_built_from_shade_hip_and_the_header_declares_both(lib):
    assert "shade.hip" in hipbuild.SOURCES and "shade_math.hpp" in hipbuild.HEADERS
    header = open(os.path.join(ROOT, "include", "mpmhip.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.SIGNATURES and f"int {n}(" in header
    assert "train_appearance.py:120-123" in header and ":31-47" in header
    assert lib.mpmhip_version() == 100
    assert len(L.SIGNATURES[NAMES[0]][1]) == 2 + 14 and len(L.SIGNATURES[NAMES[1]][1]) == 2 + 23


@pytest.mark.parametrize("name", NAMES)
def test_invalid_then_no_device_then_empty(lib, buf, name):
    f, p = getattr(lib, name), C.addressof(buf)
    before = buf.raw
    assert f(-1, None, *_args(name, p)) == L.ERR_NO_DEVICE
    bad = [dict(N=-1), dict(N_FACES=-1), dict(DEG=-1), dict(DEG=4), dict(K=15), dict(DEG=1, K=3), dict(MAP_H=0), dict(MAP_W=-2),
           dict(DC=None, MAP=None), dict(MEANS=None), dict(CAMPOS=None), dict(REST=None), dict(UV=None), dict(BINDING=None)]
    bad += [dict(OUT=None)] if name == NAMES[0] else [dict(SCRATCH=None), dict(F_START=None), dict(T_START=None), dict(F_ITEMS=None),
                                                      dict(T_ITEMS=None), dict(DC=None, D_DC=p), dict(MAP=None, D_MAP=p)]
    for change in bad:
        assert f(-1, None, *_args(name, p, **change)) == L.ERR_INVALID, change
    # an argument error wins over the device, and over an empty request
    assert f(-1, None, *_args(name, p, N=0, DEG=4)) == L.ERR_INVALID
    # valid forms reach the device check: no shadow map (binding, uv and the tables may be NULL), no features, n = 0, K = 1
    free = dict(MAP=None, UV=None, BINDING=None, MAP_H=0, MAP_W=0, N_FACES=0)
    if name == NAMES[1]:
        free.update(D_MAP=None, F_START=None, F_ITEMS=None, T_START=None, T_ITEMS=None, SCRATCH=None)
    assert f(-1, None, *_args(name, p, **free)) == L.ERR_NO_DEVICE
    no_features = dict(DC=None, REST=None, MEANS=None, CAMPOS=None, DEG=-5, K=0)
    if name == NAMES[1]:
        no_features.update(D_DC=None, D_REST=None, D_MEANS=None)
    assert f(-1, None, *_args(name, p, **no_features)) == L.ERR_NO_DEVICE
    assert f(-1, None, *_args(name, p, N=0)) == L.ERR_NO_DEVICE
    assert f(-1, None, *_args(name, p, N=0, MEANS=None, REST=None, BINDING=None)) == L.ERR_NO_DEVICE      # no rows: no row pointers
    k1 = dict(DEG=0, K=1, REST=None)
    if name == NAMES[1]:
        k1.update(D_REST=None)
    assert f(-1, None, *_args(name, p, **k1)) == L.ERR_NO_DEVICE
    if name == NAMES[1]:
        assert f(-1, None, *_args(name, p, G=None)) == L.ERR_NO_DEVICE                          # no upstream counts as zero
        assert f(-1, None, *_args(name, p, D_DC=None, D_REST=None, D_MEANS=None, D_MAP=None)) == L.ERR_NO_DEVICE   # nothing wanted
    assert buf.raw == before                                                   # nothing was written through any pointer
