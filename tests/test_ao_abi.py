"""The six entry points of csrc/ao.hip as return codes, without a GPU (like tests/test_shade_abi.py): a bad argument is
MPMHIP_ERR_INVALID whatever the device, a device that does not exist is MPMHIP_ERR_NO_DEVICE, and nothing is written either way.
Every call names device -1, so nothing is launched on any machine; the pointers are addresses of a host buffer nothing reads before
the return."""
import ctypes as C
import os

import pytest

from mpmavatar_amd import _lib as L
from mpmavatar_amd import build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mpmhip_ao_coverage", "mpmhip_ao_scratch_bytes", "mpmhip_ao_texel_frames", "mpmhip_ao_build_grid", "mpmhip_ao_trace", "mpmhip_ao_margin")


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return L.load()


def test_the_library_was_built_from_ao_hip_and_the_header_declares_all_six(lib):
    assert "ao.hip" in hipbuild.SOURCES and "ao_math.hpp" in hipbuild.HEADERS
    header = open(os.path.join(ROOT, "include", "mpmhip.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.SIGNATURES and f"int {n}(" in header
    for cite in ("train_material_params.py:819-822", "bake.py:37", "bake.py:50", "bake.py:73"):
        assert cite in header


def test_invalid_then_no_device(lib):
    buf = C.create_string_buffer(b"\x5a" * 256, 256)
    p, before = C.addressof(buf), buf.raw
    out = C.c_int64(-7)
    big = 1 << 40
    # (device, stream,) then a valid request with every pointer p; each entry of `bad` replaces arguments by position
    valid = {
        "mpmhip_ao_coverage": ([p, p, 2, p, 4, 8, 8, p, p], [{2: -1}, {4: -1}, {4: 0}, {5: 0}, {6: -3}, {5: 65536, 6: 65536}, {7: None}, {8: None}, {0: None}, {1: None}, {3: None}]),
        "mpmhip_ao_texel_frames": ([p, p, 2, 8, 8, p, p, p, p, p, p], [{2: -1}, {3: 0}, {4: 0}, {0: None}, {1: None}, {5: None}, {6: None}, {7: None}, {8: None}, {9: None}, {10: None}]),
        "mpmhip_ao_build_grid": ([p, p, 2, 64, 256, p, big], [{2: -1}, {3: 0}, {4: 0}, {5: None}, {0: None}, {1: None}]),
        "mpmhip_ao_trace": ([p, p, 2, p, p, p, 3, p, p, 16, 1e-4, 10.0, 64, 256, p, big, p],
                            [{2: -1}, {6: -1}, {9: 0}, {9: 4097}, {12: 0}, {13: 0}, {14: None}, {16: None}, {0: None}, {3: None}, {4: None}, {5: None}, {7: None}, {8: None}, {2: 0}]),
        "mpmhip_ao_margin": ([8, 8, p, p, p + 128, p + 192], [{0: 0}, {1: -1}, {2: None}, {3: None}, {4: None}, {5: None}, {4: p}, {5: p}]),
    }
    for name, (args, bad) in valid.items():
        f = getattr(lib, name)
        assert f(-1, None, *args) == L.ERR_NO_DEVICE, name
        for change in bad:
            a = list(args)
            for k, v in change.items():
                a[k] = v
            assert f(-1, None, *a) == L.ERR_INVALID, (name, change)
    assert lib.mpmhip_ao_scratch_bytes(-1, 2, 64, 256, C.byref(out)) == L.ERR_NO_DEVICE
    for a in ((-1, 64, 256), (2, 0, 256), (2, 64, 0)):
        assert lib.mpmhip_ao_scratch_bytes(-1, *a, C.byref(out)) == L.ERR_INVALID
    assert lib.mpmhip_ao_scratch_bytes(-1, 2, 64, 256, None) == L.ERR_INVALID
    # requests for nothing are valid and reach the device check: no faces, no covered texels
    assert lib.mpmhip_ao_coverage(-1, None, None, None, 0, None, 0, 8, 8, p, p) == L.ERR_NO_DEVICE
    assert lib.mpmhip_ao_build_grid(-1, None, None, None, 0, 64, 256, p, big) == L.ERR_NO_DEVICE
    assert lib.mpmhip_ao_trace(-1, None, None, None, 0, None, None, None, 0, None, None, 16, 1e-4, 10.0, 64, 256, p, big, p) == L.ERR_NO_DEVICE
    assert buf.raw == before and out.value == -7
