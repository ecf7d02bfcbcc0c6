"""The two entry points of csrc/raster_extra.hip without a GPU: the header declares them and cites the reference's lines, _lib.py
binds them with as many arguments as the header declares, the library was built from the new source, and a call that names no
handle is MPMHIP_ERR_INVALID and writes nothing (nothing is launched on any machine)."""
import ctypes as C
import os
import re

import pytest

from mpmavatar_amd import _lib as L
from mpmavatar_amd import build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORWARD, BACKWARD = NAMES = ("mpmhip_raster_extra_forward", "mpmhip_raster_backward_extra")


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return L.load()


def test_the_header_declares_and_cites_and_the_library_binds(lib):
    assert "raster_extra.hip" in hipbuild.SOURCES and "raster_extra_math.hpp" in hipbuild.HEADERS
    header = open(os.path.join(ROOT, "include", "mpmhip.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.SIGNATURES and f"int {n}(" in header
        declared = re.search(r"int %s\((.*?)\);" % n, header, re.S).group(1).count(",") + 1
        assert declared == len(L.SIGNATURES[n][1]), n
    for cite in ("train_mesh_lbs_4ddress.py:260-277", ":299", ":306"):
        assert cite in header, cite
    block = header[header.index("extra attribute channels"):header.index("int mpmhip_raster_stats(")]
    for n in NAMES:                                                       # every entry's own line of the comment cites all three
        line = block[block.index(n):]
        line = line[:line.index("\n *   mpmhip") if "\n *   mpmhip" in line else line.index("MPMHIP_ERR_INVALID and nothing")]
        for cite in ("train_mesh_lbs_4ddress.py", ":260-277", ":299", ":306"):
            assert cite in line, (n, cite)
    # the backward entry is the old one plus four arguments; the old ones keep their signatures
    assert len(L.SIGNATURES[BACKWARD][1]) == len(L.SIGNATURES["mpmhip_raster_backward"][1]) + 4
    assert L.SIGNATURES[BACKWARD][1][:24] == L.SIGNATURES["mpmhip_raster_backward"][1]
    assert len(L.SIGNATURES["mpmhip_raster_backward"][1]) == 24 and len(L.SIGNATURES["mpmhip_raster_forward_grad"][1]) == 14


def test_the_python_signature_takes_extra_attrs():
    import inspect
    from mpmavatar_amd import rasterizer
    from mpmavatar_amd.compat import diff_gauss
    p = inspect.signature(rasterizer.GaussianRasterizer.forward).parameters
    assert list(p)[-1] == "extra_attrs" and p["extra_attrs"].default is None
    assert diff_gauss.GaussianRasterizer is rasterizer.GaussianRasterizer and rasterizer.MAX_EXTRA_ATTRS == 8


def test_no_handle_is_invalid_and_writes_nothing(lib):
    buf = C.create_string_buffer(b"\x5a" * 256, 256)
    p, before = C.addressof(buf), buf.raw
    cs = L.RasterSettings(2, 3, 0.5, 0.5, L.f3(0, 0, 0), 1.0, 0, p, p, p)
    for E in (0, 1, 8, 9):
        assert lib.mpmhip_raster_extra_forward(None, C.byref(cs), 1, p, E, p) == L.ERR_INVALID
        assert lib.mpmhip_raster_backward_extra(None, C.byref(cs), 1, p, None, 0, p, p, p, p, None, p, 64, 0, p, p, p, p, None, p, p, p, p, None,
                                                p, E, p, p) == L.ERR_INVALID
    assert buf.raw == before
