"""mpmhip_adam_step as return codes, without a GPU (like tests/test_reg_abi.py): the check order of DESIGN.md section 10 -- a bad
argument is MPMHIP_ERR_INVALID whatever the device, a device that does not exist is MPMHIP_ERR_NO_DEVICE even for a request for
nothing -- and nothing is written on MPMHIP_ERR_INVALID.  Every call names device -1, so nothing is launched on any machine; the
tensor pointers are addresses of a host buffer nothing reads before the return."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mpmavatar_amd import _lib as L
from mpmavatar_amd import build as hipbuild
from mpmavatar_amd import optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mpmhip_adam_step"
# positions behind (device, stream, n_tensors)
PARAMS, GRADS, EXP_AVG, EXP_AVG_SQ, COUNTS, STEP_SIZE, BC2_SQRT, W1, BETA2, W2, EPS, UPDATE = range(12)


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return L.load()


class Request:
    """a valid request for n tensors of 5 elements each, every tensor pointer the address of `buf`"""

    def __init__(self, buf, n=3):
        self.n = n
        self.ptrs = [(C.c_void_p * n)(*[C.addressof(buf)] * n) for _ in range(4)]
        self.counts = (C.c_int64 * n)(*[5] * n)
        self.scalars = [np.full(n, 0.5, np.float32) for _ in range(6)]
        self.update = (C.c_uint8 * n)(*[1] * n)

    def args(self, **null):
        a = [C.addressof(x) for x in self.ptrs] + [C.addressof(self.counts)] + [s.ctypes.data for s in self.scalars] + [C.addressof(self.update)]
        for k in null:
            a[globals()[k]] = None
        return a


def test_the_library_was_built_from_adam_hip_and_the_header_declares_it(lib):
    assert "adam.hip" in hipbuild.SOURCES and "adam_math.hpp" in hipbuild.HEADERS
    header = open(os.path.join(ROOT, "include", "mpmhip.h")).read()
    assert hasattr(lib, NAME) and NAME in L.SIGNATURES and f"int {NAME}(" in header
    declared = re.search(r"int %s\((.*?)\);" % NAME, header, re.S).group(1).count(",") + 1
    assert declared == len(L.SIGNATURES[NAME][1]) == 15
    for cite in ("train_appearance.py:260-261", "scene/gaussian_model.py:207-234", "scene/mesh_gaussian_model.py:148-170"):
        assert cite in header, cite
    assert f"#define MPMHIP_ADAM_CHUNK {optim.ADAM_CHUNK}\n" in header and f"#define MPMHIP_ADAM_MAX_TENSORS {optim.MAX_TENSORS}\n" in header


def test_invalid_then_no_device_then_empty(lib):
    f = getattr(lib, NAME)
    buf = C.create_string_buffer(b"\x5a" * 256, 256)
    before = buf.raw
    r = Request(buf)
    assert f(-1, None, r.n, *r.args()) == L.ERR_NO_DEVICE
    assert f(-1, None, -1, *r.args()) == L.ERR_INVALID
    for k in ("PARAMS", "GRADS", "EXP_AVG", "EXP_AVG_SQ", "COUNTS", "STEP_SIZE", "BC2_SQRT", "W1", "BETA2", "W2", "EPS", "UPDATE"):
        assert f(-1, None, r.n, *r.args(**{k: None})) == L.ERR_INVALID, k                   # a NULL array
    for k in range(4):                                                                       # a NULL tensor with a positive count
        r = Request(buf)
        r.ptrs[k][1] = None
        assert f(-1, None, r.n, *r.args()) == L.ERR_INVALID, k
        r.counts[1] = 0                                                                      # ... is fine without elements
        assert f(-1, None, r.n, *r.args()) == L.ERR_NO_DEVICE, k
    r = Request(buf)
    r.counts[2] = -1
    assert f(-1, None, r.n, *r.args()) == L.ERR_INVALID
    r.counts[0] = r.counts[1] = 0
    assert f(-1, None, r.n, *r.args()) == L.ERR_INVALID                                      # an argument error wins over an empty request
    r.counts[2] = ((2 ** 31 - 1) // optim.MAX_TENSORS) * optim.ADAM_CHUNK + 1                # more than a launch can index
    assert f(-1, None, r.n, *r.args()) == L.ERR_INVALID
    # the device is checked even where there is nothing to do: no tensors (no arrays needed), only empty tensors
    assert f(-1, None, 0, *[None] * 12) == L.ERR_NO_DEVICE
    r = Request(buf)
    for i in range(r.n):
        r.counts[i] = 0
    assert f(-1, None, r.n, *r.args()) == L.ERR_NO_DEVICE
    assert buf.raw == before                                                                 # nothing was written through any pointer
