"""The five entry points of csrc/image_head.hip as return codes, without a GPU (like tests/test_reg_abi.py): the check order of
DESIGN.md section 10 -- a bad argument is MPMHIP_ERR_INVALID whatever the device, a device that does not exist is
MPMHIP_ERR_NO_DEVICE -- and nothing is written on either.  Every call names device -1, so nothing is launched on any machine; the
pointers are addresses of host buffers nothing reads before the return."""
import ctypes as C
import os
import re

import pytest

from mpmavatar_amd import _lib as L
from mpmavatar_amd import build as hipbuild
from mpmavatar_amd import image_head

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORWARD, BACKWARD, BYTES, COMPOSE, PAIR = NAMES = ("mpmhip_image_head_forward", "mpmhip_image_head_backward", "mpmhip_image_head_bytes",
                                                   "mpmhip_image_compose", "mpmhip_eval_pair")
# positions behind (device, stream)
RENDER, MASK, CAM_M, CAM_C, N_CAM, CAM, H, W = range(8)                        # forward and backward
OUT_IMAGE = 8                                                                  # forward
G_IMAGE, SCRATCH, D_RENDER, D_MASK, D_CAM_M, D_CAM_C = range(8, 14)            # backward
B_WHITE, B_H, B_W, OUT_U8 = range(6, 10)                                       # bytes: render .. cam as above, then these
C_RGB, C_MSK, C_WHITE, C_H, C_W, C_OUT = range(6)                              # compose
P_PRED, P_GT, P_MASK, P_WHITE, P_H, P_W, P_OUT_PRED, P_OUT_GT = range(8)       # eval pair


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return L.load()


@pytest.fixture()
def buf():
    return C.create_string_buffer(b"\x5a" * 256, 256)


def _args(name, p, **change):
    """a valid request: 2 x 3 pixels, camera 1 of 2, every pointer `p`"""
    a = {FORWARD: [p, p, p, p, 2, 1, 2, 3, p], BACKWARD: [p, p, p, p, 2, 1, 2, 3, p, p, p, p, p, p], BYTES: [p, p, p, p, 2, 1, 0, 2, 3, p],
         COMPOSE: [p, p, 1, 2, 3, p], PAIR: [p, p, p, 1, 2, 3, p, p]}[name]
    for k, v in change.items():
        a[globals()[k]] = v
    return a


def test_the_library_was_built_from_image_head_hip_and_the_header_declares_all_five(lib):
    assert hipbuild.SOURCES[-1] == "image_head.hip" and "image_head_math.hpp" in hipbuild.HEADERS
    header = open(os.path.join(ROOT, "include", "mpmhip.h")).read()
    for n in NAMES:
        assert hasattr(lib, n) and n in L.SIGNATURES and f"int {n}(" in header
        declared = re.search(r"int %s\((.*?)\);" % n, header, re.S).group(1).count(",") + 1
        assert declared == len(L.SIGNATURES[n][1]), n
    for cite in ("train_appearance.py:126-127", "train_material_params.py:865-870", "train_material_params.py:865-876", "eval.py:68-87",
                 "train_appearance.py:108-110", "train_appearance.py:155"):
        assert cite in header, cite
    assert "MPMHIP_IMAGE_HEAD_SCRATCH" in header and "MPMHIP_IMAGE_HEAD_WORKGROUPS" in header


def test_the_scratch_macro_is_the_python_helper(tmp_path):
    """the macro of the header, evaluated by the C compiler, against image_head.scratch_doubles and image_head.workgroups"""
    import subprocess
    sizes = [(1, 1), (32, 32), (37, 29), (48, 64), (1024, 1024), (1024, 1025), (2160, 3840), (1, 2 ** 31 - 1), (46340, 46340)]
    src = tmp_path / "macro.c"
    rows = "\n".join('  printf("%%lld %%lld\\n", (long long)MPMHIP_IMAGE_HEAD_WORKGROUPS(%d, %d), (long long)MPMHIP_IMAGE_HEAD_SCRATCH(%d, %d));'
                     % (h, w, h, w) for h, w in sizes)
    src.write_text('#include <stdio.h>\n#include "mpmhip.h"\nint main(void) {\n%s\n  return 0;\n}\n' % rows)
    exe = tmp_path / "macro"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    for (h, w), line in zip(sizes, out):
        wg, doubles = (int(x) for x in line.split())
        assert wg == image_head.workgroups(h, w) and doubles == image_head.scratch_doubles(h, w) == 6 * wg, (h, w)
    assert image_head.workgroups(37, 29) == 2 and image_head.workgroups(1024, 1024) == 1024 == image_head.workgroups(4096, 4096)


@pytest.mark.parametrize("name", (FORWARD, BACKWARD))
def test_head_invalid_then_no_device(lib, buf, name):
    f, p = getattr(lib, name), C.addressof(buf)
    before = buf.raw
    assert f(-1, None, *_args(name, p)) == L.ERR_NO_DEVICE
    bad = [dict(RENDER=None), dict(MASK=None), dict(CAM_M=None), dict(CAM_C=None), dict(N_CAM=0), dict(N_CAM=-1), dict(CAM=-1), dict(CAM=2),
           dict(H=0), dict(W=0), dict(H=-1), dict(W=-3), dict(H=46341, W=46341), dict(H=2 ** 16, W=2 ** 15)]
    bad += [dict(OUT_IMAGE=None)] if name == FORWARD else [dict(SCRATCH=None), dict(SCRATCH=None, D_CAM_M=None), dict(SCRATCH=None, D_CAM_C=None)]
    for change in bad:
        assert f(-1, None, *_args(name, p, **change)) == L.ERR_INVALID, change
    assert f(-1, None, *_args(name, p, H=46340, W=46341)) == L.ERR_NO_DEVICE          # 2147441940 pixels: below 2^31 - 1
    assert f(-1, None, *_args(name, p, CAM=0)) == L.ERR_NO_DEVICE
    if name == BACKWARD:          # the optional pointers: no upstream gradient; each output not wanted; no scratch without a cam gradient
        for change in (dict(G_IMAGE=None), dict(D_RENDER=None), dict(D_MASK=None), dict(D_CAM_M=None), dict(D_CAM_C=None),
                       dict(SCRATCH=None, D_CAM_M=None, D_CAM_C=None), dict(D_RENDER=None, D_MASK=None, D_CAM_M=None, D_CAM_C=None)):
            assert f(-1, None, *_args(name, p, **change)) == L.ERR_NO_DEVICE, change
    assert buf.raw == before                                                   # nothing was written through any pointer


def test_bytes_invalid_then_no_device(lib, buf):
    f, p = lib.mpmhip_image_head_bytes, C.addressof(buf)
    before = buf.raw
    assert f(-1, None, *_args(BYTES, p)) == L.ERR_NO_DEVICE
    assert f(-1, None, *_args(BYTES, p, B_WHITE=1)) == L.ERR_NO_DEVICE
    assert f(-1, None, *_args(BYTES, p, CAM_M=None, CAM_C=None, N_CAM=0, CAM=0)) == L.ERR_NO_DEVICE       # the identity
    assert f(-1, None, *_args(BYTES, p, CAM_M=None, CAM_C=None, N_CAM=-5, CAM=9)) == L.ERR_NO_DEVICE      # ... looks at neither
    for change in (dict(RENDER=None), dict(MASK=None), dict(CAM_M=None), dict(CAM_C=None), dict(N_CAM=0), dict(CAM=-1), dict(CAM=2),
                   dict(B_H=0), dict(B_W=-1), dict(B_H=46341, B_W=46341), dict(OUT_U8=None)):
        assert f(-1, None, *_args(BYTES, p, **change)) == L.ERR_INVALID, change
    assert buf.raw == before


def test_compose_and_eval_pair_invalid_then_no_device(lib, buf):
    p = C.addressof(buf)
    before = buf.raw
    f = lib.mpmhip_image_compose
    assert f(-1, None, *_args(COMPOSE, p)) == L.ERR_NO_DEVICE
    for change in (dict(C_RGB=None), dict(C_MSK=None), dict(C_OUT=None), dict(C_H=0), dict(C_W=0), dict(C_H=-2), dict(C_H=65536, C_W=32768)):
        assert f(-1, None, *_args(COMPOSE, p, **change)) == L.ERR_INVALID, change
    f = lib.mpmhip_eval_pair
    assert f(-1, None, *_args(PAIR, p)) == L.ERR_NO_DEVICE
    for change in (dict(P_PRED=None), dict(P_GT=None), dict(P_MASK=None), dict(P_OUT_PRED=None), dict(P_OUT_GT=None), dict(P_H=0), dict(P_W=0),
                   dict(P_W=-2), dict(P_H=65536, P_W=32768)):
        assert f(-1, None, *_args(PAIR, p, **change)) == L.ERR_INVALID, change
    assert buf.raw == before
