"""The per-face forward of the mesh binding without a GPU: frm::face_frame_row of mpmavatar_amd/csrc/frames_math.hpp compiled with g++
(tests/hostframes/hostframes.cpp: the serial loop that mirrors k_face_frames) against tests/golden/frames.npz with the bounds the
GPU test asserts (tests/test_frames.py): mat 2e-6, scale 1e-6, center 5e-7 on the regular faces; finite and atol = 1e-5 on the five
degenerate ones; quat 5e-6 against oracle/face_frames.py with the same sign.  And what needs no tolerance: the branch, the two
statements of the matrix -> quaternion map in the header (the forward's one function, the backward's pieces) giving the same bits,
rows that do not depend on how many rows the call has, a call with nothing to do.  The per-Gaussian rows and cov_from_F are device
code only (frames.hip) and are tested on the GPU.  Every comparison prints its figures before it asserts (run with -s)."""
import os

import numpy as np
import pytest
import torch

import binding_grad_cases as bc
import binding_twin_torch as tw
from binding_grad_cases import _f32, _p

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames.npz"))
SLICES = (1, 255, 256, 257)     # around the 256 items of a workgroup


def test_host_frames_against_the_reference():
    n = int(GOLD["n_regular"])
    center, mat, quat, scale = bc.host_frames_forward(GOLD["verts"], GOLD["faces"])
    o_center, o_mat, o_quat, o_scale = bc.oracle_frames(GOLD["verts"], GOLD["faces"])
    errs = {"mat": np.abs(mat[:n] - GOLD["orientation"][:n]).max(), "scale": np.abs(scale[:n] - GOLD["scale"][:n]).max(),
            "center": np.abs(center - GOLD["center"]).max(), "quat": np.abs(quat[:n] - o_quat[:n]).max()}
    print(", ".join("%s %.3g of %.3g" % (k, v, bc.FRAME_TOL[k]) for k, v in errs.items()))
    for k, v in errs.items():
        assert v < bc.FRAME_TOL[k], k
    assert GOLD["faces"].shape[0] - n == 5
    assert np.isfinite(mat).all() and np.allclose(mat[n:], GOLD["orientation"][n:], atol=1e-5)      # the degenerate faces
    # on every regular face the forward takes the oracle's branch
    assert np.array_equal(bc.host_quat_branch(mat)[:n], tw.quat_branch(torch.from_numpy(o_mat))[0].numpy()[:n])


@pytest.mark.parametrize("name", ("frames",) + bc.CASES)
def test_the_two_statements_of_the_quaternion_map_give_the_same_bits(name):
    """frames_math.hpp states matrix -> quaternion as one function for the forward and as quat_branch / quat_numerators / norm4 for
    the backward; on the matrix the forward saved, the pieces give the quaternion the forward wrote, bit for bit, on every face"""
    verts, faces = (GOLD["verts"], GOLD["faces"]) if name == "frames" else (bc.case(name)["verts"], bc.case(name)["faces"])
    _, mat, quat, _ = bc.host_frames_forward(verts, faces)
    branch, again = bc.host_quat_from_pieces(mat)
    assert np.array_equal(quat, again, equal_nan=True)
    if name == "main":
        assert (np.bincount(branch, minlength=4) > 0).all()       # all four branches


@pytest.mark.parametrize("k", SLICES)
def test_rows_do_not_depend_on_the_row_count(k):
    full = bc.host_frames_forward(GOLD["verts"], GOLD["faces"])
    part = bc.host_frames_forward(GOLD["verts"], GOLD["faces"], n_f=k)
    for a, b in zip(part, full):
        assert a.shape[0] == k and np.array_equal(a, b[:k], equal_nan=True)


def test_a_call_with_nothing_to_do_writes_nothing():
    face = [np.full(s, np.nan, np.float32) for s in ((2, 3), (2, 3, 3), (2, 4), (2, 1))]
    bc.frames_lib().hfr_face_frames(_p(_f32(GOLD["verts"])), _p(np.ascontiguousarray(GOLD["faces"], np.int32)), 0, *[_p(a) for a in face])
    assert all(np.isnan(a).all() for a in face)
