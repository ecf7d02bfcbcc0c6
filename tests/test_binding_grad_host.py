"""The gradients of the mesh binding without a GPU: the twin (tests/binding_twin_torch.py) pinned against the reference's fixtures,
oracle/face_frames.py and SciPy; the measurement of G32, the constant the bound is built on; the conditions the cases must meet;
mpmavatar_amd/csrc/frames_grad_math.hpp compiled with g++ (tests/hostframes_grad/hostframes_grad.cpp: serial loops that mirror the
four kernels) against the float64 twin; a central-difference spot check of the twin; and the same file as a stand-alone program
under AddressSanitizer and UBSan.  Every comparison prints its figures before it asserts (run with -s)."""
import os
import subprocess

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation as Rot

import binding_grad_cases as bc
import binding_twin_torch as tw
from oracle import face_frames as ff

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- the twin is the reference -----------------------------------------------------------------------------------------------

def test_twin_forward_is_the_reference_fp32():
    """frames.npz and render_inputs.npz hold outputs of the reference's own functions on float32 inputs"""
    g = np.load(os.path.join(GOLD, "frames.npz"))
    n = int(g["n_regular"])
    center, mat, quat, scale = tw.face_frames(torch.from_numpy(g["verts"]), torch.from_numpy(g["faces"]))
    assert np.array_equal(mat.numpy(), g["orientation"]) and np.array_equal(scale.numpy(), g["scale"])   # the same torch expressions
    assert np.array_equal(center.numpy(), g["center"])
    assert np.isfinite(quat.numpy()[:n]).all()
    r = np.load(os.path.join(GOLD, "render_inputs.npz"))
    out = tw.render_inputs(*[torch.from_numpy(r[k]) for k in ("verts", "faces", "binding", "_xyz", "_rotation", "_scaling", "_opacity")])
    for k in bc.OUTS:
        err = np.abs(out[k].numpy() - r[k]).max()
        print(k, "max abs difference %.3g" % err)
        assert err <= 2e-6   # the fixture's quaternions came from the float32 NumPy oracle, everything else from the same expressions
    for k in ("means3D", "scales", "opacities"):
        assert np.abs(out[k].numpy() - r[k]).max() <= 1e-7


def test_twin_rotmat_to_unitquat_against_oracle_and_scipy():
    g = np.load(os.path.join(GOLD, "frames.npz"))
    n = int(g["n_regular"])
    R = g["orientation"][:n]
    q32 = tw.rotmat_to_unitquat(torch.from_numpy(R)).numpy()
    assert np.abs(q32 - ff.rotmat_to_unitquat_xyzw(R)).max() <= 2e-7          # same branch, same sign
    q64 = tw.rotmat_to_unitquat(torch.from_numpy(R.astype(np.float64))).numpy()
    assert np.abs(q64 - Rot.from_matrix(R.astype(np.float64)).as_quat()).max() < 1e-6
    c = bc.case("main")
    _, mat, _, _ = tw.face_frames(torch.tensor(c["verts"], dtype=torch.float64), torch.tensor(c["faces"]))
    q = tw.rotmat_to_unitquat(mat).numpy()
    assert np.abs(q - Rot.from_matrix(mat.numpy()).as_quat()).max() < 1e-12      # all four branches (the conditions below)


def test_twin_reproduces_the_reference_gradients():
    """tests/golden/binding_grad.npz: the reference's own compute_face_orientation and GaussianModel getters under autograd, float64"""
    c, g = bc.case("main"), bc.g64("main")
    for k in bc.NAMES:
        err = bc.rel_grad(g[k], c["d_" + k])
        print(k, "twin against the fixture %.3g" % err)
        assert c["d_" + k].dtype == np.float64 and err < 1e-13


def test_twin_against_central_differences():
    """an anchor independent of autograd: central differences of the float64 twin's loss on a handful of coordinates"""
    c, g = bc.case("main"), bc.g64("main")
    hot = int(c["hot_face"])

    def loss(t):
        out = tw.render_inputs(t["verts"], torch.from_numpy(c["faces"].astype(np.int64)), torch.from_numpy(c["binding"].astype(np.int64)),
                               t["_xyz"], t["_rotation"], t["_scaling"], t["_opacity"])
        return float(sum((torch.tensor(c["w_" + k], dtype=torch.float64) * out[k]).sum() for k in bc.OUTS))

    base = {k: torch.tensor(c[k], dtype=torch.float64) for k in bc.NAMES}
    spots = [("verts", int(c["faces"][hot, 0]), 0), ("verts", int(c["faces"][hot, 2]), 1), ("verts", 5, 2), ("_xyz", 3, 1),
             ("_rotation", 10, 0), ("_rotation", 11, 3), ("_scaling", 7, 2), ("_opacity", 20, 0)]
    h = 1e-6
    for k, i, j in spots:
        t = {n: v.clone() for n, v in base.items()}
        t[k][i, j] += h
        up = loss(t)
        t[k][i, j] -= 2 * h
        fd = (up - loss(t)) / (2 * h)
        print(k, i, j, "autograd %.9g central difference %.9g" % (g[k][i, j], fd))
        assert abs(fd - g[k][i, j]) <= 1e-6 * max(1.0, abs(g[k][i, j]))


# ---- the yardstick and the conditions of the comparison ---------------------------------------------------------------------------

def test_g32_is_the_measurement():
    worst = 0.0
    for name in bc.CASES:
        g32 = bc.twin_grads(bc.case(name), torch.float32)
        errs = {k: bc.rel_grad(g32[k], bc.g64(name)[k]) for k in bc.NAMES}
        print(name, ", ".join("%s %.3g" % kv for kv in errs.items()))
        worst = max(worst, max(errs.values()))
    print("G32 measured %.4g, committed %.4g" % (worst, bc.G32))
    assert 0.5 * bc.G32 < worst <= bc.G32
    assert bc.BOUND == 10 * bc.G32


def _frames(name, dtype):
    c = bc.case(name)
    v = torch.tensor(c["verts"], dtype=dtype)
    return v, tw.face_frames(v, torch.from_numpy(c["faces"].astype(np.int64)))


@pytest.mark.parametrize("name", bc.CASES)
def test_cases_meet_the_conditions(name):
    """over EVERY face and EVERY Gaussian: the quaternion branch is the same in float32 and float64; no clamp binds; on `main` all
    four branches are present, every one decided by more than 1e-3, and the index structure is the stated one.  (`render` is a
    nearly flat sheet: two branches, the closest decision 6.8e-4 -- four thousand float32 roundings of a matrix entry -- so for it the
    equality of the branches in both precisions is asserted, and a margin of 1e-4.)"""
    c = bc.case(name)
    choice, margin = {}, {}
    for dtype in (torch.float32, torch.float64):
        v, (center, mat, quat, scale) = _frames(name, dtype)
        choice[dtype], dm = tw.quat_branch(mat)
        top = dm.sort(-1, descending=True).values
        margin[dtype] = float((top[:, 0] - top[:, 1]).min())
        f = torch.from_numpy(c["faces"].astype(np.int64))
        e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
        a0, a1 = mat[:, :, 0], mat[:, :, 1]
        for x in (e1, torch.cross(a0, e2, dim=-1), torch.cross(a1, a0, dim=-1)):      # the three length() clamps at 1e-20
            assert float(tw.dot(x, x).min()) > 1e-10
        assert float(tw.dot(mat[:, :, 2], e2).abs().min()) > 1e-4                      # the |.| of the scale is away from its kink
        for q in (torch.tensor(c["_rotation"], dtype=dtype), quat):                     # the two normalize clamps at 1e-12
            assert float(torch.norm(q, dim=-1).min()) > 1e-3
    counts = np.bincount(choice[torch.float64].numpy(), minlength=4)
    print(name, "faces per branch", counts, "smallest margin %.3g (fp32) %.3g (fp64)" % (margin[torch.float32], margin[torch.float64]))
    assert torch.equal(choice[torch.float32], choice[torch.float64])
    if name == "main":
        assert (counts > 0).all() and min(margin.values()) > bc.MIN_MARGIN
        n_f, n = c["faces"].shape[0], c["binding"].shape[0]
        per_face = np.bincount(c["binding"], minlength=n_f)
        assert (c["verts"].shape[0], n_f, n) == (162, 320, 2 * 320 + 17) and n % 256 != 0
        assert per_face[int(c["hot_face"])] == 300 and (per_face[-5:] == 0).all() and (np.diff(c["binding"]) < 0).any()
    else:
        assert min(margin.values()) > 1e-4


# ---- frames_grad_math.hpp on the host against the float64 twin ---------------------------------------------------------------------

@pytest.mark.parametrize("name", bc.CASES)
def test_host_forward_agrees_with_the_oracle(name):
    """the saved frames the backward is fed come from the host build of the forward itself (frames_math.hpp); the oracle stays pinned
    to it within the bounds the device is held to (bc.FRAME_TOL), and both take the same quaternion branch on every face"""
    c = bc.case(name)
    got, want = bc.host_frames_forward(c["verts"], c["faces"]), bc.oracle_frames(c["verts"], c["faces"])
    for k, g, w in zip(("center", "mat", "quat", "scale"), got, want):
        err = np.abs(g - w).max()
        print(name, k, "%.3g of bound %.3g" % (err, bc.FRAME_TOL[k]))
        assert g.shape == w.shape and err < bc.FRAME_TOL[k], k
    assert np.array_equal(bc.host_quat_branch(got[1]), tw.quat_branch(torch.from_numpy(want[1]))[0].numpy())


@pytest.mark.parametrize("name", bc.CASES)
def test_host_gradients_against_float64(name):
    got, want = bc.host_grads(bc.case(name)), bc.g64(name)
    for k in bc.NAMES:
        err = bc.rel_grad(got[k], want[k])
        print(name, k, "%.3g of bound %.3g" % (err, bc.BOUND))
        assert np.isfinite(got[k]).all() and err <= bc.BOUND, k


def test_host_exact_zeros_and_null_upstreams():
    """faces without Gaussians get exactly zero frame gradients; a vertex in no face gets exactly zero; a null upstream counts as
    zero and gives exactly zero; n = 0 writes zeros to every face"""
    c = bc.case("main")
    n_f = c["faces"].shape[0]
    verts = np.concatenate([c["verts"], [[9.0, 9.0, 9.0]]]).astype(np.float32)          # one more vertex, in no face
    _, mat, quat, fscale = bc.host_frames_forward(verts, c["faces"])
    r = bc.host_binding_backward(n_f, c["binding"], c["_xyz"], c["_rotation"], c["_scaling"], c["_opacity"], mat, quat, fscale,
                                 c["w_means3D"], c["w_opacities"], c["w_scales"], c["w_rotations"])
    for t in r[4:]:
        assert (t[-5:] == 0).all() and (t[:-5] != 0).any()
    d_verts, _ = bc.host_frames_backward(verts, c["faces"], mat, quat, *r[4:])
    assert (d_verts[-1] == 0).all() and (d_verts[:-1] != 0).all()
    only_scales = bc.host_binding_backward(n_f, c["binding"], c["_xyz"], c["_rotation"], c["_scaling"], c["_opacity"], mat, quat, fscale,
                                           None, None, c["w_scales"], None)
    assert (only_scales[0] == 0).all() and (only_scales[1] == 0).all() and (only_scales[3] == 0).all() and (only_scales[2] != 0).any()
    assert (only_scales[4] == 0).all() and (only_scales[5] == 0).all() and (only_scales[6] == 0).all() and (only_scales[7][:-5] != 0).any()
    e = lambda w: np.zeros((0, w), np.float32)
    none = bc.host_binding_backward(n_f, np.zeros(0, np.int32), e(3), e(4), e(3), e(1), mat, quat, fscale, e(3), e(1), e(3), e(4))
    for t in none[4:]:
        assert t.shape[0] == n_f and (t == 0).all()


def test_stand_alone_program_under_sanitizers(tmp_path):
    """the loops over the main case's index structure (the empty faces, the 300-entry face), one more vertex in no face, and n = 0,
    as a stand-alone program built with -fsanitize=address,undefined: an index past a row or a table ends it with a report"""
    c = bc.case("main")
    path = tmp_path / "structure.bin"
    n_v = c["verts"].shape[0] + 1
    with open(path, "wb") as f:
        np.array([n_v, c["faces"].shape[0], c["binding"].shape[0]], np.int32).tofile(f)
        c["faces"].astype(np.int32).tofile(f)
        c["binding"].astype(np.int32).tofile(f)
    exe = bc.sanitizer_program()
    for args in ([str(path)], []):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        print(r.stdout.strip(), r.stderr.strip()[:2000])
        assert r.returncode == 0 and r.stdout.startswith("ok:"), (r.returncode, r.stderr[-2000:])
        if args:
            empty = int((np.bincount(c["binding"], minlength=320) == 0).sum())
            assert empty >= 5 and f"163 vertices (1 in no face), 320 faces ({empty} without Gaussians), 657 Gaussians" in r.stdout
