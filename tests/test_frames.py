"""Face frames and bound Gaussians.

CPU: oracle/face_frames.py against golden vectors produced by the REFERENCE's own compute_face_orientation
(tests/golden/frames.npz, tests/golden/make_golden_frames.py) -- this row of the oracle is pinned -- and the restated
roma quaternion helpers against SciPy.  GPU: the HIP kernels through the C ABI against the oracle and the fixture."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

from oracle import face_frames as ff

GOLD = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "frames.npz"))


def _inputs(seed=0, n_g=4000):
    rng = np.random.default_rng(seed)
    n_f = GOLD["faces"].shape[0]
    return dict(binding=rng.integers(0, int(GOLD["n_regular"]), n_g).astype(np.int32),
                xyz=rng.normal(0, 0.3, (n_g, 3)).astype(np.float32), rot=rng.normal(0, 1, (n_g, 4)).astype(np.float32),
                scl=rng.normal(-3, 0.5, (n_g, 3)).astype(np.float32)), n_f


def test_oracle_matches_the_reference_function():
    o, s = ff.compute_face_orientation(GOLD["verts"], GOLD["faces"])
    n = int(GOLD["n_regular"])
    assert np.abs(o[:n] - GOLD["orientation"][:n]).max() < 5e-7
    assert np.abs(s[:n] - GOLD["scale"][:n]).max() < 1e-7
    # degenerate / needle triangles: eps-clamped normalisation, same numbers as the reference (incl. zeros)
    assert np.allclose(o[n:], GOLD["orientation"][n:], atol=1e-6) and np.allclose(s[n:], GOLD["scale"][n:], atol=1e-7)
    m = ff.MeshFramesOracle(GOLD["faces"])
    m.set_mesh_by_verts(GOLD["verts"])
    assert np.abs(m.face_center - GOLD["center"]).max() < 2e-7


def test_quaternion_helpers_against_scipy():
    n = int(GOLD["n_regular"])
    R = GOLD["orientation"][:n].astype(np.float64)
    assert np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max() < 1e-5 and np.abs(np.linalg.det(R) - 1).max() < 1e-5
    q = ff.rotmat_to_unitquat_xyzw(R)
    qs = Rot.from_matrix(R).as_quat()
    assert np.abs(q - qs).max() < 1e-6               # same branch selection and sign as SciPy
    assert np.abs(Rot.from_quat(q).as_matrix() - R).max() < 1e-5
    rng = np.random.default_rng(1)
    a, b = rng.normal(size=(500, 4)), rng.normal(size=(500, 4))
    a, b = a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True)
    prod = ff.quat_product_xyzw(a.astype(np.float32), b.astype(np.float32))
    ref = (Rot.from_quat(a) * Rot.from_quat(b)).as_quat()
    assert np.minimum(np.abs(prod - ref).max(1), np.abs(prod + ref).max(1)).max() < 1e-5


@pytest.mark.gpu
def test_hip_frames_and_binding():
    import torch
    from mpmavatar_amd.mesh_frames import MeshFrames
    dev = torch.device("cuda:0")
    verts, faces = torch.from_numpy(GOLD["verts"]).to(dev), torch.from_numpy(GOLD["faces"]).to(dev)
    fr = MeshFrames(faces)
    fr.set_mesh_by_verts(verts)
    n = int(GOLD["n_regular"])
    mat, scl, ctr = fr.face_orien_mat.cpu().numpy(), fr.face_scaling.cpu().numpy(), fr.face_center.cpu().numpy()
    assert np.abs(mat[:n] - GOLD["orientation"][:n]).max() < 2e-6      # vs the reference's outputs
    assert np.abs(scl[:n] - GOLD["scale"][:n]).max() < 1e-6 and np.abs(ctr - GOLD["center"]).max() < 5e-7
    assert np.isfinite(mat).all() and np.allclose(mat[n:], GOLD["orientation"][n:], atol=1e-5)
    o = ff.MeshFramesOracle(GOLD["faces"])
    o.set_mesh_by_verts(GOLD["verts"])
    q = fr.face_orien_quat.cpu().numpy()
    assert np.abs(q[:n] - o.face_orien_quat[:n]).max() < 5e-6           # WXYZ, same sign convention
    assert np.abs(Rot.from_quat(q[:n][:, [1, 2, 3, 0]]).as_matrix() - GOLD["orientation"][:n]).max() < 1e-5
    inp, _ = _inputs()
    t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    xyz, rot, s3 = fr.get_all(t["binding"], t["xyz"], t["rot"], t["scl"])
    assert np.abs(xyz.cpu().numpy() - o.get_xyz(inp["binding"], inp["xyz"])).max() < 2e-6
    assert np.abs(rot.cpu().numpy() - o.get_rotation(inp["binding"], inp["rot"])).max() < 5e-6
    assert rel_ok(s3.cpu().numpy(), o.get_scaling(inp["binding"], inp["scl"]))
    assert np.abs(fr.get_xyz(t["binding"], t["xyz"]).cpu().numpy() - xyz.cpu().numpy()).max() == 0.0


def rel_ok(a, b, tol=2e-6):
    return bool((np.abs(a - b) <= tol * np.abs(b) + 1e-12).all())


# ---- the four forward kernels on small inputs, through the entry points --------------------------------------------------------------
# The first 257 faces of frames.npz and its five degenerate ones (TPB is 256: one full workgroup and a partial one), and the first 257
# Gaussians of render_inputs.npz on that fixture's own 198 faces, which their binding already lies in.  The inputs are a subset of the
# ones the bounds of test_hip_frames_and_binding and test_render_inputs.TOL were set on, rows do not depend on one another, so the
# bounds are those.  Keeping the Gaussians on their own mesh is what lets their rows be held to the fixture; the price is that
# the render kernel is never run here on frames of the small face set of frames.npz (test_hip_frames_and_binding binds 4000
# Gaussians to the whole of it).

N_SMALL = 257


def _small_mesh():
    n = int(GOLD["n_regular"])
    rows = np.r_[0:N_SMALL, n:GOLD["faces"].shape[0]]
    return rows, np.ascontiguousarray(GOLD["faces"][rows])


def _device_frames(verts, faces, n_f, rows=None):
    """mpmhip_face_frames over the first n_f faces into NaN-filled outputs of `rows` rows -> (center, mat, quat, scale) as numpy"""
    import torch
    from mpmavatar_amd._call import call
    dev = torch.device("cuda:0")
    v, f = torch.from_numpy(np.ascontiguousarray(verts)).to(dev), torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(dev)
    out = [torch.full((n_f if rows is None else rows, *s), float("nan"), device=dev) for s in ((3,), (3, 3), (4,), (1,))]
    call("mpmhip_face_frames", dev, v.data_ptr(), f.data_ptr(), n_f, *[t.data_ptr() for t in out])
    return [t.cpu().numpy() for t in out]


def _device_render(n_g, n_x, rows=None):
    """mpmhip_render_inputs over the first n_g Gaussians and the first n_x `extra` rows of render_inputs.npz, on that fixture's mesh,
    into NaN-filled outputs of `rows` rows -> dict of numpy arrays"""
    import torch
    import test_render_inputs as tri
    from mpmavatar_amd._call import call
    R = tri.GOLD
    dev = torch.device("cuda:0")
    t = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    frames = [torch.from_numpy(a).to(dev) for a in _device_frames(R["verts"], R["faces"], R["faces"].shape[0])]
    ins = [t(R["binding"], np.int32)] + [t(R[k]) for k in ("_xyz", "_rotation", "_scaling", "_opacity")]
    ext = [t(R["extra_" + k]) for k in ("xyz", "opacity", "scales", "rotations")]
    out = {k: torch.full((n_g + n_x if rows is None else rows, w), float("nan"), device=dev)
           for k, w in (("means3D", 3), ("means2D", 3), ("opacities", 1), ("scales", 3), ("rotations", 4))}
    call("mpmhip_render_inputs", dev, n_g, n_x, *[a.data_ptr() for a in ins], *[a.data_ptr() for a in frames], *[a.data_ptr() for a in ext],
         *[a.data_ptr() for a in out.values()])
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.gpu
def test_hip_small_frames_match_the_fixture_and_the_host_branch():
    import torch
    import binding_grad_cases as bc
    import binding_twin_torch as tw
    rows, faces = _small_mesh()
    center, mat, quat, scl = _device_frames(GOLD["verts"], faces, faces.shape[0])
    n = N_SMALL
    assert np.abs(mat[:n] - GOLD["orientation"][rows][:n]).max() < 2e-6
    assert np.abs(scl[:n] - GOLD["scale"][rows][:n]).max() < 1e-6 and np.abs(center - GOLD["center"][rows]).max() < 5e-7
    assert np.isfinite(mat).all() and np.allclose(mat[n:], GOLD["orientation"][rows][n:], atol=1e-5)
    o = ff.MeshFramesOracle(faces)
    o.set_mesh_by_verts(GOLD["verts"])
    assert np.abs(quat[:n] - o.face_orien_quat[:n]).max() < 5e-6
    # the branch the device took, recovered from the matrix it saved, is the host build's on every regular face
    host_mat = bc.host_frames_forward(GOLD["verts"], faces)[1]
    assert np.array_equal(tw.quat_branch(torch.from_numpy(mat))[0].numpy()[:n], bc.host_quat_branch(host_mat)[:n])
    for k in (1, 255, 256, 257):                                           # rows do not depend on the row count: bitwise
        part = _device_frames(GOLD["verts"], faces, k)
        for a, b in zip(part, (center, mat, quat, scl)):
            assert np.array_equal(a, b[:k]), k
    for a in _device_frames(GOLD["verts"], faces, 0, rows=2):              # nothing to do: OK, and nothing written
        assert np.isnan(a).all()


@pytest.mark.gpu
def test_hip_small_render_inputs_match_the_fixture():
    import test_render_inputs as tri
    R, n = tri.GOLD, N_SMALL
    whole = _device_render(n, 3)
    for k in tri.KEYS:
        assert tri._close(whole[k][:n], R[k][:n], tri.TOL[k]), k
    for n_g, n_x in ((1, 0), (253, 3), (254, 3), (0, 3)):                  # 1, 256, 257 rows, and `extra` rows alone
        part = _device_render(n_g, n_x, rows=n_g + n_x + 2)
        for k, e in (("means3D", "xyz"), ("opacities", "opacity"), ("scales", "scales"), ("rotations", "rotations")):
            assert np.array_equal(part[k][:n_g], whole[k][:n_g]), (k, n_g)
            assert np.array_equal(part[k][n_g:n_g + n_x], R["extra_" + e][:n_x].reshape(n_x, part[k].shape[1])), (k, n_g)      # bitwise copies
            assert np.isnan(part[k][n_g + n_x:]).all(), (k, n_g)
        assert (part["means2D"][:n_g + n_x] == 0).all() and np.isnan(part["means2D"][n_g + n_x:]).all()
    for a in _device_render(0, 0, rows=2).values():                       # nothing to do: OK, and nothing written
        assert np.isnan(a).all()


@pytest.mark.gpu
def test_hip_frames_from_simulated_vertices():
    """The intended use: frames of the cloth faces straight from the solver's particle_x (no host copy), sized like the
    reference's garments (~80k faces); size-independent properties: orthonormal right-handed frames, centres inside
    the triangles' bounding boxes, quaternion <-> matrix round trip."""
    import torch
    from mpmavatar_amd import harness, scenes
    from mpmavatar_amd.mesh_frames import MeshFrames
    sc = scenes.garment_cylinder(aniso=True)
    sim = harness.build_solver(sc, "cuda:0", mode="fast")
    harness.run(sim, 20, fused=True)
    verts = sim.state.particle_x[sc.n_elements + sc.n_traditional:].contiguous()
    fr = MeshFrames(torch.as_tensor(sc.faces, device=verts.device))
    fr.set_mesh_by_verts(verts)
    R = fr.face_orien_mat.double()
    eye = torch.eye(3, dtype=torch.float64, device=R.device)
    assert (R.transpose(1, 2) @ R - eye).abs().max() < 1e-5 and (torch.linalg.det(R) - 1).abs().max() < 1e-5
    tri = verts[torch.as_tensor(sc.faces, device=verts.device).long()]
    assert (fr.face_center <= tri.max(1).values + 1e-6).all() and (fr.face_center >= tri.min(1).values - 1e-6).all()
    q = fr.face_orien_quat.cpu().numpy()[:, [1, 2, 3, 0]]
    assert np.abs(Rot.from_quat(q).as_matrix() - R.cpu().numpy()).max() < 1e-5
    assert fr.face_scaling.min() > 0
