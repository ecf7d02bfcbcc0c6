"""TEST INFRASTRUCTURE ONLY -- a dtype-generic torch restatement of the mesh binding of the reference, differentiable by torch's own
autograd: the yardstick of the binding gradients (tests/test_binding_grad_host.py, tests/test_gpu_binding_grad.py) and the comparison
path of tools/binding_bench.py.  Restates, operation by operation,

  * dot / length / safe_normalize / compute_face_orientation(return_scale=True)       utils/graphics_utils.py:79-107
  * MeshGaussianModel.set_mesh_by_verts (face_center, face_orien_mat, face_scaling, face_orien_quat)
                                                                                        scene/mesh_gaussian_model.py:122-146
  * GaussianModel.get_xyz / get_rotation / get_scaling / get_opacity with a binding    scene/gaussian_model.py:112-160
  * roma's rotmat_to_unitquat, quat_product, quat_xyzw_to_wxyz, quat_wxyz_to_xyzw

PINNING: the fp32 forward against tests/golden/frames.npz and render_inputs.npz (the reference's own code), rotmat_to_unitquat against
oracle/face_frames.py and SciPy, the float64 gradients against tests/golden/binding_grad.npz (the reference's own code under autograd,
with roma's helpers taken from HERE).  roma itself is not installed: its rotmat_to_unitquat is taken to be SciPy's
Rotation.from_matrix selection (the largest of R00, R11, R22, trace picks the branch, first maximum wins) followed by a plain
normalisation, and its backward to be plain autograd through the branch-indexed expressions.  PARITY UNPINNED with roma in that respect.
"""
import torch


def dot(x, y):
    return torch.sum(x * y, -1, keepdim=True)


def length(x, eps=1e-20):
    return torch.sqrt(torch.clamp(dot(x, x), min=eps))


def safe_normalize(x, eps=1e-20):
    return x / length(x, eps)


def compute_face_orientation(verts, faces):
    """-> (orientation [n_f, 3, 3] with columns a0 a1 a2, scale [n_f, 1])"""
    i0, i1, i2 = faces[..., 0].long(), faces[..., 1].long(), faces[..., 2].long()
    v0, v1, v2 = verts[..., i0, :], verts[..., i1, :], verts[..., i2, :]
    a0 = safe_normalize(v1 - v0)
    a1 = safe_normalize(torch.cross(a0, v2 - v0, dim=-1))
    a2 = -safe_normalize(torch.cross(a1, a0, dim=-1))
    orientation = torch.cat([a0[..., None], a1[..., None], a2[..., None]], dim=-1)
    s0 = length(v1 - v0)
    s1 = dot(a2, (v2 - v0)).abs()
    return orientation, (s0 + s1) / 2


def quat_branch(R):
    """(choice [n] in 0..3, decision values [n, 4] = R00, R11, R22, trace): the first maximum wins"""
    diag = torch.diagonal(R, dim1=-2, dim2=-1)
    dm = torch.cat([diag, diag.sum(-1, keepdim=True)], -1)
    return dm.argmax(-1), dm


def rotmat_to_unitquat(R):
    """[n, 3, 3] -> [n, 4] XYZW, no sign canonicalisation.  Differentiable: all four branch expressions are formed and the chosen one
    is gathered, so the gradient flows through the chosen branch alone, then through the normalisation."""
    choice, dm = quat_branch(R)
    tr = dm[:, 3]
    cands = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        q = [None] * 4
        q[i] = 1 - tr + 2 * R[:, i, i]
        q[j] = R[:, j, i] + R[:, i, j]
        q[k] = R[:, k, i] + R[:, i, k]
        q[3] = R[:, k, j] - R[:, j, k]
        cands.append(torch.stack(q, -1))
    cands.append(torch.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1], 1 + tr], -1))
    q = torch.stack(cands, 1).gather(1, choice[:, None, None].expand(-1, 1, 4)).squeeze(1)
    return q / torch.norm(q, dim=-1, keepdim=True)


def quat_product(p, q):
    """Hamilton product, XYZW"""
    px, py, pz, pw = p.unbind(-1)
    qx, qy, qz, qw = q.unbind(-1)
    return torch.stack([pw * qx + px * qw + py * qz - pz * qy, pw * qy - px * qz + py * qw + pz * qx,
                        pw * qz + px * qy - py * qx + pz * qw, pw * qw - px * qx - py * qy - pz * qz], -1)


def quat_xyzw_to_wxyz(q):
    return torch.cat([q[..., 3:], q[..., :3]], -1)


def quat_wxyz_to_xyzw(q):
    return torch.cat([q[..., 1:], q[..., :1]], -1)


def face_frames(verts, faces):
    """set_mesh_by_verts -> (face_center [n_f, 3], face_orien_mat [n_f, 3, 3], face_orien_quat [n_f, 4] WXYZ, face_scaling [n_f, 1])"""
    center = verts[faces.long()].mean(dim=-2)
    mat, scale = compute_face_orientation(verts, faces)
    return center, mat, quat_xyzw_to_wxyz(rotmat_to_unitquat(mat)), scale


def get_xyz(binding, xyz, center, mat, scale):
    b = binding.long()
    return torch.bmm(mat[b], xyz[..., None]).squeeze(-1) * scale[b] + center[b]


def get_rotation(binding, rotation, quat):
    rot = torch.nn.functional.normalize(rotation)
    fq = torch.nn.functional.normalize(quat[binding.long()])
    return quat_xyzw_to_wxyz(quat_product(quat_wxyz_to_xyzw(fq), quat_wxyz_to_xyzw(rot)))


def get_scaling(binding, scaling, scale):
    return torch.exp(scaling) * scale[binding.long()]


def render_inputs(verts, faces, binding, xyz, rotation, scaling, opacity):
    """-> dict means3D, rotations, scales, opacities of the bound Gaussians"""
    center, mat, quat, scale = face_frames(verts, faces)
    return {"means3D": get_xyz(binding, xyz, center, mat, scale), "rotations": get_rotation(binding, rotation, quat),
            "scales": get_scaling(binding, scaling, scale), "opacities": torch.sigmoid(opacity)}
