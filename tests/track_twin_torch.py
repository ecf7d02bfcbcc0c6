"""The mesh tracking step (preprocess/train_mesh_lbs_actorshq.py:209-279) restated in torch with the dtype as a parameter, so that
autograd gives the gradients mpmavatar_amd/csrc/track_math.hpp must reproduce: the barycentres, face normals, areas, frame matrices
and vertex normals of utils/geo_utils.py, the loss terms area, scale and opacity (:242, :254, :263-268) and collision_penalty
(preprocess/losses/physics.py).  Pinned against the reference's own functions by tests/golden/track.npz (tests/test_track_host.py).

``matrix_to_quaternion`` is this project's restatement of pytorch3d.transforms.matrix_to_quaternion and is UNCONFIRMED against
pytorch3d itself (not installed where the fixtures are made): the fixture pins the matrices that go into it, nothing pins what
comes out but the properties test_track_host.py checks (R(q) = the matrix, |q| = 1, w >= 0).

torch's own rules are the ones the kernels state: abs has sign(0) = 0, max(dim) and argmax return the first of equal maxima on
the CPU, and torch.maximum splits the slope in halves where its arguments are equal.

Test infrastructure only; nothing under mpmavatar_amd/ imports it."""
import math

import torch


def corners(verts, faces):
    return verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]


def barycenters(verts, faces):
    v1, v2, v3 = corners(verts, faces)
    return (v1 + v2 + v3) / 3


def face_normals(verts, faces):
    v1, v2, v3 = corners(verts, faces)
    n = torch.linalg.cross(v2 - v1, v3 - v2)
    return n / n.norm(dim=1, keepdim=True)


def face_areas(verts, faces):
    v1, v2, v3 = corners(verts, faces)
    return torch.linalg.cross(v2 - v1, v3 - v2).norm(dim=1) / 2


def edge_lengths(verts, faces):
    """-> [F, 3]: |e1|, |e2|, |e3|, on which the longest edge is chosen"""
    v1, v2, v3 = corners(verts, faces)
    return torch.stack([(v2 - v1).norm(dim=1), (v3 - v2).norm(dim=1), (v1 - v3).norm(dim=1)], 1)


def frame_matrices(verts, faces):
    """-> [F, 3, 3] with columns x (the first of the longest edges), y = z x x, z = the normal normalised once more"""
    v1, v2, v3 = corners(verts, faces)
    e = torch.stack([v2 - v1, v3 - v2, v1 - v3], 1)
    idx = edge_lengths(verts, faces).max(dim=1).indices
    x = e[torch.arange(e.shape[0]), idx]
    x = x / x.norm(dim=1, keepdim=True)
    n = face_normals(verts, faces)
    z = n / n.norm(dim=1, keepdim=True)
    y = torch.linalg.cross(z, x)
    y = y / y.norm(dim=1, keepdim=True)
    return torch.stack([x, y, z], 2)


def quaternion_roots(m):
    """-> [F, 4]: sqrt(max(0, 1 +- m00 +- m11 +- m22)), zero slope where clamped"""
    m00, m11, m22 = m[:, 0, 0], m[:, 1, 1], m[:, 2, 2]
    arg = torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], 1)
    root = torch.zeros_like(arg)
    pos = arg > 0
    root[pos] = torch.sqrt(arg[pos])
    return root


def matrix_to_quaternion(m):
    """[F, 3, 3] -> [F, 4] WXYZ with w >= 0.  UNCONFIRMED against pytorch3d (module docstring)."""
    r = quaternion_roots(m)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m.reshape(-1, 9).unbind(1)
    rows = torch.stack([torch.stack([r[:, 0] ** 2, m21 - m12, m02 - m20, m10 - m01], 1),
                        torch.stack([m21 - m12, r[:, 1] ** 2, m10 + m01, m02 + m20], 1),
                        torch.stack([m02 - m20, m10 + m01, r[:, 2] ** 2, m12 + m21], 1),
                        torch.stack([m10 - m01, m20 + m02, m21 + m12, r[:, 3] ** 2], 1)], 1)
    cand = rows / (2.0 * r[:, :, None].clamp(min=0.1))
    q = cand[torch.arange(m.shape[0]), r.argmax(dim=1)]
    return torch.where(q[:, :1] < 0, -q, q)


def quaternion_to_matrix(q):
    """WXYZ unit quaternions -> [F, 3, 3], the textbook formula (for the property R(q) = the frame matrix)"""
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def render_vars(verts, faces, log_scales, logit_opacities):
    """-> (means3D [F, 3], rotations [F, 4], scales [F, 3], opacities [F, 1])"""
    return (barycenters(verts, faces), matrix_to_quaternion(frame_matrices(verts, faces)), torch.exp(log_scales),
            torch.sigmoid(logit_opacities))


def area_gap(verts, faces, log_scales):
    """face_area - pi s0 s1, inside the absolute value of the area term"""
    s = torch.exp(log_scales)
    return face_areas(verts, faces) - s[:, 0] * s[:, 1] * math.pi


def terms(verts, faces, log_scales, logit_opacities):
    """-> [area, scale, opacity]"""
    return torch.stack([area_gap(verts, faces, log_scales).abs().mean(), torch.exp(log_scales)[:, -1].mean(),
                        (1 - torch.sigmoid(logit_opacities)).mean()])


def vertex_normals(verts, faces):
    t = verts[faces]
    n = torch.linalg.cross(t[:, 0] - t[:, 1], t[:, 2] - t[:, 1])
    out = torch.zeros_like(verts)
    for i in range(3):
        out = out.index_add(0, faces[:, i], n)
    return out / out.norm(dim=1, keepdim=True)


def squared_distances(a, b):
    """[n, m], the direct form |a - b|^2 (the reference's PairwiseDistance expands it)"""
    return ((a[:, None] - b[None]) ** 2).sum(-1)


def nearest(a, b):
    return squared_distances(a, b).argmin(dim=1)


def collision(va, vb, nb, eps, mode, index=None):
    """mode: "distance" -> [n], "average" or "cubed" -> 0-dim"""
    j = nearest(va.detach(), vb) if index is None else index
    d = (-nb[j] * (va - vb[j])).sum(-1)
    if mode == "distance":
        return d
    pen = torch.maximum(eps - d, torch.zeros((), dtype=va.dtype))
    return pen.sum() / va.shape[0] if mode == "average" else (pen ** 3).sum()
