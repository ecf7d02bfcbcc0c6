"""A torch twin of re-posing (mpmavatar_amd/reposing.py), written from the formulas and run in float64 (the yardstick) or float32 (the
measurement of S32).  Test infrastructure only.  tests/test_repose_host.py pins it against the reference's own SmplxDeformer methods
(tests/golden/repose.npz); the k-nearest search under them is pinned by nothing but this file, because pytorch3d is not installed
where the fixture is made: brute force, the direct-form squared distance, a stable sort, so the lowest index on ties."""
import torch


def squared_distances(a, b):
    """a [N, D], b [M, D] -> [N, M], sum_d (a_d - b_d)^2 accumulated in ascending d"""
    s = torch.zeros(a.shape[0], b.shape[0], dtype=a.dtype)
    for d in range(a.shape[1]):
        e = a[:, None, d] - b[None, :, d]
        s = s + e * e
    return s


def knn(a, b, k):
    """-> (dists [N, k] ascending, idx int64 [N, k]); equal distances in ascending index order"""
    d2, order = torch.sort(squared_distances(a, b), dim=1, stable=True)
    return d2[:, :k], order[:, :k]


def knn_self(p, k):
    d2, idx = knn(p, p, k + 1)
    return d2[:, 1:], idx[:, 1:]


def six(x, normals, normal_weight):
    """the points find_k_closest_verts searches: (x, normal_weight * n)"""
    return torch.cat([x, normal_weight * normals], dim=-1)


def shepard(d2, power):
    """[..., k] squared distances -> weights [..., k]"""
    w = torch.clamp(d2, min=1e-8) ** (-power)
    return w / w.sum(-1, keepdim=True)


def shepard_lbs(d2, idx, lbs, power=2):
    """d2, idx [P, k], lbs [V, J] -> W [P, J]"""
    return (shepard(d2, power)[:, :, None] * lbs[idx]).sum(1)


def blend(W, A):
    """W [B or 1, P, J], A [B, J, 4, 4] -> T [B, P, 4, 4]"""
    B = A.shape[0]
    return torch.einsum("bpj,bjrc->bprc", W.expand(B, -1, -1), A)


def _scale(scale):
    return scale.reshape(-1, 1, 1) if scale.dim() else scale


def to_pose(v, W, A, transl=None, scale=None):
    """v [B or 1, P, 3] -> (pnts [B, P, 3], T [B, P, 4, 4])"""
    T = blend(W, A)
    out = torch.einsum("bprc,bpc->bpr", T[:, :, :3, :3], v.expand(A.shape[0], -1, -1)) + T[:, :, :3, 3]
    if transl is not None:
        out = out + transl[:, None, :]
    if scale is not None:
        out = out * _scale(scale)
    return out, T


def to_tpose(v, W, A, transl, scale):
    """-> (pnts [B, P, 3], the inverse transforms [B, P, 4, 4])"""
    Ti = torch.linalg.inv(blend(W, A))
    u = v.expand(A.shape[0], -1, -1) / _scale(scale) - transl[:, None, :]
    return torch.einsum("bprc,bpc->bpr", Ti[:, :, :3, :3], u) + Ti[:, :, :3, 3], Ti
