"""The two further terms of the 4D-DRESS tracking script (preprocess/train_mesh_lbs_4ddress.py) restated in torch with the dtype as a
parameter, so that autograd gives the gradients mpmavatar_amd/csrc/track4d_math.hpp must reproduce.

``scale_ratio_loss`` (:279-292) is pinned against the reference's own function by tests/golden/track4d.npz (tests/test_track4d_host.py).

``laplacian`` evaluates the reference's literal expression of :363, ``L.mm(vertices).norm(dim=1).mean()``, on the matrix L of the
uniform Laplacian: L[i, j] = 1 / deg(i) for every undirected edge {i, j} of the faces (each once, however many faces share it),
L[i, i] = -1.  That matrix restates pytorch3d's ``Meshes.laplacian_packed()`` and is UNCONFIRMED against pytorch3d itself, which is
not installed where the fixtures are made: nothing pins it but this definition.  L is dense up to DENSE_MAX vertices, as the
reference's; above, the same matrix is a sparse COO tensor under the same ``.mm`` (a dense float64 [33306, 33306] is 8.9 GB).

torch's rules are the ones the kernels state: max(dim) and min(dim) return the first of equal extrema on the CPU, clamp(min=th) has
slope 1 at x == th, and norm has gradient 0 at 0.

Test infrastructure only; nothing under mpmavatar_amd/ imports it."""
import torch

DENSE_MAX = 4096


def adjacency(faces, n_verts):
    """-> (row, col) int64: the undirected edges of `faces` in both directions, each once, sorted by row and ascending within it"""
    f = faces.long()
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = torch.unique(torch.cat([e[:, 0] * n_verts + e[:, 1], e[:, 1] * n_verts + e[:, 0]]))
    row = torch.div(key, n_verts, rounding_mode="floor")
    return row, key - row * n_verts


def laplacian_matrix(faces, n_verts, dtype):
    row, col = adjacency(faces, n_verts)
    deg = torch.bincount(row, minlength=n_verts).to(dtype)
    diag = torch.arange(n_verts)
    idx = torch.stack([torch.cat([row, diag]), torch.cat([col, diag])])
    val = torch.cat([1 / deg[row], -torch.ones(n_verts, dtype=dtype)])
    m = torch.sparse_coo_tensor(idx, val, (n_verts, n_verts)).coalesce()
    return m.to_dense() if n_verts <= DENSE_MAX else m


def apply(matrix, verts):
    return matrix.mm(verts)


def laplacian(matrix, verts):
    return matrix.mm(verts).norm(dim=1).mean()


def face_quantities(verts, faces, scale):
    """-> (r, q, longest edge length), each [F]"""
    vert_faces = verts[faces]
    m = (vert_faces - vert_faces[:, [1, 2, 0]]).norm(dim=2).max(dim=1)[0]
    a, b = scale[:, :2].max(dim=1)[0], scale[:, :2].min(dim=1)[0]
    return a / (b + 1e-8), a / (m + 1e-8), m


def scale_ratio_loss(verts, faces, scale, scale_ratio_th=5.0, scale_edge_ratio_th=1.0):
    r, q, _ = face_quantities(verts, faces, scale)
    return (r.clamp(min=scale_ratio_th) - scale_ratio_th).mean(), (q.clamp(min=scale_edge_ratio_th) - scale_edge_ratio_th).mean(), q.var()
