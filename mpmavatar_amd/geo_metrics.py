"""Geometry metrics on the GPU: the evaluation every run of the reference ends with.  Mirrors
/root/reference/metric.py (all of it) and the geometry loop of eval.py:30-56 over four HIP entry points
(``mpmhip_face_areas``, ``mpmhip_mesh_sample``, ``mpmhip_nn_dist2``, ``mpmhip_geo_reduce``): simulated vertices stay on
the device,

    ev = GeoEval(faces_pred)                                   # faces of the simulated mesh
    for frame in frames:
        ev.add_frame(verts_pred, verts_gt, faces_gt)           # nothing leaves the device, nothing synchronises
    ev.save(output_path)                                       # geo_metric.npz, keys "CD" and "F-Score"

Nearest neighbours are exact brute force (the reference asks SciPy's cKDTree).  Random numbers come from torch, not
from NumPy as in trimesh, so sample sets differ from the reference's draw by draw; the construction is the same.
No CPU fallback: tensors must live on an MI355X.
"""
from __future__ import annotations

import torch

from . import io_formats
from ._call import call, expect, ptr

TAU = 1e-3                 # metric.py:60
REDUCE_SCRATCH = 256       # MPMHIP_GEO_REDUCE_SCRATCH


def _chk(t, dtype, name, last=None):
    return expect(t, dtype, name, last=last, rows=True)


def face_area_cdf(verts, faces):
    """(area [n_f] float32, inclusive cumulative sum [n_f] float64) of the mesh's faces."""
    v, f = _chk(verts, torch.float32, "verts", 3), _chk(faces, torch.int32, "faces", 3)
    area = torch.empty(f.shape[0], dtype=torch.float32, device=v.device)
    call("mpmhip_face_areas", v.device, v.data_ptr(), f.data_ptr(), f.shape[0], area.data_ptr())
    return area, torch.cumsum(area.double(), 0)


def _sample_into(verts, faces, cdf, uniforms, points, face_index):
    call("mpmhip_mesh_sample", verts.device, verts.data_ptr(), faces.data_ptr(), faces.shape[0], cdf.data_ptr(),
         uniforms.data_ptr(), uniforms.shape[0], points.data_ptr(), ptr(face_index))


def sample_surface(verts, faces, count, generator=None):
    """metric.py:4-8 (trimesh's mesh.sample(count, return_index=True)): `count` area-weighted points on the surface and
    the face each lies on.  The uniforms are torch.rand(count, 3) on the device: (face pick, u1, u2) per sample."""
    v = _chk(verts, torch.float32, "verts", 3)
    f = _chk(faces.to(torch.int32).contiguous(), torch.int32, "faces", 3)
    if count <= 0:
        raise RuntimeError("count must be positive")
    _, cdf = face_area_cdf(v, f)
    u = torch.rand(count, 3, generator=generator, dtype=torch.float32, device=v.device)
    points = torch.empty(count, 3, dtype=torch.float32, device=v.device)
    face_index = torch.empty(count, dtype=torch.int32, device=v.device)
    _sample_into(v, f, cdf, u, points, face_index)
    return points, face_index


def _nn_into(src, dst, slices, best, dist2, index):
    call("mpmhip_nn_dist2", src.device, src.data_ptr(), src.shape[0], dst.data_ptr(), dst.shape[0], slices, best.data_ptr(),
         dist2.data_ptr(), ptr(index))


def nearest_dist2(src, dst, return_index=False, slices=0):
    """metric.py:18-21 squared: for every src point the squared distance to (and the index of) its nearest dst point.
    slices = 0 lets the library cut the targets; any other value gives the same bits."""
    s, d = _chk(src, torch.float32, "src", 3), _chk(dst, torch.float32, "dst", 3)
    if s.device != d.device:
        raise RuntimeError("src and dst must be on the same device")
    n = s.shape[0]
    best = torch.empty(n, dtype=torch.int64, device=s.device)
    dist2 = torch.empty(n, dtype=torch.float32, device=s.device)
    index = torch.empty(n, dtype=torch.int32, device=s.device) if return_index else None
    _nn_into(s, d, slices, best, dist2, index)
    return (dist2, index) if return_index else dist2


def _reduce_into(d12, d21, tau, scratch, out):
    call("mpmhip_geo_reduce", d12.device, d12.data_ptr(), d12.shape[0], d21.data_ptr(), d21.shape[0], float(tau),
         scratch.data_ptr(), out.data_ptr())


def reduce_dist2(dist2_12, dist2_21, tau=TAU):
    """(F-score, Chamfer, precision, recall) as four doubles on the device from the two squared-distance arrays."""
    a, b = _chk(dist2_12, torch.float32, "dist2_12"), _chk(dist2_21, torch.float32, "dist2_21")
    scratch = torch.empty(REDUCE_SCRATCH, dtype=torch.float64, device=a.device)
    out = torch.empty(4, dtype=torch.float64, device=a.device)
    _reduce_into(a, b, tau, scratch, out)
    return out


def chamfer_fscore(points1, points2, tau=TAU):
    """metric.fscore + metric.mesh_chamfer_via_points on two point sets (metric.py:23-54, one pair of nearest-neighbour
    passes instead of the reference's two): tensor [F-score, Chamfer, precision, recall], float64, on the device."""
    return reduce_dist2(nearest_dist2(points1, points2), nearest_dist2(points2, points1), tau)


def all_mesh_metrics(verts1, faces1, verts2, faces2, sample_count=100000, generator=None):
    """metric.py:56-63: (fscore at tau = 1e-3, chamfer) of two meshes, as 0-d device tensors."""
    p1, _ = sample_surface(verts1, faces1, sample_count, generator)
    p2, _ = sample_surface(verts2, faces2, sample_count, generator)
    out = chamfer_fscore(p1, p2)
    return out[0], out[1]


def all_mesh_metrics_points(points, verts2, faces2, sample_count=100000, generator=None):
    """metric.py:65-72: a point cloud (sample_count of its points, chosen without replacement) against a mesh."""
    p = _chk(points, torch.float32, "points", 3)
    if sample_count > p.shape[0]:
        raise RuntimeError("cannot choose more points than there are without replacement")
    pick = torch.randperm(p.shape[0], generator=generator, device=p.device)[:sample_count]
    p2, _ = sample_surface(verts2, faces2, sample_count, generator)
    out = chamfer_fscore(p[pick].contiguous(), p2)
    return out[0], out[1]


class GeoEval:
    """The geometry loop of eval.py:30-56 with everything on the device: one row of (F-score, Chamfer, precision, recall)
    per frame.  Every buffer is allocated here, once; add_frame launches kernels and returns."""

    def __init__(self, faces_pred, sample_count=100000, seed=0):
        self.faces_pred = _chk(faces_pred.to(torch.int32).contiguous(), torch.int32, "faces_pred", 3)
        dev = self.faces_pred.device
        n = self.n = int(sample_count)
        if n <= 0:
            raise RuntimeError("sample_count must be positive")
        self.generator = torch.Generator(device=dev)
        self.generator.manual_seed(seed)
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        self._u = new((n, 3), torch.float32)
        self._p = [new((n, 3), torch.float32), new((n, 3), torch.float32)]
        self._d = [new((n,), torch.float32), new((n,), torch.float32)]
        self._best = new((n,), torch.int64)
        self._scratch = new((REDUCE_SCRATCH,), torch.float64)
        self.rows = []

    def _sample(self, verts, faces, points):
        _, cdf = face_area_cdf(verts, faces)
        torch.rand(self._u.shape, generator=self.generator, out=self._u)
        _sample_into(verts, faces, cdf, self._u, points, None)

    def add_frame(self, verts_pred, verts_gt, faces_gt):
        """eval.py:49: all_mesh_metrics(mesh_gt, mesh_pred).  Returns the frame's row (a device tensor of 4 doubles)."""
        vp, vg = _chk(verts_pred, torch.float32, "verts_pred", 3), _chk(verts_gt, torch.float32, "verts_gt", 3)
        fg = _chk(faces_gt.to(torch.int32).contiguous(), torch.int32, "faces_gt", 3)
        self._sample(vg, fg, self._p[0])
        self._sample(vp, self.faces_pred, self._p[1])
        _nn_into(self._p[0], self._p[1], 0, self._best, self._d[0], None)
        _nn_into(self._p[1], self._p[0], 0, self._best, self._d[1], None)
        row = torch.empty(4, dtype=torch.float64, device=vp.device)
        _reduce_into(self._d[0], self._d[1], TAU, self._scratch, row)
        self.rows.append(row)
        return row

    def results(self):
        """{"CD": [...], "F-Score": [...]} per frame, on the host (the one synchronisation)."""
        r = torch.stack(self.rows).cpu().numpy() if self.rows else torch.zeros(0, 4, dtype=torch.float64).numpy()
        return {"CD": r[:, 1].copy(), "F-Score": r[:, 0].copy()}

    def save(self, directory):
        """geo_metric.npz as eval.py:56 writes it."""
        res = self.results()
        return io_formats.write_geo_metric_npz(directory, res["CD"], res["F-Score"])
