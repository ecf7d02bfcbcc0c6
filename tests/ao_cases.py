"""The meshes, atlases and bake settings that the AO tests share (tests/test_ao_host.py on the CPU, tests/test_gpu_ao_bake.py on the
device), each small enough for brute force on the host, plus the ctypes face of tests/hostao.  Test infrastructure only."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from hostbuild import host_lib
from mpmavatar_amd import garment
from mpmavatar_amd.ao_bake import direction_table, rotation_table

BIAS, MAX_DISTANCE = 1e-4, 10.0


@dataclass
class Case:
    name: str
    verts: np.ndarray      # [n, 3] float32
    faces: np.ndarray      # [F, 3] int32
    vt: np.ndarray         # [T, 2] float32
    ft: np.ndarray         # [F, 3] int32
    height: int = 32
    width: int = 32
    samples: int = 64

    @property
    def cap_cells(self):   # AOBaker's default
        return min(1 << 21, max(512, 8 * len(self.faces)))


def _sheet(n=9, half=0.4):
    v, f = garment.grid_sheet(n, n, -half, half, -half, half, 0.0)
    return v, f


def case_a():
    """open sheet: 8 x 8 quads in the plane y = 0 (normals +y), planar UVs filling [0.1, 0.9]^2"""
    v, f = _sheet()
    vt = np.stack([0.1 + (v[:, 0].astype(np.float64) + 0.4), 0.1 + (v[:, 2].astype(np.float64) + 0.4)], -1).astype(np.float32)
    return Case("A", v, f, vt, f.copy())


def case_b():
    """lid: A under a two-triangle plate at y = 0.05 that is 1000 times wider; the plate's UVs lie outside the map"""
    a = case_a()
    w = 400.0
    plate = np.array([[-w, 0.05, -w], [w, 0.05, -w], [w, 0.05, w], [-w, 0.05, w]], np.float32)
    n, t = len(a.verts), len(a.vt)
    faces = np.concatenate([a.faces, np.array([[n, n + 1, n + 2], [n, n + 2, n + 3]], np.int32)])
    vt = np.concatenate([a.vt, np.array([[2.0, 2.0], [3.0, 2.0], [3.0, 3.0], [2.0, 3.0]], np.float32)])
    ft = np.concatenate([a.ft, np.array([[t, t + 1, t + 2], [t, t + 2, t + 3]], np.int32)])
    return Case("B", np.concatenate([a.verts, plate]), faces, vt, ft)


def per_face_atlas(n_faces):
    """every face its own UV triangle: two faces per cell of a square grid of cells, inset by a tenth of a cell -> (vt, ft)"""
    cells = (n_faces + 1) // 2
    n = int(np.ceil(np.sqrt(cells)))
    w = 1.0 / n
    vt, ft = [], []
    for f in range(n_faces):
        cx, cy = (f // 2) % n * w, (f // 2) // n * w
        if f % 2 == 0:
            tri = [(cx + 0.1 * w, cy + 0.1 * w), (cx + 0.8 * w, cy + 0.1 * w), (cx + 0.1 * w, cy + 0.8 * w)]
        else:
            tri = [(cx + 0.9 * w, cy + 0.9 * w), (cx + 0.2 * w, cy + 0.9 * w), (cx + 0.9 * w, cy + 0.2 * w)]
        ft.append([len(vt), len(vt) + 1, len(vt) + 2])
        vt += tri
    return np.asarray(vt, np.float32), np.asarray(ft, np.int32)


def case_c(seed=0):
    """sphere over a wavy sheet: icosphere(2, 0.3, (0, 0.35, 0)), 320 faces, over a 9 x 9-vertex sheet y = 0.05 sin 4x cos 3z on
    [-0.6, 0.6]^2 with +-0.01 jitter, 128 faces; a per-face atlas, so ft != faces and every edge is a UV seam"""
    rng = np.random.default_rng(seed)
    sv, sf = garment.icosphere(2, 0.3, (0.0, 0.35, 0.0))
    hv, hf = garment.grid_sheet(9, 9, -0.6, 0.6, -0.6, 0.6, 0.0)
    hv = hv.astype(np.float64)
    hv[:, 1] = 0.05 * np.sin(4 * hv[:, 0]) * np.cos(3 * hv[:, 2])
    hv += rng.uniform(-0.01, 0.01, hv.shape)
    verts = np.concatenate([sv, hv.astype(np.float32)])
    faces = np.concatenate([sf, hf + len(sv)]).astype(np.int32)
    vt, ft = per_face_atlas(len(faces))
    return Case(f"C{seed}", verts, faces, vt, ft)


def case_d():
    """degenerates: C plus a face without area (a repeated vertex), a face without UV area, a face whose UV triangle is that of
    face 5 (the lower index must win), and a vertex that no face names"""
    c = case_c(0)
    n, t = len(c.verts), len(c.vt)
    verts = np.concatenate([c.verts, np.array([[0.5, 0.3, 0.5], [0.55, 0.35, 0.5], [0.5, 0.35, 0.55], [3.0, 3.0, 3.0]], np.float32)])
    faces = np.concatenate([c.faces, np.array([[n, n, n + 1], [n, n + 1, n + 2], [n + 2, n + 1, n]], np.int32)])
    vt = np.concatenate([c.vt, np.array([[0.5, 0.5], [0.7, 0.7], [0.9, 0.9]], np.float32)])
    ft = np.concatenate([c.ft, np.array([[t, t + 1, t + 2], [t, t + 1, t + 2], c.ft[5]], np.int32)])
    return Case("D", verts, faces, vt, ft)


def soup(n_faces=200, n_rays=20000, seed=7):
    """a random triangle soup in the unit cube and random rays through it -> (verts, faces, origins, directions)"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0.0, 1.0, (n_faces, 1, 3))
    verts = (centre + rng.uniform(-0.12, 0.12, (n_faces, 3, 3))).reshape(-1, 3).astype(np.float32)
    faces = np.arange(3 * n_faces, dtype=np.int32).reshape(-1, 3)
    o = rng.uniform(-0.3, 1.3, (n_rays, 3)).astype(np.float32)
    d = rng.normal(size=(n_rays, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d[::97, 1] = 0.0      # some rays run inside a plane of cell walls' normals, some along an axis
    d[::389, :2] = 0.0
    d[::389, 2] = 1.0
    return verts, faces, o, d


# ---- tests/hostao through ctypes

_fp, _ip, _bp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def _p(a, t):
    return a.ctypes.data_as(t)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def lib():
    h = host_lib("hostao")
    for name in ("ha_coverage", "ha_frames", "ha_count", "ha_bake", "ha_ray_faces", "ha_margin"):
        getattr(h, name).restype = None
    return h


def tables(case):
    return direction_table(case.samples), rotation_table(case.height, case.width)


def host_coverage(case):
    n_t = case.height * case.width
    face, bary = np.empty(n_t, np.int32), np.empty((n_t, 2), np.float32)
    lib().ha_coverage(len(case.faces), _p(_i32(case.faces), _ip), _p(_i32(case.ft), _ip), _p(_f32(case.vt), _fp), case.height, case.width,
                      _p(face, _ip), _p(bary, _fp))
    return face, bary


def host_frames(case, face, bary, rot, verts=None):
    n_t = case.height * case.width
    o, n, t, b = (np.empty((n_t, 3), np.float32) for _ in range(4))
    v = _f32(case.verts if verts is None else verts)
    lib().ha_frames(_p(v, _fp), _p(_i32(case.faces), _ip), case.height, case.width, _p(_i32(face), _ip), _p(_f32(bary), _fp), _p(_f32(rot), _fp),
                    _p(o, _fp), _p(n, _fp), _p(t, _fp), _p(b, _fp))
    return o, n, t, b


def host_count(case, face, origin, normal, tangent, dirs, brute, verts=None, cap_cells=None):
    """occluded rays per texel from given frames, by the grid walk or by brute force"""
    occ = np.empty(case.height * case.width, np.int32)
    v = _f32(case.verts if verts is None else verts)
    lib().ha_count(len(case.faces), _p(v, _fp), _p(_i32(case.faces), _ip), cap_cells or case.cap_cells, case.height, case.width, _p(_i32(face), _ip),
                   _p(_f32(origin), _fp), _p(_f32(normal), _fp), _p(_f32(tangent), _fp), len(dirs), _p(_f32(dirs), _fp),
                   C.c_float(BIAS), C.c_float(MAX_DISTANCE), int(brute), _p(occ, _ip))
    return occ


def host_bake(case, face, bary, rot, dirs, brute=False, verts=None, cap_cells=None):
    """(ao [H*W] before the margin, occluded [H*W])"""
    n_t = case.height * case.width
    ao, occ = np.empty(n_t, np.float32), np.empty(n_t, np.int32)
    v = _f32(case.verts if verts is None else verts)
    lib().ha_bake(len(case.faces), _p(v, _fp), _p(_i32(case.faces), _ip), cap_cells or case.cap_cells, case.height, case.width, _p(_i32(face), _ip),
                  _p(_f32(bary), _fp), _p(_f32(rot), _fp), len(dirs), _p(_f32(dirs), _fp), C.c_float(BIAS), C.c_float(MAX_DISTANCE), int(brute),
                  _p(ao, _fp), _p(occ, _ip))
    return ao, occ


def host_ray_faces(verts, faces, o, d, brute, cap_cells):
    """(hits [n_rays, F] uint8, (cells per axis x 3, entries))"""
    hits = np.empty((len(o), len(faces)), np.uint8)
    dims = np.zeros(4, np.int64)
    lib().ha_ray_faces(len(faces), _p(_f32(verts), _fp), _p(_i32(faces), _ip), cap_cells, len(o), _p(_f32(o), _fp), _p(_f32(d), _fp), C.c_float(BIAS),
                       C.c_float(MAX_DISTANCE), int(brute), _p(hits, _bp), dims.ctypes.data_as(C.POINTER(C.c_int64)))
    return hits, dims


def host_margin(val, mask, height, width):
    out_v, out_m = np.empty(height * width, np.float32), np.empty(height * width, np.uint8)
    m = np.ascontiguousarray(mask, np.uint8)
    lib().ha_margin(height, width, _p(_f32(val), _fp), _p(m, _bp), _p(out_v, _fp), _p(out_m, _bp))
    return out_v, out_m


def rays_of(origin, normal, tangent, bitangent, dirs, face):
    """every ray of every covered texel -> (o [n, 3], d [n, 3]) in fp32, d formed as ao::ray_dir forms it up to rounding"""
    cov = np.nonzero(face >= 0)[0]
    d = (dirs[None, :, 0:1] * tangent[cov, None, :] + dirs[None, :, 1:2] * bitangent[cov, None, :] + dirs[None, :, 2:3] * normal[cov, None, :])
    o = np.repeat(origin[cov], len(dirs), 0)
    return o.astype(np.float32), d.reshape(-1, 3).astype(np.float32)


CASES = {"A": case_a, "B": case_b, "C0": lambda: case_c(0), "C1": lambda: case_c(1), "C2": lambda: case_c(2), "D": case_d}
_baked = {}


def baked(name):
    """everything the host build makes of a case, computed once and shared by the tests of a session: never modified by a test"""
    if name not in _baked:
        case = CASES[name]()
        dirs, rot = tables(case)
        face, bary = host_coverage(case)
        o, n, t, b = host_frames(case, face, bary, rot)
        ao, occ = host_bake(case, face, bary, rot, dirs)
        _baked[name] = dict(case=case, dirs=dirs, rot=rot, face=face, bary=bary, o=o, n=n, t=t, b=b, ao=ao, occ=occ)
    return _baked[name]
