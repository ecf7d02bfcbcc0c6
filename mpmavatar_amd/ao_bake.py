"""The ambient-occlusion bake on the GPU: what the reference's evaluation and demo loops run as a Blender subprocess per frame
(train_material_params.py:819-822 -> blender/bake.py: uvmesh/NNN.obj -> Cycles AO bake -> aomap/NNN.png).  Here the frame's
vertices stay on the device and the [H, W] AO map comes back as a device tensor: no file, no subprocess, no synchronisation,
the same bits on every run,

    baker = AOBaker.from_uv_obj(uv_path, faces)            # once per mesh: coverage, tables, scratch
    for i, verts in enumerate(frames):
        ao_maps[i] = baker.bake(verts)[None]               # [1, H, W], what the ShadowUNet reads
        baker.write_png(os.path.join(out, "aomap"), i, ao_maps[i, 0])   # only if the file is wanted

over six HIP entry points (``mpmhip_ao_coverage``, ``_scratch_bytes``, ``_texel_frames``, ``_build_grid``, ``_trace``,
``_margin``; csrc/ao.hip, csrc/ao_math.hpp).

What is taken from bake.py and its consumers: the resolution (``--ao_res``, 256), the margin (``ao_res // 256``), the bake type AO,
the black background (``bpy.ops.image.new``), the row order of the PNG, and that the PNG is read back with
``.convert("L") / 255`` into a [1, H, W] float map.  What could NOT be checked: Blender is not available where this was written,
so Cycles' sampling pattern, its ray offset, and the transfer curve it applies when it saves the 8-bit file are unknown.  The
sampling below is therefore this project's definition, not a copy of Cycles': cosine-weighted Hammersley directions about the
flat face normal, rotated per texel by a hashed angle, any-hit against every other face, ``bias < t <= max_distance``.
``write_png`` takes ``encoding="linear" | "srgb"`` and defaults to linear; which one matches a given ShadowUNet's training data is
an open point that the caller has to settle.

Occluders that are not in the UV mesh, smooth normals and gradients through the bake are out of scope.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib as L
from . import io_formats
from ._call import call, expect

MAX_SAMPLES = 4096                 # ao::MAX_SAMPLES
MAX_CELLS = 1 << 21                # the grid's cell count is capped at about 2 M


def direction_table(samples):
    """[S, 3] float32: cosine-weighted hemisphere directions about +z.  Hammersley: u = (i + 0.5) / S, phi = 2 pi * (the base-2
    radical inverse of i), r = sqrt(u), z = sqrt(1 - u).  Built in float64, rounded once."""
    i = np.arange(samples, dtype=np.uint64)
    inv = np.zeros(samples, np.float64)
    f, k = 0.5, i.copy()
    while k.any():
        inv += f * (k & np.uint64(1)).astype(np.float64)
        k >>= np.uint64(1)
        f *= 0.5
    u = (i.astype(np.float64) + 0.5) / samples
    phi = 2.0 * np.pi * inv
    r = np.sqrt(u)
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u)], -1).astype(np.float32)


def texel_hash(index):
    """uint32 -> uint32, an integer finaliser (xorshift-multiply, two rounds) of the texel index"""
    x = np.asarray(index, np.uint64) & np.uint64(0xFFFFFFFF)
    m = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def rotation_table(height, width):
    """[H*W, 2] float32: (cos, sin) of the angle 2 pi * hash(texel) / 2^32 by which a texel's tangent is turned about its normal,
    so that neighbouring texels do not share one ray pattern.  Built in float64, rounded once; the device does no trigonometry."""
    ang = 2.0 * np.pi * texel_hash(np.arange(height * width)).astype(np.float64) / 4294967296.0
    return np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32)


def read_uv_template(uv_path):
    """(vt [T, 2] float32, ft [F, 3] int32, 0-based) from the 'vt' and 'f v/vt v/vt v/vt' lines of the UV template, the lines
    io_formats.UVMeshWriter copies and scene/mesh_gaussian_model.py:102-109 reads."""
    vt, ft = [], []
    with open(uv_path, "r") as f:
        for line in f:
            if line[:2] == "vt":
                p = line.strip().split()
                vt.append([float(p[1]), float(p[2])])
            elif line[:2] == "f ":
                p = line.strip().split()
                ft.append([int(p[1].split("/")[1]) - 1, int(p[2].split("/")[1]) - 1, int(p[3].split("/")[1]) - 1])
    return np.asarray(vt, np.float32).reshape(-1, 2), np.asarray(ft, np.int32).reshape(-1, 3)


def encode(ao, encoding="linear"):
    """the value written to the 8-bit file for an AO value in [0, 1]: itself, or the sRGB transfer curve of it"""
    a = np.clip(np.asarray(ao, np.float64), 0.0, 1.0)
    if encoding == "linear":
        return a
    if encoding == "srgb":
        return np.where(a <= 0.0031308, 12.92 * a, 1.055 * np.power(a, 1.0 / 2.4) - 0.055)
    raise RuntimeError(f"encoding must be 'linear' or 'srgb', got {encoding!r}")


class AOBaker:
    """One mesh's baker.  Everything that does not depend on the frame is made here, once: the coverage (which face each texel
    lies in and where), the list of covered texels, the direction and rotation tables and the scratch of the per-frame grid.
    ``bake`` launches kernels on the current stream and returns."""

    def __init__(self, faces, vt, ft, height=256, width=256, samples=256, bias=1e-4, max_distance=10.0, margin=None,
                 max_cells=None, max_entries=None):
        self.faces = expect(faces, torch.int32, "faces", last=3)
        if self.faces.dim() != 2:
            raise RuntimeError("faces: expected an [F, 3] tensor")
        dev = self.faces.device
        n_f = self.n_faces = self.faces.shape[0]
        # the checks below read host copies: nothing is launched before they pass
        vt_h = np.ascontiguousarray(vt.detach().cpu().numpy() if isinstance(vt, torch.Tensor) else np.asarray(vt))
        ft_h = np.ascontiguousarray(ft.detach().cpu().numpy() if isinstance(ft, torch.Tensor) else np.asarray(ft))
        if vt_h.dtype != np.float32 or vt_h.ndim != 2 or vt_h.shape[1] != 2:
            raise RuntimeError("vt: expected a float32 [T, 2] array")
        if ft_h.dtype != np.int32 or ft_h.ndim != 2 or ft_h.shape[1] != 3:
            raise RuntimeError("ft: expected an int32 [F, 3] array")
        if ft_h.shape[0] != n_f:
            raise RuntimeError(f"the UV template has {ft_h.shape[0]} faces, the mesh has {n_f}")
        if not (isinstance(height, int) and isinstance(width, int) and height > 0 and width > 0 and height * width < 2 ** 31 - 1):
            raise RuntimeError("height and width must be positive integers with height * width < 2^31 - 1")
        if not (isinstance(samples, int) and 1 <= samples <= MAX_SAMPLES):
            raise RuntimeError(f"samples must be an integer in [1, {MAX_SAMPLES}]")
        if not (np.isfinite(bias) and np.isfinite(max_distance) and 0.0 <= bias < max_distance):
            raise RuntimeError("expected 0 <= bias < max_distance, both finite")
        if not np.isfinite(vt_h).all():
            raise RuntimeError("vt: non-finite UV coordinates")
        if n_f and (ft_h.min() < 0 or ft_h.max() >= vt_h.shape[0]):
            raise RuntimeError("ft: index outside the vt rows")
        faces_h = self.faces.cpu().numpy()
        if n_f and faces_h.min() < 0:
            raise RuntimeError("faces: negative vertex index")
        self.min_verts = int(faces_h.max()) + 1 if n_f else 0
        self.height, self.width, self.samples = height, width, samples
        self.bias, self.max_distance = float(bias), float(max_distance)
        self.margin = max(height, width) // 256 if margin is None else int(margin)     # bake.py:37
        if self.margin < 0:
            raise RuntimeError("margin must not be negative")
        self.cap_cells = int(max_cells) if max_cells is not None else min(MAX_CELLS, max(512, 8 * n_f))
        self.cap_entries = int(max_entries) if max_entries is not None else 32 * n_f + 2 * self.cap_cells + 1024
        if self.cap_cells < 1 or self.cap_entries < 1:
            raise RuntimeError("max_cells and max_entries must be positive")

        n_t = height * width
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
        self.vt = torch.from_numpy(vt_h).to(dev)
        self.ft = torch.from_numpy(ft_h).to(dev)
        self.dirs = torch.from_numpy(direction_table(samples)).to(dev)
        self.rot = torch.from_numpy(rotation_table(height, width)).to(dev)
        self._face = new((n_t,), torch.int32)
        self._bary = new((n_t, 2), torch.float32)
        call("mpmhip_ao_coverage", dev, self.faces.data_ptr(), self.ft.data_ptr(), n_f, self.vt.data_ptr(), self.vt.shape[0], height,
             width, self._face.data_ptr(), self._bary.data_ptr())
        self._mask = [(self._face >= 0).to(torch.uint8), new((n_t,), torch.uint8), new((n_t,), torch.uint8)]
        self.covered = torch.nonzero(self._mask[0]).view(-1).to(torch.int32)   # the trace's work list (the one synchronisation)
        self.n_covered = self.covered.shape[0]
        nbytes = C.c_int64(0)
        index = dev.index if dev.index is not None else torch.cuda.current_device()
        rc = L.load().mpmhip_ao_scratch_bytes(index, n_f, self.cap_cells, self.cap_entries, C.byref(nbytes))
        if rc != L.OK:
            raise L.MPMHipError(rc, "mpmhip_ao_scratch_bytes failed")
        self._scratch = new((nbytes.value,), torch.uint8)
        self._raw = torch.zeros(n_t, dtype=torch.float32, device=dev)   # uncovered texels stay 0: the black image of bake.py:62
        self._val = [new((n_t,), torch.float32), new((n_t,), torch.float32)] if self.margin > 1 else []

    @classmethod
    def from_uv_obj(cls, uv_path, faces, **kw):
        """The baker of a mesh whose UVs are a template OBJ, parsed as io_formats.UVMeshWriter parses it."""
        vt, ft = read_uv_template(uv_path)
        return cls(faces, vt, ft, **kw)

    @property
    def coverage(self):
        """(face [H, W] int32, -1 = no face; bary [H, W, 2]: the weights of the face's second and third corner)"""
        return self._face.view(self.height, self.width), self._bary.view(self.height, self.width, 2)

    def _verts(self, verts):
        v = expect(verts, torch.float32, "verts", last=3)
        if v.dim() != 2 or v.shape[0] < self.min_verts or v.device != self.faces.device:
            raise RuntimeError(f"verts: expected [n, 3] with n >= {self.min_verts} on {self.faces.device}")
        return v

    def texel_frames(self, verts):
        """(origin, normal, tangent), [H*W, 3] each: where every texel's rays leave from and the frame they are laid out in
        (bitangent = normal x tangent); zeros on uncovered texels."""
        v = self._verts(verts)
        o, n, t = (torch.empty(self.height * self.width, 3, dtype=torch.float32, device=v.device) for _ in range(3))
        call("mpmhip_ao_texel_frames", v.device, v.data_ptr(), self.faces.data_ptr(), self.n_faces, self.height, self.width,
             self._face.data_ptr(), self._bary.data_ptr(), self.rot.data_ptr(), o.data_ptr(), n.data_ptr(), t.data_ptr())
        return o, n, t

    def build_grid(self, verts):
        """stage 1 of bake: triangle records, bounding box and the uniform grid of this frame, into the scratch"""
        v = self._verts(verts)
        call("mpmhip_ao_build_grid", v.device, v.data_ptr(), self.faces.data_ptr(), self.n_faces, self.cap_cells, self.cap_entries,
             self._scratch.data_ptr(), self._scratch.numel())

    def trace(self, verts):
        """stage 2 of bake: AO on the covered texels, from the grid build_grid left in the scratch -> the [H*W] map before the margin
        (the baker's own buffer)"""
        v = self._verts(verts)
        call("mpmhip_ao_trace", v.device, v.data_ptr(), self.faces.data_ptr(), self.n_faces, self._face.data_ptr(), self._bary.data_ptr(),
             self.covered.data_ptr(), self.n_covered, self.rot.data_ptr(), self.dirs.data_ptr(), self.samples, self.bias,
             self.max_distance, self.cap_cells, self.cap_entries, self._scratch.data_ptr(), self._scratch.numel(), self._raw.data_ptr())
        return self._raw

    def add_margin(self, out):
        """stage 3 of bake: the margin pixels around the covered texels, one pass each -> out [H, W]"""
        src_v, src_m = self._raw, self._mask[0]
        for k in range(self.margin):
            dst_v = out if k == self.margin - 1 else self._val[k % 2]
            dst_m = self._mask[1 + k % 2]
            call("mpmhip_ao_margin", out.device, self.height, self.width, src_v.data_ptr(), src_m.data_ptr(), dst_v.data_ptr(), dst_m.data_ptr())
            src_v, src_m = dst_v, dst_m
        if self.margin == 0:
            out.view(-1).copy_(self._raw)
        return out

    def bake(self, verts, out=None):
        """The AO map [H, W] float32 of the mesh at ``verts`` [n, 3]: 1 = open, 0 = fully occluded, 0 where no face lies (outside
        the margin).  Row 0 is the top of the image.  If a frame's grid needs more entries than the scratch holds, every covered
        texel is NaN (raise max_entries)."""
        v = self._verts(verts)
        if out is None:
            out = torch.empty(self.height, self.width, dtype=torch.float32, device=v.device)
        else:
            expect(out, torch.float32, "out", shape=(self.height, self.width))
        self.build_grid(v)
        self.trace(v)
        return self.add_margin(out)

    def write_png(self, directory, frame, ao, encoding="linear"):
        """aomap/NNN.png (bake.py:76-78) with three equal channels, so that ``.convert("L")`` gives the value back."""
        a = ao.detach().cpu().numpy() if isinstance(ao, torch.Tensor) else np.asarray(ao)
        if a.shape != (self.height, self.width):
            raise RuntimeError(f"ao: expected shape {(self.height, self.width)}, got {tuple(a.shape)}")
        e = encode(a, encoding).astype(np.float32)
        return io_formats.write_png(os.path.join(directory, f"{frame:03d}.png"), np.stack([e, e, e]))
