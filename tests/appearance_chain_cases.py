"""Cases, the composite float64 / float32 twin and the constants shared by tests/test_appearance_chain_host.py and
tests/test_gpu_appearance_chain.py: the whole appearance step, loss to leaves.  Test infrastructure only.

The twin is a composition of the four pinned ones, nothing new:

    binding_twin_torch.render_inputs(verts + offset, ...)              means3D, rotations (WXYZ), scales, opacities of the bound rows
    shade_twin_torch.shaded(deg, dc, rest, means3D, campos, map, uv)   colours of the bound rows, from THAT means3D
    torch.cat([bound, extra])                                          bound rows first (render_inputs.py, frames.hip:k_render_inputs)
    raster_twin_torch.render(cam, BG, <values>, leaves={...})          the tensors above stay in the graph; discrete part held fixed
    picture = image | (image * alpha).clip(0, 1)
    p = where(keep, picture, gt);  loss = (1 - LAMBDA) mean |p - gt| + LAMBDA (1 - twin_ssim(p, gt))

  case    image     set-up                                                                                      picture
  far     33 x 40   sphere centre on the axis at depth 2.2; 20 extra primitives; shaded colours, degree 3, 6 x 5 map   image
  close   33 x 40   the same at depth 0.9 and 0.4 off the axis: 40 Gaussians culled, 403 rows with a zero gradient     (image * alpha).clip(0, 1)
  sh      17 x 33   depth 1.6, no extras, override_color=None: the rasteriser's own SH path at degree 2                image

All three use binding_grad_cases.case("main") (162 vertices, 320 faces, 657 Gaussians bound unsorted, 300 on one face, five empty
faces, all four quaternion branches), raster_twin.simple_camera and raster_scenes.BG.  33 x 40 is 3 x 3 tiles, ragged both ways, for
the rasteriser and for the loss; 17 x 33 is one ragged row of tiles under a full one.

A pixel is LEFT OUT (keep = False) when one of its decisions is close to a threshold in either twin: the rasteriser twins' ``near``;
some channel with 0 < |p - gt| < image_loss_cases.MIN_DIFF (the sign of the L1 term); and, where the picture is clipped,
0 < p < 1e-4 or |p - 1| < 1e-4 (exact zeros are the background, where alpha is 0: not near).  Left-out pixels are replaced by the
target on both sides before the loss, so they contribute neither a value nor a gradient.  The target is one float32 array: the float32
twin's picture plus N(0, 0.1) noise, clipped to [0, 1].
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import binding_grad_cases as bc
import binding_twin_torch as btw
import image_loss_cases as ic
import raster_scenes as rs
import raster_twin as tw
import raster_twin_torch as tt
import shade_twin_torch as stw

CASES = ("far", "close", "sh")
BOUND_LEAVES = ("verts", "_xyz", "_rotation", "_scaling", "_opacity", "_features_dc", "_features_rest")
EXTRA = ("extra_xyz", "extra_colors", "extra_opacity", "extra_scales", "extra_rotations")     # the order of render_inputs' ``extra``
PER_GAUSSIAN = ("_xyz", "_rotation", "_scaling", "_opacity", "_features_dc", "_features_rest")
LAMBDA = ic.LAMBDA
CLIP_MARGIN = 1e-4
CLAMP_MARGIN = 1e-4        # the rasteriser's frustum and SH clamps, the shading's SH clamp (tests/raster_grad_scenes.py, shade_cases.py)
N_EXTRA = 20
MAP_H, MAP_W = 6, 5
K = 16                     # SH coefficients per Gaussian

#          image (h, w)  centre of the sphere (x, depth)  extras  degree  shaded  clipped  seed
_SETUP = {"far": ((33, 40), (0.0, 2.2), True, 3, True, False, 101),
          "close": ((33, 40), (0.4, 0.9), True, 3, True, True, 112),
          "sh": ((17, 33), (0.0, 1.6), False, 2, False, False, 103)}
# `close` off the axis and its seed: seen from 0.9 a pixel looks through a stack of large, soft Gaussians, T passes 1e-4 in small
# steps, and with the sphere centred 12 .. 16 of the 1,320 pixels have a decision near a threshold (cap: 13).  Off the axis part of
# the sphere leaves the frustum (the culled rows); of the seeds 102, 112, 122, 132 (5 .. 13 pixels) the one with the widest margin.

# Measured on the CPU (tests/test_appearance_chain_host.py::test_e2e32_is_the_measurement asserts both, from above and from below at
# half): E2E32 = the worst, over the three cases and every leaf, of max |g32 - g64| / max |g64| of the composite TWIN, its float32
# run against its float64 run; V32 = the worst relative difference of the two runs' loss values.  The code under test plays no part
# in either.  The device must lie within BOUND_G = 10 * E2E32 (gradients, and the picture on kept pixels) and BOUND_V = 10 *
# max(V32, 2^-24) (the loss comes back as one fp32 number) of the float64 twin -- the project's margin for a different exp, FMA
# contraction, the device's division and another summation order (tests/raster_grad_scenes.py).
# Both float32 runs go through torch's float32 conv2d (the SSIM window), whose summation order may differ from one CPU to another, and
# V32 is the rounding of ONE fp32 number (4.4 ulps of the loss): hence a tenth of headroom on E2E32 and one ulp either way on V32.
E2E32 = 6.0e-6   # measured 5.418e-6 (means2D of `close`); the other 35 figures 2.8e-7 .. 5.3e-6
V32 = 5.5e-7     # measured 4.171e-7 (`far`: 4.4 ulps of 0.156; one ulp is 0.95e-7); `close` 3.0e-8, `sh` 4.0e-8
BOUND_G = 10 * E2E32
BOUND_V = 10 * max(V32, 2.0 ** -24)
MAX_LEFT_OUT_SHARE = rs.MAX_LEFT_OUT_SHARE     # a condition, not a measurement


def leaf_names(name):
    """the leaves of a case, in a fixed order; ``means2D`` (the additive NDC leaf in the published convention) comes last"""
    _, _, extras, _, shaded, _, _ = _SETUP[name]
    return BOUND_LEAVES + (("shadow_map",) if shaded else ()) + (EXTRA if extras else ()) + ("means2D",)


@functools.lru_cache(maxsize=None)
def case(name):
    """SimpleNamespace of read-only arrays and settings: the binding case's tensors, offset, _features_dc / _features_rest, shadow_map,
    face_uv, the five extra_* arrays (m = 0 rows without extras), cam, degree, shaded, clipped"""
    (h, w), (x, depth), extras, degree, shaded, clipped, seed = _SETUP[name]
    b = bc.case("main")
    rng = np.random.default_rng(seed)
    n, n_f = b["binding"].shape[0], b["faces"].shape[0]
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    centre = np.asarray(b["verts"], np.float64).mean(0)
    a = {k: b[k] for k in ("verts", "faces", "binding", "_xyz", "_rotation", "_scaling", "_opacity")}
    a["offset"] = f32(np.array([x, 0.0, depth]) - np.round(centre, 3))            # the sphere's centre in view space
    a["_features_dc"] = f32(rng.normal(0, 0.5, (n, 1, 3)))
    a["_features_rest"] = f32(rng.normal(0, 0.3, (n, K - 1, 3)))
    a["shadow_map"] = f32(rng.uniform(0.2, 1.0, (MAP_H, MAP_W)))
    a["face_uv"] = f32(rng.uniform(-1.05, 1.05, (n_f, 2)))
    # Twenty loose primitives behind the bound rows, as run_demo.py adds them: large and nearly opaque (never at the 0.99 clamp),
    # INSIDE the sphere.  The near half of the sphere is seen in front of them; a pixel that reaches them finishes within a few big
    # steps of T, and the far half of the sphere is hidden.
    m = N_EXTRA if extras else 0
    ang, rad = rng.uniform(0, 2 * np.pi, m), rng.uniform(0.0, 0.3, m)
    a["extra_xyz"] = f32(np.stack([x + rad * np.cos(ang), rad * np.sin(ang), depth + rng.uniform(-0.1, 0.1, m)], 1))
    a["extra_colors"] = f32(rng.uniform(0.05, 0.95, (m, 3)))
    a["extra_opacity"] = f32(rng.uniform(0.9, 0.97, (m, 1)))
    a["extra_scales"] = f32(np.exp(rng.uniform(np.log(0.1), np.log(0.3), (m, 3))))
    a["extra_rotations"] = f32(rng.normal(size=(m, 4)))
    for v in a.values():
        v.setflags(write=False)
    return SimpleNamespace(name=name, cam=tw.simple_camera(h, w), degree=degree, shaded=shaded, clipped=clipped, extras=extras, n=n, m=m,
                           noise_seed=seed + 1000, **a)


def leaves_of(c, dtype, values=None):
    """{leaf name: tensor of `dtype` requiring grad} from the case's float32 arrays (or from `values`, a dict of arrays)"""
    src = values or {}
    names = [k for k in leaf_names(c.name) if k != "means2D"]
    return {k: torch.tensor(np.asarray(src.get(k, getattr(c, k))), dtype=dtype).requires_grad_(True) for k in names}


def forward(c, t, dtype=torch.float64, drop_shading_share=False, extras_first=False, xyzw=False):
    """leaves `t` -> SimpleNamespace(r = the rasteriser twin's TorchRender, picture [3, H, W] in the graph, args = the rasteriser's
    inputs, quat_margin).  The three switches are the seam mutations of the host test, never used for a yardstick:
    drop_shading_share detaches the means3D the shading sees, extras_first puts the extra rows of the geometry in front of the bound
    rows (the colours stay bound-first), xyzw hands the rotations over as XYZW."""
    npd = np.float64 if dtype == torch.float64 else np.float32
    const = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    faces, binding = torch.from_numpy(np.asarray(c.faces).astype(np.int64)), torch.from_numpy(np.asarray(c.binding).astype(np.int64))
    verts = t["verts"] + const(c.offset)
    out = btw.render_inputs(verts, faces, binding, t["_xyz"], t["_rotation"], t["_scaling"], t["_opacity"])
    with torch.no_grad():
        dm = btw.quat_branch(btw.compute_face_orientation(verts, faces)[0])[1]
        top = torch.sort(dm, dim=1, descending=True).values
        quat_margin = float((top[:, 0] - top[:, 1]).min())
    rows = dict(means3D=out["means3D"], opacities=out["opacities"], scales=out["scales"], rotations=out["rotations"])
    if xyzw:
        rows["rotations"] = btw.quat_wxyz_to_xyzw(rows["rotations"])
    kw, sh_margin = {}, np.inf
    if c.shaded:
        seen = out["means3D"].detach() if drop_shading_share else out["means3D"]
        campos = const(c.cam.campos)
        colour = stw.shaded(c.degree, t["_features_dc"], t["_features_rest"], seen, campos, t["shadow_map"], const(c.face_uv), binding)
        rows["colors_precomp"] = colour
        with torch.no_grad():
            sh_margin = float(stw.sh_colour(c.degree, t["_features_dc"], t["_features_rest"], seen, campos)[1].abs().min())
    else:
        rows["shs"] = torch.cat([t["_features_dc"], t["_features_rest"]], 1)       # get_features
        kw["sh_degree"] = c.degree
    if c.extras:
        tail = dict(means3D=t["extra_xyz"], opacities=t["extra_opacity"], scales=t["extra_scales"], rotations=t["extra_rotations"],
                    colors_precomp=t["extra_colors"])
        swap = lambda k: extras_first and k != "colors_precomp"
        rows = {k: torch.cat([tail[k], v] if swap(k) else [v, tail[k]]) for k, v in rows.items()}
    r = tt.render(c.cam, rs.BG, dtype=npd, leaves=rows, **{k: v.detach().numpy() for k, v in rows.items()}, **kw)
    picture = (r.image * r.alpha).clip(0.0, 1.0) if c.clipped else r.image
    return SimpleNamespace(r=r, picture=picture, args=rows, quat_margin=quat_margin, sh_margin=sh_margin)


def loss_of(picture, gt, keep):
    """the loss of the appearance step on the kept pixels; gt [3, H, W] float32 array, keep [H, W] bool array"""
    g = torch.tensor(np.asarray(gt), dtype=picture.dtype)
    p = torch.where(torch.tensor(np.asarray(keep))[None], picture, g)
    return (1.0 - LAMBDA) * (p - g).abs().mean() + LAMBDA * (1.0 - ic.twin_ssim(p, g))


def gradients(loss, t, r, names):
    """-> {leaf: float64 array}; means2D [n + m, 3] from the NDC leaf in the published convention, column 2 zero"""
    order = [k for k in names if k != "means2D"]
    gs = torch.autograd.grad(loss, [t[k] for k in order] + [r.leaves["ndc"]], allow_unused=True)
    out = {k: (np.zeros(tuple(t[k].shape)) if g is None else g.detach().double().numpy()) for k, g in zip(order, gs)}
    ndc = np.zeros(tuple(r.leaves["ndc"].shape)) if gs[-1] is None else gs[-1].detach().double().numpy()
    out["means2D"] = np.concatenate([ndc, np.zeros((ndc.shape[0], 1))], 1)
    return out


def near_the_loss(picture, gt, clipped):
    """[H, W] bool: some channel of this picture decides the sign of the L1 term, or the clip, by less than the margin"""
    p, g = np.asarray(picture, np.float64), np.asarray(gt, np.float64)
    d = np.abs(p - g)
    near = (d > 0) & (d < ic.MIN_DIFF)
    if clipped:
        near |= ((p > 0) & (p < CLIP_MARGIN)) | (np.abs(p - 1.0) < CLIP_MARGIN)
    return near.any(0)


@functools.lru_cache(maxsize=None)
def twins(name):
    """The two runs of the composite twin of a case, computed once and shared, every array read-only:
    gt [3, H, W] float32, keep [H, W] bool, left_out (share), loss64 / loss32 (float), g64 / g32 {leaf: array}, picture64, radii64 /
    radii32, culled [n + m] bool, hidden [n] bool (bound rows whose gradient row is identically zero in BOTH runs in every
    per-Gaussian leaf and in means2D), max_tile_entries, clamp_margin, sh_margin, quat_margin, n_visible."""
    c = case(name)
    names = leaf_names(name)
    t64, t32 = leaves_of(c, torch.float64), leaves_of(c, torch.float32)
    f64, f32 = forward(c, t64, torch.float64), forward(c, t32, torch.float32)
    p64, p32 = f64.picture.detach().numpy(), f32.picture.detach().numpy()
    rng = np.random.default_rng(c.noise_seed)
    gt = np.clip(p32.astype(np.float64) + rng.normal(0, 0.1, p32.shape), 0.0, 1.0).astype(np.float32)
    near = f64.r.near | f32.r.near | near_the_loss(p64, gt, c.clipped) | near_the_loss(p32, gt, c.clipped)
    keep = ~near
    l64, l32 = loss_of(f64.picture, gt, keep), loss_of(f32.picture, gt, keep)
    g64, g32 = gradients(l64, t64, f64.r, names), gradients(l32, t32, f32.r, names)
    zero_row = np.ones(c.n, bool)
    for g in (g64, g32):
        for k in PER_GAUSSIAN + ("means2D",):
            zero_row &= (g[k][:c.n].reshape(c.n, -1) == 0).all(1)
    out = SimpleNamespace(case=c, names=names, gt=gt, keep=keep, left_out=float(near.mean()), loss64=float(l64.detach()), loss32=float(l32.detach()),
                          g64=g64, g32=g32, picture64=p64, radii64=f64.r.base.radii, radii32=f32.r.base.radii,
                          culled=f64.r.base.radii == 0, hidden=zero_row, max_tile_entries=f64.r.base.max_tile_entries,
                          clamp_margin=min(f64.r.clamp_margin, f32.r.clamp_margin), sh_margin=min(f64.sh_margin, f32.sh_margin),
                          quat_margin=min(f64.quat_margin, f32.quat_margin), n_visible=int((f64.r.base.radii > 0).sum()))
    for v in list(vars(out).values()) + list(g64.values()) + list(g32.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def rel(g, g64):
    """max |g - g64| / max |g64| over EVERY element; a tensor that is all zero in float64 must be all zero"""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    assert g.shape == g64.shape, (g.shape, g64.shape)
    if g64.size == 0:
        return 0.0
    top = np.abs(g64).max()
    if top == 0.0:
        assert (g == 0).all()
        return 0.0
    return float(np.abs(g - g64).max() / top)
