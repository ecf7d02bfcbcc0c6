"""The forward twin (tests/raster_twin.py) restated in torch with the dtype as a parameter, so that autograd gives the gradient the
backward pass (mpmavatar_amd/csrc/raster_grad_math.hpp, raster_backward.hip) must reproduce: dense over pixels, looping over the
Gaussians in depth order, every decision a mask.  The discrete part (radii, tile rectangles, order) is taken from the NumPy twin
of the same dtype and held fixed; the clamps differentiate as clamps, zero slope where they bind.  Adds the SH path, the
cov3Ds_precomp path and the additive NDC leaf that defines the gradient of means2D.

Test infrastructure only; nothing under mpmavatar_amd/ imports it."""
from typing import NamedTuple

import numpy as np
import torch

import raster_twin as tw

TILE = tw.TILE
ALPHA_MAX = 0.99


class TorchRender(NamedTuple):
    image: torch.Tensor    # [3, H, W], in the graph
    alpha: torch.Tensor    # [1, H, W], in the graph
    leaves: dict           # name -> leaf tensor (requires_grad); "ndc" [n, 2] is the additive NDC offset of the pixel centre
    near: np.ndarray       # [H, W] bool: the NumPy twin's near, or opacity exp(power) within 1e-4 relative of the 0.99 clamp
    base: object           # the NumPy twin's Render of the same dtype
    clamp_margin: float    # min over visible Gaussians of the relative distance to the frustum clamp and to the SH zero clamp


def _clamp_fixed(v, lo, hi):
    """clamp with zero slope where it binds (torch.clamp passes the gradient through at the bound itself; here a bound is strict)"""
    return torch.where(v > hi, torch.full_like(v, hi), torch.where(v < lo, torch.full_like(v, lo), v))


def sh_colour(deg, sh, means, campos):
    f = lambda v: torch.tensor(v, dtype=sh.dtype)
    d = means - campos
    d = d / torch.sqrt((d * d).sum(1, keepdim=True))
    x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    C1, C2, C3 = f(tw.C1), [f(v) for v in tw.C2], [f(v) for v in tw.C3]
    r = f(tw.C0) * sh[:, 0]
    if deg > 0:
        r = r - C1 * y * sh[:, 1] + C1 * z * sh[:, 2] - C1 * x * sh[:, 3]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        r = (r + C2[0] * xy * sh[:, 4] + C2[1] * yz * sh[:, 5] + C2[2] * (2 * zz - xx - yy) * sh[:, 6] + C2[3] * xz * sh[:, 7]
             + C2[4] * (xx - yy) * sh[:, 8])
    if deg > 2:
        r = (r + C3[0] * y * (3 * xx - yy) * sh[:, 9] + C3[1] * xy * z * sh[:, 10] + C3[2] * y * (4 * zz - xx - yy) * sh[:, 11]
             + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[:, 12] + C3[4] * x * (4 * zz - xx - yy) * sh[:, 13]
             + C3[5] * z * (xx - yy) * sh[:, 14] + C3[6] * x * (xx - 3 * yy) * sh[:, 15])
    raw = r + 0.5
    return torch.where(raw > 0, raw, torch.zeros_like(raw)), raw


def cov3d(scales, rotations, mod):
    q = rotations / torch.sqrt((rotations * rotations).sum(1, keepdim=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], 1),
                     torch.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], 1),
                     torch.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1)], 1)
    M = R * (mod * scales)[:, None, :]
    S = M @ M.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)


def render(cam, bg, means3D, opacities, colors_precomp=None, shs=None, sh_degree=0, scales=None, rotations=None, cov3Ds_precomp=None,
           scale_modifier=1.0, dtype=np.float64, leaves=None):
    """The whole forward pass under autograd.  Arguments are NumPy arrays as for raster_twin.render; leaves = {name: tensor} puts
    the caller's tensors into the graph in place of fresh leaves of the same values (torch.autograd.gradcheck)."""
    td = torch.float64 if dtype == np.float64 else torch.float32
    base = tw.render(cam, bg, means3D, opacities, colors_precomp=colors_precomp, shs=shs, sh_degree=sh_degree, scales=scales,
                     rotations=rotations, cov3Ds_precomp=cov3Ds_precomp, scale_modifier=scale_modifier, dtype=dtype)
    given = leaves or {}
    leaf = lambda a, name: given[name] if name in given else torch.tensor(np.asarray(a), dtype=td).requires_grad_(True)
    const = lambda a: torch.tensor(np.asarray(a), dtype=td)
    L = dict(means3D=leaf(means3D, "means3D"), opacities=leaf(opacities, "opacities"))
    n = L["means3D"].shape[0]
    L["ndc"] = torch.zeros(n, 2, dtype=td, requires_grad=True)
    H, W = cam.image_height, cam.image_width
    V, P, campos = const(cam.viewmatrix), const(cam.projmatrix), const(cam.campos)
    margin = np.inf
    if cov3Ds_precomp is not None:
        L["cov3Ds_precomp"] = leaf(cov3Ds_precomp, "cov3Ds_precomp")
        c6 = L["cov3Ds_precomp"]
    else:
        L["scales"], L["rotations"] = leaf(scales, "scales"), leaf(rotations, "rotations")
        c6 = cov3d(L["scales"], L["rotations"], scale_modifier)
    vis = base.radii > 0
    if shs is not None:
        L["shs"] = leaf(shs, "shs")
        col, raw = sh_colour(sh_degree, L["shs"], L["means3D"], campos)
        if vis.any():
            margin = min(margin, float(raw.detach().abs()[torch.from_numpy(vis)].min()))
    else:
        L["colors_precomp"] = leaf(colors_precomp, "colors_precomp")
        col = L["colors_precomp"]
    m = L["means3D"]
    safe = torch.from_numpy(base.splats.depth > 0.2)           # keep the culled ones out of the divisions
    t = m @ V[:3, :3] + V[3, :3]
    tz = torch.where(safe, t[:, 2], torch.ones_like(t[:, 2]))
    fx, fy = W / (2 * cam.tanfovx), H / (2 * cam.tanfovy)
    limx, limy = 1.3 * cam.tanfovx, 1.3 * cam.tanfovy
    rx, ry = t[:, 0] / tz, t[:, 1] / tz
    if vis.any():
        v = torch.from_numpy(vis)
        margin = min(margin, float(((rx.detach().abs() / limx - 1).abs())[v].min()), float(((ry.detach().abs() / limy - 1).abs())[v].min()))
    ux, uy = _clamp_fixed(rx, -limx, limx), _clamp_fixed(ry, -limy, limy)
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, zero, -(fx * ux) / tz], 1), torch.stack([zero, fy / tz, -(fy * uy) / tz], 1)], 1)
    T = J @ V[:3, :3].T
    S = torch.stack([torch.stack([c6[:, 0], c6[:, 1], c6[:, 2]], 1), torch.stack([c6[:, 1], c6[:, 3], c6[:, 4]], 1),
                     torch.stack([c6[:, 2], c6[:, 4], c6[:, 5]], 1)], 1)
    S2 = T @ S @ T.transpose(1, 2)
    a, b, c = S2[:, 0, 0] + 0.3, S2[:, 0, 1], S2[:, 1, 1] + 0.3
    det = a * c - b * b
    det = torch.where(torch.from_numpy(vis), det, torch.ones_like(det))
    cA, cB, cC = c / det, -b / det, a / det
    h = m @ P[:3, :] + P[3, :]
    w = h[:, 3] + 1e-7
    w = torch.where(torch.from_numpy(vis), w, torch.ones_like(w))
    px = ((h[:, 0] / w + L["ndc"][:, 0] + 1) * W - 1) * 0.5
    py = ((h[:, 1] / w + L["ndc"][:, 1] + 1) * H - 1) * 0.5
    op = L["opacities"].reshape(-1)

    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    tyy, txx = ys // TILE, xs // TILE
    fxs, fys = torch.tensor(xs, dtype=td), torch.tensor(ys, dtype=td)
    Tr = torch.ones(H, W, dtype=td)
    C = torch.zeros(3, H, W, dtype=td)
    done = np.zeros((H, W), bool)
    near = base.near.copy()
    for i in base.order:
        x0, y0, x1, y1 = base.splats.rect[i]
        live = (txx >= x0) & (txx < x1) & (tyy >= y0) & (tyy < y1) & ~done
        if not live.any():
            continue
        dx, dy = px[i] - fxs, py[i] - fys
        power = -0.5 * (cA[i] * dx * dx + cC[i] * dy * dy) - cB[i] * dx * dy
        pos = power.detach() > 0
        raw = op[i] * torch.exp(torch.where(pos, torch.zeros_like(power), power))
        alpha = torch.where(raw > ALPHA_MAX, torch.full_like(raw, ALPHA_MAX), raw)
        a_np = alpha.detach()
        small = a_np < 1.0 / 255.0
        test_T = Tr * (1 - alpha)
        fin = test_T.detach() < 1e-4
        reach_t = torch.from_numpy(live) & ~pos & ~small
        add = reach_t & ~fin
        near |= (add & ((raw.detach().double() / ALPHA_MAX - 1).abs() < 1e-4)).numpy()
        wgt = torch.where(add, alpha * Tr, torch.zeros_like(Tr))
        C = C + col[i][:, None, None] * wgt[None]
        Tr = torch.where(add, test_T, Tr)
        done |= (reach_t & fin).numpy()
    bgv = const(np.asarray(bg).reshape(3))
    return TorchRender(C + Tr[None] * bgv[:, None, None], (1 - Tr)[None], L, near, base, float(margin))


def gradients(r, Wi, Wa):
    """d (sum Wi image + sum Wa alpha) / d every leaf, as NumPy float64 arrays; means2D [n, 3] in the published convention
    (the NDC leaf times W/2, H/2; column 2 zero)."""
    td = r.image.dtype
    loss = (torch.tensor(Wi, dtype=td) * r.image).sum() + (torch.tensor(Wa, dtype=td) * r.alpha).sum()
    names = list(r.leaves)
    if not loss.requires_grad:                                 # nothing visible
        return {("means2D" if k == "ndc" else k): np.zeros(tuple(v.shape[:1]) + ((3,) if k == "ndc" else tuple(v.shape[1:])))
                for k, v in r.leaves.items()}
    gs = torch.autograd.grad(loss, [r.leaves[k] for k in names], allow_unused=True)
    out = {}
    for k, g in zip(names, gs):
        g = torch.zeros_like(r.leaves[k]) if g is None else g
        g = g.detach().double().numpy()
        if k == "ndc":
            # the leaf is an NDC offset: px = ((ndc + 1) W - 1) / 2, so d/dndc = dL/dpx W/2 -- the published means2D gradient
            out["means2D"] = np.concatenate([g, np.zeros((g.shape[0], 1))], 1)
        else:
            out[k] = g
    return out
