"""The colour path of the appearance loop (train_appearance.py:120-123) restated in torch with the dtype as a parameter, so that
autograd gives the gradients mpmavatar_amd/csrc/shade_math.hpp must reproduce:

    colors = sample(shadow_map, uv)[binding][:, None] * clamp_min(eval_sh(deg, features, normalize(means3D - campos)) + 0.5, 0)

``sample`` is grid_sample's rule for bilinear / align_corners=False / zeros padding written out (the cell by floor, four products,
taps outside the map dropped); the SH part is tests/raster_twin_torch.py's, whose clamp has zero slope where it binds.  It is pinned
against the reference's own functions and torch's F.grid_sample by tests/golden/shade.npz (tests/test_shade_host.py).

Test infrastructure only; nothing under mpmavatar_amd/ imports it."""
import torch

import raster_twin_torch as tt


def taps(uv, H, W):
    """-> (idx [F, 4] long, -1 outside the map; w [F, 4]) in uv's dtype; corners north-west, north-east, south-west, south-east"""
    ix, iy = ((uv[:, 0] + 1) * W - 1) / 2, ((uv[:, 1] + 1) * H - 1) / 2
    x0, y0 = torch.floor(ix), torch.floor(iy)
    x1, y1 = x0 + 1, y0 + 1
    w = torch.stack([(x1 - ix) * (y1 - iy), (ix - x0) * (y1 - iy), (x1 - ix) * (iy - y0), (ix - x0) * (iy - y0)], 1)
    xs, ys = torch.stack([x0, x1, x0, x1], 1), torch.stack([y0, y0, y1, y1], 1)
    inside = (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
    idx = ys.clamp(0, H - 1).long() * W + xs.clamp(0, W - 1).long()
    return torch.where(inside, idx, torch.full_like(idx, -1)), w


def sample(smap, uv):
    """smap [H, W], uv [F, 2] -> [F]"""
    H, W = smap.shape
    idx, w = taps(uv, H, W)
    vals = smap.reshape(-1)[idx.clamp(min=0)]
    return torch.where(idx >= 0, vals * w, torch.zeros_like(w)).sum(1)


def sh_colour(deg, dc, rest, means, campos):
    """-> (clamped colour [n, 3], the unclamped sh + 0.5)"""
    return tt.sh_colour(deg, torch.cat([dc, rest], 1), means, campos)


def shaded(deg, dc, rest, means, campos, smap=None, uv=None, binding=None):
    """-> colors [n, 3]; dc = None: the colour before the shadow is 1; smap = None: no shadow"""
    if dc is None:
        colour = torch.ones(binding.shape[0], 3, dtype=smap.dtype)
    else:
        colour = sh_colour(deg, dc, rest, means, campos)[0]
    if smap is None:
        return colour
    return sample(smap, uv)[binding.long()][:, None] * colour
