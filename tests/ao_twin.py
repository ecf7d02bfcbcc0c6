"""A float64 NumPy twin of the AO bake, written from the definition and not from csrc/ao_math.hpp: coverage,
texel frames, any-hit occlusion over ALL faces (no grid), the margin, and the analytic form factor of a disc.  Test infrastructure
only; nothing here is fast."""
import numpy as np


def coverage(faces, vt, ft, height, width):
    """(face [H*W] int, -1 = none; bary [H*W, 2] float64)"""
    vt = np.asarray(vt, np.float64)
    x, y = np.meshgrid(np.arange(width), np.arange(height))
    pu = ((x + 0.5) / width).reshape(-1)
    pv = (1.0 - (y + 0.5) / height).reshape(-1)
    face = np.full(height * width, -1, np.int64)
    bary = np.zeros((height * width, 2))

    def edge(a, b):
        return (b[0] - a[0]) * (pv - a[1]) - (b[1] - a[1]) * (pu - a[0])

    for f in range(len(faces) - 1, -1, -1):          # descending, so that the lowest face is written last
        if len(set(int(i) for i in faces[f])) < 3:
            continue
        a, b, c = vt[ft[f, 0]], vt[ft[f, 1]], vt[ft[f, 2]]
        area = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        if area == 0.0:
            continue
        w0, w1, w2 = edge(b, c), edge(c, a), edge(a, b)
        inside = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0))
        face[inside] = f
        bary[inside, 0] = w1[inside] / area
        bary[inside, 1] = w2[inside] / area
    return face, bary


def frames(verts, faces, face, bary, rot):
    """(origin, normal, tangent, bitangent) [H*W, 3] float64, zeros on uncovered texels"""
    v = np.asarray(verts, np.float64)
    n_t = len(face)
    out = [np.zeros((n_t, 3)) for _ in range(4)]
    cov = np.nonzero(face >= 0)[0]
    tri = v[np.asarray(faces)[face[cov]]]
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    b = np.asarray(bary, np.float64)[cov]
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    k = np.argmin(np.abs(n), axis=1)                 # the first of equal minima, as the definition asks
    axis = np.eye(3)[k]
    t0 = axis - n * np.take_along_axis(n, k[:, None], 1)
    t0 /= np.linalg.norm(t0, axis=1, keepdims=True)
    b0 = np.cross(n, t0)
    c, s = np.asarray(rot, np.float64)[cov, 0:1], np.asarray(rot, np.float64)[cov, 1:2]
    t = c * t0 + s * b0
    out[0][cov] = tri[:, 0] + b[:, 0:1] * e1 + b[:, 1:2] * e2
    out[1][cov] = n
    out[2][cov] = t
    out[3][cov] = np.cross(n, t)
    return out


def hits(o, d, v0, e1, e2, bias, max_distance):
    """[n_rays, F] bool: Moeller-Trumbore in float64, both sides, bias < t <= max_distance"""
    with np.errstate(divide="ignore", invalid="ignore"):
        pvec = np.cross(d[:, None, :], e2[None, :, :])
        det = np.einsum("fk,rfk->rf", e1, pvec)
        tvec = o[:, None, :] - v0[None, :, :]
        u = np.einsum("rfk,rfk->rf", tvec, pvec) / det
        qvec = np.cross(tvec, e1[None, :, :])
        v = np.einsum("rk,rfk->rf", d, qvec) / det
        t = np.einsum("fk,rfk->rf", e2, qvec) / det
        return (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > bias) & (t <= max_distance)


def occluded(verts, faces, face, origin, normal, tangent, dirs, bias, max_distance):
    """[H*W, S] bool from the given frames (bitangent = normal x tangent), against every face but the texel's own"""
    v = np.asarray(verts, np.float64)
    tri = v[np.asarray(faces)]
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    dirs = np.asarray(dirs, np.float64)
    out = np.zeros((len(face), len(dirs)), bool)
    for t in np.nonzero(face >= 0)[0]:
        n, tg = np.asarray(normal[t], np.float64), np.asarray(tangent[t], np.float64)
        if not n.any():
            continue
        bt = np.cross(n, tg)
        d = dirs[:, 0:1] * tg + dirs[:, 1:2] * bt + dirs[:, 2:3] * n
        h = hits(np.repeat(np.asarray(origin[t], np.float64)[None], len(dirs), 0), d, v0, e1, e2, bias, max_distance)
        h[:, face[t]] = False
        out[t] = h.any(1)
    return out


def margin(val, mask, height, width):
    """one margin pixel -> (values, mask)"""
    v, m = np.asarray(val, np.float64).reshape(height, width), np.asarray(mask, bool).reshape(height, width)
    out_v, out_m = v.copy(), m.copy()
    for y in range(height):
        for x in range(width):
            if m[y, x]:
                continue
            nb = [(yy, xx) for yy in (y - 1, y, y + 1) for xx in (x - 1, x, x + 1)
                  if (yy, xx) != (y, x) and 0 <= yy < height and 0 <= xx < width and m[yy, xx]]
            out_v[y, x] = sum(v[p] for p in nb) / len(nb) if nb else 0.0
            out_m[y, x] = bool(nb)
    return out_v.reshape(-1), out_m.reshape(-1)


def directions(samples):
    """the direction table, again: cosine-weighted Hammersley points about +z"""
    out = np.zeros((samples, 3))
    for i in range(samples):
        inv, f, k = 0.0, 0.5, i
        while k:
            inv += f * (k & 1)
            k >>= 1
            f *= 0.5
        u = (i + 0.5) / samples
        out[i] = [np.sqrt(u) * np.cos(2 * np.pi * inv), np.sqrt(u) * np.sin(2 * np.pi * inv), np.sqrt(1 - u)]
    return out


def disc_fraction(radius, h, samples, sides=64, angle=0.0):
    """the fraction of the table's rays from the origin (normal +z, tangent turned by `angle`) that a regular `sides`-gon of
    circumradius `radius` at height h stops; the cosine-weighted form factor of the disc is R^2 / (R^2 + h^2)"""
    ring = np.stack([radius * np.cos(2 * np.pi * np.arange(sides) / sides), radius * np.sin(2 * np.pi * np.arange(sides) / sides),
                     np.full(sides, h)], -1)
    centre = np.array([[0.0, 0.0, h]])
    v0 = np.repeat(centre, sides, 0)
    e1, e2 = ring - v0, np.roll(ring, -1, 0) - v0
    d = directions(samples)
    c, s = np.cos(angle), np.sin(angle)
    d = np.stack([c * d[:, 0] - s * d[:, 1], s * d[:, 0] + c * d[:, 1], d[:, 2]], -1)
    return hits(np.zeros((samples, 3)), d, v0, e1, e2, 1e-4, 1e9).any(1).mean()
