"""The AO bake on the device (mpmavatar_amd.ao_bake over csrc/ao.hip) against the host build of the same header (tests/hostao) and the
float64 twin (tests/ao_twin.py), on the cases of tests/ao_cases.py; then what only the device can get wrong: re-use of one baker's
scratch, two streams, the launch shapes, the argument checks."""
import dataclasses
import importlib.util
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import ao_cases as ac
import ao_twin as tw
from mpmavatar_amd.ao_bake import AOBaker, encode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def baker_of(case, **kw):
    kw = {"height": case.height, "width": case.width, "samples": case.samples, "bias": ac.BIAS, "max_distance": ac.MAX_DISTANCE, **kw}
    return AOBaker(dev(case.faces), case.vt, case.ft, **kw)


def counts(ao, samples):
    """occluded rays per texel, read back from the map"""
    return np.rint((1.0 - ao.astype(np.float64)) * samples).astype(np.int64)


_device = {}


def device_bake(name):
    """one device bake per case, shared: (baker, ao [H*W] numpy)"""
    if name not in _device:
        case = ac.baked(name)["case"]
        b = baker_of(case)
        _device[name] = (b, b.bake(dev(case.verts)).cpu().numpy().reshape(-1))
    return _device[name]


@pytest.mark.parametrize("name", ["A", "B", "C0", "D"])
def test_agrees_with_the_host_build(name):
    h = ac.baked(name)
    case = h["case"]
    b, ao = device_bake(name)
    face, bary = (x.cpu().numpy() for x in b.coverage)
    assert face.shape == (case.height, case.width) and bary.shape == (case.height, case.width, 2)
    assert np.array_equal(face.reshape(-1), h["face"])
    assert np.array_equal(bary.reshape(-1, 2).view(np.uint32), h["bary"].view(np.uint32))
    assert np.array_equal(b.covered.cpu().numpy(), np.nonzero(h["face"] >= 0)[0])
    o, n, t = (x.cpu().numpy() for x in b.texel_frames(dev(case.verts)))
    for got, want, what in ((o, h["o"], "origin"), (n, h["n"], "normal"), (t, h["t"], "tangent")):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}: {np.abs(got - want).max()}"
    cov = h["face"] >= 0
    assert np.array_equal(counts(ao, case.samples)[cov], h["occ"][cov])
    assert np.array_equal(ao.view(np.uint32), h["ao"].view(np.uint32))              # margin 0 at this size: the map is the trace's
    assert not ao[~cov].any()
    # the device's own frames, fed to the host's brute force over all faces
    assert np.array_equal(ac.host_count(case, h["face"], o, n, t, h["dirs"], brute=True)[cov], counts(ao, case.samples)[cov])
    if name == "A":
        assert (ao[cov] == 1.0).all()
    if name == "B":
        assert (ao[cov] == 0.0).all()


def test_against_the_float64_twin():
    h = ac.baked("C0")
    case = h["case"]
    b, ao = device_bake("C0")
    o, n, t = (x.cpu().numpy() for x in b.texel_frames(dev(case.verts)))
    want = tw.occluded(case.verts, case.faces, h["face"], o, n, t, h["dirs"], ac.BIAS, ac.MAX_DISTANCE).sum(1)
    cov = h["face"] >= 0
    diff = np.abs(want - counts(ao, case.samples))[cov]
    print(f"{cov.sum() * case.samples} rays, {diff.sum()} differing counts, worst texel {diff.max()}")
    assert diff.sum() <= 1e-3 * cov.sum() * case.samples and diff.max() <= 2


def test_rerun_and_reuse_of_one_baker():
    case = ac.baked("C0")["case"]
    b, first = device_bake("C0")
    v = dev(case.verts)
    moved = (v * 3.0 + torch.tensor([5.0, 0.0, 0.0], device=DEV)).contiguous()
    again = b.bake(v).cpu().numpy().reshape(-1)
    assert np.array_equal(again.view(np.uint32), first.view(np.uint32))
    # C, then C scaled by 3 and moved by (5, 0, 0), then C again, through ONE baker: stale cell counts or a stale box would show
    one = baker_of(case)
    seq = [one.bake(x).clone() for x in (v, moved, v)]
    fresh = [baker_of(case).bake(x) for x in (v, moved, v)]
    for got, want in zip(seq, fresh):
        assert torch.equal(got, want)
    assert torch.equal(seq[0], seq[2]) and np.array_equal(seq[0].cpu().numpy().reshape(-1).view(np.uint32), first.view(np.uint32))
    # the moved mesh against the host build, with the scaled bias the larger mesh still clears
    h = ac.baked("C0")
    ao_h, _ = ac.host_bake(case, h["face"], h["bary"], h["rot"], h["dirs"], verts=moved.cpu().numpy())
    assert np.array_equal(seq[1].cpu().numpy().reshape(-1).view(np.uint32), ao_h.view(np.uint32))


def test_two_bakers_on_two_streams():
    h0, h1 = ac.baked("C0"), ac.baked("C1")
    b0, b1 = baker_of(h0["case"]), baker_of(h1["case"])
    v0, v1 = dev(h0["case"].verts), dev(h1["case"].verts)
    torch.cuda.synchronize()
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = [[], []]
    for _ in range(3):
        with torch.cuda.stream(s0):
            outs[0].append(b0.bake(v0))
        with torch.cuda.stream(s1):
            outs[1].append(b1.bake(v1))
    torch.cuda.synchronize()
    for got in outs[0]:
        assert np.array_equal(got.cpu().numpy().reshape(-1).view(np.uint32), device_bake("C0")[1].view(np.uint32))
    for got in outs[1]:
        assert np.array_equal(got.cpu().numpy().reshape(-1).view(np.uint32), h1["ao"].view(np.uint32))


@pytest.mark.parametrize("samples", [1, 63, 64, 65, 256])
def test_sample_counts_around_the_wave(samples):
    h = ac.baked("C0")
    case = dataclasses.replace(h["case"], samples=samples)
    dirs, _ = ac.tables(case)
    want, occ = ac.host_bake(case, h["face"], h["bary"], h["rot"], dirs)
    got = baker_of(case).bake(dev(case.verts)).cpu().numpy().reshape(-1)
    cov = h["face"] >= 0
    assert np.array_equal(counts(got, samples)[cov], occ[cov]) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert occ[cov].max() > 0 and not got[~cov].any()


@pytest.mark.parametrize("height,width", [(1, 1), (33, 17)])
def test_map_sizes(height, width):
    base = ac.baked("A")["case"] if height == 1 else ac.baked("C0")["case"]
    case = dataclasses.replace(base, height=height, width=width)
    dirs, rot = ac.tables(case)
    face, bary = ac.host_coverage(case)
    want, _ = ac.host_bake(case, face, bary, rot, dirs)
    b = baker_of(case)
    got = b.bake(dev(case.verts))
    assert tuple(got.shape) == (height, width)
    assert np.array_equal(b.coverage[0].cpu().numpy().reshape(-1), face) and (face >= 0).sum() >= 1
    assert np.array_equal(got.cpu().numpy().reshape(-1).view(np.uint32), want.view(np.uint32))


def test_a_mesh_that_covers_nothing_gives_zeros():
    base = ac.baked("C0")["case"]
    case = dataclasses.replace(base, vt=(base.vt + 4.0).astype(np.float32))          # every UV triangle outside the map
    b = baker_of(case)
    assert b.n_covered == 0 and (b.coverage[0] == -1).all()
    assert not b.bake(dev(case.verts)).any()
    o, n, t = b.texel_frames(dev(case.verts))
    assert not o.any() and not n.any() and not t.any()
    none = AOBaker(torch.zeros(0, 3, dtype=torch.int32, device=DEV), np.zeros((0, 2), np.float32), np.zeros((0, 3), np.int32), height=8, width=8)
    assert not none.bake(torch.zeros(1, 3, device=DEV)).any()


@pytest.mark.parametrize("margin", [1, 2])
def test_margin_against_the_host_build(margin):
    h = ac.baked("C0")
    case = h["case"]
    got = baker_of(case, margin=margin).bake(dev(case.verts)).cpu().numpy().reshape(-1)
    val, mask = h["ao"], (h["face"] >= 0).astype(np.uint8)
    for _ in range(margin):
        val, mask = ac.host_margin(val, mask, case.height, case.width)
    assert mask.sum() > (h["face"] >= 0).sum()
    assert np.array_equal(got.view(np.uint32), val.view(np.uint32))


def test_default_resolution_has_one_margin_pixel():
    a = ac.baked("A")["case"]
    b = AOBaker(dev(a.faces), a.vt, a.ft, samples=16)
    assert (b.height, b.width, b.margin) == (256, 256, 1)                            # bake.py: --ao_res 256, margin = ao_res // 256
    ao = b.bake(dev(a.verts))
    ao, cov = ao.cpu(), (b.coverage[0] >= 0).cpu()
    ring = torch.nn.functional.max_pool2d(cov[None, None].float(), 3, 1, 1)[0, 0].bool() & ~cov      # on the host
    assert cov.sum() > 40000 and ring.sum() > 800
    assert (ao[cov] == 1.0).all() and (ao[ring] == 1.0).all() and not ao[~cov & ~ring].any()


def test_a_grid_that_does_not_fit_is_loud():
    h = ac.baked("C0")
    case = h["case"]
    ao = baker_of(case, max_entries=100).bake(dev(case.verts)).cpu().numpy().reshape(-1)
    cov = h["face"] >= 0
    assert np.isnan(ao[cov]).all() and not ao[~cov].any()
    one = baker_of(case, max_cells=1).bake(dev(case.verts)).cpu().numpy().reshape(-1)        # one cell: brute force through the grid's code
    assert np.array_equal(one.view(np.uint32), h["ao"].view(np.uint32))


def test_argument_errors_raise_before_any_launch():
    c = ac.baked("C0")["case"]
    f = dev(c.faces)
    bad_ft = c.ft.copy()
    bad_ft[3, 1] = len(c.vt)
    bad_vt = c.vt.copy()
    bad_vt[7, 0] = np.nan
    bad_f = c.faces.copy()
    bad_f[0, 0] = -1
    for args, kw in (((f, c.vt, c.ft[:-1]), {}), ((f, c.vt, bad_ft), {}), ((f, bad_vt, c.ft), {}), ((dev(bad_f), c.vt, c.ft), {}),
                     ((f, c.vt, c.ft), {"samples": 0}), ((f, c.vt, c.ft), {"samples": 4097}), ((f, c.vt, c.ft), {"height": 0}),
                     ((f.cpu(), c.vt, c.ft), {}), ((f.long(), c.vt, c.ft), {}), ((f, c.vt.astype(np.float64), c.ft), {}),
                     ((f, c.vt, c.ft), {"bias": 1.0, "max_distance": 0.5})):
        with pytest.raises(RuntimeError):
            AOBaker(*args, **kw)
    b = device_bake("C0")[0]
    v = dev(c.verts)
    for verts in (v[:-1].contiguous(), v.double(), v.cpu(), v[:, :2].contiguous(), c.verts):
        with pytest.raises(RuntimeError):
            b.bake(verts)
        with pytest.raises(RuntimeError):
            b.texel_frames(verts)
    with pytest.raises(RuntimeError):
        b.bake(v, out=torch.empty(3, 3, device=DEV))


def _read_png(path):
    """[H, W, 3] uint8 of an 8-bit RGB PNG whose rows use filter 0 (what io_formats.write_png writes)"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, size = 8, b"", None
    while at < len(data):
        n, tag = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        if tag == b"IHDR":
            size = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        at += 12 + n
    w, h = size[0], size[1]
    assert size[2:] == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, 3)


def test_write_png_round_trip(tmp_path):
    b, ao = device_bake("C0")
    path = b.write_png(str(tmp_path / "aomap"), 7, torch.from_numpy(ao).view(b.height, b.width))
    assert path.endswith("aomap/007.png")
    px = _read_png(path)
    want = np.floor(255.0 * ao.astype(np.float32) + np.float32(0.5)).astype(np.uint8).reshape(b.height, b.width)     # round(255 AO)
    assert len(np.unique(want)) > 10
    for c in range(3):
        assert np.array_equal(px[:, :, c], want)
    srgb = _read_png(b.write_png(str(tmp_path / "srgb"), 7, ao.reshape(b.height, b.width), encoding="srgb"))
    assert np.array_equal(srgb[:, :, 0], np.floor(255.0 * encode(ao, "srgb").astype(np.float32) + np.float32(0.5)).astype(np.uint8).reshape(b.height, b.width))
    assert (srgb[:, :, 0] >= px[:, :, 0]).all() and (srgb[:, :, 0] > px[:, :, 0]).any()
    with pytest.raises(RuntimeError):
        b.write_png(str(tmp_path), 0, ao.reshape(b.height, b.width), encoding="gamma")


def test_demo_end_to_end(tmp_path):
    """solver -> bake -> shaded colours -> rasteriser -> aomap/NNN.png and frame_NNN.png (examples/ao_bake_demo.py), small"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ao_bake_demo", os.path.join(root, "examples", "ao_bake_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--out", str(tmp_path), "--frames", "2", "--substeps", "60", "--size", "96", "--ao-res", "64", "--samples", "64",
                    "--gaussians-per-face", "2"])
    ao, image = out["ao"].cpu().numpy(), out["image"].cpu().numpy()
    assert ao.shape == (64, 64) and image.shape == (3, 96, 96) and np.isfinite(ao).all() and np.isfinite(image).all()
    print("ao_bake_demo at 64 x 64: over the sphere %.3f, at the corner %.3f, mean %.3f" % (ao[32, 32], ao[3, 3], out["mean_ao"][-1]))
    assert ao[32, 32] < 0.6 and ao[3, 3] > 0.9                              # the sphere shades the middle of the sheet, not its corner
    for k in (1, 2):
        px = _read_png(str(tmp_path / "aomap" / f"{k:03d}.png"))
        assert px.shape == (64, 64, 3) and (px[:, :, 0] == px[:, :, 1]).all() and (px[:, :, 0] == px[:, :, 2]).all()
        frame = _read_png(str(tmp_path / f"frame_{k:03d}.png"))
        assert frame.shape == (96, 96, 3) and (frame == 255).all(2).any() and not (frame == 255).all()
    assert np.array_equal(px[:, :, 0], np.floor(255.0 * ao + np.float32(0.5)).astype(np.uint8))      # the file is the returned map
