"""Cases, yardstick and helpers shared by tests/test_image_head_host.py, tests/test_image_head_abi.py and
tests/test_gpu_image_head.py.  Test infrastructure only.

  case    H x W    n_cam  cam  what it holds
  main    37 x 29  5      2    H W odd: the pixel-by-pixel path, two workgroups with the second nearly empty; render in about
                               [-0.1, 1.2] so both sides of the clip bind; mask in [0, 1] with a block of exact zeros
  vec     48 x 64  3      0    the 16-byte path, three workgroups
  last    16 x 20  4      3    the last row of cam_m / cam_c; LAST_AS_ROW runs it again with both given as [3] and camera_idx None
  one     1 x 1    2      1    a single pixel
  dark    8 x 8    3      1    mask == 0 everywhere: image zero, d_render zero, d_mask not, the cam gradients zero
  edges   16 x 16  3      1    cam_m[cam][0] = cam_c[cam][0] = 0; planted pixels of channel 0 with render = 0 under a non-zero mask
                               (v = 0 exactly) and with render = 1 under mask = 1 (v = 1 exactly): the gradient passes at both

The loss of a case is sum(w * image); its gradients go to render, mask, cam_m and cam_c (GRADS).  The yardstick is the float64 run of
tests/image_head_twin_torch.py on the float32 inputs.  A case is drawn from its seed; a draw that leaves a pixel's unclipped value
within CLIP_MARGIN of a clip bound is thrown away whole and the next seed drawn (no pixel is ever left out), and render values whose
8-bit frame would sit within BYTE_MARGIN of a byte boundary are redrawn (`case` asserts both)."""
import ctypes as C
import functools

import numpy as np
import torch

import hostbuild
import image_head_twin_torch as tw

CASES = ("main", "vec", "last", "one", "dark", "edges")
BYTE_CASES = ("main", "vec", "last", "one")     # the cases frame_bytes is run on
GRADS = ("render", "mask", "cam_m", "cam_c")
TENSORS = ("image",) + GRADS
CLIP_MARGIN = 1e-5     # the fp32 error of v for |v| <= 2 is below 5e-7: beyond this margin fp32 and float64 clip alike
BYTE_MARGIN = 1e-3     # in units of one byte: 255 * 5e-7 is far below it, so fp32 and float64 truncate alike

# Measured on the CPU (tests/test_image_head_host.py::test_s32_is_the_measurement asserts it, from above and from below at half):
# S32 = the worst, over the cases and the five tensors, of max |t32 - t64| / max |t64| of the TWIN, its float32 run against its
# float64 run.  The code under test plays no part in it.  Host restatement and GPU must lie within BOUND = 10 * S32 of the float64
# twin -- the margin the sibling features give a different operation order and a different expf.
S32 = 1.6e-7   # measured 1.542e-7 (cam_c of `main`); the other 29 figures 0 .. 1.34e-7
BOUND = 10 * S32

_SHAPES = {"main": (37, 29, 5, 2, 0), "vec": (48, 64, 3, 0, 1), "last": (16, 20, 4, 3, 2), "one": (1, 1, 2, 1, 3),
           "dark": (8, 8, 3, 1, 4), "edges": (16, 16, 3, 1, 5)}      # H, W, n_cam, cam, first seed
EDGE_ZERO = ((2, 3), (7, 7), (15, 0))      # (y, x): render[0] = 0, mask != 0
EDGE_ONE = ((0, 0), (9, 12), (15, 15))     # (y, x): render[0] = 1, mask = 1
FRAME_FORMS = ((True, False), (True, True), (False, False), (False, True))     # (with the affine, white_bkgd)


def _t64(c, k):
    return torch.tensor(np.asarray(c[k]), dtype=torch.float64)


def unclipped64(c):
    """v of every pixel in float64 [3, H, W]"""
    return tw.unclipped(_t64(c, "render"), _t64(c, "mask"), _t64(c, "cam_m"), _t64(c, "cam_c"), c["cam"]).numpy()


def planted(name, shape):
    """bool [3, H, W]: the pixels of `edges` whose v is an exact 0 or 1 by construction"""
    p = np.zeros(shape, bool)
    if name == "edges":
        for y, x in EDGE_ZERO + EDGE_ONE:
            p[0, y, x] = True
    return p


def clip_distance(name, c):
    """the least distance of a v from a clip bound over EVERY pixel that is neither zero through its mask nor planted; inf if none"""
    v = unclipped64(c)
    exact = (np.broadcast_to(c["mask"] == 0, v.shape) & (v == 0)) | (planted(name, v.shape) & ((v == 0) | (v == 1)))
    d = np.minimum(np.abs(v), np.abs(v - 1.0))
    return float(d[~exact].min()) if (~exact).any() else float("inf")


def frame64(c, affine, white):
    """255 * the clamped frame in float64, [H, W, 3]"""
    a = (_t64(c, "cam_m"), _t64(c, "cam_c"), c["cam"]) if affine else (None, None, None)
    return 255.0 * tw.frame(_t64(c, "render"), _t64(c, "mask")[None], *a, white).numpy()


def byte_offenders(c):
    """bool [H, W]: pixels where, in some form of the frame, 255 r is within BYTE_MARGIN of a byte boundary other than an exact 0 or
    255 that the mask made (r = 0 or 1 through mask == 0, in fp32 as in float64)"""
    bad = np.zeros(c["mask"].shape, bool)
    for affine, white in FRAME_FORMS:
        f = frame64(c, affine, white)
        near = np.abs(f - np.rint(f)) <= BYTE_MARGIN
        near &= ~(c["mask"] == 0)[..., None]
        # far beyond a clip bound the clamp decides, alike in both precisions
        a = (_t64(c, "cam_m"), _t64(c, "cam_c"), c["cam"]) if affine else (None, None, None)
        raw = tw.unclipped(_t64(c, "render"), _t64(c, "mask"), *a).numpy() if affine else (_t64(c, "render") * _t64(c, "mask")).numpy()
        if white:
            raw = raw + (1.0 - c["mask"].astype(np.float64))
        beyond = (raw < -CLIP_MARGIN) | (raw > 1.0 + CLIP_MARGIN)
        near &= ~np.moveaxis(beyond, 0, -1)
        bad |= near.any(axis=-1)
    return bad


def _draw(name, seed):
    H, W, n_cam, cam, _ = _SHAPES[name]
    rng = np.random.default_rng(seed)
    c = {"render": rng.uniform(-0.1, 1.2, (3, H, W)).astype(np.float32), "mask": rng.uniform(0.0, 1.0, (H, W)).astype(np.float32),
         "cam_m": rng.normal(0, 0.2, (n_cam, 3)).astype(np.float32), "cam_c": rng.normal(0, 0.05, (n_cam, 3)).astype(np.float32),
         "w": rng.normal(size=(3, H, W)).astype(np.float32), "cam": cam}
    if name == "main":
        c["mask"][5:12, 3:17] = 0.0
        c["mask"][30:, 20:] = 1.0
    elif name == "one":
        c["render"][:, 0, 0] = (0.3, 0.5, 0.7)
        c["mask"][0, 0] = 0.8
    elif name == "dark":
        c["mask"][:] = 0.0
    elif name == "edges":
        c["cam_m"][cam, 0] = 0.0
        c["cam_c"][cam, 0] = 0.0
        for y, x in EDGE_ZERO:
            c["render"][0, y, x] = 0.0
            c["mask"][y, x] = max(c["mask"][y, x], np.float32(0.25))
        for y, x in EDGE_ONE:
            c["render"][0, y, x] = 1.0
            c["mask"][y, x] = 1.0
    if name in BYTE_CASES:
        for _ in range(100):
            bad = byte_offenders(c)
            if not bad.any():
                break
            c["render"][:, bad] = rng.uniform(-0.1, 1.2, (3, int(bad.sum()))).astype(np.float32)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: render [3, H, W], mask [H, W], cam_m, cam_c [n_cam, 3], w [3, H, W] (read-only float32 arrays), cam (int)"""
    seed = _SHAPES[name][4]
    while True:
        c = _draw(name, seed)
        if clip_distance(name, c) > CLIP_MARGIN:
            break
        seed += 100                                  # the whole draw again: no pixel is left out
    assert clip_distance(name, c) > CLIP_MARGIN
    assert name not in BYTE_CASES or not byte_offenders(c).any()
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def rel(t, t64):
    """max |t - t64| / max |t64| over EVERY element; a tensor that is all zero in float64 must be all zero"""
    t, t64 = np.asarray(t, np.float64), np.asarray(t64, np.float64)
    assert t.shape == t64.shape, (t.shape, t64.shape)
    top = np.abs(t64).max()
    if top == 0.0:
        assert (t == 0).all()
        return 0.0
    return float(np.abs(t - t64).max() / top)


def twin(c, dtype=torch.float64, upstream=None):
    """the twin's image and the gradients of sum(w * image) in `dtype` -> dict over TENSORS (numpy); upstream: another w"""
    t = {k: torch.tensor(np.asarray(c[k]), dtype=dtype, requires_grad=True) for k in GRADS}
    image = tw.camera_image(t["render"], t["mask"], t["cam_m"], t["cam_c"], c["cam"])
    w = torch.tensor(np.asarray(c["w"] if upstream is None else upstream), dtype=dtype)
    grads = torch.autograd.grad((w * image).sum(), [t[k] for k in GRADS])
    out = {"image": image.detach().numpy()}
    out.update({k: g.numpy() for k, g in zip(GRADS, grads)})
    return out


@functools.lru_cache(maxsize=None)
def t64(name):
    """the float64 twin of a case, computed once and shared"""
    out = twin(case(name))
    for v in out.values():
        v.setflags(write=False)
    return out


def bytes64(c, affine, white):
    """the expected frame: floor of the float64 value, uint8 [H, W, 3]"""
    return np.floor(frame64(c, affine, white)).astype(np.uint8)


# ---- the host build of image_head_math.hpp ---------------------------------------------------------------------------------------

def host_lib():
    lib = hostbuild.host_lib("hostimagehead")
    lib.ih_workgroups.restype = C.c_int32
    lib.ih_workgroups.argtypes = [C.c_int64]
    return lib


def sanitizer_program():
    """the same file as a stand-alone program under AddressSanitizer and UBSan (run as a subprocess; nothing is loaded into Python)"""
    return hostbuild.host_program("hostimagehead", name="hostimagehead_asan",
                                  flags=["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DHOSTIMAGEHEAD_MAIN"])


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def scratch_doubles(H, W):
    return min((H * W + 1023) // 1024, 1024) * 6


def host_run(c, want=GRADS, g=True):
    """forward, backward map and fold on the host -> dict over TENSORS; a gradient not in `want` goes in as NULL and comes back None"""
    _, H, W = c["render"].shape
    n_cam = c["cam_m"].shape[0]
    render, mask, cam_m, cam_c = [_f32(c[k]) for k in GRADS]
    image = np.full((3, H, W), np.nan, np.float32)
    d = {k: (np.full(np.asarray(c[k]).shape, np.nan, np.float32) if k in want else None) for k in GRADS}
    scratch = np.full(scratch_doubles(H, W), np.nan, np.float64)
    lib = host_lib()
    shared = [_p(render), _p(mask), _p(cam_m), _p(cam_c), n_cam, c["cam"], H, W]
    lib.ih_forward(*shared, _p(image))
    lib.ih_backward(*shared, _p(_f32(c["w"])) if g else None, _p(scratch), _p(d["render"]), _p(d["mask"]), _p(d["cam_m"]), _p(d["cam_c"]))
    return {"image": image, **d}


def host_bytes(render, mask, cam_m, cam_c, cam, white):
    _, H, W = render.shape
    out = np.full((H, W, 3), 77, np.uint8)
    n_cam = 0 if cam_m is None else cam_m.shape[0]
    host_lib().ih_bytes(_p(_f32(render)), _p(_f32(mask)), _p(_f32(cam_m)), _p(_f32(cam_c)), n_cam, cam or 0, int(white), H, W, _p(out))
    return out


def host_compose(rgb, msk, white):
    _, H, W = rgb.shape
    out = np.full((3, H, W), np.nan, np.float32)
    host_lib().ih_compose(_p(_f32(rgb)), _p(_f32(msk)), int(white), H, W, _p(out))
    return out


def host_eval_pair(pred, gt, mask, remove_white):
    H, W = mask.shape
    a, b = np.full((3, H, W), np.nan, np.float32), np.full((3, H, W), np.nan, np.float32)
    host_lib().ih_eval_pair(_p(np.ascontiguousarray(pred, np.uint8)), _p(np.ascontiguousarray(gt, np.uint8)), _p(_f32(mask)), int(remove_white),
                            H, W, _p(a), _p(b))
    return a, b


# ---- numpy's statement of the evaluation side ------------------------------------------------------------------------------------

def numpy_compose(rgb, msk, white):
    """train_appearance.py:108-110 in float32"""
    out = rgb.astype(np.float32) * msk.astype(np.float32)
    return out + (np.float32(1.0) - msk.astype(np.float32)) if white else out


def numpy_eval_pair(pred, gt, mask, remove_white):
    """eval.py:68-87 with numpy in place of torch: astype(float32).transpose(2, 0, 1) / 255., mean(axis=0) > 0.90, times the mask"""
    out = []
    for img in (pred, gt):
        f = img.astype(np.float32).transpose(2, 0, 1) / np.float32(255.)
        if remove_white:
            f = f.copy()
            f[:, torch.from_numpy(np.ascontiguousarray(f)).mean(axis=0).numpy() > 0.90] = 0
        out.append(f * mask.astype(np.float32)[None])
    return out


def eval_frames(H, W, seed=11):
    """two random byte frames with white, nearly white and exactly-at-the-rule pixels planted, and a float mask"""
    rng = np.random.default_rng(seed)
    pred, gt = rng.integers(0, 256, (H, W, 3)).astype(np.uint8), rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    pred[0, 0], pred[0, 1], pred[0, 2] = (255, 255, 255), (230, 229, 229), (230, 230, 229)       # sums 765, 688, 689
    gt[0, 1], gt[0, 2], gt[H - 1, W - 1] = (229, 230, 230), (228, 230, 230), (255, 255, 179)     # sums 689, 688, 689
    mask = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    mask[0, 0] = 1.0
    return pred, gt, mask
