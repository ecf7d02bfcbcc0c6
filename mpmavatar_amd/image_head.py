"""The image head of the appearance loop on the GPU: the expression between the render call and the loss
(train_appearance.py:126-127, again at :206-207, train_material_params.py:865-870 and run_demo.py),

    image = render_pkg["render"] * torch.exp(gaussians.cam_m[camera_idx])[:, None, None] + gaussians.cam_c[camera_idx][:, None, None]
    image = (image * render_pkg["mask"]).clip(0., 1.)

becomes

    from mpmavatar_amd.image_head import camera_image
    image = camera_image(render_pkg["render"], render_pkg["mask"], gaussians.cam_m, gaussians.cam_c, camera_idx)

over ``mpmhip_image_head_forward`` and ``mpmhip_image_head_backward`` (csrc/image_head.hip): ONE forward launch and, in
``loss.backward()``, two (the map with the partial sums, then their fold) where torch issues about seven and a dozen.  This is
where the trained per-camera parameters ``cam_m`` and ``cam_c`` get their gradient, and where the rasteriser's alpha gets its
second gradient path (``image * mask``).

The evaluation side, forward only, replaces the PNG, OpenCV and host detour of train_material_params.py:865-876 and
eval.py:68-87:

    pred_u8 = frame_bytes(render, mask, cam_m, cam_c, camera_idx, white_bkgd)      # uint8 [H, W, 3]: what :870 writes to a PNG
    gt_u8 = frame_bytes(gt_rgb, gt_msk, None, None, None, white_bkgd)              # :847-849 and :874
    img_pred, img_gt = eval_inputs(pred_u8, gt_u8, eval_mask(mask_gt), remove_white)   # eval.py:68-87
    ev.add_frame(img_pred, img_gt)                                                 # mpmavatar_amd.image_loss.AppEval

and ``compose_gt(rgb, msk, white_bkgd)`` is the ground-truth image of the training loop (train_appearance.py:108-110).

Inputs are fp32 tensors on the GPU (the byte frames uint8); the kernels run on the current torch stream; no value passes
through the host; there is no double backward.  No CPU fallback: tensors must live on an MI355X (``eval_mask`` alone is torch
operations and runs wherever its argument lives).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from ._call import call, expect, ptr, upstream

WHITE_SUM = 689      # eval.py:73: mean of three bytes / 255 > 0.90  <=>  their sum >= 689


def workgroups(H, W):
    """MPMHIP_IMAGE_HEAD_WORKGROUPS of include/mpmhip.h: one workgroup per 1024 pixels, at most 1024."""
    return min((H * W + 1023) // 1024, 1024)


def scratch_doubles(H, W):
    """MPMHIP_IMAGE_HEAD_SCRATCH of include/mpmhip.h: six partial sums per workgroup."""
    return workgroups(H, W) * 6


def _planes(render, mask, names=("render", "mask")):
    """(render [3, H, W], mask [H, W]) contiguous, of one device"""
    expect(render, torch.float32, names[0], contiguous=False)
    expect(mask, torch.float32, names[1], contiguous=False)
    if render.dim() != 3 or render.shape[0] != 3 or render.numel() == 0:
        raise RuntimeError(f"{names[0]}: expected a non-empty [3, H, W] tensor, got {tuple(render.shape)}")
    H, W = render.shape[1:]
    if tuple(mask.shape) not in ((1, H, W), (H, W)):
        raise RuntimeError(f"{names[1]}: expected shape {(1, H, W)} or {(H, W)}, got {tuple(mask.shape)}")
    if mask.device != render.device:
        raise RuntimeError(f"{names[0]} and {names[1]} must be on one device")
    if H * W > 2 ** 31 - 1:
        raise RuntimeError("more than 2^31 - 1 pixels")
    return render.contiguous(), mask.contiguous()


def _camera(cam_m, cam_c, camera_idx, dev):
    """(cam_m, cam_c) as [n_cam, 3] views and the row as a Python int.  The row of a CPU tensor is read on the host, where it
    lives; a GPU tensor would hide a synchronisation and is refused."""
    expect(cam_m, torch.float32, "cam_m")
    expect(cam_c, torch.float32, "cam_c")
    if cam_m.shape != cam_c.shape or cam_m.device != dev or cam_c.device != dev:
        raise RuntimeError(f"cam_m and cam_c must have one shape and the images' device, got {tuple(cam_m.shape)} and {tuple(cam_c.shape)}")
    if cam_m.dim() == 1:
        if tuple(cam_m.shape) != (3,) or camera_idx is not None:
            raise RuntimeError("cam_m and cam_c of one camera are [3] and take camera_idx=None")
        return cam_m.view(1, 3), cam_c.view(1, 3), 0
    if cam_m.dim() != 2 or cam_m.shape[1] != 3 or cam_m.shape[0] == 0:
        raise RuntimeError(f"cam_m: expected [n_cam, 3] or [3], got {tuple(cam_m.shape)}")
    if isinstance(camera_idx, torch.Tensor):
        if camera_idx.is_cuda:
            raise TypeError("camera_idx is a GPU tensor: reading it would synchronise; pass a Python int or a CPU tensor")
        if camera_idx.numel() != 1 or camera_idx.dtype.is_floating_point or camera_idx.dtype == torch.bool:
            raise RuntimeError("camera_idx: expected one integer")
        camera_idx = int(camera_idx)
    if isinstance(camera_idx, bool) or not isinstance(camera_idx, int):
        raise RuntimeError(f"camera_idx: expected a Python int or a CPU integer tensor, got {type(camera_idx).__name__}")
    if not 0 <= camera_idx < cam_m.shape[0]:
        raise RuntimeError(f"camera_idx {camera_idx} outside [0, {cam_m.shape[0]})")
    return cam_m, cam_c, camera_idx


class _CameraImage(torch.autograd.Function):
    """(render [3, H, W], mask, cam_m, cam_c [n_cam, 3]) -> image [3, H, W].  want_grad: whether a graph is being built (the
    caller's grad mode; ctx.needs_input_grad ignores it)."""

    @staticmethod
    def forward(ctx, render, mask, cam_m, cam_c, cam, want_grad):
        _, H, W = render.shape
        image = torch.empty_like(render)
        call("mpmhip_image_head_forward", render.device, render.data_ptr(), mask.data_ptr(), cam_m.data_ptr(), cam_c.data_ptr(),
             cam_m.shape[0], cam, H, W, image.data_ptr())
        if want_grad:
            ctx.save_for_backward(render, mask, cam_m, cam_c)
            ctx.cam = cam
        return image

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_image):
        render, mask, cam_m, cam_c = ctx.saved_tensors
        _, H, W = render.shape
        dev = render.device
        want = ctx.needs_input_grad
        d_render = torch.empty_like(render) if want[0] else None
        d_mask = torch.empty_like(mask) if want[1] else None
        d_cam_m = torch.empty_like(cam_m) if want[2] else None
        d_cam_c = torch.empty_like(cam_c) if want[3] else None
        scratch = torch.empty(scratch_doubles(H, W), dtype=torch.float64, device=dev) if want[2] or want[3] else None
        g = upstream(g_image, render.shape)
        call("mpmhip_image_head_backward", dev, render.data_ptr(), mask.data_ptr(), cam_m.data_ptr(), cam_c.data_ptr(), cam_m.shape[0],
             ctx.cam, H, W, ptr(g), ptr(scratch), ptr(d_render), ptr(d_mask), ptr(d_cam_m), ptr(d_cam_c))
        return d_render, d_mask, d_cam_m, d_cam_c, None, None


def camera_image(render, mask, cam_m, cam_c, camera_idx):
    """train_appearance.py:126-127: ``((render * exp(cam_m[camera_idx]) + cam_c[camera_idx]) * mask).clip(0, 1)`` as a
    contiguous [3, H, W] tensor, NaN propagating as in torch.  render [3, H, W]; mask [1, H, W] or [H, W] (the rasteriser's
    alpha); cam_m, cam_c [n_cam, 3] with camera_idx a Python int or a CPU integer tensor (a GPU tensor raises TypeError: it would
    hide a synchronisation), or both [3] with camera_idx None.  Gradients go to all four tensors, each only where it is
    required; the clip has torch's slope (the gradient passes where 0 <= v <= 1, both ends included), and the gradients of
    cam_m and cam_c are dense, zero off the camera's row, as torch's index backward makes them.  Under ``torch.no_grad()``, or
    when nothing requires grad, the launch and the bits are the same and nothing is saved."""
    r, m = _planes(render, mask)
    cm, cc, cam = _camera(cam_m, cam_c, camera_idx, r.device)
    want = torch.is_grad_enabled() and any(t.requires_grad for t in (r, m, cm, cc))
    return _CameraImage.apply(r, m, cm, cc, cam, want)


def frame_bytes(render, mask, cam_m=None, cam_c=None, camera_idx=None, white_bkgd=False):
    """train_material_params.py:865-870: ``(clamp((render * exp(m) + c) * mask (+ 1 - mask), 0, 1) * 255.)`` truncated to uint8
    [H, W, 3], the array the reference hands to ``Image.fromarray``, in one launch.  cam_m = cam_c = None: the identity, so
    ``frame_bytes(gt_rgb, gt_msk, None, None, None, white_bkgd)`` is the ground-truth frame of :847-849 and :874.  No graph."""
    r, m = _planes(render.detach(), mask.detach())
    _, H, W = r.shape
    if cam_m is None and cam_c is None:
        if camera_idx is not None:
            raise RuntimeError("camera_idx without cam_m and cam_c")
        cm = cc = None
        n_cam = cam = 0
    elif cam_m is None or cam_c is None:
        raise RuntimeError("cam_m and cam_c are given together or not at all")
    else:
        cm, cc, cam = _camera(cam_m.detach(), cam_c.detach(), camera_idx, r.device)
        n_cam = cm.shape[0]
    out = torch.empty((H, W, 3), dtype=torch.uint8, device=r.device)
    call("mpmhip_image_head_bytes", r.device, r.data_ptr(), m.data_ptr(), ptr(cm), ptr(cc), n_cam, cam, int(bool(white_bkgd)), H, W,
         out.data_ptr())
    return out


def compose_gt(rgb, msk, white_bkgd=False):
    """train_appearance.py:108-110: ``rgb * msk`` plus ``1 - msk`` on a white background, float [3, H, W], not clipped, in one
    launch.  No graph."""
    r, m = _planes(rgb.detach(), msk.detach(), ("rgb", "msk"))
    _, H, W = r.shape
    out = torch.empty_like(r)
    call("mpmhip_image_compose", r.device, r.data_ptr(), m.data_ptr(), int(bool(white_bkgd)), H, W, out.data_ptr())
    return out


def eval_inputs(pred_u8, gt_u8, mask, remove_white=False):
    """eval.py:68-87 in one launch: the two uint8 [H, W, 3] frames and the float [H, W] mask (``eval_mask`` of the data set's
    mask) -> ``(img_pred, img_gt)``, each float [1, 3, H, W], ready for ``AppEval.add_frame(img_pred, img_gt)``.  Bytes become
    floats by a true fp32 division by 255; with remove_white (the actorshq branch, :73-76) a pixel whose three bytes sum to
    >= 689 -- for bytes exactly ``mean(axis=0) > 0.90`` -- is zero in that image, each image on its own; both are then
    multiplied by the mask."""
    expect(pred_u8, torch.uint8, "pred_u8", contiguous=False)
    expect(gt_u8, torch.uint8, "gt_u8", contiguous=False)
    if pred_u8.dim() != 3 or pred_u8.shape[2] != 3 or pred_u8.numel() == 0 or gt_u8.shape != pred_u8.shape:
        raise RuntimeError(f"pred_u8 and gt_u8: expected two non-empty [H, W, 3] tensors, got {tuple(pred_u8.shape)} and {tuple(gt_u8.shape)}")
    H, W = pred_u8.shape[:2]
    expect(mask, torch.float32, "mask", shape=(H, W), contiguous=False)
    if not (pred_u8.device == gt_u8.device == mask.device):
        raise RuntimeError("pred_u8, gt_u8 and mask must be on one device")
    if H * W > 2 ** 31 - 1:
        raise RuntimeError("more than 2^31 - 1 pixels")
    p, g, m = pred_u8.contiguous(), gt_u8.contiguous(), mask.detach().contiguous()
    out = torch.empty((2, 1, 3, H, W), dtype=torch.float32, device=p.device)
    call("mpmhip_eval_pair", p.device, p.data_ptr(), g.data_ptr(), m.data_ptr(), int(bool(remove_white)), H, W, out[0].data_ptr(),
         out[1].data_ptr())
    return out[0], out[1]


def eval_mask(mask):
    """eval.py:81-84 without OpenCV, in torch operations on a float [H, W] mask (H, W >= 3), once per frame:
    ``cv2.erode(mask, np.ones((3, 3)), iterations=5)`` then ``cv2.GaussianBlur(mask, (5, 5), 0)``.  Five 3 x 3 erosions compose to
    one 11 x 11 minimum; OpenCV's default border for erode is a constant +inf, so pixels outside the image are ignored and the
    border itself never erodes: ``-max_pool2d(-m, 11, 1, 5)``, whose padding is -inf.  For a 5 x 5 kernel with sigma 0 OpenCV
    takes its fixed small kernel [1, 4, 6, 4, 1] / 16 per axis with BORDER_REFLECT_101, which is ``F.pad(mode="reflect")``.
    Equal to scipy.ndimage bit for bit in the erosion and within 1e-6 in the blur (tests/test_image_head_host.py).
    UNCONFIRMED against cv2: OpenCV is not available where this was written; the two statements about its defaults are from
    its documentation."""
    if not (isinstance(mask, torch.Tensor) and mask.dtype == torch.float32 and mask.dim() == 2 and min(mask.shape) >= 3):
        raise RuntimeError("mask: expected a torch.float32 [H, W] tensor with H, W >= 3")
    m = mask.detach()[None, None]
    m = -F.max_pool2d(-m, kernel_size=11, stride=1, padding=5)
    k = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], dtype=torch.float32, device=m.device) / 16.0
    m = F.conv2d(F.pad(m, (2, 2, 0, 0), mode="reflect"), k.view(1, 1, 1, 5))
    m = F.conv2d(F.pad(m, (0, 0, 2, 2), mode="reflect"), k.view(1, 1, 5, 1))
    return m[0, 0].contiguous()
