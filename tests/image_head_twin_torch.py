"""The image head as the reference writes it, in plain torch, at any dtype: the two lines of train_appearance.py:126-127 and the
frame of train_material_params.py:865-870 before its conversion to bytes.  Test infrastructure only: the float64 run of this file
under torch's autograd is the expected value of tests/test_image_head_host.py and tests/test_gpu_image_head.py."""
import torch


def unclipped(render, mask, cam_m, cam_c, camera_idx):
    """train_appearance.py:126 and the product of :127.  cam_m, cam_c [n_cam, 3] with an index, or [3] with None"""
    m = cam_m if camera_idx is None else cam_m[camera_idx]
    c = cam_c if camera_idx is None else cam_c[camera_idx]
    image = render * torch.exp(m)[:, None, None] + c[:, None, None]
    return image * mask


def camera_image(render, mask, cam_m, cam_c, camera_idx):
    return unclipped(render, mask, cam_m, cam_c, camera_idx).clip(0., 1.)


def frame(render, mask, cam_m, cam_c, camera_idx, white_bkgd):
    """train_material_params.py:865-870 up to the clamp, HWC; cam_m None: the ground-truth frame of :847-849 and :874"""
    r = render * mask if cam_m is None else unclipped(render, mask, cam_m, cam_c, camera_idx)
    if white_bkgd:
        r = r + (1.0 - mask)
    return torch.clamp(r.permute(1, 2, 0), 0., 1.)
