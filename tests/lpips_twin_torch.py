"""LPIPS (net_type 'vgg', version 0.1) in plain torch, the twin the tests compare against: F.conv2d, F.relu, F.max_pool2d and the
distance head over a dict of tensors under the reference's 33 state-dict keys.  It runs in whatever dtype its arguments have (float64
for the yardstick, float32 for the measurement of S32 and for the on-device comparison).  tests/test_lpips_host.py pins it against the
reference's own class (tests/golden/lpips.npz).  Test infrastructure only."""
import torch
import torch.nn.functional as F

CONV_AT = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)       # the convolutions of torchvision's vgg16().features[0:30]
POOL_AT = (4, 9, 16, 23)
TAP_AFTER = (3, 8, 15, 22, 29)                                   # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (target_layers - 1)
CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
            (512, 512), (512, 512), (512, 512))
TAP_CHANNELS = (64, 128, 256, 512, 512)
MEAN, STD = (-.030, -.088, -.188), (.458, .448, .450)


def state_shapes():
    """the reference's state_dict() in order -> [(key, shape)]"""
    out = [("net.mean", (1, 3, 1, 1)), ("net.std", (1, 3, 1, 1))]
    for at, (cin, cout) in zip(CONV_AT, CHANNELS):
        out += [(f"net.layers.{at}.weight", (cout, cin, 3, 3)), (f"net.layers.{at}.bias", (cout,))]
    return out + [(f"lin.{i}.1.weight", (1, c, 1, 1)) for i, c in enumerate(TAP_CHANNELS)]


def features(p, v):
    """the five tap maps of v [N, 3, H, W]"""
    v = (v - p["net.mean"]) / p["net.std"]
    taps = []
    for at in range(30):
        if at in CONV_AT:
            v = F.conv2d(v, p[f"net.layers.{at}.weight"], p[f"net.layers.{at}.bias"], padding=1)
        elif at in POOL_AT:
            v = F.max_pool2d(v, 2, 2)
        else:
            v = F.relu(v)
        if at in TAP_AFTER:
            taps.append(v)
    return taps


def forward(p, x, y):
    """-> [1, 1, 1, 1]: the sum over the five taps and over the batch"""
    res = []
    for i, (fx, fy) in enumerate(zip(features(p, x), features(p, y))):
        ux = fx / (torch.sqrt(torch.sum(fx ** 2, dim=1, keepdim=True)) + 1e-10)
        uy = fy / (torch.sqrt(torch.sum(fy ** 2, dim=1, keepdim=True)) + 1e-10)
        res.append(F.conv2d((ux - uy) ** 2, p[f"lin.{i}.1.weight"]).mean((2, 3), True))
    return torch.sum(torch.cat(res, 0), 0, True)
