"""The shadow network (scene/shadow.py:14-181 over scene/network.py) as a functional restatement in torch ops, usable with any dtype:
the yardstick of tests/test_shadow_host.py and tests/test_gpu_shadow_net.py in float64, and the measurement of S32 in float32.  Test
infrastructure only.  Parameters are an ordered {name: tensor} in the reference's named_parameters() order (param_names)."""
import torch
import torch.nn.functional as F


def conv_names():
    return [f"enc_layers.{i}.0" for i in range(4)] + [f"dec_layers.{j}.0" for j in range(4)] + ["shadow_pred"]


def channels(c, layer):
    return (1 if layer == 0 else 2 * c if 5 <= layer <= 7 else c), (1 if layer == 8 else c)


def param_shapes(shadow_size, n_dims, biases):
    """[(name, shape)] in the reference's named_parameters() order: bias, weight_g, weight_v per convolution"""
    sizes = [shadow_size // 2 ** i for i in range(4)]
    out = []
    for layer, conv in enumerate(conv_names()):
        cin, cout = channels(n_dims, layer)
        size = sizes[layer] if layer < 4 else sizes[7 - layer] if layer < 8 else shadow_size
        out.append((conv + ".bias", (1,) if layer == 8 and not biases else (cout, size, size)))
        out.append((conv + ".weight_g", (cout, 1, 1, 1)))
        out.append((conv + ".weight_v", (cout, cin, 3, 3)))
    return out


def weight(v, g):
    """weight norm with g_dim = 0 and v_dim = None: ONE norm over the whole of v"""
    return v * (g / torch.linalg.vector_norm(v))


def conv(p, name, x, slope=None):
    y = F.conv2d(x, weight(p[name + ".weight_v"], p[name + ".weight_g"]), None, 1, 1)
    b = p[name + ".bias"]
    y = y + (b.reshape(1, 1, 1, 1) if b.dim() == 1 else b[None])
    return y if slope is None else F.leaky_relu(y, slope)


def forward(p, ao_map, ao_mean, shadow_size, uv_size, slope=0.2, beta=1.0):
    """ao_map [N, 1, h, w], ao_mean [1, hm, wm] -> (shadow_map [N, 1, U, U], lowres [N, 1, S, S], resized ao_map)"""
    s = shadow_size
    mean = F.interpolate(ao_mean[None], size=(s, s))[0]
    if tuple(ao_map.shape[-2:]) != (s, s):
        ao_map = F.interpolate(ao_map, size=(s, s))
    x = ao_map - mean
    skips = []
    for i in range(4):
        x = conv(p, f"enc_layers.{i}.0", x, slope)
        skips.append(x)
        if i < 3:
            x = F.interpolate(x, size=(x.shape[-1] // 2,) * 2, mode="bilinear", align_corners=True)
    for j in range(4):
        if j > 0:
            skip = skips[3 - j]
            x = torch.cat([F.interpolate(x, size=skip.shape[2:4], mode="bilinear", align_corners=True), skip], dim=1)
        x = conv(p, f"dec_layers.{j}.0", x, slope)
    low = torch.sigmoid(conv(p, "shadow_pred", x) + beta)
    return F.interpolate(low, (uv_size, uv_size), mode="bilinear", align_corners=False), low, ao_map
