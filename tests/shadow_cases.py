"""Cases, yardstick and helpers shared by tests/test_shadow_host.py, tests/test_shadow_abi.py and tests/test_gpu_shadow_net.py.  Test
infrastructure only.

  case    shadow_size  levels         uv_size  input  n_dims  biases  N   what it exercises
  odd     20           20,10,5,2      24       33     4       False   1   an odd level, floor, a 2 x 2 map where every tap meets padding, the
                                                                         nearest resize (of ao_mean too), a non-integer final upsample
  tiles   40           40,20,10,5     40       40     8       True    3   tile seams and partial tiles, identity resize, untied head bias, batch sum
  shrink  16           16,8,4,2       12       16     4       False   1   the final downsample
  tiny    9            9,4,2,1        9        9      4       False   1   a 1 x 1 level, the out == 1 rule
  ref     256          256,128,64,32  256      256    4       False   1   the reference's construction (scene/mesh_gaussian_model.py:113-120)

Parameters are seeded, not the constructor's: weight_v ~ N(0, 1), weight_g ~ U(0.5, 2.5), biases ~ 0.3 N(0, 1); at its own
initialisation the map is flat and pins nothing.  The loss of a case is sum(w * shadow_map); its gradients go to every parameter.  The
yardstick is the float64 run of tests/shadow_twin_torch.py on the float32 inputs.  tests/golden/shadow_net.npz holds the reference's
own results on the four small cases (tests/golden/make_golden_shadow.py reads the inputs from here)."""
import ctypes as C
import functools

import numpy as np
import torch

import hostbuild
import shadow_twin_torch as tw
from mpmavatar_amd import _lib as L

#         S    U    input  C  biases  N  seed
_SHAPES = {"odd": (20, 24, 33, 4, False, 1, 0), "tiles": (40, 40, 40, 8, True, 3, 1), "shrink": (16, 12, 16, 4, False, 1, 2),
           "tiny": (9, 9, 9, 4, False, 1, 3), "ref": (256, 256, 256, 4, False, 1, 4)}
CASES = tuple(_SHAPES)
SMALL = CASES[:4]
OUTPUTS = ("shadow_map", "shadow_map_lowres", "ao_map")
SLOPE, BETA = 0.2, 1.0

# Measured on the CPU (tests/test_shadow_host.py::test_s32_is_the_measurement asserts that no figure it sees is above these): per case,
# the worst over the three outputs and every parameter gradient of max |t32 - t64| / max |t64| of the TWIN, its float32 run against
# its float64 run.  The code under test plays no part in it.  Host restatement and GPU must lie within BOUND = 10 * S32 of the float64
# twin, the project's margin (shade_cases.py, reg_cases.py): FMA contraction, the device's division and exp, and our own summation order
# of dW over up to 65,536 pixels.  torch's float32 convolution sums a batch in an order that depends on the number of threads, so the
# measurement is taken twice, with the threads torch starts with and with one, and the larger figure counts; each constant is that
# figure rounded up by about a quarter, since another CPU may pick another algorithm.
# measured here: odd 1.628e-6 (enc_layers.2.0.weight_g), tiles 1.443e-6 and 2.232e-6 on one thread (enc_layers.1.0.weight_v), shrink
# 3.382e-6 (enc_layers.1.0.weight_g), tiny 4.512e-7 (dec_layers.3.0.weight_g), ref 2.444e-5 (enc_layers.1.0.weight_g); only `tiles`,
# the one batch, differs between the two
S32 = {"odd": 2.1e-6, "tiles": 2.8e-6, "shrink": 4.3e-6, "tiny": 5.7e-7, "ref": 3.1e-5}
BOUND = {k: 10 * v for k, v in S32.items()}


def fixture_stride(numel):
    """tests/golden/shadow_net.npz stores a gradient flattened, at every eighth element where it has more than 2,048"""
    return 8 if numel > 2048 else 1


def shape(name):
    s, u, size_in, c, biases, n, _ = _SHAPES[name]
    return dict(shadow_size=s, uv_size=u, input=size_in, n_dims=c, biases=biases, n=n)


def names(name):
    s, _, _, c, biases, _, _ = _SHAPES[name]
    return [k for k, _ in tw.param_shapes(s, c, biases)]


@functools.lru_cache(maxsize=None)
def case(name):
    """dict of read-only float32 arrays: ao_map [N, 1, h, w], ao_mean [1, h, w] (at the input's size: the constructor resizes it),
    w [N, 1, U, U] and every parameter under its name"""
    s, u, size_in, c, biases, n, seed = _SHAPES[name]
    rng = np.random.default_rng(seed)
    out = {"ao_map": rng.uniform(0, 1, (n, 1, size_in, size_in)), "ao_mean": rng.uniform(0.3, 0.7, (1, size_in, size_in)),
           "w": rng.normal(size=(n, 1, u, u))}
    for k, shp in tw.param_shapes(s, c, biases):
        out[k] = rng.normal(size=shp) if k.endswith("weight_v") else rng.uniform(0.5, 2.5, shp) if k.endswith("weight_g") \
            else 0.3 * rng.normal(size=shp)
    out = {k: v.astype(np.float32) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def rel(t, t64):
    """max |t - t64| / max |t64| over EVERY element; a tensor that is all zero in float64 must be all zero"""
    t, t64 = np.asarray(t, np.float64), np.asarray(t64, np.float64)
    assert t.shape == t64.shape, (t.shape, t64.shape)
    top = np.abs(t64).max()
    if top == 0.0:
        assert (t == 0).all()
        return 0.0
    return float(np.abs(t - t64).max() / top)


def twin(name, dtype=torch.float64, c=None):
    """the twin's three outputs and the gradients of sum(w * shadow_map) to every parameter in `dtype` -> {name: numpy}"""
    c = case(name) if c is None else c
    sh = shape(name)
    p = {k: torch.tensor(np.asarray(c[k]), dtype=dtype, requires_grad=True) for k in names(name)}
    f = lambda k: torch.tensor(np.asarray(c[k]), dtype=dtype)
    smap, low, ao = tw.forward(p, f("ao_map"), f("ao_mean"), sh["shadow_size"], sh["uv_size"], SLOPE, BETA)
    grads = torch.autograd.grad((f("w") * smap).sum(), list(p.values()))
    out = {"shadow_map": smap.detach().numpy(), "shadow_map_lowres": low.detach().numpy(), "ao_map": ao.detach().numpy()}
    out.update({k: g.numpy() for k, g in zip(p, grads)})
    return out


@functools.lru_cache(maxsize=None)
def t64(name):
    """the float64 twin of a case, computed once and shared"""
    out = twin(name)
    for v in out.values():
        v.setflags(write=False)
    return out


def report(name, got, want, bound, label):
    """every figure printed, then the worst asserted"""
    worst = 0.0
    for k in want:
        err = rel(got[k], want[k])
        worst = max(worst, err)
        print(name, label, k, "%.3g of bound %.3g" % (err, bound))
        assert np.isfinite(np.asarray(got[k])).all() and err <= bound, (name, k, err, bound)
    return worst


# ---- the host build of shadow_math.hpp -----------------------------------------------------------------------------------------------

def host_lib():
    lib = hostbuild.host_lib("hostshadow")
    lib.hsn_table_words.restype = lib.hsn_workspace_words.restype = C.c_int64
    return lib


def sanitizer_program():
    """the same file as a stand-alone program under AddressSanitizer and UBSan (run as a subprocess; nothing is loaded into Python)"""
    return hostbuild.host_program("hostshadow", name="hostshadow_asan",
                                  flags=["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DHOSTSHADOW_MAIN"])


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_tables(in_h, in_w, s, u):
    lib = host_lib()
    words = np.zeros(lib.hsn_table_words(s, u), np.int32)
    lib.hsn_fill_tables(_p(words), in_h, in_w, s, u)
    return words


def split_tables(words, s, u):
    """the blob of csrc/shadow_math.hpp -> {"ny", "nx", "down0".."down2", "up0".."up2", "fin"}, a resampling being a dict of
    in, out, i0, i1, l1, inv_start, inv_dst, inv_w"""
    out, at = {"ny": words[:s], "nx": words[s:2 * s]}, 2 * s
    level = lambda i: s >> i
    pairs = [("down%d" % i, level(i), level(i + 1)) for i in range(3)] + [("up%d" % k, level(3 - k), level(2 - k)) for k in range(3)]
    for key, n_in, n_out in pairs + [("fin", s, u)]:
        w = words[at:at + 7 * n_out + n_in + 1]
        at += w.size
        out[key] = {"in": n_in, "out": n_out, "i0": w[:n_out], "i1": w[n_out:2 * n_out], "l1": w[2 * n_out:3 * n_out].view(np.float32),
                    "inv_start": w[3 * n_out:3 * n_out + n_in + 1], "inv_dst": w[3 * n_out + n_in + 1:5 * n_out + n_in + 1],
                    "inv_w": w[5 * n_out + n_in + 1:].view(np.float32)}
    assert at == words.size
    return out


def host_run(name, frozen=()):
    """forward and backward on the host -> {name: numpy} like twin(); parameters named in `frozen` get no gradient (None)"""
    c, sh, lib = case(name), shape(name), host_lib()
    s, u, n, cdim = sh["shadow_size"], sh["uv_size"], sh["n"], sh["n_dims"]
    h, w = c["ao_map"].shape[-2:]
    mean = torch.nn.functional.interpolate(torch.tensor(c["ao_mean"])[None], size=(s, s))[0].numpy().copy()
    tables = host_tables(h, w, s, u)
    keep = [tables, mean]
    d = L.ShadowDesc()
    d.n, d.in_h, d.in_w, d.shadow_size, d.uv_size, d.n_dims, d.untied_head_bias = n, h, w, s, u, cdim, int(sh["biases"])
    d.lrelu_slope, d.beta, d.ao_mean, d.tables = SLOPE, BETA, mean.ctypes.data, tables.ctypes.data
    grads = {}
    for i, k in enumerate(names(name)):
        a = np.ascontiguousarray(c[k])
        g = None if k in frozen else np.full(a.shape, np.nan, np.float32)
        keep.append(a)
        grads[k] = g
        kind = {"bias": "bias", "weight_g": "weight_g", "weight_v": "weight_v"}[k.rsplit(".", 1)[1]]
        getattr(d, kind)[i // 3] = a.ctypes.data
        getattr(d, "d_" + kind)[i // 3] = None if g is None else g.ctypes.data
    ws = np.zeros(lib.hsn_workspace_words(n, s, cdim), np.float32)
    ao = np.ascontiguousarray(c["ao_map"]).reshape(n, h, w)
    out = {"shadow_map": np.full((n, 1, u, u), np.nan, np.float32), "shadow_map_lowres": np.full((n, 1, s, s), np.nan, np.float32),
           "ao_map": np.full((n, 1, s, s), np.nan, np.float32)}
    lib.hsn_forward(C.byref(d), _p(ao), _p(ws), _p(out["ao_map"]), _p(out["shadow_map_lowres"]), _p(out["shadow_map"]))
    lib.hsn_backward(C.byref(d), _p(ao), _p(out["shadow_map_lowres"]), _p(np.ascontiguousarray(c["w"])), None, _p(ws))
    out.update(grads)
    return out
