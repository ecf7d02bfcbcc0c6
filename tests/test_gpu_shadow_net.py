"""The shadow network on the GPU: mpmavatar_amd.shadow_net.ShadowUNet under torch autograd (csrc/shadow.hip) against the float64 twin
(tests/shadow_twin_torch.py) within BOUND = 10 * S32 per case (tests/shadow_cases.py, measured on the CPU), and the properties the
module promises: the same bits on every run, the graph rules, the input forms, the state dict, the batch, the chain into
shaded_colors, and the optimiser.  Every comparison prints its figures before it asserts (-s)."""
import numpy as np
import pytest
import torch

import adam_cases as ac
import shade_cases as shc
import shade_twin_torch as shtw
import shadow_cases as sc
import shadow_twin_torch as tw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _net(name, c=None):
    """the module of a case with the case's parameters, on the GPU"""
    from mpmavatar_amd.shadow_net import ShadowUNet
    c, sh = sc.case(name) if c is None else c, sc.shape(name)
    net = ShadowUNet(uv_size=sh["uv_size"], ao_mean=torch.tensor(c["ao_mean"]), shadow_size=sh["shadow_size"], lrelu_slope=sc.SLOPE,
                     beta=sc.BETA, n_dims=sh["n_dims"], interp_mode="bilinear", biases=sh["biases"])
    assert [(k, tuple(p.shape)) for k, p in net.named_parameters()] == tw.param_shapes(sh["shadow_size"], sh["n_dims"], sh["biases"])
    with torch.no_grad():
        for k, p in net.named_parameters():
            p.copy_(torch.tensor(c[k]))
    return net.to(DEV)


def _run(name, net=None, ao=None, w=None):
    """-> {name: numpy} like shadow_cases.twin(): the three outputs and the gradient of every parameter (None where it got none)"""
    c = sc.case(name)
    net = _net(name) if net is None else net
    net.zero_grad(set_to_none=True)
    res = net(torch.tensor(c["ao_map"], device=DEV) if ao is None else ao)
    (torch.tensor(c["w"] if w is None else w, device=DEV) * res["shadow_map"]).sum().backward()
    out = {k: res[k].detach().cpu().numpy() for k in sc.OUTPUTS}
    out.update({k: (None if p.grad is None else p.grad.cpu().numpy()) for k, p in net.named_parameters()})
    return out, res


# ---- 1. every case against the twin ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.CASES)
def test_against_the_twin(name):
    got, res = _run(name)
    sh = sc.shape(name)
    assert res["shadow_map"].grad_fn is not None and res["shadow_map"].shape == (sh["n"], 1, sh["uv_size"], sh["uv_size"])
    assert res["shadow_map_lowres"].shape == (sh["n"], 1, sh["shadow_size"], sh["shadow_size"])
    sc.report(name, got, sc.t64(name), sc.BOUND[name], "gpu")


# ---- 2. the same bits on two runs ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tiles", "ref"])
def test_two_runs_give_the_same_bits(name):
    net = _net(name)
    a, _ = _run(name, net)
    b, _ = _run(name, net)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- 3. the graph rules ------------------------------------------------------------------------------------------------------------------

def test_grad_mode_frozen_parameters_and_refusals():
    from mpmavatar_amd.shadow_net import ShadowUNet
    name = "odd"
    c, net = sc.case(name), _net(name)
    ao = torch.tensor(c["ao_map"], device=DEV)
    base, _ = _run(name, net)
    with torch.no_grad():
        quiet = net(ao)
    assert all(quiet[k].grad_fn is None for k in sc.OUTPUTS)
    for k in sc.OUTPUTS:
        assert np.array_equal(quiet[k].cpu().numpy(), base[k]), k
    frozen = ("enc_layers.0.0.weight_v", "enc_layers.0.0.weight_g", "enc_layers.2.0.bias", "dec_layers.1.0.weight_g", "shadow_pred.bias",
              "shadow_pred.weight_v")
    for k, p in net.named_parameters():
        p.requires_grad_(k not in frozen)
    part, _ = _run(name, net)
    for k in sc.names(name):
        if k in frozen:
            assert part[k] is None, k
        else:
            assert np.array_equal(part[k], base[k]), k
    for p in net.parameters():
        p.requires_grad_(False)
    assert net(ao)["shadow_map"].grad_fn is None                                   # nothing requires grad: no graph
    with pytest.raises(RuntimeError, match="ao_map"):
        net(ao.clone().requires_grad_(True))
    mean = torch.tensor(c["ao_mean"])
    for bad, word in [(dict(n_dims=64), "n_dims"), (dict(n_dims=5), "n_dims"), (dict(shadow_size=7), "shadow_size"), (dict(uv_size=0), "uv_size"),
                      (dict(interp_mode="nearest"), "interp_mode"), (dict(trainable_mean=True), "trainable_mean"), (dict(lrelu_slope=-0.1), "lrelu_slope")]:
        args = dict(uv_size=24, ao_mean=mean, shadow_size=20, n_dims=4)
        args.update(bad)
        with pytest.raises(ValueError, match=word):
            ShadowUNet(**args)
    with pytest.raises(RuntimeError):
        net(torch.tensor(c["ao_map"]))                                              # no CPU fallback


# ---- 4. the identity resize and the input forms ----------------------------------------------------------------------------------------

def test_identity_resize_and_input_forms():
    name = "tiny"                                                                   # U == S, N == 1
    c, net = sc.case(name), _net(name)
    base, res = _run(name, net)
    assert np.array_equal(base["shadow_map"], base["shadow_map_lowres"])
    ao4 = torch.tensor(c["ao_map"], device=DEV)
    assert np.array_equal(base["ao_map"], c["ao_map"])
    for ao in (ao4[0, 0], ao4[0], ao4):
        got, r = _run(name, net, ao=ao)
        assert r["shadow_map"].shape == (1, 1, 9, 9) and r["ao_map"] is ao           # not resized: the input itself
        for k in base:
            if k != "ao_map":
                assert np.array_equal(got[k], base[k]), (tuple(ao.shape), k)
    got, _ = _run("odd", ao=torch.tensor(sc.case("odd")["ao_map"], device=DEV)[0])   # [1, h, w] with the nearest resize, as the reference is called
    want, _ = _run("odd")
    for k in want:
        assert np.array_equal(got[k], want[k]), k


# ---- 5. the state dict and the batch ---------------------------------------------------------------------------------------------------

def test_state_dict_round_trip_and_batch():
    from mpmavatar_amd.shadow_net import ShadowUNet
    name = "tiles"
    c, sh, net = sc.case(name), sc.shape(name), _net(name)
    g = np.load(sc.__file__.replace("shadow_cases.py", "golden/shadow_net.npz"))
    state = net.state_dict()
    assert [k for k in state if k != "ao_mean"] == list(g[f"{name}/names"]) and "ao_mean" in state
    other = ShadowUNet(uv_size=sh["uv_size"], ao_mean=torch.zeros(1, 40, 40), shadow_size=sh["shadow_size"], n_dims=sh["n_dims"],
                       biases=sh["biases"]).to(DEV)
    other.load_state_dict({k: v.cpu() for k, v in state.items()})
    base, _ = _run(name, net)
    again, _ = _run(name, other)
    for k in base:
        assert np.array_equal(again[k], base[k]), k
    total = None
    for n in range(sh["n"]):
        one, r = _run(name, net, ao=torch.tensor(c["ao_map"][n:n + 1], device=DEV), w=c["w"][n:n + 1])
        for k in ("shadow_map", "shadow_map_lowres"):
            assert np.array_equal(one[k][0], base[k][n]), (n, k)                    # a map does not depend on its neighbours in the batch
        total = {k: one[k].astype(np.float64) for k in sc.names(name)} if total is None else {k: total[k] + one[k] for k in total}
    for k in sc.names(name):
        err = sc.rel(base[k], total[k])
        print(k, "batch of three against three calls %.3g of bound %.3g" % (err, sc.BOUND[name]))
        assert err <= sc.BOUND[name], k


# ---- 6. the chain into the colours -------------------------------------------------------------------------------------------------------

def test_chain_into_shaded_colors():
    """ShadowUNet -> shaded_colors -> (w . colors).sum().backward() on shade_cases `main` (a 5 x 7 map does not fit a square network,
    so the network's 9 x 9 map of `tiny` is sampled by the faces of `main`) against the two twins composed"""
    from mpmavatar_amd.shading import ShadowSampler, shaded_colors
    name, deg = "tiny", 3
    c, m, sh = sc.case(name), shc.case("main"), sc.shape(name)
    net = _net(name)
    leaves = {k: torch.tensor(np.asarray(m[k]), device=DEV).requires_grad_(True) for k in ("features_dc", "features_rest", "means3D")}
    sampler = ShadowSampler(torch.tensor(m["face_uv"], device=DEV)[None, None], 9, 9)
    smap = net(torch.tensor(c["ao_map"], device=DEV)[0])["shadow_map"]
    colors = shaded_colors(leaves["features_dc"], leaves["features_rest"], deg, leaves["means3D"], torch.tensor(m["campos"], device=DEV),
                           binding=torch.tensor(m["binding"], device=DEV), shadow_map=smap, sampler=sampler)
    (torch.tensor(m["w"], device=DEV) * colors).sum().backward()
    f = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    p = {k: f(c[k]).requires_grad_(True) for k in sc.names(name)}
    t = {k: f(m[k]).requires_grad_(True) for k in leaves}
    smap64 = tw.forward(p, f(c["ao_map"]), f(c["ao_mean"]), sh["shadow_size"], sh["uv_size"], sc.SLOPE, sc.BETA)[0]
    colors64 = shtw.shaded(deg, t["features_dc"], t["features_rest"], t["means3D"], f(m["campos"]), smap64[0, 0], f(m["face_uv"]),
                           torch.from_numpy(m["binding"].astype(np.int64)))
    (f(m["w"]) * colors64).sum().backward()
    bound = sc.BOUND[name] + shc.BOUND
    got = {"colors": colors.detach().cpu().numpy(), **{k: v.grad.cpu().numpy() for k, v in leaves.items()},
           **{k: q.grad.cpu().numpy() for k, q in net.named_parameters()}}
    want = {"colors": colors64.detach().numpy(), **{k: v.grad.numpy() for k, v in t.items()}, **{k: v.grad.numpy() for k, v in p.items()}}
    sc.report("tiny -> main", got, want, bound, "chain")


# ---- 7. the optimiser ------------------------------------------------------------------------------------------------------------------

def test_parameters_go_into_the_fused_optimiser():
    from mpmavatar_amd.optim import FusedAdam, appearance_param_groups
    name = "odd"
    net = _net(name)
    z = lambda *s: torch.zeros(*s, device=DEV, requires_grad=True)
    groups = appearance_param_groups(z(4, 3), z(4, 1, 3), z(4, 15, 3), z(4, 1), z(4, 3), z(4, 4), z(5, 3), [z(3), z(3)], net.parameters(),
                                     ac.OPT, spatial_lr_scale=1.0)
    assert [id(p) for p in groups[-1]["params"]] == [id(p) for p in net.parameters()] and len(groups[-1]["params"]) == 27
    opt = FusedAdam(groups, lr=0.0, eps=1e-15)
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    _run(name, net)
    opt.step()
    for k, p in net.named_parameters():
        moved, hit = p != before[k], p.grad != 0                                    # Adam moves every element with a non-zero gradient
        assert bool(torch.isfinite(p).all()) and bool(hit.any()) and bool(moved[hit].all()), k
