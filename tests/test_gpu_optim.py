"""The optimiser step on the GPU: mpmavatar_amd.optim.FusedAdam (csrc/adam.hip) against the float64 twin
(tests/adam_twin_torch.py) within BOUND = 10 * S32 per class (tests/adam_cases.py, measured on the CPU), and what the module
promises: the same bits on every run, every shape at which the kernel takes another path, the semantics of torch.optim.Adam (a
missing gradient, a changed rate, lr == 0, a late group, the unsupported options), the state_dict both ways, the hand-over through a
densification, and the example.  Every comparison prints its figures before it asserts (-s)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import adam_cases as ac
import adam_twin_torch as tw
import densify_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _leaves(arrays):
    return {k: torch.nn.Parameter(torch.tensor(np.asarray(v), device=DEV)) for k, v in arrays.items()}


def _fused(groups=None, cls=None):
    """the base case's nine groups on the GPU under FusedAdam (or cls) -> (optimizer, {tensor name: Parameter})"""
    from mpmavatar_amd.optim import FusedAdam
    leaves, out = {}, []
    for g in groups or ac.groups():
        ps = _leaves(g["params"])
        leaves.update(ps)
        out.append({**{k: v for k, v in g.items() if k != "params"}, "params": list(ps.values())})
    return (cls or FusedAdam)(out, lr=0.0, eps=1e-15), leaves


def _step(opt, leaves, grads, iteration=None):
    from mpmavatar_amd.optim import update_learning_rate
    if iteration is not None:
        update_learning_rate(opt, iteration)
    for k, p in leaves.items():
        g = grads.get(k)
        p.grad = None if g is None else torch.tensor(np.asarray(g), device=DEV)
    opt.step()


def _result(opt, leaves):
    out = {}
    for k, p in leaves.items():
        st = opt.state.get(p, {})
        out["p_" + k] = p.detach().cpu().numpy()
        out["m_" + k] = st["exp_avg"].cpu().numpy() if st else np.zeros(p.shape, np.float32)
        out["v_" + k] = st["exp_avg_sq"].cpu().numpy() if st else np.zeros(p.shape, np.float32)
    return out


def _run(k_steps):
    opt, leaves = _fused()
    for k in range(1, k_steps + 1):
        _step(opt, leaves, ac.grads(k), ac.iteration(k))
    return _result(opt, leaves), opt, leaves


def _within(got, want, label, tensors=None):
    for c in ac.CLASSES:
        worst = max((ac.rel(got[f"{c}_{k}"], want[f"{c}_{k}"]), k) for k in (tensors or ac.TENSORS))
        print("%s %s: %.3g (%s) of bound %.3g" % (label, c, *worst, ac.BOUND[c]))
        assert np.isfinite(worst[0]) and worst[0] <= ac.BOUND[c], (label, c, worst)


# ---- 1. every case against the twin; 2. the same bits twice ---------------------------------------------------------------------------

@pytest.mark.parametrize("k_steps", ac.K_STEPS)
def test_every_case_against_the_twin(k_steps):
    got, opt, leaves = _run(k_steps)
    _within(got, ac.twin64(k_steps), "K = %d" % k_steps)
    for p in leaves.values():
        st = opt.state[p]
        assert st["step"].dtype == torch.float32 and st["step"].device.type == "cpu" and float(st["step"]) == k_steps
    host = ac.host_run(k_steps)
    same = {k: np.array_equal(got[k], host[k]) for k in got}
    print("K = %d: GPU and host restatement agree bit for bit in %d of %d tensors%s" % (
        k_steps, sum(same.values()), len(same), "" if all(same.values()) else "; not in " + ", ".join(k for k, v in same.items() if not v)))


def test_the_same_bits_on_two_runs():
    a, b = _run(25)[0], _run(25)[0]
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- 3. shapes where the kernel can go wrong ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ac.shape_lists(4096, 48)))
def test_shapes(name):
    """element counts around the vector width and the chunk, each of p, g, m, v in turn a view one float into a larger buffer (the
    all-scalar path), and more tensors than one launch holds; the floats either side of every tensor keep their bits"""
    from mpmavatar_amd.optim import ADAM_CHUNK, MAX_TENSORS, FusedAdam, adam_scalars
    counts, offsets = ac.shape_lists(ADAM_CHUNK, MAX_TENSORS)[name]
    rng = np.random.default_rng(5)
    bufs, views, rows = [], [], []
    for i, n in enumerate(counts):
        host = [rng.normal(0, 1, n + 8).astype(np.float32) for _ in range(4)]
        host[3] = np.abs(host[3])
        dev = [torch.tensor(h, device=DEV) for h in host]
        off = [4 + (1 if offsets is not None and offsets[i] == j else 0) for j in range(4)]          # 4: a 16-byte aligned interior
        view = [d[o:o + n] for d, o in zip(dev, off)]
        assert all((v.data_ptr() % 16 == 0) == (o == 4) for v, o in zip(view, off) if n)
        bufs.append((host, dev, off))
        views.append(view)
        rows.append(tuple(h[o:o + n].copy() for h, o in zip(host, off)) + (adam_scalars(1e-2, (0.9, 0.999), 1e-15, 3.0), True))
    params = [torch.nn.Parameter(v[0]) for v in views]
    opt = FusedAdam(params, lr=1e-2, eps=1e-15)
    for p, v in zip(params, views):
        p.grad = v[1]
        opt.state[p] = {"step": torch.tensor(2.0), "exp_avg": v[2], "exp_avg_sq": v[3]}
    opt.step()
    torch.cuda.synchronize()
    for i, (n, (host, dev, off), row) in enumerate(zip(counts, bufs, rows)):
        assert float(opt.state[params[i]]["step"]) == 3.0
        want = ac.expected(row)
        for j, w64, c in ((0, want[0], "p"), (2, want[1], "m"), (3, want[2], "v")):
            got = dev[j].cpu().numpy()
            o = off[j]
            assert np.array_equal(got[:o], host[j][:o]) and np.array_equal(got[o + n:], host[j][o + n:]), (name, n, c, "wrote outside")
            assert ac.rel(got[o:o + n], w64) <= ac.BOUND[c], (name, n, c)
        assert np.array_equal(dev[1].cpu().numpy(), host[1])                                       # the gradient is read only


def test_more_chunks_than_workgroups():
    """one tensor of more chunks than the grid has workgroups, next to a small one: the stride takes every chunk once"""
    from mpmavatar_amd.optim import ADAM_CHUNK, FusedAdam
    n = (2048 + 37) * ADAM_CHUNK + 2
    g = torch.Generator(device=DEV).manual_seed(0)
    p = [torch.nn.Parameter(torch.randn(k, device=DEV, generator=g)) for k in (n, 5)]
    before = [x.detach().clone() for x in p]
    opt = FusedAdam(p, lr=1e-2, eps=1e-15)
    for x in p:
        x.grad = torch.randn(x.shape, device=DEV, generator=g) + 3.0                                # no gradient near zero
    opt.step()
    for x, b in zip(p, before):
        # the first step of Adam moves every element by lr * sign(g), up to rounding
        assert torch.allclose(x.detach() - b, -1e-2 * torch.sign(x.grad), rtol=0, atol=1e-6)
        assert torch.allclose(opt.state[x]["exp_avg"], 0.1 * x.grad, rtol=1e-6, atol=0)


# ---- 4. semantics ------------------------------------------------------------------------------------------------------------------

def test_a_missing_gradient_keeps_the_state_and_the_step_count():
    opt, leaves = _fused()
    t_opt, t_leaves = tw.make(ac.groups())
    for k in (1, 2, 3, 4):
        g = dict(ac.grads(k))
        if k == 2:
            g["_opacity"] = g["cam_c"] = None
        _step(opt, leaves, g, ac.iteration(k))
        tw.step(t_opt, t_leaves, g, ac.iteration(k))
        if k == 2:
            assert float(opt.state[leaves["_opacity"]]["step"]) == 1.0 and float(opt.state[leaves["_xyz"]]["step"]) == 2.0
    assert float(opt.state[leaves["_opacity"]]["step"]) == 3.0 == float(t_opt.state[t_leaves["_opacity"]]["step"])
    _within(_result(opt, leaves), tw.result(t_opt, t_leaves), "missing gradient")
    # a parameter that never had a gradient has no state
    opt, leaves = _fused()
    _step(opt, leaves, {k: v for k, v in ac.grads(1).items() if k != "cam_m"})
    assert leaves["cam_m"] not in opt.state or not opt.state[leaves["cam_m"]]
    assert np.array_equal(leaves["cam_m"].detach().cpu().numpy(), ac.params()["cam_m"])


def test_a_changed_rate_takes_effect_and_a_zero_rate_moves_the_moments_only():
    opt, leaves = _fused()
    t_opt, t_leaves = tw.make(ac.groups())
    for k, rate in ((1, 0.05), (2, np.float64(0.2)), (3, 0.0), (4, 0.01)):
        for o in (opt, t_opt):
            o.param_groups[3]["lr"] = rate                  # opacity
        before = leaves["_opacity"].detach().clone()
        m_before = None if k == 1 else opt.state[leaves["_opacity"]]["exp_avg"].clone()
        _step(opt, leaves, ac.grads(k))
        tw.step(t_opt, t_leaves, ac.grads(k))
        moved = not torch.equal(before, leaves["_opacity"].detach())
        assert moved == (rate != 0)
        if rate == 0:
            assert not torch.equal(m_before, opt.state[leaves["_opacity"]]["exp_avg"])
    _within(_result(opt, leaves), tw.result(t_opt, t_leaves), "changed rates")
    # f_rest, lr == 0 throughout: the parameter keeps its bits, NaN payloads included, which no read-modify-write would
    opt, leaves = _fused()
    with torch.no_grad():
        leaves["_features_rest"].view(-1)[::7] = float("nan")
    bits = leaves["_features_rest"].detach().view(torch.int32).clone()
    _step(opt, leaves, ac.grads(1))
    assert torch.equal(bits, leaves["_features_rest"].detach().view(torch.int32)) and opt.state[leaves["_features_rest"]]["exp_avg"].any()


def test_a_group_added_after_the_first_step():
    from mpmavatar_amd.optim import FusedAdam
    arrays = ac.params()
    first, late = _leaves({k: arrays[k] for k in ("_scaling", "cam_m")}), _leaves({"shadow3": arrays["shadow3"]})
    t_first = {k: torch.nn.Parameter(torch.tensor(arrays[k], dtype=torch.float64)) for k in first}
    t_late = {"shadow3": torch.nn.Parameter(torch.tensor(arrays["shadow3"], dtype=torch.float64))}
    opt = FusedAdam([{"params": list(first.values()), "lr": 5e-3}], lr=0.0, eps=1e-15)
    t_opt = torch.optim.Adam([{"params": list(t_first.values()), "lr": 5e-3}], lr=0.0, eps=1e-15, foreach=False)
    _step(opt, first, ac.grads(1))
    tw.step(t_opt, t_first, ac.grads(1))
    opt.add_param_group({"params": list(late.values()), "lr": 1e-4, "name": "shadow"})
    t_opt.add_param_group({"params": list(t_late.values()), "lr": 1e-4, "name": "shadow"})
    leaves, t_leaves = {**first, **late}, {**t_first, **t_late}
    for k in (2, 3):
        _step(opt, leaves, ac.grads(k))
        tw.step(t_opt, t_leaves, ac.grads(k))
    assert float(opt.state[late["shadow3"]]["step"]) == 2.0 and float(opt.state[first["cam_m"]]["step"]) == 3.0
    _within(_result(opt, leaves), tw.result(t_opt, t_leaves), "late group", tensors=list(leaves))
    with pytest.raises(ValueError):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3, device=DEV))], "weight_decay": 0.1})


def test_unsupported_options_and_tensors_raise_before_any_launch():
    from mpmavatar_amd.optim import FusedAdam
    p = lambda: torch.nn.Parameter(torch.ones(5, device=DEV))
    for kw in (dict(weight_decay=0.1), dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True)):
        with pytest.raises(ValueError):
            FusedAdam([p()], lr=1e-3, **kw)
    with pytest.raises(ValueError):
        FusedAdam([p()], lr=torch.tensor(1e-3))
    good = p()
    bad = {"cpu": torch.nn.Parameter(torch.ones(5)), "float64": torch.nn.Parameter(torch.ones(5, device=DEV, dtype=torch.float64)),
           "strided": torch.nn.Parameter(torch.ones(5, 4, device=DEV).t()), "float16": torch.nn.Parameter(torch.ones(5, device=DEV, dtype=torch.float16))}
    for label, q in bad.items():
        opt = FusedAdam([good, q], lr=1e-3)
        good.grad, q.grad = torch.ones_like(good), torch.ones_like(q)
        with pytest.raises(ValueError):
            opt.step()
        assert not opt.state and torch.equal(good.detach(), torch.ones(5, device=DEV)), label     # the good one, in front, was not touched
    for label, grad in (("sparse", torch.sparse_coo_tensor(torch.tensor([[1]]), torch.tensor([1.0]), (5,)).to(DEV)),):
        q = p()
        opt = FusedAdam([good, q], lr=1e-3)
        good.grad = torch.ones_like(good)
        q.grad = grad
        with pytest.raises(ValueError):
            opt.step()
        assert not opt.state and torch.equal(good.detach(), torch.ones(5, device=DEV)), label
    opt = FusedAdam([good], lr=1e-3)
    good.grad = torch.ones_like(good)
    with pytest.raises(ValueError):
        opt.step(lambda: 0.0)
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(ValueError):
        opt.step()
    assert not opt.state
    # a gradient that is not contiguous is taken contiguous; zero_grad is torch's
    opt = FusedAdam([good], lr=1e-3)
    good.grad = torch.ones(5, 2, device=DEV)[:, 0]
    assert not good.grad.is_contiguous()
    opt.step()
    assert torch.allclose(good.detach(), torch.full((5,), 1 - 1e-3, device=DEV))
    opt.zero_grad(set_to_none=True)
    assert good.grad is None


# ---- 5. interop --------------------------------------------------------------------------------------------------------------------

def test_state_dict_round_trips_with_torch_adam():
    ours, leaves = _fused()
    theirs, t_leaves = _fused(cls=lambda g, **kw: torch.optim.Adam(g, foreach=False, **kw))
    for k in (1, 2):
        _step(ours, leaves, ac.grads(k), ac.iteration(k))
        _step(theirs, t_leaves, ac.grads(k), ac.iteration(k))
    sd_ours, sd_theirs = ours.state_dict(), theirs.state_dict()
    assert set(sd_ours["param_groups"][0]) == set(sd_theirs["param_groups"][0])
    for a, b in zip(sd_ours["state"].values(), sd_theirs["state"].values()):
        assert set(a) == set(b) == {"step", "exp_avg", "exp_avg_sq"}
        assert all(a[k].dtype == b[k].dtype and a[k].device == b[k].device and a[k].shape == b[k].shape for k in a)
    # each loads the other's, and the next step of both agrees with the twin's third step
    ours2, leaves2 = _fused()
    theirs2, t_leaves2 = _fused(cls=lambda g, **kw: torch.optim.Adam(g, foreach=False, **kw))
    with torch.no_grad():
        for k in leaves:
            leaves2[k].copy_(t_leaves[k])
            t_leaves2[k].copy_(leaves[k])
    ours2.load_state_dict(sd_theirs)
    theirs2.load_state_dict(sd_ours)
    _step(ours2, leaves2, ac.grads(3), ac.iteration(3))
    _step(theirs2, t_leaves2, ac.grads(3), ac.iteration(3))
    assert float(ours2.state[leaves2["_xyz"]]["step"]) == 3.0 == float(theirs2.state[t_leaves2["_xyz"]]["step"])
    _within(_result(ours2, leaves2), ac.twin64(3), "ours from torch's state")
    _within(_result(theirs2, t_leaves2), ac.twin64(3), "torch from our state")


def test_hand_over_through_a_densification():
    """step -> densify_and_prune(moments=adam_moments(opt)) -> swap_into(opt) -> reset_opacity(..., opt) -> step, against the twin,
    to which the same src / kind gather and the zeroed opacity moments are applied in float64"""
    from mpmavatar_amd.densify import GROUPS, DensifyStats, adam_moments, densify_and_prune, reset_opacity
    from mpmavatar_amd.optim import FusedAdam
    c = dc.case("main")
    n, h = c["binding"].shape[0], c["hyper"]
    rates = {"_xyz": 1e-3, "_features_dc": 2.5e-3, "_features_rest": 0.0, "_opacity": 0.05, "_scaling": 5e-3, "_rotation": 1e-3}
    leaves = _leaves({k: c[k] for k in dc.PARAMS})
    extra = _leaves({"verts": np.ones((7, 3), np.float32)})
    t_leaves = {k: torch.nn.Parameter(torch.tensor(c[k], dtype=torch.float64)) for k in dc.PARAMS}
    t_extra = {"verts": torch.nn.Parameter(torch.ones(7, 3, dtype=torch.float64))}
    mk = lambda lv, ex: [{"params": [lv[k]], "lr": rates[k], "name": GROUPS[k]} for k in dc.PARAMS] + [{"params": [ex["verts"]], "lr": 1e-3, "name": "verts"}]
    opt = FusedAdam(mk(leaves, extra), lr=0.0, eps=1e-15)
    t_opt = torch.optim.Adam(mk(t_leaves, t_extra), lr=0.0, eps=1e-15, foreach=False)
    rng = np.random.default_rng(11)
    draw = lambda lv: {k: (10.0 ** rng.uniform(-6, 0, tuple(p.shape)) * rng.choice([-1.0, 1.0], tuple(p.shape))).astype(np.float32) for k, p in lv.items()}
    g1 = draw({**leaves, **extra})
    _step(opt, {**leaves, **extra}, g1)
    tw.step(t_opt, {**t_leaves, **t_extra}, g1)
    stats = DensifyStats(n, DEV)
    stats.xyz_gradient_accum, stats.denom = torch.tensor(c["accum"], device=DEV), torch.tensor(c["denom"], device=DEV)
    res = densify_and_prune(*[leaves[k].detach() for k in dc.PARAMS], torch.tensor(c["binding"], device=DEV), c["n_faces"],
                            torch.tensor(c["face_scaling"], device=DEV), stats, h["max_grad"], h["min_opacity"], h["extent"], h["max_screen_size"],
                            h["percent_dense"], moments=adam_moments(opt), noise=torch.tensor(c["noise"], device=DEV))
    new = res.swap_into(opt)
    new["_opacity"] = reset_opacity(new["_opacity"], opt)
    assert res.n_out != n and res.n_cloned > 0 and res.n_split > 0
    for k in dc.PARAMS:
        st = opt.state[new[k]]
        assert float(st["step"]) == 1.0 and st["step"].device.type == "cpu" and st["exp_avg"].shape == new[k].shape           # `step` is preserved
    # the same on the twin
    src, kind = res.src.cpu().long(), res.kind.cpu()
    t_new = {}
    for i, k in enumerate(dc.PARAMS):
        old = t_leaves[k]
        st = t_opt.state.pop(old)
        value = old.detach()[src].clone()
        if k in dc.COMPUTED:                                      # what a split child computes is the densification's, tested there
            value[kind == 2] = new[k].detach().cpu().double()[kind == 2]
        keep = (kind == 0).reshape((-1,) + (1,) * (value.dim() - 1)).to(torch.float64)
        m, v = st["exp_avg"][src] * keep, st["exp_avg_sq"][src] * keep
        if k == "_opacity":
            x = torch.minimum(torch.sigmoid(value), torch.full_like(value, 0.01))
            value, m, v = torch.log(x / (1 - x)), torch.zeros_like(m), torch.zeros_like(v)
        t_new[k] = torch.nn.Parameter(value)
        t_opt.param_groups[i]["params"][0] = t_new[k]
        t_opt.state[t_new[k]] = {"step": st["step"], "exp_avg": m, "exp_avg_sq": v}
    g2 = draw({**new, **extra})
    _step(opt, {**new, **extra}, g2)
    tw.step(t_opt, {**t_new, **t_extra}, g2)
    got, want = _result(opt, {**new, **extra}), tw.result(t_opt, {**t_new, **t_extra})
    assert float(opt.state[new["_xyz"]]["step"]) == 2.0 == float(opt.state[extra["verts"]]["step"])
    _within(got, want, "after the densification", tensors=list(new) + ["verts"])


# ---- 6. the example ---------------------------------------------------------------------------------------------------------------

def test_the_example_trains():
    path = os.path.join(ROOT, "examples", "appearance_train_demo.py")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, path, "--size", "32"], capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-1500:])
    assert r.returncode == 0 and "densification:" in r.stdout and "reset_opacity" in r.stdout
    losses = [float(line.split("loss")[1].split()[0]) for line in r.stdout.splitlines() if line.startswith("iteration")]
    assert len(losses) >= 30 and losses[-1] < losses[0]
