"""Densification on the GPU: mpmavatar_amd.densify (csrc/densify.hip) against the float64 twin (tests/densify_twin_torch.py) -- src,
kind, binding, binding_counter, the counts, copied rows and moments exactly, computed values within BOUND = 10 * S32
(tests/densify_cases.py, measured on the CPU) -- and the properties the module promises: the same bits on every run, the statistics
update with int32 radii and with a bool mask, a bad binding raises, one host synchronisation per densification and none per
statistics update, the hand-over to a real Adam, reset_opacity, and the example.  Every comparison prints its figures before it
asserts (-s)."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import densify_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLEEP_CYCLES = 50_000_000              # tens of milliseconds of device time in front of the work whose launch must not wait for it


def _dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


def _stats(c, prefix=""):
    from mpmavatar_amd.densify import DensifyStats
    s = DensifyStats(c["binding"].shape[0], DEV)
    s.xyz_gradient_accum, s.denom = _dev(c[prefix + "accum"]), _dev(c[prefix + "denom"])
    if prefix:
        s.max_radii2D = _dev(c["add_max_radii"])
    else:
        s.max_radii2D.fill_(50.0)        # far above any screen size: the reference's screen-size test is dead
    return s


def _inputs(c):
    t = {k: _dev(c[k]) for k in dc.PARAMS + ("binding", "face_scaling", "noise")}
    t["moments"] = {k: (_dev(c["m_" + k]), _dev(c["v_" + k])) for k in dc.PARAMS}
    return t


def _densify(c, t=None, stats=None, **kw):
    from mpmavatar_amd.densify import densify_and_prune
    t, h = t or _inputs(c), c["hyper"]
    stats = stats or _stats(c)
    res = densify_and_prune(*[t[k] for k in dc.PARAMS], t["binding"], c["n_faces"], t["face_scaling"], stats, h["max_grad"], h["min_opacity"],
                            h["extent"], h["max_screen_size"], h["percent_dense"], moments=t["moments"], noise=t["noise"], **kw)
    return res, stats


def _arrays(res):
    out = {k: getattr(res, k).cpu().numpy() for k in dc.PARAMS + ("binding", "binding_counter", "src", "kind")}
    for k in dc.PARAMS:
        out["m_" + k], out["v_" + k] = (m.cpu().numpy() for m in res.moments[k])
    out["counts"] = np.array([res.n_out, res.n_cloned, res.n_split, res.n_pruned], np.int32)
    return out


@pytest.mark.parametrize("name", dc.CASES)
def test_every_case_against_float64(name):
    c = dc.case(name)
    res, stats = _densify(c)
    got = _arrays(res)
    assert all(v.dtype in (np.float32, np.int32) for v in got.values())
    dc.compare(got, dc.twin64(name), dc.BOUND, name)
    # afterwards: all three statistics are zero and of the new length
    assert stats.xyz_gradient_accum.shape == (res.n_out, 1) and stats.denom.shape == (res.n_out, 1) and stats.max_radii2D.shape == (res.n_out,)
    assert not stats.xyz_gradient_accum.any() and not stats.denom.any() and not stats.max_radii2D.any()


def test_the_same_bits_on_two_runs():
    c = dc.case("main")
    a, b = _arrays(_densify(c)[0]), _arrays(_densify(c)[0])
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k


def test_drawn_noise_only_moves_the_children():
    """without `noise` the module draws it from the generator: the same seed gives the same bits, and everything but the children's
    _xyz is what the given noise gives"""
    c = dc.case("main")
    t = _inputs(c)
    given = _arrays(_densify(c, t)[0])
    t["noise"] = None
    gen = lambda: torch.Generator(device=DEV).manual_seed(5)
    a, b = _arrays(_densify(c, t, generator=gen())[0]), _arrays(_densify(c, t, generator=gen())[0])
    new = a["kind"] == 2
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        if k != "_xyz":
            assert np.array_equal(a[k], given[k]), k
    assert np.array_equal(a["_xyz"][~new], given["_xyz"][~new]) and (a["_xyz"][new] != given["_xyz"][new]).any(1).all()


@pytest.mark.parametrize("name", ("main", "tiny", "empty"))
@pytest.mark.parametrize("mask", (False, True), ids=("radii", "mask"))
def test_stats_add_against_float64(name, mask):
    c = dc.case(name)
    s = _stats(c, "add_")
    ptrs = [t.data_ptr() for t in (s.xyz_gradient_accum, s.denom, s.max_radii2D)]
    s.add(_dev(c["grad"]), _dev(c["radii"] > 0) if mask else _dev(c["radii"]))
    assert ptrs == [t.data_ptr() for t in (s.xyz_gradient_accum, s.denom, s.max_radii2D)]                # in place
    got = dict(add_accum=s.xyz_gradient_accum.cpu().numpy(), add_denom=s.denom.cpu().numpy(), add_max_radii=s.max_radii2D.cpu().numpy())
    want = dc.twin64(name, mask)
    for k, v in got.items():
        err = dc.rel(v, want[k])
        print(name, k, "%.3g of bound %.3g" % (err, dc.BOUND))
        assert err <= dc.BOUND, k
    hidden = c["radii"] == 0
    for k in got:
        assert np.array_equal(got[k][hidden], c[k][hidden]), k
    assert np.array_equal(got["add_denom"], want["add_denom"]) and np.array_equal(got["add_max_radii"], want["add_max_radii"])


def test_reset_opacity_against_float64():
    from mpmavatar_amd.densify import reset_opacity
    for name in ("main", "empty"):
        got = reset_opacity(_dev(dc.case(name)["_opacity"])).cpu().numpy()
        err = dc.rel(got, dc.twin64(name)["reset"])
        print(name, "reset %.3g of bound %.3g" % (err, dc.BOUND))
        assert got.dtype == np.float32 and err <= dc.BOUND


def test_a_bad_binding_raises():
    c = dc.case("main")
    for value in (-1, c["n_faces"]):
        t = _inputs(c)
        t["binding"][300] = value
        with pytest.raises(RuntimeError, match="binding: index out of range"):
            _densify(c, t)
    t = _inputs(c)
    for k, bad in (("_scaling", t["_scaling"][:-1]), ("_opacity", t["_opacity"].double()), ("binding", t["binding"].long()), ("noise", t["noise"][:, :1])):
        with pytest.raises(RuntimeError, match=k):
            _densify(c, dict(t, **{k: bad}))
    with pytest.raises(RuntimeError, match="GPU"):
        _densify(c, dict(t, _xyz=t["_xyz"].cpu()))


def _synchronisations(fn):
    """the number of synchronising torch calls `fn` makes, and whether it returned while the stream still had work in front of it:
    the stream is made busy first (a spin kernel of SLEEP_CYCLES) and QUERIED on return -- nothing is timed"""
    stream = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(SLEEP_CYCLES)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                out = fn()
            finally:
                torch.cuda.set_sync_debug_mode(previous)
        busy = not stream.query()
    stream.synchronize()
    reported = [str(w.message) for w in caught if "synchronizing" in str(w.message).lower() and "prototype" not in str(w.message)]
    for m in reported:
        print("   reported:", m[:200])
    return len(reported), busy, out


def test_one_synchronisation_per_densification_and_none_per_statistics_update():
    c = dc.case("main")
    s = _stats(c, "add_")
    grad, radii = _dev(c["grad"]), _dev(c["radii"])
    s.add(grad, radii)                                       # the library is loaded and the kernel's code object is on the device
    count, busy, _ = _synchronisations(lambda: s.add(grad, radii))
    print("stats.add: %d synchronisations, stream still busy on return: %s" % (count, busy))
    assert count == 0 and busy
    t, stats = _inputs(c), _stats(c)
    _densify(c, t, _stats(c))
    with torch.cuda.stream(torch.cuda.Stream(DEV)):          # the probe itself: torch reports a .cpu() here
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            torch.ones(1, device=DEV).cpu()
        torch.cuda.set_sync_debug_mode("default")
    per_copy = sum("synchronizing" in str(w.message).lower() and "prototype" not in str(w.message) for w in caught)
    count, busy, (res, _) = _synchronisations(lambda: _densify(c, t, stats))
    print("densify_and_prune: %d synchronising calls reported; one device-to-host copy reports %d" % (count, per_copy))
    assert per_copy >= 1 and count == per_copy and res.n_out == dc.twin64("main")["counts"][0]


def test_swap_into_a_real_adam():
    from mpmavatar_amd.densify import GROUPS, adam_moments, reset_opacity
    c = dc.case("main")
    t = _inputs(c)
    params = {k: torch.nn.Parameter(t[k].clone()) for k in dc.PARAMS}
    verts, cams = torch.nn.Parameter(torch.ones(33, 3, device=DEV)), torch.nn.Parameter(torch.ones(c["binding"].shape[0], device=DEV))
    groups = [{"params": [p], "lr": 1e-3, "name": GROUPS[k]} for k, p in params.items()]
    groups += [{"params": [verts], "lr": 1e-3, "name": "verts"}, {"params": [cams], "lr": 1e-3, "name": "cams"}]      # cams: n rows by chance
    opt = torch.optim.Adam(groups, eps=1e-15)
    for p in list(params.values()) + [verts, cams]:
        p.grad = torch.ones_like(p)
    for _ in range(3):
        opt.step()
    moments = adam_moments(opt)
    assert set(moments) == set(dc.PARAMS) and moments["_xyz"][0] is opt.state[params["_xyz"]]["exp_avg"]
    before = {k: (p.detach().clone(), moments[k][0].clone(), moments[k][1].clone()) for k, p in params.items()}
    t.update({k: p for k, p in params.items()}, moments=moments)
    res, _ = _densify(c, t)
    new = res.swap_into(opt)
    src, kept = res.src.long(), res.kind == 0
    assert len(opt.param_groups) == 8 and len(opt.state) == 8
    for i, k in enumerate(dc.PARAMS):
        p = opt.param_groups[i]["params"][0]
        st = opt.state[p]
        assert p is new[k] is getattr(res, k) and isinstance(p, torch.nn.Parameter) and p.requires_grad and p.is_leaf
        assert p.shape[0] == res.n_out and float(st["step"]) == 3 and params[k] not in opt.state
        for m, old in zip((st["exp_avg"], st["exp_avg_sq"]), before[k][1:]):
            assert m.shape == p.shape and torch.equal(m[kept], old[src[kept]]) and not m[~kept].any()
        if k not in dc.COMPUTED:
            assert torch.equal(p.detach(), before[k][0][src])
    assert opt.param_groups[6]["params"][0] is verts and opt.param_groups[7]["params"][0] is cams
    assert float(opt.state[verts]["step"]) == 3 and opt.state[cams]["exp_avg"].shape == cams.shape
    # reset_opacity with the optimiser: a new parameter, zero moments, step kept
    opa = reset_opacity(new["_opacity"], opt)
    st = opt.state[opa]
    assert opt.param_groups[3]["params"][0] is opa and float(st["step"]) == 3 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert new["_opacity"] not in opt.state and float(opa.detach().max()) <= np.log(0.01 / 0.99) + 1e-6
    new["_opacity"] = opa
    # an optimiser step on the grown set works and moves every row
    for p in list(new.values()) + [verts, cams]:
        p.grad = torch.ones_like(p)
    old = {k: p.detach().clone() for k, p in new.items()}
    opt.step()
    for k, p in new.items():
        if p.numel():
            assert float(opt.state[p]["step"]) == 4 and (p.detach() != old[k]).all(), k


def test_the_example_trains_across_a_densification():
    path = os.path.join(ROOT, "examples", "densify_demo.py")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, path, "--size", "32", "--steps", "8", "--reset"], capture_output=True, text=True)
    print(r.stdout[-1500:], r.stderr[-1500:])
    assert r.returncode == 0 and "densification:" in r.stdout and "loss" in r.stdout
