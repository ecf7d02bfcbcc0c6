"""The regularisation terms of the appearance loop on the GPU: mpmavatar_amd.regularizers under torch autograd (csrc/reg.hip) against
the float64 twin (tests/reg_twin_torch.py) within BOUND = 10 * S32 (tests/reg_cases.py, measured on the CPU), and the properties the
ops promise: the same bits on every run, exact zeros, NaN with nothing visible, the bool mask, the graph rules, gradients that add
to the binding's on the same leaves, the input checks, and the example with the terms in its loss.  Every comparison prints its
figures before it asserts (-s)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import binding_grad_cases as bc
import binding_twin_torch as btw
import reg_cases as rc
import reg_twin_torch as tw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WEIGHTS = (0.1, 20.0, 1000.0)


def _dev(a, grad=False):
    return torch.tensor(np.asarray(a), device=DEV).requires_grad_(grad)


def _regularizer(name, given=True):
    """the case's MeshRegularizer: with the neighbour array handed over, or left to adjacent_faces"""
    from mpmavatar_amd.regularizers import MeshRegularizer
    c = rc.mesh_case(name)
    return MeshRegularizer(_dev(c["faces"]), _dev(c["verts0"]), _dev(rc.neighbors(name)) if given else None)


def _mesh_run(name, reg=None):
    """-> dict over MESH_TENSORS: the terms and one backward per term (a one-hot upstream, so two entries of it are zero)"""
    reg = reg or _regularizer(name)
    verts = _dev(rc.mesh_case(name)["verts"], True)
    terms = reg.terms(verts)
    assert terms.shape == (3,) and terms.dtype == torch.float32 and terms.grad_fn is not None
    out = dict(zip(rc.MESH_VALUES, terms.detach().cpu().numpy()))
    for i, k in enumerate(rc.MESH_GRADS):
        out[k] = torch.autograd.grad(terms[i], verts, retain_graph=True)[0].cpu().numpy()
    return out


def _gauss_leaves(c, grad=rc.GAUSS_GRADS):
    return {k: _dev(c[k], k in grad) for k in rc.GAUSS_GRADS}


def _gauss_run(name, mask=False, grad=rc.GAUSS_GRADS):
    from mpmavatar_amd.regularizers import gaussian_terms
    c = rc.gauss_case(name)
    t = _gauss_leaves(c, grad)
    radii = _dev(c["radii"] > 0) if mask else _dev(c["radii"])
    terms = gaussian_terms(t["_opacity"], t["_xyz"], t["_scaling"], radii, *rc.THRESHOLDS)
    out = dict(zip(rc.GAUSS_VALUES, terms.detach().cpu().numpy()))
    if grad:
        terms.sum().backward()
    out.update({k: None if v.grad is None else v.grad.cpu().numpy() for k, v in t.items()})
    return out, terms


# ---- 1. every case against the twin ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", rc.MESH_CASES + ("wide",))
def test_mesh_against_the_twin(name):
    reg = _regularizer(name)
    got, want = _mesh_run(name, reg), rc.mesh64(name)
    for k in rc.MESH_TENSORS:
        err = rc.rel(got[k], want[k])
        print(name, k, "%.3g of bound %.3g" % (err, rc.BOUND))
        assert np.isfinite(got[k]).all() and err <= rc.BOUND, (name, k, err)
    with torch.no_grad():                                                        # the same launch, the same bits, no graph
        quiet = reg.terms(_dev(rc.mesh_case(name)["verts"], True))
    plain = reg.terms(_dev(rc.mesh_case(name)["verts"]))
    for t in (quiet, plain):
        assert t.grad_fn is None and not t.requires_grad
        assert np.array_equal(t.cpu().numpy(), np.array([got[k] for k in rc.MESH_VALUES]))
    normal, iso, eq_faces = reg(_dev(rc.mesh_case(name)["verts"]))
    assert normal.dim() == 0 and float(iso) == got["iso"] and float(eq_faces) == got["area"]


def test_mesh_set_up_and_adjacent_faces():
    """neighbor_dist / neighbor_weight against the reference's own (the fixture); the regulariser that finds its neighbours itself
    gives the same bits"""
    g = np.load(os.path.join(bc.ROOT, "tests", "golden", "reg.npz"))
    for name in ("sheet", "closed", "one"):
        reg, own = _regularizer(name), _regularizer(name, given=False)
        assert torch.equal(reg.face_neighbors, own.face_neighbors) and reg.face_neighbors.dtype == torch.int32
        for k, mine in (("neighbor_dist", reg.neighbor_dist), ("neighbor_weight", reg.neighbor_weight)):
            err = rc.rel(mine.cpu().numpy(), g[f"{name}_{k}"])
            print(name, k, "%.3g of bound %.3g" % (err, rc.BOUND))
            assert err <= rc.BOUND and torch.equal(mine, getattr(own, k))


@pytest.mark.parametrize("name", rc.GAUSS_CASES)
def test_gauss_against_the_twin(name):
    got, terms = _gauss_run(name)
    want = rc.gauss64(name)
    assert terms.grad_fn is not None and terms.shape == (3,)
    for k in rc.GAUSS_TENSORS:
        if np.isnan(want[k]).any():
            assert name == "none_visible" and k in ("xyz", "scale") and np.isnan(got[k])
            continue
        err = rc.rel(got[k], want[k])
        print(name, k, "%.3g of bound %.3g" % (err, rc.BOUND))
        assert np.isfinite(got[k]).all() and err <= rc.BOUND, (name, k, err)
    quiet, terms0 = _gauss_run(name, grad=())
    assert terms0.grad_fn is None
    for k in rc.GAUSS_VALUES:
        assert np.array_equal(quiet[k], got[k], equal_nan=True)


# ---- 2. determinism ---------------------------------------------------------------------------------------------------------------

def test_two_runs_give_the_same_bits():
    """the wide sheet (258 partials, vertices of six faces) and 20,000 Gaussians, forward and backward twice"""
    from mpmavatar_amd.regularizers import gaussian_terms
    reg = _regularizer("wide")
    w = _dev(np.array(WEIGHTS, np.float32))

    def mesh_once():
        verts = _dev(rc.mesh_case("wide")["verts"], True)
        terms = reg.terms(verts)
        (w * terms).sum().backward()
        return [terms.detach(), verts.grad]

    rng = np.random.default_rng(3)
    n = 20000
    data = [rng.normal(0, 2, (n, 1)), rng.normal(0, 0.8, (n, 3)), rng.normal(-0.9, 0.5, (n, 3))]
    radii = _dev(rng.integers(0, 4, n).astype(np.int32))

    def gauss_once():
        leaves = [_dev(a.astype(np.float32), True) for a in data]
        terms = gaussian_terms(*leaves, radii, *rc.THRESHOLDS)
        (w * terms).sum().backward()
        return [terms.detach()] + [t.grad for t in leaves]

    for once in (mesh_once, gauss_once):
        a, b = once(), once()
        for x, y in zip(a, b):
            assert torch.isfinite(x).all() and (x != 0).any() and torch.equal(x, y)


# ---- 3. and 4. exact zeros, nothing visible, the bool mask -------------------------------------------------------------------------------

def test_exact_zeros():
    r = _mesh_run("flat")
    assert r["normal"] == 0 and r["area"] == 0 and 0 < r["iso"] < 2e-10
    for k in rc.MESH_GRADS:
        assert (r[k] == 0).all(), k
    r = _mesh_run("one")
    assert r["normal"] <= 2.0 ** -22 and r["area"] == 0
    for k in rc.MESH_GRADS:
        assert (r[k] == 0).all(), k
    # a vertex in no face gets exactly 0
    from mpmavatar_amd.regularizers import MeshRegularizer
    c = rc.mesh_case("sheet")
    more = lambda a: np.concatenate([a, [[1, 2, 3]]]).astype(np.float32)
    reg = MeshRegularizer(_dev(c["faces"]), _dev(more(c["verts0"])))
    verts = _dev(more(c["verts"]), True)
    (reg.terms(verts) * _dev(np.array(WEIGHTS, np.float32))).sum().backward()
    assert (verts.grad[-1] == 0).all() and (verts.grad[:-1] != 0).any(1).all()
    # the invisible Gaussians, and a relu that binds
    g = rc.gauss_case("main")
    r = _gauss_run("main")[0]
    hidden = g["radii"] == 0
    assert hidden.any() and (r["_xyz"][hidden] == 0).all() and (r["_scaling"][hidden] == 0).all()
    assert (r["_xyz"][~hidden] != 0).any() and (r["_scaling"][~hidden] != 0).any() and (r["_opacity"] != 0).all()
    b = np.exp(g["_scaling"].astype(np.float64)) - rc.THRESHOLDS[1]
    assert (r["_scaling"][b <= 0] == 0).all() and (r["_scaling"][~hidden][(b > 0)[~hidden]] != 0).all()


def test_none_visible_and_the_bool_mask():
    r, terms = _gauss_run("none_visible")
    assert np.isnan(r["xyz"]) and np.isnan(r["scale"]) and np.isfinite(r["opacity"])
    assert (r["_xyz"] == 0).all() and (r["_scaling"] == 0).all()
    main = _gauss_run("main")[0]
    assert r["opacity"] == main["opacity"] and np.array_equal(r["_opacity"], main["_opacity"])
    masked = _gauss_run("main", mask=True)[0]
    for k in rc.GAUSS_TENSORS:
        assert np.array_equal(masked[k], main[k]), k
    from mpmavatar_amd.regularizers import gaussian_regularizers
    t = _gauss_leaves(rc.gauss_case("main"))
    opacity, xyz, scale = gaussian_regularizers(t["_opacity"], t["_xyz"], t["_scaling"], _dev(rc.gauss_case("main")["radii"]), *rc.THRESHOLDS)
    assert opacity.dim() == 0 and tuple(float(t.detach()) for t in (opacity, xyz, scale)) == tuple(main[k] for k in rc.GAUSS_VALUES)


# ---- 5. the graph rules -------------------------------------------------------------------------------------------------------------

def test_graph_rules():
    from mpmavatar_amd.regularizers import gaussian_regularizers, gaussian_terms
    want = rc.gauss64("main")
    for k in rc.GAUSS_GRADS:                                                     # one leaf at a time: None for the others
        got, terms = _gauss_run("main", grad=(k,))
        assert terms.grad_fn is not None and all(got[o] is None for o in rc.GAUSS_GRADS if o != k)
        err = rc.rel(got[k], want[k])
        print(k, "alone %.3g of bound %.3g" % (err, rc.BOUND))
        assert err <= rc.BOUND
    # a weighted sum through the unbound scalars and through the [3] tensor: the same bits
    c, w = rc.gauss_case("main"), (0.05, 1.0, 0.0)                               # a zero entry in the upstream
    a, b = _gauss_leaves(c), _gauss_leaves(c)
    opacity, xyz, scale = gaussian_regularizers(a["_opacity"], a["_xyz"], a["_scaling"], _dev(c["radii"]), *rc.THRESHOLDS)
    (w[0] * opacity + w[1] * xyz + w[2] * scale).backward()
    (_dev(np.array(w, np.float32)) * gaussian_terms(b["_opacity"], b["_xyz"], b["_scaling"], _dev(c["radii"]), *rc.THRESHOLDS)).sum().backward()
    for k in rc.GAUSS_GRADS:
        assert torch.equal(a[k].grad, b[k].grad), k
    assert (a["_scaling"].grad == 0).all() and (a["_xyz"].grad != 0).any()
    reg = _regularizer("sheet")
    va, vb = _dev(rc.mesh_case("sheet")["verts"], True), _dev(rc.mesh_case("sheet")["verts"], True)
    normal, iso, eq_faces = reg(va)
    (WEIGHTS[0] * normal + WEIGHTS[1] * iso + WEIGHTS[2] * eq_faces).backward()
    (_dev(np.array(WEIGHTS, np.float32)) * reg.terms(vb)).sum().backward()
    assert torch.equal(va.grad, vb.grad)
    # a term that takes no part in the loss: no upstream gradient, no launch, no gradient
    v = _dev(rc.mesh_case("sheet")["verts"], True)
    (reg.terms(v).sum() * 0 + v.sum()).backward()
    assert (v.grad == 1).all()


# ---- 6. the gradients add to the binding's on the same leaves ---------------------------------------------------------------------------

def test_gradients_add_to_the_bindings():
    """verts -> MeshFrames.set_mesh_by_verts -> BoundGaussians.render_inputs -> a weighted sum standing for the rasteriser, plus the six
    terms on the same verts, _xyz, _scaling and _opacity: each leaf receives the sum of both paths, against binding_twin_torch and
    reg_twin_torch in float64 -- and against the two paths run separately on the device"""
    from mpmavatar_amd.mesh_frames import MeshFrames
    from mpmavatar_amd.regularizers import MeshRegularizer, gaussian_terms
    from mpmavatar_amd.render_inputs import BoundGaussians
    b = bc.case("main")
    n = b["binding"].shape[0]
    rng = np.random.default_rng(9)
    radii = rng.integers(0, 4, n).astype(np.int32)
    verts0 = (b["verts"] + rng.normal(0, 0.01, b["verts"].shape)).astype(np.float32)
    w_reg = np.array([300.0, 4e5, 2.5e4, 50.0, 100.0, 200.0], np.float32)        # on this mesh of unit size: a share of 1 % and more on every leaf
    outs = ("means3D", "scales", "opacities", "rotations")
    leaves = ("verts", "_xyz", "_scaling", "_opacity")
    reg = MeshRegularizer(_dev(b["faces"]), _dev(verts0))

    def ours(raster, regs):
        t = {k: _dev(b[k], True) for k in bc.NAMES}
        loss = 0
        if raster:
            fr = MeshFrames(_dev(b["faces"]))
            bg = BoundGaussians(t["_xyz"], t["_rotation"], t["_scaling"], t["_opacity"], torch.zeros(n, 1, 3, device=DEV), torch.zeros(n, 0, 3, device=DEV),
                                _dev(b["binding"]))
            fr.set_mesh_by_verts(t["verts"])
            out = bg.render_inputs(fr)
            loss = loss + sum((_dev(b["w_" + k]) * out[k]).sum() for k in outs)
        if regs:
            terms = torch.cat([reg.terms(t["verts"]), gaussian_terms(t["_opacity"], t["_xyz"], t["_scaling"], _dev(radii), *rc.THRESHOLDS)])
            loss = loss + (_dev(w_reg) * terms).sum()
        loss.backward()
        return {k: t[k].grad.double().cpu().numpy() for k in leaves}

    both, only_raster, only_reg = ours(True, True), ours(True, False), ours(False, True)
    d = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    u = {k: d(b[k]).requires_grad_(True) for k in bc.NAMES}
    faces64, binding64 = torch.tensor(b["faces"].astype(np.int64)), torch.tensor(b["binding"].astype(np.int64))
    nb64 = torch.tensor(reg.face_neighbors.cpu().numpy().astype(np.int64))
    out = btw.render_inputs(u["verts"], faces64, binding64, u["_xyz"], u["_rotation"], u["_scaling"], u["_opacity"])
    nd, nw = tw.setup(d(verts0), faces64, nb64)
    terms = torch.cat([tw.mesh_terms(u["verts"], faces64, nb64, nd, nw),
                       tw.gauss_terms(u["_opacity"], u["_xyz"], u["_scaling"], torch.from_numpy(radii > 0), *rc.THRESHOLDS)])
    (sum((d(b["w_" + k]) * out[k]).sum() for k in outs) + (d(w_reg) * terms).sum()).backward()
    bound = max(rc.BOUND, bc.BOUND)
    for k in leaves:
        err, parts = rc.rel(both[k], u[k].grad.numpy()), rc.rel(both[k], only_raster[k] + only_reg[k])
        share = rc.rel(only_raster[k], both[k])
        print(k, "against float64 %.3g, against the sum of the separate gradients %.3g, of bound %.3g; the terms' share %.3g" % (err, parts, bound, share))
        assert err <= bound and parts <= bound and share > 1e-2, k


# ---- 7. input checks ------------------------------------------------------------------------------------------------------------------

def test_input_checks():
    from mpmavatar_amd.regularizers import MeshRegularizer, gaussian_terms
    c, g = rc.mesh_case("sheet"), rc.gauss_case("main")
    reg = _regularizer("sheet")
    verts = _dev(c["verts"])
    bad_verts = [verts.double(), verts[:-1], verts.cpu(), torch.cat([verts, verts], 1)[:, :3], verts.reshape(-1)]
    for v in bad_verts:
        with pytest.raises(RuntimeError):
            reg.terms(v)
    for faces, verts0, nb in ((_dev(c["faces"]), _dev(c["verts0"])[:100], None), (_dev(c["faces"]), _dev(c["verts0"]).double(), None),
                              (_dev(c["faces"]), _dev(c["verts0"]), _dev(rc.neighbors("sheet"))[:-1]),
                              (_dev(c["faces"]), _dev(c["verts0"]), _dev(rc.neighbors("sheet")) + 1),
                              (_dev(c["faces"])[:0], _dev(c["verts0"]), None)):
        with pytest.raises(RuntimeError):
            MeshRegularizer(faces, verts0, nb)
    t, radii = _gauss_leaves(g, ()), _dev(g["radii"])
    ok = [t["_opacity"], t["_xyz"], t["_scaling"], radii]
    bad = [(0, t["_opacity"].double()), (0, t["_opacity"][:-1]), (1, t["_xyz"].cpu()), (1, torch.cat([t["_xyz"], t["_xyz"]], 1)[:, :3]),
           (2, t["_scaling"][:, :2]), (2, t["_scaling"].half()), (3, radii.long()), (3, radii[:-1]), (3, radii.float()), (3, g["radii"])]
    for i, x in bad:
        args = list(ok)
        args[i] = x
        with pytest.raises(RuntimeError):
            gaussian_terms(*args, *rc.THRESHOLDS)
    assert torch.isfinite(gaussian_terms(t["_opacity"].reshape(-1), t["_xyz"], t["_scaling"], radii, *rc.THRESHOLDS)).all()      # [n] is fine


# ---- 8. the example with the terms in its loss ------------------------------------------------------------------------------------------

def test_reg_demo_lowers_its_loss():
    """a fresh child process under a time limit of its own"""
    path = os.path.join(bc.ROOT, "examples", "appearance_step_demo.py")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, path, "--reg", "--size", "32", "--steps", "10"], capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.returncode
    last = r.stdout.strip().splitlines()[-1]
    first, final = [float(x) for x in last.split()[1:4:2]]
    assert "eq_faces_weight" in r.stdout and np.isfinite([first, final]).all() and final < first
