"""The gradients of the mesh binding on the GPU: MeshFrames.set_mesh_by_verts, the MeshFrames getters and
BoundGaussians.render_inputs under torch autograd (csrc/frames_backward.hip) against the float64 twin (tests/binding_twin_torch.py)
within BOUND = 10 * G32 (tests/binding_grad_cases.py, measured on the CPU), and the properties the backward pass promises: exact zeros,
gradient subsets, the table cache, degenerate faces equal to the host build of the same header, the same bits on every run, and the
whole chain down from the image loss.  Every comparison prints its figures before it asserts (run with -s)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import binding_grad_cases as bc
import binding_twin_torch as tw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PARAMS = ("_xyz", "_rotation", "_scaling", "_opacity")


def _leaves(c, grad=bc.NAMES, verts=None):
    return {k: torch.tensor(np.asarray(c[k] if k != "verts" or verts is None else verts), device=DEV).requires_grad_(k in grad)
            for k in bc.NAMES}


def _weights(c):
    return {k: torch.tensor(c["w_" + k], device=DEV) for k in bc.OUTS}


def _model(c, t, binding=None):
    from mpmavatar_amd.mesh_frames import MeshFrames
    from mpmavatar_amd.render_inputs import BoundGaussians
    n = c["binding"].shape[0]
    fr = MeshFrames(torch.tensor(c["faces"], device=DEV))
    fr.set_mesh_by_verts(t["verts"])
    b = torch.tensor(c["binding"] if binding is None else binding, device=DEV)
    bg = BoundGaussians(t["_xyz"], t["_rotation"], t["_scaling"], t["_opacity"], torch.zeros(n, 1, 3, device=DEV),
                        torch.zeros(n, 0, 3, device=DEV), b)
    return fr, bg


def _grads(t):
    return {k: (None if v.grad is None else v.grad.cpu().numpy()) for k, v in t.items()}


def _through_render(c, grad=bc.NAMES, binding=None, outs=bc.OUTS):
    """-> (gradients of the case's loss over `outs`, the four outputs, frames, gaussians)"""
    t = _leaves(c, grad)
    fr, bg = _model(c, t, binding)
    args = bg.render_inputs(fr)
    w = _weights(c)
    sum((w[k] * args[k]).sum() for k in outs).backward()
    return _grads(t), args, fr, bg


def _assert_within_bound(got, want, names, tag):
    for k in names:
        err = bc.rel_grad(got[k], want[k])
        print(tag, k, "%.3g of bound %.3g" % (err, bc.BOUND))
        assert np.isfinite(got[k]).all() and err <= bc.BOUND, (tag, k, err)


# ---- 1. the main case against the twin -------------------------------------------------------------------------------------------

def test_main_case_against_the_twin():
    c, want = bc.case("main"), bc.g64("main")
    n = c["binding"].shape[0]
    got, args, fr, bg = _through_render(c)
    assert all(args[k].grad_fn is not None for k in bc.OUTS) and args["means2D"].grad_fn is None and not args["means2D"].requires_grad
    _assert_within_bound(got, want, bc.NAMES, "render_inputs")
    # the outputs are bitwise those of the no-grad call, which carry no graph
    with torch.no_grad():
        fr0, bg0 = _model(c, _leaves(c))
        quiet = bg0.render_inputs(fr0)
    for k in bc.OUTS + ("means2D",):
        assert quiet[k].grad_fn is None and torch.equal(quiet[k], args[k]), k
    for a, b in ((fr0.face_center, fr.face_center), (fr0.face_orien_mat, fr.face_orien_mat), (fr0.face_orien_quat, fr.face_orien_quat),
                 (fr0.face_scaling, fr.face_scaling)):
        assert a.grad_fn is None and b.grad_fn is not None and torch.equal(a, b)
    # again through get_all: the same bits (the opacity is torch's sigmoid there and takes no part in the other four)
    t = _leaves(c)
    fr2, _ = _model(c, t)
    xyz, rot, scl = fr2.get_all(torch.tensor(c["binding"], device=DEV), t["_xyz"], t["_rotation"], t["_scaling"])
    w = _weights(c)
    ((w["means3D"] * xyz).sum() + (w["rotations"] * rot).sum() + (w["scales"] * scl).sum()).backward()
    again = _grads(t)
    for k in ("verts", "_xyz", "_rotation", "_scaling"):
        assert np.array_equal(again[k], got[k]), k
    assert torch.equal(xyz, args["means3D"]) and torch.equal(rot, args["rotations"]) and torch.equal(scl, args["scales"])
    # the single getters: one output each, the same parameter gradients
    t = _leaves(c)
    fr3, _ = _model(c, t)
    b = torch.tensor(c["binding"], device=DEV)
    ((w["means3D"] * fr3.get_xyz(b, t["_xyz"])).sum() + (w["rotations"] * fr3.get_rotation(b, t["_rotation"])).sum() +
     (w["scales"] * fr3.get_scaling(b, t["_scaling"])).sum()).backward()
    single = _grads(t)
    for k in ("_xyz", "_rotation", "_scaling"):
        assert np.array_equal(single[k], got[k]), k
    _assert_within_bound(single, want, ("verts",), "three getters")          # three partial sums per vertex, added by torch
    # extra primitives behind the bound ones: their gradients are the upstream rows, exactly
    m = 19
    g = torch.Generator().manual_seed(5)
    extra = [torch.randn(m, k, generator=g).to(DEV).requires_grad_(True) for k in (3, 3, 1, 3, 4)]
    W = {k: torch.cat([w[k], torch.randn(m, w[k].shape[1], generator=g).to(DEV)]) for k in bc.OUTS}
    t = _leaves(c)
    fr4, bg4 = _model(c, t)
    a4 = bg4.render_inputs(fr4, override_color=torch.rand(n, 3, generator=g).to(DEV), extra=extra)
    assert a4["means3D"].shape == (n + m, 3) and torch.equal(a4["means3D"][:n], args["means3D"]) and torch.equal(a4["means3D"][n:], extra[0])
    sum((W[k] * a4[k]).sum() for k in bc.OUTS).backward()
    for e, k in ((extra[0], "means3D"), (extra[2], "opacities"), (extra[3], "scales"), (extra[4], "rotations")):
        assert torch.equal(e.grad, W[k][n:]), k
    assert extra[1].grad is None
    with_extra = _grads(t)
    for k in bc.NAMES:
        assert np.array_equal(with_extra[k], got[k]), k


def test_render_case_against_the_twin():
    got, _, _, _ = _through_render(bc.case("render"))
    _assert_within_bound(got, bc.g64("render"), bc.NAMES, "render")


# ---- 2. exact zeros ---------------------------------------------------------------------------------------------------------------------

def test_exact_zeros():
    c = bc.case("main")
    n_f = c["faces"].shape[0]
    verts = np.concatenate([c["verts"], [[9.0, 9.0, 9.0]]]).astype(np.float32)          # one more vertex, in no face
    t = _leaves(c, verts=verts)
    fr, bg = _model(c, t)
    frame_tensors = (fr.face_center, fr.face_orien_mat, fr.face_orien_quat, fr.face_scaling)
    for x in frame_tensors:
        x.retain_grad()
    args = bg.render_inputs(fr)
    w = _weights(c)
    sum((w[k] * args[k]).sum() for k in bc.OUTS).backward()
    for x in frame_tensors:                                                             # the last five faces hold no Gaussian
        assert x.grad.shape == x.shape and (x.grad[-5:] == 0).all() and (x.grad[:-5] != 0).any()
    assert (t["verts"].grad[-1] == 0).all() and (t["verts"].grad[:-1] != 0).all()
    # a loss on scales alone: the other upstreams are None, the other parameter gradients exactly zero
    only = {"scales": c["w_scales"], "means3D": None, "rotations": None, "opacities": None}
    got, _, _, _ = _through_render(c, outs=("scales",))
    for k in ("_xyz", "_rotation", "_opacity"):
        assert got[k].shape == c[k].shape and (got[k] == 0).all(), k
    _assert_within_bound(got, bc.twin_grads(c, weights=only), ("verts", "_scaling"), "scales only")
    # n = 0 bound Gaussians with m > 0 extra ones
    from mpmavatar_amd.render_inputs import BoundGaussians
    e = lambda k: torch.zeros(0, k, device=DEV)
    m = 7
    extra = [torch.rand(m, k, device=DEV).requires_grad_(True) for k in (3, 3, 1, 3, 4)]
    t = _leaves(c)
    fr0, _ = _model(c, t)
    bg0 = BoundGaussians(e(3), e(4), e(3), e(1), torch.zeros(0, 1, 3, device=DEV), torch.zeros(0, 0, 3, device=DEV),
                         torch.zeros(0, dtype=torch.int32, device=DEV))
    a0 = bg0.render_inputs(fr0, override_color=e(3), extra=extra)
    assert a0["scales"].shape == (m, 3) and torch.equal(a0["rotations"], extra[4])
    (3.0 * a0["means3D"].sum() + a0["opacities"].sum()).backward()
    assert (extra[0].grad == 3).all() and (extra[2].grad == 1).all() and extra[3].grad is None
    assert t["verts"].grad.shape == t["verts"].shape and (t["verts"].grad == 0).all() and n_f == 320


# ---- 3. subsets of what requires grad ---------------------------------------------------------------------------------------------

def test_grad_subsets():
    c, want = bc.case("main"), bc.g64("main")
    got, args, fr, bg = _through_render(c, grad=("_opacity",))
    assert fr.face_center.grad_fn is None and args["means3D"].grad_fn is not None
    assert bg._gtable._t is None and fr._vtable._t is None                 # no frame gradient was computed: the tables were never built
    assert all(got[k] is None for k in bc.NAMES if k != "_opacity")
    _assert_within_bound(got, want, ("_opacity",), "opacity only")
    got, args, fr, bg = _through_render(c, grad=("verts",))
    assert all(got[k] is None for k in PARAMS)
    _assert_within_bound(got, want, ("verts",), "verts only")
    # the frame tensors as leaves: against the twin's binding expressions differentiated at float64 frames
    t = _leaves(c, grad=())
    fr, bg = _model(c, t)
    names = ("face_center", "face_orien_mat", "face_orien_quat", "face_scaling")
    for k in names:
        assert getattr(fr, k).grad_fn is None
        setattr(fr, k, getattr(fr, k).clone().requires_grad_(True))
    args = bg.render_inputs(fr)
    w = _weights(c)
    sum((w[k] * args[k]).sum() for k in bc.OUTS).backward()
    assert all(v.grad is None for v in t.values())
    d = {k: torch.tensor(c[k], dtype=torch.float64) for k in bc.NAMES}
    b = torch.tensor(c["binding"].astype(np.int64))
    f64 = [x.detach().requires_grad_(True) for x in tw.face_frames(d["verts"], torch.tensor(c["faces"].astype(np.int64)))]
    loss = ((torch.tensor(c["w_means3D"], dtype=torch.float64) * tw.get_xyz(b, d["_xyz"], f64[0], f64[1], f64[3])).sum() +
            (torch.tensor(c["w_rotations"], dtype=torch.float64) * tw.get_rotation(b, d["_rotation"], f64[2])).sum() +
            (torch.tensor(c["w_scales"], dtype=torch.float64) * tw.get_scaling(b, d["_scaling"], f64[3])).sum())
    ref = torch.autograd.grad(loss, f64)
    got = {k: getattr(fr, k).grad.cpu().numpy() for k in names}
    _assert_within_bound(got, dict(zip(names, (r.numpy() for r in ref))), names, "frame leaves")


# ---- 4. the table cache and the version check --------------------------------------------------------------------------------------

def test_table_cache_follows_the_binding():
    c = bc.case("main")
    t = _leaves(c)
    fr, bg = _model(c, t)
    w = _weights(c)

    def run():
        for v in t.values():
            v.grad = None
        fr.set_mesh_by_verts(t["verts"])
        args = bg.render_inputs(fr)
        sum((w[k] * args[k]).sum() for k in bc.OUTS).backward()
        return _grads(t)

    first = run()
    table = bg._gtable._t
    assert table is not None and np.array_equal(run()["verts"], first["verts"]) and bg._gtable._t is table     # kept
    changed = c["binding"].copy()
    changed[::3] = (changed[::3] * 7 + 3) % 320                    # an in-place edit of the binding, onto the empty faces too
    bg.binding.copy_(torch.tensor(changed, device=DEV))
    got = run()
    assert bg._gtable._t is not table                                        # rebuilt
    _assert_within_bound(got, bc.twin_grads(c, binding=changed), bc.NAMES, "after the edit")
    # an in-place write to a saved input between forward and backward is caught by torch's version check
    fr.set_mesh_by_verts(t["verts"])
    args = bg.render_inputs(fr)
    with torch.no_grad():
        t["_xyz"].add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        args["means3D"].sum().backward()


# ---- 5. degenerate and needle faces: the GPU equals the host build of the same header ------------------------------------------------

def test_degenerate_faces_equal_the_host_build():
    from mpmavatar_amd.mesh_frames import MeshFrames
    g = np.load(os.path.join(bc.HERE, "golden", "frames.npz"))
    n, n_f = int(g["n_regular"]), g["faces"].shape[0]
    first_vertex = int(g["faces"][n:].min())                                  # the degenerate faces have vertices of their own
    assert n_f - n == 5 and first_vertex > int(g["faces"][:n].max())
    rng = np.random.default_rng(3)
    w = [rng.normal(size=s).astype(np.float32) for s in ((n_f, 3), (n_f, 3, 3), (n_f, 4), (n_f, 1))]
    verts = torch.tensor(g["verts"], device=DEV).requires_grad_(True)
    fr = MeshFrames(torch.tensor(g["faces"], device=DEV))
    fr.set_mesh_by_verts(verts)
    outs = (fr.face_center, fr.face_orien_mat, fr.face_orien_quat, fr.face_scaling)
    sum((torch.tensor(x, device=DEV) * o).sum() for x, o in zip(w, outs)).backward()
    got = verts.grad.cpu().numpy()
    host, _ = bc.host_frames_backward(g["verts"], g["faces"], fr.face_orien_mat.detach().cpu().numpy(),
                                      fr.face_orien_quat.detach().cpu().numpy(), *w)
    assert np.array_equal(np.isfinite(got), np.isfinite(host))
    fin = np.isfinite(host)
    scale = np.abs(np.where(fin, host, 0)).max(1, keepdims=True)              # per vertex
    err = np.where(fin, np.abs(np.where(fin, got, 0) - np.where(fin, host, 0)), 0) / np.maximum(scale, 1e-30)
    print("degenerate vertices: worst relative difference %.3g, regular %.3g; largest magnitude %.3g" %
          (err[first_vertex:].max(), err[:first_vertex].max(), scale.max()))
    assert err.max() <= 1e-5


# ---- 6. determinism ----------------------------------------------------------------------------------------------------------------

def test_two_backward_passes_give_the_same_bits():
    c = bc.case("main")
    a, _, _, _ = _through_render(c)
    b, _, _, _ = _through_render(c)
    for k in bc.NAMES:
        assert np.array_equal(a[k], b[k]), k


# ---- 7. the whole chain: image loss -> rasteriser -> binding -> frames ------------------------------------------------------------------

def _example():
    path = os.path.join(bc.ROOT, "examples", "appearance_step_demo.py")
    spec = importlib.util.spec_from_file_location("appearance_step_demo", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("eye", [(0.0, 0.3, -2.0), (0.0, 0.3, -0.6)], ids=["example", "close"])
def test_chain_from_the_image_loss(eye):
    """the example's set-up at 32 x 32 (and once more with the camera inside the near range of the sphere, so that Gaussians are
    culled): one backward() through image_loss and the rasteriser reaches every leaf; a small step against the gradient lowers the loss"""
    sc = _example().Scene(32, DEV, eye=eye)
    loss, radii = sc.loss()
    loss.backward()
    culled = radii == 0
    L = float(loss.detach())
    print("loss %.6f, %d of %d Gaussians culled" % (L, int(culled.sum()), radii.numel()))
    assert bool(culled.any()) == (eye[2] > -1.0) and not bool(culled.all())
    sq = 0.0
    for k, p in sc.params.items():
        assert p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all() and (p.grad != 0).any(), k
        if k != "verts_offset":
            assert (p.grad[culled] == 0).all(), k
        sq += float((p.grad.double() ** 2).sum())
    eps = 1e-3 * L / sq                                   # predicted decrease eps |g|^2 = 1e-3 L
    assert eps * sq >= 100 * float(np.spacing(np.float32(L)))
    with torch.no_grad():
        for p in sc.params.values():
            p.sub_(eps * p.grad)
        after = float(sc.loss()[0])
    print("L %.8f -> %.8f, predicted decrease %.3g, actual %.3g" % (L, after, eps * sq, L - after))
    assert after < L
