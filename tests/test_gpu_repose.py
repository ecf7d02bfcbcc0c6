"""Re-posing on the GPU (mpmavatar_amd/reposing.py over csrc/repose.hip, csrc/knn_device.hpp): every case of tests/repose_cases.py
against the float64 twin within BOUND = 10 x S32, S32 being the twin's own float32 error measured on the CPU; neighbour indices equal
to the fixture's on every row (the gap condition of tests/test_repose_host.py is what allows that), the dyadic tie case exact; the
shapes, dtypes and devices of the reference; and the promises of the module: the same bits with and without T, with W broadcast or
repeated, on a second run, and however the targets are sliced; no graph on any output; ValueError before any launch.  Every
comparison prints its figures before it asserts (run with -s)."""
import os
import types

import numpy as np
import pytest
import torch

import repose_cases as rc

pytestmark = pytest.mark.gpu

from mpmavatar_amd import reposing as R  # noqa: E402
from mpmavatar_amd import tracking  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "repose.npz")
DEV = "cuda"


def _g(a, dtype=torch.float32):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


def _search(name, slices=0):
    c = rc.knn_case(name)
    if c["self"]:
        d, i = R.knn_self(_g(c["p1"]), c["K"] - 1)
        return d, i, 1
    out = R.knn_points(_g(c["p1"])[None], _g(c["p2"])[None], K=c["K"], slices=slices)
    assert isinstance(out, tuple) and out.dists is out[0] and out.idx is out[1]
    return out.dists[0], out.idx[0], 0


@pytest.mark.parametrize("name", rc.ALL_KNN)
def test_knn_against_float64(name):
    c = rc.knn_case(name)
    d64, i64 = rc.knn64(name)
    d, i, drop = _search(name)
    n, k = c["p1"].shape[0], c["K"] - drop
    assert d.shape == i.shape == (n, k) and d.dtype == torch.float32 and i.dtype == torch.int64 and d.is_cuda and i.is_cuda
    assert not d.requires_grad
    err = rc.rel(d.cpu().numpy(), d64[:, drop:])
    print(name, "dists %.3g of bound %.3g" % (err, rc.BOUND))
    assert np.array_equal(i.cpu().numpy(), np.load(GOLD)[f"{name}_idx"][:, drop:]), name            # every row
    assert err <= rc.BOUND
    if name == "dyadic":
        assert np.array_equal(d.cpu().numpy(), d64.astype(np.float32))
        for row, want in rc.DYADIC_WANT.items():
            assert i[row].tolist() == want


@pytest.mark.parametrize("name", ["main", "six", "dyadic"])
def test_knn_same_bits_however_sliced_and_on_a_second_run(name):
    d0, i0, _ = _search(name)
    for slices in (0, 1, 2, 7, 64):
        d, i, _ = _search(name, slices)
        assert _same_bits(d, d0) and torch.equal(i, i0), slices


def test_knn_k1_agrees_with_nearest_neighbour():
    c = rc.knn_case("main")
    a, b = _g(c["p1"]), _g(c["p2"])
    got = R.knn_points(a[None], b[None], K=1)
    assert got.idx.shape == (1, 700, 1)
    assert torch.equal(got.idx[0, :, 0], tracking.nearest_neighbour(a, b).to(torch.int64))


def test_knn_batches_and_empty_queries():
    c = rc.knn_case("short4")
    a, b = _g(c["p1"]), _g(c["p2"])
    two = R.knn_points(torch.stack([a, a.flip(0)]), torch.stack([b, b]), K=4)
    one = R.knn_points(a[None], b[None], K=4)
    assert two.idx.shape == (2, 3, 4) and torch.equal(two.idx[0], one.idx[0]) and torch.equal(two.idx[1], one.idx[0].flip(0))
    none = R.knn_points(a[None, :0], b[None], K=4)
    assert none.dists.shape == none.idx.shape == (1, 0, 4) and none.idx.dtype == torch.int64


def _smplx(c):
    return types.SimpleNamespace(transform_mat=_g(c["A"]), vertices=_g(c.get("body")))


def _run(name, with_T=True, W=None, verts=None):
    """a skinning case through Reposer -> (pnts, T, W)"""
    c = rc.skin_case(name)
    searched = c["W"] is None
    rp = R.Reposer(_g(c["lbs"]) if searched else torch.zeros(12, c["A"].shape[1], device=DEV))
    verts = _g(c["verts"]) if verts is None else verts
    W = (None if searched else _g(c["W"])) if W is None else W
    if c["direction"] == "pose":
        pnts, T = rp.transform_to_pose(verts, W, _smplx(c), _g(c["transl"]), _g(c["scale"]), with_T=with_T)
        return pnts, T, W
    return rp.transform_to_t_pose(verts, _smplx(c), _g(c["transl"]), _g(c["scale"]), lbs_w=W, k=c.get("k", 10), v_normals=_g(c.get("normals")),
                                  smplx_normals=_g(c.get("body_normals")), normal_weight=rc.NORMAL_WEIGHT, with_T=with_T)


@pytest.mark.parametrize("name", rc.ALL_SKIN)
def test_skin_against_float64(name):
    c, want = rc.skin_case(name), rc.skin64(name)
    B, P, J = c["A"].shape[0], c["verts"].shape[1], c["A"].shape[1]
    pnts, T, W = _run(name)
    assert pnts.shape == (1, B, P, 3) and T.shape == (1, B, P, 4, 4)
    assert all(t.dtype == torch.float32 and t.is_cuda and not t.requires_grad for t in (pnts, T, W))
    got = {"pnts": pnts, "T": T}
    if name in rc.SEARCHED_CASES:
        assert W.shape == (B, P, J)
        got["W"] = W
        rp = R.Reposer(_g(c["lbs"]))
        dists, idx = rp.find_k_closest_verts(_g(c["verts"]), _g(c["body"]), c["k"], _g(c["normals"]), _g(c["body_normals"]), rc.NORMAL_WEIGHT)
        assert idx.dtype == torch.int64 and idx.shape == dists.shape == (B, P, c["k"])
        assert np.array_equal(idx.cpu().numpy(), np.load(GOLD)[f"{name}_idx"])                       # every row
        got["dists"] = dists
        weights, idx2 = rp.weights_from_k_closest_verts(_g(c["verts"]), _g(c["body"]), c["k"], _g(c["normals"]), _g(c["body_normals"]),
                                                        rc.NORMAL_WEIGHT, p=2)
        err = rc.rel(weights.cpu().numpy(), rc.tw.shepard(torch.tensor(want["dists"]), 2).numpy())
        print(name, "weights %.3g of bound %.3g" % (err, rc.BOUND))
        assert torch.equal(idx2, idx) and weights.shape == (B, P, c["k"]) and err <= rc.BOUND
    else:
        assert W.shape == c["W"].shape                                             # what was passed in
    for k, t in got.items():
        err = rc.rel(t.cpu().numpy(), want[k])
        print(name, k, "%.3g of bound %.3g" % (err, rc.BOUND))
        assert torch.isfinite(t).all() and err <= rc.BOUND, k


@pytest.mark.parametrize("name", ["pose_a", "tpose_a", "tpose_sum", "tpose_knn"])
def test_same_bits_without_T_with_repeated_W_and_on_a_second_run(name):
    c = rc.skin_case(name)
    B = c["A"].shape[0]
    pnts, T, W = _run(name)
    again = _run(name)
    assert _same_bits(again[0], pnts) and _same_bits(again[1], T) and _same_bits(again[2], W)
    bare = _run(name, with_T=False)
    assert bare[1] is None and _same_bits(bare[0], pnts)
    if c["W"] is not None and c["W"].shape[0] == 1 and B > 1:
        rep = _run(name, W=_g(c["W"]).repeat(B, 1, 1))
        assert _same_bits(rep[0], pnts) and _same_bits(rep[1], T)
        one = _run(name, W=_g(c["W"]), verts=_g(c["verts"][:1]))                   # vertices [1, P, 3] serve every frame too
        rep = _run(name, W=_g(c["W"]), verts=_g(c["verts"][:1]).repeat(B, 1, 1))
        assert _same_bits(one[0], rep[0]) and _same_bits(_run(name, W=_g(c["W"]), verts=_g(c["verts"][0]))[0], one[0])


@pytest.mark.parametrize("name", ["tpose_a", "tpose_b", "tpose_sum"])
def test_round_trip(name):
    """to the T-pose and back to the same pose.  The way back is held to BOUND against the float64 twin on the very points it was
    given; the whole trip returns rc.round_trip_expected -- the input itself where the rows of W sum to 1 -- within
    BOUND * (1 + 1.5 max|t-pose| / max|input|): the second step's own error, plus the first step's error carried through a map of
    norm at most (sum of |w|) * scale <= 1.2 * 1.25."""
    c = rc.skin_case(name)
    rp = R.Reposer(torch.zeros(12, c["A"].shape[1], device=DEV))
    t_pnts, _, W = _run(name)
    back, _ = rp.transform_to_pose(t_pnts[0], W, _smplx(c), _g(c["transl"]), _g(c["scale"]))
    twin = rc.skin_twin(dict(c, direction="pose", verts=t_pnts[0].cpu().numpy().astype(np.float64)))["pnts"]
    step = rc.rel(back.cpu().numpy(), twin)
    trip = rc.rel(back[0].cpu().numpy(), rc.round_trip_expected(name))
    bound = rc.BOUND * (1 + 1.5 * float(t_pnts.abs().max()) / float(np.abs(c["verts"]).max()))
    print(name, "way back %.3g of %.3g; round trip %.3g of %.3g" % (step, rc.BOUND, trip, bound))
    assert step <= rc.BOUND and trip <= bound
    if name != "tpose_sum":
        assert rc.rel(back[0].cpu().numpy(), c["verts"].astype(np.float64)) <= bound + 5e-7         # rows of W sum to 1 within 1e-7


def test_outputs_carry_no_graph():
    c = rc.skin_case("tpose_knn")
    leaf = lambda a: _g(a).requires_grad_(True)
    rp = R.Reposer(leaf(c["lbs"]))
    smplx = types.SimpleNamespace(transform_mat=leaf(c["A"]), vertices=leaf(c["body"]))
    outs = list(rp.transform_to_t_pose(leaf(c["verts"]), smplx, leaf(c["transl"]), leaf(c["scale"]), k=c["k"], v_normals=leaf(c["normals"]),
                                       smplx_normals=leaf(c["body_normals"])))
    outs += list(rp.transform_to_pose(outs[0][0], outs[2].clone().requires_grad_(True), smplx, leaf(c["transl"]), leaf(c["scale"])))
    outs += list(rp.transform_to_t_pose(leaf(c["verts"]), smplx, leaf(c["transl"]), leaf(c["scale"]), lbs_w=outs[2].clone().requires_grad_(True)))
    outs += list(R.knn_points(leaf(c["verts"]), leaf(c["body"]), K=3)) + list(R.knn_self(leaf(c["verts"][0]), 3))
    outs += list(rp.weights_from_k_closest_verts(leaf(c["verts"]), leaf(c["body"]), 4))
    assert len(outs) == 14 and all(t.grad_fn is None and not t.requires_grad for t in outs)


def test_input_checks_raise_before_any_launch():
    c = rc.skin_case("tpose_knn")
    v, body, A, lbs, tr, sc = (_g(c[k]) for k in ("verts", "body", "A", "lbs", "transl", "scale"))
    rp = R.Reposer(lbs)
    smplx = types.SimpleNamespace(transform_mat=A, vertices=body)
    W = torch.rand(2, 257, 55, device=DEV)
    bad = [lambda: R.knn_points(v, body, K=0), lambda: R.knn_points(v, body, K=17), lambda: R.knn_points(v, body[:, :5], K=6),
           lambda: R.knn_points(v, body, K=2.0), lambda: R.knn_points(v.double(), body, K=1), lambda: R.knn_points(v.cpu(), body, K=1),
           lambda: R.knn_points(v[0], body[0], K=1), lambda: R.knn_points(v, body[:1], K=1), lambda: R.knn_points(v[..., :2], body[..., :2], K=1),
           lambda: R.knn_points(v, torch.cat([body, body], -1), K=1), lambda: R.knn_points(v, body[:, :0], K=1),
           lambda: R.knn_points(v, body, K=1, slices=-1), lambda: R.knn_points(v.cpu().numpy(), body, K=1),
           lambda: R.knn_self(v[0], 0), lambda: R.knn_self(v[0], 16), lambda: R.knn_self(v[0, :3], 3), lambda: R.knn_self(v, 3),
           lambda: R.Reposer(lbs.cpu()), lambda: R.Reposer(lbs[0]), lambda: R.Reposer(torch.zeros(4, 128, device=DEV)), lambda: R.Reposer(lbs[:0]),
           lambda: rp.find_k_closest_verts(v, body, 0), lambda: rp.find_k_closest_verts(v, body, 3, points_normals=v[:, :5]),
           lambda: rp.weights_from_k_closest_verts(v, body, 3, p=-1), lambda: rp.weights_from_k_closest_verts(v, body, 3, p=1.5),
           lambda: rp.transform_to_t_pose(v, smplx, None, sc), lambda: rp.transform_to_t_pose(v, smplx, tr, None),
           lambda: rp.transform_to_t_pose(v, smplx, tr, sc, k=17), lambda: rp.transform_to_t_pose(v, smplx, tr[:1].repeat(3, 1), sc),
           lambda: rp.transform_to_t_pose(v, smplx, tr, torch.ones(3, device=DEV)), lambda: rp.transform_to_t_pose(v, smplx, tr, 1.0),
           lambda: rp.transform_to_t_pose(v, types.SimpleNamespace(transform_mat=A[:, :54], vertices=body), tr, sc),
           lambda: rp.transform_to_t_pose(v, types.SimpleNamespace(transform_mat=A, vertices=body[:, :299]), tr, sc),
           lambda: rp.transform_to_t_pose(v, types.SimpleNamespace(transform_mat=A), tr, sc),
           lambda: rp.transform_to_t_pose(v[:, :256], smplx, tr, sc, lbs_w=W), lambda: rp.transform_to_t_pose(v, smplx, tr, sc, lbs_w=W[..., :54]),
           lambda: rp.transform_to_pose(v, W[0], smplx), lambda: rp.transform_to_pose(v, W.double(), smplx),
           lambda: rp.transform_to_pose(v, torch.rand(3, 257, 55, device=DEV), smplx), lambda: rp.transform_to_pose(v[..., :2], W, smplx),
           lambda: rp.transform_to_pose(v, W, smplx, tr[:, :2]), lambda: rp.transform_to_pose(v, W, smplx, tr, sc.reshape(1, 1)),
           lambda: rp.transform_to_pose(v, W, types.SimpleNamespace(transform_mat=A.reshape(2, 55, 16)))]
    for n, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"input check {n} did not fire")


def test_non_contiguous_inputs_and_a_side_stream():
    c = rc.skin_case("pose_c")
    want = _run("pose_c")
    rp = R.Reposer(torch.zeros(12, 55, device=DEV))
    strided = lambda a: torch.stack([_g(a), _g(a)], -1)[..., 0]                    # the same values with a stride of 2
    v, W, A, tr = strided(c["verts"]), strided(c["W"]), strided(c["A"]), strided(c["transl"])
    assert not v.is_contiguous() and not W.is_contiguous() and not A.is_contiguous()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pnts, T = rp.transform_to_pose(v, W, types.SimpleNamespace(transform_mat=A), tr, None)
        k = rc.knn_case("main")
        found = R.knn_points(strided(k["p1"])[None], strided(k["p2"])[None], K=k["K"])
    side.synchronize()
    assert _same_bits(pnts, want[0]) and _same_bits(T, want[1])
    assert np.array_equal(found.idx[0].cpu().numpy(), np.load(GOLD)["main_idx"])
