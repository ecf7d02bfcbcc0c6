"""The product's device math header (mpmavatar_amd/csrc/mpm_math.hpp) on the CPU, against the reference-produced fixtures.

mpm_math.hpp is plain per-particle C++ (no memory traffic); compiled with g++ over a 20-line stand-in for
<hip/hip_runtime.h> it runs on the host.  The oracle's test hooks (oracle/mpm_oracle.c: orc_hook_element /
orc_hook_traditional) let it take the place of the oracle's own constitutive restatement inside the oracle's substep, so
the ARITHMETIC THE GPU KERNELS USE -- QR, return mappings, Kirchhoff stresses, the Jacobi SVD -- is checked here, without
a GPU, against sequences the reference's own source produced (tests/golden/ref_seq_*.npz).  Those sequences start from rest
and stay near well-conditioned states; the same host builds are held to float64, function by function (svd3 itself
included), at the shapes and thresholds where the update branches by tests/test_constitutive_edges.py.  What no host build
can see: FMA contraction as hipcc applies it (the host build is contraction-free, like the oracle; a second build with
g++'s contraction on brackets it), v_rcp / v_rsq being 1-ulp approximations on the device, and the wave-wide vote that ends
svd3's sweep loop (the stub's __any has one lane) -- tests/test_gpu_constitutive_edges.py runs the same edge table through
the kernels for those.

This is the test that found the round-1/2 Gram-Schmidt QR (q2 = q0 x q1, not re-normalised) to be biased at the r22 = 1
discontinuity of the cloth return mapping (mpm_utils.py:196-204): 2.7x further from the reference than the Givens QR of
wp.qr3 as the oracle restates it; `test_gram_schmidt_qr_is_the_outlier` keeps that witness.
"""
import ctypes as C

import numpy as np
import pytest

import refgolden as rg
from hostbuild import host_lib


ELEM = C.CFUNCTYPE(None, *([C.POINTER(C.c_float)] * 2 + [C.c_float] * 6 + [C.POINTER(C.c_float)] * 5))
TRAD = C.CFUNCTYPE(None, C.POINTER(C.c_float), C.c_int, *([C.c_float] * 6 + [C.POINTER(C.c_float)] * 5))


def _build(contract):
    flags = ["-ffp-contract=off"] if contract == "off" else ["-ffp-contract=fast", "-mfma"]
    return host_lib("hostmath", name=f"hostmath_{contract}", flags=["-Wno-unknown-pragmas", *flags])


@pytest.fixture(scope="module")
def hm():
    return {"off": _build("off"), "fma": _build("fma")}


class hooked:
    """Run the oracle with the header's constitutive functions in place of its own (always restored)."""

    def __init__(self, lib, element="hm_element", traditional="hm_traditional"):
        from oracle import oracle as oo
        self.olib = oo._load(False)
        self.fe = C.cast(getattr(lib, element), C.c_void_p) if element else C.c_void_p(0)
        self.ft = C.cast(getattr(lib, traditional), C.c_void_p) if traditional else C.c_void_p(0)

    def __enter__(self):
        C.c_void_p.in_dll(self.olib, "orc_hook_element").value = self.fe.value
        C.c_void_p.in_dll(self.olib, "orc_hook_traditional").value = self.ft.value

    def __exit__(self, *a):
        C.c_void_p.in_dll(self.olib, "orc_hook_element").value = None
        C.c_void_p.in_dll(self.olib, "orc_hook_traditional").value = None


def _follow(name, upto=None):
    """(checkpoint, v distance to the reference, bound from the reference's own envelope, x distance) per checkpoint."""
    from oracle.scene_adapter import oracle_from_scene
    z = rg.load(name)
    sc = rg.scene_from_npz(z)
    o = oracle_from_scene(sc)
    done, out = 0, []
    for cp in z["checkpoints"]:
        if upto is not None and int(cp) > upto:
            break
        for k in range(done, int(cp)):
            o.p2g2p(sc.dt, **rg.step_inputs(sc, k))
        done = int(cp)
        out.append((int(cp), rg.rel(o.v, z[f"s{cp}_particle_v"]), rg.seq_bound(z, cp), rg.rel(o.x, z[f"s{cp}_particle_x"]),
                    rg.rel_pp(o.v, z[f"s{cp}_particle_v"])))
    return out


SEQS = rg.names("seq")


@pytest.mark.parametrize("contract", ["off", "fma"])
@pytest.mark.parametrize("name", SEQS)
def test_device_math_follows_the_reference_sequences(name, contract, hm):
    strict = name.endswith(("_jelly", "_gamma0"))
    with hooked(hm[contract]):
        rows = _follow(name)
    for cp, ev, bound, ex, evpp in rows:
        assert ex < 1e-4, f"{name}[{contract}] substep {cp}: x {ex:.2e}"
        b = 1e-4 if strict else bound
        assert ev < b, f"{name}[{contract}] substep {cp}: v {ev:.2e} (bound {b:.2e})"
        if strict:
            assert evpp < 1e-4, f"{name}[{contract}] substep {cp}: per-particle v {evpp:.2e}"


def test_gram_schmidt_qr_is_the_outlier(hm):
    """Same scene, same everything, only the QR algorithm of the cloth path swapped: the Givens form (shipped, = the oracle's =
    wp.qr3's) ends inside the reference's own envelope, the Gram-Schmidt form of rounds 1-2 >= 2x outside the Givens distance."""
    name = "ref_seq_sheet"
    with hooked(hm["off"]):
        giv = _follow(name)[-1]
    with hooked(hm["off"], element="hm_element_gram_schmidt"):
        gs = _follow(name)[-1]
    assert giv[1] < giv[2], giv
    assert gs[1] > 2.0 * giv[1], (gs, giv)


def test_qr_is_the_oracles_bit_for_bit(hm):
    from oracle import oracle as oo
    lib = hm["off"]
    rng = np.random.default_rng(5)
    fp = C.POINTER(C.c_float)
    worst = 0
    for _ in range(2000):
        d = rng.normal(size=(3, 3)).astype(np.float32)
        if rng.random() < 0.3:  # near-rest cloth: orthogonal edges, unit normal
            d = (np.linalg.qr(rng.normal(size=(3, 3)))[0] @ np.diag([0.01, 0.02, 1.0]) + 1e-7 * rng.normal(size=(3, 3))).astype(np.float32)
        Q, R = oo.qr_signfixed(d)
        Q2, R2 = np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32)
        lib.hm_qr(np.ascontiguousarray(d).ctypes.data_as(fp), Q2.ctypes.data_as(fp), R2.ctypes.data_as(fp))
        worst = max(worst, int(np.abs(Q.view(np.int32) - Q2.view(np.int32)).max()), int(np.abs(np.triu(R).view(np.int32) - np.triu(R2).view(np.int32)).max()))
    assert worst == 0, f"Givens QR of mpm_math.hpp differs from the oracle's by {worst} ulp"
