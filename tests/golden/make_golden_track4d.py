"""Golden vectors for the scale-ratio terms FROM THE REFERENCE'S OWN FUNCTION (tests/golden/track4d.npz).

``scale_ratio_loss`` (preprocess/train_mesh_lbs_4ddress.py:279-292) is cut out of the reference's file with ``ast`` at generation time
and executed unchanged; this script contains none of its text.  Everything in float64 on the float32 inputs of the small cases of
tests/track4d_cases.py (FIXTURE_CASES): the three values with the thresholds of :361, and the gradient of each to ``verts`` and to
``scale`` (the first term does not read ``verts``).  The Laplacian term has no such pin: its matrix comes from pytorch3d, which is
not installed where this runs (UNCONFIRMED, tests/track4d_twin_torch.py).
Data only: expected outputs.
    python tests/golden/make_golden_track4d.py        (needs the reference checkout that make_golden_raster.py names)"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import track4d_cases as t4  # noqa: E402
from make_golden_raster import REF, cut  # noqa: E402


def main():
    fn = cut(os.path.join(REF, "preprocess", "train_mesh_lbs_4ddress.py"), ["scale_ratio_loss"], {"torch": torch})["scale_ratio_loss"]
    d = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    out = {}
    for name in t4.FIXTURE_CASES:
        c = t4.case(name)
        faces, v, s = torch.from_numpy(c["faces"].astype(np.int64)), d(c["verts"]).requires_grad_(True), d(c["scale"]).requires_grad_(True)
        terms = fn(v, faces, s, scale_ratio_th=t4.TH[0], scale_edge_ratio_th=t4.TH[1])
        grad = lambda y, x: torch.autograd.grad(y, x, retain_graph=True)[0].numpy()
        out.update({f"{name}_{k}": t.detach().numpy() for k, t in zip(t4.SCALE_VALUES, terms)})
        out.update({f"{name}_d_ratio_scale": grad(terms[0], s), f"{name}_d_edge_verts": grad(terms[1], v), f"{name}_d_edge_scale": grad(terms[1], s),
                    f"{name}_d_var_verts": grad(terms[2], v), f"{name}_d_var_scale": grad(terms[2], s)})
    path = os.path.join(HERE, "track4d.npz")
    np.savez_compressed(path, **out)
    print("track4d.npz: %d bytes" % os.path.getsize(path), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
