"""Optional: ``from diff_gauss import GaussianRasterizationSettings, GaussianRasterizer`` for an UNEDITED
``gaussian_renderer/__init__.py`` of the reference on a machine without the CUDA extension.

Put ``mpmavatar_amd/compat`` on PYTHONPATH.  These are the two names of ``mpmavatar_amd/rasterizer.py``, nothing more: the
forward pass, and the backward pass when an input other than ``means2D`` requires grad: the render call and
``loss.backward()`` of ``train_appearance.py`` work, ``viewspace_point_tensor.grad`` included.  ``extra_attrs=`` [N, E <= 8] comes
back blended as the sixth value, with gradients, as ``preprocess/train_mesh_lbs_4ddress.py`` (:260-277, :299, :306) uses it; the
depth and normal slots stay ``None``.  Still not supported:
``BoundGaussians.render_inputs`` is a forward-only launch, so gradients stop at its outputs; densification is the caller's.
"""
from mpmavatar_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer  # noqa: F401
