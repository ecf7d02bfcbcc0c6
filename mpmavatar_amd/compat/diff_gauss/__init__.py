"""Optional: ``from diff_gauss import GaussianRasterizationSettings, GaussianRasterizer`` for an UNEDITED
``gaussian_renderer/__init__.py`` of the reference on a machine without the CUDA extension.

Put ``mpmavatar_amd/compat`` on PYTHONPATH.  These are the two names of ``mpmavatar_amd/rasterizer.py``, nothing more: the
forward pass only (no backward; ``train_appearance.py`` cannot use it).
"""
from mpmavatar_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer  # noqa: F401
