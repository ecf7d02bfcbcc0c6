"""Optional: ``from lpipsPyTorch import lpips`` (eval.py) and ``from lpipsPyTorch.modules.lpips import LPIPS``
(train_appearance.py) for UNEDITED drivers of the reference.

Put ``mpmavatar_amd/compat`` on PYTHONPATH.  These are the two names of ``mpmavatar_amd/lpips.py``; ``LPIPS("vgg")`` here and
``lpips(x, y, net_type="vgg")`` read the weights from the two files MPMHIP_LPIPS_VGG16 and MPMHIP_LPIPS_LIN name (torchvision's VGG16
state dict and the upstream vgg.pth) and raise, naming both, where they are unset: nothing is downloaded.  Only net_type 'vgg'.
"""
from mpmavatar_amd.lpips import lpips  # noqa: F401

from .modules.lpips import LPIPS  # noqa: F401
