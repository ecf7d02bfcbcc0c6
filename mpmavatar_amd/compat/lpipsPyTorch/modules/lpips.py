"""``from lpipsPyTorch.modules.lpips import LPIPS``: the module of mpmavatar_amd/lpips.py, constructed with its weights as the
reference's constructor is (there from a download, here from the files MPMHIP_LPIPS_VGG16 and MPMHIP_LPIPS_LIN name)."""
from mpmavatar_amd import lpips as _lpips


class LPIPS(_lpips.LPIPS):
    def __new__(cls, net_type: str = "alex", version: str = "0.1"):
        return _lpips.LPIPS.from_environment(net_type, version)
