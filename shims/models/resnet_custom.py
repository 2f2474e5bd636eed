# Overlay for a reference checkout: replaces models/resnet_custom.py with the gfx950 implementation (ResNet-50 baseline).
from hipt_abmil_atec23_amd.resnet_custom import *  # noqa: F401,F403
from hipt_abmil_atec23_amd import resnet_custom as _impl
globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
