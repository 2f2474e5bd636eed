# Overlay for a reference checkout: replaces models/model_mil.py with the gfx950 implementation.
from hipt_abmil_atec23_amd.model_mil import *  # noqa: F401,F403
from hipt_abmil_atec23_amd import model_mil as _impl
globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
