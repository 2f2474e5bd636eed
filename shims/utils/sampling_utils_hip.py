# Overlay for a reference checkout: copy next to utils/sampling_utils.py and import it once before utils.eval_utils
# (`import utils.sampling_utils_hip`): it rebinds the two sampling functions summary_sampling calls on the reference's own
# module, whose plotting helpers stay as they are.
import hipt_abmil_atec23_amd as _amd

_amd.install(sampling=True)
