"""Records tests/golden/mil_reference.npz: the outputs of the REFERENCE's own models/model_mil.py (MIL_fc, MIL_fc_mc with 3 classes), run on
the CPU on the weights and the bag of tests/mil_ref.py.

    python tools/record_mil_golden.py --reference /path/to/HIPT_ABMIL_ATEC23

The reference's module imports ``utils.utils`` for ``initialize_weights`` only, and that module imports torchvision; a stand-in module
that supplies that one function is put into ``sys.modules`` first.  The [512, 1024] weights are not stored: the test draws them again
from mil_ref's seeded PCG64 stream and checks the float64 checksum stored here, so a drifted stream fails loudly.  No test reads the
reference tree: only this tool does."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mil_ref as R  # noqa: E402

N_ROWS, PLANTED = 33, 32


def initialize_weights(module):
    for m in module.modules():
        if isinstance(m, nn.Linear):
            nn.init.xavier_normal_(m.weight)
            m.bias.data.zero_()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mil_reference.npz"))
    args = ap.parse_args()
    pkg, stub = types.ModuleType("utils"), types.ModuleType("utils.utils")
    stub.initialize_weights = initialize_weights
    pkg.utils = stub
    sys.modules["utils"], sys.modules["utils.utils"] = pkg, stub
    spec = importlib.util.spec_from_file_location("ref_model_mil", os.path.join(args.reference, "models", "model_mil.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {"n_rows": np.int64(N_ROWS), "planted": np.int64(PLANTED)}
    for C in (2, 3):
        multi = C > 2
        p = R.weights(C)
        m = ref.MIL_fc_mc(n_classes=C) if multi else ref.MIL_fc()
        m.load_state_dict(R.state_dict(p, multi), strict=True)
        m.eval()
        x = R.bag(N_ROWS, N_ROWS, PLANTED, p, multi)
        with torch.no_grad():
            top, Y_prob, Y_hat, y_probs, _ = m(torch.from_numpy(x))
        out.update({f"c{C}_top_instance": top.numpy(), f"c{C}_Y_prob": Y_prob.numpy(), f"c{C}_Y_hat": Y_hat.numpy(), f"c{C}_y_probs": y_probs.numpy(),
                    f"c{C}_checksum": np.float64(R.checksum(p)), f"c{C}_bag_checksum": np.float64(np.asarray(x, np.float64).sum())})
    np.savez(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
