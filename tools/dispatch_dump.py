"""dispatch_dump.py OUT: the C-ABI's host-side dispatch (tests/dispatch_walk_util.py) as text, one line per probe: return
code, value returned and pinn_last_error() of every query and call over the grid of descriptors.  PINN_HIP_LIB selects the
library; dump two builds and diff the files to see whether a change to the host code moved any decision or message.
The probes with non-NULL arrays are host logic only without a GPU: they are left out where one is visible."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                            # noqa: E402
from tests import dispatch_walk_util as W               # noqa: E402
from pinn_depthestimation_amd import _lib               # noqa: E402

with open(sys.argv[1], "w") as f:
    n = 0
    for line in W.dump_lines(_lib.load(), with_dummy=not torch.cuda.is_available()):
        f.write(line + "\n")
        n += 1
print(f"{n} probes of {_lib.LIB_PATH} -> {sys.argv[1]}")
