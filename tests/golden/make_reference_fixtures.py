"""Fixtures that let tests/test_host_cpu.py check files the REFERENCE makes or ships, without the reference present:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_reference_fixtures.py REFERENCE_DIR

reference_configs/*.json  The reference's four run configurations, byte for byte (data files: the test parses them
                          verbatim with pinn_depthestimation_amd.config.load_config).
ref_dnn_module.pth        torch.save of a WHOLE dnn.DNN module made by the reference's own class (what train.py:179
                          writes and test.py:37 loads): 2 -> 10x10 -> 6, xavier, dropout 0, torch.manual_seed(3).
                          torch.save normally embeds each nn.Module subclass's source text for its "source changed"
                          warning; that is switched off here, so the file holds the object's state and the class
                          NAME (dnn.DNN) only, never code.
ref_dnn_state_dict.pth    the same module's state_dict.
The module is built in a child process that imports the reference in place; nothing of it is copied.
"""
import os
import shutil
import subprocess
import sys
import zipfile

OUT = os.path.dirname(os.path.abspath(__file__))
CONFIGS = ("config_CMB.json", "config_CMB_h.json", "config.json", "config_txyz.json")

CHILD = r"""
import sys, torch, torch.serialization
sys.dont_write_bytecode = True
sys.path.insert(0, sys.argv[1])
import dnn


def no_source(obj):
    raise OSError("class source is not stored in this fixture")


torch.serialization.get_source_lines_and_file = no_source
torch.manual_seed(3)
m = dnn.DNN([2] + [10] * 10 + [6], 0.0, "xavier")
torch.save(m, sys.argv[2])
torch.save(m.state_dict(), sys.argv[3])
"""


def main(ref):
    ref = os.path.abspath(ref)
    cdir = os.path.join(OUT, "reference_configs")
    os.makedirs(cdir, exist_ok=True)
    for f in CONFIGS:
        shutil.copyfile(os.path.join(ref, f), os.path.join(cdir, f))
    mod, sd = os.path.join(OUT, "ref_dnn_module.pth"), os.path.join(OUT, "ref_dnn_state_dict.pth")
    subprocess.run([sys.executable, "-W", "ignore", "-c", CHILD, ref, mod, sd], check=True, cwd=OUT)
    with zipfile.ZipFile(mod) as z:                      # the class's code must not have travelled into the pickle
        blob = b"".join(z.read(n) for n in z.namelist())
    assert b"def forward" not in blob and ref.encode() not in blob, "class source or path leaked into the fixture"
    print("wrote", ", ".join(os.path.relpath(p, OUT) for p in [cdir, mod, sd]))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
