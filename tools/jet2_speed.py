"""jet2_speed.py: Engine.forward_jet2 + Engine.jet2_backward (all three adjoints) per call on both jet2 engines (FUSED:
the MFMA layer kernels, AUTO's choice at these shapes; GENERIC: the VALU layer kernels) at the three reference shapes.
Prints one line per case and writes them as JSON to the path given as the first argument (optional)."""
import json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from pinn_depthestimation_amd import Engine, NetDesc
from pinn_depthestimation_amd.dnn import init_flat_params
from pinn_depthestimation_amd._lib import ENGINE_FUSED, ENGINE_GENERIC

CASES = (("3->8x64->4 k=3", NetDesc(3, 4, 8, 64, (0, 1, 2)), 1 << 20),
         ("2->10x10->6 k=2", NetDesc(2, 6, 10, 10, (0, 1)), 1 << 20),
         ("2->100x20->3 k=2", NetDesc(2, 3, 100, 20, (0, 1)), 12514))
rows = []
for (tag, desc, N), (ename, engine) in [(c, e) for c in CASES for e in (("mfma", ENGINE_FUSED), ("generic", ENGINE_GENERIC))]:
    g = torch.Generator().manual_seed(3)
    X = (torch.rand(N, desc.d_in, generator=g) * 2 - 1).cuda()
    params = init_flat_params(desc.layers, "xavier", g).cuda()
    eng = Engine(desc.with_(engine=engine))
    P = desc.k * (desc.k + 1) // 2
    gY = torch.randn(N, desc.d_out, device="cuda")
    gdY = torch.randn(desc.k, N, desc.d_out, device="cuda")
    gd2Y = torch.randn(P, N, desc.d_out, device="cuda")
    grad = torch.zeros(desc.n_params, device="cuda")
    reps = 3
    times = {}
    for what in ("forward_jet2", "jet2_backward"):
        call = (lambda: eng.forward_jet2(params, X)) if what == "forward_jet2" else \
               (lambda: eng.jet2_backward(params, X, gY, gdY, gd2Y, grad))
        call(); torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps): call()
        b.record(); torch.cuda.synchronize()
        times[what] = a.elapsed_time(b) / reps
    row = {"case": tag, "engine": ename, "N": N, "forward_jet2_ms": round(times["forward_jet2"], 3),
           "jet2_backward_ms": round(times["jet2_backward"], 3),
           "total_ms": round(times["forward_jet2"] + times["jet2_backward"], 3),
           "workspace_MiB": round(eng.jet2_workspace(N).numel() / 2 ** 20, 1)}
    rows.append(row)
    print(json.dumps(row), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(rows, f, indent=1)
