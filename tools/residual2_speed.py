"""residual2_speed.py [OUT.json]: one loss + gradient of the residual with the lateral-mixing term -nu lap(U), three ways, in
one process and alternating (round-robin over the routes, median of the rounds):
  (a) formula   DNN.forward, the formula with nested compute_gradient (forward_jet2), loss.backward() (jet2_backward):
                what the commit before pinn_residual2_loss_grad does
  (b) generic   Engine.residual2_loss_grad on the VALU layer kernels and k2_wgrad
  (c) mfma      Engine.residual2_loss_grad on the MFMA layer kernels and k2m_wgrad
Shapes: 3 -> 8 x 64 -> 4 Navier_Stokes and 2 -> 10 x 10 -> 6 physics_equation at 2^14, 2^17 and 2^20 points.
Default output: profiles/r06/residual2_speed.json."""
import json, os, statistics, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec, physics
from pinn_depthestimation_amd.dnn import DNN
from pinn_depthestimation_amd._lib import ENGINE_FUSED, ENGINE_GENERIC

NU, ROUNDS = 0.05, 5
CASES = (("3->8x64->4 Navier_Stokes", "Navier_Stokes", NetDesc(3, 4, 8, 64, (0, 1, 2)), ("t", "x", "y"), ("h", "z", "u", "v")),
         ("2->10x10->6 physics_equation", "physics_equation", NetDesc(2, 6, 10, 10, (0, 1)), ("x", "y"),
          ("h", "U", "V", "eta_mean", "Hrms", "k")))
SIZES = (1 << 14, 1 << 17, 1 << 20)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)


rows = []
for tag, res, desc, ins, outs in CASES:
    for N in SIZES:
        torch.manual_seed(3)
        model = DNN(desc.layers, 0.0, "xavier").to("cuda")
        with torch.no_grad():                       # depths away from zero (physics_equation divides by eta + h)
            b = model._ordered_params()[-1]
            b[outs.index("h")] = 2.0
            if "eta_mean" in outs:
                b[outs.index("eta_mean")] = 0.2
        X = (torch.rand(N, desc.d_in, generator=torch.Generator().manual_seed(4)) * 2 - 1).cuda()
        flat = model.flat_params()
        spec = ResidualSpec.from_names(res, ins, desc.grad_cols, outs, nu=NU)
        scale = torch.full((3,), 1.0 / N, device="cuda")
        engines = {"generic": Engine(desc.with_(engine=ENGINE_GENERIC)), "mfma": Engine(desc.with_(engine=ENGINE_FUSED))}
        grad = torch.zeros_like(flat)

        def formula():
            cols = [X[:, i:i + 1].clone().requires_grad_(True) for i in range(desc.d_in)]
            pred = model(torch.cat(cols, -1))
            # (x 1.0: plain tensors, so the drop-in function evaluates the formula instead of the hard-wired entry)
            loss = getattr(physics, res)(*cols, *[pred[:, i:i + 1] * 1.0 for i in range(len(outs))], nu=NU)
            model.zero_grad()
            loss.backward()

        routes = {"formula": formula,
                  "generic": lambda: engines["generic"].residual2_loss_grad(spec, scale, flat, X, grad=grad),
                  "mfma": lambda: engines["mfma"].residual2_loss_grad(spec, scale, flat, X, grad=grad)}
        for fn in routes.values():
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in routes}
        for _ in range(ROUNDS):
            for k, fn in routes.items():
                t[k].append(timed(fn))
        row = {"case": tag, "N": N, "nu": NU, "rounds": ROUNDS}
        for k in routes:
            row[k + "_ms"] = round(statistics.median(t[k]), 3)
            row[k + "_min_ms"], row[k + "_max_ms"] = round(min(t[k]), 3), round(max(t[k]), 3)
        row["mfma_over_formula"] = round(row["mfma_ms"] / row["formula_ms"], 3)
        row["mfma_over_generic"] = round(row["mfma_ms"] / row["generic_ms"], 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del model, X, engines, grad
        torch.cuda.empty_cache()
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r06", "residual2_speed.json")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump(rows, f, indent=1)
