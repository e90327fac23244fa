"""jet_backward_speed.py: what a residual written with compute_gradient costs against a hard-wired one.
(a) Engine.jet_backward (gY and gdY given) on the GENERIC engine and on FUSED (the tile kernel's external-adjoint
    instances), (b) Engine.residual_loss_grad on FUSED for the same network and points, at N = 2^14, 2^17, 2^20;
(c) one physics_equation(corrected=True) forward + backward() through the drop-in face at 2^20 points.
HIP-event times after a warm-up call.  Prints one JSON line per row and writes them all to the path given as the first
argument (optional).  PINN_HIP_LIB=<another build of the library> measures that build with the same script (a build
that knows no MFMA jet_backward runs it on the generic engine whatever the descriptor says)."""
import json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec, physics
from pinn_depthestimation_amd.dnn import DNN, init_flat_params
from pinn_depthestimation_amd._lib import ENGINE_FUSED, ENGINE_GENERIC

CASES = (("3->8x64->4 k=3", NetDesc(3, 4, 8, 64, (0, 1, 2)), "Navier_Stokes", ("t", "x", "y"), ("h", "z", "u", "v")),
         ("2->10x10->6 k=2", NetDesc(2, 6, 10, 10, (0, 1)), "physics_equation", ("x", "y"), ("h", "U", "V", "eta_mean", "Hrms", "k")),
         ("2->100x20->3 k=2", NetDesc(2, 3, 100, 20, (0, 1)), "continuity_ftemp", ("x", "y"), ("U", "V", "h")))
SIZES = (1 << 14, 1 << 17, 1 << 20)


def timed(call, reps):
    call(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): call()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


rows = []
only = os.environ.get("JB_ONLY", "abc")
for tag, desc, res, inn, outn in CASES if ("a" in only or "b" in only) else ():
    for N in SIZES:
        g = torch.Generator().manual_seed(3)
        X = (torch.rand(N, desc.d_in, generator=g) * 2 - 1).cuda()
        params = init_flat_params(desc.layers, "xavier", g).cuda()
        if res == "physics_equation":
            params[desc.n_params - desc.d_out + 0] = 0.75
            params[desc.n_params - desc.d_out + 3] = 0.0
        gY = torch.randn(N, desc.d_out, device="cuda") / N
        gdY = torch.randn(desc.k, N, desc.d_out, device="cuda") / N
        grad = torch.zeros(desc.n_params, device="cuda")
        row = {"case": tag, "N": N}
        reps = 10 if N < (1 << 20) else 3
        if "a" in only:
            for name, engine in (("generic", ENGINE_GENERIC), ("fused", ENGINE_FUSED)):
                eng = Engine(desc.with_(engine=engine))
                row[f"jet_backward_{name}_ms"] = round(timed(lambda: eng.jet_backward(params, X, gY, gdY, grad), reps), 4)
                del eng
                torch.cuda.empty_cache()
            row["generic_over_fused"] = round(row["jet_backward_generic_ms"] / row["jet_backward_fused_ms"], 2)
        if "b" in only:
            eng = Engine(desc.with_(engine=ENGINE_FUSED))
            spec = ResidualSpec.from_names(res, inn, desc.grad_cols, outn)
            scale = torch.full((spec.n_terms,), 1.0 / N, device="cuda")
            row["residual_loss_grad_fused_ms"] = round(timed(lambda: eng.residual_loss_grad(spec, scale, params, X, grad), reps), 4)
            if "a" in only:
                row["jet_backward_fused_over_residual"] = round(row["jet_backward_fused_ms"] / row["residual_loss_grad_fused_ms"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)

if "c" in only:
    for tag, layers in (("2->10x10->6", [2] + [10] * 10 + [6]), ("2->8x64->6", [2] + [64] * 8 + [6])):
        N = 1 << 20
        torch.manual_seed(3)
        model = DNN(layers, 0.0, "xavier").to("cuda")
        last = [m for m in model.modules() if isinstance(m, torch.nn.Linear)][-1]
        with torch.no_grad():
            last.bias[0] = 2.0; last.bias[4] = 0.2; last.bias[5] = 1.0
        Xh = (torch.rand(N, 2, generator=torch.Generator().manual_seed(5)) * 2 - 1).cuda()

        def step():
            x, y = [Xh[:, i:i + 1].clone().requires_grad_(True) for i in range(2)]
            pred = model(torch.cat([x, y], -1))
            loss = physics.physics_equation(x, y, *[pred[:, i:i + 1] for i in range(6)], corrected=True)
            model.zero_grad()
            loss.backward()

        row = {"case": f"physics_equation(corrected=True) forward + backward, {tag}", "N": N, "step_ms": round(timed(step, 3), 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)

if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(rows, f, indent=1)
