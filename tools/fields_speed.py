"""fields_speed.py: Engine.residual_fields (pinn_residual_fields, the tile kernel's field instances) against what the
same map cost before that call existed — Engine.forward_jet plus the residual's formulas in torch — and against the
bare forward_jet, all on ENGINE_FUSED.  Shapes 3->8x64->4 (Navier_Stokes) and 2->10x10->6 (physics_equation) at
N = 2^17 and 2^20.  Three warm-up calls, then one HIP-event pair per call, median of 25.  Prints one JSON line per row
and writes them all to the path given as the first argument (optional)."""
import json, os, statistics, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec
from pinn_depthestimation_amd.dnn import init_flat_params
from pinn_depthestimation_amd._lib import ENGINE_FUSED

CASES = (("3->8x64->4", NetDesc(3, 4, 8, 64, (0, 1, 2), engine=ENGINE_FUSED), "Navier_Stokes", ("t", "x", "y"), ("h", "z", "u", "v")),
         ("2->10x10->6", NetDesc(2, 6, 10, 10, (0, 1), engine=ENGINE_FUSED), "physics_equation", ("x", "y"), ("h", "U", "V", "eta_mean", "Hrms", "k")))
REPS = 25


def median_ms(call):
    for _ in range(3): call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def torch_fields(res, Y, dY):
    """The formulas of physics.py:81-83 / 113-115 on a jet, as a user had to type them."""
    if res == "Navier_Stokes":
        h, z, u, v = Y.unbind(1)
        (_, z_t, u_t, v_t), (h_x, z_x, u_x, v_x), (h_y, z_y, u_y, v_y) = (d.unbind(1) for d in dY)
        H, Hx, Hy, cb = h + z, h_x + z_x, h_y + z_y, 3.0 / 16.0 * 9.81 * 0.78 ** 2
        return torch.stack([z_t + Hx * u + H * u_x + Hy * v + H * v_y,
                            u_t + u * u_x + v * u_y + 9.81 * z_x + cb * Hx * H,
                            v_t + u * v_x + v * v_y + 9.81 * z_y + cb * Hy * H])
    h, U, V, eta, _, _ = Y.unbind(1)
    (_, U_x, V_x, e_x, _, _), (_, U_y, V_y, e_y, _, _) = (d.unbind(1) for d in dY)
    D = 1.0 / (1025.0 * (eta + h))
    return torch.stack([U_x + V_y, U * U_x + V * U_y + 9.81 * e_x + D * (2.05 * U * U.abs()),
                        U * V_x + V * V_y + 9.81 * e_y + D * (2.05 * V * V.abs())])


rows = []
for tag, desc, res, inn, outn in CASES:
    spec = ResidualSpec.from_names(res, inn, desc.grad_cols, outn)
    eng = Engine(desc)
    g = torch.Generator().manual_seed(3)
    params = init_flat_params(desc.layers, "xavier", g).cuda()
    if res == "physics_equation":
        params[desc.n_params - desc.d_out + 0] = 0.75
        params[desc.n_params - desc.d_out + 3] = 0.0
    for N in (1 << 17, 1 << 20):
        X = (torch.rand(N, desc.d_in, generator=g) * 2 - 1).cuda()
        F = eng.residual_fields(spec, params, X)
        ref = torch_fields(res, *eng.forward_jet(params, X))
        row = {"case": tag, "residual": res, "N": N, "reps": REPS,
               "max_abs_diff_vs_torch_formulas": float((F - ref).abs().max())}
        for name, call in (("residual_fields_ms", lambda: eng.residual_fields(spec, params, X)),
                           ("forward_jet_ms", lambda: eng.forward_jet(params, X)),
                           ("forward_jet_plus_torch_formulas_ms", lambda: torch_fields(res, *eng.forward_jet(params, X)))):
            med, lo, hi = median_ms(call)
            row[name] = round(med, 4); row[name.replace("_ms", "_min_max_ms")] = [round(lo, 4), round(hi, 4)]
        row["composition_over_fields"] = round(row["forward_jet_plus_torch_formulas_ms"] / row["residual_fields_ms"], 2)
        row["fields_over_bare_jet"] = round(row["residual_fields_ms"] / row["forward_jet_ms"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)

if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(rows, f, indent=1)
