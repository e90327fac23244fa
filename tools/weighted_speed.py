"""weighted_speed.py OUT.json [--parent-tree DIR]: what per-point weights on the residual cost per call, ms, at N = 2^14, 2^17,
2^20 on 3->8x64->4 (Navier_Stokes) and 2->10x10->6 (physics_equation), conditioned networks:
  (a) Engine.residual_weighted_loss_grad on ENGINE_FUSED_TILE with gradient and fields, w_rows = n_w — the tile kernel's
      weighted instances, this tree,
  (b) Engine.residual_loss_grad on ENGINE_FUSED_TILE: the same chain without weights,
  (c) what a build without (a) runs for the same loss: DNN forward, the residual written with compute_gradient and the weights
      multiplied in, backward() — forward jet, torch autograd, jet_backward,
  (d) (b) plus an Engine.residual_fields call: loss, gradient and residual map without (a).
(b), (c) and (d) come from a build of the PARENT commit when --parent-tree names one (a checkout with its library built), else
from this tree; each tree is measured by a fresh child process, in the same call on the same device.  Three warm-up calls,
then one HIP-event pair per call, median of 15 (min and max kept).  Writes OUT.json (default profiles/r11/weighted_speed.json)
with (a)/(b), (c)/(a) and (d)/(a); no ratio is asserted."""
import json, os, statistics, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = (("3->8x64->4 Navier_Stokes", "Navier_Stokes", [3] + [64] * 8 + [4], ("t", "x", "y"), ("h", "z", "u", "v"), 0.6,
          [2.0, 0.2, 0.0, 0.0]),
         ("2->10x10->6 physics_equation", "physics_equation", [2] + [10] * 10 + [6], ("x", "y"),
          ("h", "U", "V", "eta_mean", "Hrms", "k"), 0.05, [2.0, 0.0, 0.0, 0.2, 0.5, 1.0]))
SIZES = (1 << 14, 1 << 17, 1 << 20)
REPS = 15


def child(root, which):
    sys.path.insert(0, root)
    import torch
    from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec
    from pinn_depthestimation_amd._lib import ENGINE_FUSED_TILE
    from pinn_depthestimation_amd.dnn import DNN
    from pinn_depthestimation_amd.physics import compute_gradient as d

    def median_ms(call):
        for _ in range(3): call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); call(); b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]

    def formula(res, c, ins, outs, w):      # the user's own residual with a weight row per term
        g = 9.81
        if res == "Navier_Stokes":
            (t, x, y), (h, z, u, v) = ins, outs
            depth, cb = h + z, 3.0 / 16.0 * g * c ** 2
            f = (d(z, t) + d(depth * u, x) + d(depth * v, y),
                 d(u, t) + u * d(u, x) + v * d(u, y) + g * d(z, x) + cb * d(depth, x) * depth,
                 d(v, t) + u * d(v, x) + v * d(v, y) + g * d(z, y) + cb * d(depth, y) * depth)
        else:
            (x, y), (h, U, V, eta, _, _), rho = ins, outs, 1025
            inv = 1 / (rho * (eta + h))
            f = (d(U, x) + d(V, y),
                 U * d(U, x) + V * d(U, y) + g * d(eta, x) + inv * (rho * c * U * abs(U)),
                 U * d(V, x) + V * d(V, y) + g * d(eta, y) + inv * (rho * c * V * abs(V)))
        return sum(torch.mean(w[t].reshape(-1, 1) * q ** 2) for t, q in enumerate(f))

    for tag, res, layers, inn, outn, c0, bias in CASES:
        torch.manual_seed(3)
        model = DNN(layers, 0.0, "xavier").to("cuda")
        last = [m for m in model.modules() if isinstance(m, torch.nn.Linear)][-1]
        with torch.no_grad():
            last.weight.mul_(0.25); last.bias.copy_(torch.tensor(bias))
        k = len(inn)
        desc = NetDesc.from_layers(layers, tuple(range(k)))
        eng = Engine(desc)
        spec = ResidualSpec.from_names(res, inn, desc.grad_cols, outn)
        for N in SIZES:
            X = (torch.rand(N, k, generator=torch.Generator().manual_seed(5)) * 2 - 1).cuda()
            flat, grad = model.flat_params().detach().clone(), torch.zeros(desc.n_params, device="cuda")
            scale = torch.full((3,), 1.0 / N, device="cuda")
            row = {"case": tag, "N": N}
            w = (torch.rand(3, N, generator=torch.Generator().manual_seed(6)) * 2).cuda()
            for key in which:
                if key == "a":
                    F = torch.empty(3, N, device="cuda")
                    call = lambda: eng.residual_weighted_loss_grad(spec, w, scale, flat, X, grad, fields=F, engine=ENGINE_FUSED_TILE)[0]
                    row[key] = median_ms(call)
                    row[key + "_loss"] = float((call() * scale).sum())
                elif key == "b":
                    call = lambda: eng.residual_loss_grad(spec, scale, flat, X, grad, engine=ENGINE_FUSED_TILE)
                    row[key] = median_ms(call)
                    row[key + "_loss"] = float((call() * scale).sum())
                elif key == "d":
                    def call():
                        s_ = eng.residual_loss_grad(spec, scale, flat, X, grad, engine=ENGINE_FUSED_TILE)
                        eng.residual_fields(spec, flat, X, engine=ENGINE_FUSED_TILE)
                        return s_
                    row[key] = median_ms(call)
                else:
                    cols = [X[:, i:i + 1].clone().requires_grad_(True) for i in range(k)]
                    c = 0.78 if res == "Navier_Stokes" else 0.002

                    def step():
                        pred = model(torch.cat(cols, -1))
                        loss = formula(res, c, cols, [pred[:, list(outn).index(r):list(outn).index(r) + 1] for r in outn], w)
                        model.zero_grad(); loss.backward()
                        return loss
                    row[key] = median_ms(step)
                    row[key + "_loss"] = float(step())
            print("ROW " + json.dumps(row), flush=True)


def run_child(root, which):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, which], capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        sys.exit(f"child for {root} failed:\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    return {(r["case"], r["N"]): r for r in (json.loads(l[4:]) for l in out.stdout.splitlines() if l.startswith("ROW "))}


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        sys.exit(0)
    args = sys.argv[1:]
    parent = None
    if "--parent-tree" in args:
        i = args.index("--parent-tree"); parent = os.path.abspath(args[i + 1]); del args[i:i + 2]
    out_path = args[0] if args else os.path.join(HERE, "..", "profiles", "r11", "weighted_speed.json")
    this = os.path.abspath(os.path.join(HERE, ".."))
    bc = run_child(parent, "bcd") if parent else None
    mine = run_child(this, "a" if parent else "abcd")
    rows = []
    for key, m in mine.items():
        src = bc[key] if parent else m
        row = {"case": key[0], "N": key[1], "reps": REPS, "b_c_d_from": "parent build" if parent else "this tree",
               "a_weighted_ms": m["a"][0], "b_unweighted_ms": src["b"][0], "c_formula_ms": src["c"][0], "d_loss_plus_fields_ms": src["d"][0],
               "a_min_max_ms": m["a"][1:], "b_min_max_ms": src["b"][1:], "c_min_max_ms": src["c"][1:], "d_min_max_ms": src["d"][1:],
               "a_over_b": round(m["a"][0] / src["b"][0], 3), "c_over_a": round(src["c"][0] / m["a"][0], 2),
               "d_over_a": round(src["d"][0] / m["a"][0], 3), "loss_a": m["a_loss"], "loss_c": src["c_loss"]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
