"""pe_wave_speed.py OUT.json --parent-tree DIR: what the wave closure's two extra terms cost per call, ms, at
N = 2^14, 2^17, 2^20 on 2->10x10->6, 2->4x32->6 and 2->8x64->6 — the three padded widths — (engine AUTO, conditioned networks: kh ~ 2, omega = 2.5, gamma = 0.42):
  (a) Engine.residual_loss_grad with ResidualSpec.corrected (three terms) from a build of the PARENT commit — DIR, a checkout
      with its library built,
  (b) Engine.residual_loss_grad with the wave closure (five terms) — the tile kernel's EPI_WAVE instances, this tree,
  (c) one drop-in step on this tree: DNN forward, physics.physics_equation(corrected=True, wave_omega=, wave_gamma=),
      backward() — forward jet, torch autograd over the formula, jet_backward: what (b) replaces.
Each tree is measured by a fresh child process, in the same call on the same device.  Three warm-up calls, then one HIP-event
pair per call, median of 15 (min and max kept).  Writes OUT.json (default profiles/r19/pe_wave_speed.json) and fails unless
(b) < (c) on every row and the losses of (b) and (c) agree to max(2e-6, 4 x noise), noise = the formula's fp32 run against
its fp64 run on the same points (plain torch on the device).  (b) / (a) gets no bar: it is reported with the min-max spread
of (a), so that a ratio outside that spread can be told from noise."""
import json, os, statistics, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = (("2->10x10->6", [2] + [10] * 10 + [6]), ("2->4x32->6", [2] + [32] * 4 + [6]), ("2->8x64->6", [2] + [64] * 8 + [6]))
SIZES = (1 << 14, 1 << 17, 1 << 20)
REPS = 15
ROLES = ("h", "U", "V", "eta_mean", "Hrms", "k")
OMEGA, GAMMA = 2.5, 0.42


def child(root, which):
    sys.path.insert(0, root)
    import torch
    from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec, physics
    from pinn_depthestimation_amd.dnn import DNN

    def median_ms(call):
        for _ in range(3): call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); call(); b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]

    def formula_loss(model, X, dtype):
        """the five-term loss of the formula on a plain torch restatement of the network, in dtype"""
        ps = [p.detach().to(dtype) for p in model._ordered_params()]
        cols = [X[:, i:i + 1].to(dtype).clone().requires_grad_(True) for i in range(2)]
        a = torch.cat(cols, -1)
        for i in range(0, len(ps), 2):
            a = torch.nn.functional.linear(a, ps[i], ps[i + 1])
            if i + 2 < len(ps):
                a = torch.tanh(a)
        return float(physics.physics_equation(*cols, *[a[:, i:i + 1] for i in range(6)], corrected=True, wave_omega=OMEGA,
                                              wave_gamma=GAMMA).detach())

    for tag, layers in SHAPES:
        torch.manual_seed(3)
        model = DNN(layers, 0.0, "xavier").to("cuda")
        last = [m for m in model.modules() if isinstance(m, torch.nn.Linear)][-1]
        with torch.no_grad():                                   # h = 2, eta = 0.2, Hrms = 0.5, k = 1: kh in [1.6, 2.4]
            last.weight.mul_(0.25); last.bias.copy_(torch.tensor([2.0, 0.0, 0.0, 0.2, 0.5, 1.0]))
        desc = NetDesc.from_layers(layers, (0, 1))
        eng = Engine(desc)
        for N in SIZES:
            X = (torch.rand(N, 2, generator=torch.Generator().manual_seed(5)) * 2 - 1).cuda()
            flat, grad = model.flat_params().detach().clone(), torch.zeros(desc.n_params, device="cuda")
            row = {"case": tag, "N": N}
            for key in which:
                if key in "ab":
                    kw = {"wave_omega": OMEGA, "wave_gamma": GAMMA} if key == "b" else {}
                    spec = ResidualSpec.from_names("physics_equation", ("x", "y"), (0, 1), ROLES, corrected=True, **kw)
                    scale = torch.full((spec.n_terms,), 1.0 / N, device="cuda")
                    row[key] = median_ms(lambda: eng.residual_loss_grad(spec, scale, flat, X, grad))
                    row[key + "_loss"] = float((eng.residual_loss_grad(spec, scale, flat, X, grad).double() * scale.double()).sum())
                else:
                    cols = [X[:, i:i + 1].clone().requires_grad_(True) for i in range(2)]

                    def step():
                        pred = model(torch.cat(cols, -1))
                        loss = physics.physics_equation(*cols, *[pred[:, i:i + 1] for i in range(6)], corrected=True,
                                                        wave_omega=OMEGA, wave_gamma=GAMMA)
                        model.zero_grad(); loss.backward()
                        return loss
                    row[key] = median_ms(step)
                    row[key + "_loss"] = float(step())
                    l64, l32 = formula_loss(model, X, torch.float64), formula_loss(model, X, torch.float32)
                    row["loss_fp64"], row["noise"] = l64, abs(l32 - l64) / abs(l64)
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
    if "--parent-tree" not in args:
        sys.exit(__doc__)
    i = args.index("--parent-tree"); parent = os.path.abspath(args[i + 1]); del args[i:i + 2]
    out_path = args[0] if args else os.path.join(HERE, "..", "profiles", "r19", "pe_wave_speed.json")
    this = os.path.abspath(os.path.join(HERE, ".."))
    theirs = run_child(parent, "a")
    mine = run_child(this, "bc")
    rows, bad = [], []
    for key, m in mine.items():
        a = theirs[key]["a"]
        bar = max(2e-6, 4 * m["noise"])
        gap = abs(m["b_loss"] - m["c_loss"]) / abs(m["loss_fp64"])
        row = {"case": key[0], "N": key[1], "reps": REPS,
               "a_corrected_parent_ms": a[0], "b_wave_ms": m["b"][0], "c_drop_in_ms": m["c"][0],
               "a_min_max_ms": a[1:], "b_min_max_ms": m["b"][1:], "c_min_max_ms": m["c"][1:],
               "b_over_a": round(m["b"][0] / a[0], 3), "a_spread": round(a[2] / a[1], 3), "c_over_b": round(m["c"][0] / m["b"][0], 2),
               "loss_b": m["b_loss"], "loss_c": m["c_loss"], "loss_fp64": m["loss_fp64"], "loss_gap_b_c": gap, "loss_bar": bar}
        rows.append(row)
        print(json.dumps(row), flush=True)
        if not row["b_wave_ms"] < row["c_drop_in_ms"]:
            bad.append((key, "(b) is not below (c)"))
        if not gap <= bar:
            bad.append((key, f"losses of (b) and (c) differ by {gap:.2e}, bar {bar:.2e}"))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
    if bad:
        sys.exit(f"failed: {bad}")
