"""pe_corrected_speed.py OUT.json [--parent-tree DIR]: what the corrected radiation-stress residual costs per call, ms, at
N = 2^14, 2^17, 2^20 on 2->10x10->6 and 2->8x64->6 (engine AUTO, conditioned networks: kh ~ 2):
  (a) the bug-compatible Engine.residual_loss_grad (E == 0: no stress terms),
  (b) Engine.residual_loss_grad with ResidualSpec.corrected — the hard-wired epilogue, this tree,
  (c) one drop-in step: DNN forward, physics.physics_equation(corrected=True), backward() — forward jet, torch autograd
      over the formula, jet_backward: what (b) replaces.
(a) and (c) come from a build of the PARENT commit when --parent-tree names one (a checkout with its library built), else
from this tree; each tree is measured by a fresh child process, in the same call on the same device.  Three warm-up calls,
then one HIP-event pair per call, median of 15 (min and max kept).  Writes OUT.json (default profiles/r08/pe_corrected_speed.json)
and fails if (b) is not below (c) anywhere."""
import json, os, statistics, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = (("2->10x10->6", [2] + [10] * 10 + [6]), ("2->8x64->6", [2] + [64] * 8 + [6]))
SIZES = (1 << 14, 1 << 17, 1 << 20)
REPS = 15
ROLES = ("h", "U", "V", "eta_mean", "Hrms", "k")


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
            scale = torch.full((3,), 1.0 / N, device="cuda")
            row = {"case": tag, "N": N}
            for key in which:
                if key in "ab":
                    kw = {"corrected": True} if key == "b" else {}
                    spec = ResidualSpec.from_names("physics_equation", ("x", "y"), (0, 1), ROLES, **kw)
                    row[key] = median_ms(lambda: eng.residual_loss_grad(spec, scale, flat, X, grad))
                    row[key + "_loss"] = float((eng.residual_loss_grad(spec, scale, flat, X, grad) * scale).sum())
                else:
                    cols = [X[:, i:i + 1].clone().requires_grad_(True) for i in range(2)]

                    def step():
                        pred = model(torch.cat(cols, -1))
                        loss = physics.physics_equation(*cols, *[pred[:, i:i + 1] for i in range(6)], corrected=True)
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
    out_path = args[0] if args else os.path.join(HERE, "..", "profiles", "r08", "pe_corrected_speed.json")
    this = os.path.abspath(os.path.join(HERE, ".."))
    ac = run_child(parent, "ac") if parent else None
    mine = run_child(this, "b" if parent else "abc")
    rows, bad = [], []
    for key, m in mine.items():
        src = ac[key] if parent else m
        row = {"case": key[0], "N": key[1], "reps": REPS, "a_and_c_from": "parent build" if parent else "this tree",
               "a_plain_ms": src["a"][0], "b_corrected_ms": m["b"][0], "c_drop_in_ms": src["c"][0],
               "a_min_max_ms": src["a"][1:], "b_min_max_ms": m["b"][1:], "c_min_max_ms": src["c"][1:],
               "b_over_a": round(m["b"][0] / src["a"][0], 3), "c_over_b": round(src["c"][0] / m["b"][0], 2),
               "loss_b": m["b_loss"], "loss_c": src["c_loss"]}
        rows.append(row)
        print(json.dumps(row), flush=True)
        if not row["b_corrected_ms"] < row["c_drop_in_ms"]:
            bad.append(key)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
    if bad:
        sys.exit(f"(b) is not below (c) at {bad}")
