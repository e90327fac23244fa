"""fourier_speed.py OUT.json [--parent-tree DIR]: what a sine first layer (PINN_ACT_SIN_TANH) costs per call, ms.
residual_loss_grad at N = 2^14, 2^17, 2^20 on 3->8x64->4 (Navier_Stokes), 2->10x10->6 (physics_equation) and 2->100x20->3
(continuity_only), the same parameters for every column:
  (a) the sine network on ENGINE_FUSED_TILE (this tree),
  (b) the same shape with tanh on ENGINE_FUSED_TILE: the baseline the layer-0 recompute is judged against,
  (c) the sine network on ENGINE_GENERIC: what a fallback costs,
and (d) the plain forward (Engine.forward under AUTO: the four-tiles-per-wave kernel) at 2^20 points, sine and tanh.
(b) and the tanh half of (d) come from a build of the PARENT commit when --parent-tree names one (a checkout with its
library built), else from this tree; each tree is measured by a fresh child process under a time limit of its own, in the
same call on the same device, and the first failing child ends the run.  Three warm-up calls, then one HIP-event pair per
call, median of 15 (min and max kept).  Writes OUT.json (default profiles/r13/fourier_speed.json); no ratio is asserted."""
import json, os, statistics, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = (("3->8x64->4 Navier_Stokes", "Navier_Stokes", [3] + [64] * 8 + [4], ("t", "x", "y"), ("h", "z", "u", "v"), None),
         ("2->10x10->6 physics_equation", "physics_equation", [2] + [10] * 10 + [6], ("x", "y"),
          ("h", "U", "V", "eta_mean", "Hrms", "k"), [0.75, 0.0, 0.0, 0.0, 0.0, 0.0]),
         ("2->100x20->3 continuity_only", "continuity_only", [2] + [20] * 100 + [3], ("x", "y"), ("U", "V", "h"), None))
SIZES = (1 << 14, 1 << 17, 1 << 20)
REPS = 15
SIGMA = 4.0


def child(root, which):
    sys.path.insert(0, root)
    import math
    import torch
    from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec
    from pinn_depthestimation_amd._lib import ENGINE_FUSED_TILE, ENGINE_GENERIC
    from pinn_depthestimation_amd.dnn import init_flat_params

    def median_ms(call):
        for _ in range(3): call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); call(); b.record(); torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]

    for tag, res, layers, inn, outn, bias in CASES:
        k = len(inn)
        g = torch.Generator().manual_seed(3)
        flat = init_flat_params(layers, "xavier", g)
        nw = layers[0] * layers[1]                     # the Fourier layer's draw, written here so that a parent tree can run it too
        flat[:nw] = torch.empty(nw).normal_(0.0, SIGMA, generator=g)
        flat[nw:nw + layers[1]] = torch.empty(layers[1]).uniform_(0.0, 2 * math.pi, generator=g)
        if bias is not None:
            flat[-len(bias) - layers[-2] * len(bias):-len(bias)] *= 0.2
            flat[-len(bias):] = torch.tensor(bias)
        flat = flat.cuda()
        engs = {act: Engine(NetDesc.from_layers(layers, tuple(range(k)), act)) for act in (0, 2) if act == 0 or "a" in which}
        plain = {act: Engine(NetDesc.from_layers(layers, (), act)) for act in engs}
        spec = ResidualSpec.from_names(res, inn, tuple(range(k)), outn)
        for N in SIZES:
            X = (torch.rand(N, k, generator=torch.Generator().manual_seed(5)) * 2 - 1).cuda()
            grad = torch.zeros(flat.numel(), device="cuda")
            scale = torch.full((spec.n_terms,), 1.0 / N, device="cuda")
            row = {"case": tag, "N": N}
            for key in which:
                act, engine = (2, ENGINE_FUSED_TILE) if key == "a" else (0, ENGINE_FUSED_TILE) if key == "b" else (2, ENGINE_GENERIC)
                call = lambda: engs[act].residual_loss_grad(spec, scale, flat, X, grad, engine=engine)
                row[key] = median_ms(call)
                row[key + "_loss"] = float((call()[:2] * scale[:2]).sum())
            if N == SIZES[-1]:
                if "a" in which: row["d_sin"] = median_ms(lambda: plain[2].forward(flat, X))
                if "b" in which: row["d_tanh"] = median_ms(lambda: plain[0].forward(flat, X))
            print("ROW " + json.dumps(row), flush=True)


def run_child(root, which):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, which], capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        sys.exit(f"child for {root} failed (exit status {out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    return {(r["case"], r["N"]): r for r in (json.loads(l[4:]) for l in out.stdout.splitlines() if l.startswith("ROW "))}


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        sys.exit(0)
    args = sys.argv[1:]
    parent = None
    if "--parent-tree" in args:
        i = args.index("--parent-tree"); parent = os.path.abspath(args[i + 1]); del args[i:i + 2]
    out_path = args[0] if args else os.path.join(HERE, "..", "profiles", "r13", "fourier_speed.json")
    this = os.path.abspath(os.path.join(HERE, ".."))
    base = run_child(parent, "b") if parent else None
    mine = run_child(this, "ac" if parent else "abc")
    rows = []
    for key, m in mine.items():
        src = base[key] if parent else m
        row = {"case": key[0], "N": key[1], "reps": REPS, "sigma": SIGMA, "b_from": "parent build" if parent else "this tree",
               "a_sin_tile_ms": m["a"][0], "b_tanh_tile_ms": src["b"][0], "c_sin_generic_ms": m["c"][0],
               "a_min_max_ms": m["a"][1:], "b_min_max_ms": src["b"][1:], "c_min_max_ms": m["c"][1:],
               "a_over_b": round(m["a"][0] / src["b"][0], 3), "c_over_a": round(m["c"][0] / m["a"][0], 2),
               "loss_a": m["a_loss"], "loss_c": m["c_loss"]}
        if "d_sin" in m:
            row.update(d_plain_forward_sin_ms=m["d_sin"][0], d_plain_forward_tanh_ms=src["d_tanh"][0],
                       d_sin_over_tanh=round(m["d_sin"][0] / src["d_tanh"][0], 3))
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
