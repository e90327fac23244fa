"""trainer_parity.py [OUT.txt] --parent-tree DIR: does trainer.PINN of this tree compute what the parent commit's computed?
DIR is a checkout of the parent with its library built.  Cells: plain, a trainable coefficient, self_adaptive per_term and loss
balancing ("sets", max_mean), each with fold_extras off and on, plus the plain request with lbfgs_impl="device".  Each cell runs
PINN.train(): 40 Adam iterations and the L-BFGS stage with max_it = 3, at N_res = 243 and N_fid = 12, on 2->10x10->6
physics_equation and 3->8x64->4 Navier_Stokes, every iteration logged.  Per cell the SHA-256 of the final parameters, of
log.txt and of the coefficients / multipliers / group weights, and the logged total losses.
Every tree is run by a fresh child process, in the same call on the same device: the parent PARENT_RUNS times, then this
tree.  A cell whose parent runs agree in all three hashes is held to bit-equality with them; one that does not reproduce
there (gradient sums by atomics) has its logged losses compared with the first parent run's, within the largest relative
difference between two parent runs' logged losses over all cells and pairs (printed: nobody had measured it).
Writes OUT.txt (default profiles/r16/trainer_parity.txt) and exits 1 when a cell misses."""
import hashlib, json, os, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from fold_ext_latency import SHAPES, config      # the two shapes and their configuration, as the latency tool has them

N_RES, N_FID, ADAM_IT, LBFGS_IT = 243, 12, 40, 3
MODES = {"plain": {}, "coefficient": None, "self_adaptive": dict(self_adaptive={"per_term": True}),
         "balanced_sets": dict(loss_balancing="max_mean", balance_groups="sets", balance_every=10)}
HASHES = ("params", "log", "extras")
PARENT_RUNS = 3


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def child(root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    from pinn_depthestimation_amd.dnn import DNN
    from pinn_depthestimation_amd.trainer import PINN

    for shape, (res, d_in, L, W, d_out, inn, outn, fid, cname, c0, bias) in SHAPES.items():
        rs = np.random.RandomState(5)
        Xr = rs.rand(N_RES, d_in).astype(np.float32) * 2 - 1
        Xf = rs.rand(N_FID, d_in).astype(np.float32) * 2 - 1
        Tf = rs.rand(N_FID, len(fid)).astype(np.float32)
        cfg = config(shape, ADAM_IT)
        cfg["lbfgs_optimizer"].update(max_it=LBFGS_IT, max_evaluation=LBFGS_IT * 5 // 4 + 1)
        cases = [(m, dict(fold_extras=f), f) for m in MODES for f in (False, True)] + [("plain", dict(lbfgs_impl="device"), False)]
        for mode, kw, fold in cases:
            kw.update(MODES[mode] if mode != "coefficient" else dict(coefficients={cname: c0}, trainable_coefficients=(cname,)))
            torch.manual_seed(3)
            model = DNN([d_in] + [W] * L + [d_out], 0.0, "xavier")
            last = [m for m in model.modules() if isinstance(m, torch.nn.Linear)][-1]
            with torch.no_grad():
                last.weight.mul_(0.25); last.bias.copy_(torch.tensor(bias))
            with tempfile.TemporaryDirectory() as tmp:
                tr = PINN(Xf, Tf, Xr, cfg, residual=res, dnn=model, log_every=1, checkpoint_every=0, log_dir=tmp, **kw)
                tr.train()
                torch.cuda.synchronize()
                if tr._log_fh is not None:
                    tr._log_fh.close()
                log = open(os.path.join(tmp, "log.txt"), "rb").read()
            extras = [t for t in (tr._coef, tr._lam, tr._bal_lam) if t is not None]
            row = {"shape": shape, "mode": mode, "fold_extras": fold, "lbfgs_impl": tr.lbfgs_impl, "iterations": tr.iter,
                   "folded_iterations": tr._folded_iters, "params": sha(tr.dnn.flat_params()), "log": hashlib.sha256(log).hexdigest(),
                   "extras": sha(torch.cat([t.reshape(-1) for t in extras])) if extras else None,
                   "total_loss": [h[3] for h in tr.history]}
            print("ROW " + json.dumps(row), flush=True)


def run_child(root):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        sys.exit(f"child for {root} failed:\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    rows = (json.loads(l[4:]) for l in out.stdout.splitlines() if l.startswith("ROW "))
    return {(r["shape"], r["mode"], r["fold_extras"], r["lbfgs_impl"]): r for r in rows}


def rel_diff(a, b):
    if len(a) != len(b):
        return float("inf")
    return max((abs(x - y) / max(abs(x), abs(y), 1e-30) for x, y in zip(a, b)), default=0.0)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2])
        sys.exit(0)
    args = sys.argv[1:]
    if "--parent-tree" not in args:
        sys.exit(__doc__)
    i = args.index("--parent-tree"); parent = os.path.abspath(args[i + 1]); del args[i:i + 2]
    out_path = args[0] if args else os.path.join(HERE, "..", "profiles", "r16", "trainer_parity.txt")
    parents = [run_child(parent) for _ in range(PARENT_RUNS)]
    br = run_child(os.path.abspath(os.path.join(HERE, "..")))
    pa = parents[0]
    noise = max(rel_diff(p[k]["total_loss"], q[k]["total_loss"]) for i, p in enumerate(parents) for q in parents[i + 1:] for k in pa)
    lines, missed = [f"parent against parent ({PARENT_RUNS} runs, every pair), largest relative difference of a logged total loss "
                     f"over all cells: {noise:.3e}"], 0
    for k, a in pa.items():
        c = br[k]
        same = all(a[h] == p[k][h] for h in HASHES for p in parents[1:])
        if same:
            ok = all(a[h] == c[h] for h in HASHES)
            how = "bit-equal" if ok else "hashes differ"
        else:
            d = rel_diff(a["total_loss"], c["total_loss"])
            ok, how = d <= noise and a["iterations"] == c["iterations"], f"loss history within {d:.3e} of the parent's"
        missed += not ok
        lines.append(f"{'ok  ' if ok else 'MISS'} {k[0]} | {k[1]} | fold_extras={int(k[2])} | lbfgs={k[3]} | iterations {c['iterations']} "
                     f"(folded {c['folded_iterations']}; parent {a['iterations']}, folded {a['folded_iterations']}) | parent reproducible: "
                     f"{same} | {how if ok else 'DIFFERS: ' + how}")
        for h in HASHES:
            lines.append(f"       sha256 {h:6s} parent {a[h]}  this tree {c[h]}")
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(1 if missed else 0)
