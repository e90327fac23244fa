"""residual_parity.py [OUT.txt] --parent-tree DIR: do the residual kernels of this tree compute, bit for bit, what the parent
commit's computed?  DIR is a checkout of the parent with its library built.  This tree's Python drives every run; the library
is chosen by PINN_HIP_LIB, each in a fresh child process, in the same call on the same device: the parent's PARENT_RUNS times,
then this tree's.  Per case the SHA-256 of every output, each on its own (term sums, column sums, fields, gradient,
coefficient gradient).
Cases: residual_loss, residual_loss_grad and residual_fields for Navier_Stokes, physics_equation (plain, corrected, wave closure),
continuity_ftemp and continuity_only (threshold 0.1: some points masked, not all); residual_coef_loss_grad for Navier_Stokes
and physics_equation at a non-default coefficient; residual_weighted_loss_grad with the field store for Navier_Stokes,
physics_equation and continuity_only; residual2_loss_grad at nu = 0.05 for Navier_Stokes, physics_equation and its corrected
form on the generic and on the MFMA path; one merged residual + fidelity call and one split call.  Each on ENGINE_GENERIC,
ENGINE_FUSED_TILE and ENGINE_FUSED_BATCH, two hidden layers of width 10, 20 and 64, N = 13 (one ragged tile), 243 (ragged last
tile) and 4101.
A request an engine refuses (PINN_ERR_UNSUPPORTED) must be refused by both libraries.  An output is held to bit-equality where the
parent's runs agree with each other, and reported as skipped where they do not.  For Navier_Stokes, physics_equation and continuity
on GENERIC and FUSED_TILE no sums, no fields and no coefficient gradient may be skipped at any size (fixed-order sums), and no
parameter gradient at N = 13: one tile is one wave adding into one gradient copy in program order, so there the tile kernel's
gradient reproduces itself and is held to the parent's bits (residual2 excepted: its kernels' unit is byte-identical to the
parent's).  With more than one tile in a workgroup the MFMA kernels' parameter gradient is summed by atomics and differs between
two runs of the parent; those skips are counted and reported.  Writes
OUT.txt (default profiles/r20/residual_parity.txt); exits 1 on a difference, a forbidden skip or a failed child (no further child
is started)."""
import hashlib, json, os, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
LIB = os.path.join("pinn_depthestimation_amd", "libpinn_hip.so")
WIDTHS, SIZES, PARENT_RUNS, NU = (10, 20, 64), (13, 243, 4101), 2, 0.05
ONE_TILE = 16      # up to here the tile kernel has one wave adding into one gradient copy in program order (pinn_hip.h): reproducible
# name -> (residual, inputs, outputs, from_names keywords, spec fields set afterwards, last-layer bias)
PE_OUT, PE_BIAS = ("h", "U", "V", "eta_mean", "Hrms", "k"), [2.0, 0.0, 0.0, 0.2, 0.5, 1.0]
RESIDUALS = {
    "NS": ("Navier_Stokes", ("t", "x", "y"), ("h", "z", "u", "v"), {}, {}, [2.0, 0.2, 0.0, 0.0]),
    "PE": ("physics_equation", ("x", "y"), PE_OUT, {}, {}, PE_BIAS),
    "PE_corrected": ("physics_equation", ("x", "y"), PE_OUT, dict(corrected=True), {}, PE_BIAS),
    "PE_wave": ("physics_equation", ("x", "y"), PE_OUT, dict(corrected=True, wave_omega=0.9, wave_gamma=0.42), {}, PE_BIAS),
    "continuity_ftemp": ("continuity_ftemp", ("x", "y"), ("U", "V", "h"), {}, {}, [0.0, 0.0, 1.0]),
    "continuity_only": ("continuity_only", ("x", "y"), ("U", "V", "h"), {}, dict(threshold=0.1), [0.0, 0.0, 1.0]),
}
FIXED_ORDER = ("NS", "PE", "continuity_ftemp", "continuity_only")     # no skip allowed on GENERIC and FUSED_TILE


def sha(*ts):
    return [hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest() for t in ts]


def child():
    sys.path.insert(0, ROOT)
    import dataclasses
    import torch
    from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec, _lib
    from pinn_depthestimation_amd.dnn import DNN
    engines = {"GENERIC": _lib.ENGINE_GENERIC, "FUSED_TILE": _lib.ENGINE_FUSED_TILE, "FUSED_BATCH": _lib.ENGINE_FUSED_BATCH}

    def emit(key, call):      # call() returns (term sums, ..., gradient last where there is one)
        try:
            row = {"key": key, "sha": sha(*call())}
        except _lib.PinnError as e:
            if f"(code {_lib.ERR_UNSUPPORTED})" not in str(e):
                raise
            row = {"key": key, "sha": None}
        print("ROW " + json.dumps(row), flush=True)

    for name, (res, inn, outn, kw, fields, bias) in RESIDUALS.items():
        k = len(inn)
        for W in WIDTHS:
            layers = [k, W, W, len(outn)]
            torch.manual_seed(3)
            model = DNN(layers, 0.0, "xavier").to("cuda")
            last = [m for m in model.modules() if isinstance(m, torch.nn.Linear)][-1]
            with torch.no_grad():
                last.weight.mul_(0.25); last.bias.copy_(torch.tensor(bias))
            desc = NetDesc.from_layers(layers, tuple(range(k)))
            eng = Engine(desc)
            spec = dataclasses.replace(ResidualSpec.from_names(res, inn, desc.grad_cols, outn, **kw), **fields)
            flat = model.flat_params().detach().clone()
            for N in SIZES:
                gen = torch.Generator().manual_seed(5)
                X = (torch.rand(N, k, generator=gen) * 2 - 1).cuda()
                wts = (torch.rand(spec.n_weighted_terms, N, generator=gen) + 0.5).cuda()
                T = torch.rand(N, 2, generator=gen).cuda()
                scale = torch.full((spec.n_terms,), 1.0 / N, device="cuda")
                cscale = torch.full((2,), 0.5 / N, device="cuda")
                zeros = lambda n=desc.n_params: torch.zeros(n, device="cuda")
                for ename, e in engines.items():
                    key = lambda call: f"{name} | {W} | {N} | {ename} | {call}"

                    def loss_grad():
                        g = zeros(); return eng.residual_loss_grad(spec, scale, flat, X, g, engine=e), g
                    emit(key("residual_loss"), lambda: (eng.residual_loss(spec, flat, X, engine=e),))
                    emit(key("residual_loss_grad"), loss_grad)
                    emit(key("residual_fields"), lambda: (eng.residual_fields(spec, flat, X, engine=e),))
                    if name in ("NS", "PE"):
                        def coef():
                            g, gc = zeros(), zeros(1)
                            c = torch.tensor([0.6 if name == "NS" else 0.05], device="cuda")
                            return eng.residual_coef_loss_grad(spec, c, scale, flat, X, g, gc, engine=e), g, gc
                        emit(key("residual_coef_loss_grad"), coef)
                    if name in ("NS", "PE", "continuity_only"):
                        def weighted():
                            g = zeros(); s, f = eng.residual_weighted_loss_grad(spec, wts, scale, flat, X, g, fields=True, engine=e)
                            return s, f, g
                        emit(key("residual_weighted_loss_grad+fields"), weighted)
                    if name in ("NS", "PE", "PE_corrected") and ename != "FUSED_BATCH":      # residual2: GENERIC or the MFMA path
                        def res2():
                            g = zeros(); s2 = dataclasses.replace(spec, nu=NU)
                            s, f = eng.residual2_loss_grad(s2, scale, flat, X, g, fields=True,
                                                           engine=_lib.ENGINE_GENERIC if ename == "GENERIC" else _lib.ENGINE_FUSED)
                            return s, f, g
                        emit(key("residual2_loss_grad nu=0.05 " + ("generic path" if ename == "GENERIC" else "MFMA path")), res2)
                    if name in ("NS", "continuity_only"):
                        def merged():
                            g = zeros(); ts, cs = eng.residual_mse_loss_grad(spec, scale, T, [0, 2], cscale, flat, X, g, engine=e)
                            return ts, cs, g

                        def split():
                            g, n_res = zeros(), N - (50 if N > 100 else 5)
                            ts, cs = eng.residual_mse_split_loss_grad(spec, scale, T[n_res:], [0, 2], cscale, flat, X, n_res, g, engine=e)
                            return ts, cs, g
                        emit(key("residual_mse_loss_grad (merged)"), merged)
                        emit(key("residual_mse_split_loss_grad (split)"), split)
    torch.cuda.synchronize()


def run_child(tree):
    env = dict(os.environ, PINN_HIP_LIB=os.path.join(tree, LIB))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=900, env=env)
    if out.returncode != 0:
        sys.exit(f"child with {env['PINN_HIP_LIB']} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    return {r["key"]: r["sha"] for r in (json.loads(l[4:]) for l in out.stdout.splitlines() if l.startswith("ROW "))}


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
        sys.exit(0)
    args = sys.argv[1:]
    if "--parent-tree" not in args:
        sys.exit(__doc__)
    i = args.index("--parent-tree"); parent = os.path.abspath(args[i + 1]); del args[i:i + 2]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r20", "residual_parity.txt")
    parents = [run_child(parent) for _ in range(PARENT_RUNS)]
    mine = run_child(ROOT)
    lines, count = [], {"bit-equal": 0, "refused by both": 0, "gradient skipped": 0, "skipped": 0, "MISS": 0}
    for key, a in parents[0].items():
        name, _, N, ename, call = key.split(" | ")
        c = mine.get(key, "absent")
        if a is None or c is None or c == "absent":
            how = "refused by both" if a is None and c is None else "MISS"
            note = "" if how != "MISS" else " (refused by one library only, or absent)"
        else:
            # outputs in call order; the parameter gradient is the last one of a *_grad call, behind it only the coefficient
            # gradient, which comes through the fixed-order reduction and is never excused
            grads = [1 if "coef" in call else len(a) - 1] if "grad" in call else []
            unstable = [i for i in range(len(a)) if any(p[key][i] != a[i] for p in parents[1:])]
            differ = [i for i in range(len(a)) if i not in unstable and a[i] != c[i]]
            strict = name in FIXED_ORDER and ename in ("GENERIC", "FUSED_TILE")
            if differ:
                how, note = "MISS", f" (outputs {differ} differ: sha256 parent {[a[i] for i in differ]} this tree {[c[i] for i in differ]})"
            elif not unstable:
                how, note = "bit-equal", f" ({len(a)} outputs)"
            elif strict and (any(i not in grads for i in unstable) or (int(N) <= ONE_TILE and "residual2" not in call)):
                how, note = "MISS", f" (outputs {unstable} of {len(a)} do not reproduce themselves on the parent where they have a fixed order)"
            elif all(i in grads for i in unstable):
                how, note = "gradient skipped", f" (outputs {unstable} of {len(a)}: the parent's gradient does not reproduce itself; the other outputs bit-equal)"
            else:
                how, note = "skipped", f" (outputs {unstable} of {len(a)} do not reproduce themselves on the parent; the other outputs bit-equal)"
        count[how] += 1
        lines.append(f"{how:17s} {key}{note}")
    lines.append(f"{len(parents[0])} cases, parent run {PARENT_RUNS} times: " + ", ".join(f"{v} {k}" for k, v in count.items())
                 + f"; {len(set(mine) - set(parents[0]))} cases only in this tree")
    print("\n".join(l for l in lines if not l.startswith(("bit-equal", "refused by both", "gradient skipped"))))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(1 if count["MISS"] or set(mine) != set(parents[0]) else 0)
