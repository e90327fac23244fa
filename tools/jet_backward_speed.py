"""jet_backward_speed.py: what a residual written with compute_gradient costs against a hard-wired one.
(a) Engine.jet_backward (gY and gdY given) on the GENERIC engine and on FUSED (the tile kernel's external-adjoint
    instances), (b) Engine.residual_loss_grad on FUSED for the same network and points, at N = 2^14, 2^17, 2^20;
(c) one physics_equation(corrected=True) forward + backward() through the drop-in face at 2^20 points.
(d) the two fused kernels of jet_backward side by side, FUSED_TILE and FUSED_BATCH alternating in one process, on the
    narrow shapes the batch kernel serves, at N = 2^12, 2^14, 2^17, 2^20, with residual_loss_grad on the same two kernels
    for reference: REPEATS event-timed repeats per cell after a warm-up, reported as median and (min, max) so that the
    run-to-run spread is known; (e) drop-in steps at 2^20 points: physics_equation(corrected=True) on 2->10x10->6 and a
    Burgers-type loss on 2->100x20->3, with repeats (runs unchanged in a checkout that has no batch jet_backward).
JB_ONLY picks the parts (default "abc"; "d" and "e" are the batch-kernel measurements of DESIGN.md 2.4b).
HIP-event times after a warm-up call.  Prints one JSON line per row and writes them all to the path given as the first
argument (optional).  PINN_HIP_LIB=<another build of the library> measures that build with the same script (a build
that knows no MFMA jet_backward runs it on the generic engine whatever the descriptor says)."""
import json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec, physics
from pinn_depthestimation_amd.dnn import DNN, init_flat_params
from pinn_depthestimation_amd._lib import ENGINE_FUSED, ENGINE_FUSED_BATCH, ENGINE_FUSED_TILE, ENGINE_GENERIC

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


def spread(call, reps, repeats):
    """median and (min, max) of `repeats` event-timed means over `reps` calls, after one warm-up call"""
    call(); torch.cuda.synchronize()
    ts = sorted(timed(call, reps) for _ in range(repeats))
    return round(ts[len(ts) // 2], 4), (round(ts[0], 4), round(ts[-1], 4))


AB_CASES = (("2->10x10->6 k=2", NetDesc(2, 6, 10, 10, (0, 1)), "physics_equation", ("x", "y"), ("h", "U", "V", "eta_mean", "Hrms", "k")),
            ("4->20x20->4 k=3", NetDesc(4, 4, 20, 20, (1, 2, 3)), "Navier_Stokes", ("s", "t", "x", "y"), ("h", "z", "u", "v")),
            ("2->100x20->3 k=2", NetDesc(2, 3, 100, 20, (0, 1)), "continuity_ftemp", ("x", "y"), ("U", "V", "h")))
AB_SIZES = (1 << 12, 1 << 14, 1 << 17, 1 << 20)
REPEATS = 5

if "d" in only:
    for tag, desc, res, inn, outn in AB_CASES:
        for N in AB_SIZES:
            g = torch.Generator().manual_seed(3)
            X = (torch.rand(N, desc.d_in, generator=g) * 2 - 1).cuda()
            params = init_flat_params(desc.layers, "xavier", g).cuda()
            if res == "physics_equation":
                params[desc.n_params - desc.d_out + 0] = 0.75
                params[desc.n_params - desc.d_out + 3] = 0.0
            gY = torch.randn(N, desc.d_out, device="cuda") / N
            gdY = torch.randn(desc.k, N, desc.d_out, device="cuda") / N
            grad = torch.zeros(desc.n_params, device="cuda")
            spec = ResidualSpec.from_names(res, inn, desc.grad_cols, outn)
            scale = torch.full((spec.n_terms,), 1.0 / N, device="cuda")
            engs = {"tile": Engine(desc.with_(engine=ENGINE_FUSED_TILE)), "batch": Engine(desc.with_(engine=ENGINE_FUSED_BATCH))}
            assert engs["tile"].jet_backward_kernel(N) == ENGINE_FUSED_TILE and engs["batch"].jet_backward_kernel(N) == ENGINE_FUSED_BATCH
            reps = 20 if N <= (1 << 14) else (10 if N < (1 << 20) else 3)
            row = {"case": tag, "N": N, "repeats": REPEATS, "calls_per_repeat": reps}
            cells = {}
            for _ in range(REPEATS):      # tile, batch, tile, batch, ...: a drift of the clock hits both columns alike
                for name, eng in engs.items():
                    eng.jet_backward(params, X, gY, gdY, grad); torch.cuda.synchronize()
                    cells.setdefault(f"jet_backward_{name}", []).append(timed(lambda: eng.jet_backward(params, X, gY, gdY, grad), reps))
                    cells.setdefault(f"residual_loss_grad_{name}", []).append(timed(lambda: eng.residual_loss_grad(spec, scale, params, X, grad), reps))
            for k, ts in cells.items():
                ts = sorted(ts)
                row[k + "_ms"] = round(ts[len(ts) // 2], 4)
                row[k + "_min_max_ms"] = [round(ts[0], 4), round(ts[-1], 4)]
            row["jet_backward_tile_over_batch"] = round(row["jet_backward_tile_ms"] / row["jet_backward_batch_ms"], 3)
            row["jet_backward_batch_over_residual_batch"] = round(row["jet_backward_batch_ms"] / row["residual_loss_grad_batch_ms"], 3)
            row["jet_backward_tile_over_residual_tile"] = round(row["jet_backward_tile_ms"] / row["residual_loss_grad_tile_ms"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del engs
            torch.cuda.empty_cache()

if "e" in only:
    def burgers2(x, y, h, u, v):
        d = physics.compute_gradient
        r1 = u * d(u, x) + v * d(u, y) + 0.3 * d(h, x)
        r2 = u * d(v, x) + v * d(v, y) + 0.3 * d(h, y)
        return torch.mean(r1 ** 2) + torch.mean(r2 ** 2) + 0.1 * torch.mean((h - 0.5) ** 2)

    def pe(x, y, *outs):
        return physics.physics_equation(x, y, *outs, corrected=True)

    for tag, layers, loss_fn in (("physics_equation(corrected=True), 2->10x10->6", [2] + [10] * 10 + [6], pe),
                                 ("Burgers-type loss, 2->100x20->3", [2] + [20] * 100 + [3], burgers2)):
        N = 1 << 20
        torch.manual_seed(3)
        model = DNN(layers, 0.0, "xavier").to("cuda")
        if layers[-1] == 6:
            last = [m for m in model.modules() if isinstance(m, torch.nn.Linear)][-1]
            with torch.no_grad():
                last.bias[0] = 2.0; last.bias[4] = 0.2; last.bias[5] = 1.0
        Xh = (torch.rand(N, 2, generator=torch.Generator().manual_seed(5)) * 2 - 1).cuda()

        def step():
            x, y = [Xh[:, i:i + 1].clone().requires_grad_(True) for i in range(2)]
            pred = model(torch.cat([x, y], -1))
            loss = loss_fn(x, y, *[pred[:, i:i + 1] for i in range(layers[-1])])
            model.zero_grad()
            loss.backward()

        med, mm = spread(step, 3, REPEATS)
        row = {"case": f"{tag}: forward + backward() through the drop-in face", "N": N, "step_ms": med, "step_min_max_ms": list(mm)}
        rows.append(row)
        print(json.dumps(row), flush=True)

if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(rows, f, indent=1)
