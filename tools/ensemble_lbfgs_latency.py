#!/usr/bin/env python3
"""ensemble_lbfgs_latency.py — microseconds per slot of the ensemble's device-resident L-BFGS loop
(lbfgs.EnsembleDeviceLBFGS, pinn_ensemble_lbfgs_loop) against M times the slot of the single loop (lbfgs.DeviceLBFGS,
pinn_lbfgs_loop), in one process, warm.  A slot is one loss + gradient evaluation of every member and one step of each
member's strong-Wolfe state machine.  History 100, tolerances 0, lr 1: the reference's settings (train.py:116-125).

Workloads: config_CMB's problem (2 -> 10 x 10 -> 6, physics_equation, 243 collocation + 12 fidelity points, one split
request) at M = 1, 8, 64, 256, and Navier-Stokes 8 x 64 on 243 points at M = 1, 8, 64.  Every figure is the median of REPS
runs of SLOTS slots from a freshly initialised state (so that every slot is a working one), the clock from the call that
enqueues them to a device synchronisation after it.  The single loop is measured twice per workload: the difference of
the two is the run-to-run spread the M = 1 comparison is read against.

    python tools/ensemble_lbfgs_latency.py
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pinn_depthestimation_amd.dnn import DNN
from pinn_depthestimation_amd.engine import Engine, NetDesc, ResidualSpec
from pinn_depthestimation_amd.lbfgs import DeviceLBFGS, EnsembleDeviceLBFGS

DEV = "cuda:0"
SLOTS, REPS = 64, 7
PE_ROLES = ("h", "U", "V", "eta_mean", "Hrms", "k")
OPTS = dict(lr=1.0, max_iter=10 ** 6, max_eval=10 ** 7, history_size=100, tolerance_grad=0.0, tolerance_change=0.0)


def rand(n, d, seed):
    return (torch.rand(n, d, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(DEV).contiguous()


def weights(layers, seed, roles=None):
    """dnn.DNN's Xavier initialisation from `seed`; physics_equation's outputs conditioned as tools/lbfgs_device_latency.py
    conditions them (eta_mean + h away from 0)."""
    torch.manual_seed(seed)
    dnn = DNN(layers, 0.0, "xavier")
    if roles is not None:
        last = [m for m in dnn.modules() if isinstance(m, torch.nn.Linear)][-1]
        with torch.no_grad():
            last.weight.mul_(0.25)
            for name, val in (("h", 2.0), ("eta_mean", 0.2), ("Hrms", 0.5), ("k", 1.0)):
                last.bias[roles.index(name)] = val
    return torch.cat([p.detach().reshape(-1) for p in dnn._ordered_params()]).to(DEV).contiguous()


class Workload:
    def __init__(self, name, desc, residual, inputs, outputs, n_res, n_fid, conditioned):
        self.name, self.desc = name, desc
        self.spec = ResidualSpec.from_names(residual, inputs, desc.grad_cols, outputs)
        self.roles = outputs if conditioned else None
        self.n_res, self.fid = n_res, list(range(len(outputs))) if n_fid else []
        nt, nc = self.spec.n_terms, len(self.fid)
        self.X = rand(n_res + n_fid, desc.d_in, 1)
        self.T = (rand(n_fid, nc, 3) * 0.1 + 0.5) if n_fid else None
        self.res_scale = torch.full((nt,), 1.0 / n_res, device=DEV)
        self.fid_scale = torch.full((nc,), 1.0 / n_fid, device=DEV) if nc else None
        rows = torch.zeros(3, nc + nt)
        if nc:
            rows[0, :nc] = 1.0 / n_fid
        rows[1, nc:] = 1.0 / n_res
        rows[2] = rows[0] + rows[1]
        self.loss_rows = rows.to(DEV).contiguous()

    def theta(self, M):
        return torch.stack([weights(self.desc.layers, 1234 + j, self.roles) for j in range(M)]).contiguous()

    def args(self):
        return (self.spec, None, self.X, self.n_res, self.res_scale, self.loss_rows, 2)

    def kw(self):
        return dict(T=self.T, out_col=self.fid, col_scale=self.fid_scale, **OPTS)


def measure(opt, theta0):
    """Median microseconds per slot over REPS runs of SLOTS slots, each from a fresh state and the same weights; how many
    of the last run's slots were working ones."""
    times = []
    for rep in range(REPS + 1):                     # (the first run is the warm-up)
        opt.params.copy_(theta0)
        opt.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr = opt.enqueue(SLOTS)
        torch.cuda.synchronize()
        if rep:
            times.append((time.perf_counter() - t0) / SLOTS * 1e6)
    return statistics.median(times), min(times), int((tr[..., 2] != 0).sum())


def main():
    ns = NetDesc(3, 4, 8, 64, (0, 1, 2))
    pe = NetDesc(2, 6, 10, 10, (0, 1))
    work = ((Workload("config_CMB 10x10 N=243+12", pe, "physics_equation", ("x", "y"), PE_ROLES, 243, 12, True), (1, 8, 64, 256)),
            (Workload("Navier-Stokes 8x64 N=243", ns, "Navier_Stokes", ("t", "x", "y"), ("h", "z", "u", "v"), 243, 0, False), (1, 8, 64)))
    print(f"{SLOTS} slots per run, median (and fastest) of {REPS} runs, microseconds per slot; history 100, tolerances 0")
    for w, Ms in work:
        eng = Engine(w.desc, DEV)
        spec, _, X, n_res, rs, rows, total = w.args()
        th1 = w.theta(1)
        single = []
        for _ in range(2):
            one = DeviceLBFGS(eng, spec, th1[0].clone(), X, n_res, rs, rows, total, **w.kw())
            single.append(measure(one, th1[0]))
            del one
        s_med = min(s[0] for s in single)
        spread = abs(single[0][0] - single[1][0])
        print(f"{w.name:28s} single loop     : {single[0][0]:8.1f} ({single[0][1]:.1f}) and {single[1][0]:8.1f} ({single[1][1]:.1f}) us/slot; "
              f"run-to-run spread {spread:.1f} us; {single[1][2]} of {SLOTS} slots working", flush=True)
        for M in Ms:
            th = w.theta(M)
            gx, _ = eng.ensemble_plan(M, X.shape[0])
            ens = EnsembleDeviceLBFGS(eng, spec, th.clone(), X, n_res, rs, rows, total, **w.kw())
            med, best, working = measure(ens, th)
            print(f"{w.name:28s} ensemble M = {M:3d} : {med:8.1f} ({best:.1f}) us/slot = {med / M:8.2f} us/member; M single slots "
                  f"{M * s_med:10.1f} us: x{M * s_med / med:6.2f}; {gx} workgroups per member in the pass; {working} of {SLOTS * M} "
                  f"member slots working", flush=True)
            del ens, th
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
