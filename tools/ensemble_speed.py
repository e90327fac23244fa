#!/usr/bin/env python3
"""ensemble_speed.py — ms per Adam iteration of an ensemble of M networks (Engine.ensemble_adam_step with an lr sequence:
pinn_ensemble_adam_loop, two launches per iteration whatever M is) against what the single-network entry can do for the
same work: M runs of pinn_adam_loop (Engine.loss_grad_adam_step with an lr sequence), one after the other, on the engine
AUTO picks for the shape.  Three shapes of the reference:
    config_CMB        2 -> 10 x 10 -> 6, physics_equation, 243 collocation + 12 fidelity points (split request)
    Navier-Stokes     3 -> 8 x 64 -> 4, residual only, N = 243
    train_newmethod   2 -> 100 x 20 -> 3, continuity_only, both terms on each of 12 514 points
Both sides run in this process, alternating, after a warm-up of each; the clock is the host's around work that ends in a
device synchronisation; the iteration count of a window is chosen from a probe so that a window lasts about --window
seconds.  Per (shape, M): the median of --reps windows and their spread.

    python tools/ensemble_speed.py [--members 1 4 16 64 256] [--reps 3] [--window 0.3] [--out profiles/r06/ensemble_speed.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec
from pinn_depthestimation_amd.dnn import init_flat_params

PE_OUT = ("h", "U", "V", "eta_mean", "Hrms", "k")
SHAPES = {
    # name: d_in, d_out, L, W, grad_cols, residual, inputs, outputs, fidelity columns, N_res, N_fid (None: one point set)
    "config_CMB 10x10 243+12": (2, 6, 10, 10, (0, 1), "physics_equation", ("x", "y"), PE_OUT, (0, 1, 2, 3, 4, 5), 243, 12),
    "Navier-Stokes 8x64 N=243": (3, 4, 8, 64, (0, 1, 2), "Navier_Stokes", ("t", "x", "y"), ("h", "z", "u", "v"), (), 243, 0),
    "train_newmethod 100x20 N=12514": (2, 3, 100, 20, (0, 1), "continuity_only", ("x", "y"), ("U", "V", "h"), (0, 1), 12514, None),
}
MAX_RUN = 256


class Problem:
    def __init__(self, name, M):
        d_in, d_out, L, W, gc, res, inn, outn, fid, n_r, n_f = SHAPES[name]
        layers = [d_in] + [W] * L + [d_out]
        g = torch.Generator().manual_seed(1234)
        rows = []
        for i in range(M):
            th = init_flat_params(layers, "xavier", torch.Generator().manual_seed(1234 + i))
            if res == "physics_equation":            # eta_mean + h away from 0: the last layer's biases (its last d_out entries)
                th[-d_out + outn.index("h")] = 0.75; th[-d_out + outn.index("eta_mean")] = 0.0
            rows.append(th)
        self.theta0 = torch.stack(rows).cuda()
        self.desc = NetDesc(d_in, d_out, L, W, gc)
        self.spec = ResidualSpec.from_names(res, inn, gc, outn)
        self.M, self.P, self.fid = M, self.theta0.shape[1], list(fid)
        N = n_r + (0 if n_f is None else n_f)
        nt = n_r if n_f is None else n_f
        X = torch.rand(N, d_in, generator=g) * 2 - 1
        if res == "continuity_only":
            X[:, 0] = X[:, 0] * 40
            self.scale = torch.tensor([1.0 / n_r, 1.0 / float((X[:, 0] < 25.5).sum()), 0.0]).cuda()
        else:
            self.scale = torch.full((self.spec.n_terms,), 1.0 / n_r).cuda()
        self.X = X.cuda()
        self.T = torch.rand(nt, len(fid), generator=g).cuda() if fid else None
        self.cscale = torch.full((len(fid),), 1.0 / max(nt, 1)).cuda() if fid else None
        self.N, self.n_res = N, (-1 if n_f is None else n_r)
        self.eng = Engine(self.desc)
        nterm, nc = self.spec.n_terms, len(fid)
        z = lambda *s: torch.zeros(*s, device="cuda")
        self.ens = dict(th=self.theta0.clone(), grad=z(M, self.P), m=z(M, self.P), v=z(M, self.P), ts=z(M, nterm), cs=z(M, nc) if nc else None)
        self.one = dict(th=self.theta0.clone(), grad=z(self.P), m=z(M, self.P), v=z(M, self.P), ts=z(nterm), cs=z(nc) if nc else None)
        self.step = 1

    def _kw(self, b):
        return dict(T=self.T, out_col=self.fid, col_scale=self.cscale, term_sums=b["ts"], col_sums=b["cs"])

    def ensemble(self, k):
        """k Adam iterations of all M members: one call per run of <= MAX_RUN iterations."""
        b, done = self.ens, 0
        while done < k:
            n = min(k - done, MAX_RUN)
            assert self.eng.ensemble_adam_step(self.spec, self.scale, b["th"], self.X, self.n_res, b["grad"], b["m"], b["v"],
                                               self.step + done, [1e-4] * n, **self._kw(b))
            done += n

    def sequential(self, k):
        """The same work through the single-network entry: member after member, each k iterations in runs of <= MAX_RUN."""
        b = self.one
        for i in range(self.M):
            done = 0
            while done < k:
                n = min(k - done, MAX_RUN)
                assert self.eng.loss_grad_adam_step(self.spec, self.scale, b["th"][i], self.X, self.n_res, b["grad"], b["m"][i],
                                                    b["v"][i], self.step + done, [1e-4] * n, **self._kw(b))
                done += n

    def timed(self, fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(k)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt / k * 1e3      # ms per iteration (of all M members)


def measure(name, M, reps, window):
    p = Problem(name, M)
    gx, lds = p.eng.ensemble_plan(M, p.N)
    for fn in (p.ensemble, p.sequential):      # warm-up: code objects loaded, workspaces allocated
        p.timed(fn, 3)
    ks = {}
    for key, fn in (("ensemble", p.ensemble), ("sequential", p.sequential)):
        probe = p.timed(fn, 4)
        ks[key] = int(max(8, min(2048, window / (probe * 1e-3))))
    t = {"ensemble": [], "sequential": []}
    for _ in range(reps):                      # alternating
        t["ensemble"].append(p.timed(p.ensemble, ks["ensemble"]))
        t["sequential"].append(p.timed(p.sequential, ks["sequential"]))
    assert bool(torch.isfinite(p.ens["th"]).all()) and bool(torch.isfinite(p.one["th"]).all())
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"shape": name, "M": M, "gx": gx, "copy_in_lds": bool(lds), "iterations_per_window": ks,
            "ensemble_ms_per_iteration": med["ensemble"], "ensemble_min_max": [min(t["ensemble"]), max(t["ensemble"])],
            "sequential_ms_per_iteration": med["sequential"], "sequential_min_max": [min(t["sequential"]), max(t["sequential"])],
            "ensemble_us_per_member_iteration": med["ensemble"] / M * 1e3,
            "sequential_us_per_member_iteration": med["sequential"] / M * 1e3,
            "speedup": med["sequential"] / med["ensemble"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, nargs="+", default=[1, 4, 16, 64, 256])
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ensemble_speed.py measures on the GPU: no device found")
    rows = []
    for name in a.shapes:
        for M in a.members:
            r = measure(name, M, a.reps, a.window)
            rows.append(r)
            print(f"{name:32s} M={M:4d} gx={r['gx']:3d}: ensemble {r['ensemble_ms_per_iteration']:9.4f} ms/it "
                  f"[{r['ensemble_min_max'][0]:.4f}, {r['ensemble_min_max'][1]:.4f}]  sequential {r['sequential_ms_per_iteration']:9.4f} ms/it "
                  f"[{r['sequential_min_max'][0]:.4f}, {r['sequential_min_max'][1]:.4f}]  x{r['speedup']:.2f}", flush=True)
            if a.out:                # (rewritten after every row: a run cut short keeps what it measured)
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                json.dump({"device": torch.cuda.get_device_name(0), "unit": "ms per Adam iteration of all M members",
                           "reps": a.reps, "window_s": a.window, "rows": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
