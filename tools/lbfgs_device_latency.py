#!/usr/bin/env python3
"""lbfgs_device_latency.py — wall time per L-BFGS iteration and per evaluation of the three drivers of the L-BFGS
stage (trainer.PINN(lbfgs_impl=...)): "torch" (torch.optim.LBFGS), "flat" (lbfgs.FlatLBFGS: the batched recursion, line
search on the host) and "device" (lbfgs.DeviceLBFGS: runs of evaluations decided on the device).  History 100, strong
Wolfe, tolerances 0: the reference's settings (train.py:116-125).  The problems of tools/lbfgs_latency.py plus the
reference's own shapes.  Every line is a fresh trainer after one warm-up run of the same kind (kernels loaded, workspaces
allocated); the clock runs from the call of the L-BFGS stage to a device synchronisation after it.

    python tools/lbfgs_device_latency.py [impl ...]        (default: flat torch device)
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pinn_depthestimation_amd.trainer import PINN
from small_n_latency import ns_config

PE_ROLES = ["h", "U", "V", "eta_mean", "Hrms", "k"]


def cmb_config():
    """config_CMB.json's shape: 2 -> 10 x 10 -> 6, physics_equation, weighted fidelity on all six outputs."""
    return {
        "layers": {"input_features": 2, "hidden_layers": 10, "hidden_width": 10, "output_features": 6, "dropout_rate": 0.0,
                   "init_type": "xavier"},
        "adam_optimizer": {"max_it": 0, "learning_rate": 1e-4, "scheduler_step_size": 10000, "scheduler_gamma": 0.8},
        "lbfgs_optimizer": {"max_it": 0, "learning_rate": 1, "history_size": 100, "line_search_fn": "strong_wolfe"},
        "loss": {f"weight_{k}_loss": 1 for k in PE_ROLES + ["fid", "res"]},
        "data_fidelity": {"inputs": ["x", "y"], "outputs": PE_ROLES, "training_points": 12},
        "data_residual": {"inputs": {k: {"requires_grad": ["true"]} for k in "xy"}, "outputs": PE_ROLES},
    }


def newmethod_config():
    """config_CMB_h.json's shape (train_newmethod.py): 2 -> 100 x 20 -> 3, continuity_only, U and V known on every point."""
    return {
        "layers": {"input_features": 2, "hidden_layers": 100, "hidden_width": 20, "output_features": 3, "dropout_rate": 0.0,
                   "init_type": "xavier"},
        "adam_optimizer": {"max_it": 0, "learning_rate": 1e-4, "scheduler_step_size": 10000, "scheduler_gamma": 0.8},
        "lbfgs_optimizer": {"max_it": 0, "learning_rate": 1, "history_size": 100, "line_search_fn": "strong_wolfe"},
        "loss": {"weight_fid_loss": 1, "weight_res_loss": 1},
        "data": {"inputs": {k: {"requires_grad": ["true"]} for k in "xy"}, "trues": ["U", "V"], "unknowns": ["h"]},
    }


def rand(n, d, seed):
    return (torch.rand(n, d, generator=torch.Generator().manual_seed(seed)) * 2 - 1).numpy()


def workloads():
    yield "config_CMB 10x10 N_res=243 N_fid=12", cmb_config, lambda: (rand(12, 2, 2), rand(12, 6, 3) * 0.1 + 0.5, rand(243, 2, 1)), 100
    for n in (243, 10000):
        yield f"Navier-Stokes 8x64 N={n}", lambda: ns_config(0), (lambda n=n: (None, None, rand(n, 3, 1234))), 100
    yield "train_newmethod 100x20 N=12514", newmethod_config, lambda: (rand(12514, 2, 1), rand(12514, 2, 3) * 0.1, None), 60
    yield "Navier-Stokes 8x64 N=2^20", lambda: ns_config(0), lambda: (None, None, rand(1 << 20, 3, 1234)), 15


def condition(tr, cfg):
    """physics_equation needs eta_mean + h away from 0: output weights x 0.25, biases h = 2, eta_mean = 0.2, Hrms = 0.5, k = 1."""
    outs = cfg.get("data_residual", {}).get("outputs", [])
    if "eta_mean" not in outs:
        return
    last = [m for m in tr.dnn.modules() if isinstance(m, torch.nn.Linear)][-1]
    with torch.no_grad():
        last.weight.mul_(0.25)
        for name, val in (("h", 2.0), ("eta_mean", 0.2), ("Hrms", 0.5), ("k", 1.0)):
            last.bias[outs.index(name)] = val


def run(cfg_fn, data_fn, impl, iters):
    cfg = cfg_fn()
    cfg["lbfgs_optimizer"].update({"max_it": iters, "tolerance_grad": 0.0, "tolerance_change": 0.0, "history_size": 100})
    cfg["lbfgs_optimizer"].pop("max_evaluation", None)
    Xf, Tf, Xr = data_fn()
    if Xr is None:
        Xr = Xf                      # one point set for both terms (train_newmethod.py:122-159)
    torch.manual_seed(1234)
    tr = PINN(Xf, Tf, Xr, cfg, log_every=1, checkpoint_every=0, lbfgs_impl=impl, log_flush_every=4096)
    condition(tr, cfg)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.train()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if impl == "device":
        n_it = tr.device_lbfgs.n_iter
    else:
        n_it = tr.optimizer_LBFGS.state_dict()["state"][0]["n_iter"]
    return dt, n_it, tr.iter, tr.last[2].item()


def main():
    impls = sys.argv[1:] or ["flat", "torch", "device"]
    for name, cfg_fn, data_fn, iters in workloads():
        for impl in impls:
            run(cfg_fn, data_fn, impl, min(iters, 10))                    # warm-up
            dt, n_it, evals, loss = run(cfg_fn, data_fn, impl, iters)
            print(f"{name:38s} {impl:6s}: {n_it:4d} iterations, {evals:4d} evaluations in {dt * 1e3:9.2f} ms = "
                  f"{dt / max(n_it, 1) * 1e3:7.3f} ms/iteration, {dt / max(evals, 1) * 1e6:9.1f} us/evaluation; final loss {loss:.6e}",
                  flush=True)


if __name__ == "__main__":
    main()
