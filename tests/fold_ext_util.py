"""Shared by tests/test_fold_ext_cpu.py and tests/test_fold_ext_gpu.py: the multiplier step of pinn_adam_loop_ext's finishing
kernel restated in NumPy — trainer.sa_weight_grad followed by torch.optim.Adam's single-tensor update, every operation
rounded in `dtype` and in the kernel's order — the comparison rules of two tile-kernel runs, and the trainer tests' problems with their
float64 / float32 torch loops (the problems and loops tests/test_coef_gpu.py and tests/test_weighted_gpu.py hold the classic
path to, restated here so that this file's tests do not change with an edit there)."""
import numpy as np
import torch

from oracle import pinn_oracle as O

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def adam_scalars(lr, step, dtype):
    """torch.optim.Adam's scalars, formed in double as Python forms them and cast once (csrc/reduce_adam.h, adam_scalars)."""
    bc1, bc2 = 1.0 - BETA1 ** step, 1.0 - BETA2 ** step
    return tuple(dtype(x) for x in (1.0 - BETA1, BETA2, 1.0 - BETA2, EPS, lr / bc1, np.sqrt(bc2)))


def adam_update(p, g, m, v, lr, step, dtype):
    """-> (p, m, v) after one step (csrc/reduce_adam.h, adam_update): no fused multiply-add, every product and sum rounded."""
    w1, b2, w2, eps, step_size, bc2_sqrt = adam_scalars(lr, step, dtype)
    m = m + w1 * (g - m)
    v = v * b2
    v = v + (w2 * g) * g
    denom = np.sqrt(v) / bc2_sqrt + eps
    return p - step_size * (m / denom), m, v


def sa_grad(lam, fields, scale, mask):
    """trainer.sa_weight_grad in NumPy: sf = (s_t f) f, summed over the weighted terms in term order for a shared row;
    -((2 lam) sf) for "square", -sf for "linear".  lam (rows, N), fields (n_fields, N), scale (n_terms,)."""
    dtype = lam.dtype.type
    n_w = min(len(scale), fields.shape[0])
    sf = [(dtype(scale[t]) * fields[t]) * fields[t] for t in range(n_w)]
    if lam.shape[0] == 1:
        tot = sf[0]
        for t in range(1, n_w):
            tot = tot + sf[t]
        sf = tot[None]
    else:
        sf = np.stack(sf)
    return -((dtype(2.0) * lam) * sf) if mask == "square" else -sf


def multiplier_step(lam, lam_m, lam_v, fields, scale, mask, lr_w, step):
    """One multiplier step of the finishing kernel: -> (lam, lam_m, lam_v, point_w) after it, in lam's dtype."""
    dtype = lam.dtype.type
    g = sa_grad(lam, fields, scale, mask).astype(lam.dtype)
    lam, lam_m, lam_v = adam_update(lam, g, lam_m, lam_v, lr_w, step, dtype)
    return lam, lam_m, lam_v, (lam * lam if mask == "square" else lam.copy())


def close(a, b):
    """Two tile-kernel runs' parameters, moments, coefficients or multipliers (tests/test_adam_fold_gpu.py's rule)."""
    return bool(torch.allclose(a, b, rtol=2e-4, atol=1e-7 * float(b.abs().max())))


def rel_l2(a, b):
    n = float(b.double().norm())
    return float((a.double() - b.double()).norm()) / n if n > 0 else float((a.double() - b.double()).norm())


# ---- the trainer tests' problems: physics_equation, 243 collocation and 12 fidelity points, StepLR(7, 0.8), 20 iterations ----
PE_OUT = ("h", "U", "V", "eta_mean", "Hrms", "k")
LR, LR_W, STEP, GAMMA, ITERS = 1e-3, 1e-2, 7, 0.8, 20
N_RES, N_FID = 243, 12
# kind: (layers, seed of the point sets, seed of the conditioned parameters)
PROBLEMS = {"coef": ([2] + [10] * 10 + [6], 77, 11), "weights": ([2, 10, 10, 6], 78, 12)}


def trainer_cfg(kind, lbfgs_it=0, **loss):
    layers = PROBLEMS[kind][0]
    return {
        "layers": {"input_features": 2, "hidden_layers": len(layers) - 2, "hidden_width": 10, "output_features": 6, "dropout_rate": 0.0,
                   "init_type": "xavier"},
        "adam_optimizer": {"max_it": ITERS, "learning_rate": LR, "weight_learning_rate": LR_W, "scheduler_step_size": STEP,
                           "scheduler_gamma": GAMMA},
        "lbfgs_optimizer": {"max_it": lbfgs_it, "learning_rate": 1, "max_evaluation": 12, "history_size": 10,
                            "tolerance_grad": 1e-9, "tolerance_change": 1e-12, "line_search_fn": "strong_wolfe"},
        "loss": {"weight_fid_loss": 1, "weight_res_loss": 1, **{f"weight_{k}_loss": 1 for k in PE_OUT}, **loss},
        "data_fidelity": {"inputs": ["x", "y"], "outputs": list(PE_OUT), "training_points": N_FID},
        "data_residual": {"inputs": {"x": {"requires_grad": ["true"]}, "y": {"requires_grad": ["true"]}}, "outputs": list(PE_OUT)},
    }


def trainer_data(kind):
    """-> (params, Xf, Tf, Xr) on the CPU: conditioned parameters (depth positive), uniform points in [-1, 1]^2."""
    from tests.residual2_util import conditioned_params
    layers, seed, pseed = PROBLEMS[kind]
    g = torch.Generator().manual_seed(seed)
    params = conditioned_params(layers, "physics_equation", PE_OUT, seed=pseed)
    Xr, Xf = torch.rand(N_RES, 2, generator=g) * 2 - 1, torch.rand(N_FID, 2, generator=g) * 2 - 1
    Tf = torch.rand(N_FID, 6, generator=g)
    return params, Xf, Tf, Xr


def trainer_model(kind, params):
    from pinn_depthestimation_amd.dnn import DNN
    m = DNN(PROBLEMS[kind][0], 0.0, "xavier")
    with torch.no_grad():
        for i, lin in enumerate(m._linears()):
            lin.weight.copy_(params[2 * i]); lin.bias.copy_(params[2 * i + 1])
    return m


def _pe_fields(p, Xr, cd, dtype):
    from tests.coef_util import formula
    cols = [Xr[:, i:i + 1].to(dtype).requires_grad_(True) for i in range(2)]
    Y = O.mlp_forward(p, torch.cat(cols, -1))
    return torch.cat(formula("physics_equation", cd, cols, [Y[:, j:j + 1] for j in range(6)]), 1)      # (N, 3)


def cd_loop(params, Xf, Tf, Xr, cd0, dtype):
    """torch.optim.Adam over network and Cd, one StepLR: (total loss per iteration, Cd before each step)."""
    p = [q.detach().clone().to(dtype).requires_grad_(True) for q in params]
    cd = torch.tensor(cd0, dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam(p + [cd], lr=LR)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=STEP, gamma=GAMMA)
    Xf_, Tf_ = Xf.to(dtype), Tf.to(dtype)
    losses, cds = [], []
    for _ in range(ITERS):
        opt.zero_grad()
        fid = ((Tf_ - O.mlp_forward(p, Xf_)) ** 2).mean(0).sum()
        loss = fid + (_pe_fields(p, Xr, cd, dtype) ** 2).mean(0).sum()
        losses.append(float(loss.detach())); cds.append(float(cd.detach()))
        loss.backward()
        opt.step(); sched.step()
    return np.array(losses), np.array(cds)


def sa_loop(params, Xf, Tf, Xr, mask, dtype):
    """The self-adaptive algorithm in torch: Adam on the network (descent) and on lambda (3, N) (ascent: its gradient
    negated), one StepLR for both: (total loss per iteration, final lambda)."""
    p = [q.detach().clone().to(dtype).requires_grad_(True) for q in params]
    lam = torch.ones(3, Xr.shape[0], dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([{"params": p, "lr": LR}, {"params": [lam], "lr": LR_W}])
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=STEP, gamma=GAMMA)
    Xf_, Tf_ = Xf.to(dtype), Tf.to(dtype)
    losses = []
    for _ in range(ITERS):
        opt.zero_grad()
        fid = ((Tf_ - O.mlp_forward(p, Xf_)) ** 2).mean(0).sum()
        f = _pe_fields(p, Xr, 0.002, dtype).t()
        w = lam * lam if mask == "square" else lam
        loss = fid + (w * f ** 2).sum() / Xr.shape[0]
        losses.append(float(loss.detach()))
        loss.backward()
        lam.grad.neg_()
        opt.step(); sched.step()
    return np.array(losses), lam.detach()
