"""Shared by tests/test_balance_cpu.py and tests/test_balance_gpu.py: the balancing rule of include/pinn_hip.h restated in
NumPy float64, the statistics and the combination as the entries define them, Adam's update in the kernels' order, and the
comparison rules of two tile-kernel runs (restated from tests/fold_ext_util.py so that an edit there does not move these
tests)."""
import numpy as np
import torch

NONE, MAX_MEAN, NORM = 0, 1, 2
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def lam_hat(mode, stats, ref, P):
    """(G,) float64: the rule's target weights, NaN where the rule leaves a group alone (MAX_MEAN's reference group)."""
    st = np.asarray(stats, dtype=np.float64)
    G = st.shape[0]
    hat = np.full(G, np.nan)
    with np.errstate(all="ignore"):
        if mode == MAX_MEAN:
            for j in range(G):
                if j != ref:
                    hat[j] = st[ref, 0] / (st[j, 1] / np.float64(P))
        elif mode == NORM:
            total = np.float64(0.0)
            for i in range(G):
                total = total + np.sqrt(st[i, 2])
            for j in range(G):
                hat[j] = total / np.sqrt(st[j, 2])
    return hat


def weights(mode, stats, lam, ref, alpha, P):
    """pinn_balance_weights_host restated: float64 throughout, one rounding to float32; a group whose target is not a finite
    positive number keeps its weight bit for bit."""
    lam = np.asarray(lam, dtype=np.float32)
    out = lam.copy()
    if mode == NONE:
        return out
    hat = lam_hat(mode, stats, ref, P)
    a = np.float64(alpha)
    for j in range(lam.shape[0]):
        if np.isfinite(hat[j]) and hat[j] > 0:
            out[j] = np.float32((np.float64(1.0) - a) * np.float64(lam[j]) + a * hat[j])
    return out


def stats_of(g):
    """(G, 3) float64 of float32 rows g (G, P): max|g|, sum|g|, sum g^2 — exact products, NumPy's float64 sums."""
    g64 = np.asarray(g, dtype=np.float64)
    return np.stack([np.abs(g64).max(1), np.abs(g64).sum(1), (g64 * g64).sum(1)], 1)


def sum_bound(P):
    """Relative distance of two double summations of P exact non-negative terms, worst case: each within (P - 1) 2^-53."""
    return 2.0 * P * 2.0 ** -53


def combine(lam, g):
    """((lam[0] g_0) + (lam[1] g_1)) + ... in float32, every product and sum rounded."""
    lam, g = np.asarray(lam, dtype=np.float32), np.asarray(g, dtype=np.float32)
    acc = lam[0] * g[0]
    for j in range(1, g.shape[0]):
        acc = acc + lam[j] * g[j]
    return acc


def adam_update(p, g, m, v, lr, step):
    """-> (p, m, v) after one step in float32 (csrc/reduce_adam.h: scalars formed in double and cast once, no fused
    multiply-add)."""
    f = np.float32
    bc1, bc2 = 1.0 - BETA1 ** step, 1.0 - BETA2 ** step
    w1, b2, w2, eps, step_size, bc2_sqrt = (f(x) for x in (1.0 - BETA1, BETA2, 1.0 - BETA2, EPS, lr / bc1, np.sqrt(bc2)))
    m = m + w1 * (g - m)
    v = v * b2
    v = v + (w2 * g) * g
    denom = np.sqrt(v) / bc2_sqrt + eps
    return p - step_size * (m / denom), m, v


def close(a, b):
    """Two tile-kernel runs' parameters and moments (tests/test_adam_fold_gpu.py's rule: a workgroup's gradient copy is added
    to in lock order, run-to-run differences of ~1e-6)."""
    return bool(torch.allclose(a, b, rtol=2e-4, atol=1e-7 * float(b.abs().max())))


def rel_l2(a, b):
    n = float(b.double().norm())
    return float((a.double() - b.double()).norm()) / n if n > 0 else float((a.double() - b.double()).norm())


GRAD_REL_L2 = 5e-6      # two tile-kernel runs' gradients (tests/test_fold_ext_gpu.py); the weights made from them get the same


# ---- the trainer tests' problem: physics_equation on 2 -> 10 x 10 -> 6, 243 collocation and 12 fidelity points ---------------
PE_OUT = ("h", "U", "V", "eta_mean", "Hrms", "k")
LAYERS = [2] + [10] * 10 + [6]
LR, STEP, GAMMA, ITERS, EVERY, ALPHA = 1e-3, 7, 0.8, 12, 3, 0.5
N_RES, N_FID = 243, 12


def trainer_cfg(lbfgs_it=0, **loss):
    return {
        "layers": {"input_features": 2, "hidden_layers": len(LAYERS) - 2, "hidden_width": 10, "output_features": 6, "dropout_rate": 0.0,
                   "init_type": "xavier"},
        "adam_optimizer": {"max_it": ITERS, "learning_rate": LR, "scheduler_step_size": STEP, "scheduler_gamma": GAMMA},
        "lbfgs_optimizer": {"max_it": lbfgs_it, "learning_rate": 1, "max_evaluation": 12, "history_size": 10,
                            "tolerance_grad": 1e-9, "tolerance_change": 1e-12, "line_search_fn": "strong_wolfe"},
        "loss": {"weight_fid_loss": 1, "weight_res_loss": 1, **{f"weight_{k}_loss": 1 for k in PE_OUT}, **loss},
        "data_fidelity": {"inputs": ["x", "y"], "outputs": list(PE_OUT), "training_points": N_FID},
        "data_residual": {"inputs": {"x": {"requires_grad": ["true"]}, "y": {"requires_grad": ["true"]}}, "outputs": list(PE_OUT)},
    }


def trainer_data():
    """-> (params, Xf, Tf, Xr) on the CPU: conditioned parameters (depth positive), uniform points in [-1, 1]^2."""
    from tests.residual2_util import conditioned_params
    g = torch.Generator().manual_seed(91)
    params = conditioned_params(LAYERS, "physics_equation", PE_OUT, seed=17)
    Xr, Xf = torch.rand(N_RES, 2, generator=g) * 2 - 1, torch.rand(N_FID, 2, generator=g) * 2 - 1
    Tf = torch.rand(N_FID, 6, generator=g)
    return params, Xf, Tf, Xr


def trainer_model(params):
    from pinn_depthestimation_amd.dnn import DNN
    m = DNN(LAYERS, 0.0, "xavier")
    with torch.no_grad():
        for i, lin in enumerate(m._linears()):
            lin.weight.copy_(params[2 * i]); lin.bias.copy_(params[2 * i + 1])
    return m


def balanced_loop(params, Xf, Tf, Xr, mode, groups, ref, dtype, iters=ITERS, every=EVERY, alpha=ALPHA):
    """The balanced Adam stage in torch autograd on oracle.pinn_oracle's network and residual fields: per-group
    gradients by autograd; statistics, the rule and torch.optim.Adam + StepLR in `dtype`.  -> (the hand-weighted total
    fid + res per iteration, as the trainer logs it; the weights each iteration stepped with, (iters, G))."""
    from oracle import pinn_oracle as O
    p = [q.detach().clone().to(dtype).requires_grad_(True) for q in params]
    opt = torch.optim.Adam(p, lr=LR)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=STEP, gamma=GAMMA)
    Xf_, Tf_ = Xf.to(dtype), Tf.to(dtype)
    G = 2 if groups == "sets" else 4
    r = 0 if ref == "residual" else G - 1
    lam = torch.ones(G, dtype=dtype)
    losses, lams = [], []
    for it in range(iters):
        cols = [Xr[:, i:i + 1].to(dtype).requires_grad_(True) for i in range(2)]
        Y = O.mlp_forward(p, torch.cat(cols, -1))
        f = torch.cat(O.physics_equation_fields(cols[0], cols[1], *[Y[:, j:j + 1] for j in range(6)]), 1)      # (N, 3)
        terms = (f ** 2).mean(0)
        fid = ((Tf_ - O.mlp_forward(p, Xf_)) ** 2).mean(0).sum()
        parts = ([terms.sum()] if groups == "sets" else [terms[0], terms[1], terms[2]]) + [fid]
        gs = [torch.cat([g.reshape(-1) for g in torch.autograd.grad(L, p, retain_graph=True)]) for L in parts]
        losses.append(float((terms.sum() + fid).detach()))
        if it % every == 0:
            if mode == "max_mean":
                hat = [gs[r].abs().max() / gs[j].abs().mean() for j in range(G)]
            else:
                tot = sum(g.square().sum().sqrt() for g in gs)
                hat = [tot / g.square().sum().sqrt() for g in gs]
            for j in range(G):
                if not (mode == "max_mean" and j == r):
                    lam[j] = (1 - alpha) * lam[j] + alpha * hat[j]
        lams.append(lam.clone().double().numpy())
        g = sum(lam[j] * gs[j] for j in range(G))
        off = 0
        for q in p:
            q.grad = g[off:off + q.numel()].reshape(q.shape).clone(); off += q.numel()
        opt.step(); sched.step()
    return np.array(losses), np.stack(lams)
