"""Shared by test_pe_corrected_cpu.py / test_pe_corrected_gpu.py: the reference of the corrected radiation-stress
residual — the Python formula of physics.physics_equation(..., corrected=True), evaluated with torch autograd over
oracle.mlp_forward on the CPU — and the networks it is evaluated on."""
import torch

from oracle import pinn_oracle as O

ROLES = ("h", "U", "V", "eta_mean", "Hrms", "k")


def pec_fields(x, y, h, U, V, eta_mean, Hrms, k):
    """(mass, mom_x, mom_y) of physics.physics_equation(..., corrected=True), its lines term for term."""
    d = O.compute_gradient
    g, rho, cd = 9.81, 1025, 0.002
    inv_depth = 1 / (rho * (eta_mean + h))
    mass = d(U, x) + d(V, y)
    mom_x = U * d(U, x) + V * d(U, y) + g * d(eta_mean, x) + inv_depth * (rho * cd * U * abs(U))
    mom_y = U * d(V, x) + V * d(V, y) + g * d(eta_mean, y) + inv_depth * (rho * cd * V * abs(V))
    E = (1.0 / 8.0) * rho * g * Hrms ** 2
    ratio = k * h / torch.sinh(2 * k * h)
    mom_x = mom_x + inv_depth * d(E * (2 * ratio + 0.5), x)
    mom_y = mom_y + inv_depth * d(E * ratio, y)
    return mass, mom_x, mom_y


def pec_loss(x, y, h, U, V, eta_mean, Hrms, k):
    return sum(torch.mean(f ** 2) for f in pec_fields(x, y, h, U, V, eta_mean, Hrms, k))


def conditioned_params(layers, outputs=ROLES, seed=0, init_type="xavier"):
    """Xavier (or Kaiming) init, output weight x 0.25, output biases h = 2.0, eta_mean = 0.2, Hrms = 0.5, k = 1.0: kh in
    [1.6, 2.4] and eta + h in [1.9, 2.5] on X in [-1, 1], where the stress terms carry weight and fp32 noise stays at 2e-7."""
    g = torch.Generator().manual_seed(seed)
    params = O.init_params(layers, init_type, g)
    params[-2] = params[-2] * 0.25
    b = params[-1].clone()
    for name, val in (("h", 2.0), ("eta_mean", 0.2), ("Hrms", 0.5), ("k", 1.0)):
        b[list(outputs).index(name)] = val
    params[-1] = b
    return params


def points(N, d_in=2, seed=1):
    return torch.rand(N, d_in, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def net_fields(params, X, xcol=0, ycol=1, outputs=ROLES, dtype=torch.float64, init_type="xavier"):
    """The three fields (3, N) of the formula on the network `params` at the rows of X, in `dtype` on the CPU; the
    parameters it was evaluated with (requires_grad) come back too."""
    p = [q.detach().to(dtype).requires_grad_(True) for q in params]
    cols = O.split_columns(X.to(dtype), (xcol, ycol))
    Y = O.mlp_forward(p, torch.cat(cols, dim=-1), init_type)
    outs = [Y[:, list(outputs).index(r):list(outputs).index(r) + 1] for r in ROLES]
    f = pec_fields(cols[xcol], cols[ycol], *outs)
    return torch.cat(f, dim=1).t(), p


def net_loss_grad(params, X, dtype=torch.float64, **kw):
    """(loss, flat gradient) of the formula in `dtype`."""
    f, p = net_fields(params, X, dtype=dtype, **kw)
    loss = (f ** 2).mean(dim=1).sum()
    return float(loss.detach()), O.flat_grad(loss, p).double()

