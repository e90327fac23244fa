"""Shared by test_residual2_cpu.py / test_residual2_gpu.py: the reference of the residuals with the lateral-mixing term
-nu lap(U) in their momentum equations — the Python formula written with torch.autograd.grad (as
tests/test_jet2_gpu.py::ref_jets), in float64 — and the networks it is evaluated on.  Never the code under test."""
import torch

from oracle import pinn_oracle as O

NS_IN, NS_OUT = ("t", "x", "y"), ("h", "z", "u", "v")
PE_IN, PE_OUT = ("x", "y"), ("h", "U", "V", "eta_mean", "Hrms", "k")
ROLES = {"Navier_Stokes": (NS_IN, NS_OUT), "physics_equation": (PE_IN, PE_OUT)}


def _d(a, b):
    """d a / d b per point, kept differentiable; zeros where a does not depend on b."""
    r = torch.autograd.grad(a.sum(), b, create_graph=True, allow_unused=True)[0]
    return torch.zeros_like(b) if r is None else r


def _lap(a, x, y):
    return _d(_d(a, x), x) + _d(_d(a, y), y)


def formula(name, corrected, nu, ins, outs):
    """The three signed fields (mass, mom_x, mom_y), each (N, 1): physics.Navier_Stokes / physics.physics_equation line
    for line, with -nu (a_xx + a_yy) added to the two momentum equations.  ins: the input columns in role order
    ((t, x, y) resp. (x, y)), each (N, 1) with requires_grad; outs: the output columns in role order."""
    if name == "Navier_Stokes":
        t, x, y = ins
        h, z, u, v = outs
        depth = h + z
        g, gamma_b = 9.81, 0.78
        cb = 3.0 / 16.0 * g * gamma_b ** 2
        mass = _d(z, t) + _d(depth * u, x) + _d(depth * v, y)
        mom_x = _d(u, t) + u * _d(u, x) + v * _d(u, y) + g * _d(z, x) + cb * _d(depth, x) * depth
        mom_y = _d(v, t) + u * _d(v, x) + v * _d(v, y) + g * _d(z, y) + cb * _d(depth, y) * depth
        if nu:
            mom_x = mom_x - nu * _lap(u, x, y)
            mom_y = mom_y - nu * _lap(v, x, y)
        return mass, mom_x, mom_y
    assert name == "physics_equation"
    x, y = ins
    h, U, V, eta_mean, Hrms, k = outs
    g, rho, cd = 9.81, 1025, 0.002
    inv_depth = 1 / (rho * (eta_mean + h))
    mass = _d(U, x) + _d(V, y)
    mom_x = U * _d(U, x) + V * _d(U, y) + g * _d(eta_mean, x) + inv_depth * (rho * cd * U * abs(U))
    mom_y = U * _d(V, x) + V * _d(V, y) + g * _d(eta_mean, y) + inv_depth * (rho * cd * V * abs(V))
    if corrected:
        E = (1.0 / 8.0) * rho * g * Hrms ** 2
        ratio = k * h / torch.sinh(2 * k * h)
        mom_x = mom_x + inv_depth * _d(E * (2 * ratio + 0.5), x)
        mom_y = mom_y + inv_depth * _d(E * ratio, y)
    if nu:
        mom_x = mom_x - nu * _lap(U, x, y)
        mom_y = mom_y - nu * _lap(V, x, y)
    return mass, mom_x, mom_y


def conditioned_params(layers, name, out_names, seed=0, init_type="xavier"):
    """Xavier (or Kaiming) init, output weight x 0.25, and output biases that keep the total depth away from zero:
    physics_equation h = 2.0, eta_mean = 0.2, Hrms = 0.5, k = 1.0 (tests/pe_corrected_util.py); Navier_Stokes h = 2.0,
    z = 0.2.  Columns that carry no role keep their random bias."""
    g = torch.Generator().manual_seed(seed)
    params = O.init_params(layers, init_type, g)
    params[-2] = params[-2] * 0.25
    b = params[-1].clone()
    vals = {"h": 2.0, "eta_mean": 0.2, "Hrms": 0.5, "k": 1.0} if name == "physics_equation" else {"h": 2.0, "z": 0.2}
    for role, val in vals.items():
        b[list(out_names).index(role)] = val
    params[-1] = b
    return params


def points(N, d_in, seed=1):
    return torch.rand(N, d_in, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def net_fields(params, X, name, corrected, nu, in_names, out_names, dtype=torch.float64, init_type="xavier", masks=None,
               p=0.0, device="cpu"):
    """(fields (3, N), parameters with requires_grad) of the formula on the network `params` at the rows of X.
    in_names / out_names: the NETWORK's input and output column names (any order, extra columns allowed)."""
    p64 = [q.detach().to(dtype).to(device).requires_grad_(True) for q in params]
    cols = [X[:, i:i + 1].detach().to(dtype).to(device).requires_grad_(True) for i in range(X.shape[1])]
    if masks is not None:
        masks = [m.to(device) for m in masks]
    Y = O.mlp_forward(p64, torch.cat(cols, -1), init_type, masks, p)
    rin, rout = ROLES[name]
    ins = [cols[list(in_names).index(r)] for r in rin]
    outs = [Y[:, list(out_names).index(r):list(out_names).index(r) + 1] for r in rout]
    f = formula(name, corrected, nu, ins, outs)
    return torch.cat(f, dim=1).t(), p64


def net_sums_grad(params, X, name, corrected, nu, in_names, out_names, scale, **kw):
    """fp64 (term_sums (3,), fields (3, N), flat gradient of sum_t scale[t] term_sums[t])."""
    f, p64 = net_fields(params, X, name, corrected, nu, in_names, out_names, **kw)
    sums = (f ** 2).sum(dim=1)
    obj = (sums * torch.tensor(scale, dtype=f.dtype, device=f.device)).sum()
    return sums.detach(), f.detach(), O.flat_grad(obj, p64).detach()


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
