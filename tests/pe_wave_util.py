"""Shared by test_pe_wave_cpu.py / test_pe_wave_gpu.py: the reference of the wave closure — the five fields of
physics.physics_equation(..., corrected=True, wave_omega=, wave_gamma=), evaluated with torch autograd over
oracle.mlp_forward on the CPU.  Fields 0..2 are pe_corrected_util.pec_fields; the networks and points are that module's."""
import math

import torch

from oracle import pinn_oracle as O
from tests.pe_corrected_util import ROLES, pec_fields

OMEGA, GAMMA = 2.5, 0.42      # the GPU tests' wave: T = 2.5 s, Thornton & Guza's breaker index
N_TERMS = 5


def wave_fields(x, y, h, U, V, eta_mean, Hrms, k, omega=OMEGA, gamma=GAMMA):
    """(mass, mom_x, mom_y, dispersion, energy) of physics.physics_equation(corrected=True, wave_omega=, wave_gamma=), its
    lines term for term."""
    d = O.compute_gradient
    g = 9.81
    s = k * h
    disp = g * k * torch.tanh(s) / omega ** 2 - 1
    cg = (omega / k) * (0.5 + s / torch.sinh(2 * s))
    q = Hrms / (gamma * h)
    eps = (1.5 * math.sqrt(math.pi)) * (omega / (2 * math.pi)) * Hrms ** 5 / (gamma ** 2 * h ** 3) * (1 - (1 + q ** 2) ** (-2.5))
    energy = d(Hrms ** 2 * cg, x) + eps
    return (*pec_fields(x, y, h, U, V, eta_mean, Hrms, k), disp, energy)


def wave_loss(x, y, *outs, omega=OMEGA, gamma=GAMMA):
    return sum(torch.mean(f ** 2) for f in wave_fields(x, y, *outs, omega=omega, gamma=gamma))


def net_fields(params, X, xcol=0, ycol=1, outputs=ROLES, dtype=torch.float64, init_type="xavier", omega=OMEGA, gamma=GAMMA):
    """The five fields (5, N) of the formula on the network `params` at the rows of X, in `dtype` on the CPU; the parameters
    it was evaluated with (requires_grad) come back too."""
    p = [q.detach().to(dtype).requires_grad_(True) for q in params]
    cols = O.split_columns(X.to(dtype), (xcol, ycol))
    Y = O.mlp_forward(p, torch.cat(cols, dim=-1), init_type)
    outs = [Y[:, list(outputs).index(r):list(outputs).index(r) + 1] for r in ROLES]
    f = wave_fields(cols[xcol], cols[ycol], *outs, omega=omega, gamma=gamma)
    return torch.cat(f, dim=1).t(), p


def net_term_grads(params, X, dtype=torch.float64, **kw):
    """(term sums (5,) — sums over points of the squared fields —, the flat gradient of every term's MEAN (5, P)) of the
    formula in `dtype`, as doubles: the gradient of any weighting of the terms is a combination of the rows."""
    f, p = net_fields(params, X, dtype=dtype, **kw)
    means = (f ** 2).mean(dim=1)
    rows = []
    for t in range(N_TERMS):
        g = torch.autograd.grad(means[t], p, retain_graph=True, allow_unused=True)
        rows.append(torch.cat([(torch.zeros_like(q) if gi is None else gi).reshape(-1) for gi, q in zip(g, p)]).double())
    return (f ** 2).sum(dim=1).detach().double(), torch.stack(rows)
