"""Shared by test_coef_cpu.py / test_coef_gpu.py: the reference of the residuals with their closure coefficient as a tensor
(gamma_b of Navier_Stokes, Cd of physics_equation) — the Python formula written with torch.autograd.grad in float64 and
float32 — the cases the GPU test runs, and its bounds.  Never the code under test."""
import functools
from types import SimpleNamespace

import torch

from oracle import pinn_oracle as O
from tests import sweep2_util as S
from tests.residual2_util import ROLES, _d
from tests.trained_state_util import assert_blocks_close, block_errors

G = 9.81
RHO = 1025
DEFAULTS = {"Navier_Stokes": 0.78, "physics_equation": 0.002}
COEF_NAME = {"Navier_Stokes": "gamma_b", "physics_equation": "Cd"}
SCALE = (0.7, 1.3, 0.9)       # unequal term scales (divided by N in the cases)
GRAD_FLOOR = 2e-5             # the project's gradient floor


def formula(name, coef, ins, outs):
    """The three signed fields (mass, mom_x, mom_y), each (N, 1): physics.Navier_Stokes / physics.physics_equation line for
    line with the closure coefficient `coef` (a tensor broadcastable against (N, 1)) in place of 0.78 / 0.002."""
    if name == "Navier_Stokes":
        t, x, y = ins
        h, z, u, v = outs
        depth = h + z
        cb = 3.0 / 16.0 * G * coef ** 2
        mass = _d(z, t) + _d(depth * u, x) + _d(depth * v, y)
        mom_x = _d(u, t) + u * _d(u, x) + v * _d(u, y) + G * _d(z, x) + cb * _d(depth, x) * depth
        mom_y = _d(v, t) + u * _d(v, x) + v * _d(v, y) + G * _d(z, y) + cb * _d(depth, y) * depth
        return mass, mom_x, mom_y
    assert name == "physics_equation"
    x, y = ins
    h, U, V, eta_mean, Hrms, k = outs
    inv_depth = 1 / (RHO * (eta_mean + h))
    mass = _d(U, x) + _d(V, y)
    mom_x = U * _d(U, x) + V * _d(U, y) + G * _d(eta_mean, x) + inv_depth * (RHO * coef * U * abs(U))
    mom_y = U * _d(V, x) + V * _d(V, y) + G * _d(eta_mean, y) + inv_depth * (RHO * coef * V * abs(V))
    return mass, mom_x, mom_y


# ---- the GPU test's cases ----------------------------------------------------------------------------------------------
# shape: (residual, layers, network input names, network output names, init type)
SHAPES = {
    "pe_10x10": ("physics_equation", (2, 10, 10, 6), ("x", "y"), ("h", "U", "V", "eta_mean", "Hrms", "k"), "xavier"),
    "pe_20x20x20_7": ("physics_equation", (2, 20, 20, 20, 7), ("x", "y"), ("k", "aux", "V", "h", "Hrms", "U", "eta_mean"), "xavier"),
    "ns_64x64": ("Navier_Stokes", (3, 64, 64, 4), ("t", "x", "y"), ("h", "z", "u", "v"), "xavier"),
    "ns_10x10x10_5": ("Navier_Stokes", (3, 10, 10, 10, 5), ("t", "x", "y"), ("v", "aux", "h", "u", "z"), "xavier"),
    "pe_10hidden_x10": ("physics_equation", (2,) + (10,) * 10 + (6,), ("x", "y"), ("h", "U", "V", "eta_mean", "Hrms", "k"), "xavier"),   # config_CMB's depth
    # the generic engine alone: a width the MFMA instances do not serve, and LeakyReLU
    "pe_100x100": ("physics_equation", (2, 100, 100, 6), ("x", "y"), ("h", "U", "V", "eta_mean", "Hrms", "k"), "xavier"),
    "ns_12x12_leaky": ("Navier_Stokes", (3, 12, 12, 4), ("t", "x", "y"), ("h", "z", "u", "v"), "kaiming"),
}
SEED = {"ns_10x10x10_5": 0, "ns_12x12_leaky": 1, "ns_64x64": 2, "pe_100x100": 3, "pe_10x10": 4, "pe_20x20x20_7": 5, "pe_10hidden_x10": 6}
TILE_SHAPES = ("pe_10x10", "pe_20x20x20_7", "ns_64x64", "ns_10x10x10_5")      # padded widths 16, 32, 64, 16
GENERIC_ONLY = ("pe_100x100", "ns_12x12_leaky")
COEFS = {"physics_equation": (0.002, 0.5), "Navier_Stokes": (0.78, 0.4)}
POINTS = (1, 15, 16, 17, 243, 4097)
LARGE = ("pe_10x10", 0.5, 50021)      # several waves share a gradient copy and walk several tiles


def shape_case(shape):
    res, layers, inn, outn, init = SHAPES[shape]
    return SimpleNamespace(res=res, layers=list(layers), inn=tuple(inn), outn=tuple(outn), init=init, d_in=layers[0])


SMALL_SET = 16           # point sets below one 16-point tile (sweep2_util.SMALL_SET)
SMALL_SET_NOISE = 1e-6   # sweep2_util.SMALL_SET_NOISE
NOISE_POINTS = 256


def _params(c, g):
    if c.init == "xavier":
        return S._params(c, g)
    from tests.trained_state_util import trained_like      # (trained_like's hidden biases on a Kaiming init, the same output biases)
    params = trained_like(c.layers, g, residual=c.res, outn=c.outn, init_type=c.init)
    b = params[-1].clone()
    b[c.outn.index("h")], b[c.outn.index("z")] = 2.0, 0.2
    params[-1] = b
    return params


def _noise_ratio(c, params, X, Xn):
    """sweep2_util.small_set_noise for a set of fewer than SMALL_SET points, from the reference alone: the largest nu_t / rms_t
    over the fields and both coefficient values, nu_t the network's fp32 noise level of field t (max |f32 - f64| over the set
    and NOISE_POINTS more points), rms_t the field's root mean square on the set.  With one or fifteen points |s32 - s64| is one
    or fifteen roundings, no noise estimate, so the sum bound falls to its 2e-6 floor, which a kernel as good as the reference
    meets only where nu / rms is about 1e-6: a point on a cancellation (a field of 1e-3 between terms of order 1) is a badly
    chosen case, not a finding."""
    Xa = torch.cat([X, Xn])
    worst = 0.0
    for coef in COEFS[c.res]:
        f64, f32 = _evaluate(c, params, Xa, coef, torch.float64).fields, _evaluate(c, params, Xa, coef, torch.float32).fields
        noise = (f32.double() - f64).abs().amax(0)
        rms = f64[:X.shape[0]].square().mean(0).sqrt()
        worst = max(worst, float((noise / rms).max()))
    return worst


SMALL_SET_DRAWS = 24


@functools.lru_cache(maxsize=None)
def inputs(shape, N):
    """(parameters [W0, b0, ...] float32, X (N, d_in) float32): trained_like plus the output biases sweep2_util._params sets;
    one draw per (shape, N), shared (callers leave them unchanged).  Below SMALL_SET points: of SMALL_SET_DRAWS draws of the
    point set, the one furthest from a cancellation (smallest _noise_ratio) — a choice made from the reference alone."""
    c = shape_case(shape)
    g = torch.Generator().manual_seed(9100 + 131 * SEED[shape] + N)
    params = _params(c, g)
    X = torch.rand(N, c.d_in, generator=g) * 2 - 1
    if N < SMALL_SET:
        Xn = torch.rand(NOISE_POINTS, c.d_in, generator=g) * 2 - 1
        draws = [X] + [torch.rand(N, c.d_in, generator=g) * 2 - 1 for _ in range(SMALL_SET_DRAWS - 1)]
        X = min(draws, key=lambda x: _noise_ratio(c, params, x, Xn))
    return params, X.contiguous()


def _evaluate(c, params, X, coef, dtype):
    """The formula on the network `params` at the rows of X in `dtype`, the coefficient a tensor: term sums (3,), the flat
    parameter gradient and the coefficient gradient of sum_t scale[t] sums[t] (scale = SCALE / N), the per-point contributions
    to the latter (N,), the fields (N, 3), and what the misreadings of test_coef_cpu need: rx, ry and d f_x / d coef,
    d f_y / d coef per point."""
    N = X.shape[0]
    p = [q.detach().to(dtype).requires_grad_(True) for q in params]
    cols = [X[:, i:i + 1].detach().to(dtype).requires_grad_(True) for i in range(X.shape[1])]
    cvec = torch.full((N, 1), coef, dtype=dtype, requires_grad=True)       # one copy per point: its gradient is per point
    Y = O.mlp_forward(p, torch.cat(cols, -1), c.init, None, 0.0)
    rin, rout = ROLES[c.res]
    ins = [cols[c.inn.index(r)] for r in rin]
    outs = [Y[:, c.outn.index(r):c.outn.index(r) + 1] for r in rout]
    f = torch.cat(formula(c.res, cvec, ins, outs), dim=1)                  # (N, 3)
    scale = torch.tensor([s / N for s in SCALE], dtype=dtype)
    sums = (f ** 2).sum(dim=0)
    obj = (sums * scale).sum()
    gs = torch.autograd.grad(obj, p + [cvec], retain_graph=True)
    dfx = torch.autograd.grad(f[:, 1].sum(), cvec, retain_graph=True)[0].reshape(-1)
    dfy = torch.autograd.grad(f[:, 2].sum(), cvec)[0].reshape(-1)
    per_point = gs[-1].reshape(-1).detach()
    fd = f.detach()
    return SimpleNamespace(sums=sums.detach(), grad=torch.cat([g_.reshape(-1) for g_ in gs[:-1]]).detach(), fields=fd,
                           gc=float(per_point.double().sum()), per_point=per_point, A=float(per_point.double().abs().sum()),
                           rx=2 * scale[1] * fd[:, 1], ry=2 * scale[2] * fd[:, 2], dfx=dfx.detach(), dfy=dfy.detach())


def evaluate(shape, N, coef, dtype):
    params, X = inputs(shape, N)
    return _evaluate(shape_case(shape), params, X, coef, dtype)


@functools.lru_cache(maxsize=None)
def reference(shape, N, coef):
    """(r64, r32): evaluate() in float64 and in float32, computed once and shared."""
    return evaluate(shape, N, coef, torch.float64), evaluate(shape, N, coef, torch.float32)


def scale_of(N):
    return [s / N for s in SCALE]


# ---- bounds ------------------------------------------------------------------------------------------------------------
def sums_ratio(got, r64, r32):
    """sweep2_util.sum_ratio: the worst relative error of a term sum over max(2e-6, 4 x the reference's own fp32 gap)."""
    return S.sum_ratio(got, r64.sums, r32.sums)


def grad_ratio(got, r64, r32, layers, what):
    """assert_blocks_close (max(2e-5, 4 gap) per block), and the worst block error over its bound: test_sweep2_gpu.gradient_ratio."""
    errs = assert_blocks_close(got, r64.grad, r32.grad, layers, what)
    gaps = block_errors(r32.grad, r64.grad, layers)
    return max(e / max(GRAD_FLOOR, 4 * gaps[k]) for k, e in errs.items() if float(gaps[k]) != float("inf"))


def grad_ratio_unasserted(got, r64, r32, layers):
    """grad_ratio's number without its assertion (test_coef_cpu's misreadings must FAIL the bound)."""
    errs = block_errors(got, r64.grad, layers)
    gaps = block_errors(r32.grad, r64.grad, layers)
    return max(e / max(GRAD_FLOOR, 4 * gaps[k]) for k, e in errs.items())


def coef_grad_bound(r64, r32):
    """|got - g64| <= max(4 |g32 - g64|, 2e-5 A), A = sum_n |per-point contribution| in fp64."""
    return max(4 * abs(r32.gc - r64.gc), GRAD_FLOOR * r64.A)


def coef_grad_ratio(got, r64, r32):
    b = coef_grad_bound(r64, r32)
    e = abs(float(got) - r64.gc)
    return e / b if b > 0 else (0.0 if e == 0 else float("inf"))
