"""Shared by test_weighted_cpu.py / test_weighted_gpu.py: the reference of the point-weighted residual losses — the formulas of
tests/coef_util.py (at the compiled-in closure constants) and the continuity residuals, written with torch.autograd.grad in
float64 and float32 and evaluated with the weights — the cases the GPU test runs, and its bounds.  Never the code under test.

  term_sums[t] = sum_n w_t[n] f_t[n]^2  for t < n_w = min(n_terms, n_fields); continuity_only's count is never weighted
  gradient     = d/d theta sum_{t < n_w} scale[t] term_sums[t]
  fields       = the unweighted signed f_t, (n_fields, N)

Bounds: sums by sweep2_util.sum_ratio <= 1 (max(2e-6, 4 x the reference's fp32-vs-fp64 gap)); gradient block by block by
trained_state_util.assert_blocks_close (max(2e-5, 4 gap)); fields by sweep2_util.field_ratios <= FIELD_BOUND."""
import functools
from types import SimpleNamespace

import torch

from oracle import pinn_oracle as O
from tests import coef_util as CU
from tests import sweep2_util as S
from tests.trained_state_util import assert_blocks_close, block_errors

SCALE = CU.SCALE
GRAD_FLOOR = CU.GRAD_FLOOR
FIELD_BOUND = S.FIELD_BOUND
N_TERMS, N_FIELDS = S.N_TERMS, S.N_FIELDS
N_W = {r: min(N_TERMS[r], N_FIELDS[r]) for r in N_TERMS}      # 3, 3, 1, 2

CONT_SHAPES = {
    "co_20x20": ("continuity_only", (2, 20, 20, 3), ("x", "y"), ("h", "U", "V"), "xavier"),
    "cf_20x20_4": ("continuity_ftemp", (2, 20, 20, 4), ("x", "y"), ("V", "aux", "h", "U"), "xavier"),   # shuffled columns, one extra
}
SHAPES = {**{k: CU.SHAPES[k] for k in CU.TILE_SHAPES + CU.GENERIC_ONLY}, **CONT_SHAPES}
TILE_SHAPES = CU.TILE_SHAPES + tuple(CONT_SHAPES)      # padded widths 16, 32, 64, 16, 32, 32
GENERIC_ONLY = CU.GENERIC_ONLY
POINTS = (1, 15, 16, 17, 243, 4097)
LARGE = ("pe_10x10", 50021)      # several waves share a gradient copy and walk several tiles
SEED = {**CU.SEED, "co_20x20": 7, "cf_20x20_4": 8}
SMALL_SET, SMALL_SET_DRAWS, NOISE_POINTS = CU.SMALL_SET, CU.SMALL_SET_DRAWS, CU.NOISE_POINTS


def shape_case(shape):
    res, layers, inn, outn, init = SHAPES[shape]
    return SimpleNamespace(res=res, layers=list(layers), inn=tuple(inn), outn=tuple(outn), init=init, d_in=layers[0])


def n_w(shape):
    return N_W[SHAPES[shape][0]]


def w_rows_of(shape):
    """The row counts a case runs with: 1 and n_w (once where n_w == 1)."""
    return (1,) if n_w(shape) == 1 else (1, n_w(shape))


def cases():
    """(shape, N) of the GPU test."""
    out = [(s, N) for s in TILE_SHAPES + GENERIC_ONLY for N in POINTS]
    return out + [LARGE]


def _draw_x(c, N, g):
    X = torch.rand(N, c.d_in, generator=g) * 2 - 1
    if c.res == "continuity_only":
        X[:, c.inn.index("x")] *= 40                                 # x < 25.5 selects a real subset
    return X


def _fields(c, params, X, dtype, graph=False):
    """(F (N, n_fields), count or None, the parameter leaves): the signed fields by the formula in `dtype`."""
    p = [q.detach().to(dtype).requires_grad_(True) for q in params]
    cols = [X[:, i:i + 1].detach().to(dtype).requires_grad_(True) for i in range(X.shape[1])]
    Y = O.mlp_forward(p, torch.cat(cols, -1), c.init, None, 0.0)
    rout, rin = S.ROLES[c.res]
    ins = [cols[c.inn.index(r)] for r in rin]
    outs = [Y[:, c.outn.index(r):c.outn.index(r) + 1] for r in rout]
    count = None
    if c.res in ("Navier_Stokes", "physics_equation"):
        f = CU.formula(c.res, CU.DEFAULTS[c.res], ins, outs)
    else:
        fc = O.continuity_fields(*ins, *outs)
        on = (ins[0] < S.THRESHOLD) if c.res == "continuity_only" else torch.zeros_like(fc, dtype=torch.bool)
        f = (fc, torch.where(on, outs[0] - S.ANCHOR, torch.zeros_like(fc)))
        count = on.sum().to(dtype).reshape(1)
    return torch.cat(f, 1), count, p


def _noise_ratio(c, params, X, Xn):
    """coef_util._noise_ratio for this file's formula: the largest (fp32 noise of field t over the set and the noise points) /
    (the field's rms on the set) over the fields that are not identically zero."""
    Xa = torch.cat([X, Xn])
    f64, f32 = _fields(c, params, Xa, torch.float64)[0].detach(), _fields(c, params, Xa, torch.float32)[0].detach()
    noise = (f32.double() - f64).abs().amax(0)
    rms = f64[:X.shape[0]].square().mean(0).sqrt()
    return max([float(n / r) for n, r in zip(noise, rms) if float(r) > 0] or [0.0])


@functools.lru_cache(maxsize=None)
def inputs(shape, N):
    """(parameters, X (N, d_in)), float32, shared.  The closure shapes take coef_util's inputs as they are; the continuity
    shapes are drawn the same way (below SMALL_SET points: of SMALL_SET_DRAWS draws the one furthest from a cancellation,
    chosen from the reference alone)."""
    if shape in CU.SHAPES:
        return CU.inputs(shape, N)
    c = shape_case(shape)
    g = torch.Generator().manual_seed(9100 + 131 * SEED[shape] + N)
    params = S._params(c, g)
    X = _draw_x(c, N, g)
    if N < SMALL_SET:
        Xn = _draw_x(c, NOISE_POINTS, g)
        draws = [X] + [_draw_x(c, N, g) for _ in range(SMALL_SET_DRAWS - 1)]
        X = min(draws, key=lambda x: _noise_ratio(c, params, x, Xn))
    return params, X.contiguous()


@functools.lru_cache(maxsize=None)
def noise_points(shape):
    c = shape_case(shape)
    return _draw_x(c, NOISE_POINTS, torch.Generator().manual_seed(77 + SEED[shape]))


@functools.lru_cache(maxsize=None)
def weights(shape, N, w_rows):
    """(w_rows, N) float32: uniform in [0, 2] with about a quarter set to exactly 0; a row that came out all zero gets its first
    entry back, so every row keeps a non-zero weight."""
    g = torch.Generator().manual_seed(4400 + 17 * SEED[shape] + 3 * N + w_rows)
    u = torch.rand(w_rows, N, generator=g) * 2
    zero = torch.rand(w_rows, N, generator=g) < 0.25
    for r in range(w_rows):
        if bool(zero[r].all()):
            zero[r, 0] = False
    return torch.where(zero, torch.zeros_like(u), u).contiguous()


def scale_of(shape, N):
    return [s / N for s in SCALE][:N_TERMS[SHAPES[shape][0]]]


def rows(w, nw):
    """The weight row of each weighted term: row 0 for every term when w has one row."""
    return [w[t if w.shape[0] > 1 else 0] for t in range(nw)]


def _evaluate(c, params, X, w, dtype):
    """sums (n_terms), grad (P), fields (n_fields, N) and the per-point squares sq (n_fields, N) in `dtype`; w (w_rows, N)."""
    N, nw, nt = X.shape[0], N_W[c.res], N_TERMS[c.res]
    F, count, p = _fields(c, params, X, dtype)
    sq = (F ** 2).t()                                                # (n_fields, N)
    wr = [r.to(dtype) for r in rows(w, nw)]
    sums = [(wr[t] * sq[t]).sum() for t in range(nw)]
    scale = [s / N for s in SCALE]
    obj = sum(scale[t] * sums[t] for t in range(nw))
    grad = O.flat_grad(obj, p)
    sums = torch.stack(sums)
    if c.res == "continuity_only":
        sums = torch.cat([sums, count])
    return SimpleNamespace(sums=sums.detach()[:nt], grad=grad.detach(), fields=F.detach().t().contiguous(), sq=sq.detach())


CHUNK = 4096      # points per autograd pass of a large case


def evaluate(shape, N, w, dtype, X=None):
    """_evaluate on the case's points.  Above CHUNK points the set is evaluated CHUNK points at a time, every chunk in `dtype`,
    and the chunks' sums and gradients are added in float64: the float32 run's error is then the formula's and the network's
    per point, not that of one 50 000-term float32 sum inside torch's matmul backward, which depends on how many threads the
    CPU at hand splits it over (seen: 9e-8 on one machine and 5.7e-6 on another in the W0 block of the same case)."""
    params, X0 = inputs(shape, N)
    X = X0 if X is None else X
    c = shape_case(shape)
    if N <= CHUNK:
        return _evaluate(c, params, X, w, dtype)
    parts = []
    for a in range(0, N, CHUNK):
        r = _evaluate(c, params, X[a:a + CHUNK], w[:, a:a + CHUNK], dtype)
        r.grad = r.grad.double() * (X[a:a + CHUNK].shape[0] / N)         # (_evaluate scales by its own point count)
        parts.append(r)
    return SimpleNamespace(sums=sum(r.sums.double() for r in parts).to(dtype), grad=sum(r.grad for r in parts).to(dtype),
                           fields=torch.cat([r.fields for r in parts], 1), sq=torch.cat([r.sq for r in parts], 1))


@functools.lru_cache(maxsize=None)
def reference(shape, N, w_rows, ones=False):
    """(r64, r32) with the case's weights (ones: with w == 1), computed once and shared.  r64 carries what field_ratios needs:
    noise = max |f32 - f64| and fmax = max |f64| per field over the case's points and the noise points."""
    c = shape_case(shape)
    w = torch.ones(w_rows, N) if ones else weights(shape, N, w_rows)
    r64, r32 = evaluate(shape, N, w, torch.float64), evaluate(shape, N, w, torch.float32)
    params, _ = inputs(shape, N)
    Xn = noise_points(shape)
    n64, n32 = _fields(c, params, Xn, torch.float64)[0].detach().t(), _fields(c, params, Xn, torch.float32)[0].detach().t()
    a64, a32 = torch.cat([r64.fields, n64], 1), torch.cat([r32.fields.double(), n32.double()], 1)
    r64.noise, r64.fmax = (a32 - a64).abs().amax(1), a64.abs().amax(1)
    r64.sums, r64.grad, r64.fields = r64.sums.double(), r64.grad.double(), r64.fields.double()
    return r64, r32


# ---- bounds ------------------------------------------------------------------------------------------------------------
def sums_ratio(got, r64, r32):
    return S.sum_ratio(got, r64.sums, r32.sums.double())


def grad_ratio(got, r64, r32, layers, what):
    errs = assert_blocks_close(got, r64.grad, r32.grad, layers, what)
    gaps = block_errors(r32.grad, r64.grad, layers)
    return max(e / max(GRAD_FLOOR, 4 * gaps[k]) for k, e in errs.items() if float(gaps[k]) != float("inf"))


def grad_ratio_unasserted(got, r64, r32, layers):
    errs = block_errors(got, r64.grad, layers)
    gaps = block_errors(r32.grad, r64.grad, layers)
    return max(e / max(GRAD_FLOOR, 4 * gaps[k]) for k, e in errs.items())


def field_ratio(got, r64):
    return max(S.field_ratios(got, r64))


# ---- the trainer's self-adaptive loop, restated in torch (test_weighted_gpu.py) ---------------------------------------------
def sa_mask(lam, mask):
    return lam * lam if mask == "square" else lam
