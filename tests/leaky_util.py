"""Shared by test_leaky_cpu.py / test_leaky_gpu.py: the seeded draws of the LeakyReLU sweep, their kink-free point sets and
their fp64 reference.

init_type "kaiming" selects a LeakyReLU(0.01) network (PINN_ACT_LEAKY_RELU), for which the library ships tile, cooperative,
plain-forward, external-adjoint, field, second-order and generic kernels; the other sweeps run loss + gradient with tanh
only.  Every result here is held to the Python formula evaluated with torch autograd on the CPU in float64
(oracle/pinn_oracle.py with init_type="kaiming"), never to another engine.

The kink.  LeakyReLU's derivative jumps by a factor of 100 at z = 0.  A unit whose pre-activation lies within fp32 rounding
of 0 may take the other slope in an fp32 run than in the fp64 reference, and the two then differ by far more than rounding:
off the kink a comparison means something only if NO unit of ANY point sits that close.  kink_free_points builds the point
sets by rejection: tau_l = KINK_MARGIN x e_l per hidden layer, e_l = max |z32 - z64| of the oracle's own forward pass on a
pilot draw of the case's distribution, and a candidate point is redrawn while any hidden unit has |z64| < tau_l.  The margin
of 16 covers another summation order (MFMA k-steps) and the fact that a maximum over a pilot set is no bound.  ON the kink
the named cases (origin, axis, negative zero) put exact zeros into z on purpose: there the arithmetic is exact on both
sides, and what is tested is the convention (torch: slope 0.01 at z == 0), not rounding.

Families (FAMILIES): loss, adam, adj, fields, fwd, second; served(family, case, engine) restates include/pinn_hip.h.
Bounds: the project's existing rules (sweep2_util.field_ratios / sum_ratio, trained_state_util.assert_blocks_close /
abs_bound)."""
import functools
import random
from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import pinn_oracle as O
from tests import residual2_util as R2
from tests import sweep2_util as S
from tests.trained_state_util import trained_like

INIT = "kaiming"
SLOPE = 0.01
FAMILIES = ("loss", "adam", "adj", "fields", "fwd", "second")
KINK_MARGIN = 16.0       # tau_l = KINK_MARGIN x e_l
PILOT_POINTS = 1024
MAX_REJECTED = 0.25      # a case whose filter rejects more than this share of its candidates is badly chosen
CUS = 256                # compute units of an MI355X: the cooperative kernel serves AUTO while tiles <= CUS (pinn_fused.hip use_coop)

DEPTHS = [1, 2, 3, 4, 6, 8, 12]
WIDTHS = S.WIDTHS
WIDE_WIDTHS = [65, 100, 128, 200, 256]
POINTS = [1, 15, 16, 17, 37, 243, 777, 4097, 9600]
ROLES, N_TERMS, N_FIELDS = S.ROLES, S.N_TERMS, S.N_FIELDS
THRESHOLD, ANCHOR = S.THRESHOLD, S.ANCHOR
NOISE_POINTS = S.NOISE_POINTS
SMALL_SET, SMALL_SET_NOISE = S.SMALL_SET, S.SMALL_SET_NOISE
# The committed seeds keep every block's gap (the reference's own fp32 run against its fp64 run) below this; GAP_CAP = 5e-6 is
# what assert_blocks_close enforces.  The fp32 run's sums over the points depend on the CPU's matrix kernels (a 9600-point
# case: 3.6e-6 on one machine, 7.5e-6 on another; 777 points of 12 x 3: 2.7e-6 and 4.5e-6), so the seeds were chosen with the
# figures of two kinds of machine, and a seed above the margin on either is skipped.
GAP_MARGIN = 4e-6


def gap_margin(c):
    return GAP_MARGIN

# The committed seeds: a range per family without the seeds that break a condition of test_leaky_cpu.py on the reference
# alone (SKIPPED, with the reason per seed in DESIGN.md 4.5).
_RANGES = {"loss": range(0, 44), "adam": range(100, 144), "adj": range(200, 232), "fields": range(300, 334),
           "fwd": range(400, 430), "second": range(500, 534)}
#   small set on a cancellation   loss 4, 7, 11, 19, 27, 29; adam 103; second 501, 504, 513, 520, 521, 522 (small_set_noise >
#                                 SMALL_SET_NOISE)
#   block gap                     loss 23, 26; adj 202, 205; second 510 (3.7e-6 .. 4.7e-6 on one of the two machines); adam 112, 120 and
#                                 second 502 (physics_equation near eta_mean + h = 0: up to 3e-3).  No slope is flipped in any of
#                                 them (checked unit by unit): conditioning, not the kink
#   block gap, second iteration   adam 121, 129, 134, 138, 139: at the parameters one Adam step on, on the second point set,
#                                 4e-6 .. 1.2e-5
#   jets                          fwd 412, 416, 419 (12 x 17 and 40 x 24): the reference's own fp32 jets use more than half of the
#                                 2e-6 bound
# The adam family caps its depth at 12 and its point count at 777.  At depth 40 every draw broke the second-iteration rule, and
# one of them (40 x 24 on exactly 16 points, a field noise of 1.8e-5 of the fields' rms) sat 1.06 x above the 2e-6 floor of the
# sum bound on the tile kernel with every gradient block within bounds: one tile of roundings on a cancellation, which
# small_set_noise covers only below 16 points.  From 4097 points on, six of its seven draws broke a gap rule on one machine or the
# other; large point sets are the loss family's.
SKIPPED = {"loss": [4, 7, 11, 19, 23, 26, 27, 29], "adam": [103, 112, 120, 121, 129, 134, 138, 139], "adj": [202, 205], "fields": [], "fwd": [412, 416, 419],
           "second": [501, 502, 504, 510, 513, 520, 521, 522]}
SEEDS = {f: [s for s in _RANGES[f] if s not in SKIPPED[f]] for f in _RANGES}


def padded_width(W):
    return 16 if W <= 16 else 32 if W <= 32 else 64


def fits_lds(L, W):
    """pinn_fused.hip fits_lds restated: the tile kernel keeps its padded gradient copy (PP floats) in LDS while it fits
    beside the fixed part (locks, transpose pads, partial sums) within 160 KiB, else in the workspace (global memory)."""
    wp = padded_width(W)
    pp = wp * 16 + (L - 1) * wp * wp + 16 * wp + L * wp + 16
    fixed = 128 + 4 * 8 * 256 + 4 * 12
    return 4 * (pp + fixed) <= 160 * 1024


def coop_fits(L, W, K1):
    """pinn_fused.hip coop_lds_bytes restated: the cooperative kernel's gradient copy, 2 K1 x 4 pads and sums in 160 KiB."""
    wp = padded_width(W)
    pp = wp * 16 + (L - 1) * wp * wp + 16 * wp + L * wp + 16
    return 4 * (pp + 2 * K1 * 4 * 256 + 12) <= 160 * 1024


@dataclass(frozen=True)
class Case:
    family: str
    seed: int
    res: Optional[str]                  # None: no residual attached (adj, fwd, and the loss family's "mse" kind)
    nu: float
    inn: Tuple[str, ...]
    outn: Tuple[str, ...]
    gc: Tuple[int, ...]
    L: int
    W: int
    N: int
    kind: str = "residual"              # residual / onepass / split / mse
    mode: str = "both"                  # adj: gY / gdY / both
    name: str = ""                      # the named cases: origin / axis
    lr: float = 1e-3                    # adam
    corrected: bool = False             # physics_equation with the corrected radiation stress (the "elsewhere" cases)

    @property
    def d_in(self): return len(self.inn)

    @property
    def d_out(self): return len(self.outn)

    @property
    def k(self): return len(self.gc)

    @property
    def K1(self): return 1 + self.k

    @property
    def wp(self): return padded_width(self.W)

    @property
    def layers(self): return O.layer_sizes(self.d_in, self.L, self.W, self.d_out)

    @property
    def n_fid(self): return {"residual": 0, "onepass": self.N, "mse": self.N, "split": max(1, self.N // 5)}[self.kind]

    @property
    def n_res(self): return self.N - self.n_fid if self.kind == "split" else (0 if self.kind == "mse" else self.N)

    @property
    def fid_cols(self):
        if self.kind == "residual":
            return []
        return sorted(random.Random(self.seed).sample(range(self.d_out), min(self.d_out, 1 + self.seed % 3)))

    @property
    def extra_dir(self):
        return self.res is not None and self.k > len(ROLES[self.res][1])

    @property
    def col0_is_no_role(self):
        return self.res is not None and self.outn[0] not in ROLES[self.res][0]

    @property
    def in_lds(self): return fits_lds(self.L, self.W)

    def term_scale(self):
        return [s / max(self.n_res, 1) for s in [1.0, 0.5, 2.0, 1.5][:N_TERMS[self.res]]]

    def col_scale(self):
        return [0.7 / max(self.n_fid, 1)] * len(self.fid_cols)

    def tag(self):
        what = "" if self.res is None else self.res + ("+c" if self.corrected else "") + (f" nu={self.nu}" if self.nu else "") + " "
        tail = self.mode if self.family == "adj" else self.kind if self.family in ("loss", "adam") else ""
        return (f"{self.family} {self.name or 'seed'} {self.seed}: {what}{self.d_in}->{self.L}x{self.W}->{self.d_out} k={self.k} "
                f"N={self.N} {tail}").rstrip()


def _columns(r, res, extra_in=(0, 0, 1, 2), extra_out=(0, 0, 1, 3), p_extra_dir=0.0):
    out_roles, dir_roles = ROLES[res]
    inn = list(dir_roles) + [f"in{i}" for i in range(r.choice(extra_in))]
    outn = list(out_roles) + [f"out{i}" for i in range(r.choice(extra_out))]
    r.shuffle(inn); r.shuffle(outn)
    gc = sorted(inn.index(d) for d in dir_roles)
    extra = [i for i in range(len(inn)) if i not in gc]
    if extra and len(gc) < 3 and r.random() < p_extra_dir:
        gc = sorted(gc + [r.choice(extra)])
    return tuple(inn), tuple(outn), tuple(gc)


def _free_net(r, ks):
    d_in, d_out = r.choice([2, 3, 3, 4, 5, 8]), r.choice([1, 2, 3, 4, 6, 9, 16])
    k = min(r.choice(ks), d_in)
    gc = tuple(sorted(r.sample(range(d_in), k)))
    return tuple(f"in{i}" for i in range(d_in)), tuple(f"out{i}" for i in range(d_out)), gc


def draw(family, seed):
    """The case of (family, seed), from random.Random alone."""
    r = random.Random(f"leaky/{family}/{seed}")
    L = r.choice(DEPTHS) if r.random() > 0.1 else 40
    if family == "adam" and L == 40: L = 12                # (see SKIPPED: two iterations at depth 40 are ill-conditioned in every draw)
    wide = r.random() < 0.1
    W = r.choice(WIDE_WIDTHS) if wide else r.choice(WIDTHS)
    N = r.choice(POINTS)
    if L == 40: W, N = min(W, 24), min(N, 4097)
    if W > 64: L, N = min(L, 4), min(N, 777)              # (the AUTO-to-generic route; its fp64 reference stays small)
    if L >= 12 and W > 32: N = min(N, 4097)
    res, nu, kind, mode = None, 0.0, "residual", "both"
    if family in ("loss", "adam"):
        kind = r.choice(["residual", "residual", "onepass", "split", "mse"] if family == "loss" else ["residual", "onepass", "split"])
        if kind == "mse":                                 # the fidelity term alone: k = 0 (K1 = 1) two draws in three
            inn, outn, gc = _free_net(r, [0, 0, 2, 3])
        else:
            res = r.choice(sorted(ROLES))
            inn, outn, gc = _columns(r, res, p_extra_dir=0.5)
        if family == "adam":
            N = min(max(N, 16), 777)                      # (larger point sets: the loss family; see SKIPPED)
            if kind == "split" and padded_width(W) == 64: kind = "onepass"      # (two passes there: not a folded request, a named case)
    elif family == "adj":
        inn, outn, gc = _free_net(r, [2, 3, 3, 0])
        mode = r.choice(["gY", "gdY", "both", "both"]) if gc else "gY"
    elif family == "fwd":
        inn, outn, gc = _free_net(r, [0, 1, 2, 3, 3])
    elif family == "fields":
        res = r.choice(sorted(ROLES))
        inn, outn, gc = _columns(r, res)
    else:
        assert family == "second"
        res = r.choice(["Navier_Stokes", "physics_equation"])
        nu = r.choice([0.05, 1.0])
        inn, outn, gc = _columns(r, res)
        N = min(N, 4097)
    c = Case(family, seed, res, nu, inn, outn, gc, L, W, N, kind, mode)
    if c.kind == "split" and c.n_res == 0:
        c = replace(c, kind="residual")
    return c


# ---- what the header documents as served for LeakyReLU -----------------------------------------------------------------
def served(family, c, engine, entry=None):
    """Whether include/pinn_hip.h says the LeakyReLU call of this family on case `c` is served under `engine` ("auto",
    "generic", "fused", "tile", "coop", "batch", "wide").  fp32, no dropout, d_in and d_out <= 16.
      loss / adam   GENERIC any shape.  FUSED: width <= 64, tanh or LeakyReLU, gradient passes k = 0, 2 or 3; FUSED_COOP
                    padded width 64 only; FUSED_BATCH has no LeakyReLU instance and "falls back to _TILE" (PINN_ENGINE_FUSED_BATCH);
                    WIDE requires tanh: refused, and width 65..256 under AUTO runs the generic kernels
      adj           FUSED (every sub-value) width <= 64, k in {0, 2, 3} or no gdY; WIDE refused
      fields        k == the residual's directions; FUSED width <= 64, tanh or LeakyReLU; GENERIC / AUTO any
      fwd           pinn_forward / pinn_forward_jet: FUSED width <= 64 (any k <= 3)
      second        FUSED: every layer at most 64 wide; residual2 wants k == the residual's directions"""
    if engine == "generic":
        ok = True
    elif engine == "wide":
        ok = False
    elif engine == "auto":
        ok = True
    else:
        ok = c.W <= 64 and c.d_in <= 16 and c.d_out <= 16
        if engine == "coop" and family in ("loss", "adam", "fwd"):
            ok = ok and c.wp == 64
    if family in ("loss", "adam") and entry != "residual_loss":
        ok = ok and c.k in (0, 2, 3)
    if family == "adj":
        if engine not in ("auto", "generic"):
            ok = ok and (c.k in (0, 2, 3) or c.mode == "gY")
    if family == "fields" or (family == "second" and entry == "residual2"):
        ok = ok and c.k == len(ROLES[c.res][1])
    if family == "second" and engine not in ("auto", "generic"):
        ok = ok and max(c.layers) <= 64
    return ok


def engines(family, c):
    """The engines the GPU module runs the case on."""
    if family == "loss":
        return ["generic", "tile"] + (["coop"] if c.wp == 64 else ["batch"]) + ["auto"]
    if family == "adam":
        return ["auto", "tile"]
    if family in ("adj", "fields"):
        return ["tile", "auto", "generic"]
    return ["auto", "fused", "generic"]


def adam_folded(c, engine):
    """Whether loss_grad_adam_step serves the case as ONE pass of the fused engine (else it reports False and launches nothing):
    width <= 64, and not the split request at padded width 64 outside the cooperative kernel (two passes there)."""
    if c.W > 64 or c.k not in (0, 2, 3):
        return False
    coop = engine == "auto" and c.wp == 64 and coop_fits(c.L, c.W, c.K1) and (c.N + 15) // 16 <= CUS
    return not (c.kind == "split" and c.wp == 64 and not coop)


# ---- the oracle's forward pass, layer by layer ---------------------------------------------------------------------------
def hidden_z(params, X, dtype, masks=None, p=0.0):
    """[z_l (N, width)] of every hidden layer: O.mlp_forward's own operations (F.linear, F.leaky_relu, the dropout masks),
    kept layer by layer."""
    q = [t.detach().to(dtype) for t in params]
    a, out = X.detach().to(dtype), []
    for i in range(len(q) // 2 - 1):
        z = F.linear(a, q[2 * i], q[2 * i + 1])
        out.append(z)
        a = F.leaky_relu(z, SLOPE)
        if masks is not None:
            a = a * masks[i].to(dtype) / (1.0 - p)
    return out


def kink_tau(params, pilot):
    """(e_l, tau_l) per hidden layer: e_l = max |z32 - z64| of the oracle's forward pass over the pilot points."""
    z32, z64 = hidden_z(params, pilot, torch.float32), hidden_z(params, pilot, torch.float64)
    e = [float((a.double() - b).abs().max()) for a, b in zip(z32, z64)]
    return e, [KINK_MARGIN * v for v in e]


def off_the_kink(params, tau, X, exact_zero_ok=False, masks=None, p=0.0):
    """(N,) bool: no hidden unit of the point has |z64| < tau_l.  exact_zero_ok (the named cases): a unit whose z is exactly
    0.0 in the fp32 AND the fp64 run is on the kink on purpose and does not reject its point."""
    ok = torch.ones(X.shape[0], dtype=torch.bool)
    z32 = hidden_z(params, X, torch.float32) if exact_zero_ok else None
    for l, (z, t) in enumerate(zip(hidden_z(params, X, torch.float64, masks, p), tau)):
        near = z.abs() < t
        if exact_zero_ok:
            near = near & ~((z == 0) & (z32[l] == 0))
        ok &= ~near.any(1)
    return ok


def kink_free_points(params, N, sampler, g, margin=1.0):
    """N points of sampler(n, g)'s distribution off the kink of `params`, by rejection from the seeded generator g.
    Returns (X (N, d_in), SimpleNamespace(e, tau, rejected share of the candidates examined))."""
    e, tau = kink_tau(params, sampler(PILOT_POINTS, g))
    tau = [margin * t for t in tau]
    kept, seen, n_kept = [], 0, 0
    while n_kept < N:
        cand = sampler(max(64, N), g)
        ok = off_the_kink(params, tau, cand)
        kept.append(cand[ok]); seen += cand.shape[0]; n_kept += int(ok.sum())
        assert seen < 64 * max(64, N), "the filter rejects almost every point"
    rejected = 1.0 - n_kept / seen
    return torch.cat(kept)[:N].contiguous(), SimpleNamespace(e=e, tau=tau, rejected=rejected)


# ---- data ----------------------------------------------------------------------------------------------------------------
def _params(c, g, hidden_bias=0.5):
    """The biased state on a Kaiming init (trained_like; hidden_bias = 0: plain init_params), physics_equation with the
    sweeps' conditioning (output layer x 0.25, test_sweep_gpu.py), the output biases of sweep2_util._params."""
    p = trained_like(c.layers, g, bias=hidden_bias, residual=c.res, outn=c.outn, init_type=INIT)
    if hidden_bias == 0.0:
        for i in range(c.L):
            p[2 * i + 1] = torch.zeros(c.W)                              # (init_params' own +0.0, not a product's -0.0)
    b = p[-1].clone()
    if c.res == "physics_equation":
        b[c.outn.index("Hrms")] = 0.5
    if c.res == "Navier_Stokes":
        b[c.outn.index("h")], b[c.outn.index("z")] = 2.0, 0.2
    p[-1] = b
    return p


def sampler_of(c):
    def sample(n, g):
        X = torch.rand(n, c.d_in, generator=g) * 2 - 1
        if c.res == "continuity_only":
            X[:, c.inn.index("x")] *= 40                                 # x < 25.5 selects a real subset
        return X
    return sample


def _finish(c, params, X, kink, g, Xn=None):
    T = torch.rand(c.n_fid, len(c.fid_cols), generator=g) if c.kind != "residual" else None
    gY = gdY = None
    if c.family == "adj":
        gY, gdY = torch.randn(c.N, c.d_out, generator=g), torch.randn(c.k, c.N, c.d_out, generator=g)
    return SimpleNamespace(case=c, params=params, X=X.contiguous(), T=T, gY=gY, gdY=gdY, Xn=Xn, kink=kink)


@functools.lru_cache(maxsize=None)
def data(family, seed):
    """The case with its parameters, kink-free points, targets and adjoints: float32 on the CPU, computed once and shared
    (callers leave them unchanged).  Xn: NOISE_POINTS more kink-free points (the field bound's noise level, as sweep2)."""
    c = draw(family, seed)
    g = torch.Generator().manual_seed(9000 + 131 * FAMILIES.index(family) + seed)
    params = _params(c, g)
    if family == "adam":
        return _adam_data(c, params, g)
    X, kink = kink_free_points(params, c.N, sampler_of(c), g)
    Xn, _ = kink_free_points(params, NOISE_POINTS, sampler_of(c), g)
    return _finish(c, params, X, kink, g, Xn)


ADAM_MARGIN = 2.0        # the second iteration's points stay ADAM_MARGIN x tau off the kink of the parameters after the first step


def adam_steps_fp64(c, params, Xs, T):
    """The parameters after one Adam iteration per point set of Xs on the case's objective in float64 (O.adam_trajectory)."""
    calls = iter(Xs)
    fn = lambda q: objective(c, q, next(calls).double(), None if T is None else T.double())[0]
    return O.adam_trajectory([p.double() for p in params], fn, len(Xs), c.lr)[1]


def _adam_data(c, params, g):
    """Two folded iterations read their points at two parameter vectors, and a point off the kink of the first may sit on the
    kink of the second (one Adam step moves every weight by about lr = 1e-3, z by far more than tau).  So the second iteration
    gets its own point set X2 of the same size, as a mini-batch loop hands it one: off the kink, by ADAM_MARGIN x tau, of
    theta1 = the parameters one fp64 Adam step on X after `params` (kink.theta1, kink.tau1).  The device's own theta1 differs
    from that by rounding; the GPU module checks X2 against it at 1 x tau before it compares."""
    X, kink = kink_free_points(params, c.N, sampler_of(c), g)
    T = torch.rand(c.n_fid, len(c.fid_cols), generator=g) if c.kind != "residual" else None
    th1 = adam_steps_fp64(c, params, [X], T)
    X2, kink2 = kink_free_points(th1, c.N, sampler_of(c), g, margin=ADAM_MARGIN)
    kink.theta1, kink.tau1, kink.rejected = th1, [t / ADAM_MARGIN for t in kink2.tau], max(kink.rejected, kink2.rejected)
    Xn, _ = kink_free_points(params, NOISE_POINTS, sampler_of(c), g)
    return SimpleNamespace(case=c, params=params, X=X, X2=X2, T=T, gY=None, gdY=None, Xn=Xn, kink=kink)


# ---- the named cases on the kink --------------------------------------------------------------------------------------------
NAMED_NETS = [(3, 16), (3, 20), (2, 64), (10, 10)]
NAMED_RES = {2: ["continuity_ftemp", "physics_equation", "continuity_only", "continuity_ftemp"], 3: ["Navier_Stokes"] * 4}
NAMED = [(name, L, W, k) for name in ("origin", "axis") for (L, W) in NAMED_NETS for k in (2, 3)]


def grid(k):
    """The 5 x 5 (k = 2) or 3 x 3 x 3 (k = 3) symmetric grid on [-1, 1]: one point is exactly the origin."""
    ax = torch.linspace(-1, 1, 5 if k == 2 else 3)
    return torch.cartesian_prod(*([ax] * k)).float().contiguous()


@functools.lru_cache(maxsize=None)
def named(name, L, W, k, family="loss", negative_zero=False):
    """origin: zero hidden biases (plain init_params, Kaiming) on the symmetric grid, so z == 0.0 in every unit of every layer
    at the origin.  axis: non-zero biases in all hidden layers but the first, and half of the first layer's units keep only
    the weight of the LAST input column: on the grid rows whose last coordinate is exactly 0 those units have z_0 == 0.0
    while the others are ordinary.  The grid points with a unit within tau of the kink that is not an exact zero are
    dropped.  negative_zero: every 0.0 of X replaced by -0.0."""
    i = NAMED_NETS.index((L, W))
    res = NAMED_RES[k][i] if family in ("loss", "fields", "adam", "second") else None
    if family == "second":
        res = "Navier_Stokes" if k == 3 else "physics_equation"
    if res is not None:
        out_roles, dir_roles = ROLES[res]
        inn, outn = tuple(dir_roles), tuple(out_roles)
    else:
        inn, outn = tuple(f"in{j}" for j in range(k)), tuple(f"out{j}" for j in range(3))
    seed = 10 * i + k + (100 if name == "axis" else 0)
    c = Case(family, seed, res, 0.05 if family == "second" else 0.0, inn, outn, tuple(range(k)), L, W, 0, name=name)
    g = torch.Generator().manual_seed(7700 + seed)
    params = _params(c, g, hidden_bias=0.0 if name == "origin" else 0.5)
    if name == "axis":
        params[1] = torch.zeros_like(params[1])
        w0 = params[0].clone()
        w0[: W // 2, : k - 1] = 0.0
        params[0] = w0
    X = grid(k)
    if res == "continuity_only":
        X[:, 0] *= 40
    _, tau = kink_tau(params, sampler_of(c)(PILOT_POINTS, g))
    ok = off_the_kink(params, tau, X, exact_zero_ok=True)
    X = X[ok].contiguous()
    z = hidden_z(params, X, torch.float64)
    exact = int(sum(((a == 0).sum()) for a in z))
    if negative_zero:
        X = torch.where(X == 0, torch.full_like(X, -0.0), X)
    c = replace(c, N=X.shape[0])
    Xn, _ = kink_free_points(params, NOISE_POINTS, sampler_of(c), g)
    d = _finish(c, params, X, SimpleNamespace(tau=tau, dropped=int((~ok).sum()), exact_zeros=exact), g, Xn)
    return d


# ---- the families that have no LeakyReLU instance on the fused engine --------------------------------------------------------
NS_IO = (("t", "x", "y"), ("h", "z", "u", "v"), (0, 1, 2))
PE_IO = (("x", "y"), ("h", "U", "V", "eta_mean", "Hrms", "k"), (0, 1))
ELSEWHERE = {
    # name: (residual, corrected, (input names, output names, differentiated columns), hidden layers, width, points)
    "coefficient": ("Navier_Stokes", False, NS_IO, 3, 20, 243),
    "weighted": ("physics_equation", False, PE_IO, 4, 12, 243),
    "corrected": ("physics_equation", True, PE_IO, 3, 20, 243),
    "ensemble": ("continuity_ftemp", False, (("x", "y"), ("h", "U", "V"), (0, 1)), 3, 16, 37),
    "dropout": ("Navier_Stokes", False, NS_IO, 4, 48, 243),
}
DROPOUT_P, DROPOUT_SEED = 0.3, 20241004


@functools.lru_cache(maxsize=None)
def elsewhere(name):
    """The named case of a family the fused engine refuses for LeakyReLU, with its kink-free points and (fp64, fp32)
    reference.  weighted: one weight per point, U(0.5, 1.5).  dropout: the engine's own masks (dropout_util.keep_masks, a
    function of the point's index), the filter run on the masked forward pass and failing points redrawn in place."""
    res, corrected, (inn, outn, gc), L, W, N = ELSEWHERE[name]
    c = Case("elsewhere", sorted(ELSEWHERE).index(name), res, 0.0, inn, outn, gc, L, W, N, name=name, corrected=corrected)
    g = torch.Generator().manual_seed(8800 + c.seed)
    params = _params(c, g)
    kw = {}
    if name == "dropout":
        from tests.dropout_util import keep_masks
        masks = [torch.from_numpy(m) for m in keep_masks(DROPOUT_SEED, DROPOUT_P, L, W, N)]
        kw = dict(masks=masks, p=DROPOUT_P)
        e, tau = kink_tau(params, sampler_of(c)(PILOT_POINTS, g))
        X, seen = sampler_of(c)(N, g), N
        while True:
            ok = off_the_kink(params, tau, X, masks=masks, p=DROPOUT_P)
            if bool(ok.all()):
                break
            X[~ok] = sampler_of(c)(int((~ok).sum()), g); seen += int((~ok).sum())
        kink = SimpleNamespace(e=e, tau=tau, rejected=1.0 - N / seen)
    else:
        X, kink = kink_free_points(params, N, sampler_of(c), g)
    if name == "weighted":
        kw = dict(weights=torch.rand(1, N, generator=g) + 0.5)
    d = _finish(c, params, X, kink, g)
    d.kw = kw
    d.ref = tuple(evaluate(c, params, X, None, t, **kw) for t in (torch.float64, torch.float32))
    return d


# ---- mis-readings of LeakyReLU (through autograd, in the reference's precision) ---------------------------------------------
def net(q, x, mis=None, masks=None, p=0.0):
    """The network's output.  mis = None: the oracle (O.mlp_forward with init_type "kaiming").  mis = (kind, layer): what a wrong
    kernel would compute — a_l = s_l z_l with the slopes s_l read wrongly in hidden layer `layer` (None: every layer);
    the slopes are constants of the piece, so autograd carries them into the tangents and the reverse sweep alike."""
    if mis is None:
        return O.mlp_forward(q, x, INIT, masks, p)
    kind, layer = mis
    n_lin, a = len(q) // 2, x
    for i in range(n_lin):
        z = F.linear(a, q[2 * i], q[2 * i + 1])
        if i == n_lin - 1:
            return z
        zd = z.detach()
        lo, hit = SLOPE, layer is None or i == layer
        if hit and kind == "tanh":
            a = torch.tanh(z)
            continue
        if hit and kind == "relu": lo = 0.0
        if hit and kind == "tenth": lo = 0.1
        pos = (zd >= 0) if (hit and kind == "one at zero") else (zd > 0)
        s = torch.where(pos, torch.ones_like(zd), torch.full_like(zd, lo))
        if hit and kind == "neighbour":
            s = torch.roll(s, -1, 1)                                     # unit j takes unit j + 1's slope
        a = s * z
    raise AssertionError


class _Scale(torch.autograd.Function):
    """z * s_fwd, with s_bwd in the reverse sweep."""
    @staticmethod
    def forward(ctx, z, s_fwd, s_bwd):
        ctx.save_for_backward(s_bwd)
        return z * s_fwd

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


def explicit_jets(q, X, gc, mis=None):
    """(Y (N, d_out), dY (k, N, d_out)) carried forward layer by layer (value and k tangents), differentiable once with respect
    to q.  mis = ("tangent", l, j): layer l applies the slope to the value and to every tangent but tangent j; ("reverse", l):
    layer l's reverse sweep applies no slope (forward unchanged).  mis = None equals autograd's jets (test_leaky_cpu.py)."""
    a = X
    da = [torch.zeros_like(X) for _ in gc]
    for j, col in enumerate(gc):
        da[j][:, col] = 1.0
    n_lin = len(q) // 2
    for i in range(n_lin):
        z = F.linear(a, q[2 * i], q[2 * i + 1])
        dz = [F.linear(t, q[2 * i]) for t in da]
        if i == n_lin - 1:
            return z, (torch.stack(dz) if dz else z.new_zeros(0, *z.shape))
        s = torch.where(z.detach() > 0, torch.ones_like(z), torch.full_like(z, SLOPE)).detach()
        one = torch.ones_like(s)
        hit = mis is not None and mis[1] == i
        sb = one if hit and mis[0] == "reverse" else s
        a = _Scale.apply(z, s, sb)
        bare = [hit and mis[0] == "tangent" and j == mis[2] for j in range(len(dz))]
        da = [_Scale.apply(t, one if bare[j] else s, one if bare[j] else sb) for j, t in enumerate(dz)]
    raise AssertionError


MISREADINGS = ("relu", "tanh", "neighbour", "tenth", "tangent", "reverse")      # ("one at zero": the origin case only)


def mis_layer(c):
    """The hidden layer a one-layer mis-reading sits in: it moves with the seed."""
    return c.seed % c.L


# ---- the reference -------------------------------------------------------------------------------------------------------
def _leaf(params, X, dtype):
    q = [t.detach().to(dtype).requires_grad_(True) for t in params]
    cols = [X[:, i:i + 1].detach().to(dtype).requires_grad_(True) for i in range(X.shape[1])]
    return q, cols


def objective(c, q, X, T, mis=None, weights=None, masks=None, p=0.0):
    """(the scalar objective, term sums, column sums, fields (n_fields, n_res)) of the case's request at the parameter list q
    (tensors of X's dtype), differentiable with respect to q: sweep2_util.evaluate with the LeakyReLU network (net)."""
    dtype = X.dtype
    cols = [X[:, i:i + 1].detach().requires_grad_(True) for i in range(X.shape[1])]
    Y = net(q, torch.cat(cols, -1), mis, masks, p)
    obj, sums, F_ = 0.0, torch.zeros(0, dtype=dtype), torch.zeros(0, 0, dtype=dtype)
    if c.res is not None:
        out_roles, dir_roles = ROLES[c.res]
        ins = [cols[c.inn.index(r)] for r in dir_roles]
        outs = [Y[:, c.outn.index(r):c.outn.index(r) + 1] for r in out_roles]
        count = None
        if c.res in ("Navier_Stokes", "physics_equation"):
            f = R2.formula(c.res, c.corrected, c.nu, ins, outs)
        else:
            fc = O.continuity_fields(*ins, *outs)
            on = (ins[0] < THRESHOLD) if c.res == "continuity_only" else torch.zeros_like(fc, dtype=torch.bool)
            f = (fc, torch.where(on, outs[0] - ANCHOR, torch.zeros_like(fc)))
            count = on[:c.n_res].sum().to(dtype).reshape(1)
        F_ = torch.cat(f, 1).t()[:, :c.n_res]                            # split: the collocation points come first
        sq = F_ ** 2 if weights is None else weights.to(dtype) * F_ ** 2  # (per-point weights: one row for all terms, or a row per term)
        sums = sq.sum(1)[:N_TERMS[c.res]] if c.res != "continuity_only" else torch.cat([sq.sum(1), count])
        scale = c.term_scale()
        n_grad = len(scale) - (1 if c.res == "continuity_only" else 0)   # continuity_only's third term is a count
        obj = sum(scale[t] * sums[t] for t in range(n_grad))
    csum = torch.zeros(0, dtype=dtype)
    if c.kind != "residual":
        rows = slice(c.n_res, c.N) if c.kind == "split" else slice(0, c.N)
        Tt = T.to(dtype)
        csum = torch.stack([((Y[rows, col] - Tt[:, j]) ** 2).sum() for j, col in enumerate(c.fid_cols)])
        obj = obj + sum(w * s for w, s in zip(c.col_scale(), csum))
    return obj, sums, csum, F_


def evaluate(c, params, X, T, dtype, mis=None, **kw):
    """The loss / fields / second request of case `c` at `params` on X (targets T) by torch autograd in `dtype`:
    SimpleNamespace(sums, cols, fields, grad), float64.  kw: objective's per-point weights and dropout masks."""
    q = [t.detach().to(dtype).requires_grad_(True) for t in params]
    obj, sums, csum, F_ = objective(c, q, X.detach().to(dtype), T, mis, **kw)
    grad = O.flat_grad(obj, q)
    cpu64 = lambda t: t.detach().double().cpu()
    return SimpleNamespace(sums=cpu64(sums), cols=cpu64(csum), fields=cpu64(F_), grad=cpu64(grad))


def evaluate_explicit(c, params, X, dtype, mis):
    """continuity_ftemp's residual request on explicit jets (fc = h_x U + h U_x + h_y V + h V_y): where the two jet-level
    mis-readings reach a loss request.  mis = None equals evaluate()."""
    assert c.res == "continuity_ftemp" and c.kind == "residual"
    q = [t.detach().to(dtype).requires_grad_(True) for t in params]
    Y, dY = explicit_jets(q, X.to(dtype), c.gc, mis)
    ix, iy = (list(c.gc).index(c.inn.index(r)) for r in ("x", "y"))
    h, U, V = (c.outn.index(r) for r in ("h", "U", "V"))
    fc = dY[ix][:, h] * Y[:, U] + Y[:, h] * dY[ix][:, U] + dY[iy][:, h] * Y[:, V] + Y[:, h] * dY[iy][:, V]
    sums = (fc ** 2).sum().reshape(1)
    grad = O.flat_grad(c.term_scale()[0] * sums[0], q)
    return SimpleNamespace(sums=sums.detach().double(), cols=torch.zeros(0, dtype=torch.float64), fields=fc.detach().double()[None],
                           grad=grad.detach().double())


def evaluate_jets(c, params, X, dtype, second=False, mis=None):
    """(Y, dY[, d2Y]) by nested autograd in `dtype` (trained_state_util.jets with the LeakyReLU network), detached float64."""
    q, cols = _leaf(params, X, dtype)
    Y = net(q, torch.cat(cols, -1), mis)
    d = R2._d
    dY = [torch.cat([d(Y[:, o:o + 1], cols[j]) for o in range(c.d_out)], 1) for j in c.gc]
    out = [Y, torch.stack(dY) if dY else Y.new_zeros(0, *Y.shape)]
    if second:
        out.append(torch.stack([torch.cat([d(dY[i][:, o:o + 1], cols[c.gc[j]]) for o in range(c.d_out)], 1)
                                for i in range(c.k) for j in range(i, c.k)]))
    return [t.detach().double() for t in out]


def evaluate_adj(c, params, X, gY, gdY, dtype, mis=None):
    """Flat gradient of sum(gY Y) + sum(gdY dY) in `dtype`; the mode's absent adjoint is zero.  The two jet-level mis-readings
    go through explicit_jets, everything else through autograd."""
    gY = torch.zeros_like(gY) if c.mode == "gdY" else gY
    gdY = torch.zeros_like(gdY) if c.mode == "gY" else gdY
    if mis is not None and mis[0] in ("tangent", "reverse"):
        q = [t.detach().to(dtype).requires_grad_(True) for t in params]
        Y, dY = explicit_jets(q, X.to(dtype), c.gc, mis)
    else:
        q, cols = _leaf(params, X, dtype)
        Y = net(q, torch.cat(cols, -1), mis)
        dY = torch.stack([torch.cat([R2._d(Y[:, o:o + 1], cols[j]) for o in range(c.d_out)], 1) for j in c.gc]) if c.gc else Y.new_zeros(0, *Y.shape)
    obj = (gY.to(dtype) * Y).sum() + ((gdY.to(dtype) * dY).sum() if c.k else 0.0)
    return SimpleNamespace(grad=O.flat_grad(obj, q).detach().double())


def _with_noise(c, d, r64, r32):
    cn = replace(c, N=NOISE_POINTS, kind="residual")
    n64, n32 = (evaluate(cn, d.params, d.Xn, None, t).fields for t in (torch.float64, torch.float32))
    r64.noise = torch.maximum((r32.fields - r64.fields).abs().amax(1), (n32 - n64).abs().amax(1))
    r64.fmax = torch.maximum(r64.fields.abs().amax(1), n64.abs().amax(1))
    r64.rms = (r64.fields ** 2).mean(1).sqrt()


def reference_of(d):
    """(fp64 result, fp32 result) of the data `d` (data() or named())."""
    c = d.case
    if c.family == "adj":
        return tuple(evaluate_adj(c, d.params, d.X, d.gY, d.gdY, t) for t in (torch.float64, torch.float32))
    if c.family == "fwd":
        return tuple(SimpleNamespace(jets=evaluate_jets(c, d.params, d.X, t)) for t in (torch.float64, torch.float32))
    r64, r32 = (evaluate(c, d.params, d.X, d.T, t) for t in (torch.float64, torch.float32))
    if c.res is not None and (c.family in ("fields", "second") or c.n_res < SMALL_SET):
        _with_noise(c, d, r64, r32)
    if c.family == "second":
        r64.jets, r32.jets = (evaluate_jets(c, d.params, d.X, t, second=True) for t in (torch.float64, torch.float32))
    return r64, r32


@functools.lru_cache(maxsize=None)
def reference(family, seed):
    """(fp64 result, fp32 result) of the seeded case, computed once and shared (callers leave it unchanged)."""
    return reference_of(data(family, seed))


@functools.lru_cache(maxsize=None)
def named_reference(name, L, W, k, family="loss"):
    return reference_of(named(name, L, W, k, family))


def mutants(d):
    """{mis-reading: fp64 result} of the mis-readings that apply to the data `d`: the slope-table ones to every case, the two
    jet-level ones where the request is written on explicit jets (adj, fwd, continuity_ftemp's residual request), "one at
    zero" to the origin case."""
    c = d.case
    out = {}
    kinds = [("relu", None), ("tanh", mis_layer(c)), ("neighbour", mis_layer(c)), ("tenth", mis_layer(c))]
    if c.name == "origin":
        kinds.append(("one at zero", None))
    # (the tangent a request certainly uses: x's for a residual, the last one where the caller's adjoints weigh them all)
    j_used = list(c.gc).index(c.inn.index("x")) if c.res else c.k - 1
    jet_level = [("tangent", mis_layer(c), j_used), ("reverse", mis_layer(c))]
    for mis in kinds:
        if c.family == "adj":
            out[mis[0]] = evaluate_adj(c, d.params, d.X, d.gY, d.gdY, torch.float64, mis)
        elif c.family == "fwd":
            out[mis[0]] = SimpleNamespace(jets=evaluate_jets(c, d.params, d.X, torch.float64, mis=mis))
        else:
            out[mis[0]] = evaluate(c, d.params, d.X, d.T, torch.float64, mis)
            if c.family == "second":
                out[mis[0]].jets = evaluate_jets(c, d.params, d.X, torch.float64, second=True, mis=mis)
    for mis in jet_level:
        if c.family == "adj" and (c.k and c.mode != "gY" or mis[0] == "reverse"):
            out[mis[0]] = evaluate_adj(c, d.params, d.X, d.gY, d.gdY, torch.float64, mis)
        elif c.family == "fwd" and mis[0] == "tangent" and c.k:
            q = [t.double() for t in d.params]
            Y, dY = explicit_jets(q, d.X.double(), c.gc, mis)
            out[mis[0]] = SimpleNamespace(jets=[Y.detach(), dY.detach()])
        elif c.family in ("loss", "adam") and c.res == "continuity_ftemp" and c.kind == "residual":
            out[mis[0]] = evaluate_explicit(c, d.params, d.X, torch.float64, mis)
    return out


def small_set_noise(c, r64):
    """sweep2_util.small_set_noise: for fewer than SMALL_SET residual points the largest nu_t / rms_t over the live terms."""
    if c.res is None or c.n_res >= SMALL_SET or not hasattr(r64, "noise"):
        return 0.0
    return max((n / r if r > 0 else 0.0) for n, r in zip(r64.noise.tolist(), r64.rms.tolist()))


field_ratios, FIELD_BOUND, sum_ratio = S.field_ratios, S.FIELD_BOUND, S.sum_ratio
JET_FLOOR = 2e-6         # Y / dY / d2Y within JET_FLOOR x max(1, max |ref|) (trained_state_util.abs_bound)


def jet_ratio(got, ref64):
    """Largest |got - ref| / (JET_FLOOR max(1, max |ref|)) over the jets given (1.0 = at the bound)."""
    worst = 0.0
    for g_, r in zip(got, ref64):
        if r.numel():
            worst = max(worst, float((torch.as_tensor(g_).detach().double().cpu() - r).abs().max()) / (JET_FLOOR * max(1.0, float(r.abs().max()))))
    return worst


# ---- census ----------------------------------------------------------------------------------------------------------------
BUCKETS = ([f"width {w} K1={k1}" for w in (16, 32, 64) for k1 in (3, 4)] +
           ["K1 = 1", "gradient copy in LDS", "gradient copy in global memory", "cooperative range", "width 64 beyond the cooperative range",
            "narrow, N >= 4097", "width > 64", "L = 1", "L = 40", "N < 16", "N = 1 mod 16", "no role in output column 0"])


def census(families=("loss", "adam", "adj")):
    """{bucket: number of cases} over the committed seeds of the gradient families."""
    cnt = {b: 0 for b in BUCKETS}
    for f in families:
        for s in SEEDS[f]:
            c = draw(f, s)
            hits = ["L = 1"] * (c.L == 1) + ["L = 40"] * (c.L == 40) + ["N < 16"] * (c.N < 16) + ["N = 1 mod 16"] * (c.N % 16 == 1)
            hits += ["no role in output column 0"] * c.col0_is_no_role
            if c.W > 64:
                hits.append("width > 64")
            else:
                hits += [f"width {c.wp} K1={c.K1}"] * (c.K1 in (3, 4)) + ["K1 = 1"] * (c.K1 == 1)
                hits.append("gradient copy in LDS" if c.in_lds else "gradient copy in global memory")
                if c.wp == 64 and f != "adj":
                    hits.append("cooperative range" if coop_fits(c.L, c.W, c.K1) and (c.N + 15) // 16 <= CUS else "width 64 beyond the cooperative range")
                hits += ["narrow, N >= 4097"] * (c.wp <= 32 and c.N >= 4097)
            for h in hits:
                cnt[h] += 1
    return cnt
