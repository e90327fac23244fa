"""Shared by test_sweep2_cpu.py / test_sweep2_gpu.py: the seeded draws of the second sweep and their fp64 reference.

tests/test_sweep_gpu.py draws random shapes for the request kinds of round 3 and compares whole gradient vectors with
the generic engine from zero hidden biases.  This sweep takes the request kinds added since (FAMILIES) through the same
kind of draw (shuffled and extra columns, an extra differentiated input, depth 1..40, width 3..64, 1..9600 points), with
non-zero hidden biases (trained_state_util.trained_like), and holds every result to a formula evaluated with torch
autograd on the CPU in float64 (never the code under test): term sums, column sums, per-point fields, and the gradient
block by block (trained_state_util.assert_blocks_close).

  pec     physics_equation with the corrected radiation stress: loss + gradient, residual / one-pass / split requests
  fields  residual_fields of the four residuals and the corrected one
  res2    residual2_loss_grad (lateral mixing nu lap(U)) with fields
  ens     ensemble_loss_grad: M members, shared or per-member point sets and targets
  adj     jet_backward forced onto the batch kernel

served(family, case, engine) restates what include/pinn_hip.h documents as served; the GPU module fails on a refusal
where it says yes and on a success where it says no.

Bounds (the project's existing rules, see field_ratios / sum_ratio / assert_blocks_close):
  fields    per field max_n |f - f64| <= 4 max(max_n |f32 - f64|, 2^-23 max_n |f64|)      (test_fields_gpu.py)
  sums      relative error <= max(2e-6, 4 |s32 - s64| / |s64|); an fp64 zero must be exactly 0   (loss_bound)
  gradient  every W_l / b_l block within max(2e-5, 4 gap), gap <= GAP_CAP                    (assert_blocks_close)
"""
import functools
import random
from dataclasses import dataclass, replace
from types import SimpleNamespace
from typing import Optional, Tuple

import torch

from oracle import pinn_oracle as O
from tests import residual2_util as R2
from tests.trained_state_util import jet_adjoint_grad, loss_bound, trained_like

FAMILIES = ("pec", "fields", "res2", "ens", "adj")
# The committed seeds of each family: 35 to 37 of a range started where test_sweep2_cpu.py's census holds, without the seeds that
# break one of its conditions on the reference alone (SKIPPED).  What was cut, seed by seed:
#   small set on a cancellation   every seed below that carries no other note: fewer than 16 residual points with
#                                 small_set_noise > SMALL_SET_NOISE.  This condition is this sweep's own (the issue lists finite
#                                 sums, live blocks and the block gap); it removes about two thirds of the N < 16 draws of these
#                                 ranges (7 of pec's 11), some as close as 1.2e-6 to the threshold; the census keeps >= 3 each.
#   block gap                     ens 172 (N = 1, a block whose fp32 run is 100 % off its fp64 run)
#   power                         ens 150 (continuity_only on 40 x 24, one-pass): swapping two output roles moves one member's
#                                 gradient by 1.7e-5 only, below the 2e-5 floor
#   near its bound                pec 60 (16 points at nu / rms = 6e-6): passed, its third term sum at 0.99 of a bound that is the
#                                 reference's own |s32 - s64|, which moves with the CPU the reference runs on
SKIPPED = {
    "pec": [28, 31, 39, 40, 52, 53, 56, 58, 59, 60, 62],
    "fields": [159, 162, 163, 164, 166, 171, 174, 181],
    "res2": [9, 12, 32, 34],
    "ens": [137, 144, 150, 152, 157, 160, 165, 170, 172, 177, 178],
    "adj": [],
}
_RANGES = {"pec": range(23, 69), "fields": range(150, 194), "res2": range(3, 43), "ens": range(132, 180), "adj": range(1, 37)}
SEEDS = {f: [s for s in _RANGES[f] if s not in SKIPPED[f]] for f in _RANGES}
GAP_MARGIN = 4e-6        # the committed seeds keep every block's gap below this (GAP_CAP = 5e-6 is what assert_blocks_close enforces)
SMALL_SET_NOISE = 1e-6   # see small_set_noise
SMALL_SET = 16           # residual points below which a request counts as a small set (one 16-point tile)

# residual name -> (output roles, direction roles)            (engine.RESIDUAL_ROLES, restated: this file imports no library)
ROLES = {
    "Navier_Stokes": (("h", "z", "u", "v"), ("t", "x", "y")),
    "physics_equation": (("h", "U", "V", "eta_mean", "Hrms", "k"), ("x", "y")),
    "continuity_ftemp": (("h", "U", "V"), ("x", "y")),
    "continuity_only": (("h", "U", "V"), ("x", "y")),
}
N_TERMS = {"Navier_Stokes": 3, "physics_equation": 3, "continuity_ftemp": 1, "continuity_only": 3}
N_FIELDS = {"Navier_Stokes": 3, "physics_equation": 3, "continuity_ftemp": 2, "continuity_only": 2}
# what each family draws its residual from ("+c": the corrected radiation stress)
RESIDUALS = {
    "pec": ["physics_equation+c", "physics_equation+c", "physics_equation+c", "physics_equation"],
    "fields": ["Navier_Stokes", "Navier_Stokes", "physics_equation", "physics_equation+c", "continuity_ftemp", "continuity_only"],
    "res2": ["Navier_Stokes", "Navier_Stokes", "physics_equation", "physics_equation+c"],
    # (the corrected stress has no ensemble kernel: a rare draw that must be refused)
    "ens": ["Navier_Stokes", "physics_equation", "continuity_ftemp", "continuity_only"] * 3 + ["physics_equation+c"],
}
DEPTHS = [1, 2, 3, 4, 6, 8, 12]
WIDTHS = [3, 7, 10, 12, 16, 17, 20, 24, 28, 32, 33, 40, 48, 57, 64]
POINTS = [1, 15, 16, 17, 37, 65, 243, 700, 4097]
ADJ_POINTS = [1, 15, 17, 65, 243, 700, 4101, 4101]      # (the large count twice: one draw in four)
MEMBERS = [1, 2, 3, 5, 16]
THRESHOLD, ANCHOR = 25.5, 0.75          # continuity_only (physics.py:26-27)
NOISE_POINTS = 256


def padded_width(W):
    return 16 if W <= 16 else 32 if W <= 32 else 64


@dataclass(frozen=True)
class Case:
    family: str
    seed: int
    res: Optional[str]                  # None for adj
    corrected: bool
    nu: float
    inn: Tuple[str, ...]
    outn: Tuple[str, ...]
    gc: Tuple[int, ...]
    L: int
    W: int
    N: int
    kind: str = "residual"              # residual / onepass / split
    M: int = 1                          # ens
    own_x: bool = False
    own_t: bool = False
    mode: str = "both"                  # adj: gY / gdY / both

    @property
    def d_in(self): return len(self.inn)

    @property
    def d_out(self): return len(self.outn)

    @property
    def k(self): return len(self.gc)

    @property
    def wp(self): return padded_width(self.W)

    @property
    def layers(self): return O.layer_sizes(self.d_in, self.L, self.W, self.d_out)

    @property
    def n_fid(self): return {"residual": 0, "onepass": self.N, "split": max(1, self.N // 5)}[self.kind]

    @property
    def n_res(self): return self.N - self.n_fid if self.kind == "split" else self.N

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

    def term_scale(self):
        return [s / max(self.n_res, 1) for s in [1.0, 0.5, 2.0, 1.5][:N_TERMS[self.res]]]

    def col_scale(self):
        return [0.7 / max(self.n_fid, 1)] * len(self.fid_cols)

    def tag(self):
        what = "" if self.res is None else self.res + ("+c" if self.corrected else "") + (f" nu={self.nu}" if self.nu else "") + " "
        ens = f" M={self.M}{' ownX' if self.own_x else ''}{' ownT' if self.own_t else ''}" if self.family == "ens" else ""
        return (f"{self.family} seed {self.seed}: {what}{self.d_in}->{self.L}x{self.W}->{self.d_out} k={self.k} N={self.N} "
                f"{self.mode if self.family == 'adj' else self.kind}{ens}")


def draw(family, seed):
    """The case of (family, seed), from random.Random alone."""
    r = random.Random(f"{family}/{seed}")
    if family == "adj":                 # a network with no residual attached, inside the batch kernel's grid
        d_in, d_out = r.choice([2, 3, 3, 4, 5, 8]), r.choice([1, 2, 3, 4, 6, 9, 16])
        k = r.choice([2, 3]) if d_in >= 3 else 2
        gc = tuple(sorted(r.sample(range(d_in), k)))
        L = r.choice(DEPTHS) if r.random() > 0.15 else 40
        W = r.choice([w for w in WIDTHS if w <= 32])
        if L == 40: W = min(W, 24)
        return Case(family, seed, None, False, 0.0, tuple(f"in{i}" for i in range(d_in)), tuple(f"out{i}" for i in range(d_out)),
                    gc, L, W, r.choice(ADJ_POINTS), mode=r.choice(["gY", "gdY", "both", "both"]))
    res = r.choice(RESIDUALS[family])
    res, corrected = res.replace("+c", ""), res.endswith("+c")
    out_roles, dir_roles = ROLES[res]
    # (physics_equation has six roles: the pec family draws extra columns more often, or no role-free column 0 comes up)
    inn = list(dir_roles) + [f"in{i}" for i in range(r.choice([0, 1, 1, 2] if family == "pec" else [0, 0, 1, 2]))]
    outn = list(out_roles) + [f"out{i}" for i in range(r.choice([0, 1, 3, 3] if family == "pec" else [0, 0, 1, 3]))]
    r.shuffle(inn); r.shuffle(outn)
    gc = sorted(inn.index(d) for d in dir_roles)
    extra = [i for i in range(len(inn)) if i not in gc]
    # an extra differentiated input: where the family's entries take k != the residual's directions (the loss entries of the
    # plain residuals and the ensembles; the corrected stress, fields and residual2 are k = directions only)
    may_extra = family in ("pec", "ens") and not corrected
    if may_extra and extra and len(gc) < 3 and r.random() < (0.9 if family == "pec" else 0.6):
        gc = sorted(gc + [r.choice(extra)])
    L = r.choice(DEPTHS) if r.random() > 0.06 else 40
    W = r.choice(WIDTHS)
    N = r.choice(POINTS) if r.random() > 0.06 else 9600
    if L == 40: W, N = min(W, 24), min(N, 4097)
    nu = r.choice([0.05, 1.0]) if family == "res2" else 0.0
    kind = r.choice(["residual", "onepass", "split"]) if family in ("pec", "ens") else "residual"
    M, own_x, own_t = 1, False, False
    if family == "ens":
        M = r.choice(MEMBERS)
        own_x, own_t = r.random() < 0.5, r.random() < 0.5
        N = min(N, 4097)
        if M == 16 and r.random() < 0.4: N = 4097        # 16 members x 65 workgroups: above the tile kernel's cap, a clamped grid
        if M * N > 12000: L = min(L, 3)                   # (the references of all members run on the CPU)
    c = Case(family, seed, res, corrected, nu, tuple(inn), tuple(outn), tuple(gc), L, W, N, kind, M, own_x, own_t)
    if c.kind == "split" and c.n_res == 0:
        c = replace(c, kind="residual")
    if c.kind == "residual":
        c = replace(c, own_t=False)
    return c


# ---- what the header documents as served --------------------------------------------------------------------------------
def served(family, c, engine):
    """Whether include/pinn_hip.h says the call of this family on case `c` is served under `engine` ("auto", "generic",
    "tile", "batch", "fused").  Every case here is fp32, tanh, no dropout, width <= 64, d_in and d_out <= 16."""
    n_dirs = len(ROLES[c.res][1]) if c.res else None
    fused_shape = c.W <= 64 and c.d_in <= 16 and c.d_out <= 16 and c.k in (2, 3)
    if family == "pec":
        # pinn_residual_loss: GENERIC any shape, k = 2 or 3.  The corrected request "runs on the engine the descriptor selects,
        # or is refused ... never moved to another engine": AUTO and every FUSED value at width <= 64 are the fused engine,
        # which has the corrected residual for k = 2 only; FUSED_BATCH "falls back to _TILE" where it has no kernel.
        if engine == "generic":
            return c.k in (2, 3)
        return fused_shape and (not c.corrected or c.k == 2)
    if family == "fields":
        # pinn_residual_fields: desc->k must equal the residual's directions; FUSED: width <= 64, d_in and d_out <= 16;
        # corrected: k = 2, tanh; GENERIC staged; AUTO the MFMA path where FUSED serves, else staged
        if c.k != n_dirs:
            return False
        return True if engine in ("auto", "generic") else fused_shape
    if family == "res2":
        # pinn_residual2_loss_grad: k == the residual's directions; FUSED: every layer at most 64 wide
        if c.k != n_dirs:
            return False
        return True if engine in ("auto", "generic") else max(c.layers) <= 64
    if family == "ens":
        # ensembles: AUTO / FUSED / FUSED_TILE, k = 2 or 3; refused: the corrected stress, the split request at width 33..64,
        # GENERIC, FUSED_BATCH
        if engine not in ("auto", "fused", "tile"):
            return False
        return fused_shape and not c.corrected and not (c.kind == "split" and c.wp == 64)
    assert family == "adj"
    # pinn_jet_backward: FUSED (every sub-value) width <= 64, d_in and d_out <= 16, k in {0, 2, 3} or no gdY
    return c.W <= 64 and c.d_in <= 16 and c.d_out <= 16 and (c.k in (0, 2, 3) or c.mode == "gY")


def adj_runs_on_batch(c):
    """pinn_jet_backward under FUSED_BATCH: "the batch kernel serves ... tanh, width <= 32, d_in <= 8, k in {2, 3} with gdY",
    every other served request runs on the tile kernel."""
    return c.W <= 32 and c.d_in <= 8 and c.k in (2, 3) and c.mode != "gY"


def engines(family, c):
    """The engines the GPU module runs the case on."""
    if family == "pec":       # FUSED_BATCH forced where the batch kernel has the corrected instance (width <= 32, k = 2)
        return ["auto", "tile"] + (["batch"] if c.W <= 32 and c.k == 2 else []) + ["generic"]
    if family == "fields":
        return ["tile", "generic", "auto"]
    if family == "res2":
        return ["generic", "fused", "auto"]
    return ["auto"] if family == "ens" else ["batch"]


# ---- data ----------------------------------------------------------------------------------------------------------------
def _params(c, g):
    p = trained_like(c.layers, g, residual=c.res, outn=c.outn)       # biased state; physics_equation: its conditioning
    b = p[-1].clone()
    if c.res == "physics_equation":
        b[c.outn.index("Hrms")] = 0.5                                # the corrected stress E ~ Hrms^2 carries weight
    if c.res == "Navier_Stokes":
        b[c.outn.index("h")], b[c.outn.index("z")] = 2.0, 0.2        # residual2_util.conditioned_params' output bias
    p[-1] = b
    return p


@functools.lru_cache(maxsize=None)
def data(family, seed):
    """The case with its parameters (one list per member), points, targets and adjoints: all float32 on the CPU, computed
    once and shared (callers leave them unchanged)."""
    c = draw(family, seed)
    g = torch.Generator().manual_seed(7000 + 97 * FAMILIES.index(family) + seed)
    members = [_params(c, g) for _ in range(c.M)]
    X = torch.rand((c.M, c.N, c.d_in) if c.own_x else (c.N, c.d_in), generator=g) * 2 - 1
    if c.res == "continuity_only":
        X[..., c.inn.index("x")] *= 40                               # x < 25.5 selects a real subset
    T = None
    if c.kind != "residual":
        T = torch.rand((c.M, c.n_fid, len(c.fid_cols)) if c.own_t else (c.n_fid, len(c.fid_cols)), generator=g)
    # NOISE_POINTS more points of the same distribution: the field bound's noise level is the NETWORK's, taken over them and the
    # case's own points together, as test_fields_gpu.check_against_oracle holds a prefix of 1 or 15 points to the noise of all
    # 777 "rather than to the luck of its own one or fifteen fp32 roundings"
    Xn = torch.rand(NOISE_POINTS, c.d_in, generator=g) * 2 - 1
    if c.res == "continuity_only":
        Xn[:, c.inn.index("x")] *= 40
    gY = gdY = None
    if family == "adj":
        gY, gdY = torch.randn(c.N, c.d_out, generator=g), torch.randn(c.k, c.N, c.d_out, generator=g)
    return SimpleNamespace(case=c, members=members, X=X.contiguous(), T=T, gY=gY, gdY=gdY, Xn=Xn)


def member_X(d, m): return d.X[m] if d.case.own_x else d.X


def member_T(d, m): return d.T[m] if (d.T is not None and d.case.own_t) else d.T


# ---- the reference -------------------------------------------------------------------------------------------------------
def evaluate(c, params, X, T, dtype, inn=None, outn=None, corrected=None, nu=None, swap_scale=False, fid_front=False,
             device="cpu"):
    """The request of case `c` at `params` on points X (targets T) by torch autograd in `dtype`: SimpleNamespace(sums
    (n_terms), cols (n_cols), fields (n_fields, n_res), grad (P)), all float64 on the CPU.  The keyword arguments re-read the
    request the way a wrong kernel might (test_sweep2_cpu.py's mutants): other column names, the flag or nu ignored, two
    term scales exchanged, the fidelity rows of a split request taken from the front."""
    inn, outn = list(c.inn if inn is None else inn), list(c.outn if outn is None else outn)
    corrected, nu = c.corrected if corrected is None else corrected, c.nu if nu is None else nu
    q = [t.detach().to(dtype).to(device).requires_grad_(True) for t in params]
    cols = [X[:, i:i + 1].detach().to(dtype).to(device).requires_grad_(True) for i in range(X.shape[1])]
    Y = O.mlp_forward(q, torch.cat(cols, -1))
    out_roles, dir_roles = ROLES[c.res]
    ins = [cols[inn.index(r)] for r in dir_roles]
    outs = [Y[:, outn.index(r):outn.index(r) + 1] for r in out_roles]
    count = None
    if c.res in ("Navier_Stokes", "physics_equation"):
        f = R2.formula(c.res, corrected, nu, ins, outs)
    else:
        fc = O.continuity_fields(*ins, *outs)
        on = (ins[0] < THRESHOLD) if c.res == "continuity_only" else torch.zeros_like(fc, dtype=torch.bool)
        f = (fc, torch.where(on, outs[0] - ANCHOR, torch.zeros_like(fc)))
        count = on[:c.n_res].sum().to(dtype).reshape(1)
    F = torch.cat(f, 1).t()[:, :c.n_res]                             # split: the collocation points come first
    sums = (F ** 2).sum(1)[:N_TERMS[c.res]] if c.res != "continuity_only" else torch.cat([(F ** 2).sum(1), count])
    scale = c.term_scale()
    if swap_scale and len(scale) >= 3:
        scale[1], scale[2] = scale[2], scale[1]
    n_grad = len(scale) - (1 if c.res == "continuity_only" else 0)   # continuity_only's third term is a count
    obj = sum(scale[t] * sums[t] for t in range(n_grad))
    csum = torch.zeros(0, dtype=dtype)
    if c.kind != "residual":
        rows = slice(0, c.N) if c.kind == "onepass" else (slice(0, c.n_fid) if fid_front else slice(c.n_res, c.N))
        Tt = T.to(dtype).to(device)
        csum = torch.stack([((Y[rows, col] - Tt[:, j]) ** 2).sum() for j, col in enumerate(c.fid_cols)])
        obj = obj + sum(w * s for w, s in zip(c.col_scale(), csum))
    grad = O.flat_grad(obj, q)
    cpu64 = lambda t: t.detach().double().cpu()
    return SimpleNamespace(sums=cpu64(sums), cols=cpu64(csum), fields=cpu64(F), grad=cpu64(grad))


def evaluate_adj(c, params, X, gY, gdY, dtype, gc=None):
    """Flat gradient of sum(gY Y) + sum(gdY dY) by torch autograd in `dtype` (trained_state_util.jet_adjoint_grad); the
    mode's absent adjoint is zero."""
    gY = torch.zeros_like(gY) if c.mode == "gdY" else gY
    gdY = torch.zeros_like(gdY) if c.mode == "gY" else gdY
    return SimpleNamespace(grad=jet_adjoint_grad(params, X, list(c.gc if gc is None else gc), gY, gdY, dtype))


@functools.lru_cache(maxsize=None)
def reference(family, seed):
    """[(fp64 result, fp32 result) per member] of the case, computed once and shared (callers leave it unchanged)."""
    d = data(family, seed)
    c = d.case
    if family == "adj":
        return [tuple(evaluate_adj(c, d.members[0], d.X, d.gY, d.gdY, t) for t in (torch.float64, torch.float32))]
    out = []
    for m in range(c.M):
        r64, r32 = (evaluate(c, d.members[m], member_X(d, m), member_T(d, m), t) for t in (torch.float64, torch.float32))
        # the network's noise level per field (data()): for the families whose fields are checked, and for small_set_noise
        if family in ("fields", "res2") or c.n_res < SMALL_SET:
            cn = replace(c, N=NOISE_POINTS, kind="residual")
            n64, n32 = (evaluate(cn, d.members[m], d.Xn, None, t).fields for t in (torch.float64, torch.float32))
            r64.noise = torch.maximum((r32.fields - r64.fields).abs().amax(1), (n32 - n64).abs().amax(1))
            r64.fmax = torch.maximum(r64.fields.abs().amax(1), n64.abs().amax(1))
            r64.rms = (r64.fields ** 2).mean(1).sqrt()
        out.append((r64, r32))
    return out


# ---- the mis-readings a wrong kernel might make (evaluated through the fp64 reference) -----------------------------------
def _swapped(names, a, b):
    names = list(names)
    i, j = names.index(a), names.index(b)
    names[i], names[j] = names[j], names[i]
    return names


def mutants(family, seed):
    """{name: [fp64 result per member]} of the mis-readings (a)-(g) that apply to the case."""
    d = data(family, seed)
    c = d.case
    out = {}
    if family == "adj":
        gc = list(c.gc); gc[-1], gc[-2] = gc[-2], gc[-1]
        if c.mode != "gY":
            out["b: direction columns swapped"] = [evaluate_adj(c, d.members[0], d.X, d.gY, d.gdY, torch.float64, gc=gc)]
        return out
    out_roles, dir_roles = ROLES[c.res]

    def run(member_shift=0, shift_x=False, shift_t=False, **kw):
        res = []
        for m in range(c.M):
            mx = (m + 1) % c.M if shift_x else m
            mt = (m + 1) % c.M if shift_t else m
            res.append(evaluate(c, d.members[m], member_X(d, mx), member_T(d, mt), torch.float64, **kw))
        return res

    has_grad = family != "fields"
    out["a: output roles swapped"] = run(outn=_swapped(c.outn, out_roles[1], out_roles[2]))
    out["b: direction columns swapped"] = run(inn=_swapped(c.inn, dir_roles[-1], dir_roles[-2]))
    if c.corrected:
        out["c: corrected ignored"] = run(corrected=False)
    if c.nu:
        out["d: nu ignored"] = run(nu=0.0)
    if has_grad and N_TERMS[c.res] >= 3:
        out["e: term scales exchanged"] = run(swap_scale=True)
    if has_grad and c.kind == "split":
        out["f: fidelity rows from the front"] = run(fid_front=True)
    if family == "ens" and c.M > 1:
        if c.own_x:
            out["g: next member's points"] = run(shift_x=True)
        if c.own_t and c.kind != "residual":
            out["g: next member's targets"] = run(shift_t=True)
    return out


def small_set_noise(c, r64):
    """For a request with fewer than SMALL_SET residual points: the largest nu_t / rms_t over the live terms, nu_t the network's fp32
    noise level of field t (max |f32 - f64| over the case's points and the NOISE_POINTS) and rms_t the field's root mean square
    on the case's points; 0 for larger point sets.  The relative error of sum f^2 under an absolute field error nu is 2 nu / f:
    with one or fifteen points |s32 - s64| is one or fifteen roundings, no noise estimate, so the sum bound falls to its 2e-6
    floor, and a kernel as good as the reference meets that floor only where nu / rms <= 1e-6.  A point set on a cancellation
    (a residual of 1e-3 between terms of order 1) is a badly chosen case, not a finding."""
    if c.n_res >= SMALL_SET:
        return 0.0
    return max((n / r if r > 0 else 0.0) for n, r in zip(r64.noise.tolist(), r64.rms.tolist()))


# ---- bounds --------------------------------------------------------------------------------------------------------------
def field_ratios(got, r64):
    """Per field: max_n |got - f64| / max(noise, 2^-23 max |f64|), noise = max |f32 - f64| of the reference, both maxima over
    the case's points and the NOISE_POINTS of data(); test_fields_gpu.check_against_oracle's bound is ratio <= 4.  A field whose
    reference is exactly zero (both dtypes) gives 0 where got is exactly zero, else inf."""
    got = torch.as_tensor(got).detach().double().cpu()
    err = (got - r64.fields).abs().amax(1)
    den = torch.maximum(r64.noise, 2.0 ** -23 * r64.fmax)
    return [float(e / d_) if d_ > 0 else (0.0 if e == 0 else float("inf")) for e, d_ in zip(err.tolist(), den.tolist())]


FIELD_BOUND = 4.0


def sum_ratio(got, s64, s32):
    """Largest (relative error of a sum) / loss_bound over the entries; an fp64 zero must be met exactly (else inf)."""
    worst = 0.0
    for g, a, b in zip(torch.as_tensor(got).detach().double().cpu().reshape(-1).tolist(), s64.tolist(), s32.tolist()):
        if a == 0.0:
            worst = max(worst, 0.0 if g == 0.0 else float("inf"))
        else:
            worst = max(worst, abs(g - a) / abs(a) / loss_bound(a, b))
    return worst


# ---- census: what the committed seed range of a family must contain ------------------------------------------------------
def buckets(family):
    """The buckets the family's draw can reach.  Padded width x k: pec holds k = 2 only (the corrected stress is k = 2; its
    plain quarter reaches k = 3 through the extra differentiated input, counted in its own bucket); adj has no width 64."""
    widths = (16, 32) if family == "adj" else (16, 32, 64)
    ks = (2,) if family == "pec" else (2, 3)
    out = [f"width {w} k={k}" for w in widths for k in ks] + ["N < 16", "N = 1 mod 16", "N >= 4097", "L = 1"]
    if family != "adj":
        out += ["no role in output column 0", "d_out above the io1 epilogue's"]
    if family in ("pec", "ens"):
        out += ["extra differentiated input"]
    return out


def census(family, seeds=None):
    """{bucket: number of cases} over the family's committed seeds."""
    cnt = {b: 0 for b in buckets(family)}
    for s in SEEDS[family] if seeds is None else seeds:
        c = draw(family, s)
        hits = [f"width {c.wp} k={c.k}"]
        hits += ["N < 16"] * (c.N < 16) + ["N = 1 mod 16"] * (c.N % 16 == 1) + ["N >= 4097"] * (c.N >= 4097) + ["L = 1"] * (c.L == 1)
        if c.res:
            hits += ["no role in output column 0"] * c.col0_is_no_role + ["extra differentiated input"] * c.extra_dir
            hits += ["d_out above the io1 epilogue's"] * (c.d_out > (8 if c.res == "physics_equation" else 4))
        for h in hits:
            if h in cnt:
                cnt[h] += 1
    return cnt
