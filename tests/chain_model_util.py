"""Shared by test_chain_model_cpu.py / test_chain_model_gpu.py: an fp64 MODEL of what bf16 mode of the wide engine computes
for one request, rounding exactly where the kernels round; fp32 EMULATIONS of a correct kernel (the same computation in fp32
with other summation orders), whose distance from the model is a case's NOISE; the bound rule; the mutants; the cases.

The model is hand-written: with rounding in it the reverse sweep is a prescribed computation, not a derivative, so autograd
cannot produce it.  With every rounding switched off it IS the derivative (test_chain_model_cpu.py holds it to the fp64
oracle at 1e-10).  Only the residual (term sums, fields, the output adjoint G = d loss / d (Y, dY)) comes from
oracle/pinn_oracle.py's residual functions through torch autograd, on a per-point linear surrogate of the network whose value
and first derivatives are the model's (Y, dY) (surrogate_outputs).

The rounding points, as read from pinn_depthestimation_amd/csrc (l = 1 .. L-1 numbers the hidden W x W matrices; a_l is the
jet (value a, tangents t_c) after hidden layer l; bf() rounds fp32 to bf16, round to nearest even):

  hidden weights       hi = bf(w), lo = bf(w - hi); both chains multiply by hi AND lo, fp32 accumulate.  The reverse chain's
                       W^T is split element by element the same way.                    pinn_wide.hip (k_chain_pack)
                       forward MFMAs chain_kernel.h:536-537, reverse :739-742.  Biases stay fp32 (:472, bias_lds :340).
  output layer forward W_L split hi + lo in the kernel, product on the stored bf16 a_L, bias and accumulate fp32.
                                                                                          chain_kernel.h:1088-1092, 1116-1117
  first layer, folded  (d_in <= 3 and L >= 2, bf16_chunk in pinn_wide.hip): z = W_0 x + b_0 in fp32 from the unrounded X and W_0,
                       a = tanh(z), t_c = (1 - a^2) W_0[:, dir_col[c]] with 1 - a^2 from the unrounded a; a and t_c are
                       rounded when they become the first MFMA operand, which is also what is stored as a_1.
                                                                                          chain_kernel.h:438-443 (make_a1)
  first layer, wide    (d_in > 3, or L == 1): fp32 MFMA (THIN_FIRST_FWD in pinn_wide_units.hip), activate() takes 1 - a^2
                       from the unrounded a (fused_kernel.h:207-211), the jet is rounded by the store (FMT_OUT16,
                       wide_kernel.h jet_st).  Same rounding points as the folded form; another tanh (tanh_f32).
  hidden layer forward z + b in fp32, a = 1 - 2 / (exp2(2 log2(e) z) + 1), 1 - a^2 from the UNROUNDED a, tangents scaled by
                       it, only then a and t_c are rounded: the next operand and the stored a_l are the same registers.
                                                                                          chain_kernel.h:476-487 (act)
  reverse chain        1 - a^2 from the STORED (rounded) a (:666-667); cross term on the stored rounded tangents (:677);
                       zbar_0 = sv abar_0 - 2 a sum_c abar_c t_c, zbar_c = abar_c sv (:678-680); zbar is rounded (:686) and
                       that one rounded value is both stored (:730) and multiplied by W^T (:739-742).  abar stays in the fp32
                       accumulators between layers (:673); at l = L-1 it is read from the bf16 abar_L (:672).  abar_1 is
                       stored as bf16 (:767).
  output layer reverse abar_L = bf(W_L^T G) from the fp32, unsplit W_L (chain_kernel.h:1038; d_out > 4: k_wide_bwd on fp32
                       MFMAs with FMT_OUT16, THIN_LAST_BWD in pinn_wide_units.hip).  dW_L = sum G (x) a_L on the bf16 a_L with fp32 G
                       (:1043; wide: k_wide_wgrad, FMT_IN16), db_L = sum_p G_0 in fp32 (:1024; k_wide_wgrad's bs).
  hidden gradients     k_chain_wgrad8: dW_l = sum zbar_l (x) a_l on the stored bf16 zbar_l and a_l (:831, :881); db_l is the
                       sum of the stored bf16 zbar_l's value quantity (:869-873).
  first layer reverse  folded (k_chain_first_bwd): zbar from the bf16 abar_1 and a_1 in fp32 (:959-964), NOT rounded: dW_0
                       and db_0 are fp32 sums of it (:965-976).  Wide (d_in > 3 or L == 1): k_wide_bwd writes zbar_0 as bf16
                       (THIN_FIRST_BWD in pinn_wide_units.hip, FMT_OUT16) and k_wide_wgrad reads that (THIN_FIRST_WGRAD, FMT_GIN16): dW_0 and db_0
                       are sums of the ROUNDED zbar_0.
  residual epilogue    fp32 on the fp32 outputs (loss_epilogue, chain_kernel.h:1121): no bf16 anywhere.

The forward value path does not depend on the tangents, so forward() (K1 = 1) and forward_jet() share their Y in the model.

Emulations (VARIANTS): the same computation in fp32 — k-steps of 16 / 32 / 64 or the whole row, ascending or descending, hi
before lo or after; tanh as tanh_bf's exp form, as act()'s exp2 form (with its shared expression for tangent 1,
(x sv - a) par + a, chain_kernel.h:481), correctly rounded, and act()'s form with exp2 and the reciprocal one ulp off in the
four sign combinations (v_exp_f32 and v_rcp_f32 are accurate to 1 ulp; a one-sided error does not average out over the points).
The largest distance of an emulation from the model, per quantity, is the case's noise; the bound is max(floor, 4 x noise).
"""
import random

import torch

from oracle import pinn_oracle as O
from tests.trained_state_util import param_blocks, trained_like

FLOOR = {"sum": 3e-6, "block": 2e-5, "jet": 3e-6}      # the project's fp32 bounds: atomics and launch geometry reorder sums
MARGIN = 4.0                                           # "4 x the reference's own noise", as everywhere in the suite
CAP = 1e-3                                             # a case's bound on every term sum and gradient block must stay below
MI355X_CUS = 256


def bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def split_hi_lo(w32):
    hi = w32.float().to(torch.bfloat16).float()
    lo = (w32.float() - hi).to(torch.bfloat16).float()
    return hi, lo


# ---- networks ---------------------------------------------------------------------------------------------------------------
NETS = {
    # name: d_in, d_out, grad_cols, residual, input names, output names
    "ns": (3, 4, (0, 1, 2), "Navier_Stokes", ("t", "x", "y"), ("h", "z", "u", "v")),                 # K1 = 4
    "cf": (2, 3, (0, 1), "continuity_ftemp", ("x", "y"), ("U", "V", "h")),                          # K1 = 3
    "co": (2, 3, (0, 1), "continuity_only", ("x", "y"), ("U", "V", "h")),                           # K1 = 3, masked term
    "pe": (2, 6, (0, 1), "physics_equation", ("x", "y"), ("h", "U", "V", "eta_mean", "Hrms", "k")),   # d_out = 6: wide output layer
    "ns4": (4, 4, (1, 2, 3), "Navier_Stokes", ("aux", "y", "t", "x"), ("z", "v", "h", "u")),         # d_in = 4: wide first layer
}


class Case:
    """One network, state, point set and request list.  n = (m, add): N = m * B + add with B = 64 * CUs."""

    def __init__(self, name, net, L, W, n, calls=("residual",), gain=1.0, seed=0):
        self.name, self.net, self.L, self.W, self.n, self.calls, self.gain, self.seed = name, net, L, W, n, tuple(calls), gain, seed
        self.d_in, self.d_out, self.gc, self.res, self.inn, self.outn = NETS[net]
        self.layers = O.layer_sizes(self.d_in, L, W, self.d_out)

    def N(self, cus):
        return self.n[0] * 64 * cus + self.n[1]

    def data(self, cus):
        """(params list fp32, X (N, d_in) fp32, T (N, 2) fp32) — biased state in the manner of trained_state_util."""
        g = torch.Generator().manual_seed(4242 + self.seed)
        params = trained_like(self.layers, g, gain=self.gain, bias=0.5, residual=self.res, outn=self.outn)
        N = self.N(cus)
        X = torch.rand(N, self.d_in, generator=g) * 2 - 1
        if self.res == "continuity_only":
            X[:, self.inn.index("x")] *= 40
        # targets that depend on the inputs: with white-noise targets the fidelity gradient of W_0 is a cancelling sum
        T = 0.5 + 0.4 * X[:, [0, self.d_in - 1]] / X.abs().max() + 0.1 * torch.rand(N, 2, generator=g)
        return params, X, T

    def request(self, kind, cus):
        """The request of call `kind` on this case's points: dict(kind, n_res, cols, scale, cscale)."""
        N = self.N(cus)
        n_res = N if kind != "split" else max(1, N - max(1, N // 5))
        if kind == "split" and n_res == N:
            n_res = N - 1 if N > 1 else N
        n_terms = {"Navier_Stokes": 3, "physics_equation": 3, "continuity_ftemp": 1, "continuity_only": 3}[self.res]
        scale = torch.tensor([1.0, 0.5, 2.0][:n_terms]) / max(n_res, 1)
        if self.res == "continuity_only":
            scale[2] = 0.0
        n_fid = {"split": N - n_res, "onepass": N, "mse": N}.get(kind, 0)
        return dict(kind=kind, n_res=n_res, cols=(0, self.d_out - 1), scale=scale, cscale=torch.tensor([0.7, 1.3]) / max(n_fid, 1))


def branches(c, kind, cus):
    """Which path of bf16_chunk (pinn_wide.hip) a call takes: a restatement of its conditions."""
    N = c.N(cus)
    nh = c.L - 1
    n_tiles = (N + 15) // 16
    n_tb = (n_tiles + 3) // 4
    grid = min(n_tb, cus)
    return {"first": "folded" if (nh > 0 and c.d_in <= 3) else "wide",
            "last_bwd": "chain" if c.d_out <= 4 else "wide",
            "nh": "0" if nh == 0 else ("1" if nh == 1 else "more"),
            "NTW": 8 if c.W <= 128 else 16,
            "K1": 1 if kind in ("mse", "forward") else 1 + len(c.gc),
            "batches": "one" if (n_tb + grid - 1) // grid <= 1 or nh == 0 else "several"}


ALL_BRANCHES = {"first": {"folded", "wide"}, "last_bwd": {"chain", "wide"}, "nh": {"0", "1", "more"}, "NTW": {8, 16},
                "K1": {1, 3, 4}, "batches": {"one", "several"}}

EVERY = ("residual", "mse", "split", "forward", "jet", "fields")
TABLE = [
    # depth 1: no chain kernel, abar_1 is abar_L
    Case("L1_ns_w128_n70", "ns", 1, 128, (0, 70), ("residual", "jet")),
    Case("L1_pe_w200_n17", "pe", 1, 200, (0, 17), ("residual", "mse")),
    # depth 2: one hidden matrix — prefetch and store fall into the same, only layer
    Case("L2_ns_w128_n1", "ns", 2, 128, (0, 1), ("residual", "jet")),
    Case("L2_cf_w65_n15", "cf", 2, 65, (0, 15), ("residual", "forward")),
    Case("L2_cf_w200_n16", "cf", 2, 200, (0, 16), ("residual", "jet")),
    Case("L2_ns_w129_n16", "ns", 2, 129, (0, 16), ("residual",)),
    Case("L2_ns_w256_n1000", "ns", 2, 256, (0, 1000), ("residual", "jet")),
    Case("L2_co_w100_n243", "co", 2, 100, (0, 243), ("residual", "split")),
    Case("L2_ns4_w256_n37", "ns4", 2, 256, (0, 37), ("residual", "jet")),
    # depth 3 and 4
    Case("L3_ns_w129_n70", "ns", 3, 129, (0, 70), ("residual", "jet")),
    Case("L3_ns_w129_n1000", "ns", 3, 129, (0, 1000), EVERY),
    Case("L3_pe_w128_n1000", "pe", 3, 128, (0, 1000), EVERY),
    Case("L3_ns4_w100_n1000", "ns4", 3, 100, (0, 1000), ("residual", "mse", "jet")),
    Case("L4_ns_w256_n4000", "ns", 4, 256, (0, 4000), ("residual", "split", "jet")),
    Case("L4_cf_w200_n1000", "cf", 4, 200, (0, 1000), ("residual", "mse", "fields")),
    Case("L4_ns_w129_n243", "ns", 4, 129, (0, 243), ("residual", "jet")),
    # depth 6, damped: the ring wraps across layers
    Case("L6_ns_w128_damped", "ns", 6, 128, (0, 4000), ("residual", "jet"), gain=0.65),
    # point counts around the batch size B = 64 CUs
    Case("L2_ns_w128_Bm1", "ns", 2, 128, (1, -1), ("residual",)),
    Case("L2_cf_w129_Bp1", "cf", 2, 129, (1, 1), ("residual",)),
    Case("L2_pe_w65_Bp1", "pe", 2, 65, (1, 1), ("residual",)),
    Case("L3_ns_w65_Bp83", "ns", 3, 65, (1, 83), ("residual", "jet")),
    Case("L2_cf_w256_Bp83", "cf", 2, 256, (1, 83), ("residual",)),
    Case("L2_ns4_w65_Bp83", "ns4", 2, 65, (1, 83), ("residual",)),
    Case("L3_ns_w100_2Bp17_mse", "ns", 3, 100, (2, 17), ("mse",)),
    Case("L2_ns_w100_2Bp17", "ns", 2, 100, (2, 17), ("residual",)),
    Case("L3_cf_w65_3Bp49", "cf", 3, 65, (3, 49), ("residual",)),
    # beyond 8 B: the loops of k_chain_first_bwd / k_chain_last_bwd (fidelity alone, K1 = 1: the test takes 1.4 s with its
    # fp64 model and three emulations; the residual request on these points took 6.5 s)
    Case("L2_cf_w65_8Bp33", "cf", 2, 65, (8, 33), ("mse",)),
]
TABLE_BY_NAME = {c.name: c for c in TABLE}
SWEEP_SEEDS = list(range(7000, 7040))


def draw(seed):
    """One sweep case: a random shallow shape, state, point count and request kind."""
    r = random.Random(seed)
    net = r.choice(["ns", "ns", "cf", "co", "pe", "ns4"])
    L = r.choice([1, 2, 2, 3, 3, 4])
    W = r.choice([65, 72, 100, 128, 129, 200, 256])
    # the smallest point count at which a depth and width keep their bounds under the cap (measured on the CPU model:
    # rounding flips average out like 1 / sqrt(N), and a flip at depth l disturbs its point in every later layer)
    least = {1: 1, 2: 1, 3: 70 if W <= 129 else 700, 4: 700 if W <= 129 else 4000}[L]
    n = r.choice([n for n in [(0, 1), (0, 15), (0, 37), (0, 243), (0, 700), (0, 4000), (1, -1), (1, 83)] if n[0] or n[1] >= least])
    if W > 128 and n[0]:
        n = (0, 4000)
    kind = r.choice(["residual", "residual", "split", "onepass", "mse"])
    return Case(f"sweep{seed}", net, L, W, n, (kind,), gain=r.choice([1.0, 0.7]), seed=seed)


# ---- the residual, from the oracle ------------------------------------------------------------------------------------------
def surrogate_outputs(c, Y, dY, X):
    """(input columns, output columns) of a per-point LINEAR network surrogate: value Y, derivative dY[i] along grad_cols[i].
    O.compute_gradient of its outputs returns dY exactly, so the oracle's residual functions see the model's jets."""
    cols = [X[:, j:j + 1].clone().requires_grad_(j in c.gc) for j in range(c.d_in)]
    Ys = Y
    for i, j in enumerate(c.gc):
        Ys = Ys + dY[i] * (cols[j] - cols[j].detach())
    return cols, Ys


def residual_fields(c, Y, dY, X):
    """List of the residual's per-point fields, (N, 1) each, differentiable in (Y, dY)."""
    from pinn_depthestimation_amd.engine import RESIDUAL_ROLES
    _, out_roles, dir_roles = RESIDUAL_ROLES[c.res]
    cols, Ys = surrogate_outputs(c, Y, dY, X)
    ins = [cols[c.inn.index(r)] for r in dir_roles]
    outs = [Ys[:, c.outn.index(r):c.outn.index(r) + 1] for r in out_roles]
    if c.res == "Navier_Stokes":
        return list(O.navier_stokes_fields(*ins, *outs)), None
    if c.res == "physics_equation":
        return list(O.physics_equation_fields(*ins, *outs)), None
    fc = O.continuity_fields(*ins, *outs)
    if c.res == "continuity_ftemp":
        return [fc], None
    on = (ins[0] < 25.5).detach()
    return [fc, torch.where(on, outs[0] - 0.75, torch.zeros_like(fc))], on


def loss_and_adjoint(c, Y, dY, X, T, rq):
    """(term sums, fidelity column sums, fields, G_Y, G_dY) of request rq at the jets (Y, dY), in their dtype."""
    dt = Y.dtype
    Yv, dYv = Y.detach().clone().requires_grad_(True), dY.detach().clone().requires_grad_(True)
    N, n_res = Y.shape[0], rq["n_res"]
    total = torch.zeros((), dtype=dt)
    sums, csums, fields = torch.zeros(0, dtype=dt), torch.zeros(0, dtype=dt), None
    if rq["kind"] in ("residual", "split", "onepass", "fields"):
        f, on = residual_fields(c, Yv[:n_res], dYv[:, :n_res], X[:n_res].to(dt))
        s = [(x ** 2).sum() for x in f]
        if on is not None:
            s.append(on.sum().to(dt))
        sums = torch.stack(s)
        total = total + (rq["scale"].to(dt) * sums).sum()
        fields = torch.cat([x.detach() for x in f], 1).T.contiguous()
    if rq["kind"] in ("mse", "split", "onepass"):
        rows = slice(n_res, N) if rq["kind"] == "split" else slice(0, N)
        Tt = T[: N - n_res] if rq["kind"] == "split" else T
        csums = torch.stack([((Tt[:, j].to(dt) - Yv[rows, o]) ** 2).sum() for j, o in enumerate(rq["cols"])])
        total = total + (rq["cscale"].to(dt) * csums).sum()
    if rq["kind"] in ("forward", "jet", "fields"):
        return sums.detach(), csums.detach(), fields, None, None
    gY, gdY = torch.autograd.grad(total, [Yv, dYv], allow_unused=True)
    gdY = torch.zeros_like(dYv) if gdY is None else gdY
    return sums.detach(), csums.detach(), fields, gY, gdY


# ---- the model and its emulations -------------------------------------------------------------------------------------------
# name: (k-chunk of the summation (0: the whole row in one product), descending chunks, hi before lo, tanh form)
VARIANTS = {
    "row_hi_lo": (0, False, True, "exp"),
    "k32_lo_hi": (32, False, False, "exp"),
    "row_lo_hi_tanh": (0, False, False, "tanh"),
    "k32_down_hi_lo_exp2": (32, True, True, "exp2"),
    "k16_hi_lo_exp2": (16, False, True, "exp2"),
    "k64_down_lo_hi_tanh": (64, True, False, "tanh"),
    # v_exp_f32 and v_rcp_f32 are accurate to 1 ulp, not correctly rounded, and nothing says their errors have mean zero:
    # act()'s formula with both results one ulp off, in the four sign combinations.  A one-sided error does not average
    # out over the points (1 - a^2 of a nearly saturated unit magnifies it): at 4 x 72, 16 000 points, exp2 one ulp up
    # and rcp one ulp down move every gradient block by 3e-5 .. 5e-5, the correctly rounded forms by 1e-5.
    "k32_hi_lo_ulp_uu": (32, False, True, "exp2++"),
    "k32_hi_lo_ulp_dd": (32, False, True, "exp2--"),
    "k32_lo_hi_ulp_ud": (32, False, False, "exp2+-"),
    "k32_down_hi_lo_ulp_du": (32, True, True, "exp2-+"),
}
# beyond MANY_POINTS points (rounding flips average out there; one-sided errors do not)
FEW_VARIANTS = ("k32_lo_hi", "row_lo_hi_tanh", "k16_hi_lo_exp2", "k32_lo_hi_ulp_ud", "k32_down_hi_lo_ulp_du")
MANY_POINTS = 2048
VERY_FEW_VARIANTS = ("k32_lo_hi", "k16_hi_lo_exp2", "k32_lo_hi_ulp_ud")     # beyond HUGE_POINTS points: the reference must stay quick
HUGE_POINTS = 65536
# The emulations are the same on every machine: each transcendental and each partial product is formed in fp64 and
# rounded to fp32 once (what an ideal fp32 unit returns), and only IEEE additions, multiplications and divisions follow in fp32.
_f = lambda fn: (lambda z: fn(z.double()).to(z.dtype))
TANH = {
    "exp": lambda z: 1 - 2 / (_f(torch.exp)(2 * z) + 1),                               # chain_kernel.h:163-164 (tanh_bf)
    "exp2": lambda z: 1 - 2 * (1 / (_f(torch.exp2)(z * 2.885390081777927) + 1)),       # chain_kernel.h:476-479 (act)
    "tanh": _f(torch.tanh),                                                           # a correctly rounded tanh
}
ULP = 2.0 ** -23


def _one_ulp_off(se, sr):
    return lambda z: 1 - 2 * ((1 / (_f(torch.exp2)(z * 2.885390081777927) * (1 + se * ULP) + 1)) * (1 + sr * ULP))


for _n, _se, _sr in (("exp2++", 1, 1), ("exp2--", -1, -1), ("exp2+-", 1, -1), ("exp2-+", -1, 1)):
    TANH[_n] = _one_ulp_off(_se, _sr)
MUTANTS = ("lo dropped, hidden forward", "lo dropped, reverse product", "lo dropped, output forward",
           "forward 1-a^2 from rounded a", "reverse 1-a^2 from unrounded a", "zbar unrounded in the weight gradient",
           "abar_L unrounded", "one tangent unrounded", "point 7 of 16 on the previous layer's weights",
           "hidden bias block shifted by one unit")


def _mm(variant):
    """(v, hi, lo) -> v @ (hi + lo)^T in the variant's summation order (None: the fp64 model, one exact product).  A chunk's
    partial product is exact (bf16 x bf16 products in fp64) and rounded to fp32 once, as an MFMA's k-step is; the chunks
    accumulate in fp32."""
    if variant is None:
        return lambda v, hi, lo: v @ (hi + lo).T
    chunk, down, hi_first, _ = VARIANTS[variant]

    def mm(v, hi, lo):
        first, second = (hi.double(), lo.double()) if hi_first else (lo.double(), hi.double())
        v = v.double()
        step = chunk or hi.shape[1]
        ks = list(range(0, hi.shape[1], step))
        acc = None
        for k in (reversed(ks) if down else ks):
            for w in (first, second):
                part = (v[:, k:k + step] @ w[:, k:k + step].T).float()
                acc = part if acc is None else acc + part
        return acc
    return mm


def _thin(variant):
    """(v, w) -> v @ w for the thin first / last layers: exact, rounded to the working precision once."""
    if variant is None:
        return lambda v, w: v @ w
    return lambda v, w: (v.double() @ w.double()).float()


def run(c, params, X, T, rq, rounding=True, variant=None, mutant=None, tap=None):
    """What bf16 mode computes for request rq: dict(Y, dY, sums, csums, fields, grad).  variant=None: the fp64 model;
    else the fp32 emulation of that name.  rounding=False: exact arithmetic (the derivative).  mutant: one of MUTANTS."""
    dt = torch.float64 if variant is None else torch.float32
    mm, thin = _mm(variant), _thin(variant)
    tanh = torch.tanh if variant is None else TANH[VARIANTS[variant][3]]
    parf = variant is not None and VARIANTS[variant][3].startswith("exp2")
    rd = bf if rounding else (lambda x: x)
    L, nh = c.L, c.L - 1
    gc = () if rq["kind"] in ("mse", "forward") else c.gc
    P = [p.to(dt) for p in params]
    Xd = X.to(dt)

    def halves(l, drop=False):
        if not rounding:
            return P[2 * l], torch.zeros_like(P[2 * l])
        hi, lo = split_hi_lo(params[2 * l])
        return hi.to(dt), (torch.zeros_like(lo) if drop else lo).to(dt)

    def bias(l):
        b = P[2 * l + 1]
        if mutant == "hidden bias block shifted by one unit" and l == min(1, nh):
            b = b.clone(); b[:16] = torch.roll(b[:16], 1)
        return b

    # ---- forward
    a = tanh(thin(Xd, P[0].T) + bias(0))
    sv = 1 - a * a
    t = [sv * P[0][:, j] for j in gc]
    skip_t = mutant == "one tangent unrounded"
    A = [None, (rd(a), [x if (skip_t and nh == 0 and i == 0) else rd(x) for i, x in enumerate(t)], a)]
    p7 = (torch.arange(X.shape[0]) % 16 == 7)[:, None]
    for l in range(1, nh + 1):
        ar, tr, _ = A[l]
        hi, lo = halves(l, drop=(mutant == "lo dropped, hidden forward" and l == nh))
        z = mm(ar, hi, lo)
        zd = [mm(x, hi, lo) for x in tr]
        if mutant == "point 7 of 16 on the previous layer's weights" and l == nh and nh >= 2:
            hp, lp = halves(l - 1)
            z = torch.where(p7, mm(ar, hp, lp), z)
            zd = [torch.where(p7, mm(x, hp, lp), y) for x, y in zip(tr, zd)]
        a = tanh(z + bias(l))
        sv = 1 - (rd(a) * rd(a) if mutant == "forward 1-a^2 from rounded a" else a * a)
        t = [sv * x for x in zd]
        if parf and t:
            t[0] = (zd[0] * sv - a) + a          # chain_kernel.h:481: tangent 1 shares its expression with the value lanes
        A.append((rd(a), [x if (skip_t and l == 1 and i == 0) else rd(x) for i, x in enumerate(t)], a))
    aL, tL, _ = A[L]
    hi, lo = halves(L, drop=(mutant == "lo dropped, output forward"))
    Y = mm(aL, hi, lo) + P[2 * L + 1]
    dY = torch.stack([mm(x, hi, lo) for x in tL]) if gc else torch.zeros(0, X.shape[0], c.d_out, dtype=dt)
    out = dict(Y=Y, dY=dY)
    out["sums"], out["csums"], out["fields"], gY, gdY = loss_and_adjoint(c, Y, dY, X, T, rq)
    if gY is None:
        return out
    # ---- reverse
    G = [gY] + [gdY[i] for i in range(len(gc))]
    grads = [None] * (2 * (L + 1))
    jet = [aL] + tL
    grads[2 * L] = sum(g.T @ x for g, x in zip(G, jet))
    grads[2 * L + 1] = gY.sum(0)
    abar = [thin(g, P[2 * L]) for g in G]
    if mutant != "abar_L unrounded":
        abar = [rd(x) for x in abar]

    def adjoint(abar, a_st, t_st, a_sv):
        sv = 1 - a_sv * a_sv
        cross = sum((ab * x for ab, x in zip(abar[1:], t_st)), torch.zeros_like(a_st))
        return [sv * abar[0] - 2 * a_st * cross] + [ab * sv for ab in abar[1:]]

    for l in range(nh, 0, -1):
        a_st, t_st, a_un = A[l + 1]
        zb = adjoint(abar, a_st, t_st, a_un if mutant == "reverse 1-a^2 from unrounded a" else a_st)
        zr = [rd(x) for x in zb]
        zw = zb if mutant == "zbar unrounded in the weight gradient" else zr
        a_in, t_in, _ = A[l]
        grads[2 * l] = sum(z.T @ x for z, x in zip(zw, [a_in] + t_in))
        grads[2 * l + 1] = zw[0].sum(0)
        if tap is not None:
            tap[l] = (zw, [a_in] + t_in)
        hi, lo = halves(l, drop=(mutant == "lo dropped, reverse product" and l == 1))
        abar = [mm(z, hi.T, lo.T) for z in zr]
    if nh > 0:
        abar = [rd(x) for x in abar]
    a_st, t_st, _ = A[1]
    zb = adjoint(abar, a_st, t_st, a_st)
    if not (nh > 0 and c.d_in <= 3):
        zb = [rd(x) for x in zb]
    dW0 = zb[0].T @ Xd
    for i, j in enumerate(gc):
        dW0[:, j] += zb[1 + i].sum(0)
    grads[0], grads[1] = dW0, zb[0].sum(0)
    out["grad"] = torch.cat([g.reshape(-1) for g in grads]).double()
    return out


# ---- quantities, noise, bounds ------------------------------------------------------------------------------------------------
def quantities(c, res):
    """{name: (kind, tensor)} of everything compared: term sums, fidelity sums, gradient blocks, jets per output column."""
    q = {}
    for i, s in enumerate(res.get("sums", ())):
        q[f"sum{i}"] = ("sum", s.double().reshape(1))
    for i, s in enumerate(res.get("csums", ())):
        q[f"col{i}"] = ("sum", s.double().reshape(1))
    if res.get("grad") is not None:
        for name, a, b in param_blocks(c.layers):
            q[name] = ("block", res["grad"][a:b].double())
    if res.get("Y") is not None:
        for o in range(c.d_out):
            q[f"Y{o}"] = ("jet", res["Y"][:, o].double())
            if res.get("dY") is not None and res["dY"].numel():
                q[f"dY{o}"] = ("jet", res["dY"][:, :, o].double().reshape(-1))
    if res.get("fields") is not None:
        for i, f in enumerate(res["fields"]):
            q[f"field{i}"] = ("jet", f.double())
    return q


def distance(got, ref):
    rn = float(ref.norm())
    dn = float((got - ref).norm())
    return dn / rn if rn > 0 else (0.0 if dn == 0 else float("inf"))


def distances(c, got, ref):
    qg, qr = quantities(c, got), quantities(c, ref)
    return {k: distance(qg[k][1], qr[k][1]) for k in qr if k in qg}


_REF = {}


def reference(c, kind, cus):
    """(model result, {quantity: bound}, {quantity: noise}) of one call of a case; computed once per process, left unchanged."""
    key = (c.name, kind, cus)
    if key not in _REF:
        params, X, T = c.data(cus)
        rq = c.request(kind, cus)
        model = run(c, params, X, T, rq)
        noise = {}
        for v in (VARIANTS if X.shape[0] <= MANY_POINTS else FEW_VARIANTS if X.shape[0] <= HUGE_POINTS else VERY_FEW_VARIANTS):
            for k, d in distances(c, run(c, params, X, T, rq, variant=v), model).items():
                noise[k] = max(noise.get(k, 0.0), d)
        kinds = {k: v[0] for k, v in quantities(c, model).items()}
        bound = {k: max(FLOOR[kinds[k]], MARGIN * noise[k]) for k in noise}
        _REF[key] = (model, bound, noise)
    return _REF[key]


def capped(c, bound):
    """The quantities of a case the 1e-3 condition speaks of (term sums, fidelity sums, gradient blocks) above the cap."""
    return {k: b for k, b in bound.items() if (k.startswith(("sum", "col", "W", "b"))) and not b <= CAP}


def cancelling(c, kind, cus):
    """A sweep draw's own reason to be skipped, or None: fewer than 16 points under continuity_only's mask (its anchor
    term is then a sum of a handful of squares), or a request whose residual part has fewer than 16 points."""
    params, X, T = c.data(cus)
    rq = c.request(kind, cus)
    if kind != "mse" and c.res == "continuity_only" and int((X[:rq["n_res"], c.inn.index("x")] < 25.5).sum()) < 16:
        return "fewer than 16 points under the mask"
    return None


def ratios(c, got, model, bound):
    """{quantity: distance / bound}; a quantity whose reference is zero must be zero."""
    return {k: d / bound[k] for k, d in distances(c, got, model).items() if k in bound}
