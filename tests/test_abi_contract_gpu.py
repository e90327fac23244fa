"""The C-ABI's buffer contract (include/pinn_hip.h, "Buffer contract"): where the library reads and writes.

Every call below goes through the raw entry point (eng._run + _ptr) with every output, every caller-owned scratch and
the workspace itself inside guard bands (tests/abi_contract_util.py; the workspace is passed with exactly the queried
number of bytes), and with a bit-exact snapshot of every read-only argument.  Four checks:
  A  extent: both bands of every buffer intact, read-only arguments unchanged;
  B  dirty workspace: the same call on a zero-filled and on a 1e30-filled workspace gives the same result;
  C  history: the last call of a sequence on ONE workspace equals that call on a zero-filled workspace of its own;
  D  grad_flat is += (checked against the fp64 oracle on a pre-filled gradient) or overwritten (the two Adam entries);
     the N = 0 early returns leave grad alone and zero the sums.
Outputs that are overwritten (Y, dY, d2Y, fields, term_sums, col_sums, losses, X_out, d) start as 1e30 in every call, so
an entry that added instead of storing is off by 1e30.

No integer, offset or pointer is read from a workspace before the same call writes it (read from the code before any
entry was run on poison):
  fused_workspace_bytes          packed W, W^T, b (k_pack writes all PW / PB floats, padding included, unless the caller
                                 says packed_valid), activation spills (each wave writes a slot in the forward sweep and
                                 reads it back in the reverse one), wg_sums / wg_grads rows (floats; rows [0, grid) are
                                 written by the pass or zeroed by the launch code, and only those are reduced).  The
                                 locks of fused_kernel.h:370-382 live in LDS and the kernel zeroes them; nothing else
                                 in the layout is an integer.
  wide_workspace_bytes           packed fp32 weights and, in bf16 mode, fragment planes (written by k_wide_pack / k_chain_pack),
                                 fp32 or bf16 jets and adjoints (written layer by layer before the next layer reads
                                 them), the partial-sum table (zeroed per chunk): floats and bf16 only.
  generic_workspace_bytes        a_0..a_L, out, two adjoint buffers, per-block partial sums: floats, each written by
                                 the launch in front of the one that reads it.
  jet2_workspace_bytes           the same with z_l added: floats only.
  fused_fields_workspace_bytes   the packed weights alone (floats); the staged path: Y, dY (floats, written by the
                                 forward jet) + the inner engine's layout above.
  pinn_stage_workspace_bytes     int block counts: k_stage_count writes all nb of them, k_stage_scan reads [0, nb) after
                                 it, k_stage_write reads what the scan left.  pinn_nanminmax_f64: 2 nb doubles, written
                                 by the partial kernel before the final one reads them.

Bit equality or 1e-6 (check B and C; `sums` / `grad` of a family below).  Point-wise outputs are always torch.equal.
Sums and gradients are torch.equal where the launch code fixes the order of the additions:
  generic     per-block partials summed in index order; k_wgrad is one block per 16 x 16 weight tile while
              N <= 16384 (its chunk), so each gradient entry receives a single add: sums and gradient exact.
  tile        a wave's tiles are fixed by its index, waves are combined in index order and k_reduce_sums /
              k_reduce_grads add the workgroups' rows in index order: sums exact.  The waves of a workgroup add into
              its gradient copy under a lock in arrival order: gradient exact only while one wave has work (N <= 16),
              else run-to-run.
  adjoint     (pinn_jet_backward) one workgroup per tile while N <= 16 W (W >= CUs): exact (pinn_hip.h).
  coop, batch, wide, bf16, dropout, jet2-backward above 512 points (k2_wgrad's chunk; atomics above it), the Adam
              entries: run-to-run figures of tests/test_fullsize_gpu.py:88-90 for the same kernels: sums rtol 1e-6,
              gradient rel-L2 < 1e-6.  (Not shown exact here; the order of LDS-lock or atomic arrivals varies.)
+= against the oracle (check D): rel-L2(grad_after - g0, fp64 oracle) < max(2e-5, 4 gnoise), gnoise the oracle's own
fp32-vs-fp64 distance (tests/test_engine_gpu.py).  The two bf16 families cannot meet an fp32 bar (bf16 operands carry 8
significant bits: a tolerance mode, pinn_hip.h): they are held to the gradient bar tests/test_sweep_gpu.py already applies
to bf16 mode on shallow nets, 1e-1 — a store, a double add or a missed layer is off by O(1) all the same.
Every family is also held to its own gradient on a zeroed grad, at 1e-6 + 4 * 2^-24 (run-to-run plus the rounding of
the final additions onto g0): the sharp form of the += check where the oracle bar is wide.
pinn_adam_loop over three iterations: only iteration 0 (and a loop of one iteration) is one pass on shared parameters
and meets check B's figures; what later iterations leave is held to tests/test_sweep_gpu.py:260-264's figures for two
runs of the same Adam iterations (sums rtol 1e-5, gradient / m / v rel-L2 5e-6, parameters in units of the step).

Every test prints its worst dirty-vs-clean and +=-vs-oracle distances (-s).
"""
import ctypes as C
import functools
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np
import pytest
import torch

from oracle import pinn_oracle as O
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec
from pinn_depthestimation_amd import _lib as L_
from pinn_depthestimation_amd._lib import (ACT_LEAKY_RELU, ACT_TANH, ENGINE_AUTO, ENGINE_FUSED, ENGINE_FUSED_BATCH,
                                           ENGINE_FUSED_COOP, ENGINE_FUSED_TILE, ENGINE_GENERIC, ENGINE_WIDE, PREC_BF16,
                                           PinnAdamState, check)
from pinn_depthestimation_amd.engine import RESIDUAL_ROLES, _ptr

from tests.abi_contract_util import POISON, assert_unchanged, guarded, poison_workspace, snapshot
from tests.dropout_util import keep_masks
from tests.golden_util import rel_l2
from tests.lbfgs_util import BAR as LBFGS_BAR

pytestmark = pytest.mark.gpu

NS = ("Navier_Stokes", ("t", "x", "y"), ("h", "z", "u", "v"), (0, 1, 2))
NS5 = ("Navier_Stokes", ("t", "x", "y", "u0", "v0"), ("h", "z", "u", "v"), (0, 1, 2))
CF = ("continuity_ftemp", ("x", "y"), ("U", "V", "h"), (0, 1))
CO = ("continuity_only", ("x", "y"), ("U", "V", "h"), (0, 1))
PE4 = ("physics_equation", ("x", "y", "a", "b"), ("h", "U", "V", "eta_mean", "Hrms", "k"), (0, 1))
ADJ2 = (None, ("x", "y"), ("o0", "o1", "o2"), (0, 1))
ADJ3 = (None, ("t", "x", "y"), tuple(f"o{i}" for i in range(7)), (0, 1, 2))

FWD = ("forward", "forward_jet")
LOSS = ("residual_loss", "residual_loss_grad", "mse_loss_grad", "residual_mse", "split")
CORE = FWD + LOSS
ALL = CORE + ("jet_backward", "fields")
GRAD_ENTRIES = ("residual_loss_grad", "mse_loss_grad", "residual_mse", "split", "jet_backward", "jet2_backward")
POINTWISE = ("Y", "dY", "d2Y", "fields")
DROP_SEED = 4242

never = lambda N: False
always = lambda N: True


@dataclass(frozen=True)
class Family:
    net: tuple                      # (residual, inputs, outputs, grad_cols)
    L: int
    W: int
    engine: int
    entries: Tuple[str, ...]
    Ns: Tuple[int, ...] = (1, 17, 777)
    act: int = ACT_TANH
    prec: int = 0
    drop: float = 0.0
    sums_exact: bool = False        # check B / C: torch.equal (True) or rtol 1e-6 — why: the module docstring
    grad_exact: Callable = never    # N -> torch.equal (True) or rel-L2 < 1e-6
    oracle_bar: Optional[float] = None   # check D: None = max(2e-5, 4 gnoise); bf16: 1e-1 (module docstring)
    n_D: int = 777


one_wave = lambda N: N <= 16
FAMILIES = {
    # generic: every order fixed (N <= 16384)
    "generic_ns5in_3x20": Family(NS5, 3, 20, ENGINE_GENERIC, ALL, sums_exact=True, grad_exact=always),
    # tile kernel, gradient copy in LDS, padded width 16 / 32 / 64: sums exact, gradient exact while one wave works
    "tile16_ns_3x12": Family(NS, 3, 12, ENGINE_FUSED_TILE, ALL, sums_exact=True, grad_exact=one_wave),
    "tile32_cf_3x32": Family(CF, 3, 32, ENGINE_FUSED_TILE, ALL, sums_exact=True, grad_exact=one_wave),
    "tile64_ns_2x48": Family(NS, 2, 48, ENGINE_FUSED_TILE, ALL, sums_exact=True, grad_exact=one_wave),
    # specialised epilogue (io1: inputs / outputs packed k-step-major) for the residual-only gradient pass
    "tile64_io1_ns_1x64": Family(NS, 1, 64, ENGINE_FUSED_TILE, CORE, sums_exact=True, grad_exact=one_wave),
    # gradient too large for LDS: per-workgroup global copies, zeroed by the launch code
    "tile_global_cf_40x20": Family(CF, 40, 20, ENGINE_FUSED_TILE, ALL, sums_exact=True, grad_exact=one_wave),
    # cooperative kernel (four waves per tile): run-to-run figures
    "coop_co_3x64": Family(CO, 3, 64, ENGINE_FUSED_COOP, CORE, Ns=(1, 17, 243), n_D=243),
    # batch kernel: gradient copies per wave in LDS / atomics into shared global copies: run-to-run figures
    "batch_lds_ns_3x12": Family(NS, 3, 12, ENGINE_FUSED_BATCH, LOSS[1:], Ns=(17, 4097)),
    "batch_atomic_cf_40x20": Family(CF, 40, 20, ENGINE_FUSED_BATCH, LOSS[1:], Ns=(17, 4097)),
    # dropout instances of the tile kernel (gradient passes).  The split request runs as two passes at this width
    # (pinn_fused.hip, fused_loss): residual on the collocation points, then the k = 0 network on the fidelity points with
    # X advanced, so the mask's point index restarts at 0 there (pinn_hip.h, dropout_p) — the oracle does the same.
    "dropout_cf_2x48": Family(CF, 2, 48, ENGINE_AUTO, ("residual_loss_grad", "mse_loss_grad", "residual_mse", "split"), drop=0.3),
    # external adjoint (pinn_jet_backward) on the tile kernel: exact while N <= 16 W
    "adj_tanh_2x3x16x3": Family(ADJ2, 3, 16, ENGINE_FUSED_TILE, FWD + ("jet_backward",), grad_exact=always),
    "adj_leaky_3x4x32x7": Family(ADJ3, 4, 32, ENGINE_FUSED_TILE, FWD + ("jet_backward",), act=ACT_LEAKY_RELU, grad_exact=always),
    # field epilogue of the tile kernel / staged fields (forward jet on the wide engine + point-wise kernel)
    "fields_fused_cf_3x20": Family(CF, 3, 20, ENGINE_FUSED_TILE, ("fields",)),
    "fields_staged_ns_3x100": Family(NS, 3, 100, ENGINE_AUTO, ("fields",)),
    # wide fp32 engine, 128- and 256-wide instances: gradient through global atomics
    "wide128_ns_2x100": Family(NS, 2, 100, ENGINE_WIDE, CORE),
    "wide256_ns_2x200": Family(NS, 2, 200, ENGINE_WIDE, CORE),
    # bf16 chain: first layer folded + streaming output layer (d_in 2, d_out 3) / neither (d_in 4, d_out 6)
    "bf16_cf_2x128": Family(CF, 2, 128, ENGINE_AUTO, CORE, prec=PREC_BF16, oracle_bar=1e-1),
    "bf16_pe4_2x128": Family(PE4, 2, 128, ENGINE_AUTO, CORE, prec=PREC_BF16, oracle_bar=1e-1),
    # second order: VALU and MFMA layer kernels (k2_wgrad: one block per weight tile and 512 points)
    "jet2_valu_cf_3x20": Family(CF, 3, 20, ENGINE_GENERIC, ("forward_jet2", "jet2_backward"), grad_exact=lambda N: N <= 512),
    "jet2_mfma_cf_3x20": Family(CF, 3, 20, ENGINE_FUSED, ("forward_jet2", "jet2_backward"), grad_exact=lambda N: N <= 512),
}


def desc_of(f: Family) -> NetDesc:
    res, inn, outn, gc = f.net
    return NetDesc(len(inn), len(outn), f.L, f.W, gc, f.act, f.engine, f.prec, f.drop)


def spec_of(f: Family) -> Optional[ResidualSpec]:
    res, inn, outn, gc = f.net
    return ResidualSpec.from_names(res, inn, gc, outn) if res else None


# ---- host side of a case: parameters, points, targets, adjoints (computed once, never written) -----------------------
@functools.lru_cache(maxsize=None)
def host_case(name, N):
    f = FAMILIES[name]
    res, inn, outn, gc = f.net
    d = desc_of(f)
    g = torch.Generator().manual_seed(sum(map(ord, name)) * 7 + N)
    init = "kaiming" if f.act == ACT_LEAKY_RELU else "xavier"
    params = O.init_params(d.layers, init, g)
    if res == "physics_equation":            # keep eta_mean + h away from 0 (1 / (rho (eta_mean + h)) is singular there)
        params[-1][outn.index("h")] = 0.75
        params[-1][outn.index("eta_mean")] = 0.0
    X = torch.rand(N, d.d_in, generator=g) * 2 - 1
    if res == "continuity_only":
        X[:, 0] = X[:, 0] * 40                # make x < 25.5 a real subset
    nc = min(2, d.d_out)
    out_col = tuple(range(d.d_out - nc, d.d_out))
    n_res = N - max(1, N // 5) if N > 1 else 0         # the boundary falls inside a tile; N = 1: fidelity point only
    c = dict(params=params, flat=O.flatten(params), X=X.contiguous(), init=init, out_col=out_col, n_res=n_res,
             T=torch.rand(N, nc, generator=g), cs=torch.tensor([0.7, 1.3][:nc]) / N,
             gY=torch.randn(N, d.d_out, generator=g), gdY=torch.randn(d.k, N, d.d_out, generator=g),
             gd2Y=torch.randn(d.k * (d.k + 1) // 2, N, d.d_out, generator=g))
    c["cs_split"] = torch.tensor([0.7, 1.3][:nc]) / (N - n_res)
    if res:
        nt = spec_of(f).n_terms

        def scale(M, Xs):
            if res == "continuity_only":
                return torch.tensor([1.0 / M, 1.0 / max(float((Xs[:, 0] < 25.5).sum()), 1.0), 0.0])
            return torch.full((nt,), 1.0 / M)
        c["ts"] = scale(N, X)
        c["ts_split"] = scale(max(n_res, 1), X[:n_res])
    return c


class Ctx:
    """The device copies of one host case plus snapshots of everything a call may only read."""

    def __init__(self, name, N, device="cuda"):
        self.name, self.N, self.f = name, N, FAMILIES[name]
        h = host_case(name, N)
        self.h = h
        for k in ("flat", "X", "T", "cs", "cs_split", "gY", "gdY", "gd2Y", "ts", "ts_split"):
            setattr(self, k, h[k].to(device).contiguous() if k in h else None)
        self.T_split = self.T[h["n_res"]:].contiguous()
        self.out_col, self.n_res = h["out_col"], h["n_res"]
        self.oc = (C.c_int32 * len(self.out_col))(*self.out_col)
        self.ro = {k: getattr(self, k) for k in ("flat", "X", "T", "T_split", "cs", "cs_split", "gY", "gdY", "gd2Y", "ts", "ts_split")
                   if getattr(self, k) is not None}
        self.snaps = {k: snapshot(v) for k, v in self.ro.items()}

    def assert_readonly(self, what):
        for k, v in self.ro.items():
            assert_unchanged(v, self.snaps[k], f"{k} ({what})")


@functools.lru_cache(maxsize=None)
def ctx(name, N):
    return Ctx(name, N)


# ---- workspaces ------------------------------------------------------------------------------------------------------
def ws_kind(entry):
    return "jet2" if "jet2" in entry else ("fields" if entry == "fields" else "main")


def query(eng, kind, N, spec=None, engine=None):
    need = C.c_int64()
    with torch.cuda.device(eng._index()):
        if kind == "jet2":
            check(eng.lib.pinn_query_jet2_workspace(C.byref(eng._d(engine)), N, C.byref(need)), "pinn_query_jet2_workspace")
        elif kind == "fields":
            check(eng.lib.pinn_query_fields_workspace(C.byref(eng._d(engine)), C.byref(spec.c_struct()), N, C.byref(need)),
                  "pinn_query_fields_workspace")
        else:
            check(eng.lib.pinn_query_workspace(C.byref(eng._d(engine)), N, C.byref(need)), "pinn_query_workspace")
    return need.value


class WS:
    """A workspace of exactly `nbytes` bytes between guard bands."""

    def __init__(self, nbytes, mode):
        self.t, self.guard = guarded(nbytes, torch.uint8, "cuda", fill=0, name="workspace")
        if mode == "poison":
            poison_workspace(self.t)
        else:
            assert mode == "zero"

    @property
    def bytes(self):
        return self.t.numel()


# ---- one raw call ----------------------------------------------------------------------------------------------------
def call(eng, cx, entry, ws, grad0=None, engine=None, N=None, params=None, n_res=None):
    """Run `entry` on the first N points of the case (default: all; entries with adjoints or targets: all or none, their
    arrays are laid out for the case's N) with guarded outputs; n_res: the split point (default: the case's).  Checks A;
    returns the outputs."""
    f, lib = cx.f, eng.lib
    N = cx.N if N is None else N
    n_res = cx.n_res if n_res is None else n_res
    assert N in (0, cx.N) or entry in ("forward", "forward_jet", "forward_jet2", "residual_loss", "residual_loss_grad", "fields")
    d, spec = C.byref(eng._d(engine)), spec_of(f)
    sp = C.byref(spec.c_struct()) if spec else None
    nP, dout, k = eng.n_params, eng.desc.d_out, eng.desc.k
    outs, guards = {}, []

    def out(nm, shape, fill=None):
        t, g = guarded(shape, torch.float32, "cuda", fill=fill, name=f"{nm} of {entry}")
        outs[nm] = t
        guards.append(g)
        return t

    def grad():
        t = out("grad", (nP,))
        t.copy_(grad0 if grad0 is not None else torch.zeros(nP, device="cuda"))
        return t
    P, X, W, nb = _ptr(cx.flat if params is None else params), _ptr(cx.X), _ptr(ws.t), ws.bytes
    nc = len(cx.out_col)
    nt = spec.n_terms if spec else 0
    if entry == "forward":
        eng._run("pinn_forward", lib.pinn_forward, d, P, X, N, _ptr(out("Y", (N, dout))), W, nb)
    elif entry == "forward_jet":
        eng._run("pinn_forward_jet", lib.pinn_forward_jet, d, P, X, N, _ptr(out("Y", (N, dout))), _ptr(out("dY", (k, N, dout))), W, nb)
    elif entry == "jet_backward":
        eng._run("pinn_jet_backward", lib.pinn_jet_backward, d, P, X, N, _ptr(cx.gY), _ptr(cx.gdY), _ptr(grad()), W, nb)
    elif entry == "forward_jet2":
        eng._run("pinn_forward_jet2", lib.pinn_forward_jet2, d, P, X, N, _ptr(out("Y", (N, dout))), _ptr(out("dY", (k, N, dout))),
                 _ptr(out("d2Y", (k * (k + 1) // 2, N, dout))), W, nb)
    elif entry == "jet2_backward":
        eng._run("pinn_jet2_backward", lib.pinn_jet2_backward, d, P, X, N, _ptr(cx.gY), _ptr(cx.gdY), _ptr(cx.gd2Y), _ptr(grad()), W, nb)
    elif entry == "residual_loss":
        eng._run("pinn_residual_loss", lib.pinn_residual_loss, d, sp, P, X, N, _ptr(out("term_sums", (nt,))), W, nb)
    elif entry == "fields":
        eng._run("pinn_residual_fields", lib.pinn_residual_fields, d, sp, P, X, N, _ptr(out("fields", (spec.n_fields, N))), W, nb)
    elif entry == "residual_loss_grad":
        eng._run("pinn_residual_loss_grad", lib.pinn_residual_loss_grad, d, sp, _ptr(cx.ts), P, X, N,
                 _ptr(out("term_sums", (nt,))), _ptr(grad()), W, nb)
    elif entry == "mse_loss_grad":
        eng._run("pinn_mse_loss_grad", lib.pinn_mse_loss_grad, d, P, X, _ptr(cx.T), N, nc, cx.oc, _ptr(cx.cs),
                 _ptr(out("col_sums", (nc,))), _ptr(grad()), W, nb)
    elif entry == "residual_mse":
        eng._run("pinn_residual_mse_loss_grad", lib.pinn_residual_mse_loss_grad, d, sp, _ptr(cx.ts), _ptr(cx.T), nc, cx.oc,
                 _ptr(cx.cs), P, X, N, _ptr(out("term_sums", (nt,))), _ptr(out("col_sums", (nc,))), _ptr(grad()), W, nb)
    elif entry == "split":
        eng._run("pinn_residual_mse_split_loss_grad", lib.pinn_residual_mse_split_loss_grad, d, sp, _ptr(cx.ts_split),
                 _ptr(cx.T_split), nc, cx.oc, _ptr(cx.cs_split), P, X, N, n_res, _ptr(out("term_sums", (nt,))),
                 _ptr(out("col_sums", (nc,))), _ptr(grad()), W, nb)
    else:
        raise KeyError(entry)
    torch.cuda.synchronize()
    for g in guards:
        g.assert_bands_intact()
    ws.guard.assert_bands_intact()
    cx.assert_readonly(entry)
    return {nm: t.clone() for nm, t in outs.items()}


class Worst:
    """Worst distances seen by one test, printed at its end."""

    def __init__(self):
        self.sums, self.grad = 0.0, 0.0

    def __str__(self):
        return f"worst dirty-vs-clean: sums rel {self.sums:.2e}, gradient rel-L2 {self.grad:.2e}"


def grad_is_exact(f, N, entry):
    """The family's rule, or the entry's: pinn_jet_backward launches one workgroup per tile up to W >= CUs workgroups and
    is bit-reproducible while N <= 16 W on the MFMA path (pinn_hip.h), and always on the generic one below 16384 points."""
    if entry == "jet_backward" and f.prec == 0 and f.drop == 0.0 and f.W <= 64:
        return N <= 16 * torch.cuda.get_device_properties(0).multi_processor_count
    return f.grad_exact(N)


def compare(f, N, entry, a, b, worst, tag):
    """Check B / C: outputs `b` (dirty workspace / after a history) against `a` (zero-filled workspace)."""
    assert a.keys() == b.keys()
    for nm in a:
        x, y = a[nm], b[nm]
        assert bool(torch.isfinite(y).all()), (tag, entry, nm, "not finite")
        if nm in POINTWISE:
            assert torch.equal(x, y), (tag, entry, nm, float((x - y).abs().max()))
        elif nm == "grad":
            dist = rel_l2(y, x)
            worst.grad = max(worst.grad, dist)
            if grad_is_exact(f, N, entry):
                assert torch.equal(x, y), (tag, entry, nm, dist)
            else:
                assert dist < 1e-6, (tag, entry, nm, dist)
        else:
            dist = float(((x.double() - y.double()).abs() / x.double().abs().clamp_min(1e-300)).max()) if x.numel() else 0.0
            worst.sums = max(worst.sums, dist if bool((x != y).any()) else 0.0)
            if f.sums_exact:
                assert torch.equal(x, y), (tag, entry, nm, x.tolist(), y.tolist())
            else:
                assert torch.allclose(y, x, rtol=1e-6, atol=0), (tag, entry, nm, x.tolist(), y.tolist())


def make_engine(name):
    eng = Engine(desc_of(FAMILIES[name]))
    eng.dropout_seed = DROP_SEED
    return eng


# ---- A + B: extent and dirty workspace, every family, every entry it serves ---------------------------------------------
@pytest.mark.parametrize("name", list(FAMILIES))
def test_extent_and_dirty_workspace(name):
    f, eng, worst = FAMILIES[name], make_engine(name), Worst()
    spec = spec_of(f)
    for N in f.Ns:
        cx = ctx(name, N)
        for entry in f.entries:
            need = query(eng, ws_kind(entry), N, spec)
            clean = call(eng, cx, entry, WS(need, "zero"))
            dirty = call(eng, cx, entry, WS(need, "poison"))
            compare(f, N, entry, clean, dirty, worst, f"{name} N={N}")
    print(f"ABI {name} Ns={f.Ns} {len(f.entries)} entries: {worst}")


def plain_forward_n():
    """The smallest N at which pinn_fused.hip hands pinn_forward to the four-tiles-per-wave kernel at padded width 32:
    n_tiles >= fused_plain_min_tiles = 4 tiles x 4 waves x 4 workgroups per CU x CUs (pinn_fused_plain.hip)."""
    tiles = 4 * 4 * 4 * torch.cuda.get_device_properties(0).multi_processor_count
    return 16 * (tiles - 1) + 1


def test_plain_forward_four_tiles_per_wave():
    """pinn_forward of CF 3x20 under AUTO at the threshold (last tile: one valid point) and one tile below it (the
    one-tile kernel): extent, dirty workspace, and the same bits from both kernels on the shared points."""
    name = "fields_fused_cf_3x20"
    eng = Engine(desc_of(FAMILIES[name]).with_(engine=ENGINE_AUTO))
    N = plain_forward_n()
    cx = Ctx(name, N)
    need = query(eng, "main", N)
    clean = call(eng, cx, "forward", WS(need, "zero"))
    dirty = call(eng, cx, "forward", WS(need, "poison"))
    assert torch.equal(clean["Y"], dirty["Y"]) and bool(torch.isfinite(dirty["Y"]).all())
    below = call(eng, cx, "forward", WS(need, "poison"), N=N - 16)
    assert torch.equal(below["Y"], clean["Y"][:N - 16])
    print(f"ABI plain forward N={N}: four-tile kernel == one-tile kernel on {N - 16} points, dirty == clean")


# ---- C: history on one workspace -----------------------------------------------------------------------------------------
def history(name, steps, worst):
    """steps: [(entry, N, engine or None)] on ONE engine and ONE workspace per kind (sized for the largest query of the
    sequence, poisoned once before the first call); the last step against the same call on a zero-filled workspace."""
    f, eng = FAMILIES[name], make_engine(name)
    spec = spec_of(f)
    wss = {}
    for kind in {ws_kind(e) for e, _, _ in steps}:
        need = max(query(eng, kind, N, spec, en) for e, N, en in steps if ws_kind(e) == kind)
        wss[kind] = WS(need, "poison")
    last = None
    for entry, N, en in steps:
        last = call(eng, ctx(name, N), entry, wss[ws_kind(entry)], engine=en)
    entry, N, en = steps[-1]
    eng2 = make_engine(name)
    fresh = call(eng2, ctx(name, N), entry, WS(query(eng2, ws_kind(entry), N, spec, en), "zero"), engine=en)
    compare(f, N, entry, fresh, last, worst, f"{name} history {[(e, n) for e, n, _ in steps]}")


def big_n():
    """A larger grid than any later call's: above 16 points x 4 waves x 3 workgroups per CU (tests/test_fields_gpu.py)."""
    return 16 * 4 * 3 * torch.cuda.get_device_properties(0).multi_processor_count + 100


HISTORY_NETS = ["generic_ns5in_3x20", "tile16_ns_3x12", "tile64_ns_2x48", "tile_global_cf_40x20", "coop_co_3x64", "wide128_ns_2x100",
                "bf16_cf_2x128"]


@pytest.mark.parametrize("name", HISTORY_NETS)
def test_history_many_points_then_few(name):
    worst, NB = Worst(), big_n()
    for entry in ("residual_loss_grad", "forward_jet"):
        history(name, [(entry, NB, None), (entry, 17, None)], worst)
    print(f"ABI history big-then-small {name} N={NB}->17: {worst}")


@pytest.mark.parametrize("name", HISTORY_NETS + ["batch_lds_ns_3x12", "batch_atomic_cf_40x20", "dropout_cf_2x48"])
def test_history_gradient_then_loss_only_and_split_then_residual_only(name):
    worst = Worst()
    N = 243 if name.startswith("coop") else 777
    history(name, [("residual_loss_grad", N, None), ("residual_loss", N, None)], worst)
    history(name, [("split", N, None), ("residual_loss_grad", N, None)], worst)
    history(name, [("residual_mse", N, None), ("mse_loss_grad", N, None), ("forward", N, None)], worst)
    print(f"ABI history grad->loss, split->residual {name}: {worst}")


@pytest.mark.parametrize("name", ["tile16_ns_3x12", "tile32_cf_3x32", "tile64_ns_2x48", "tile_global_cf_40x20", "generic_ns5in_3x20"])
def test_history_loss_then_external_adjoint_then_loss(name):
    """pinn_residual_loss_grad, pinn_jet_backward, pinn_residual_loss_grad on one workspace: different epilogues, the
    same packed weights, spill slots and gradient copies."""
    worst = Worst()
    history(name, [("residual_loss_grad", 777, None), ("jet_backward", 777, None), ("residual_loss_grad", 777, None)], worst)
    history(name, [("residual_loss_grad", 777, None), ("fields", 777, None), ("jet_backward", 777, None)], worst)
    print(f"ABI history loss->adjoint->loss {name}: {worst}")


def test_history_bf16_then_fp32_on_a_wide_shape():
    """One workspace, a bf16 call then an fp32 call on the same 2 x 128 network (the two modes carve it differently)."""
    name, N, worst = "bf16_cf_2x128", 777, Worst()
    f = FAMILIES[name]
    spec, cx = spec_of(f), ctx(name, N)
    e16, e32 = make_engine(name), Engine(desc_of(f).with_(precision=0))
    ws = WS(max(query(e16, "main", N), query(e32, "main", N)), "poison")
    call(e16, cx, "residual_loss_grad", ws)
    last = call(e32, cx, "residual_loss_grad", ws)
    fresh = call(Engine(desc_of(f).with_(precision=0)), cx, "residual_loss_grad", WS(query(e32, "main", N), "zero"))
    compare(f, N, "residual_loss_grad", fresh, last, worst, "bf16 -> fp32")
    last = call(e16, cx, "residual_loss_grad", ws)
    fresh = call(make_engine(name), cx, "residual_loss_grad", WS(query(e16, "main", N), "zero"))
    compare(f, N, "residual_loss_grad", fresh, last, worst, "fp32 -> bf16")
    print(f"ABI history bf16 <-> fp32 on 2x128: {worst}")


@pytest.mark.parametrize("name,seq", [
    # (padded width 64 has no batch kernel: BATCH leaves the choice between tile and cooperative to the point count, and
    # 243 points are 16 tiles, fewer than the CUs: the cooperative kernel runs)
    ("coop_co_3x64", (ENGINE_FUSED_TILE, ENGINE_FUSED_COOP, ENGINE_FUSED_BATCH, ENGINE_FUSED_TILE)),
    ("coop_co_3x64", (ENGINE_FUSED_TILE, ENGINE_FUSED_BATCH, ENGINE_FUSED_COOP)),
    # (padded width 16 has no cooperative kernel; the family's figures are the batch kernel's run-to-run ones)
    ("batch_lds_ns_3x12", (ENGINE_FUSED_TILE, ENGINE_FUSED_BATCH, ENGINE_FUSED_TILE)),
    ("batch_lds_ns_3x12", (ENGINE_FUSED_BATCH, ENGINE_FUSED_TILE, ENGINE_FUSED_BATCH)),
], ids=["w64-tile-coop-coop_via_batch-tile", "w64-tile-coop_via_batch-coop", "w12-tile-batch-tile", "w12-batch-tile-batch"])
def test_history_tile_coop_batch_on_one_engine(name, seq):
    """The fused engine's kernels in turn on one engine and one workspace through the engine argument (each packs the
    weights in its own unit order and carves the spill area its own way)."""
    worst = Worst()
    history(name, [("residual_loss_grad", 243, en) for en in seq], worst)
    print(f"ABI history kernels {seq} {name}: {worst}")


# ---- D: += against the fp64 oracle -----------------------------------------------------------------------------------------
def _objectives(name, N, dtype):
    """Flat oracle gradient of what each += entry adds, in `dtype` (CPU autograd)."""
    f, h = FAMILIES[name], host_case(name, N)
    res, inn, outn, gc = f.net
    d = desc_of(f)
    X = h["X"].to(dtype)
    masks = None
    if f.drop > 0:
        masks = [torch.from_numpy(m) for m in keep_masks(DROP_SEED, f.drop, f.L, f.W, N)]
    fresh = lambda: [q.to(dtype).clone().requires_grad_(True) for q in h["params"]]
    out = {}

    def mse(p, Xs, T, cs, mk):
        Y = O.mlp_forward(p, Xs, h["init"], mk, f.drop)
        return sum(cs[j].to(dtype) * ((T[:, j].to(dtype) - Y[:, o]) ** 2).sum() for j, o in enumerate(h["out_col"]))

    def resid(p, Xs, mk):
        _, out_roles, dir_roles = RESIDUAL_ROLES[res]
        # the oracle returns sum_t mean_t: host_case sets the entries' term scales to those means' 1 / count
        return O.residual_loss(p, Xs, res, [inn.index(r) for r in dir_roles], [outn.index(r) for r in out_roles], gc, h["init"], mk, f.drop)
    if res and any(e in f.entries for e in ("residual_loss_grad", "residual_mse", "split")):
        p = fresh(); out["residual_loss_grad"] = O.flat_grad(resid(p, X, masks), p)
        p = fresh(); out["mse_loss_grad"] = O.flat_grad(mse(p, X, h["T"], h["cs"], masks), p)
        out["residual_mse"] = out["residual_loss_grad"] + out["mse_loss_grad"]
        if "split" in f.entries:
            nr = h["n_res"]
            m_res = m_fid = None
            if f.drop > 0:      # two passes: the fidelity points' mask index restarts at 0 (the family's comment)
                m_res = [mk[:nr] for mk in masks]
                m_fid = [torch.from_numpy(mk) for mk in keep_masks(DROP_SEED, f.drop, f.L, f.W, N - nr)]
            p = fresh(); a = O.flat_grad(resid(p, X[:nr], m_res), p)
            p = fresh(); b = O.flat_grad(mse(p, X[nr:], h["T"][nr:], h["cs_split"], m_fid), p)
            out["split"] = a + b
    if "jet_backward" in f.entries or "jet2_backward" in f.entries:
        p = fresh()
        cols = O.split_columns(X, gc)
        Y = O.mlp_forward(p, torch.cat(cols, -1), h["init"])
        dcol = lambda T_, j: torch.cat([O.compute_gradient(T_[:, c:c + 1], cols[j]) for c in range(d.d_out)], 1)
        dY = [dcol(Y, j) for j in gc]
        obj = (Y * h["gY"].to(dtype)).sum() + (torch.stack(dY) * h["gdY"].to(dtype)).sum()
        if "jet2_backward" in f.entries:
            d2Y = torch.stack([dcol(dY[i], gc[j]) for i in range(d.k) for j in range(i, d.k)])
            obj = obj + (d2Y * h["gd2Y"].to(dtype)).sum()
            out["jet2_backward"] = O.flat_grad(obj, p)
        else:
            out["jet_backward"] = O.flat_grad(obj, p)
    return out


@functools.lru_cache(maxsize=None)
def oracle_grads(name, N):
    g64, g32 = _objectives(name, N, torch.float64), _objectives(name, N, torch.float32)
    return {e: (g64[e], rel_l2(g32[e], g64[e])) for e in g64}


def permuted_within_layers(g, desc, seed):
    """A seeded permutation of g inside each layer's block [W_l, b_l]: the answer's magnitudes, not a multiple of it."""
    gen, out, off = torch.Generator().manual_seed(seed), g.clone(), 0
    ls = desc.layers
    for i in range(len(ls) - 1):
        n = ls[i] * ls[i + 1] + ls[i + 1]
        out[off:off + n] = g[off:off + n][torch.randperm(n, generator=gen).to(g.device)]
        off += n
    assert off == g.numel()
    return out


@pytest.mark.parametrize("name", [n for n, f in FAMILIES.items() if any(e in GRAD_ENTRIES for e in f.entries)])
def test_grad_is_accumulated_onto_what_the_caller_left_there(name):
    f, eng = FAMILIES[name], make_engine(name)
    N, spec = f.n_D, spec_of(f)
    cx, ref = ctx(name, N), oracle_grads(name, N)
    worst = 0.0
    for entry in [e for e in f.entries if e in GRAD_ENTRIES]:
        need = query(eng, ws_kind(entry), N, spec)
        clean = call(eng, cx, entry, WS(need, "zero"))["grad"]
        g0 = permuted_within_layers(clean, eng.desc, seed=N + len(entry))
        assert not torch.equal(g0, clean)
        after = call(eng, cx, entry, WS(need, "poison"), grad0=g0)["grad"]
        added = after.double() - g0.double()
        g64, gnoise = ref[entry]
        bar = f.oracle_bar if f.oracle_bar is not None else max(2e-5, 4 * gnoise)
        dist = rel_l2(added.cpu(), g64)
        worst = max(worst, dist / bar)
        # ... and against the engine's own gradient on a zeroed grad: run-to-run 1e-6 (check B) plus the rounding of the
        # final fp32 additions onto g0, 2^-24 (|g0| + |g|) per element and |g0| = |g| as vectors: 1e-6 + 4 * 2^-24.  This
        # is the sharp form of the check for the bf16 families, whose oracle bar is wide.
        own, own_bar = rel_l2(added, clean.double()), 1e-6 + 4 * 2.0 ** -24
        print(f"ABI += {name} {entry} N={N}: rel-L2(grad_after - g0, fp64 oracle) {dist:.2e} (bar {bar:.2e}, oracle fp32 noise {gnoise:.2e}); "
              f"against its own clean gradient {own:.2e} (bar {own_bar:.2e})")
        assert dist < bar, (name, entry, dist, bar)
        assert own < own_bar, (name, entry, own, own_bar)
    print(f"ABI += {name}: worst distance / bar {worst:.3f}")


def test_n_zero_leaves_grad_alone_and_zeroes_the_sums():
    """The five N = 0 early returns of pinn_abi.hip (residual_impl: two entries, pinn_mse_loss_grad, residual_mse_impl:
    two entries): grad untouched bit for bit, the sums zeroed, nothing else written."""
    name = "tile32_cf_3x32"
    for engine in (ENGINE_FUSED_TILE, ENGINE_GENERIC):
        eng = Engine(desc_of(FAMILIES[name]).with_(engine=engine))
        cx = ctx(name, 17)
        g0 = torch.linspace(-3, 3, eng.n_params, device="cuda")
        snap = snapshot(g0)
        for entry in LOSS:
            ws = WS(query(eng, "main", 1), "poison")
            r = call(eng, cx, entry, ws, grad0=g0, N=0, n_res=0)
            for nm in ("term_sums", "col_sums"):
                if nm in r:
                    assert float(r[nm].abs().max()) == 0.0, (entry, nm, r[nm].tolist())
            if "grad" in r:
                assert_unchanged(r["grad"], snap, f"grad ({entry}, N = 0)")
            assert bool((ws.t.view(torch.float32) == POISON).all()), (entry, "workspace written at N = 0")
    print("ABI N = 0: five entries x two engines: grad untouched, sums zero, workspace untouched")


# ---- the two Adam entries: grad, sums and losses overwritten; packed weights across calls ------------------------------
def adam_call(eng, cx, ws, params, m, v, step, lrs, packed_valid, pre, n_res, with_cols, loop):
    """pinn_loss_grad_adam_step (loop False: lrs has one entry) or pinn_adam_loop on guarded m, v, grad, sums, losses.
    pre: value grad / term_sums / col_sums / losses hold on entry.  Returns the outputs (params, m, v updated copies)."""
    f, lib = cx.f, eng.lib
    spec = spec_of(f)
    nP, N, nt = eng.n_params, cx.N, spec.n_terms
    nc = len(cx.out_col) if with_cols else 0
    assert n_res == (-1 if with_cols else N)          # residual only, or both terms on every point
    n_it, n_rows = len(lrs), 2
    outs, guards = {}, []

    def buf(nm, shape, src=None, fill=None):
        t, g = guarded(shape, torch.float32, "cuda", fill=fill, name=f"{nm} of adam")
        if src is not None:
            t.copy_(src)
        outs[nm] = t
        guards.append(g)
        return t
    th, mm, vv = buf("params", (nP,), params), buf("m", (nP,), m), buf("v", (nP,), v)
    grad, ts = buf("grad", (nP,), fill=pre), buf("term_sums", (nt,), fill=pre)
    cs = buf("col_sums", (max(nc, 1),), fill=pre)[:nc]
    losses = buf("losses", (n_it, n_rows), fill=pre)
    rows = torch.tensor([[0.5] * nc + [1.0] * nt, [1.0] * nc + [0.0] * nt], device="cuda")
    rows_snap = snapshot(rows)
    st = PinnAdamState(_ptr(mm), _ptr(vv), step, float(lrs[0]), 0.9, 0.999, 1e-8, 1 if packed_valid else 0, n_rows, _ptr(rows), _ptr(losses))
    head = (C.byref(eng._d()), C.byref(spec.c_struct()), _ptr(cx.ts),
            _ptr(cx.T) if nc else None, nc, cx.oc, _ptr(cx.cs) if nc else None,
            _ptr(th), _ptr(cx.X), N, n_res, _ptr(ts), _ptr(cs) if nc else None, _ptr(grad), C.byref(st))
    with torch.cuda.device(eng._index()):
        tail = (_ptr(ws.t), ws.bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if loop:
            rc = lib.pinn_adam_loop(*head, n_it, (C.c_double * n_it)(*lrs), *tail)
        else:
            rc = lib.pinn_loss_grad_adam_step(*head, *tail)
    check(rc, "adam entry")
    torch.cuda.synchronize()
    for g in guards:
        g.assert_bands_intact()
    ws.guard.assert_bands_intact()
    cx.assert_readonly("adam")
    assert_unchanged(rows, rows_snap, "loss_rows")
    r = {nm: t.clone() for nm, t in outs.items()}
    r["col_sums"] = r["col_sums"][:nc]
    return r


ADAM_CASES = {"step_coop_co_3x64": ("coop_co_3x64", ENGINE_AUTO, 243, False), "loop_cf_3x32": ("tile32_cf_3x32", ENGINE_AUTO, 777, True)}


def _adam_setup(case):
    name, engine, N, loop = ADAM_CASES[case]
    f = FAMILIES[name]
    eng = Engine(desc_of(f).with_(engine=engine))
    cx = ctx(name, N)
    z = torch.zeros(eng.n_params, device="cuda")
    lrs = [1e-3, 8e-4, 6e-4] if loop else [1e-3]
    return f, eng, cx, z, lrs, loop


ONE_PASS = ("term_sums", "col_sums", "losses", "grad", "m", "v")


def _adam_pair(eng, cx, need, lrs, n_res, cols, loop):
    z = torch.zeros(eng.n_params, device="cuda")
    a = adam_call(eng, cx, WS(need, "zero"), cx.flat, z, z, 1, lrs, False, 0.0, n_res, cols, loop)
    b = adam_call(eng, cx, WS(need, "poison"), cx.flat, z, z, 1, lrs, False, POISON, n_res, cols, loop)
    for nm in ONE_PASS + ("params",):
        assert bool(torch.isfinite(b[nm]).all()), (nm, "not finite")
    assert float(a["term_sums"].abs().max()) > 0
    return a, b


def _adam_distances(a, b):
    d = {nm: rel_l2(b[nm], a[nm]) for nm in ("grad", "m", "v")}
    for nm in ("term_sums", "col_sums", "losses"):
        x, y = a[nm].double().reshape(-1), b[nm].double().reshape(-1)
        d[nm] = float(((x - y).abs() / x.abs().clamp_min(1e-300)).max()) if x.numel() else 0.0
    return d


@pytest.mark.parametrize("case", list(ADAM_CASES))
def test_adam_entries_overwrite_grad_sums_and_losses(case):
    """grad, term_sums, col_sums and losses full of 1e30 on entry, workspace poisoned, against the run that found zeros.
    One iteration (pinn_loss_grad_adam_step, and pinn_adam_loop with n_iters = 1) is one pass on the same parameters:
    every output at check B's figures, sums rtol 1e-6, grad / m / v rel-L2 < 1e-6.
    Three iterations of pinn_adam_loop: iteration 0's losses at 1e-6; what later iterations leave (the last iteration's
    sums and grad, m, v, losses[1:]) starts from parameters the two runs no longer share to the bit, so it is held to the
    figures tests/test_sweep_gpu.py:260-264 applies to a folded run against another run of the same iterations: sums and
    losses rtol 1e-5, grad / m / v rel-L2 < 5e-6, parameters in units of the step."""
    f, eng, cx, z, lrs, loop = _adam_setup(case)
    need, worst = query(eng, "main", cx.N), Worst()
    for n_res, cols in ((cx.N, False), (-1, True)):
        a, b = _adam_pair(eng, cx, need, lrs[:1], n_res, cols, loop)
        d = _adam_distances(a, b)
        print(f"ABI adam overwrite {case} cols={cols} one iteration: " + " ".join(f"{k} {v:.2e}" for k, v in d.items()))
        worst.grad, worst.sums = max(worst.grad, d["grad"], d["m"], d["v"]), max(worst.sums, d["term_sums"], d["col_sums"], d["losses"])
        for nm in ("term_sums", "col_sums", "losses"):
            assert torch.allclose(b[nm], a[nm], rtol=1e-6, atol=0), (nm, a[nm], b[nm])
        for nm in ("grad", "m", "v"):
            assert d[nm] < 1e-6, (nm, d[nm])
        assert float((a["params"] - b["params"]).abs().max()) < 1.025 * lrs[0]
        assert float((a["params"] - b["params"]).norm() / (a["params"] - cx.flat).norm()) < 2e-2
        if not loop:
            continue
        a, b = _adam_pair(eng, cx, need, lrs, n_res, cols, True)
        d = _adam_distances(a, b)
        print(f"ABI adam overwrite {case} cols={cols} {len(lrs)} iterations: " + " ".join(f"{k} {v:.2e}" for k, v in d.items()))
        worst.grad, worst.sums = max(worst.grad, d["grad"], d["m"], d["v"]), max(worst.sums, d["term_sums"], d["col_sums"], d["losses"])
        assert torch.allclose(b["losses"][0], a["losses"][0], rtol=1e-6, atol=0), (a["losses"], b["losses"])
        for nm in ("term_sums", "col_sums", "losses"):
            assert torch.allclose(b[nm], a[nm], rtol=1e-5, atol=0), (nm, a[nm], b[nm])
        for nm in ("grad", "m", "v"):
            assert d[nm] < 5e-6, (nm, d[nm])
        assert float((a["params"] - b["params"]).abs().max()) < 1.025 * sum(lrs)
        assert float((a["params"] - b["params"]).norm() / (a["params"] - cx.flat).norm()) < 2e-2
    print(f"ABI adam overwrite {case}: {worst}")


@pytest.mark.parametrize("case", list(ADAM_CASES))
def test_history_adam_step_then_a_plain_call_with_other_params(case):
    """The folded step leaves ITS updated parameters packed in the workspace; a plain loss call on the same workspace
    with different params must pack its own."""
    f, eng, cx, z, lrs, loop = _adam_setup(case)
    name = ADAM_CASES[case][0]
    need = query(eng, "main", cx.N)
    ws, worst = WS(need, "poison"), Worst()
    adam_call(eng, cx, ws, cx.flat * 1.5, z, z, 1, lrs, False, POISON, cx.N, False, loop)
    last = call(eng, cx, "residual_loss_grad", ws)
    fresh = call(Engine(eng.desc), cx, "residual_loss_grad", WS(need, "zero"))
    compare(f, cx.N, "residual_loss_grad", fresh, last, worst, "adam -> plain")
    last = call(eng, cx, "forward_jet", ws)
    fresh = call(Engine(eng.desc), cx, "forward_jet", WS(need, "zero"))
    compare(f, cx.N, "forward_jet", fresh, last, worst, "adam -> plain forward")
    print(f"ABI history adam -> plain {case} ({name}): {worst}")


@pytest.mark.parametrize("case", list(ADAM_CASES))
def test_history_adam_twice_with_packed_valid_against_the_unfolded_calls(case):
    """Two folded steps, the second with packed_valid = 1 (it reads the packed weights the first one refreshed, padding
    included), on a poisoned workspace, against loss call + pinn_adam_step twice."""
    f, eng, cx, z, lrs, loop = _adam_setup(case)
    need, nP = query(eng, "main", cx.N), eng.n_params
    ws = WS(need, "poison")
    a = adam_call(eng, cx, ws, cx.flat, z, z, 1, lrs[:1], False, POISON, cx.N, False, False)
    a = adam_call(eng, cx, ws, a["params"], a["m"], a["v"], 2, lrs[:1], True, POISON, cx.N, False, False)
    th, m, v = cx.flat.clone(), z.clone(), z.clone()
    ws2 = WS(need, "zero")
    for step in (1, 2):
        r = call(eng, cx, "residual_loss_grad", ws2, params=th)
        eng.adam_step(th, r["grad"].contiguous(), m, v, step, lrs[0])
    torch.cuda.synchronize()
    gdist, mdist, vdist = rel_l2(a["grad"], r["grad"]), rel_l2(a["m"], m), rel_l2(a["v"], v)
    print(f"ABI adam x2 packed_valid {case}: grad {gdist:.2e} m {mdist:.2e} v {vdist:.2e} "
          f"params max {float((a['params'] - th).abs().max()):.2e}")
    assert torch.allclose(a["term_sums"], r["term_sums"], rtol=1e-5)
    # Adam's first steps move every parameter by ~lr whatever the gradient's size: in units of the step (tests/test_sweep_gpu.py:259-265)
    assert float((a["params"] - th).abs().max()) < 2.05 * lrs[0]
    assert float((a["params"] - th).norm() / (th - cx.flat).norm()) < 2e-2
    assert gdist < 5e-6          # folded against unfolded gradient: the figure of tests/test_sweep_gpu.py:260
    assert mdist < 1e-6 and vdist < 1e-6


# ---- L-BFGS and staging ------------------------------------------------------------------------------------------------------
def test_lbfgs_push_and_direction_extents():
    """m = 8, P = 1000: push writes row `slot` of S, Y and row + column `slot` of M, nothing else; direction writes d,
    tmp, coef, q inside their extents and reads S, Y, M, g only; dirty scratch gives the same d."""
    lib, m, P = L_.load(), 8, 1000
    gen = torch.Generator().manual_seed(3)
    f32 = lambda nm, shape, fill=None: guarded(shape, torch.float32, "cuda", fill=fill, name=nm)
    S, gS = f32("S", (m, P), 0.0)
    Y, gYy = f32("Y", (m, P), 0.0)
    M, gM = guarded((m, m), torch.float64, "cuda", fill=0.0, name="M")
    k = 5
    for slot in range(k):
        s, y = torch.randn(P, generator=gen).cuda(), torch.randn(P, generator=gen).cuda()
        y = 0.5 * s + 0.1 * y
        snaps = (snapshot(s), snapshot(y), snapshot(S), snapshot(Y), snapshot(M))
        check(lib.pinn_lbfgs_push(_ptr(S), _ptr(Y), _ptr(M), m, P, slot, _ptr(s), _ptr(y), None), "pinn_lbfgs_push")
        torch.cuda.synchronize()
        for g in (gS, gYy, gM):
            g.assert_bands_intact()
        assert_unchanged(s, snaps[0], "s"); assert_unchanged(y, snaps[1], "y")
        rows = [r for r in range(m) if r != slot]
        assert_unchanged(S[rows], snapshot(snaps[2].view(torch.int32).view(m, P)[rows]), "S rows other than slot")
        assert_unchanged(Y[rows], snapshot(snaps[3].view(torch.int32).view(m, P)[rows]), "Y rows other than slot")
        assert torch.equal(S[slot], s) and torch.equal(Y[slot], y)
        Mb, Ma = snaps[4].view(m, m), snapshot(M).view(m, m)
        keep = torch.ones(m, m, dtype=torch.bool, device="cuda"); keep[slot, :] = False; keep[:, slot] = False
        assert torch.equal(Mb[keep], Ma[keep]), "M outside row / column slot"
    g = torch.randn(P, generator=gen).cuda()
    H = float(Y[k - 1].double().dot(S[k - 1].double()) / Y[k - 1].double().dot(Y[k - 1].double()))
    ds = []
    for fill in (0.0, POISON):
        d, gd = f32("d", (P,))
        tmp, gt = guarded((4 * m,), torch.float64, "cuda", fill=fill, name="tmp")
        coef, gc = f32("coef", (2 * m,), fill)
        q, gq = f32("q", (P,), fill)
        Md = M.clone() if fill == 0.0 else None
        if Md is None:
            Md, gM2 = guarded((m, m), torch.float64, "cuda", name="M (unused entries poisoned)")
            Md[:k, :k] = M[:k, :k]
        ro = dict(S=S, Y=Y, M=Md, g=g)
        snaps = {nm: snapshot(t) for nm, t in ro.items()}
        check(lib.pinn_lbfgs_direction(_ptr(S), _ptr(Y), _ptr(Md), m, P, 0, k, _ptr(g), H, _ptr(d), _ptr(tmp), _ptr(coef), _ptr(q), None),
              "pinn_lbfgs_direction")
        torch.cuda.synchronize()
        for gg in (gd, gt, gc, gq, gS, gYy, gM) + ((gM2,) if fill else ()):
            gg.assert_bands_intact()
        for nm, t in ro.items():
            assert_unchanged(t, snaps[nm], nm)
        ds.append(d.clone())
    ref = O.lbfgs_two_loop(S[:k].cpu(), Y[:k].cpu(), g.cpu(), H)
    print(f"ABI lbfgs m=8 P=1000 k=5: direction rel-L2 vs fp64 two-loop {rel_l2(ds[0].cpu(), ref):.2e}, poisoned == clean: {torch.equal(ds[0], ds[1])}")
    assert torch.equal(ds[0], ds[1]) and bool(torch.isfinite(ds[1]).all())
    assert rel_l2(ds[0].cpu(), ref) < LBFGS_BAR


def test_staging_extents():
    """pinn_nanminmax_f64 and pinn_stage_grid_columns on a 9 x 7 grid with NaNs, intervals (2, 3): out2, X_out (band behind
    its full capacity of ceil(ny/ix) ceil(nx/iy) rows), the int64 row count and the workspace inside guard bands; grids
    and minmax read-only; dirty workspace gives the same rows; the rows are the host path's."""
    lib = L_.load()
    ny, nx, ix, iy, d_in = 9, 7, 2, 3, 2
    gen = torch.Generator().manual_seed(5)
    grids = [torch.rand(ny, nx, generator=gen, dtype=torch.float64) * 10 - 3 for _ in range(d_in)]
    grids[0][0, 0] = float("nan"); grids[1][2, 3] = float("nan"); grids[0][8, 6] = float("nan"); grids[1][5, 1] = float("nan")
    gd = [t.cuda().contiguous() for t in grids]
    mm, gmm = guarded((d_in, 2), torch.float64, "cuda", name="minmax")
    for c in range(d_in):
        for mode in ("zero", "poison"):
            n = ny * nx
            # (no query call exists for this entry: the size is the check of pinn_ingest.hip, pinn_nanminmax_f64 —
            # nb = min(n / 256 + 1, 1024) blocks x 16 bytes; if that formula grows, this line follows it)
            ws = WS(min(n // 256 + 1, 1024) * 16, mode)
            out2, go = guarded((2,), torch.float64, "cuda", name="out2")
            snap = snapshot(gd[c])
            check(lib.pinn_nanminmax_f64(_ptr(gd[c]), n, _ptr(out2), _ptr(ws.t), ws.bytes, None), "pinn_nanminmax_f64")
            torch.cuda.synchronize()
            go.assert_bands_intact(); ws.guard.assert_bands_intact(); assert_unchanged(gd[c], snap, "data")
            assert out2.tolist() == [float(np.nanmin(grids[c].numpy())), float(np.nanmax(grids[c].numpy()))]
            mm[c] = out2
    cap = -(-ny // ix) * -(-nx // iy)
    need = lib.pinn_stage_workspace_bytes(ny, nx, ix, iy)
    ptrs = (C.c_void_p * d_in)(*[t.data_ptr() for t in gd])
    got = []
    for mode in ("zero", "poison"):
        ws = WS(need, mode)
        X_out, gx = guarded((cap, d_in), torch.float32, "cuda", name="X_out")
        n_rows, gn = guarded((1,), torch.int64, "cuda", name="n_rows_out")
        snaps = [snapshot(t) for t in gd] + [snapshot(mm)]
        check(lib.pinn_stage_grid_columns(ptrs, d_in, ny, nx, ix, iy, _ptr(mm), _ptr(X_out), _ptr(n_rows), _ptr(ws.t), ws.bytes, None),
              "pinn_stage_grid_columns")
        torch.cuda.synchronize()
        for g in (gx, gn, gmm, ws.guard):
            g.assert_bands_intact()
        for t, s in zip(gd + [mm], snaps):
            assert_unchanged(t, s, "grids / minmax")
        got.append(X_out[:int(n_rows.item())].clone())
    # the host path: subsample, normalise, column-major flatten, drop NaN rows (train.py:260-277)
    cols = []
    for c in range(d_in):
        sub = grids[c].numpy()[::ix, ::iy]
        lo, hi = np.nanmin(grids[c].numpy()), np.nanmax(grids[c].numpy())
        cols.append((2 * (sub - lo) / (hi - lo) - 1).T.reshape(-1, 1))
    want = np.concatenate(cols, 1)
    want = torch.from_numpy(want[~np.isnan(want).any(1)]).float()
    assert 0 < want.shape[0] < cap
    assert torch.equal(got[0].cpu(), want) and torch.equal(got[0], got[1])
    print(f"ABI staging 9x7 / (2, 3): {want.shape[0]} of {cap} rows, dirty == clean")
