"""Every kernel family at states with NON-ZERO hidden biases (tests/trained_state_util.py), each parameter block (W_l, b_l)
held to the bound on its own, against the fp64 oracle on the CPU.

Why: init_params leaves every hidden bias at exactly zero and every other parity test starts there, so a kernel that
dropped a hidden bias, read the neighbouring unit's, another layer's or another ensemble member's passed the suite; and the
whole-vector rel-L2 of the gradient checks lets a bias block (about 1e-2 of the norm) be 0.2 % wrong.
tests/test_trained_state_cpu.py shows on the reference side that the comparisons used here reject such mis-readings.

Bounds (none of them taken from what the kernels give):
  gradient   per block max(2e-5, 4 x the oracle's own fp32-vs-fp64 gap in that block); the gap itself must be <= 5e-6
  loss       max(2e-6, 4 x the oracle's fp32 noise), relative               (tests/test_engine_gpu.py)
  Y, dY, d2Y 2e-6 max(1, max|ref|), absolute                                (tests/test_engine_gpu.py)
  fields     per field 4 x max(oracle fp32 noise, 2^-23 max|f|)             (tests/test_fields_gpu.py)
  bf16 mode  term sums 3e-2 relative, gradient 1e-1 per block               (tests/test_sweep_gpu.py's bounds for the mode)
  folded Adam: in units of the step, as tests/test_sweep_gpu.py: max|theta - theta_ref| < 1.025 x iterations x lr and
             |theta - theta_ref| / |theta_ref - theta_0| < 2e-2; the SECOND iteration's gradient per block against the
             oracle at the parameters the first iteration left on the device.
Engines are forced through NetDesc.with_(engine=...).  N = 777 (ragged for every tile size) unless stated (the plain forward's
four-tiles-per-wave kernel: 150 001 / 300 001 points).

bf16 mode carries 8 significant bits: the 1e-1 block bound catches a layer's biases dropped or shifted (measured on the
oracle for 3x128: every block off by >= 4.5e-1) but NOT a single unit's bias (1e-2); the fp32 cases of the same shapes do.

Measured on an MI355X (every test prints its own line under `pytest -s`; the MFMA kernels' figures move in the second
digit from run to run with the order of their atomic adds).  Largest per-block gradient error per family,
generic kernels / MFMA kernels, with the block and the oracle's own fp32-vs-fp64 gap in that block:
  loss + gradient, biased      1.1e-6 (co_3x64 W2, gap 1.2e-7)    / 6.3e-7 (cf_40x20 tile b8, gap 7.7e-8)
  loss + gradient, saturating  9.8e-7 (co_3x64 W3, gap 4.3e-7)    / 6.2e-7 (ns_3x12 batch W0, gap 6.3e-7)
  fidelity columns, split      8.7e-7 (pe_10x10 one pass W10)     / 1.7e-7 (pe_10x10 split batch W0, gap 2.6e-7)
  LeakyReLU / Kaiming          5.8e-7 (W2, gap 1.0e-7)            / 2.2e-7 (b0, gap 7.6e-8)
  jet_backward                 1.6e-6 (pe_10x10 W2, gap 7.8e-7)   / 1.0e-6 (pe_10x10 tile b2, gap 1.4e-6)
  corrected radiation stress   8.9e-7 (10x10 W6, gap 3.2e-7)      / 1.9e-7 (10x10 tile b6, gap 1.6e-7)
  ensemble, M = 3                                                   7.9e-7 (co40x20_both member 1 b0, gap 1.1e-6)
  wide engine, fp32 mode                                            2.6e-7 (co_2x100 W0, gap 4.0e-7)
  wide engine, bf16 mode                                            2.9e-4 (5x256 b0; 3x128: 2.5e-4 in b3); term sums 8.0e-4
  second order (nu = 0.1)      8.1e-7 (ns_8x64 W1, gap 1.7e-7)    / 2.8e-7 (pe_10x10 b4, gap 1.4e-7)
  dropout instance (p = 0.3)   7.5e-7 (W4, gap 2.6e-7)            / 2.8e-7 (tile W2, gap 3.4e-7)
  folded Adam, 2nd iteration                                        1.1e-6 (pe_10x10 b9, gap 1.3e-6)
Nothing lands between the reference's noise and the bound: every fp32 block is within about 10 x the oracle's own fp32
gap and 12 x or more under the 2e-5 bound, at the saturating state too (11-40 % of the last hidden activations above 0.99).
Losses are within 3.7e-7 (bound 2e-6), Y / dY / d2Y within 1.1e-6 / 3.1e-6 of 4.8e-6 / 8.6e-6 (cf_3x32 saturating, the
largest; the plain forward on k_fused_plain4 within 4.9e-7 of 2.0e-6), the parameters after two folded Adam iterations
within 5e-8 (5e-5 of a step) of the fp64 trajectory.
"""
import functools

import pytest
import torch

from oracle import pinn_oracle as O
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec
from pinn_depthestimation_amd._lib import (ACT_LEAKY_RELU, ENGINE_AUTO, ENGINE_FUSED, ENGINE_FUSED_BATCH, ENGINE_FUSED_COOP,
                                           ENGINE_FUSED_TILE, ENGINE_GENERIC, ENGINE_WIDE, PREC_BF16)
from tests import pe_corrected_util as PC
from tests import residual2_util as R2
from tests import trained_state_util as U
from tests.dropout_util import keep_masks

pytestmark = pytest.mark.gpu

ENG = {"generic": ENGINE_GENERIC, "tile": ENGINE_FUSED_TILE, "coop": ENGINE_FUSED_COOP, "batch": ENGINE_FUSED_BATCH,
       "fused": ENGINE_FUSED, "wide": ENGINE_WIDE, "auto": ENGINE_AUTO}
N = U.N_POINTS


def engines_for(width):
    """The engines that serve a loss + gradient request at this hidden width."""
    if width > 64:
        return ["wide", "auto"]
    return ["generic", "tile", "coop" if width > 32 else "batch", "auto"]


def report(family, what, errs, g64, g32, layers, extra=""):
    k, e = U.worst(errs)
    gap = U.block_errors(g32, g64, layers)[k]
    print(f"TRAINED {family} | {what}: worst block {k} {e:.2e} (oracle fp32 gap there {gap:.1e}){extra}")


def dev(case, params=None):
    return O.flatten(case.params if params is None else params).cuda(), case.X.cuda().contiguous()


# ---- a. loss + gradient (and g: the wide engine in fp32 mode) --------------------------------------------------------------
LOSS_GRAD = [(n, s, e) for n, s in U.LOSS_GRAD for e in engines_for(U.CASES[n][3])]


@pytest.mark.parametrize("name,state,tag", LOSS_GRAD, ids=[f"{n}-{s}-{e}" for n, s, e in LOSS_GRAD])
def test_loss_and_gradient(name, state, tag):
    c, l64, g64, l32, g32 = U.reference(name, state)
    eng, spec = Engine(c.desc(engine=ENG[tag])), c.spec()
    flat, Xd = dev(c)
    scale = c.term_scale().cuda()
    grad = torch.zeros(eng.n_params, device="cuda")
    sums = eng.residual_loss_grad(spec, scale, flat, Xd, grad)
    sums_only = eng.residual_loss(spec, flat, Xd)
    assert torch.allclose(sums, sums_only, rtol=1e-6, atol=0), (sums, sums_only)
    if c.res == "continuity_only":
        assert float(sums[2]) == float((c.X[:, 0] < 25.5).sum())
    loss = float((sums.cpu().double() * scale.cpu().double()).sum())
    el = abs(loss - l64) / abs(l64)
    print(f"TRAINED loss | {name} {state} {tag}: loss off by {el:.2e} (bound {U.loss_bound(l64, l32):.1e})")
    errs = U.assert_blocks_close(grad, g64, g32, c.layers, f"{name} {state} {tag}")
    report("wide fp32" if c.W > 64 else f"loss+grad {state}", f"{name} {tag}", errs, g64, g32, c.layers, f" loss {el:.1e}")
    assert el < U.loss_bound(l64, l32), (name, state, tag, loss, l64)


# ---- b. one pass with fidelity columns, and the split request ---------------------------------------------------------------
FID_W = [0.7, 1.3, 2.0]
N_RES_SPLIT = 700      # the boundary falls inside a 16-point tile (700 = 43 * 16 + 12); 77 fidelity points


@functools.lru_cache(maxsize=None)
def fidelity_reference(name, kind):
    c = U.Case(name, "biased")
    n_fid = N if kind == "onepass" else N - N_RES_SPLIT
    T = torch.rand(n_fid, 3, generator=torch.Generator().manual_seed(11))
    n_res = None if kind == "onepass" else N_RES_SPLIT
    l64, g64 = U.oracle_total(c, torch.float64, n_res=n_res, T=T, cols=(0, 1, 2), weights=FID_W)
    l32, g32 = U.oracle_total(c, torch.float32, n_res=n_res, T=T, cols=(0, 1, 2), weights=FID_W)
    return c, T, l64, g64, l32, g32


FID = [(n, k, e) for n in ("pe_10x10", "ns_8x64") for k in ("onepass", "split") for e in engines_for(U.CASES[n][3])]


@pytest.mark.parametrize("name,kind,tag", FID, ids=[f"{n}-{k}-{e}" for n, k, e in FID])
def test_fidelity_columns_in_the_same_pass(name, kind, tag):
    c, T, l64, g64, l32, g32 = fidelity_reference(name, kind)
    eng, spec = Engine(c.desc(engine=ENG[tag])), c.spec()
    flat, Xd = dev(c)
    n_res = N if kind == "onepass" else N_RES_SPLIT
    ts = torch.full((spec.n_terms,), 1.0 / n_res).cuda()
    cs = (torch.tensor(FID_W) / T.shape[0]).cuda()
    grad = torch.zeros(eng.n_params, device="cuda")
    if kind == "onepass":
        t_sums, c_sums = eng.residual_mse_loss_grad(spec, ts, T.cuda(), [0, 1, 2], cs, flat, Xd, grad)
    else:
        t_sums, c_sums = eng.residual_mse_split_loss_grad(spec, ts, T.cuda(), [0, 1, 2], cs, flat, Xd, n_res, grad)
    loss = float((t_sums.double() * ts.double()).sum() + (c_sums.double() * cs.double()).sum())
    el = abs(loss - l64) / abs(l64)
    errs = U.assert_blocks_close(grad, g64, g32, c.layers, f"{name} {kind} {tag}")
    report("fidelity", f"{name} {kind} {tag}", errs, g64, g32, c.layers, f" loss {el:.1e}")
    assert el < U.loss_bound(l64, l32), (name, kind, tag, loss, l64)


# ---- c. forward and forward_jet ---------------------------------------------------------------------------------------------
# (no "batch": the batch kernel has gradient passes only, a forced FUSED_BATCH forward runs the tile kernel again)
FWD = [(n, s, e) for n, s in (("ns_8x64", "biased"), ("pe_10x10", "biased"), ("cf_3x32", "biased"), ("cf_3x32", "saturating"))
       for e in engines_for(U.CASES[n][3]) if e != "batch"]


@functools.lru_cache(maxsize=None)
def jet_reference(name, state):
    c = U.Case(name, state)
    Yo, dYo = O.jet([p.double() for p in c.params], c.X.double(), c.gc)
    return c, Yo, dYo


@pytest.mark.parametrize("name,state,tag", FWD, ids=[f"{n}-{s}-{e}" for n, s, e in FWD])
def test_forward_and_jet(name, state, tag):
    c, Yo, dYo = jet_reference(name, state)
    eng = Engine(c.desc(engine=ENG[tag]))
    flat, Xd = dev(c)
    Y = eng.forward(flat, Xd)
    Yj, dY = eng.forward_jet(flat, Xd)
    ey, eyj, ed = [float((a.cpu().double() - b).abs().max()) for a, b in ((Y, Yo), (Yj, Yo), (dY, dYo))]
    print(f"TRAINED forward | {name} {state} {tag}: Y {ey:.1e} / {eyj:.1e} (bound {U.abs_bound(Yo):.1e}), dY {ed:.1e} (bound {U.abs_bound(dYo):.1e})")
    assert ey < U.abs_bound(Yo) and eyj < U.abs_bound(Yo) and ed < U.abs_bound(dYo)


# (d_in, d_out, hidden layers, width, points, whether AUTO / FUSED run k_fused_plain4 there)
PLAIN = {
    "3x20_150001": (5, 4, 3, 20, 150001, False),     # below the rule for padded width 32: the one-tile kernel at a large N
    "3x10_300001": (2, 6, 3, 10, 300001, True),      # the padded-width-16 instance
    "3x20_300001": (5, 4, 3, 20, 300001, True),      # the padded-width-32 instance
    "3x48_150001": (3, 4, 3, 48, 150001, True),      # the padded-width-64 instance
}


def plain4_min_tiles(width):
    """pinn_fused_plain.hip, fused_plain_min_tiles: a pass of four tiles for each of the 4 waves of every workgroup the chip
    holds (2 per compute unit at padded width 64, else 4)."""
    return 4 * 4 * (2 if width > 32 else 4) * torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def plain_reference(name):
    d_in, d_out, L, W, n_pts, _ = PLAIN[name]
    g = torch.Generator().manual_seed(77)
    params = U.trained_like(O.layer_sizes(d_in, L, W, d_out), g)
    X = torch.rand(n_pts, d_in, generator=g) * 2 - 1
    return params, X, O.mlp_forward([p.double() for p in params], X.double())


@pytest.mark.parametrize("tag", ["auto", "fused", "generic"])
@pytest.mark.parametrize("name", sorted(PLAIN))
def test_plain_forward_at_many_points(name, tag):
    """pinn_forward on enough points runs pinn_fused_plain.hip's four-tiles-per-wave kernel (engine AUTO or FUSED, from
    fused_plain_min_tiles tiles on: 131 072 points at padded width 64 and 262 144 at 16 / 32 on 256 compute units), which
    reads the packed hidden biases by its own code.  Against the fp64 forward at every point."""
    d_in, d_out, L, W, n_pts, plain4 = PLAIN[name]
    assert ((n_pts + 15) // 16 >= plain4_min_tiles(W)) == plain4, (name, plain4_min_tiles(W))      # the kernel this case is about
    params, X, Yo = plain_reference(name)
    Y = Engine(NetDesc(d_in, d_out, L, W, (0, 1), engine=ENG[tag])).forward(O.flatten(params).cuda(), X.cuda())
    err = (Y.cpu().double() - Yo).abs()
    print(f"TRAINED forward | plain {name} {tag}: Y {float(err.max()):.1e} at point {int(err.amax(1).argmax())} (bound {U.abs_bound(Yo):.1e})")
    assert float(err.max()) < U.abs_bound(Yo)


@pytest.mark.parametrize("tag", ["generic", "fused"])
def test_leaky_relu_kaiming_network(tag):
    """The network of tests/test_engine_gpu.py::test_leaky_relu_kaiming_network (init_type 'kaiming' -> LeakyReLU(0.01)) at
    the biased state: jet, loss and gradient per block."""
    desc = NetDesc(2, 3, 3, 16, (0, 1), ACT_LEAKY_RELU, ENG[tag])
    g = torch.Generator().manual_seed(5)
    params = U.trained_like(desc.layers, g, init_type="kaiming")
    X = torch.rand(333, 2, generator=g) * 2 - 1
    eng, flat = Engine(desc), O.flatten(params).cuda()
    Y, dY = eng.forward_jet(flat, X.cuda())
    Yo, dYo = O.jet([p.double() for p in params], X.double(), (0, 1), "kaiming")
    assert float((Y.cpu().double() - Yo).abs().max()) < U.abs_bound(Yo)
    assert float((dY.cpu().double() - dYo).abs().max()) < U.abs_bound(dYo)

    def oracle(dtype):
        q = [p.to(dtype).clone().requires_grad_(True) for p in params]
        lo = O.residual_loss(q, X.to(dtype), "continuity_ftemp", [0, 1], [2, 0, 1], (0, 1), "kaiming")
        return float(lo.detach()), O.flat_grad(lo, q).double()
    (l64, g64), (l32, g32) = oracle(torch.float64), oracle(torch.float32)
    spec = ResidualSpec.from_names("continuity_ftemp", ("x", "y"), (0, 1), ("U", "V", "h"))
    grad = torch.zeros(desc.n_params, device="cuda")
    sums = eng.residual_loss_grad(spec, torch.full((1,), 1.0 / 333, device="cuda"), flat, X.cuda(), grad)
    errs = U.assert_blocks_close(grad, g64, g32, desc.layers, f"leaky {tag}")
    report("leaky", f"3x16 {tag}", errs, g64, g32, desc.layers)
    assert abs(float(sums[0]) / 333 - l64) / l64 < U.loss_bound(l64, l32)


# ---- d. jet_backward: the external-adjoint instances --------------------------------------------------------------------------
JB_CASES = ["pe_10x10", "ns_3x12", "cf_3x32", "ns_5in", "pe_8x64", "ns_8x64"]      # padded width 16, 32, 64 with K1 = 3 and 4
JB = [(n, e) for n in JB_CASES for e in (["generic", "tile"] + (["batch"] if U.CASES[n][3] <= 32 else []))]


@functools.lru_cache(maxsize=None)
def jet_backward_reference(name):
    c = U.Case(name, "biased")
    g = torch.Generator().manual_seed(3)
    gY, gdY = torch.randn(N, c.d_out, generator=g), torch.randn(len(c.gc), N, c.d_out, generator=g)
    return (c, gY, gdY, U.jet_adjoint_grad(c.params, c.X, c.gc, gY, gdY, torch.float64),
            U.jet_adjoint_grad(c.params, c.X, c.gc, gY, gdY, torch.float32))


@pytest.mark.parametrize("name,tag", JB, ids=[f"{n}-{e}" for n, e in JB])
def test_jet_backward(name, tag):
    c, gY, gdY, g64, g32 = jet_backward_reference(name)
    eng = Engine(c.desc(engine=ENG[tag]))
    assert eng.jet_backward_kernel(N) == ENG[tag]          # the kernel this case is about, no silent fallback
    flat, Xd = dev(c)
    grad = torch.zeros(eng.n_params, device="cuda")
    eng.jet_backward(flat, Xd, gY.cuda(), gdY.cuda(), grad)
    errs = U.assert_blocks_close(grad, g64, g32, c.layers, f"jet_backward {name} {tag}")
    report("jet_backward", f"{name} {tag}", errs, g64, g32, c.layers)


# ---- e. residual_fields, and the corrected radiation stress -----------------------------------------------------------------
def assert_fields(tag, got, f64, f32):
    err = (got.cpu().double() - f64).abs().amax(1)
    noise, floor = (f32 - f64).abs().amax(1), 2.0 ** -23 * f64.abs().amax(1)
    print(f"TRAINED fields | {tag}: err {[f'{e:.1e}' for e in err.tolist()]} oracle fp32 {[f'{e:.1e}' for e in noise.tolist()]}")
    assert bool((err <= 4 * torch.maximum(noise, floor)).all()), (tag, err.tolist(), noise.tolist(), floor.tolist())


@functools.lru_cache(maxsize=None)
def fields_reference(name):
    c = U.Case(name, "biased")
    return c, U.oracle_fields(c, torch.float64), U.oracle_fields(c, torch.float32)


@pytest.mark.parametrize("tag", ["tile", "generic"])
@pytest.mark.parametrize("name", ["pe_10x10", "ns_5in", "ns_8x64"])       # the field instances at width 10, 20, 64
def test_residual_fields(name, tag):
    c, f64, f32 = fields_reference(name)
    flat, Xd = dev(c)
    got = Engine(c.desc(engine=ENG[tag])).residual_fields(c.spec(), flat, Xd)
    assert got.shape == (3, N)
    assert_fields(f"{name} {tag}", got, f64, f32)


@functools.lru_cache(maxsize=None)
def corrected_reference(L, W):
    """The corrected residual's conditioning (tests/pe_corrected_util.py: output weights x 0.25, h = 2, eta_mean = 0.2,
    Hrms = 0.5, k = 1) on the biased state."""
    g = torch.Generator().manual_seed(1234)
    layers = O.layer_sizes(2, L, W, 6)
    params = U.trained_like(layers, g)
    params[-2] = params[-2] * 0.25
    params[-1] = torch.tensor([2.0, 0.0, 0.0, 0.2, 0.5, 1.0]) + params[-1] * torch.tensor([0.0, 1, 1, 0, 0, 0])
    X = torch.rand(N, 2, generator=g) * 2 - 1
    f64, _ = PC.net_fields(params, X)
    f32, _ = PC.net_fields(params, X, dtype=torch.float32)
    (l64, g64), (l32, g32) = PC.net_loss_grad(params, X), PC.net_loss_grad(params, X, dtype=torch.float32)
    return layers, params, X, f64.detach().double(), f32.detach().double(), l64, g64, l32, g32


@pytest.mark.parametrize("tag", ["generic", "tile", "auto"])
@pytest.mark.parametrize("L,W", [(10, 10), (8, 64)])
def test_corrected_radiation_stress(L, W, tag):
    layers, params, X, f64, f32, l64, g64, l32, g32 = corrected_reference(L, W)
    desc = NetDesc(2, 6, L, W, (0, 1), engine=ENG[tag])
    spec = ResidualSpec.from_names("physics_equation", ("x", "y"), (0, 1), PC.ROLES, corrected=True)
    eng, flat, Xd = Engine(desc), O.flatten(params).cuda(), X.cuda()
    assert_fields(f"corrected {L}x{W} {tag}", eng.residual_fields(spec, flat, Xd), f64, f32)
    grad = torch.zeros(desc.n_params, device="cuda")
    sums = eng.residual_loss_grad(spec, torch.full((3,), 1.0 / N, device="cuda"), flat, Xd, grad)
    errs = U.assert_blocks_close(grad, g64, g32, layers, f"corrected {L}x{W} {tag}")
    el = abs(float(sums.double().sum()) / N - l64) / abs(l64)
    report("corrected", f"{L}x{W} {tag}", errs, g64, g32, layers, f" loss {el:.1e}")
    assert el < U.loss_bound(l64, l32)


# ---- f. ensembles: every member its own draw (tests/trained_state_util.py, ensemble_reference) ---------------------------------
@pytest.mark.parametrize("name", sorted(U.ENSEMBLE))
def test_ensemble_members_against_their_own_oracle(name):
    """M = 3 members, each with its own trained_like draw: a wrong member stride reads another member's biases.  Each member
    against ITS fp64 oracle per block — not against the single-network call, which shares the code."""
    cname, fid, n_r, n_f = U.ENSEMBLE[name]
    c, members, T, refs = U.ensemble_reference(name)
    n_t = n_r if n_f is None else n_f
    eng, spec = Engine(c.desc()), c.spec()
    scale = torch.full((spec.n_terms,), 1.0 / n_r)
    if c.res == "continuity_only":
        scale = torch.tensor([1.0 / n_r, 1.0 / float((c.X[:, 0] < 25.5).sum()), 0.0])
    cscale = torch.full((len(fid),), 1.0 / max(n_t, 1)).cuda() if fid else None
    theta = torch.stack([O.flatten(p) for p in members]).cuda()
    grad = torch.zeros_like(theta)
    n_res = -1 if n_f is None else n_r
    ts, cs = eng.ensemble_loss_grad(spec, scale.cuda(), theta, c.X.cuda().contiguous(), n_res, grad,
                                    T=None if T is None else T.cuda(), out_col=list(fid), col_scale=cscale)
    for m, (l64, g64, l32, g32) in enumerate(refs):
        loss = float((ts[m].cpu().double() * scale.double()).sum())
        if fid:
            loss += float((cs[m].double() * cscale.double()).sum())
        el = abs(loss - l64) / abs(l64)
        errs = U.assert_blocks_close(grad[m], g64, g32, c.layers, f"ensemble {name} member {m}")
        report("ensemble", f"{name} member {m}", errs, g64, g32, c.layers, f" loss {el:.1e}")
        assert el < U.loss_bound(l64, l32), (name, m, loss, l64)


# ---- g. the wide engine in bf16 mode (fp32 mode: test_loss_and_gradient) ------------------------------------------------------
@pytest.mark.parametrize("tag", ["wide", "auto"])
@pytest.mark.parametrize("name", ["ns_3x128", "ns_5x256"])
def test_bf16_mode(name, tag):
    """bf16 MFMA operands on the wide engine's first / last layer kernels and the chain kernels in between: term sums 3e-2,
    gradient 1e-1 PER BLOCK against fp64.  This catches a layer's biases dropped or shifted (>= 4.5e-1 in every block),
    not a single unit's."""
    c, l64, g64, l32, g32 = U.reference(name, "biased")
    f64 = U.oracle_fields(c, torch.float64)
    s64 = (f64 ** 2).sum(1)
    eng = Engine(c.desc(engine=ENG[tag], precision=PREC_BF16))
    flat, Xd = dev(c)
    grad = torch.zeros(eng.n_params, device="cuda")
    sums = eng.residual_loss_grad(c.spec(), c.term_scale().cuda(), flat, Xd, grad)
    es = ((sums.cpu().double() - s64) / s64).abs()
    errs = U.block_errors(grad, g64, c.layers)
    print(f"TRAINED bf16 | {name} {tag}: sums off by {float(es.max()):.1e}, blocks {', '.join(f'{k} {v:.1e}' for k, v in errs.items())}")
    U.assert_blocks_close(grad, g64, g64, c.layers, f"bf16 {name} {tag}", floor=1e-1, gap_cap=None)
    assert float(es.max()) < 3e-2, (sums.tolist(), s64.tolist())


# ---- h. second order ---------------------------------------------------------------------------------------------------------
NU = 0.1
SCALE2 = (0.7, 1.3, 0.9)


@functools.lru_cache(maxsize=None)
def second_order_reference(name):
    c = U.Case(name, "biased")
    sc = [s / N for s in SCALE2]
    r64 = R2.net_sums_grad(c.params, c.X, c.res, False, NU, c.inn, c.outn, sc)
    r32 = R2.net_sums_grad(c.params, c.X, c.res, False, NU, c.inn, c.outn, sc, dtype=torch.float32)
    j64 = [t.detach() for t in U.jets(c.params, c.X, c.gc, torch.float64, second=True)[1:]]
    return c, r64, r32, j64


@pytest.mark.parametrize("tag", ["generic", "fused"])
@pytest.mark.parametrize("name", ["ns_8x64", "pe_10x10"])
def test_second_order(name, tag):
    """forward_jet2 and residual2_loss_grad (nu = 0.1) on the generic kernels and on the MFMA ones."""
    c, (s64, f64, g64), (s32, f32, g32), j64 = second_order_reference(name)
    eng = Engine(c.desc(engine=ENG[tag]))
    flat, Xd = dev(c)
    got = eng.forward_jet2(flat, Xd)
    for what, a, r64 in zip(("Y", "dY", "d2Y"), got, j64):
        e, b = float((a.cpu().double() - r64).abs().max()), U.abs_bound(r64)
        print(f"TRAINED second order | {name} {tag}: {what} {e:.1e} (bound {b:.1e})")
        assert e < b, (what, e, b)
    scale = torch.tensor([s / N for s in SCALE2], device="cuda")
    grad = torch.zeros(eng.n_params, device="cuda")
    sums, F = eng.residual2_loss_grad(c.spec(nu=NU), scale, flat, Xd, grad=grad, fields=True)
    errs = U.assert_blocks_close(grad, g64, g32, c.layers, f"residual2 {name} {tag}")
    report("second order", f"{name} {tag}", errs, g64, g32, c.layers)
    assert_fields(f"residual2 {name} {tag}", F, f64.double(), f32.double())
    for t in range(3):
        noise = abs(float(s32[t]) - float(s64[t])) / float(s64[t])
        assert abs(float(sums[t]) - float(s64[t])) / float(s64[t]) < max(2e-6, 4 * noise), (t, sums.tolist(), s64.tolist())


# ---- i. the dropout instance --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["tile", "generic"])
def test_dropout_instance(tag):
    """Training-mode dropout (p = 0.3) on the tile kernel's dropout instance (width 33..64) and on the generic kernels: the
    oracle gets the engine's own masks (tests/dropout_util.py)."""
    p, seed = 0.3, 20241004
    c = U.Case("pe_4x48", "biased")
    masks = [torch.from_numpy(m) for m in keep_masks(seed, p, c.L, c.W, N)]
    (l64, g64), (l32, g32) = (U.oracle_total(c, dt, masks=masks, p=p) for dt in (torch.float64, torch.float32))
    eng = Engine(c.desc(engine=ENG[tag], dropout_p=p))
    eng.dropout_seed = seed
    flat, Xd = dev(c)
    grad = torch.zeros(eng.n_params, device="cuda")
    sums = eng.residual_loss_grad(c.spec(), c.term_scale().cuda(), flat, Xd, grad)
    el = abs(float(sums.double().sum()) / N - l64) / abs(l64)
    errs = U.assert_blocks_close(grad, g64, g32, c.layers, f"dropout {tag}")
    report("dropout", f"pe_4x48 p=0.3 {tag}", errs, g64, g32, c.layers, f" loss {el:.1e}")
    assert el < U.loss_bound(l64, l32)


# ---- j. the folded Adam iteration ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pe_10x10", "ns_8x64"])
def test_two_folded_adam_iterations(name):
    """Two loss_grad_adam_step iterations from the biased state.  The second one reads the packed biases (Bp) that the first
    one's finishing kernel wrote: its gradient is held per block to the oracle at the parameters the first iteration left,
    and the parameters after both to two Adam steps of the oracle in float64, in units of the step."""
    lr, iters = 1e-3, 2
    c, l64, g64, l32, g32 = U.reference(name, "biased")
    eng, spec = Engine(c.desc()), c.spec()
    flat0, Xd = dev(c)
    nP = eng.n_params
    th, grad, m, v = flat0.clone(), torch.zeros(nP, device="cuda"), torch.zeros(nP, device="cuda"), torch.zeros(nP, device="cuda")
    ts, scale = torch.zeros(spec.n_terms, device="cuda"), c.term_scale().cuda()
    assert eng.loss_grad_adam_step(spec, scale, th, Xd, N, grad, m, v, 1, lr, term_sums=ts)
    e1 = U.assert_blocks_close(grad, g64, g32, c.layers, f"folded Adam {name}: first gradient")
    th1 = O.unflatten(th.cpu().clone(), c.layers)
    tok, ws = eng._packed_tok, eng.workspace(N)
    # the second call must NOT re-pack: the engine hands packed_valid = 1 exactly when this token matches the call
    assert tok is not None and tok[0] is ws and tok[1] == th.data_ptr() and tok[2] == th._version and tok[3] is None
    assert tok[4] == (N, N, 0, spec.residual_id, spec.corrected)
    assert eng.loss_grad_adam_step(spec, scale, th, Xd, N, grad, m, v, 2, lr, term_sums=ts)
    (l64b, g64b), (l32b, g32b) = U.oracle_total(c, torch.float64, params=th1), U.oracle_total(c, torch.float32, params=th1)
    e2 = U.assert_blocks_close(grad, g64b, g32b, c.layers, f"folded Adam {name}: second gradient (packed biases rewritten)")
    report("folded Adam", f"{name} first gradient", e1, g64, g32, c.layers)
    report("folded Adam", f"{name} second gradient", e2, g64b, g32b, c.layers)
    assert abs(float((ts.cpu().double() * scale.cpu().double()).sum()) - l64b) / abs(l64b) < U.loss_bound(l64b, l32b)
    _, ref = O.adam_trajectory([p.double() for p in c.params], U.residual_loss_fn(c), iters, lr)
    ref, got, th0 = O.flatten(ref), th.cpu().double(), flat0.cpu().double()
    dmax, drel = float((got - ref).abs().max()), float((got - ref).norm() / (ref - th0).norm())
    print(f"TRAINED folded Adam | {name}: max|theta - ref| {dmax:.2e} ({dmax / lr:.3f} steps), relative to the path {drel:.2e}")
    assert dmax < 1.025 * iters * lr and drel < 2e-2
    for nm, a, b in U.param_blocks(c.layers):          # every block moved, the bias blocks among them
        assert float((got[a:b] - th0[a:b]).abs().max()) > 0.5 * lr, nm

