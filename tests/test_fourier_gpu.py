"""The sine first layer (PINN_ACT_SIN_TANH) on the GPU: the generic engine and the fused tile kernel against the fp64
reference of tests/fourier_util.py, request kind by request kind, and the dispatch rules around them.

Error measure and bars: fourier_util's — err = max|q - q64| / max|q64| per quantity (Y, dY, each term sum, each block of the
flat gradient), bar = max(the tanh sibling's bar in test_engine_gpu.py, 4 x the fp32-CPU yardstick's error on the same case).
Every figure is printed before it is asserted."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import pinn_oracle as O
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec
from pinn_depthestimation_amd._lib import (ACT_SIN_TANH, ACT_TANH, ENGINE_AUTO, ENGINE_FUSED, ENGINE_FUSED_BATCH, ENGINE_FUSED_COOP,
                                           ENGINE_FUSED_TILE, ENGINE_GENERIC, ENGINE_WIDE, PREC_BF16, PinnError)

from tests import fourier_util as F

pytestmark = pytest.mark.gpu

ENGINES = [ENGINE_GENERIC, ENGINE_FUSED_TILE]
ENGINE_IDS = ["generic", "tile"]
WORST = {}          # (engine, quantity) -> (error, bar, case): what DESIGN 2.14 quotes


def note(engine, quantity, e, b, case):
    key = ("generic" if engine == ENGINE_GENERIC else "tile", quantity)
    if key not in WORST or e / b > WORST[key][0] / WORST[key][1]:
        WORST[key] = (e, b, case)


def check(engine, quantity, kind, got, ref64, ref32, case):
    e, y = F.err(got, ref64), F.err(ref32, ref64)
    b = F.bar(kind, y)
    note(engine, quantity, e, b, case)
    print(f"  {case} {quantity}: err {e:.2e} yardstick {y:.2e} bar {b:.2e}")
    assert e <= b, (case, quantity, e, y, b)


def desc_of(layers, grad_cols, engine, act=ACT_SIN_TANH, **kw):
    return NetDesc.from_layers(layers, grad_cols, act, engine, **kw)


# ---- 1. forward and forward jet ----------------------------------------------------------------------------------------
JET_SHAPES = {"3-8x64-4": ([3] + [64] * 8 + [4], (0, 1, 2)), "2-10x10-6": ([2] + [10] * 10 + [6], (0, 1)),
              "4-3x20-4": ([4] + [20] * 3 + [4], (1, 2, 3)), "3-1x40-2": ([3, 40, 2], ())}


@functools.lru_cache(maxsize=None)
def jet_case(shape, N, sigma):
    layers, gc = JET_SHAPES[shape]
    params = F.make_params(layers, sigma, seed=17 * N + int(sigma))
    X = F.points(N, layers[0], seed=N + 3)
    return layers, gc, params, X, F.jet(params, X, gc, torch.float64), F.jet(params, X, gc, torch.float32)


@pytest.mark.parametrize("engine", ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize("sigma", [1.0, 16.0])
@pytest.mark.parametrize("shape", list(JET_SHAPES))
def test_forward_and_forward_jet(shape, sigma, engine):
    for N in (1, 16, 17, 243):
        layers, gc, params, X, (Y64, dY64), (Y32, dY32) = jet_case(shape, N, sigma)
        eng = Engine(desc_of(layers, gc, engine))
        flat, Xd = O.flatten(params).cuda(), X.cuda().contiguous()
        case = f"{shape} s={sigma:g} N={N}"
        check(engine, "Y", "Y", eng.forward(flat, Xd), Y64, Y32, case + " forward")
        if gc:
            Y, dY = eng.forward_jet(flat, Xd)
            check(engine, "Y", "Y", Y, Y64, Y32, case + " jet")
            check(engine, "dY", "dY", dY, dY64, dY32, case + " jet")


@pytest.mark.parametrize("shape", ["3-8x64-4", "2-10x10-6", "4-3x20-4"])
def test_plain_forward_kernel(shape):
    """pinn_forward under AUTO on enough points takes the plain forward's own kernel (four tiles per wave): another kernel than
    the tile kernel's K1 = 1 instance, compared on its own — against the tile kernel on every point (the same arithmetic per
    point: bit-equal) and against fp64 on a 512-point subsample."""
    layers, gc = JET_SHAPES[shape]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = 16 * (4 * 4 * 4 * cus) + 5          # >= fused_plain_min_tiles for every width (4 tiles x 4 waves x at most 4 workgroups per CU)
    params = F.make_params(layers, 4.0, seed=5)
    X = F.points(N, layers[0], seed=6)
    flat, Xd = O.flatten(params).cuda(), X.cuda().contiguous()
    Yp = Engine(desc_of(layers, gc, ENGINE_AUTO)).forward(flat, Xd)
    Yt = Engine(desc_of(layers, gc, ENGINE_FUSED_TILE)).forward(flat, Xd)
    assert torch.equal(Yp, Yt)
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:512]
    Y64, _ = F.jet(params, X[idx], (), torch.float64)
    Y32, _ = F.jet(params, X[idx], (), torch.float32)
    check(ENGINE_FUSED_TILE, "Y (plain kernel)", "Y", Yp[idx.cuda()], Y64, Y32, f"{shape} plain N={N}")
    # ... and it is the sine network it ran, not a tanh or LeakyReLU one
    Ytanh = Engine(desc_of(layers, gc, ENGINE_AUTO, act=ACT_TANH)).forward(flat, Xd)
    assert F.err(Ytanh[idx.cuda()], Y64) > 100 * 2e-6


# ---- 2. loss and gradient, every loss kind of the generic epilogue, block by block ------------------------------------------
def run_loss(eng, c):
    """The request of case c on engine eng: (term sums or None, column sums or None, flat gradient)."""
    flat, Xd = O.flatten(c["params"]).cuda(), c["X"].cuda().contiguous()
    grad = torch.zeros(flat.numel(), device="cuda")
    kind = c["kind"]
    spec = None if c["residual"] is None else ResidualSpec.from_names(c["residual"], c["inn"], c["grad_cols"], c["outn"])
    if kind in ("ns", "pe", "co"):
        ts = eng.residual_loss_grad(spec, c["scale"].cuda(), flat, Xd, grad)
        ts_only = eng.residual_loss(spec, flat, Xd)
        assert torch.allclose(ts, ts_only, rtol=1e-6, atol=0)
        return ts, None, grad
    if kind == "mse":
        return None, eng.mse_loss_grad(flat, Xd, c["T"].cuda(), c["out_cols"], c["col_scale"].cuda(), grad), grad
    if kind == "merged":
        ts, cs = eng.residual_mse_loss_grad(spec, c["scale"].cuda(), c["T"].cuda(), c["out_cols"], c["col_scale"].cuda(), flat, Xd, grad)
        return ts, cs, grad
    ts, cs = eng.residual_mse_split_loss_grad(spec, c["scale"].cuda(), c["T"].cuda(), c["out_cols"], c["col_scale"].cuda(), flat, Xd,
                                              c["n_split"], grad)
    return ts, cs, grad


def check_loss(engine, c, got, case):
    ts, cs, grad = got
    ts64, cs64, g64 = c["ref"]
    ts32, cs32, g32 = c["y32"]
    if ts is not None:
        for t in range(len(ts64)):
            if c["residual"] == "continuity_only" and t == 2:
                assert float(ts[2]) == float(ts64[2])          # the count of anchored points: exact
            elif float(ts64[t]) == 0.0:
                assert float(ts[t]) == 0.0
            else:
                check(engine, "term sums", "sums", ts[t:t + 1], ts64[t:t + 1], ts32[t:t + 1], f"{case} term {t}")
    if cs is not None:
        for j in range(len(cs64)):
            check(engine, "column sums", "sums", cs[j:j + 1], cs64[j:j + 1], cs32[j:j + 1], f"{case} column {j}")
    for name, sl in F.blocks(c["layers"]).items():
        if float(g64[sl].abs().max()) == 0.0:
            assert float(grad[sl].abs().max()) == 0.0
            continue
        check(engine, f"gradient block {name}", "grad", grad[sl], g64[sl], g32[sl], f"{case} grad[{name}]")
    check(engine, "gradient (whole)", "grad", grad, g64, g32, f"{case} grad")


@pytest.mark.parametrize("engine", ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize("N", [1, 17, 243])
@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("kind", ["ns", "pe", "co", "mse", "merged", "split"])
def test_loss_and_gradient_block_by_block(kind, L, N, engine):
    """Every width of a (kind, depth, N, engine) is run and its figures printed before the test fails on the first miss.
    (N = 1: a term sum is ONE squared field, its relative error twice the field's — the case that showed that an fp32 z_0 is
    the largest error of a sine layer; the kernels form it in double.)"""
    misses = []
    for W in (10, 20, 40, 64):
        c = F.loss_case(kind, L, W, N)
        eng = Engine(desc_of(c["layers"], c["grad_cols"], engine))
        try:
            check_loss(engine, c, run_loss(eng, c), f"{kind} L={L} W={W} N={N}")
        except AssertionError as e:
            misses.append(str(e).splitlines()[0])
    assert not misses, misses


# ---- 3. the gradient copy in global memory ----------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ENGINES, ids=ENGINE_IDS)
def test_gradient_copy_in_global_memory(engine):
    """2 -> 100 x 20 -> 3: the padded gradient (100 layers of 32 x 32) does not fit LDS — the LDSACC = false instance."""
    layers = [2] + [20] * 100 + [3]
    params = F.make_params(layers, 4.0, seed=9)
    X = F.points(33, 2, seed=10)
    X[:, 0] = X[:, 0] * 40
    inn, outn, _ = F.RES["continuity_only"]
    scale = F.scales("continuity_only", X, 33)
    c = dict(kind="co", residual="continuity_only", inn=inn, outn=outn, layers=layers, params=params, X=X, grad_cols=(0, 1),
             scale=scale, T=None, out_cols=None, col_scale=None, n_split=-1,
             ref=F.loss_and_grad(params, X, torch.float64, "continuity_only", (0, 1), scale),
             y32=F.loss_and_grad(params, X, torch.float32, "continuity_only", (0, 1), scale))
    eng = Engine(desc_of(layers, (0, 1), engine))
    check_loss(engine, c, run_loss(eng, c), "100x20 continuity_only N=33")


# ---- 4. more than one tile per wave, and the input prefetch -----------------------------------------------------------------
def test_more_than_one_tile_per_wave():
    """2 -> 2 x 10 -> 6 on more tiles than the tile kernel launches waves: a width-16 instance runs at most 3 workgroups of 4
    waves on each compute unit (the engine's grid cap, read here from the device's CU count), so 16 x (12 CUs) + 5 points give
    every wave its first tile, some a second one through the prefetched inputs, and a ragged last tile."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = 16 * (4 * 3 * cus) + 5
    layers = [2, 10, 10, 6]
    inn, outn, _ = F.RES["physics_equation"]
    params = F.make_params(layers, 4.0, seed=21, out_scale=0.2)
    params[-1][0], params[-1][3] = 0.75, 0.0
    X = F.points(N, 2, seed=22)
    flat, Xd = O.flatten(params).cuda(), X.cuda().contiguous()
    spec = ResidualSpec.from_names("physics_equation", inn, (0, 1), outn)
    scale = torch.full((3,), 1.0 / N)
    out = {}
    for engine in ENGINES:
        eng = Engine(desc_of(layers, (0, 1), engine))
        grad = torch.zeros(flat.numel(), device="cuda")
        ts = eng.residual_loss_grad(spec, scale.cuda(), flat, Xd, grad)
        out[engine] = (ts.cpu().double(), grad.cpu().double(), eng.forward_jet(flat, Xd))
    tg, gg, (Yg, dYg) = out[ENGINE_GENERIC]
    tt, gt, (Yt, dYt) = out[ENGINE_FUSED_TILE]
    print(f"  N={N}: tile vs generic: sums {F.err(tt, tg):.2e} grad {F.err(gt, gg):.2e} Y {F.err(Yt, Yg):.2e} dY {F.err(dYt, dYg):.2e}")
    # two fp32 evaluations of the same formula: each within the tanh sibling's bar of fp64, so within twice it of each other
    assert F.err(tt, tg) < 2 * 2e-6 and F.err(gt, gg) < 2 * 2e-5 and F.err(Yt, Yg) < 2 * 2e-6 and F.err(dYt, dYg) < 2 * 2e-6
    # the fields' inputs against fp64 on a 512-point subsample that reaches into the second tiles and the ragged tail
    idx = torch.cat([torch.randperm(N, generator=torch.Generator().manual_seed(2))[:500], torch.arange(N - 12, N)])
    Y64, dY64 = F.jet(params, X[idx], (0, 1), torch.float64)
    Y32, dY32 = F.jet(params, X[idx], (0, 1), torch.float32)
    for engine, (Y, dY) in ((ENGINE_GENERIC, (Yg, dYg)), (ENGINE_FUSED_TILE, (Yt, dYt))):
        check(engine, "Y", "Y", Y[idx.cuda()], Y64, Y32, f"N={N} subsample")
        check(engine, "dY", "dY", dY[:, idx.cuda()], dY64, dY32, f"N={N} subsample")
    cols = O.split_columns(X[idx].double(), (0, 1))
    f64 = torch.cat(F.fields("physics_equation", cols, F.sin_mlp([p.double() for p in params], torch.cat(cols, -1))), 1).t().detach()
    cols = O.split_columns(X[idx], (0, 1))
    f32 = torch.cat(F.fields("physics_equation", cols, F.sin_mlp(params, torch.cat(cols, -1))), 1).t().detach()
    got = Engine(desc_of(layers, (0, 1), ENGINE_AUTO)).residual_fields(spec, flat, Xd)[:, idx.cuda()]
    check(ENGINE_FUSED_TILE, "fields", "sums", got, f64, f32, f"N={N} fields subsample")


# ---- 5. a sine network is not a tanh network --------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [10, 20, 64])
def test_a_sine_network_is_not_a_tanh_network(W):
    c = F.loss_case("pe", 2, W, 243)
    flat, Xd = O.flatten(c["params"]).cuda(), c["X"].cuda().contiguous()
    spec = ResidualSpec.from_names(c["residual"], c["inn"], c["grad_cols"], c["outn"])
    loss = {}
    for act in (ACT_TANH, ACT_SIN_TANH):
        eng = Engine(desc_of(c["layers"], c["grad_cols"], ENGINE_FUSED_TILE, act=act))
        grad = torch.zeros(flat.numel(), device="cuda")
        ts = eng.residual_loss_grad(spec, c["scale"].cuda(), flat, Xd, grad)
        loss[act] = float((ts.cpu().double() * c["scale"].double()).sum())
    ts64, _, _ = c["ref"]
    l64 = float((ts64 * c["scale"].double()).sum())
    bar = F.bar("sums", F.err(c["y32"][0], ts64))
    print(f"  W={W}: loss sine {loss[ACT_SIN_TANH]:.6e} tanh {loss[ACT_TANH]:.6e} fp64 sine {l64:.6e} bar {bar:.1e}")
    assert abs(loss[ACT_SIN_TANH] - loss[ACT_TANH]) / abs(l64) > 100 * bar
    assert abs(loss[ACT_SIN_TANH] - l64) / abs(l64) <= bar


# ---- 6. dispatch --------------------------------------------------------------------------------------------------------
def _pe_case(N=243, conditioned=False):
    layers = [2, 20, 20, 20, 6]
    inn, outn, _ = F.RES["physics_equation"]
    params = F.make_params(layers, 4.0, seed=31, out_scale=0.25 if conditioned else 0.2)
    if conditioned:        # the corrected stress: kh in [1.6, 2.4], eta + h near 2.2 (tests/pe_corrected_util.py)
        for name, val in (("h", 2.0), ("eta_mean", 0.2), ("Hrms", 0.5), ("k", 1.0)):
            params[-1][outn.index(name)] = val
    else:
        params[-1][0], params[-1][3] = 0.75, 0.0
    return layers, inn, outn, params, F.points(N, 2, seed=32)


def _ref_weighted(params, X, dtype, scale, fields_fn, w=None):
    p = [q.to(dtype).requires_grad_(True) for q in params]
    cols = O.split_columns(X.to(dtype), (0, 1))
    Y = F.sin_mlp(p, torch.cat(cols, -1))
    f = torch.cat(fields_fn(cols, Y), 1).t()                       # (3, N)
    ww = torch.ones_like(f) if w is None else w.to(dtype)
    ts = (ww * f ** 2).sum(dim=1)
    g = O.flat_grad((ts * scale.to(dtype)).sum(), p)
    return ts.detach(), g.detach(), f.detach()


def test_dispatch_requests_without_a_sine_instance_run_under_auto():
    """Coefficient, weighted, corrected-stress, residual_fields and jet_backward requests on a sine network under AUTO: no fused
    instance serves them, they run on the generic engine's kernels (residual_fields through the forward jet) and match fp64."""
    from tests.pe_corrected_util import pec_fields
    layers, inn, outn, params, X = _pe_case()
    flat, Xd = O.flatten(params).cuda(), X.cuda().contiguous()
    N, P = X.shape[0], flat.numel()
    scale = torch.full((3,), 1.0 / N)
    eng = Engine(desc_of(layers, (0, 1), ENGINE_AUTO))
    spec = ResidualSpec.from_names("physics_equation", inn, (0, 1), outn)
    plain = lambda cols, Y: F.fields("physics_equation", cols, Y)
    r64, r32 = (_ref_weighted(params, X, dt, scale, plain) for dt in (torch.float64, torch.float32))
    A = ENGINE_AUTO
    # coefficients at their compiled-in values: the plain residual's numbers
    coef = torch.tensor(spec.coef_defaults, dtype=torch.float32, device="cuda")
    grad, cg = torch.zeros(P, device="cuda"), torch.zeros_like(coef)
    ts = eng.residual_coef_loss_grad(spec, coef, scale.cuda(), flat, Xd, grad, cg)
    check(A, "term sums (coef)", "sums", ts, r64[0], r32[0], "coef")
    check(A, "gradient (coef)", "grad", grad, r64[1], r32[1], "coef")
    assert bool(torch.isfinite(cg).all()) and float(cg.abs().max()) > 0
    # point weights, one row per term
    w = torch.rand(3, N, generator=torch.Generator().manual_seed(33)) + 0.5
    w64, w32 = (_ref_weighted(params, X, dt, scale, plain, w) for dt in (torch.float64, torch.float32))
    grad = torch.zeros(P, device="cuda")
    ts, fl = eng.residual_weighted_loss_grad(spec, w.cuda().contiguous(), scale.cuda(), flat, Xd, grad, fields=True)
    check(A, "term sums (weighted)", "sums", ts, w64[0], w32[0], "weighted")
    check(A, "gradient (weighted)", "grad", grad, w64[1], w32[1], "weighted")
    check(A, "fields (weighted)", "sums", fl, w64[2], w32[2], "weighted")
    # residual_fields and jet_backward
    check(A, "fields", "sums", eng.residual_fields(spec, flat, Xd), r64[2], r32[2], "residual_fields")
    g = torch.Generator().manual_seed(34)
    gY, gdY = torch.randn(N, 6, generator=g), torch.randn(2, N, 6, generator=g)
    jb = []
    for dt in (torch.float64, torch.float32):
        p = [q.to(dt).requires_grad_(True) for q in params]
        cols = O.split_columns(X.to(dt), (0, 1))
        Y = F.sin_mlp(p, torch.cat(cols, -1))
        dY = torch.stack([torch.cat([O.compute_gradient(Y[:, c:c + 1], cols[j]) for c in range(6)], 1) for j in (0, 1)])
        jb.append(O.flat_grad((Y * gY.to(dt)).sum() + (dY * gdY.to(dt)).sum(), p).detach())
    grad = torch.zeros(P, device="cuda")
    eng.jet_backward(flat, Xd, gY.cuda(), gdY.cuda(), grad)
    check(A, "gradient (jet_backward)", "grad", grad, jb[0], jb[1], "jet_backward")
    assert eng.jet_backward_kernel(N) == ENGINE_GENERIC
    # the corrected radiation stress
    layers, inn, outn, params, X = _pe_case(conditioned=True)
    flat, Xd = O.flatten(params).cuda(), X.cuda().contiguous()
    specc = ResidualSpec.from_names("physics_equation", inn, (0, 1), outn, corrected=True)
    corr = lambda cols, Y: pec_fields(cols[0], cols[1], *[Y[:, r:r + 1] for r in range(6)])
    c64, c32 = (_ref_weighted(params, X, dt, scale, corr) for dt in (torch.float64, torch.float32))
    grad = torch.zeros(P, device="cuda")
    ts = eng.residual_loss_grad(specc, scale.cuda(), flat, Xd, grad)
    check(A, "term sums (corrected)", "sums", ts, c64[0], c32[0], "corrected")
    check(A, "gradient (corrected)", "grad", grad, c64[1], c32[1], "corrected")
    check(A, "fields (corrected)", "sums", eng.residual_fields(specc, flat, Xd), c64[2], c32[2], "corrected fields")
    # ... and an explicit fused engine is refused for each, with the sine layer named
    tile = Engine(desc_of(layers, (0, 1), ENGINE_FUSED_TILE))
    grad = torch.zeros(P, device="cuda")
    for call in (lambda: tile.residual_coef_loss_grad(spec, coef, scale.cuda(), flat, Xd, grad),
                 lambda: tile.residual_weighted_loss_grad(spec, w.cuda().contiguous(), scale.cuda(), flat, Xd, grad),
                 lambda: tile.residual_loss_grad(specc, scale.cuda(), flat, Xd, grad),
                 lambda: tile.residual_fields(spec, flat, Xd),
                 lambda: tile.jet_backward(flat, Xd, gY.cuda(), gdY.cuda(), grad)):
        with pytest.raises(PinnError, match="sine first layer"):
            call()
    assert float(grad.abs().max()) == 0.0


def test_dispatch_refusals_name_the_sine_layer():
    layers, inn, outn, params, X = _pe_case(N=48)
    flat, Xd = O.flatten(params).cuda(), X.cuda().contiguous()
    spec = ResidualSpec.from_names("physics_equation", inn, (0, 1), outn)
    scale = torch.full((3,), 1.0 / 48, device="cuda")
    grad = torch.zeros(flat.numel(), device="cuda")
    pat = "sine first layer|activation 2"
    for engine in (ENGINE_FUSED_COOP, ENGINE_FUSED_BATCH):
        with pytest.raises(PinnError, match=pat):
            Engine(desc_of(layers, (0, 1), engine)).residual_loss_grad(spec, scale, flat, Xd, grad)
    wide_layers = [2, 128, 128, 6]
    wflat = O.flatten(F.make_params(wide_layers, 1.0, seed=1)).cuda()
    wgrad = torch.zeros_like(wflat)
    with pytest.raises(PinnError, match=pat):
        Engine(desc_of(wide_layers, (0, 1), ENGINE_WIDE)).residual_loss_grad(spec, scale, wflat, Xd, wgrad)
    with pytest.raises(PinnError, match=pat):
        Engine(desc_of(wide_layers, (0, 1), ENGINE_AUTO, precision=PREC_BF16)).residual_loss_grad(spec, scale, wflat, Xd, wgrad)
    # (width 128 in fp32 under AUTO: neither MFMA engine has a sine kernel, the generic engine runs it)
    ts = Engine(desc_of(wide_layers, (0, 1), ENGINE_AUTO)).residual_loss_grad(spec, scale, wflat, Xd, wgrad)
    assert bool(torch.isfinite(ts).all()) and float(wgrad.abs().max()) > 0
    ens = Engine(desc_of(layers, (0, 1), ENGINE_AUTO))
    why = ens.ensemble_refusal(spec, 2, 48, 48, 0)
    assert why and "sine first layer" in why
    with pytest.raises(PinnError, match=pat):
        ens.ensemble_loss_grad(spec, scale, flat.repeat(2, 1).contiguous(), Xd, 48, torch.zeros(2, flat.numel(), device="cuda"))
    with pytest.raises(PinnError, match=pat):
        ens.forward_jet2(flat, Xd)
    with pytest.raises(PinnError, match=pat):
        ens.residual2_loss_grad(ResidualSpec.from_names("physics_equation", inn, (0, 1), outn, nu=0.1), scale, flat, Xd, grad)
    assert float(grad.abs().max()) == 0.0
    from pinn_depthestimation_amd.config import load_config
    from pinn_depthestimation_amd.ensemble import EnsemblePINN
    with pytest.raises(PinnError, match="sine first layer"):
        EnsemblePINN(None, None, X.numpy(), load_config(_cfg(3, 0)), members=2)


# ---- 7. training --------------------------------------------------------------------------------------------------------
def _cfg(adam_it, lbfgs_it, **layer_keys):
    return {"layers": dict({"input_features": 2, "hidden_layers": 3, "hidden_width": 20, "output_features": 6,
                            "first_activation": "sin", "fourier_sigma": 4.0}, **layer_keys),
            "adam_optimizer": {"max_it": adam_it, "learning_rate": 1e-3, "scheduler_step_size": 10000, "scheduler_gamma": 0.8},
            "lbfgs_optimizer": {"max_it": lbfgs_it, "learning_rate": 1, "max_evaluation": None, "history_size": 100,
                                "tolerance_grad": 1e-9, "tolerance_change": 1e-12, "line_search_fn": "strong_wolfe"},
            "loss": {"weight_fid_loss": 1, "weight_res_loss": 1},
            "data_fidelity": {"inputs": ["x", "y"], "outputs": ["h", "U"]},
            "data_residual": {"inputs": {k: {"requires_grad": ["true"]} for k in "xy"},
                              "outputs": ["h", "U", "V", "eta_mean", "Hrms", "k"]}}


@functools.lru_cache(maxsize=None)
def _training_problem():
    layers, inn, outn, params, _ = _pe_case()
    Xr, Xf = F.points(243, 2, seed=41), F.points(12, 2, seed=42)
    Tf = torch.rand(12, 2, generator=torch.Generator().manual_seed(43))

    def run(dt):
        def loss_fn(p):
            cols = O.split_columns(Xr.to(dt), (0, 1))
            fs = F.fields("physics_equation", cols, F.sin_mlp(p, torch.cat(cols, -1)))
            Yf = F.sin_mlp(p, Xf.to(dt))
            fid = sum(torch.mean((Tf.to(dt)[:, j:j + 1] - Yf[:, j:j + 1]) ** 2) for j in range(2))     # oracle.fidelity_loss's form
            return fid + sum(torch.mean(f ** 2) for f in fs)
        return np.array(O.adam_trajectory([q.to(dt) for q in params], loss_fn, 30, 1e-3)[0])

    l64, l32 = run(torch.float64), run(torch.float32)
    return layers, params, Xr, Xf, Tf, l64, float(np.max(np.abs(l32 - l64) / np.abs(l64)))


def _trainer(fold, lbfgs_it=0, **kw):
    from pinn_depthestimation_amd.trainer import PINN
    layers, params, Xr, Xf, Tf, _, _ = _training_problem()
    tr = PINN(Xf.numpy(), Tf.numpy(), Xr.numpy(), _cfg(30, lbfgs_it), log_every=1, checkpoint_every=0, fold_adam=fold, **kw)
    assert tr.dnn.first_activation == "sin" and tr.dnn.fourier_sigma == 4.0 and tr.evaluator.eng.desc.activation == ACT_SIN_TANH
    with torch.no_grad():                       # the problem's own parameters (the module's draw is another network)
        for p, q in zip(tr.dnn._ordered_params(), params):
            p.copy_(q)
    return tr


def test_training_folded_equals_classic_and_walks_the_fp64_trajectory():
    _, _, _, _, _, l64, gap = _training_problem()
    res = {}
    for fold in (False, True):
        tr = _trainer(fold)
        if fold:
            tr.train_adam(30)
        else:
            for _ in range(30):
                tr.adam_step()
        assert (tr._folded_iters > 0) == fold and tr.iter == 30
        res[fold] = (tr.dnn.flat_params().clone(), np.array([r[3] for r in tr.history]), np.array(tr.history))
    # tests/test_adam_fold_gpu.py's comparison of the two paths on a kernel whose gradient copies are added to in lock order (the
    # tile kernel; only the cooperative kernel, which a sine network never runs, is bit-reproducible): parameters to
    # rtol 2e-4 / atol 1e-7 max|theta|, logged losses to fp32 rounding of the weighted sum
    a, b = res[False][0], res[True][0]
    print(f"  folded vs classic after 30 iterations: max |d theta| {float((a - b).abs().max()):.2e} (max |theta| {float(a.abs().max()):.2e}), "
          f"max rel loss difference {np.max(np.abs(res[True][2][:, 1:] / res[False][2][:, 1:] - 1)):.2e}")
    assert torch.allclose(a, b, rtol=2e-4, atol=1e-7 * float(a.abs().max()))
    assert np.allclose(res[True][2][:, 1:], res[False][2][:, 1:], rtol=2e-6, atol=0.0)
    for fold in (False, True):
        rel = np.abs(res[fold][1] - l64) / np.abs(l64)
        print(f"  sine trainer fold={fold}: max rel loss error over 30 iterations {rel.max():.2e}, after 30 {rel[-1]:.2e} (fp32 gap {gap:.2e})")
        assert len(rel) == 30 and float(rel.max()) < max(1e-5, 4 * gap)
        assert res[fold][1][-1] < res[fold][1][0]


def test_training_device_lbfgs_lowers_the_loss():
    tr = _trainer(True, lbfgs_it=3, lbfgs_impl="device")
    tr.train_adam(30)
    before = float(tr.history[-1][3])
    tr.train_lbfgs_device()
    after = float(tr.history[-1][3])
    print(f"  sine trainer: loss after 30 Adam iterations {before:.6e}, after 3 device L-BFGS iterations {after:.6e}")
    assert math.isfinite(after) and after < before


# ---- 8. checkpoint round trip -----------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_is_bit_equal(tmp_path):
    from pinn_depthestimation_amd.dnn import DNN
    torch.manual_seed(7)
    m = DNN([2, 20, 20, 20, 6], 0.0, "xavier", first_activation="sin", fourier_sigma=4.0).cuda().eval()
    X = F.points(300, 2, seed=8).cuda()
    with torch.no_grad():
        Y = m(X).clone()
    Y64, _ = F.jet([p.detach().cpu() for p in m._ordered_params()], X.cpu(), (), torch.float64)
    assert F.err(Y, Y64) < 1e-5                                   # it is the sine network the module runs
    torch.save(m, str(tmp_path / "whole.pth"))
    torch.save(m.state_dict(), str(tmp_path / "state.pth"))
    whole = torch.load(str(tmp_path / "whole.pth"), weights_only=False)
    assert whole.first_activation == "sin" and whole.activation_id == ACT_SIN_TANH
    fresh = DNN([2, 20, 20, 20, 6], 0.0, "xavier", first_activation="sin", fourier_sigma=4.0)
    fresh.load_state_dict(torch.load(str(tmp_path / "state.pth"), weights_only=True))
    fresh = fresh.cuda().eval()
    with torch.no_grad():
        assert torch.equal(whole(X), Y) and torch.equal(fresh(X), Y)
    # the same state dict in a module WITHOUT the keyword is a tanh network: another function
    plain = DNN([2, 20, 20, 20, 6], 0.0, "xavier")
    plain.load_state_dict(torch.load(str(tmp_path / "state.pth"), weights_only=True))
    with torch.no_grad():
        assert not torch.allclose(plain.cuda().eval()(X), Y, atol=1e-3)


def test_zz_report_worst_errors():
    """Prints the worst measured error of every quantity over the tests above, against its bar (DESIGN 2.14 quotes these)."""
    for (eng, q), (e, b, case) in sorted(WORST.items()):
        print(f"  WORST {eng:8s} {q:28s} err {e:.2e} bar {b:.2e} ({case})")
