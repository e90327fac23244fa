"""pinn_residual_fields on the GPU: the per-point residual fields against the fp64 oracle, the tile loop's point
counts, consistency with the loss sums, the staged (forward jet + point-wise kernel) path, and RAD in the trainer.

Bounds.  Against the oracle: per field, max_n |f_gpu - f_64| <= 4 * max(max_n |f_32 - f_64|, 2^-23 * max_n |f_64|),
f_32 the same oracle functions in float32 on the CPU (4 x the reference's own fp32 noise, as tests/test_g6b_gpu.py).
Staged path: |f - F64(jet)| <= 64 * 2^-24 * A_n point by point, F64 the field formula in float64 on the engine's OWN
forward_jet output and A_n the same formula with every product and every term replaced by its absolute value — the
rounding of a dozen fp32 operations, none of the jet's own error.  Loss: sum_n f^2 (float64, host) against
residual_loss's term_sums at rtol 2e-6, the bar between two summation orders of the same squares.
"""
import ctypes as C
import functools

import pytest
import torch

from oracle import pinn_oracle as O
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec
from pinn_depthestimation_amd._lib import (ACT_LEAKY_RELU, ENGINE_FUSED, ENGINE_FUSED_TILE, ENGINE_GENERIC, PREC_BF16,
                                           PinnError)
from pinn_depthestimation_amd.engine import RESIDUAL_ROLES, _ptr

from tests.test_engine_gpu import make_case
from tests.test_fields_cpu import CFG, StubEvaluator

pytestmark = pytest.mark.gpu

ENGINES = [ENGINE_FUSED_TILE, ENGINE_GENERIC]
ORACLE_CASES = ["ns_8x64", "pe_10x10", "cf_4x20", "co_3x64", "ns_out_first_3x12", "cf_out_first_2x64", "ns_2x48", "ns_5in",
                "leaky_3x20"]
LEAKY = (2, 3, 3, 20, (0, 1), "continuity_ftemp", ("x", "y"), ("U", "V", "h"))


def oracle_fields(params, X, res, inn, outn, grad_cols, dtype, init_type="xavier"):
    """(NF, N): O.navier_stokes_fields / physics_equation_fields / continuity_fields on O.mlp_forward in `dtype` (CPU)."""
    cols = O.split_columns(X.to(dtype), grad_cols)
    Y = O.mlp_forward([p.to(dtype) for p in params], torch.cat(cols, -1), init_type)
    _, out_roles, dir_roles = RESIDUAL_ROLES[res]
    ins = [cols[inn.index(r)] for r in dir_roles]
    outs = [Y[:, outn.index(r):outn.index(r) + 1] for r in out_roles]
    if res == "Navier_Stokes":
        f = O.navier_stokes_fields(*ins, *outs)
    elif res == "physics_equation":
        f = O.physics_equation_fields(*ins, *outs)
    else:
        fc = O.continuity_fields(*ins, *outs)
        on = (ins[0] < 25.5) if res == "continuity_only" else torch.zeros_like(fc, dtype=torch.bool)
        f = (fc, torch.where(on, outs[0] - 0.75, torch.zeros_like(fc)))
    return torch.cat([t.detach() for t in f], 1).T.contiguous()


@functools.lru_cache(maxsize=None)
def case(name, N):
    """Network, points and the two oracle runs of one case, computed once and shared (nothing below writes to them)."""
    if name == "leaky_3x20":
        d_in, d_out, L, W, gc, res, inn, outn = LEAKY
        g = torch.Generator().manual_seed(5)
        desc = NetDesc(d_in, d_out, L, W, gc, ACT_LEAKY_RELU)
        params, init = O.init_params(desc.layers, "kaiming", g), "kaiming"
        X = torch.rand(N, d_in, generator=g) * 2 - 1
    else:
        _, params, X, desc, res, inn, outn = make_case(name, N)
        init = "xavier"
        if res == "continuity_only":
            X[:, 0] = X[:, 0] * 40          # make x < 25.5 a real subset
    f64 = oracle_fields(params, X, res, inn, outn, desc.grad_cols, torch.float64, init)
    f32 = oracle_fields(params, X, res, inn, outn, desc.grad_cols, torch.float32, init).double()
    spec = ResidualSpec.from_names(res, inn, desc.grad_cols, outn)
    return desc, spec, O.flatten(params), X.contiguous(), f64, f32


def check_against_oracle(tag, got, f64, f32):
    """The module's oracle bound for the first got.shape[1] points of a case; prints the measured ratio per field.
    The right-hand side (the reference's own fp32 noise and the magnitude of the field) is taken over ALL points the
    case's oracle ran on: it is the noise level of the network, and a prefix of one or fifteen points is held to it
    rather than to the luck of its own one or fifteen fp32 roundings."""
    n = got.shape[1]
    err = (got.cpu().double() - f64[:, :n]).abs().amax(1)
    noise = (f32 - f64).abs().amax(1)
    floor = 2.0 ** -23 * f64.abs().amax(1)
    bound = 4 * torch.maximum(noise, floor)
    ratio = err / torch.maximum(noise, floor).clamp_min(1e-300)
    print(f"FIELDS {tag} N={n}: err {[f'{e:.2e}' for e in err.tolist()]} ref-noise {[f'{e:.2e}' for e in noise.tolist()]} "
          f"ratio {[f'{r:.2f}' for r in ratio.tolist()]}")
    assert bool((err <= bound).all()), (tag, err.tolist(), bound.tolist())


@pytest.mark.parametrize("engine", ENGINES, ids=["tile", "generic"])
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_fields_against_fp64_oracle(name, engine):
    desc, spec, flat, X, f64, f32 = case(name, 777)
    eng = Engine(desc.with_(engine=engine))
    got = eng.residual_fields(spec, flat.cuda(), X.cuda())
    assert got.shape == (spec.n_fields, 777) and got.dtype == torch.float32
    check_against_oracle(f"{name}/{'tile' if engine == ENGINE_FUSED_TILE else 'generic'}", got, f64, f32)
    if spec.name == "continuity_only":
        m = X[:, 0] < 25.5
        assert 0 < int(m.sum()) < 777 and bool((got[1].cpu()[~m] == 0).all()) and bool((got[1].cpu()[m] != 0).any())
    if spec.name == "continuity_ftemp":
        assert float(got[1].abs().max()) == 0.0


def big_n():
    """Above 16 points x 4 waves x the largest grid the host launches (3 workgroups per CU at padded width 16): a wave
    walks more than one tile and the prefetch of the next tile's X is exercised."""
    return 16 * 4 * 3 * torch.cuda.get_device_properties(0).multi_processor_count + 100


@pytest.mark.parametrize("engine", ENGINES, ids=["tile", "generic"])
@pytest.mark.parametrize("name", ["ns_8x64", "pe_10x10"])
def test_point_counts_of_the_tile_loop(name, engine):
    NB = big_n()
    desc, spec, flat, X, f64, f32 = case(name, NB)          # one oracle run; every count below is a prefix of its points
    eng = Engine(desc.with_(engine=engine))
    fl, Xd = flat.cuda(), X.cuda()
    rows = {}
    for N in (1, 15, 16, 17, 777, NB):
        got = eng.residual_fields(spec, fl, Xd[:N].contiguous())
        assert got.shape == (spec.n_fields, N)
        check_against_oracle(f"{name}/N", got, f64, f32)
        rows[N] = got
    # a point's value does not depend on its neighbours
    assert torch.equal(rows[17], rows[777][:, :17])
    assert torch.equal(rows[777], rows[NB][:, :777])
    # nothing is written past NF * N
    for N in (17, 777):
        nf = spec.n_fields
        buf = torch.full((nf * N + 64,), 1e30, device="cuda")
        ws = eng.fields_workspace(spec, N)
        eng._run("pinn_residual_fields", eng.lib.pinn_residual_fields, C.byref(eng._d()), C.byref(spec.c_struct()),
                 _ptr(fl), _ptr(Xd), N, _ptr(buf), _ptr(ws), ws.numel())
        assert bool((buf[nf * N:] == 1e30).all())
        assert torch.equal(buf[:nf * N].view(nf, N), rows[N])


@pytest.mark.parametrize("engine", ENGINES, ids=["tile", "generic"])
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_fields_square_to_the_loss_sums(name, engine):
    desc, spec, flat, X, _, _ = case(name, 777)
    eng = Engine(desc.with_(engine=engine))
    fl, Xd = flat.cuda(), X.cuda()
    F = eng.residual_fields(spec, fl, Xd).cpu().double()
    sums = eng.residual_loss(spec, fl, Xd).cpu().double()
    sq = F.square().sum(1)
    n_cmp = 1 if spec.name == "continuity_ftemp" else (2 if spec.name == "continuity_only" else 3)
    rel = (sq[:n_cmp] - sums[:n_cmp]).abs() / sums[:n_cmp].abs()
    print(f"FIELDS-vs-loss {name}: rel {[f'{r:.2e}' for r in rel.tolist()]}")
    assert bool((rel <= 2e-6).all()), (sq.tolist(), sums.tolist())
    if spec.name == "continuity_only":
        assert int((F[1] != 0).sum()) <= int(sums[2])
        h = eng.forward(fl, Xd)[:, spec.out_col[0]].cpu()
        m = X[:, 0] < 25.5
        diff = (F[1][m] - (h[m] - 0.75).double()).abs().max()
        print(f"FIELDS da vs forward {name}: max diff {float(diff):.2e}")
        assert torch.equal(F[1][m].float(), h[m] - 0.75)


# ---- the staged path: forward jet + point-wise kernel ---------------------------------------------------------------
def jet_fields64(spec, X, Y, dY, absval=False):
    """The residual's field formulas in float64 on a jet Y (N, d_out), dY (k, N, d_out); absval: every product and
    every term replaced by its absolute value (the magnitude fp32 rounding acts on)."""
    Y, dY = Y.double(), dY.double()
    a = (lambda t: t.abs()) if absval else (lambda t: t)
    val = lambda r: a(Y[:, spec.out_col[r]])
    der = lambda d, r: a(dY[spec.dir_of[d], :, spec.out_col[r]])
    if spec.name == "Navier_Stokes":
        h, z, u, w = (val(r) for r in range(4))
        G, CB = 9.81, 3.0 / 16.0 * 9.81 * 0.78 ** 2
        H, Hx, Hy = h + z, der(1, 0) + der(1, 1), der(2, 0) + der(2, 1)
        fc = der(0, 1) + Hx * u + H * der(1, 2) + Hy * w + H * der(2, 3)
        fx = der(0, 2) + u * der(1, 2) + w * der(2, 2) + G * der(1, 1) + CB * Hx * H
        fy = der(0, 3) + u * der(1, 3) + w * der(2, 3) + G * der(2, 1) + CB * Hy * H
        return torch.stack([fc, fx, fy])
    assert spec.name == "continuity_ftemp"
    h, U, V = (val(r) for r in range(3))
    fc = der(0, 0) * U + h * der(0, 1) + der(1, 0) * V + h * der(1, 2)
    return torch.stack([fc, torch.zeros_like(fc)])


STAGED = {
    # name: (descriptor, residual, inputs, outputs)
    "wide_3x100": (NetDesc(3, 4, 3, 100, (0, 1, 2)), "Navier_Stokes", ("t", "x", "y"), ("h", "z", "u", "v")),
    "dropout_3x20": (NetDesc(2, 3, 3, 20, (0, 1), dropout_p=0.2), "continuity_ftemp", ("x", "y"), ("U", "V", "h")),
    "bf16_2x128": (NetDesc(2, 3, 2, 128, (0, 1), precision=PREC_BF16), "continuity_ftemp", ("x", "y"), ("U", "V", "h")),
}


@pytest.mark.parametrize("name", list(STAGED))
def test_staged_path_against_its_own_jet(name):
    desc, res, inn, outn = STAGED[name]
    g = torch.Generator().manual_seed(21)
    flat = O.flatten(O.init_params(desc.layers, "xavier", g)).cuda()
    X = (torch.rand(777, desc.d_in, generator=g) * 2 - 1).cuda()
    spec = ResidualSpec.from_names(res, inn, desc.grad_cols, outn)
    eng = Engine(desc)
    eng.dropout_seed = 4242                     # the same mask for the jet and for the fields
    Y, dY = eng.forward_jet(flat, X)
    F = eng.residual_fields(spec, flat, X)
    want = jet_fields64(spec, X, Y.cpu(), dY.cpu())
    A = jet_fields64(spec, X, Y.cpu(), dY.cpu(), absval=True)
    diff = (F.cpu().double() - want).abs()
    bound = 64 * 2.0 ** -24 * A
    print(f"FIELDS staged {name}: max diff / bound {float((diff / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((diff <= bound).all())
    if name == "dropout_3x20":                  # the mask is on: the eval-mode engine gives other values
        F0 = Engine(desc.with_(dropout_p=0.0)).residual_fields(spec, flat, X)
        assert not torch.equal(F0, F)


def test_staged_path_walks_more_than_one_chunk():
    """N = 65536 + 17 on the generic engine: a full chunk and a short last one (n0 > 0, the X offset, the write at
    fields[f * N + n0 + i]).  A point's value does not depend on the call it is part of, so the result must equal, to
    the bit, two separate calls on the two parts.  The tile kernel (one launch, no chunks) is compared too: each engine is
    held to 4 x max(reference fp32 noise, 2^-23 |f|) of the fp64 oracle (test_fields_against_fp64_oracle), so two engines
    are within twice that of each other; the noise is the case's own (same network, its 777 oracle points)."""
    N0, N = 65536, 65536 + 17
    desc, spec, flat, X, f64, f32 = case("pe_10x10", 777)
    g = torch.Generator().manual_seed(77)
    Xd = (torch.rand(N, desc.d_in, generator=g) * 2 - 1).cuda()
    fl = flat.cuda()
    eng = Engine(desc.with_(engine=ENGINE_GENERIC))
    buf = torch.full((spec.n_fields * N + 64,), 1e30, device="cuda")
    ws = eng.fields_workspace(spec, N)
    eng._run("pinn_residual_fields", eng.lib.pinn_residual_fields, C.byref(eng._d()), C.byref(spec.c_struct()),
             _ptr(fl), _ptr(Xd), N, _ptr(buf), _ptr(ws), ws.numel())
    F = buf[:spec.n_fields * N].view(spec.n_fields, N)
    assert bool((buf[spec.n_fields * N:] == 1e30).all())
    head = eng.residual_fields(spec, fl, Xd[:N0].contiguous())
    tail = eng.residual_fields(spec, fl, Xd[N0:].contiguous())
    assert torch.equal(F[:, :N0], head) and torch.equal(F[:, N0:], tail)
    T = Engine(desc.with_(engine=ENGINE_FUSED_TILE)).residual_fields(spec, fl, Xd)
    gap = (T.double() - F.double()).abs().amax(1).cpu()
    noise = torch.maximum((f32 - f64).abs().amax(1), 2.0 ** -23 * F.double().abs().amax(1).cpu())
    print(f"FIELDS chunks: tile vs staged max gap {gap.tolist()}, reference noise {noise.tolist()}")
    assert bool((gap <= 8 * noise).all())


def test_tester_residual_fields_on_a_grid():
    """inference.Tester.residual_fields: the engine's fields on an ny x nx grid, published as plot_res_<name>, inputs
    denormalised as test() does."""
    from pinn_depthestimation_amd.dnn import DNN
    from pinn_depthestimation_amd.inference import FIELD_NAMES, Tester
    ny, nx = 7, 9
    cfg = dict(CFG, data_test={"nx": nx, "ny": ny})
    torch.manual_seed(11)
    model = DNN([2, 20, 20, 20, 3], 0.0, "xavier")
    t = Tester(model, cfg)
    assert t.residual == "continuity_ftemp"
    grid = torch.rand(ny * nx, 2, generator=torch.Generator().manual_seed(2)) * 2 - 1
    out = t.residual_fields(grid.numpy(), input_min_max={"x": (10.0, 30.0)})
    assert out.shape == (2, ny * nx)
    desc = NetDesc(2, 3, 3, 20, (0, 1))
    spec = ResidualSpec.from_names("continuity_ftemp", ("x", "y"), (0, 1), ("U", "V", "h"))
    want = Engine(desc).residual_fields(spec, t.model.flat_params(), grid.cuda())
    assert torch.equal(torch.from_numpy(out), want.cpu())
    assert float(want[0].abs().max()) > 0
    for name, row in zip(FIELD_NAMES["continuity_ftemp"], out):
        assert getattr(t, f"plot_res_{name}").shape == (ny, nx)
        assert (getattr(t, f"plot_res_{name}") == row.reshape(ny, nx)).all()
    from pinn_depthestimation_amd import operations as op
    assert (t.plot_input_x == op.denormalize(grid[:, 0].numpy().reshape(ny, nx), 10.0, 30.0)).all()
    assert (t.plot_input_y == grid[:, 1].numpy().reshape(ny, nx)).all()
    assert t.residual_fields(grid[:5].numpy()).shape == (2, 5)          # not a grid: no maps, same fields
    assert (t.residual_fields(grid[:5].numpy()) == out[:, :5]).all()


def test_fused_engine_refuses_a_wide_network():
    desc, res, inn, outn = STAGED["wide_3x100"]
    spec = ResidualSpec.from_names(res, inn, desc.grad_cols, outn)
    eng = Engine(desc.with_(engine=ENGINE_FUSED))
    with pytest.raises(PinnError, match=r"code -2.*width above 64"):
        eng.residual_fields(spec, torch.zeros(desc.n_params, device="cuda"), torch.zeros(32, 3, device="cuda"))


# ---- trainer -------------------------------------------------------------------------------------------------------
def _trainer(**kw):
    from pinn_depthestimation_amd.dnn import DNN
    from pinn_depthestimation_amd.trainer import PINN
    torch.manual_seed(3)
    Xr = torch.rand(4096, 2, generator=torch.Generator().manual_seed(5)) * 2 - 1
    return PINN(None, None, Xr.numpy(), CFG, dnn=DNN([2, 20, 20, 20, 3], 0.0, "xavier"), checkpoint_every=0, **kw), Xr


def test_rad_training_runs_and_residual_fields_face():
    tr, Xr = _trainer(residual_batch=512, resample="rad", rad_every=5)
    tr.train()
    hist = tr.history
    assert len(hist) == 12 and all(torch.isfinite(torch.tensor(h[1:])).all() for h in hist)
    assert tr._rad_at == 10                      # scored at iterations 0, 5, 10
    F = tr.residual_fields()
    assert F.shape == (2, 4096) and bool(torch.isfinite(F).all()) and float(F[1].abs().max()) == 0.0
    assert tr.residual_fields(Xr[:100].numpy()).shape == (2, 100)
    assert torch.equal(tr.residual_fields(Xr[:100].numpy()), F[:, :100])


def test_rad_draws_only_scored_rows_on_the_device():
    ev = StubEvaluator(torch.arange(0, 4096, 64))
    tr, Xr = _trainer(residual_batch=512, resample="rad", rad_every=5, rad_c=0.0, evaluator=ev)
    for _ in range(12):
        tr.adam_step()
    hot = {tuple(r) for r in Xr[ev.hot].tolist()}
    assert ev.scored == 3 and len(ev.batches) == 12
    for b in ev.batches:
        assert b.is_cuda and b.shape == (512, 2) and all(tuple(r) in hot for r in b.cpu().tolist())


def test_uniform_resampling_is_bit_identical_to_before():
    # the generic engine: bit-reproducible from run to run (include/pinn_hip.h), so two trainers can be compared to the bit
    a, _ = _trainer(residual_batch=512, engine=ENGINE_GENERIC)
    b, _ = _trainer(residual_batch=512, engine=ENGINE_GENERIC, resample="uniform")
    a.train(); b.train()
    assert len(a.history) == 12 and a.history == b.history
    assert torch.equal(a.dnn.flat_params(), b.dnn.flat_params())
