"""Ensembles: M networks of one shape through one launch of the tile kernel's ensemble instances (pinn_hip.h, "ensembles";
fused_kernel.h, k_fused_ens).  Member m must get what the single-network entry gives on params[m].

Tolerances.  A member's pass differs from the single call the way two tile-kernel runs with another grid differ (another
gx, lock-ordered adds into the workgroup's gradient copy), so the comparisons use what tests/test_adam_fold_gpu.py applies
to two such runs: loss sums rtol 1e-5, gradient relative L2 error < 5e-6, parameters and Adam moments after six
iterations rtol 2e-4 with atol 1e-7 max|x|.  Where both paths launch one workgroup with one working wave (one tile) the
order of the adds is the same and the comparison is torch.equal.  The oracle comparison is
tests/test_engine_gpu.py::test_residual_loss_grad's: max(2e-6, 4 x the oracle's own fp32-fp64 difference) on the loss,
max(2e-5, 4 x ...) on the gradient's relative L2 error."""
import numpy as np
import pytest
import torch

from oracle import pinn_oracle as O          # parameter initialisation and the fp64 reference
from pinn_depthestimation_amd import Engine, EnsemblePINN, NetDesc, PinnError, ResidualSpec
from pinn_depthestimation_amd import _lib
from pinn_depthestimation_amd.dnn import DNN, init_flat_params
from pinn_depthestimation_amd.trainer import PINN

from tests.golden_util import CMB, rel_l2

pytestmark = pytest.mark.gpu

PE_OUT = ("h", "U", "V", "eta_mean", "Hrms", "k")
CASES = {
    # name: d_in, d_out, L, W, grad_cols, residual, inputs, outputs, fidelity columns, N_res, N_fid (None: one point set)
    "pe10x10_split": (2, 6, 10, 10, (0, 1), "physics_equation", ("x", "y"), PE_OUT, (0, 1, 2, 3, 4, 5), 243, 12),
    "ns8x64_res_only": (3, 4, 8, 64, (0, 1, 2), "Navier_Stokes", ("t", "x", "y"), ("h", "z", "u", "v"), (), 243, 0),
    "co40x20_both": (2, 3, 40, 20, (0, 1), "continuity_only", ("x", "y"), ("U", "V", "h"), (0, 1), 100, None),
    "pe10x10_one_tile": (2, 6, 10, 10, (0, 1), "physics_equation", ("x", "y"), PE_OUT, (0, 1, 2, 3, 4, 5), 12, 4),
}


class Case:
    def __init__(self, name, M, seed=77, own_sets=False):
        d_in, d_out, L, W, gc, res, inn, outn, fid, n_r, n_f = CASES[name]
        g = torch.Generator().manual_seed(seed)
        rows = []
        for _ in range(M):
            params = O.init_params(O.layer_sizes(d_in, L, W, d_out), "xavier", g)
            if res == "physics_equation":            # keep eta_mean + h away from 0 (the residual divides by it)
                params[-1][outn.index("h")] = 0.75; params[-1][outn.index("eta_mean")] = 0.0
            rows.append(O.flatten(params))
        self.layers = O.layer_sizes(d_in, L, W, d_out)
        self.res, self.inn, self.outn, self.gc = res, inn, outn, gc
        self.desc = NetDesc(d_in, d_out, L, W, gc)
        self.spec = ResidualSpec.from_names(res, inn, gc, outn)
        self.theta = torch.stack(rows).cuda()
        self.M, self.P, self.fid = M, self.theta.shape[1], list(fid)
        N = n_r + (0 if n_f is None else n_f)
        nt = n_r if n_f is None else n_f
        lead = (M,) if own_sets else ()
        X = torch.rand(*lead, N, d_in, generator=g) * 2 - 1
        if res == "continuity_only":
            X[..., 0] = X[..., 0] * 40               # make x < 25.5 a real subset
            cnt = float((X[..., 0] < 25.5).sum()) / (M if own_sets else 1)
            self.scale = torch.tensor([1.0 / n_r, 1.0 / cnt, 0.0]).cuda()
        else:
            self.scale = torch.full((self.spec.n_terms,), 1.0 / n_r).cuda()
        self.X = X.cuda().contiguous()
        self.T = torch.rand(*lead, nt, len(fid), generator=g).cuda() if fid else None
        self.cscale = torch.full((len(fid),), 1.0 / max(nt, 1)).cuda() if fid else None
        self.N, self.n_res = N, (-1 if n_f is None else n_r)      # (n_f == 0: n_res == N, the residual alone)

    def single(self, eng, m, grad=None, X=None, T=None):
        """Member m through the single-network entry its request runs on: (term sums, column sums, gradient)."""
        X = self.X if X is None else X
        T = self.T if T is None else T
        th = self.theta[m].contiguous()
        grad = torch.zeros(self.P, device="cuda") if grad is None else grad
        if not self.fid:
            return eng.residual_loss_grad(self.spec, self.scale, th, X, grad), None, grad
        if self.n_res < 0:
            ts, cs = eng.residual_mse_loss_grad(self.spec, self.scale, T, self.fid, self.cscale, th, X, grad)
        else:
            ts, cs = eng.residual_mse_split_loss_grad(self.spec, self.scale, T, self.fid, self.cscale, th, X, self.n_res, grad)
        return ts, cs, grad

    def ensemble(self, eng, theta=None, grad=None, X=None, T=None):
        theta = self.theta if theta is None else theta
        grad = torch.zeros_like(theta) if grad is None else grad
        ts, cs = eng.ensemble_loss_grad(self.spec, self.scale, theta, self.X if X is None else X, self.n_res, grad,
                                        T=self.T if T is None else T, out_col=self.fid, col_scale=self.cscale)
        return ts, cs, grad


def close_sums(a, b):
    return a is None and b is None or bool(torch.allclose(a, b, rtol=1e-5))


def assert_member_is_single(ens, m, one, what=""):
    ts, cs, g = ens
    assert close_sums(ts[m], one[0]), f"{what} member {m}: term sums {ts[m].tolist()} vs {one[0].tolist()}"
    assert close_sums(None if cs is None else cs[m], one[1]), f"{what} member {m}: column sums"
    rel = rel_l2(g[m], one[2])
    assert rel < 5e-6, f"{what} member {m}: gradient differs by {rel:.2e}"


# ---- 1. member m equals the single-network call ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,gx_gt_1,lds", [("pe10x10_split", True, True), ("ns8x64_res_only", True, True),
                                             ("co40x20_both", True, False)])
def test_member_equals_the_single_network_call(name, gx_gt_1, lds):
    c = Case(name, 3)
    eng = Engine(c.desc)
    gx, in_lds = eng.ensemble_plan(3, c.N)
    assert (gx > 1) == gx_gt_1 and in_lds == lds, (gx, in_lds)      # the case this test is about: several workgroups per
    ens = c.ensemble(eng)                                             # member, a ragged last tile; where the copy lives
    for m in range(3):
        assert_member_is_single(ens, m, c.single(eng, m), name)
    if name == "co40x20_both":
        cnt = float((c.X[:, 0] < 25.5).sum())
        assert [float(v) for v in ens[0][:, 2]] == [cnt] * 3        # the third "sum" of continuity_only counts its points
    if name == "pe10x10_split":     # ... and one member against the fp64 oracle, both loss terms
        m, nr = 1, c.n_res
        fid_w = [1.0] * 6

        def oracle(dtype):
            p = [q.to(dtype).clone().requires_grad_(True) for q in O.unflatten(c.theta[m].cpu(), c.layers)]
            X = c.X.cpu().to(dtype)
            lr = O.residual_loss(p, X[:nr], c.res, [0, 1], [c.outn.index(r) for r in PE_OUT], c.gc)
            lf = O.fidelity_loss(p, X[nr:], c.T.cpu().to(dtype), c.fid, fid_w)
            return (lr + lf).detach(), O.flat_grad(lr + lf, p)
        l64, g64 = oracle(torch.float64)
        l32, g32 = oracle(torch.float32)
        ts, cs, g = ens
        loss = float((ts[m].double() * c.scale.double()).sum() + (cs[m].double() * c.cscale.double()).sum())
        noise = abs(float(l32) - float(l64)) / abs(float(l64))
        assert abs(loss - float(l64)) / abs(float(l64)) < max(2e-6, 4 * noise)
        assert rel_l2(g[m].cpu(), g64) < max(2e-5, 4 * rel_l2(g32, g64))


# ---- 2. one tile: the same order of additions, the same bits ---------------------------------------------------------------
def test_one_tile_is_bitwise_the_single_call():
    c = Case("pe10x10_one_tile", 5)
    assert c.N == 16
    eng = Engine(c.desc)
    assert eng.ensemble_plan(5, 16) == (1, True)
    ts, cs, g = c.ensemble(eng)
    for m in range(5):
        ots, ocs, og = c.single(eng, m)
        assert torch.equal(ts[m], ots) and torch.equal(cs[m], ocs), m
        assert torch.equal(g[m], og), (m, rel_l2(g[m], og))


# ---- 3. members do not touch each other; the buffer contract ---------------------------------------------------------------
def test_members_do_not_touch_each_other():
    c = Case("pe10x10_split", 4)
    eng = Engine(c.desc)
    ones = [c.single(eng, m) for m in range(4)]
    for poisoned in ([1, 2, 3], [0]):
        th = c.theta.clone()
        th[poisoned] = float("nan")
        ens = c.ensemble(eng, theta=th)
        for m in range(4):
            if m in poisoned:
                assert bool(torch.isnan(ens[2][m]).any())
            else:
                assert bool(torch.isfinite(ens[0][m]).all() and torch.isfinite(ens[1][m]).all() and torch.isfinite(ens[2][m]).all())
                assert_member_is_single(ens, m, ones[m], f"poisoned {poisoned}:")


def test_grad_accumulates_guard_bands_hold_and_a_dirty_workspace_does_not_matter():
    c = Case("pe10x10_split", 4)
    eng = Engine(c.desc)
    M, P, nt, nc, G = c.M, c.P, c.spec.n_terms, len(c.fid), 64
    ones = [c.single(eng, m) for m in range(4)]

    def banded(n):
        buf = torch.full((G + n + G,), 1e30, device="cuda")
        return buf, buf[G:G + n]
    gb, g = banded(M * P); tb, ts = banded(M * nt); cb, cs = banded(M * nc)
    g, ts, cs = g.view(M, P).zero_(), ts.view(M, nt), cs.view(M, nc)
    eng.ensemble_workspace(M, c.N).view(torch.float32).fill_(1e30)          # a dirty workspace: every region is written before read
    eng.ensemble_loss_grad(c.spec, c.scale, c.theta, c.X, c.n_res, g, T=c.T, out_col=c.fid, col_scale=c.cscale, term_sums=ts, col_sums=cs)
    for m in range(4):
        assert_member_is_single((ts, cs, g), m, ones[m], "dirty workspace:")
    first = g.clone()
    eng.ensemble_loss_grad(c.spec, c.scale, c.theta, c.X, c.n_res, g, T=c.T, out_col=c.fid, col_scale=c.cscale, term_sums=ts, col_sums=cs)
    assert rel_l2(g, 2 * first) < 5e-6                                       # grad +=: a second call doubles it
    for m in range(4):
        assert close_sums(ts[m], ones[m][0]) and close_sums(cs[m], ones[m][1])   # the sums are overwritten, not added to
    # ... and the folded update's buffers
    mb, mm = banded(M * P); vb, vv = banded(M * P)
    mm, vv = mm.view(M, P).zero_(), vv.view(M, P).zero_()
    th = c.theta.clone()
    assert eng.ensemble_adam_step(c.spec, c.scale, th, c.X, c.n_res, g, mm, vv, 1, 1e-3, T=c.T, out_col=c.fid, col_scale=c.cscale,
                                  term_sums=ts, col_sums=cs)
    assert rel_l2(g, first) < 5e-6                                           # the Adam entry OVERWRITES grad
    torch.cuda.synchronize()
    for band in (gb, tb, cb, mb, vb):
        assert bool((band[:G] == 1e30).all() and (band[-G:] == 1e30).all())
    assert bool(torch.isfinite(th).all()) and float((th - c.theta).abs().max()) > 0


# ---- 4. more members than the grid has room for --------------------------------------------------------------------------------
def test_clamped_grid():
    c3 = Case("pe10x10_split", 3)
    eng = Engine(c3.desc)
    base = Case("pe10x10_split", 300, seed=5)
    gx3, gx300 = eng.ensemble_plan(3, base.N)[0], eng.ensemble_plan(300, base.N)[0]
    assert 1 <= gx300 < gx3, (gx300, gx3)
    ens = base.ensemble(eng)
    for m in (0, 150, 299):
        assert_member_is_single(ens, m, base.single(eng, m), "M = 300:")
    assert bool(torch.isfinite(ens[2]).all())


# ---- 5. one point set per member -----------------------------------------------------------------------------------------------
def test_per_member_point_sets():
    c = Case("pe10x10_split", 3, own_sets=True)
    eng = Engine(c.desc)
    assert c.X.shape == (3, 255, 2) and c.T.shape == (3, 12, 6)
    ens = c.ensemble(eng)                                            # flags bits 0 and 1
    for m in range(3):
        assert_member_is_single(ens, m, c.single(eng, m, X=c.X[m].contiguous(), T=c.T[m].contiguous()), "own X, T:")
    # one bit at a time: own X with shared T, shared X with own T
    ex = c.ensemble(eng, T=c.T[0].contiguous())
    et = c.ensemble(eng, X=c.X[0].contiguous())
    for m in range(3):
        assert_member_is_single(ex, m, c.single(eng, m, X=c.X[m].contiguous(), T=c.T[0].contiguous()), "own X:")
        assert_member_is_single(et, m, c.single(eng, m, X=c.X[0].contiguous(), T=c.T[m].contiguous()), "own T:")
    # equal arrays for every member: what the shared form computes
    Xs, Ts = c.X[1].contiguous(), c.T[1].contiguous()
    shared = c.ensemble(eng, X=Xs, T=Ts)
    own = c.ensemble(eng, X=Xs.unsqueeze(0).repeat(3, 1, 1), T=Ts.unsqueeze(0).repeat(3, 1, 1))
    for m in range(3):
        assert_member_is_single(own, m, (shared[0][m], shared[1][m], shared[2][m]), "equal arrays:")
    # both terms on every point (n_res < 0): T is (M, N, n_cols)
    b = Case("co40x20_both", 2, own_sets=True)
    engb = Engine(b.desc)
    eb = b.ensemble(engb)
    for m in range(2):
        assert_member_is_single(eb, m, b.single(engb, m, X=b.X[m].contiguous(), T=b.T[m].contiguous()), "own X, T, n_res < 0:")


# ---- 6. Adam ---------------------------------------------------------------------------------------------------------------------
def _lr(step):
    return 1e-3 * 0.8 ** (step // 3)


@pytest.fixture(scope="module")
def adam_single_runs():
    """Three single-network runs of six folded iterations (tests/test_adam_fold_gpu.py's schedule), computed once."""
    c = Case("pe10x10_split", 3)
    out = []
    for m in range(3):
        eng = Engine(c.desc)
        th, grad = c.theta[m].clone(), torch.zeros(c.P, device="cuda")
        mm, vv = torch.zeros(c.P, device="cuda"), torch.zeros(c.P, device="cuda")
        ts, cs = torch.zeros(c.spec.n_terms, device="cuda"), torch.zeros(len(c.fid), device="cuda")
        hist = []
        for step in range(1, 7):
            if step == 4:
                th.mul_(1.0 + 1e-3)
            assert eng.loss_grad_adam_step(c.spec, c.scale, th, c.X, c.n_res, grad, mm, vv, step, _lr(step), T=c.T, out_col=c.fid,
                                           col_scale=c.cscale, term_sums=ts, col_sums=cs)
            hist.append((ts.clone(), cs.clone(), grad.clone()))
        out.append((th, mm, vv, hist))
    torch.cuda.synchronize()
    return c, out


def _same(x, y):
    return bool(torch.allclose(x, y, rtol=2e-4, atol=1e-7 * float(x.abs().max())))


def test_six_adam_iterations_against_three_single_network_runs(adam_single_runs):
    c, ref = adam_single_runs
    eng = Engine(c.desc)
    th, grad = c.theta.clone(), torch.zeros(3, c.P, device="cuda")
    mm, vv = torch.zeros_like(grad), torch.zeros_like(grad)
    ts, cs = torch.zeros(3, c.spec.n_terms, device="cuda"), torch.zeros(3, len(c.fid), device="cuda")
    for step in range(1, 7):
        if step == 4:
            th.mul_(1.0 + 1e-3)        # a write by torch between iterations: the M packed copies must not be trusted
        assert eng.ensemble_adam_step(c.spec, c.scale, th, c.X, c.n_res, grad, mm, vv, step, _lr(step), T=c.T, out_col=c.fid,
                                      col_scale=c.cscale, term_sums=ts, col_sums=cs)
        for m in range(3):
            assert_member_is_single((ts, cs, grad), m, ref[m][3][step - 1], f"iteration {step}:")
    for m in range(3):
        assert _same(ref[m][0], th[m]) and _same(ref[m][1], mm[m]) and _same(ref[m][2], vv[m]), m
    assert bool(torch.isfinite(th).all()) and float((th - c.theta).abs().max()) > 0


def test_the_lr_sequence_form_and_the_weighted_losses(adam_single_runs):
    c, _ = adam_single_runs
    rows = torch.rand(3, len(c.fid) + c.spec.n_terms, generator=torch.Generator().manual_seed(2)).cuda()
    lrs = [_lr(s) for s in range(1, 7)]
    runs = {}
    for mode in ("steps", "loop"):
        eng = Engine(c.desc)
        th, grad = c.theta.clone(), torch.zeros(3, c.P, device="cuda")
        mm, vv = torch.zeros_like(grad), torch.zeros_like(grad)
        ts, cs = torch.zeros(3, c.spec.n_terms, device="cuda"), torch.zeros(3, len(c.fid), device="cuda")
        losses = torch.zeros(6, 3, 3, device="cuda")
        if mode == "loop":
            assert eng.ensemble_adam_step(c.spec, c.scale, th, c.X, c.n_res, grad, mm, vv, 1, lrs, T=c.T, out_col=c.fid,
                                          col_scale=c.cscale, term_sums=ts, col_sums=cs, loss_rows=rows, losses=losses)
        else:
            for i, lr in enumerate(lrs):
                assert eng.ensemble_adam_step(c.spec, c.scale, th, c.X, c.n_res, grad, mm, vv, 1 + i, lr, T=c.T, out_col=c.fid,
                                              col_scale=c.cscale, term_sums=ts, col_sums=cs, loss_rows=rows, losses=losses[i])
                if i == 5:       # losses (M, rows) = loss_rows @ [col sums | term sums], formed in double by the finishing kernel
                    ref = torch.cat([cs, ts], 1).double() @ rows.double().T
                    assert torch.allclose(losses[5].double(), ref, rtol=1e-6)
        runs[mode] = (th, mm, vv, losses, ts.clone(), cs.clone())
    a, b = runs["steps"], runs["loop"]
    for m in range(3):
        assert _same(a[0][m], b[0][m]) and _same(a[1][m], b[1][m]) and _same(a[2][m], b[2][m]), m
    assert torch.allclose(a[3], b[3], rtol=1e-5)
    ref = torch.cat([b[5], b[4]], 1).double() @ rows.double().T       # the loop's last iteration
    assert torch.allclose(b[3][5].double(), ref, rtol=1e-6)


# ---- 7. refusals launch nothing --------------------------------------------------------------------------------------------------
NS = dict(d_in=3, d_out=4, n_hidden=8, width=64, grad_cols=(0, 1, 2))
PE = dict(d_in=2, d_out=6, n_hidden=10, width=10, grad_cols=(0, 1))
REFUSED = [
    ("generic", dict(PE, engine=_lib.ENGINE_GENERIC), "physics_equation", 255, "GENERIC"),
    ("wide", dict(NS, width=128, engine=_lib.ENGINE_WIDE), "Navier_Stokes", 255, "WIDE"),
    ("coop", dict(NS, engine=_lib.ENGINE_FUSED_COOP), "Navier_Stokes", 255, "FUSED_COOP"),
    ("batch", dict(PE, engine=_lib.ENGINE_FUSED_BATCH), "physics_equation", 255, "FUSED_BATCH"),
    ("bf16", dict(NS, width=128, precision=_lib.PREC_BF16), "Navier_Stokes", 255, "bf16"),
    ("width", dict(NS, width=65), "Navier_Stokes", 255, "width above 64"),
    ("leaky", dict(PE, activation=_lib.ACT_LEAKY_RELU), "physics_equation", 255, "LeakyReLU"),
    ("dropout", dict(NS, dropout_p=0.1), "Navier_Stokes", 255, "dropout"),
    ("corrected", dict(PE), "physics_equation_corrected", 255, "corrected"),
    ("split_w64", dict(NS), "Navier_Stokes", 243, "split"),
]


@pytest.mark.parametrize("name,kw,res,n_res,what", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals_launch_nothing(name, kw, res, n_res, what):
    desc = NetDesc(**kw)
    if res.startswith("physics_equation"):
        spec = ResidualSpec.from_names("physics_equation", ("x", "y"), desc.grad_cols, PE_OUT, corrected=res.endswith("corrected"))
    else:
        spec = ResidualSpec.from_names(res, ("t", "x", "y"), desc.grad_cols, ("h", "z", "u", "v"))
    eng = Engine(desc)
    g = torch.Generator().manual_seed(3)
    M, P, N, nc = 3, desc.n_params, 255, 2
    th = torch.randn(M, P, generator=g).mul_(0.1).cuda()
    X = (torch.rand(N, desc.d_in, generator=g) * 2 - 1).cuda()
    T = torch.rand(N - n_res if n_res < N else 1, nc, generator=g).cuda()
    grad, mm, vv = (torch.full((M, P), 3.0, device="cuda") for _ in range(3))
    before = [t.clone() for t in (th, grad, mm, vv)]
    kw_call = dict(T=T if n_res < N else None, out_col=[0, 1], col_scale=torch.ones(nc, device="cuda"))
    with pytest.raises(PinnError, match=what):
        eng.ensemble_loss_grad(spec, torch.ones(spec.n_terms, device="cuda"), th, X, n_res, grad, **kw_call)
    ok = eng.ensemble_adam_step(spec, torch.ones(spec.n_terms, device="cuda"), th, X, n_res, grad, mm, vv, 1, 1e-3, **kw_call)
    assert ok is False and what in eng.last_error(), eng.last_error()
    ok = eng.ensemble_adam_step(spec, torch.ones(spec.n_terms, device="cuda"), th, X, n_res, grad, mm, vv, 1, [1e-3, 1e-3], **kw_call)
    assert ok is False and what in eng.last_error()
    assert what in eng.ensemble_refusal(spec, M, N, n_res, nc)
    torch.cuda.synchronize()
    for t, b in zip((th, grad, mm, vv), before):
        assert torch.equal(t, b)


def test_k_other_than_2_or_3_and_bad_member_counts_are_refused():
    for gc in ((), (0,)):
        eng = Engine(NetDesc(**dict(PE, grad_cols=gc)))
        with pytest.raises(PinnError, match="k must be 2 or 3"):
            eng.ensemble_plan(3, 255)
        with pytest.raises(PinnError, match="k must be 2 or 3"):
            eng.ensemble_workspace(3, 255)
    eng = Engine(NetDesc(**PE))
    for M in (0, 65536):
        with pytest.raises(PinnError, match="M ="):
            eng.ensemble_plan(M, 255)
    assert eng.ensemble_plan(1, 255)[0] >= 1            # M = 1 is valid
    c = Case("pe10x10_split", 1)
    assert_member_is_single(c.ensemble(Engine(c.desc)), 0, c.single(Engine(c.desc), 0), "M = 1:")


# ---- 8. the trainer -----------------------------------------------------------------------------------------------------------------
def _cmb(adam_it):
    cfg = {k: dict(v) for k, v in CMB.items()}
    cfg["adam_optimizer"] = dict(cfg["adam_optimizer"], max_it=adam_it, learning_rate=1e-3, scheduler_step_size=3)
    cfg["lbfgs_optimizer"] = dict(cfg["lbfgs_optimizer"], max_it=0)
    return cfg


def test_ensemble_trainer_against_single_trainers():
    rs = np.random.RandomState(5)
    Xr = rs.rand(243, 2).astype(np.float32) * 2 - 1
    Xf = rs.rand(12, 2).astype(np.float32) * 2 - 1
    Tf = rs.rand(12, 6).astype(np.float32)
    Tf[:, 0] += 1.0                                      # h + eta_mean away from 0
    cfg, M = _cmb(6), 4
    ens = EnsemblePINN(Xf, Tf, Xr, cfg, M, seeds=(11, 12, 13, 99))
    layers = [2] + [10] * 10 + [6]
    for i, s in enumerate((11, 12, 13, 99)):
        assert torch.equal(ens.theta[i].cpu(), init_flat_params(layers, "xavier", torch.Generator().manual_seed(s)))
    # physics_equation divides by eta_mean + h: a raw initialisation puts points next to that pole, where a last-bit
    # difference of the parameters moves the residual sum by 1e-4 (measured: iteration 5 of member 1, fidelity loss equal
    # to nine digits).  Conditioned as tools/lbfgs_device_latency.py conditions it — written through member(i), so the
    # aliasing is part of what the comparison below rests on.
    for i in range(M):
        last = [mod for mod in ens.member(i).modules() if isinstance(mod, torch.nn.Linear)][-1]
        with torch.no_grad():
            last.weight.mul_(0.25)
            for name, val in (("h", 2.0), ("eta_mean", 0.2), ("Hrms", 0.5), ("k", 1.0)):
                last.bias[PE_OUT.index(name)] = val
    assert float(ens.theta[3, -6]) == 2.0 and float(ens.theta[0, -3]) == pytest.approx(0.2)
    theta0 = ens.theta.clone()
    ens.train_adam(6)
    hist = ens.history
    assert [h[0] for h in hist] == [1, 2, 3, 4, 5, 6] and all(h[k].shape == (M,) for h in hist for k in (1, 2, 3))
    assert ens.iter == 6
    for i in range(M):
        dnn = DNN(layers, 0.0, "xavier").cuda()
        dnn.flat_params().copy_(theta0[i])
        tr = PINN(Xf, Tf, Xr, cfg, dnn=dnn, log_every=1, checkpoint_every=0)
        tr.train_adam(6)
        assert tr._folded_iters == 6
        single = np.array(tr.history)                    # (6, 4): iteration, fidelity, residual, total
        mine = np.array([[h[0], float(h[1][i]), float(h[2][i]), float(h[3][i])] for h in hist])
        assert np.allclose(mine, single, rtol=1e-5, atol=0.0), (i, mine, single)
        assert _same(tr.dnn.flat_params(), ens.theta[i]), i
    # member(i) aliases row i
    d2 = ens.member(2)
    assert d2 is ens.member(2) and d2.flat_params().data_ptr() == ens.theta[2].data_ptr()
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in d2.parameters()]), ens.theta[2])
    keep = ens.theta.clone()
    with torch.no_grad():
        next(d2.parameters()).mul_(2.0)
    assert not torch.equal(ens.theta[2], keep[2]) and torch.equal(ens.theta[[0, 1, 3]], keep[[0, 1, 3]])
    # ... and the next iterations see the write (the packed copies are not trusted)
    ens.train_adam(1)
    assert ens.iter == 7 and bool(torch.isfinite(ens.theta).all())
    # predictions
    grid = rs.rand(37, 2).astype(np.float32) * 2 - 1
    Y = ens.predict(grid)
    assert Y.shape == (M, 37, 6)
    eng = Engine(NetDesc(2, 6, 10, 10, (0, 1)))
    for i in range(M):
        assert torch.equal(Y[i], eng.forward(ens.theta[i].contiguous(), torch.from_numpy(grid).cuda()))
    assert torch.allclose(Y[2], d2(torch.from_numpy(grid).cuda()).detach(), rtol=1e-6, atol=1e-7)   # (the module's own forward path)
    mean, std = ens.predict_stats(grid)
    assert torch.equal(mean, Y.mean(0)) and torch.equal(std, Y.std(0, unbiased=True))
    # an L-BFGS stage of ONE member through the single-network trainer works on the ensemble's own buffer
    cfgl = _cmb(0)
    cfgl["lbfgs_optimizer"] = dict(cfgl["lbfgs_optimizer"], max_it=3, max_evaluation=8)
    keep = ens.theta.clone()
    tr = PINN(Xf, Tf, Xr, cfgl, dnn=ens.member(0), checkpoint_every=0)
    assert tr.theta.data_ptr() == ens.theta[0].data_ptr()
    tr.train()
    assert tr.iter >= 2 and bool(torch.isfinite(ens.theta).all())
    assert not torch.equal(ens.theta[0], keep[0]) and torch.equal(ens.theta[1:], keep[1:])


def test_ensemble_trainer_refusals():
    rs = np.random.RandomState(6)
    Xr = rs.rand(243, 2).astype(np.float32) * 2 - 1
    Xf, Tf = rs.rand(12, 2).astype(np.float32), rs.rand(12, 6).astype(np.float32)
    for change, what in ((dict(layers=dict(CMB["layers"], init_type="kaiming")), "LeakyReLU"),
                         (dict(layers=dict(CMB["layers"], dropout_rate=0.1)), "dropout"),
                         (dict(layers=dict(CMB["layers"], hidden_width=65)), "width above 64"),
                         (dict(layers=dict(CMB["layers"], hidden_width=40)), "split"),
                         (dict(loss=dict(CMB["loss"], corrected_radiation_stress=True)), "corrected")):
        with pytest.raises(PinnError, match=what):
            EnsemblePINN(Xf, Tf, Xr, dict(_cmb(6), **change), 3)
    with pytest.raises(PinnError, match="GENERIC"):
        EnsemblePINN(Xf, Tf, Xr, _cmb(6), 3, engine=_lib.ENGINE_GENERIC)
    with pytest.raises(PinnError, match="seed"):
        EnsemblePINN(Xf, Tf, Xr, _cmb(6), 3, seeds=(1, 1, 2))
    # continuity_only's data-dependent count with one collocation set per member
    co = {
        "layers": {"input_features": 2, "hidden_layers": 4, "hidden_width": 20, "output_features": 3},
        "adam_optimizer": {"max_it": 2, "learning_rate": 1e-3, "scheduler_step_size": 7, "scheduler_gamma": 0.8},
        "lbfgs_optimizer": {"max_it": 0},
        "loss": {"weight_fid_loss": 1, "weight_res_loss": 1},
        "data": {"inputs": {"x": {"requires_grad": ["true"]}, "y": {"requires_grad": ["true"]}}, "trues": ["U", "V"], "unknowns": ["h"]},
    }
    X3 = rs.rand(3, 100, 2).astype(np.float32) * 40
    with pytest.raises(PinnError, match="continuity_only"):
        EnsemblePINN(X3, rs.rand(3, 100, 2).astype(np.float32), X3, co, 3)
    # ... while one shared set trains (both terms on every point, the gradient copies in global memory or LDS as planned)
    X1 = X3[0]
    e = EnsemblePINN(X1, rs.rand(100, 2).astype(np.float32), X1, co, 3)
    e.train_adam(2)
    assert len(e.history) == 2 and bool(torch.isfinite(e.theta).all())
