"""pinn_adam_loop_ext: device-enqueued Adam runs of the residual with runtime coefficients or with point weights (fixed or
self-adaptive).  An iteration is the residual pass, the fidelity pass and ONE finishing kernel; it must give what the
classic sequence gives — mse_loss_grad + residual_coef_loss_grad / residual_weighted_loss_grad + adam_step on theta, on the
coefficients, on lambda through trainer.sa_weight_grad.  What is bit-reproducible in the single entries (term sums,
coefficient gradient, fields — and with them the first coefficient and multiplier step) is compared BIT FOR BIT after the
first iteration, where both runs started from identical inputs; everything else as tests/test_adam_fold_gpu.py compares two
tile-kernel runs (a workgroup's gradient copy is added to in lock order: run-to-run differences of ~1e-6)."""
import numpy as np
import pytest
import torch

from oracle import pinn_oracle as O          # parameter initialisation only
from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec
from pinn_depthestimation_amd._lib import ENGINE_FUSED_BATCH, ENGINE_FUSED_COOP, ENGINE_GENERIC, PREC_BF16
from pinn_depthestimation_amd.trainer import PINN, sa_weight_grad, sa_weights
from tests import fold_ext_util as F

pytestmark = pytest.mark.gpu

PE_OUT = ("h", "U", "V", "eta_mean", "Hrms", "k")
SHAPES = {
    # d_in, d_out, hidden layers, width, grad_cols, residual, inputs, outputs, fidelity columns
    "pe10x10": (2, 6, 10, 10, (0, 1), "physics_equation", ("x", "y"), PE_OUT, (0, 1, 2, 3, 4, 5)),      # WP 16, P = 1086
    "ns8x64": (3, 4, 8, 64, (0, 1, 2), "Navier_Stokes", ("t", "x", "y"), ("h", "z", "u", "v"), (2, 3)),  # WP 64, copy in LDS
    "co100x20": (2, 3, 100, 20, (0, 1), "continuity_only", ("x", "y"), ("U", "V", "h"), (0, 1)),         # copies in the workspace
}
POINTS = (1, 15, 16, 17, 243, 4099)
FID_KINDS = ("none", "12", "alias")
COEF0 = {"physics_equation": 0.05, "Navier_Stokes": 0.6}
# mode: what rides with the network — "coef" a trainable coefficient; "wfix" fixed weights (one row); "sa_square" multipliers
# with a row per term, w = lambda^2; "sa_linear1" one shared row, w = lambda
MODES = ("coef", "wfix", "sa_square", "sa_linear1")


def lr_of(step):
    return 1e-3 * 0.8 ** (step // 3)          # the network's; the coefficient's is 5 x, the multipliers' 2 x this


def setup(shape, n_res, fid_kind, seed=77):
    d_in, d_out, L, W, gc, res, inn, outn, fid = SHAPES[shape]
    g = torch.Generator().manual_seed(seed + n_res)
    params = O.init_params(O.layer_sizes(d_in, L, W, d_out), "xavier", g)
    if res == "physics_equation":
        params[-1][outn.index("h")] = 0.75; params[-1][outn.index("eta_mean")] = 0.0
    desc = NetDesc(d_in, d_out, L, W, gc)
    spec = ResidualSpec.from_names(res, inn, desc.grad_cols, outn)
    X = (torch.rand(n_res, d_in, generator=g) * 2 - 1).cuda()
    Xf = None if fid_kind == "none" else (X if fid_kind == "alias" else (torch.rand(12, d_in, generator=g) * 2 - 1).cuda())
    nf = 0 if Xf is None else Xf.shape[0]
    T = torch.rand(nf, len(fid), generator=g).cuda() if nf else None
    return dict(desc=desc, spec=spec, flat0=O.flatten(params).cuda(), X=X, Xf=Xf, T=T, fid=list(fid), res=res,
                scale=(torch.tensor([0.7, 1.3, 0.9][:spec.n_terms]) / n_res).cuda(),
                cscale=torch.full((len(fid),), 1.0 / max(nf, 1)).cuda(), gen=g)


def state(c, mode, frozen=False):
    """The tensors one run owns: theta, moments, gradient, sums and the mode's own."""
    P, spec, N = c["flat0"].numel(), c["spec"], c["X"].shape[0]
    z = lambda *s: torch.zeros(*s, device="cuda")
    st = dict(th=c["flat0"].clone(), m=z(P), v=z(P), grad=z(P), ts=z(spec.n_terms), cs=z(len(c["fid"])))
    g = torch.Generator().manual_seed(5)
    if mode == "coef":
        st.update(coef=torch.tensor([COEF0[c["res"]]], device="cuda"), cm=z(1), cv=z(1), cg=None if frozen else z(1))
    else:
        rows = 1 if mode in ("wfix", "sa_linear1") else spec.n_weighted_terms
        st.update(w=(0.5 + torch.rand(rows, N, generator=g)).cuda(), fields=z(spec.n_fields, N))
        if mode.startswith("sa"):
            st.update(lam=st["w"].clone(), lm=z(rows, N), lv=z(rows, N), mask="square" if mode == "sa_square" else "linear")
            st["w"] = sa_weights(st["lam"], st["mask"]).contiguous()
    return st


def classic_iteration(eng, c, st, step):
    """One iteration of the path the trainer takes without fold_extras."""
    lr, spec = lr_of(step), c["spec"]
    st["grad"].zero_()
    if c["Xf"] is not None:
        eng.mse_loss_grad(st["th"], c["Xf"], c["T"], c["fid"], c["cscale"], st["grad"], sums=st["cs"])
    else:
        st["cs"].zero_()
    if "coef" in st:
        if st["cg"] is not None:
            st["cg"].zero_()
        eng.residual_coef_loss_grad(spec, st["coef"], c["scale"], st["th"], c["X"], st["grad"], st["cg"], sums=st["ts"])
    else:
        if "lam" in st:
            st["w"].copy_(sa_weights(st["lam"], st["mask"]))
        eng.residual_weighted_loss_grad(spec, st["w"], c["scale"], st["th"], c["X"], st["grad"], sums=st["ts"], fields=st["fields"])
    eng.adam_step(st["th"], st["grad"], st["m"], st["v"], step, lr)
    if st.get("cg") is not None:
        eng.adam_step(st["coef"], st["cg"], st["cm"], st["cv"], step, 5 * lr, count=1)
    if "lam" in st:
        g = sa_weight_grad(st["lam"], st["fields"], c["scale"], st["mask"]).contiguous()
        eng.adam_step(st["lam"].view(-1), g.view(-1), st["lm"].view(-1), st["lv"].view(-1), step, 2 * lr, count=st["lam"].numel())


def ext_run(eng, c, st, step0, n, **kw):
    """n iterations by ONE call, steps step0 .. step0 + n - 1."""
    steps = range(step0, step0 + n)
    a = dict(Xf=c["Xf"], T=c["T"], out_col=c["fid"], col_scale=c["cscale"], term_sums=st["ts"], col_sums=st["cs"])
    if "coef" in st:
        a.update(coef=st["coef"], coef_m=st["cm"], coef_v=st["cv"], coef_grad=st["cg"], lr_coef=[5 * lr_of(s) for s in steps])
    else:
        a.update(point_w=st["w"], fields=st["fields"])
        if "lam" in st:
            a.update(lam=st["lam"], lam_m=st["lm"], lam_v=st["lv"], sa_mask=st["mask"], lr_w=[2 * lr_of(s) for s in steps])
    a.update(kw)
    return eng.adam_loop_ext(c["spec"], c["scale"], st["th"], c["X"], st["grad"], st["m"], st["v"], step0,
                             [lr_of(s) for s in steps], **a)


def snap(st):
    out = {k: v.clone() for k, v in st.items() if torch.is_tensor(v)}
    if "lam" in st:      # the weights of the NEXT pass: the folded run has written them, the classic one forms them then
        out["w_next"] = sa_weights(st["lam"], st["mask"]).contiguous()
    return out


SUMS, EXACT_FIRST = ("ts", "cs"), ("ts", "cg", "fields", "coef", "cm", "cv")
EXACT_FIRST_PER_TERM = ("lam", "lm", "lv", "w_next")
STATE = ("th", "m", "v", "coef", "cm", "cv", "lam", "lm", "lv", "w_next")


def compare(a, b, first, per_term, what):
    """a: classic, b: folded (snapshots).  first: both runs started this iteration from identical inputs."""
    exact = (EXACT_FIRST + (EXACT_FIRST_PER_TERM if per_term else ())) if first else ()
    b = dict(b)
    if "lam" in b:
        b["w_next"] = b["w"]
    for k in exact:
        if k in a:
            assert torch.equal(a[k], b[k]), f"{what}: {k} is not bit-identical (max diff {float((a[k] - b[k]).abs().max()):.3e})"
    for k in SUMS:
        assert torch.allclose(a[k], b[k], rtol=1e-5, atol=0), f"{what}: {k} {a[k].tolist()} vs {b[k].tolist()}"
    if "cg" in a:
        assert torch.allclose(a["cg"], b["cg"], rtol=1e-5, atol=1e-7 * float(a["cg"].abs().max())), f"{what}: coef_grad"
    if "fields" in a:
        assert F.rel_l2(b["fields"], a["fields"]) < 5e-6, f"{what}: fields"
    rel = F.rel_l2(b["grad"], a["grad"])
    assert rel < 5e-6, f"{what}: gradient rel-L2 {rel:.2e}"
    for k in STATE:
        if k in a:
            assert F.close(b[k], a[k]), f"{what}: {k} (max diff {float((a[k] - b[k]).abs().max()):.3e} of {float(a[k].abs().max()):.3e})"
    assert all(bool(torch.isfinite(v).all()) for v in b.values())


def cases():
    out = []
    for shape in ("pe10x10", "ns8x64"):
        for im, mode in enumerate(MODES):
            for ip, n in enumerate(POINTS):
                out.append((shape, mode, n, FID_KINDS[(im + ip) % 3]))
    for im, mode in enumerate(MODES[1:]):
        out.append(("co100x20", mode, 1251, ("alias", "12", "alias")[im]))
    return out


@pytest.mark.parametrize("shape,mode,n_res,fid_kind", cases())
def test_runs_in_pieces_are_the_classic_sequence(shape, mode, n_res, fid_kind):
    """Six iterations, the learning rate changing at step 3 and a write by torch before step 4; the folded run in calls of
    1, 2 and 3 iterations (the second and third on the packed weights of the one before, the third after the write)."""
    c = setup(shape, n_res, fid_kind)
    per_term = mode != "sa_linear1"       # a shared row sums the terms: torch's order over them is not promised
    ea, eb = Engine(c["desc"]), Engine(c["desc"])
    a, b = state(c, mode), state(c, mode)
    ends, step = {}, 1
    for step in range(1, 7):
        if step == 4:
            a["th"].mul_(1.0 + 1e-3)
        classic_iteration(ea, c, a, step)
        if step in (1, 3, 6):
            ends[step] = snap(a)
    step = 1
    for n in (1, 2, 3):
        if step == 4:
            b["th"].mul_(1.0 + 1e-3)       # the packed copy must not be trusted after it
        assert ext_run(eb, c, b, step, n), eb.last_error()
        step += n
        torch.cuda.synchronize()
        compare(ends[step - 1], snap(b), first=step == 2, per_term=per_term, what=f"{shape} {mode} N={n_res} fid={fid_kind} after iteration {step - 1}")
    assert float((b["th"] - c["flat0"]).abs().max()) > 0
    if mode == "wfix":
        assert torch.equal(b["w"], state(c, mode)["w"])          # fixed weights are read only
    if mode.startswith("sa"):
        # ... and the first multiplier step is the NumPy restatement of the kernel (tests/test_fold_ext_cpu.py holds it to
        # sa_weight_grad + torch.optim.Adam) from the first pass's fields, bit for bit for a row per term
        s0 = state(c, mode)
        lam1 = F.multiplier_step(s0["lam"].cpu().numpy(), s0["lm"].cpu().numpy(), s0["lv"].cpu().numpy(),
                                 ends[1]["fields"].cpu().numpy(), c["scale"].cpu().numpy(), s0["mask"], 2 * lr_of(1), 1)[0]
        if per_term:
            assert np.array_equal(lam1, ends[1]["lam"].cpu().numpy())
        else:
            assert np.allclose(lam1, ends[1]["lam"].cpu().numpy(), rtol=2e-4, atol=0)


@pytest.mark.parametrize("fid_kind", ["12", "none"])
def test_coef_log_and_losses(fid_kind):
    """coef_log row i is the coefficient iteration i ran with; losses row i is loss_rows @ [col sums | term sums] of iteration
    i in double, also without fidelity points, where the caller's n_cols is still the stride of loss_rows."""
    c = setup("pe10x10", 243, fid_kind)
    nc, nt, K = len(c["fid"]), c["spec"].n_terms, 4
    rows = torch.rand(3, nc + nt, generator=torch.Generator().manual_seed(2)).cuda()
    # run A: K iterations by one call
    ea, a = Engine(c["desc"]), state(c, "coef")
    log, losses = torch.full((K, 1), -1.0, device="cuda"), torch.full((K, 3), -1.0, device="cuda")
    assert ext_run(ea, c, a, 1, K, coef_log=log, loss_rows=rows, losses=losses)
    # run B: one iteration per call, the coefficient read before each
    eb, b = Engine(c["desc"]), state(c, "coef")
    before = []
    for step in range(1, K + 1):
        before.append(b["coef"].clone())
        one = torch.zeros(1, 3, device="cuda")
        assert ext_run(eb, c, b, step, 1, loss_rows=rows, losses=one)
        ref = rows.double() @ torch.cat([b["cs"], b["ts"]]).double()
        assert torch.allclose(one[0].double(), ref, rtol=1e-6, atol=0), (step, one, ref)
        assert torch.allclose(losses[step - 1], one[0], rtol=1e-5, atol=0)
        if fid_kind == "none":
            assert float(b["cs"].abs().max()) == 0.0        # zeroed, and their columns of loss_rows weigh nothing
    before = torch.stack(before)
    assert torch.equal(log[0], before[0]) and F.close(log, before), (log, before)
    assert float((log[-1] - log[0]).abs()) > 0 and not torch.equal(a["coef"], log[-1])
    ref = rows.double() @ torch.cat([a["cs"], a["ts"]]).double()
    assert torch.allclose(losses[-1].double(), ref, rtol=1e-6, atol=0)


@pytest.mark.parametrize("shape,mode,fid_kind", [("pe10x10", "coef", "12"), ("ns8x64", "sa_square", "alias"), ("co100x20", "sa_linear1", "12"),
                                                 ("pe10x10", "wfix", "none")])
def test_buffer_contract(shape, mode, fid_kind):
    """A workspace full of NaN and a gradient full of NaN on entry: finite results equal to a clean run's; guard bands around
    the coefficient, the multipliers, the weights and the fields untouched."""
    n_res = 1251 if shape == "co100x20" else 243
    c = setup(shape, n_res, fid_kind)
    ec, clean = Engine(c["desc"]), state(c, mode)
    assert ext_run(ec, c, clean, 1, 3)
    G = 64
    eng, st = Engine(c["desc"]), state(c, mode)
    assert ext_run(eng, c, state(c, mode), 1, 1)          # (allocates the engine's workspace)
    ws = eng._ws["adamext"]
    ws[:ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    eng.invalidate_packed()
    bands = {}
    for k in ("coef", "cm", "cv", "cg", "lam", "lm", "lv", "w", "fields"):
        if st.get(k) is not None:
            buf = torch.full((st[k].numel() + 2 * G,), 7.25, device="cuda")
            view = buf[G:G + st[k].numel()].view(st[k].shape)
            view.copy_(st[k])
            bands[k], st[k] = buf, view
    st["grad"].fill_(float("nan"))
    assert ext_run(eng, c, st, 1, 3)
    torch.cuda.synchronize()
    compare(snap(clean), snap(st), first=False, per_term=False, what=f"{shape} {mode} dirty buffers")
    for k, buf in bands.items():
        assert bool((buf[:G] == 7.25).all()) and bool((buf[-G:] == 7.25).all()), f"guard band of {k} written"


def test_frozen_cases():
    c = setup("pe10x10", 243, "12")
    # coef_grad = None: values only
    eng, st = Engine(c["desc"]), state(c, "coef", frozen=True)
    c0 = st["coef"].clone()
    log = torch.zeros(3, 1, device="cuda")
    assert ext_run(eng, c, st, 1, 3, coef_log=log)
    assert torch.equal(st["coef"], c0) and torch.equal(log, c0.expand(3, 1)) and float((st["th"] - c["flat0"]).abs().max()) > 0
    assert float(st["cm"].abs().max()) == 0.0 and float(st["cv"].abs().max()) == 0.0
    # a 0 mask entry: gradient 0, no movement
    eng, st = Engine(c["desc"]), state(c, "coef")
    assert ext_run(eng, c, st, 1, 3, coef_mask=torch.zeros(1, device="cuda"))
    assert torch.equal(st["coef"], c0) and float(st["cg"].abs().max()) == 0.0
    # ... and a 1 entry is no mask at all
    e1, s1 = Engine(c["desc"]), state(c, "coef")
    e2, s2 = Engine(c["desc"]), state(c, "coef")
    assert ext_run(e1, c, s1, 1, 1, coef_mask=torch.ones(1, device="cuda")) and ext_run(e2, c, s2, 1, 1)
    assert torch.equal(s1["coef"], s2["coef"]) and torch.equal(s1["cg"], s2["cg"]) and not torch.equal(s1["coef"], c0)
    # fixed weights are read only
    for mode in ("wfix",):
        eng, st = Engine(c["desc"]), state(c, mode)
        w0 = st["w"].clone()
        assert ext_run(eng, c, st, 1, 3)
        assert torch.equal(st["w"], w0) and float(st["fields"].abs().max()) > 0


def test_refusals_launch_nothing():
    c = setup("pe10x10", 243, "12")
    pec = ResidualSpec.from_names("physics_equation", ("x", "y"), c["desc"].grad_cols, PE_OUT, corrected=True)
    for what, desc, spec, mode in (("generic", c["desc"].with_(engine=ENGINE_GENERIC), c["spec"], "coef"),
                                   ("coop", c["desc"].with_(engine=ENGINE_FUSED_COOP), c["spec"], "sa_square"),
                                   ("batch", c["desc"].with_(engine=ENGINE_FUSED_BATCH), c["spec"], "wfix"),
                                   ("bf16", c["desc"].with_(precision=PREC_BF16), c["spec"], "coef"),
                                   ("corrected", c["desc"], pec, "sa_linear1")):
        eng, st = Engine(desc), state(c, mode)
        st["grad"].fill_(3.0)
        keep = snap(st)
        assert ext_run(eng, dict(c, spec=spec), st, 1, 3) is False, what
        torch.cuda.synchronize()
        for k, v in snap(st).items():
            assert torch.equal(v, keep[k]), (what, k)
        assert eng.last_error()
    # both groups: no kernel carries both
    eng, st = Engine(c["desc"]), state(c, "coef")
    w = torch.ones(243, device="cuda")
    assert ext_run(eng, c, st, 1, 1, point_w=w) is False and "both" in eng.last_error()
    assert torch.equal(st["th"], c["flat0"])


def test_packed_weights_are_not_trusted_after_another_call_on_the_engine():
    """Between two runs another call on the engine may re-pack a workspace from ITS parameters (here the run's own workspace
    is overwritten as such a call would): the next run must pack again."""
    c = setup("ns8x64", 243, "12")
    out = []
    for disturb in (False, True):
        eng, st = Engine(c["desc"]), state(c, "coef")
        for step in (1, 2, 3):
            assert ext_run(eng, c, st, step, 1)
            if disturb:
                eng.forward(torch.zeros_like(st["th"]), c["X"])            # someone else's parameters through the same engine
                ws = eng._ws["adamext"]
                ws[:ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
        out.append(snap(st))
    compare(out[0], out[1], first=False, per_term=False, what="re-packed")


# ---- the trainer --------------------------------------------------------------------------------------------------------------
def test_trainer_learns_cd_in_device_enqueued_runs(tmp_path):
    """The trajectory test of tests/test_coef_gpu.py (its problem, fp64 loop and bounds: max(1e-5, 4 x the fp32 twin's gap))
    with fold_extras on: every iteration folded."""
    params, Xf, Tf, Xr = F.trainer_data("coef")
    l64, c64 = F.cd_loop(params, Xf, Tf, Xr, 0.05, torch.float64)
    l32, c32 = F.cd_loop(params, Xf, Tf, Xr, 0.05, torch.float32)
    tr = PINN(Xf.numpy(), Tf.numpy(), Xr.numpy(), F.trainer_cfg("coef", lbfgs_it=4), dnn=F.trainer_model("coef", params), log_every=1, checkpoint_every=0,
              log_dir=str(tmp_path), coefficients={"Cd": 0.05}, trainable_coefficients=("Cd",), lbfgs_impl="flat", fold_extras=True)
    assert tr.fold_extras and tr.fold_extras_why is None
    tr.train_adam(F.ITERS)
    assert tr._folded_iters == F.ITERS and tr.iter == F.ITERS and tr._adam_step == F.ITERS
    got = np.array([h[3] for h in tr.history])
    cds = np.array([r[1] for r in tr._coef_history])
    assert got.shape == (F.ITERS,) and cds.shape == (F.ITERS,)
    gap_l = np.maximum.accumulate(np.abs(l32 - l64) / np.abs(l64))
    gap_c = np.maximum.accumulate(np.abs(c32 - c64) / np.abs(c64))
    rel_l, rel_c = np.abs(got - l64) / np.abs(l64), np.abs(cds - c64) / np.abs(c64)
    tol_l, tol_c = np.maximum(1e-5, 4 * gap_l), np.maximum(1e-5, 4 * gap_c)
    print(f"folded trainable Cd: loss max rel err {rel_l.max():.2e} (worst over its bound {(rel_l / tol_l).max():.3f}); Cd max rel err "
          f"{rel_c.max():.2e} (worst over its bound {(rel_c / tol_c).max():.3f}); Cd {cds[0]:.6f} -> {tr.coefficients()['Cd']:.6f}")
    assert (rel_l < tol_l).all(), (int(np.argmax(rel_l / tol_l)), rel_l.max())
    assert (rel_c < tol_c).all(), (int(np.argmax(rel_c / tol_c)), rel_c.max())
    assert cds[0] == np.float32(0.05)
    after_adam = tr.coefficients()
    assert abs(after_adam["Cd"] - 0.05) > 1e-3
    tr.flush_log()
    lines = open(tmp_path / "log.txt").read().splitlines()
    assert lines[0].endswith(", Cd") and len(lines) == 1 + F.ITERS and all(len(ln.split(", ")) == 5 for ln in lines[1:])
    loss_before = float(tr.last[2])
    tr.optimizer_LBFGS.step(tr.closure)
    torch.cuda.synchronize()
    assert tr.iter > F.ITERS and tr.coefficients() == after_adam
    assert np.isfinite(float(tr.last[2])) and float(tr.last[2]) <= loss_before


@pytest.mark.parametrize("mask", ["square", "linear"])
def test_trainer_self_adaptive_in_device_enqueued_runs(mask):
    """The self-adaptive test of tests/test_weighted_gpu.py (its problem, fp64 loop and bounds) with fold_extras on."""
    params, Xf, Tf, Xr = F.trainer_data("weights")
    l64, lam64 = F.sa_loop(params, Xf, Tf, Xr, mask, torch.float64)
    l32, lam32 = F.sa_loop(params, Xf, Tf, Xr, mask, torch.float32)
    tr = PINN(Xf.numpy(), Tf.numpy(), Xr.numpy(), F.trainer_cfg("weights", lbfgs_it=4), dnn=F.trainer_model("weights", params), log_every=1, checkpoint_every=0,
              self_adaptive={"mask": mask}, lbfgs_impl="flat", fold_extras=True)
    tr.train_adam(F.ITERS)
    assert tr._folded_iters == F.ITERS and tr.iter == F.ITERS
    got = np.array([h[3] for h in tr.history])
    lam = tr._lam.detach().cpu().double()
    gap_l = np.maximum.accumulate(np.abs(l32 - l64) / np.abs(l64))
    rel_l = np.abs(got - l64) / np.abs(l64)
    tol_l = np.maximum(1e-5, 4 * gap_l)
    gap_lam = float(((lam32.double() - lam64).abs() / lam64.abs()).max())
    rel_lam = float(((lam - lam64).abs() / lam64.abs()).max())
    tol_lam = max(1e-5, 4 * gap_lam)
    print(f"folded self-adaptive {mask}: loss max rel err {rel_l.max():.2e} (worst over its bound {(rel_l / tol_l).max():.3f}); lambda max "
          f"rel err {rel_lam:.2e} (bound {tol_lam:.2e})")
    assert (rel_l < tol_l).all(), (int(np.argmax(rel_l / tol_l)), rel_l.max())
    assert rel_lam < tol_lam, (rel_lam, tol_lam)
    w = tr._lam * tr._lam if mask == "square" else tr._lam
    assert torch.equal(tr.residual_weights(), w) and torch.equal(tr._w_fixed, w)      # the device left m(lambda) for the next pass
    lam_before = tr._lam.clone()
    tr.optimizer_LBFGS.step(tr.closure)
    torch.cuda.synchronize()
    assert tr.iter > F.ITERS and torch.equal(tr._lam, lam_before)


def _trainer(kind, tmp, **kw):
    prob = "coef" if kind == "coef" else "weights"
    params, Xf, Tf, Xr = F.trainer_data(prob)
    extra = {"coef": dict(coefficients={"Cd": 0.05}, trainable_coefficients=("Cd",)),
             "sa": dict(self_adaptive={"mask": "square"}),
             "wfix": dict(residual_weights=0.5 + np.random.RandomState(3).rand(3, Xr.shape[0]).astype(np.float32))}[kind]
    torch.manual_seed(1234)
    return PINN(Xf.numpy(), Tf.numpy(), Xr.numpy(), F.trainer_cfg(prob), dnn=F.trainer_model(prob, params), log_dir=str(tmp), **extra, **kw), F.ITERS


@pytest.mark.parametrize("kind", ["coef", "sa", "wfix"])
def test_trainer_with_and_without_fold_extras(kind, tmp_path):
    """The folded trainer against the classic one, held to what two classic trainers hold each other to: the larger of 1e-5
    (tests/test_coef_gpu.py: test_fixed_default_cd_walks_the_trainer_s_own_trajectory) and 4 x their own spread in the logged
    totals.  Then log_every = 7 with checkpoints inside the run: the same iterations logged, the checkpoint iterations on the
    classic path."""
    tot = []
    for i in range(2):
        tr, iters = _trainer(kind, tmp_path / f"c{i}", log_every=1, checkpoint_every=0)
        tr.train_adam(iters)
        assert tr._folded_iters == 0
        tot.append(np.array([h[3] for h in tr.history]))
    classic_state = (tr.coefficients(), None if tr.residual_weights() is None else tr.residual_weights().clone())
    spread = float((np.abs(tot[1] - tot[0]) / np.abs(tot[0])).max())
    bound = max(1e-5, 4 * spread)
    tr, iters = _trainer(kind, tmp_path / "f", log_every=1, checkpoint_every=0, fold_extras=True)
    tr.train_adam(iters)
    assert tr._folded_iters == iters
    got = np.array([h[3] for h in tr.history])
    rel = float((np.abs(got - tot[0]) / np.abs(tot[0])).max())
    print(f"{kind}: folded against classic: max rel err of the logged totals {rel:.2e}; two classic trainers: {spread:.2e}; bound {bound:.2e}")
    assert got.shape == tot[0].shape and rel <= bound
    if kind == "coef":
        assert abs(tr.coefficients()["Cd"] - classic_state[0]["Cd"]) <= 2e-4 * abs(classic_state[0]["Cd"])
    else:
        assert F.close(tr.residual_weights(), classic_state[1])
    # log_every = 7, checkpoints at 10 and 20: runs of 9 iterations between them
    tr, iters = _trainer(kind, tmp_path / "g", log_every=7, checkpoint_every=10, fold_extras=True)
    tr.train_adam(iters)
    assert tr.iter == iters and tr._folded_iters == iters - iters // 10
    hist = tr.history
    assert [h[0] for h in hist] == [it for it in range(1, iters + 1) if it % 7 == 0]
    for h in hist:
        assert abs(h[3] - tot[0][h[0] - 1]) <= bound * abs(tot[0][h[0] - 1]), h
    if kind == "coef":
        assert [r[0] for r in tr._coef_history] == [h[0] for h in hist]
        import json
        saved = json.load(open(tmp_path / "g" / "coefficients.json"))
        assert saved["iteration"] == iters and saved["trainable"] == ["Cd"]
