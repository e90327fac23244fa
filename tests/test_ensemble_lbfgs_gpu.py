"""The device-resident L-BFGS loop of an ensemble (pinn_ensemble_lbfgs_loop, lbfgs.EnsembleDeviceLBFGS,
EnsemblePINN(lbfgs_stage=True)) on the GPU: member j must be what the single loop (lbfgs.DeviceLBFGS) is on row j.

Shapes.  "one tile": 2 -> 10 x 10 -> 6, physics_equation on 12 collocation + 4 fidelity points, one workgroup with one
working wave per member: there the ensemble pass gives the bits of the single call (tests/test_ensemble_gpu.py), so every
comparison is bit for bit.  "split": 243 + 12 points, several workgroups per member: the pass's gradient adds are
lock-ordered, so the comparison is tests/test_lbfgs_loop_gpu.py's compare_drivers, per member.  Weights are
pe_corrected_util.conditioned_params with seed SEED + j for member j.  Every test prints what it measured."""
import ctypes as C

import numpy as np
import pytest
import torch

from pinn_depthestimation_amd import EnsemblePINN, _lib
from pinn_depthestimation_amd._lib import (ENGINE_AUTO, ENGINE_FUSED_TILE, LBFGS_ACT_ACCEPT, LBFGS_ACT_CONTINUE, LBFGS_ACT_INERT,
                                           LBFGS_ACT_INITIAL, LBFGS_TRACE_COLS, PinnError)
from pinn_depthestimation_amd.dnn import DNN
from pinn_depthestimation_amd.engine import Engine, NetDesc, ResidualSpec, _out_cols, _ptr
from pinn_depthestimation_amd.lbfgs import EnsembleDeviceLBFGS, FlatLBFGS
from pinn_depthestimation_amd.trainer import PINN
from tests.abi_contract_util import assert_unchanged, guarded, poison_workspace, snapshot
from tests.golden_util import CMB
from tests.pe_corrected_util import ROLES, points
from tests.test_ensemble_gpu import PE, REFUSED, _same
from tests.test_lbfgs_loop_gpu import DEV, OPTS, eval_iterations, pe_problem, rel

pytestmark = pytest.mark.gpu

SEED = 3          # member j's weights: conditioned_params(seed = SEED + j); the tests assert what the seed must satisfy
ONE_TILE = dict(n_res=12, n_fid=4)
SPLIT = dict(n_res=243, n_fid=12)


class Ens:
    """M problems of tests/test_lbfgs_loop_gpu.py (member j: weights of seed SEED + j) on one point set — member 0's X
    and T — or, own_x / own_t, on member j's own (X: points(seed = 1 + j); T: drawn around member j's output biases)."""

    def __init__(self, M, shape, engine=ENGINE_AUTO, own_x=False, own_t=False, seed=SEED):
        self.pbs = [pe_problem(engine, seed=seed + j, **shape) for j in range(M)]
        p0 = self.pbs[0]
        for j, pb in enumerate(self.pbs):
            pb.X = points(pb.n_res + pb.n_fid, 2, seed=1 + j).to(DEV).contiguous() if own_x else p0.X
            pb.T = pb.T if own_t else p0.T
        self.M, self.eng, self.spec = M, p0.eng, p0.spec
        self.theta0 = torch.stack([pb.theta0 for pb in self.pbs]).contiguous()
        self.X = torch.stack([pb.X for pb in self.pbs]).contiguous() if own_x else p0.X
        self.T = torch.stack([pb.T for pb in self.pbs]).contiguous() if own_t else p0.T
        self.N = p0.n_res + p0.n_fid

    def device(self, theta=None, **kw):
        p0 = self.pbs[0]
        theta = self.theta0.clone() if theta is None else theta
        return EnsembleDeviceLBFGS(self.eng, self.spec, theta, self.X, p0.n_res, p0.res_scale, p0.loss_rows, 2, T=self.T,
                                   out_col=p0.fid_cols, col_scale=p0.fid_scale, **{**OPTS, **kw})

    def single(self, j, theta=None, **kw):
        """lbfgs.DeviceLBFGS on row j (a copy), member j's point set."""
        return self.pbs[j].device(theta=(self.theta0[j] if theta is None else theta).clone(), **kw)


def ctrl_fields(c, skip=()):
    """A control block field by field, the line-search state's fields included: {name: repr(value)} (repr: NaN == NaN)."""
    out = {}
    for name, _ in c._fields_:
        v = getattr(c, name)
        if isinstance(v, C.Structure):
            out.update({f"{name}.{k}": r for k, r in ctrl_fields(v).items()})
        else:
            out[name] = repr(list(v)) if isinstance(v, C.Array) else repr(v)
    return {k: v for k, v in out.items() if k not in skip}


def assert_member_is_single(ens_opt, j, one, what="", slots=None):
    """Bit for bit: trace slice, row j of params, control block j."""
    tr_e, tr_s = ens_opt.trace[:, j, :], one.trace
    if slots is not None:
        tr_e, tr_s = tr_e[:slots], tr_s[:slots]
    assert torch.equal(tr_e.nan_to_num(nan=-7.0), tr_s.nan_to_num(nan=-7.0)), f"{what} member {j}: traces differ"
    assert torch.equal(ens_opt.params[j].nan_to_num(nan=-7.0), one.params.nan_to_num(nan=-7.0)), f"{what} member {j}: params differ"
    a, b = ctrl_fields(ens_opt.ctrls()[j]), ctrl_fields(one.ctrl())
    assert a == b, f"{what} member {j}: control blocks differ: {[(k, a[k], b[k]) for k in a if a[k] != b[k]]}"


def searches_that_zoom(trace):
    """Line searches of one member's trace in which a later trial step is SMALLER than an earlier one: the bracketing phase
    only extrapolates, so the search went into its zoom phase."""
    n, last = 0, None
    zoomed = False
    for row in trace.tolist():
        act = int(row[2])
        if act == LBFGS_ACT_CONTINUE or act == LBFGS_ACT_ACCEPT:
            if last is not None and row[3] < last:
                zoomed = True
            last = row[3]
        if act in (LBFGS_ACT_ACCEPT, LBFGS_ACT_INITIAL, LBFGS_ACT_INERT):
            n, last, zoomed = n + int(zoomed), None, False
    return n


# ---- 1. one tile, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lr", [1.0, 6.0], ids=["lr=1", "lr=6"])
def test_one_tile_members_are_the_single_loop_bit_for_bit(lr):
    e = Ens(5, ONE_TILE)
    assert e.eng.ensemble_plan(5, e.N) == (1, True) and e.N == 16
    opt = e.device(lr=lr, history_size=3)
    opt.run(48)
    tr = opt.trace
    acts = tr[:, :, 2]
    differ = int((acts != acts[:, :1]).any(dim=1).sum())
    wrapped = [j for j, c in enumerate(opt.ctrls()) if c.k == c.m == 3 and int((acts[:, j] == LBFGS_ACT_ACCEPT).sum()) > 3 and c.head != 0]
    zooms = [searches_that_zoom(tr[:, j, :]) for j in range(5)]
    print(f"lr = {lr}: evaluations {opt.func_evals}, iterations {opt.n_iter}; slots in which two members' actions differ {differ}; "
          f"members whose ring has wrapped {wrapped}; searches that zoom per member {zooms}")
    # conditions on the input
    assert differ >= 1, "every member took the same action in every slot: pick another seed"
    assert wrapped, "no member's ring has wrapped: pick another seed"
    if lr == 6.0:
        assert sum(zooms) >= 1, "no search zooms: pick another seed"
    for j in range(5):
        one = e.single(j, lr=lr, history_size=3)
        one.run(48)
        assert_member_is_single(opt, j, one, f"lr = {lr}:")
    assert not torch.equal(opt.params, e.theta0) and bool(torch.isfinite(opt.params).all())


# ---- 2. several workgroups per member --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("history", [100, 3])
def test_several_workgroups_per_member(history):
    M = 4
    e = Ens(M, SPLIT, engine=ENGINE_FUSED_TILE)
    gx, _ = e.eng.ensemble_plan(M, e.N)
    assert gx > 1, gx
    kw = dict(max_iter=8, history_size=history)
    opt = e.device(**kw).step()
    for j in range(M):
        pb = e.pbs[j]
        th_f, it_f = pb.host(FlatLBFGS, **kw)
        one = pb.device(**kw).step()
        it_s = eval_iterations(one.trace)
        assert it_f == it_s, f"member {j}: flat and the single device loop disagree on this input, pick another seed: {it_f} vs {it_s}"
        floor = rel(one.params, th_f)
        it_e, dist = eval_iterations(opt.trace[:, j, :]), rel(opt.params[j], one.params)
        print(f"history {history}, member {j}: {len(it_s)} evaluations, {opt.n_iter[j]} iterations, stop '{opt.stop_reason[j]}'; floor "
              f"(flat vs single device) {floor:.2e}, ensemble vs single device {dist:.2e}, bar {max(4 * floor, 1e-6):.2e}")
        assert it_e == it_s, (j, it_e, it_s)
        assert dist <= max(4 * floor, 1e-6), (j, dist, floor)
        assert opt.n_iter[j] == one.n_iter and opt.stop_reason[j] == one.stop_reason


# ---- 3. members stop at different slots --------------------------------------------------------------------------------------------
def test_members_stop_at_different_slots():
    M = 5
    e = Ens(M, ONE_TILE)
    # (lr = 6: searches that bracket and zoom, so that the members need different numbers of evaluations for their six
    # iterations; max_eval out of the way, so that it is max_iter that stops them)
    kw = dict(max_iter=6, max_eval=100, lr=6.0, history_size=3)
    opt = e.device(**kw)
    stop_slot, frozen = {}, {}
    slot = 0
    while not opt.done:
        slot += 1
        assert slot <= 200
        tr = opt.run(1)[0]
        for j, c in enumerate(opt.ctrls()):
            if j in stop_slot:      # from its stop on: zero trace rows, the row of params and the control block as they were
                assert bool((tr[j] == 0).all()), (slot, j)
                assert torch.equal(opt.params[j], frozen[j][0]), (slot, j)
                assert ctrl_fields(c, skip=("action",)) == frozen[j][1], (slot, j)
                assert c.action == LBFGS_ACT_INERT
            elif c.done:
                stop_slot[j] = slot
                frozen[j] = (opt.params[j].clone(), ctrl_fields(c, skip=("action",)))
    print(f"max_iter = 6: members stopped at slots {stop_slot}, reasons {opt.stop_reason}")
    assert len(set(stop_slot.values())) >= 2, "every member stopped at the same slot: pick another seed"
    for j in range(M):
        one = e.single(j, **kw).step()
        assert stop_slot[j] == int((one.trace[:, 2] != LBFGS_ACT_INERT).sum())
        assert_member_is_single(opt, j, one, "stops:", slots=stop_slot[j])
        # (n_slots counts inert slots too; the single run stopped enqueuing earlier)
    assert all(r == "max_iter" for r in opt.stop_reason)


# ---- 4. members do not touch each other ----------------------------------------------------------------------------------------------
def test_members_do_not_touch_each_other():
    M, n = 4, 24
    e = Ens(M, ONE_TILE)
    clean = e.device(history_size=3)
    clean.run(n)
    th = e.theta0.clone()
    th[1] = float("nan")
    opt = e.device(theta=th, history_size=3)
    opt.run(n)                       # (returns: nothing hangs)
    for j in (0, 2, 3):
        assert torch.equal(opt.trace[:, j, :], clean.trace[:, j, :]) and torch.equal(opt.params[j], clean.params[j]), j
        assert ctrl_fields(opt.ctrls()[j]) == ctrl_fields(clean.ctrls()[j]), j
    one = e.single(1, theta=th[1], history_size=3)
    one.run(n)
    assert torch.allclose(opt.trace[:, 1, :], one.trace, rtol=0, atol=0, equal_nan=True)
    assert torch.allclose(opt.params[1], one.params, rtol=0, atol=0, equal_nan=True)
    assert ctrl_fields(opt.ctrls()[1]) == ctrl_fields(one.ctrl())
    print(f"NaN member: {opt.func_evals[1]} evaluations, done {opt.ctrls()[1].done}, reason '{opt.stop_reason[1]}'; the others "
          f"{[opt.func_evals[j] for j in (0, 2, 3)]} evaluations, bits of the clean run")
    assert bool(torch.isfinite(opt.params[[0, 2, 3]]).all())


# ---- 5. resumption ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_of_n_slots_are_one_call_of_2n():
    e = Ens(3, ONE_TILE)
    a, b = e.device(history_size=3), e.device(history_size=3)
    a.run(12); a.run(12)
    b.run(24)
    same_state = torch.equal(a.state, b.state)
    print(f"2 x 12 vs 1 x 24 slots: evaluations {a.func_evals}; params equal {torch.equal(a.params, b.params)}, trace equal "
          f"{torch.equal(a.trace, b.trace)}, state equal {same_state}")
    assert torch.equal(a.params, b.params) and torch.equal(a.trace, b.trace) and same_state
    assert not torch.equal(a.params, e.theta0)


# ---- 6. own point sets -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own_x,own_t", [(True, True), (True, False), (False, True)], ids=["own X, T", "own X", "own T"])
def test_own_point_sets(own_x, own_t):
    e = Ens(3, ONE_TILE, own_x=own_x, own_t=own_t)
    assert e.X.dim() == (3 if own_x else 2) and e.T.dim() == (3 if own_t else 2)
    if own_x:
        assert not torch.equal(e.X[0], e.X[1])
    if own_t:
        assert not torch.equal(e.T[0], e.T[1])
    opt = e.device(history_size=3)
    opt.run(20)
    for j in range(3):
        one = e.single(j, history_size=3)
        one.run(20)
        assert_member_is_single(opt, j, one, f"own_x {own_x}, own_t {own_t}:")
    assert not torch.equal(opt.params, e.theta0)


# ---- 7. buffer contract ----------------------------------------------------------------------------------------------------------------
def test_buffer_contract():
    """Guard bands around params, state and trace, a workspace full of 1e30, a second stream: the bits of the plain call,
    nothing written outside the stated extents, read-only arguments untouched."""
    M, n, hist = 3, 20, 3
    e = Ens(M, ONE_TILE)
    p0 = e.pbs[0]
    ref = e.device(max_iter=6, history_size=hist)
    ref.run(n)
    P = e.theta0.shape[1]
    ws_bytes, st_bytes = e.eng.ensemble_lbfgs_loop_query(M, e.N, hist)
    assert st_bytes == _lib.ensemble_lbfgs_state_bytes(M, P, hist)
    state, g_state = guarded(st_bytes, torch.uint8, DEV, name="state")
    trace, g_trace = guarded((n, M, LBFGS_TRACE_COLS), torch.float64, DEV, name="trace")
    params, g_params = guarded((M, P), torch.float32, DEV, name="params")
    ws, g_ws = guarded(ws_bytes, torch.uint8, DEV, name="workspace")
    poison_workspace(ws)
    params.copy_(e.theta0)
    ro = dict(X=e.X, T=e.T, res_scale=p0.res_scale, fid_scale=p0.fid_scale, loss_rows=p0.loss_rows)
    snaps = {k: snapshot(v) for k, v in ro.items()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        e.eng.ensemble_lbfgs_loop_init(state, M, 1.0, 6, 7, hist, 0.0, 0.0)
        for k in (8, 12):      # two calls: the state carries over; the workspace is poisoned again in between
            e.eng.ensemble_lbfgs_loop(e.spec, p0.res_scale, params, e.X, p0.n_res, p0.loss_rows, 2, hist, state, k,
                                      trace[:8] if k == 8 else trace[8:], T=e.T, out_col=p0.fid_cols, col_scale=p0.fid_scale, ws=ws)
            poison_workspace(ws)
    side.synchronize()
    for g in (g_state, g_trace, g_params, g_ws):
        g.assert_bands_intact()
    for k, v in ro.items():
        assert_unchanged(v, snaps[k], k)
    print(f"contract: {int((trace[:, :, 2] != 0).sum())} evaluations on a side stream, params equal {torch.equal(params, ref.params)}, "
          f"trace equal {torch.equal(trace.cpu(), ref.trace)}")
    assert torch.equal(params, ref.params) and torch.equal(trace.cpu(), ref.trace)
    assert bool(torch.isfinite(trace).all())


# ---- 8. refusals launch nothing --------------------------------------------------------------------------------------------------------
def _raw_call(eng, spec, M, th, X, T, n_res, nc, state, ws, hist=3, n_slots=2, n_loss_rows=3, total_row=2, null=(), M_arg=None,
              state_bytes=None, ws_bytes=None):
    """pinn_ensemble_lbfgs_loop itself (no Python-side checks in between): (rc, message)."""
    N, nt = X.shape[0], spec.n_terms
    a = dict(term_scale=torch.ones(nt, device=DEV), col_scale=torch.ones(nc, device=DEV), params=th, X=X, T=T,
             loss_rows=torch.ones(max(n_loss_rows, 1), nc + nt, device=DEV), state=state, ws=ws)
    p = {k: (None if k in null or v is None else _ptr(v)) for k, v in a.items()}
    with eng._guard():
        rc = eng.lib.pinn_ensemble_lbfgs_loop(
            C.byref(eng._d()), C.byref(spec.c_struct()), M if M_arg is None else M_arg, p["term_scale"], p["T"], nc,
            _out_cols(range(nc)), p["col_scale"], p["params"], p["X"], N, int(n_res), 0, n_loss_rows, p["loss_rows"], total_row,
            hist, p["state"], state.numel() if state_bytes is None else state_bytes, n_slots, None, p["ws"],
            ws.numel() if ws_bytes is None else ws_bytes, eng._stream())
    return rc, eng.last_error()


def _refusal_setup(desc, M=3, N=255, nc=2):
    g = torch.Generator().manual_seed(3)
    th = torch.randn(M, desc.n_params, generator=g).mul_(0.1).to(DEV)
    X = (torch.rand(N, desc.d_in, generator=g) * 2 - 1).to(DEV)
    state = torch.full((1 << 16,), 7, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    return th, X, state, ws


@pytest.mark.parametrize("name,kw,res,n_res,what", REFUSED, ids=[r[0] for r in REFUSED])
def test_what_the_ensemble_pass_refuses_is_refused_in_its_words(name, kw, res, n_res, what):
    desc = NetDesc(**kw)
    if res.startswith("physics_equation"):
        spec = ResidualSpec.from_names("physics_equation", ("x", "y"), desc.grad_cols, ROLES, corrected=res.endswith("corrected"))
    else:
        spec = ResidualSpec.from_names(res, ("t", "x", "y"), desc.grad_cols, ("h", "z", "u", "v"))
    eng = Engine(desc, DEV)
    M, N, nc = 3, 255, 2
    th, X, state, ws = _refusal_setup(desc)
    T = torch.rand(N - n_res if n_res < N else 1, nc).to(DEV)
    before = th.clone(), state.clone()
    rc, msg = _raw_call(eng, spec, M, th, X, T if n_res < N else None, n_res, nc, state, ws)
    theirs = eng.ensemble_refusal(spec, M, N, n_res, nc)
    print(f"{name}: rc {rc}: {msg}")
    assert rc == _lib.ERR_UNSUPPORTED and what in msg
    assert msg.replace("pinn_ensemble_lbfgs_loop", "WHO") == theirs.replace("pinn_ensemble_loss_grad", "WHO").replace("pinn_ensemble_plan", "WHO")
    if name not in ("corrected", "split_w64"):      # the descriptor's refusals: the query gives them too
        with pytest.raises(PinnError, match=what):
            eng.ensemble_lbfgs_loop_query(M, N, 3)
    torch.cuda.synchronize()
    assert torch.equal(th, before[0]) and torch.equal(state, before[1])


def test_bad_arguments_are_refused_before_any_device_work():
    desc = NetDesc(**PE)
    spec = ResidualSpec.from_names("physics_equation", ("x", "y"), desc.grad_cols, ROLES)
    eng = Engine(desc, DEV)
    M, N, nc, n_res = 3, 255, 2, 243
    th, X, _, _ = _refusal_setup(desc)
    T = torch.rand(N - n_res, nc).to(DEV)
    ws_bytes, st_bytes = eng.ensemble_lbfgs_loop_query(M, N, 3)
    state = torch.full((st_bytes,), 7, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(max(ws_bytes, 256), dtype=torch.uint8, device=DEV)
    before = th.clone(), state.clone()
    INV, WSP, UNS = _lib.ERR_INVALID, _lib.ERR_WORKSPACE, _lib.ERR_UNSUPPORTED
    cases = [
        ("M = 0", dict(M_arg=0), INV, "M = 0 outside 1..65535"),
        ("M = 65536", dict(M_arg=65536), INV, "M = 65536 outside 1..65535"),
        ("history 0", dict(hist=0), INV, "history_size = 0 outside 1..256"),
        ("history 257", dict(hist=257), INV, "history_size = 257 outside 1..256"),
        ("n_slots < 0", dict(n_slots=-1), INV, "n_slots = -1"),
        ("n_loss_rows 0", dict(n_loss_rows=0), INV, "n_loss_rows = 0 outside 1..8"),
        ("n_loss_rows 9", dict(n_loss_rows=9), INV, "n_loss_rows = 9 outside 1..8"),
        ("total_row", dict(total_row=3), INV, "total_row = 3 outside it"),
        ("params NULL", dict(null=("params",)), INV, "NULL pointer"),
        ("X NULL", dict(null=("X",)), INV, "NULL pointer"),
        ("term_scale NULL", dict(null=("term_scale",)), INV, "NULL pointer"),
        ("loss_rows NULL", dict(null=("loss_rows",)), INV, "NULL pointer"),
        ("state NULL", dict(null=("state",)), INV, "NULL pointer"),
        ("T NULL", dict(null=("T",)), INV, "NULL pointer"),
        ("col_scale NULL", dict(null=("col_scale",)), INV, "NULL pointer"),
        ("state too small", dict(state_bytes=st_bytes - 1), WSP, "state too small"),
        ("workspace too small", dict(ws_bytes=ws_bytes - 1), WSP, "workspace"),
        ("workspace NULL", dict(null=("ws",)), WSP, "workspace"),
    ]
    for label, kw, want, what in cases:
        rc, msg = _raw_call(eng, spec, M, th, X, T, n_res, nc, state, ws, **kw)
        print(f"{label}: rc {rc}: {msg}")
        assert rc == want and what in msg, (label, rc, msg)
        assert msg.startswith("pinn_ensemble_lbfgs_loop") or "workspace too small" in msg, (label, msg)
    for gc in ((), (0,)):            # k other than 2 or 3
        e1 = Engine(NetDesc(**dict(PE, grad_cols=gc)), DEV)
        with pytest.raises(PinnError, match="k must be 2 or 3"):
            e1.ensemble_lbfgs_loop_query(M, N, 3)
    # the init's own: M, history, options, a state smaller than the query's answer
    o = _lib.PinnLbfgsOpts(1.0, 0.0, 0.0, 6, 7, 3)
    for label, args, want, what in (("M", (st_bytes, 0, desc.n_params, o), INV, "M = 0"),
                                    ("history", (st_bytes, M, desc.n_params, _lib.PinnLbfgsOpts(1.0, 0.0, 0.0, 6, 7, 300)), INV, "history_size = 300"),
                                    ("lr", (st_bytes, M, desc.n_params, _lib.PinnLbfgsOpts(0.0, 0.0, 0.0, 6, 7, 3)), INV, "lr = 0"),
                                    ("state", (st_bytes - 1, M, desc.n_params, o), WSP, "state too small")):
        with eng._guard():
            rc = eng.lib.pinn_ensemble_lbfgs_loop_init(_ptr(state), args[0], args[1], args[2], C.byref(args[3]), eng._stream())
        print(f"init, {label}: rc {rc}: {eng.last_error()}")
        assert rc == want and what in eng.last_error()
    torch.cuda.synchronize()
    assert torch.equal(th, before[0]) and torch.equal(state, before[1])


# ---- 9. trainer ------------------------------------------------------------------------------------------------------------------------
def _cmb(adam_it, lbfgs_it, **lb):
    cfg = {k: dict(v) for k, v in CMB.items()}
    cfg["adam_optimizer"] = dict(cfg["adam_optimizer"], max_it=adam_it, learning_rate=1e-3, scheduler_step_size=3)
    cfg["lbfgs_optimizer"] = dict(cfg["lbfgs_optimizer"], max_it=lbfgs_it, tolerance_grad=0.0, tolerance_change=0.0, **lb)
    return cfg


def _condition(dnn):
    """tests/test_ensemble_gpu.py's conditioning of physics_equation's outputs, written through the module."""
    last = [mod for mod in dnn.modules() if isinstance(mod, torch.nn.Linear)][-1]
    with torch.no_grad():
        last.weight.mul_(0.25)
        for name, val in (("h", 2.0), ("eta_mean", 0.2), ("Hrms", 0.5), ("k", 1.0)):
            last.bias[ROLES.index(name)] = val


def test_trainer_lbfgs_stage():
    rs = np.random.RandomState(5)
    Xr = rs.rand(243, 2).astype(np.float32) * 2 - 1
    Xf = rs.rand(12, 2).astype(np.float32) * 2 - 1
    Tf = rs.rand(12, 6).astype(np.float32)
    Tf[:, 0] += 1.0
    cfg, M, seeds = _cmb(5, 6), 3, (11, 12, 13)
    assert cfg["lbfgs_optimizer"]["line_search_fn"] == "strong_wolfe"
    layers = [2] + [10] * 10 + [6]
    ens = EnsemblePINN(Xf, Tf, Xr, cfg, M, seeds=seeds, device=DEV, lbfgs_stage=True)
    for i in range(M):
        _condition(ens.member(i))
    theta0 = ens.theta.clone()
    # with the default, train() is the Adam stage alone
    plain = EnsemblePINN(Xf, Tf, Xr, cfg, M, seeds=seeds, device=DEV)
    plain.theta.copy_(theta0)
    plain.train()
    assert plain.iter == 5 and plain.device_lbfgs is None and plain.lbfgs_history[0].shape == (0, 3)
    ens.train()
    opt = ens.device_lbfgs
    assert opt is not None and opt.done and ens.iter == 5 + max(opt.func_evals)
    hist = ens.lbfgs_history
    for i in range(M):
        runs = {}
        for impl in ("device", "flat"):
            dnn = DNN(layers, 0.0, "xavier").to(DEV)
            dnn.flat_params().copy_(theta0[i])
            tr = PINN(Xf, Tf, Xr, cfg, dnn=dnn, device=DEV, log_every=1, checkpoint_every=0, lbfgs_impl=impl)
            seq = []
            if impl == "flat":
                lb, inner = tr.optimizer_LBFGS, tr.closure

                def closure(seq=seq, lb=lb, inner=inner, tr=tr):
                    seq.append(lb.state[tr.theta_param].get("n_iter", 0))
                    return inner()

                tr.closure = closure
            tr.train()
            its = seq if impl == "flat" else eval_iterations(tr.device_lbfgs.trace)
            runs[impl] = (tr, its, float(tr.history[-1][3]))
        (tr_d, it_d, l_d), (tr_f, it_f, l_f) = runs["device"], runs["flat"]
        assert it_d == it_f, f"member {i}: flat and device disagree on this input, pick other seeds: {it_f} vs {it_d}"
        floor = abs(l_d - l_f) / abs(l_f)
        it_e = eval_iterations(opt.trace[:, i, :])
        l_e = float(hist[i][-1, 2])
        d = abs(l_e - l_d) / abs(l_d)
        print(f"member {i}: {len(it_e)} evaluations, {opt.n_iter[i]} iterations, stop '{opt.stop_reason[i]}'; final total loss ensemble "
              f"{l_e!r}, single device {l_d!r}, flat {l_f!r}; floor {floor:.2e}, ensemble vs device {d:.2e}, bar {max(4 * floor, 1e-6):.2e}")
        assert it_e == it_d, (i, it_e, it_d)
        assert d <= max(4 * floor, 1e-6), (i, d, floor)
        assert hist[i].shape == (opt.func_evals[i], 3) == (len(it_e), 3)
    # member(i) predicts with the final weights
    grid = torch.from_numpy(rs.rand(37, 2).astype(np.float32) * 2 - 1).to(DEV)
    eng = Engine(NetDesc(2, 6, 10, 10, (0, 1)), DEV)
    for i in range(M):
        assert ens.member(i).flat_params().data_ptr() == ens.theta[i].data_ptr()
        assert torch.allclose(ens.member(i)(grid).detach(), eng.forward(ens.theta[i].contiguous(), grid), rtol=1e-6, atol=1e-7)
    assert not torch.equal(ens.theta, theta0)
    # Adam after the stage: the packed copies of the Adam stage are not trusted
    fresh = EnsemblePINN(Xf, Tf, Xr, cfg, M, seeds=seeds, device=DEV)
    fresh.theta.copy_(ens.theta)
    fresh._adam_m.copy_(ens._adam_m); fresh._adam_v.copy_(ens._adam_v)
    fresh._adam_step, fresh._sched_steps = ens._adam_step, ens._sched_steps
    ens.train_adam(2)
    fresh.train_adam(2)
    for i in range(M):
        assert _same(fresh.theta[i], ens.theta[i]), (i, rel(ens.theta[i], fresh.theta[i]))
    assert not torch.equal(ens.theta, theta0)
