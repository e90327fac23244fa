"""Gradient-statistics loss balancing, everything that needs no GPU: pinn_balance_weights_host against the NumPy float64
restatement of the rule (tests/balance_util.py) bit for bit, its guards and its INVALID table; the refusal tables of
pinn_balance_update, pinn_query_adam_balanced_workspace and pinn_adam_loop_balanced (decided before any device work, so they
answer without a device; FAKE pointers, nothing dereferenced); the trainer's host logic (balance_refusal, the config keys)."""
import ctypes as C

import numpy as np
import pytest

from pinn_depthestimation_amd import NetDesc, ResidualSpec, _lib
from pinn_depthestimation_amd._lib import (ACT_LEAKY_RELU, ACT_SIN_TANH, ENGINE_AUTO, ENGINE_FUSED, ENGINE_FUSED_BATCH,
                                           ENGINE_FUSED_COOP, ENGINE_FUSED_TILE, ENGINE_GENERIC, ENGINE_WIDE, ERR_INVALID,
                                           ERR_UNSUPPORTED, ERR_WORKSPACE, PREC_BF16)
from pinn_depthestimation_amd.config import load_config
from pinn_depthestimation_amd.trainer import balance_refusal
from tests import balance_util as B

PE_OUT = ("h", "U", "V", "eta_mean", "Hrms", "k")
FAKE = 0x1000      # a non-NULL address nothing dereferences
DP, FP = C.POINTER(C.c_double), C.POINTER(C.c_float)


def host(mode, stats, lam, ref=0, alpha=0.1, P=1086, G=None):
    lib = _lib.load()
    st = np.ascontiguousarray(stats, dtype=np.float64)
    lam = np.ascontiguousarray(lam, dtype=np.float32)
    out = np.full_like(lam, -7.0)
    rc = lib.pinn_balance_weights_host(mode, lam.shape[0] if G is None else G, ref, alpha, P, st.ctypes.data_as(DP),
                                       lam.ctypes.data_as(FP), out.ctypes.data_as(FP))
    return rc, out


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def draw(rng, G):
    """Statistics of gradients whose groups differ by up to 1e+-4 in scale, and weights of a few magnitudes."""
    s = 10.0 ** rng.uniform(-4, 4, G)
    stats = np.stack([s * rng.uniform(1, 30, G), s * rng.uniform(200, 900, G), s * s * rng.uniform(50, 5000, G)], 1)
    return stats, (10.0 ** rng.uniform(-2, 3, G)).astype(np.float32)


def test_abi_version_stays_4():
    assert _lib.load().pinn_version() == 4 == _lib.ABI_VERSION


@pytest.mark.parametrize("alpha", [1.0, 0.1, 1e-3])
@pytest.mark.parametrize("G", [1, 2, 4, 8])
@pytest.mark.parametrize("mode", [B.MAX_MEAN, B.NORM])
def test_host_rule_is_the_fp64_formula_rounded_once(mode, G, alpha):
    rng = np.random.default_rng(100 * mode + 10 * G + int(alpha * 1000) % 7)
    for ref in range(G):
        for trial in range(8):
            stats, lam = draw(rng, G)
            rc, out = host(mode, stats, lam, ref, alpha)
            want = B.weights(mode, stats, lam, ref, alpha, 1086)
            assert rc == 0 and np.array_equal(bits(out), bits(want)), (mode, G, ref, alpha, out, want)
            if mode == B.MAX_MEAN:
                assert bits(out)[ref] == bits(lam)[ref]                    # the reference group is left alone
                assert G == 1 or (np.delete(out, ref) != np.delete(lam, ref)).any()
            else:
                assert (out != lam).any()


def test_none_copies_and_in_place_is_allowed():
    stats, lam = draw(np.random.default_rng(3), 4)
    rc, out = host(B.NONE, stats, lam)
    assert rc == 0 and np.array_equal(bits(out), bits(lam))
    lib = _lib.load()
    buf = lam.copy()
    assert lib.pinn_balance_weights_host(B.NORM, 4, 0, 0.5, 10, stats.ctypes.data_as(DP), buf.ctypes.data_as(FP), buf.ctypes.data_as(FP)) == 0
    assert np.array_equal(bits(buf), bits(B.weights(B.NORM, stats, lam, 0, 0.5, 10)))


@pytest.mark.parametrize("bad", [0.0, np.nan, np.inf, -np.inf])
def test_guards_max_mean(bad):
    """A group whose own denominator S is zero, NaN or infinite keeps its weight bit for bit while the others move; a
    reference maximum that is zero, NaN or infinite moves nobody.  A (of a non-reference group) and Q are not read."""
    rng = np.random.default_rng(11)
    G, ref = 4, 1
    stats, lam = draw(rng, G)
    for j in (0, 2, 3):
        st = stats.copy(); st[j, 1] = bad
        rc, out = host(B.MAX_MEAN, st, lam, ref, 0.5)
        assert rc == 0 and np.array_equal(bits(out), bits(B.weights(B.MAX_MEAN, st, lam, ref, 0.5, 1086)))
        moved = bits(out) != bits(lam)
        assert not moved[j] and not moved[ref] and moved[[i for i in range(G) if i not in (j, ref)]].all(), (bad, j, out, lam)
    st = stats.copy(); st[ref, 0] = bad
    rc, out = host(B.MAX_MEAN, st, lam, ref, 0.5)
    assert rc == 0 and np.array_equal(bits(out), bits(lam))
    for j, col in ((0, 0), (0, 2), (ref, 1), (ref, 2)):                    # statistics the rule does not read
        st = stats.copy(); st[j, col] = bad
        rc, out = host(B.MAX_MEAN, st, lam, ref, 0.5)
        assert rc == 0 and np.array_equal(bits(out), bits(B.weights(B.MAX_MEAN, stats, lam, ref, 0.5, 1086)))


@pytest.mark.parametrize("bad", [0.0, np.nan, np.inf, -1.0])
def test_guards_norm(bad):
    """Q[j] = 0: that group's target is infinite, it keeps its weight and the others move.  A NaN, infinite or negative Q makes
    the SUM of the norms non-finite, so every target is and every group keeps its weight.  A and S are not read."""
    rng = np.random.default_rng(12)
    G = 4
    stats, lam = draw(rng, G)
    for j in range(G):
        st = stats.copy(); st[j, 2] = bad
        rc, out = host(B.NORM, st, lam, 0, 0.5)
        assert rc == 0 and np.array_equal(bits(out), bits(B.weights(B.NORM, st, lam, 0, 0.5, 1086)))
        moved = bits(out) != bits(lam)
        assert not moved[j]
        assert moved[[i for i in range(G) if i != j]].all() if bad == 0.0 else not moved.any(), (bad, j, out, lam)
        for col in (0, 1):
            st = stats.copy(); st[j, col] = bad
            rc, out = host(B.NORM, st, lam, 0, 0.5)
            assert rc == 0 and np.array_equal(bits(out), bits(B.weights(B.NORM, stats, lam, 0, 0.5, 1086)))


def test_host_invalid_table():
    stats, lam = draw(np.random.default_rng(5), 8)
    ok = dict(mode=B.NORM, stats=stats[:2], lam=lam[:2], ref=0, alpha=0.1, P=10)
    assert host(**ok)[0] == 0
    for kw, word in ((dict(alpha=0.0), "alpha"), (dict(alpha=-0.1), "alpha"), (dict(alpha=1.0000001), "alpha"), (dict(alpha=np.nan), "alpha"),
                     (dict(G=0), "G"), (dict(G=9), "G"), (dict(ref=-1), "ref"), (dict(ref=2), "ref"), (dict(P=0), "P"),
                     (dict(mode=3), "mode"), (dict(mode=-1), "mode")):
        rc, out = host(**{**ok, **kw})
        assert rc == ERR_INVALID and word in _lib.load().pinn_last_error().decode(), kw
        assert (out == -7.0).all()
    assert host(B.NORM, stats, lam, ref=7, alpha=1.0, P=1)[0] == 0
    lib = _lib.load()
    assert lib.pinn_balance_weights_host(B.NORM, 2, 0, 0.1, 10, None, lam.ctypes.data_as(FP), lam.ctypes.data_as(FP)) == ERR_INVALID
    assert lib.pinn_balance_weights_host(B.NORM, 2, 0, 0.1, 10, stats.ctypes.data_as(DP), None, lam.ctypes.data_as(FP)) == ERR_INVALID


def test_balance_update_refusals_and_query():
    lib, b = _lib.load(), C.c_int64(-1)
    prev = 0
    for P in (1, 63, 1086, 29636, 1 << 22):
        for G in (1, 8):
            assert lib.pinn_query_balance_workspace(P, G, C.byref(b)) == 0 and b.value > 0 and b.value % 256 == 0
        assert b.value >= prev
        prev = b.value
    assert lib.pinn_query_balance_workspace(0, 2, C.byref(b)) == ERR_INVALID
    assert lib.pinn_query_balance_workspace(10, 9, C.byref(b)) == ERR_INVALID and lib.pinn_query_balance_workspace(10, 0, C.byref(b)) == ERR_INVALID
    assert lib.pinn_query_balance_workspace(10, 2, None) == ERR_INVALID

    def upd(mode=B.NORM, G=2, ref=0, alpha=0.1, grads=FAKE, P=100, ld=100, lam=FAKE, ws=FAKE, ws_bytes=1 << 20):
        return lib.pinn_balance_update(mode, G, ref, alpha, grads, P, ld, lam, None, FAKE, ws, ws_bytes, None)
    assert upd(ld=99) == ERR_INVALID and "ld" in lib.pinn_last_error().decode()
    assert upd(grads=None) == ERR_INVALID and upd(lam=None) == ERR_INVALID
    assert upd(mode=5) == ERR_INVALID and upd(G=9) == ERR_INVALID and upd(ref=2) == ERR_INVALID and upd(alpha=0.0) == ERR_INVALID
    assert upd(P=0, ld=0) == ERR_INVALID
    assert upd(ws_bytes=8) == ERR_WORKSPACE and upd(ws=None) == ERR_WORKSPACE
    assert upd(mode=B.NONE, grads=None) == ERR_INVALID


# ---- pinn_adam_loop_balanced: the refusal table ------------------------------------------------------------------------
def _pe(**kw):
    d = NetDesc(2, 6, 10, 10, (0, 1), **kw)
    return d, ResidualSpec.from_names("physics_equation", ("x", "y"), d.grad_cols, PE_OUT)


def _ns(**kw):
    d = NetDesc(3, 4, 8, 64, (0, 1, 2), **kw)
    return d, ResidualSpec.from_names("Navier_Stokes", ("t", "x", "y"), d.grad_cols, ("h", "z", "u", "v"))


def _bal(mode=B.NORM, every=3, ref=0, alpha=0.5, lam=FAKE):
    return _lib.PinnBalance(mode, every, ref, alpha, lam, None, None, None)


def _query(desc, spec, n_res=243, n_fid=12):
    lib, b = _lib.load(), C.c_int64(-1)
    rc = lib.pinn_query_adam_balanced_workspace(C.byref(desc.c_struct()), C.byref(spec.c_struct()), n_res, n_fid, C.byref(b))
    return rc, b.value, lib.pinn_last_error().decode()


def _loop(desc, spec, bal, n_iters=3, n_res=243, n_fid=12):
    """The call itself WITHOUT arrays: a refusal comes back with its code; a served request stops at the NULL arguments."""
    lib = _lib.load()
    st = _lib.PinnAdamState(None, None, 1, 0.0, 0.9, 0.999, 1e-8, 0, 0, None, None)
    rc = lib.pinn_adam_loop_balanced(C.byref(desc.c_struct()), C.byref(spec.c_struct()), None, None, None, n_fid, 0, None, None,
                                     None, None, n_res, None, None, None, C.byref(st), None if bal is None else C.byref(bal),
                                     n_iters, None, None, 0, None)
    return rc, lib.pinn_last_error().decode()


@pytest.mark.parametrize("engine,served", [(ENGINE_AUTO, True), (ENGINE_FUSED, True), (ENGINE_FUSED_TILE, True), (ENGINE_FUSED_COOP, True),
                                           (ENGINE_GENERIC, False), (ENGINE_WIDE, False), (ENGINE_FUSED_BATCH, False)])
def test_every_engine_value(engine, served):
    for mk in (_pe, _ns):
        desc, spec = mk(engine=engine)
        if engine == ENGINE_FUSED_COOP and mk is _pe:
            served_here = False          # the cooperative kernel exists at padded width 64 only, as in the single entries
        else:
            served_here = served
        rc, b, msg = _query(desc, spec)
        rcl, msgl = _loop(desc, spec, _bal())
        if served_here:
            assert rc == 0 and b > 0, msg
            assert rcl == ERR_INVALID and "bad arguments" in msgl          # past every refusal, stopped at the NULL arrays
        else:
            assert rc == ERR_UNSUPPORTED and rcl == ERR_UNSUPPORTED, (rc, rcl, msg)


def test_descriptor_refusals():
    for what, kw, word in (("bf16", dict(precision=PREC_BF16), "bf16"), ("dropout", dict(dropout_p=0.1), "dropout"),
                           ("leaky", dict(activation=ACT_LEAKY_RELU), "LeakyReLU"), ("sine", dict(activation=ACT_SIN_TANH), "sine")):
        for mk in (_pe, _ns):
            desc, spec = mk(**kw)
            rc, _, msg = _query(desc, spec)
            assert rc == ERR_UNSUPPORTED and word in msg, (what, rc, msg)
            rcl, msg = _loop(desc, spec, _bal())
            assert rcl == ERR_UNSUPPORTED and word in msg, (what, msg)
    d65 = NetDesc(2, 6, 3, 65, (0, 1))
    s65 = ResidualSpec.from_names("physics_equation", ("x", "y"), d65.grad_cols, PE_OUT)
    rc, _, msg = _query(d65, s65)
    assert rc == ERR_UNSUPPORTED and "width" in msg
    assert _loop(d65, s65, _bal())[0] == ERR_UNSUPPORTED
    desc, _ = _pe()
    pec = ResidualSpec.from_names("physics_equation", ("x", "y"), desc.grad_cols, PE_OUT, corrected=True)
    rc, _, msg = _query(desc, pec)
    assert rc == ERR_UNSUPPORTED and "corrected" in msg
    rcl, msg = _loop(desc, pec, _bal())
    assert rcl == ERR_UNSUPPORTED and "corrected" in msg
    d3 = NetDesc(3, 6, 2, 10, (0, 1, 2))          # k must be the residual's directions
    s3 = ResidualSpec.from_names("physics_equation", ("t", "x", "y"), d3.grad_cols, PE_OUT)
    assert _query(d3, s3)[0] == ERR_UNSUPPORTED and _loop(d3, s3, _bal())[0] == ERR_UNSUPPORTED


def test_invalid_arguments_and_zero_iterations():
    desc, spec = _pe()
    assert _query(desc, spec, n_fid=0)[0] == ERR_INVALID and _query(desc, spec, n_res=0)[0] == ERR_INVALID
    assert _loop(desc, spec, _bal(), n_fid=0)[0] == ERR_INVALID and _loop(desc, spec, _bal(), n_res=0)[0] == ERR_INVALID
    for bal, word in ((_bal(every=0), "every"), (_bal(alpha=0.0), "alpha"), (_bal(alpha=1.5), "alpha"), (_bal(mode=B.NONE), "mode"),
                      (_bal(mode=3), "mode"), (_bal(ref=2), "ref"), (_bal(ref=-1), "ref"), (_bal(lam=None), "lam"), (None, "balance")):
        rc, msg = _loop(desc, spec, bal)
        assert rc == ERR_INVALID and word in msg, (word, rc, msg)
        assert _loop(desc, spec, bal, n_iters=0)[0] == ERR_INVALID
    assert _loop(desc, spec, _bal(), n_iters=0)[0] == 0
    assert _loop(desc, spec, _bal(), n_iters=-1)[0] == ERR_INVALID
    dg, sg = _pe(engine=ENGINE_GENERIC)          # ... but a refusal is a refusal whatever n_iters
    assert _loop(dg, sg, _bal(), n_iters=0)[0] == ERR_UNSUPPORTED


@pytest.mark.parametrize("mk", [_pe, _ns])
def test_query_covers_the_extended_loop_and_the_single_entries(mk):
    lib = _lib.load()
    desc, spec = mk()
    ex = _lib.PinnAdamExtras()
    ex.point_w, ex.w_rows = FAKE, 1
    prev = 0
    for n_res, n_fid in ((1, 1), (243, 12), (4099, 12), (243, 1 << 16), (1 << 20, 12)):
        rc, b, msg = _query(desc, spec, n_res, n_fid)
        e, s = C.c_int64(), C.c_int64()
        assert rc == 0, msg
        assert lib.pinn_query_adam_ext_workspace(C.byref(desc.c_struct()), C.byref(spec.c_struct()), C.byref(ex), n_res, n_fid, C.byref(e)) == 0
        assert lib.pinn_query_workspace(C.byref(desc.c_struct()), max(n_res, n_fid), C.byref(s)) == 0
        assert b >= e.value >= s.value and b >= prev, (n_res, n_fid, b, e.value, s.value)
        prev = max(prev, b) if n_fid == 12 else prev


# ---- the trainer's host logic --------------------------------------------------------------------------------------------
def test_balance_refusal():
    assert balance_refusal(None) is None                                         # the option is off: nothing to decide
    assert balance_refusal("max_mean") is None and balance_refusal("norm") is None
    assert balance_refusal("norm", groups="terms") is None
    assert balance_refusal("norm", fold_extras=True) is None
    for kw, word in ((dict(coefficients=True), "coefficient"), (dict(weighted=True), "weight"), (dict(rad_importance=True), "rad"),
                     (dict(eddy_viscosity=0.1), "eddy_viscosity"), (dict(reducer_active=True), "parallel"),
                     (dict(custom_evaluator=True), "custom"), (dict(groups="terms", fold_extras=True), "terms"),
                     (dict(groups="columns"), "balance_groups"), (dict(every=0), "balance_every"), (dict(alpha=0.0), "balance_alpha"),
                     (dict(alpha=1.5), "balance_alpha"), (dict(ref="gauges"), "balance_ref")):
        for mode in ("max_mean", "norm"):
            why = balance_refusal(mode, **kw)
            assert why and word in why, (kw, why)
    assert "loss_balancing" in balance_refusal("softadapt")


def test_config_keys():
    cfg = {
        "layers": {"input_features": 2, "hidden_layers": 2, "hidden_width": 10, "output_features": 6, "dropout_rate": 0.0, "init_type": "xavier"},
        "adam_optimizer": {"max_it": 20, "learning_rate": 1e-3, "scheduler_step_size": 7, "scheduler_gamma": 0.8},
        "lbfgs_optimizer": {"max_it": 0, "learning_rate": 1, "max_evaluation": 12, "history_size": 10,
                            "tolerance_grad": 1e-9, "tolerance_change": 1e-12, "line_search_fn": "strong_wolfe"},
        "loss": {"weight_fid_loss": 1, "weight_res_loss": 1},
        "data_fidelity": {"inputs": ["x", "y"], "outputs": list(PE_OUT), "training_points": 12},
        "data_residual": {"inputs": {"x": {"requires_grad": ["true"]}, "y": {"requires_grad": ["true"]}}, "outputs": list(PE_OUT)},
    }
    c = load_config(cfg)
    assert c.loss_balancing is None and c.balance_every == 10 and c.balance_alpha == 0.1
    assert c.balance_ref == "residual" and c.balance_groups == "sets"
    cfg["loss"].update(balancing="norm", balance_every=3, balance_alpha=0.5, balance_ref="fidelity", balance_groups="terms")
    c = load_config(cfg)
    assert (c.loss_balancing, c.balance_every, c.balance_alpha, c.balance_ref, c.balance_groups) == ("norm", 3, 0.5, "fidelity", "terms")
