"""The ensemble's device-resident L-BFGS loop (pinn_ensemble_lbfgs_loop, lbfgs.EnsembleDeviceLBFGS, EnsemblePINN(lbfgs_stage=
True)) without a device: the query and its refusals, the state-size formula of include/pinn_hip.h, the ctypes mirrors, and
the option refusals of the trainer, which must be raised before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pinn_depthestimation_amd import _lib
from pinn_depthestimation_amd._lib import ERR_INVALID, ERR_UNSUPPORTED, PinnLbfgsCtrl, PinnLbfgsOpts
from pinn_depthestimation_amd.engine import NetDesc

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "pinn_hip.h")
NEW = ("pinn_ensemble_query_lbfgs_loop", "pinn_ensemble_lbfgs_loop_init", "pinn_ensemble_lbfgs_loop")


def _desc(width=10, hidden=10, **kw):
    return NetDesc(2, 6, hidden, width, kw.pop("grad_cols", (0, 1)), **kw)


def _query(desc, M=3, N=255, m=100, ws=True, st=True):
    lib = _lib.load()
    w, s = C.c_int64(-1), C.c_int64(-1)
    rc = lib.pinn_ensemble_query_lbfgs_loop(C.byref(desc.c_struct()), M, N, m, C.byref(w) if ws else None, C.byref(s) if st else None)
    return rc, w.value, s.value, lib.pinn_last_error().decode()


def _a256(v):
    return (v + 255) // 256 * 256


def _formula(M, P, m):
    """include/pinn_hip.h, "the device-resident L-BFGS loop of an ensemble", written out once more."""
    member = _a256(4 * 4 * P) + 4 * _a256(4 * P) + _a256(8 * 256 * 8) + _a256(32) + _a256(8 * 4 * 256) + _a256(4 * 2 * 256) \
        + 2 * _a256(4 * m * P) + _a256(8 * m * m)
    return M * _a256(C.sizeof(PinnLbfgsCtrl)) + 3 * _a256(4 * M * P) + 2 * _a256(4 * M * 8) + M * member


def test_state_bytes_follow_the_documented_formula():
    lib = _lib.load()
    for width, hidden in ((10, 10), (64, 8)):
        desc = _desc(width, hidden)
        P = desc.n_params
        for M in (1, 3, 256):
            for m in (1, 100, 256):
                rc, ws, st, msg = _query(desc, M, 255, m)
                assert rc == 0, msg
                ws0 = C.c_int64()
                _lib.check(lib.pinn_ensemble_query_workspace(C.byref(desc.c_struct()), M, 255, C.byref(ws0)), "query ws")
                assert ws == ws0.value                         # the ensemble pass's own workspace, nothing else
                assert st == _formula(M, P, m) == _lib.ensemble_lbfgs_state_bytes(M, P, m), (M, P, m, st)
                assert st % 256 == 0
    # what the header's text says the formula is made of
    text = open(HEADER).read()
    assert "state_bytes = M a(sizeof(pinn_lbfgs_ctrl)) + 3 a(4 M P) + 2 a(4 M PINN_MAX_ROLES) + M member_bytes" in text
    assert _lib.PINN_MAX_ROLES == 8 and _lib.LS_POOL_ROWS == 4


def test_query_refusals():
    d = _desc()
    for kw, code, word in ((dict(M=0), ERR_INVALID, "M = 0 outside 1..65535"), (dict(M=65536), ERR_INVALID, "M = 65536"),
                           (dict(m=0), ERR_INVALID, "history_size = 0 outside 1..256"), (dict(m=257), ERR_INVALID, "history_size = 257"),
                           (dict(N=0), ERR_INVALID, "bad arguments"), (dict(ws=False), ERR_INVALID, "bad arguments"),
                           (dict(st=False), ERR_INVALID, "bad arguments")):
        rc, _, _, msg = _query(d, **kw)
        print(kw, rc, msg)
        assert rc == code and word in msg and msg.startswith("pinn_ensemble_query_lbfgs_loop"), (kw, rc, msg)
    assert _query(d, M=1, m=1)[0] == 0 and _query(d, M=65535, m=256)[0] == 0
    # the descriptor's refusals, in the ensemble pass's words: the message is pinn_ensemble_query_workspace's but for the name
    lib = _lib.load()
    ns = dict(grad_cols=(0, 1, 2))
    for label, desc, word in (("generic", _desc(engine=_lib.ENGINE_GENERIC), "GENERIC"),
                              ("wide", NetDesc(3, 4, 8, 128, (0, 1, 2), engine=_lib.ENGINE_WIDE), "WIDE"),
                              ("coop", NetDesc(3, 4, 8, 64, (0, 1, 2), engine=_lib.ENGINE_FUSED_COOP), "FUSED_COOP"),
                              ("batch", _desc(engine=_lib.ENGINE_FUSED_BATCH), "FUSED_BATCH"),
                              ("bf16", NetDesc(3, 4, 8, 128, (0, 1, 2), precision=_lib.PREC_BF16), "bf16"),
                              ("width", NetDesc(3, 4, 8, 65, (0, 1, 2)), "width above 64"),
                              ("leaky", _desc(activation=_lib.ACT_LEAKY_RELU), "LeakyReLU"),
                              ("sine", _desc(activation=_lib.ACT_SIN_TANH), "sine"),
                              ("dropout", _desc(dropout_p=0.1), "dropout"),
                              ("k = 0", _desc(grad_cols=()), "k must be 2 or 3"),
                              ("k = 1", _desc(grad_cols=(0,)), "k must be 2 or 3")):
        rc, _, _, msg = _query(desc)
        b = C.c_int64()
        rc0 = lib.pinn_ensemble_query_workspace(C.byref(desc.c_struct()), 3, 255, C.byref(b))
        theirs = lib.pinn_last_error().decode()
        print(label, rc, msg)
        assert rc == rc0 == ERR_UNSUPPORTED and word in msg, (label, rc, rc0, msg)
        assert msg == theirs.replace("pinn_ensemble_query_workspace", "pinn_ensemble_query_lbfgs_loop"), (msg, theirs)


def test_lib_mirrors():
    lib = _lib.load()
    text = open(HEADER).read()
    for name in NEW:
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        proto = re.search(r"int32_t %s\((.*?)\);" % name, text, re.S)
        assert proto, f"{name} is not declared in pinn_hip.h"
        args = [a.strip() for a in proto.group(1).split(",")]
        res, argtypes = _lib._SIGNATURES[name]
        assert res is C.c_int32 and len(argtypes) == len(args), (name, len(argtypes), len(args))
        for a, t in zip(args, argtypes):      # the scalar types, one by one; every pointer is a pointer
            if "*" in a:
                assert t is C.c_void_p or hasattr(t, "contents") or issubclass(t, C._Pointer), (name, a, t)
            else:
                assert t is {"int32_t": C.c_int32, "int64_t": C.c_int64}[a.split()[0]], (name, a, t)
    # the new entries come after the single loop's, under the ABI version that loop has
    assert text.index("int32_t pinn_lbfgs_loop(") < text.index("int32_t pinn_ensemble_query_lbfgs_loop(")
    assert lib.pinn_version() == _lib.ABI_VERSION == 4 and "#define PINN_ABI_VERSION 4" in text
    # the control blocks' stride and where Python finds x_trial
    assert _lib.ensemble_lbfgs_ctrl_stride() == _a256(C.sizeof(PinnLbfgsCtrl)) and C.sizeof(PinnLbfgsCtrl) % 8 == 0
    assert [f[0] for f in PinnLbfgsOpts._fields_] == ["lr", "tolerance_grad", "tolerance_change", "max_iter", "max_eval", "history_size"]
    assert (_lib.ENSEMBLE_OWN_X, _lib.ENSEMBLE_OWN_T, _lib.ENSEMBLE_MAX_MEMBERS) == (1, 2, 65535)


def test_init_refusals_need_no_device():
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(lr=1.0, tolerance_grad=1e-7, tolerance_change=1e-9, max_iter=10, max_eval=12, history_size=100)

    def init(state=p, state_bytes=1 << 40, M=3, P=226, opts=True, **kw):
        o = PinnLbfgsOpts(**{**ok, **kw})
        rc = lib.pinn_ensemble_lbfgs_loop_init(state, state_bytes, M, P, C.byref(o) if opts else None, None)
        return rc, lib.pinn_last_error().decode()

    for kw, code, word in ((dict(history_size=0), ERR_INVALID, "history_size"), (dict(history_size=257), ERR_INVALID, "history_size"),
                           (dict(M=0), ERR_INVALID, "M = 0"), (dict(M=65536), ERR_INVALID, "M = 65536"),
                           (dict(state=None), ERR_INVALID, "NULL"), (dict(opts=False), ERR_INVALID, "NULL"), (dict(P=0), ERR_INVALID, "P < 1"),
                           (dict(max_eval=0), ERR_INVALID, "max_eval"), (dict(max_iter=-1), ERR_INVALID, "max_iter"),
                           (dict(lr=0.0), ERR_INVALID, "lr"), (dict(state_bytes=4096), _lib.ERR_WORKSPACE, "state too small")):
        rc, msg = init(**kw)
        print(kw, rc, msg)
        assert rc == code and word in msg and msg.startswith("pinn_ensemble_lbfgs_loop_init"), (kw, rc, msg)


def _loop(desc, M=3, n_cols=2, N=255, n_res=243, flags=0, n_loss_rows=3, total_row=2, hist=100, n_slots=4, state_bytes=1 << 40,
          ws=None, ws_bytes=0, null=(), corrected=False):
    """pinn_ensemble_lbfgs_loop with host buffers standing in for device ones: every case here must be refused before any
    device work, so none of them is ever dereferenced."""
    from pinn_depthestimation_amd.engine import ResidualSpec
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    a = {k: (None if k in null else p) for k in ("term_scale", "T", "col_scale", "params", "X", "loss_rows", "state")}
    oc = None if "out_col" in null else (C.c_int32 * 8)(0, 1)
    if desc.d_in == 2:
        sp = ResidualSpec.from_names("physics_equation", ("x", "y"), desc.grad_cols, ("h", "U", "V", "eta_mean", "Hrms", "k"),
                                     corrected=corrected)
    else:
        sp = ResidualSpec.from_names("Navier_Stokes", ("t", "x", "y"), desc.grad_cols, ("h", "z", "u", "v"))
    rc = lib.pinn_ensemble_lbfgs_loop(C.byref(desc.c_struct()), None if "spec" in null else C.byref(sp.c_struct()), M,
                                      a["term_scale"], a["T"], n_cols, oc, a["col_scale"], a["params"], a["X"], N, n_res, flags,
                                      n_loss_rows, a["loss_rows"], total_row, hist, a["state"], state_bytes, n_slots, None, ws,
                                      ws_bytes, None)
    return rc, lib.pinn_last_error().decode()


def test_loop_refusals_come_before_any_device_work():
    d = _desc()
    W = _lib.ERR_WORKSPACE
    for kw, code, word in (
            (dict(M=0), ERR_INVALID, "M = 0 outside"), (dict(M=65536), ERR_INVALID, "M = 65536 outside"),
            (dict(hist=0), ERR_INVALID, "history_size = 0"), (dict(hist=257), ERR_INVALID, "history_size = 257"),
            (dict(n_slots=-1), ERR_INVALID, "n_slots = -1"),
            (dict(null=("spec",)), ERR_INVALID, "spec is NULL"),
            (dict(n_res=300), ERR_INVALID, "exceeds"), (dict(n_cols=9), ERR_INVALID, "n_cols"),
            (dict(n_cols=0), ERR_INVALID, "n_res must equal N"), (dict(N=0, n_res=0, n_cols=0), ERR_INVALID, "N = 0"),
            (dict(flags=4), ERR_INVALID, "unknown flags"),
            (dict(n_loss_rows=0), ERR_INVALID, "n_loss_rows = 0"), (dict(n_loss_rows=9), ERR_INVALID, "n_loss_rows = 9"),
            (dict(total_row=3), ERR_INVALID, "total_row = 3"), (dict(total_row=-1), ERR_INVALID, "total_row = -1"),
            (dict(null=("params",)), ERR_INVALID, "NULL"), (dict(null=("X",)), ERR_INVALID, "NULL"),
            (dict(null=("state",)), ERR_INVALID, "NULL"), (dict(null=("loss_rows",)), ERR_INVALID, "NULL"),
            (dict(null=("term_scale",)), ERR_INVALID, "NULL"), (dict(null=("out_col",)), ERR_INVALID, "NULL"),
            (dict(null=("col_scale",)), ERR_INVALID, "NULL"), (dict(null=("T",)), ERR_INVALID, "NULL"),
            (dict(state_bytes=1024), W, "state too small"),
            (dict(), W, "workspace too small"),                      # no workspace at all
    ):
        rc, msg = _loop(d, **kw)
        print(kw, rc, msg)
        assert rc == code and word in msg, (kw, rc, msg)
    # a state sized for another history is too small for this one
    st3 = _lib.ensemble_lbfgs_state_bytes(3, d.n_params, 3)
    assert _loop(d, hist=100, state_bytes=st3)[0] == W and "state too small" in _loop(d, hist=100, state_bytes=st3)[1]
    assert "workspace too small" in _loop(d, hist=3, state_bytes=st3)[1]
    # the request's own refusals, before the pointers are looked at
    rc, msg = _loop(d, corrected=True, null=("params", "X", "state"))
    assert rc == ERR_UNSUPPORTED and "corrected radiation stress" in msg and msg.startswith("pinn_ensemble_lbfgs_loop:"), msg
    rc, msg = _loop(NetDesc(3, 4, 8, 64, (0, 1, 2)), null=("params", "X", "state"))
    assert rc == ERR_UNSUPPORTED and "split request" in msg and "33..64" in msg, msg
    rc, msg = _loop(_desc(dropout_p=0.1))
    assert rc == ERR_UNSUPPORTED and "dropout" in msg, msg


def test_trainer_option_refusals_come_before_any_device_call():
    from pinn_depthestimation_amd import EnsemblePINN

    def cfg(**lb):
        roles = ["h", "U", "V", "eta_mean", "Hrms", "k"]
        return {"layers": {"input_features": 2, "hidden_layers": 2, "hidden_width": 10, "output_features": 6, "dropout_rate": 0.0,
                           "init_type": "xavier"},
                "adam_optimizer": {"max_it": 0, "learning_rate": 1e-4},
                "lbfgs_optimizer": {"max_it": 5, "learning_rate": 1, "history_size": 10, "line_search_fn": "strong_wolfe", **lb},
                "loss": {},
                "data_fidelity": {"inputs": ["x", "y"], "outputs": roles},
                "data_residual": {"inputs": {k: {"requires_grad": ["true"]} for k in "xy"}, "outputs": roles}}

    rs = np.random.RandomState(0)
    Xr, Xf, Tf = rs.rand(20, 2).astype(np.float32), rs.rand(4, 2).astype(np.float32), rs.rand(4, 6).astype(np.float32)
    from pinn_depthestimation_amd.lbfgs import DeviceLBFGS
    # device="cuda:0" on purpose: each of these must be refused before a tensor is moved anywhere or the library is asked
    for lb, word in ((dict(line_search_fn=None), "strong_wolfe"), (dict(line_search_fn="armijo"), "strong_wolfe"),
                     (dict(history_size=0), "history_size"), (dict(history_size=257), "history_size")):
        with pytest.raises(_lib.PinnError) as e:
            EnsemblePINN(Xf, Tf, Xr, cfg(**lb), 3, device="cuda:0", lbfgs_stage=True)
        c = cfg(**lb)["lbfgs_optimizer"]
        with pytest.raises(_lib.PinnError) as want:      # DeviceLBFGS.check_options' own words
            DeviceLBFGS.check_options(1.0, 5, None, c["history_size"], 1e-7, 1e-9, c["line_search_fn"])
        print(lb, e.value)
        assert word in str(e.value) and str(e.value) == str(want.value)
