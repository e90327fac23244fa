"""pinn_residual_fields and the RAD sampler, everything that needs no GPU: the two new C-ABI symbols and their
argument validation (done before the first HIP call), the workspace query, the pure sampling functions of
trainer.py and the constructor's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from pinn_depthestimation_amd import NetDesc, ResidualSpec, _lib
from pinn_depthestimation_amd._lib import (ENGINE_FUSED, ENGINE_FUSED_TILE, ENGINE_GENERIC, ENGINE_WIDE, ERR_INVALID,
                                           ERR_UNSUPPORTED, ERR_WORKSPACE, PinnError)

NS = ("Navier_Stokes", ("t", "x", "y"), ("h", "z", "u", "v"))
PE = ("physics_equation", ("x", "y"), ("h", "U", "V", "eta_mean", "Hrms", "k"))
CF = ("continuity_ftemp", ("x", "y"), ("U", "V", "h"))


def _spec(fam, desc):
    name, inn, outn = fam
    return ResidualSpec.from_names(name, inn, desc.grad_cols, outn)


def _query(desc, spec, N):
    lib = _lib.load()
    need = C.c_int64(-1)
    rc = lib.pinn_query_fields_workspace(C.byref(desc.c_struct()), C.byref(spec.c_struct()), N, C.byref(need))
    return rc, need.value, lib.pinn_last_error().decode()


def _call(desc, cspec, N, params=1, X=1, fields=1, ws=1, ws_bytes=1 << 40):
    """pinn_residual_fields with fake non-NULL pointers: every case here must be refused before they are touched."""
    lib = _lib.load()
    p = lambda v: C.c_void_p(0x1000 if v else None)
    rc = lib.pinn_residual_fields(C.byref(desc.c_struct()), cspec, p(params), p(X), N, p(fields), p(ws), ws_bytes, None)
    return rc, lib.pinn_last_error().decode()


def test_symbols_exported_and_bound_version_unchanged():
    lib = _lib.load()
    for name in ("pinn_query_fields_workspace", "pinn_residual_fields"):
        assert name in _lib.exported_symbols()
        assert getattr(lib, name).restype is C.c_int32
    assert lib.pinn_version() == _lib.ABI_VERSION == 4
    assert _lib.RES_FIELDS == {1: 3, 2: 3, 3: 2, 4: 2}
    d = NetDesc(3, 4, 8, 64, (0, 1, 2))
    assert _spec(NS, d).n_fields == 3 and _spec(CF, NetDesc(2, 3, 4, 20, (0, 1))).n_fields == 2


def test_validation_errors_before_any_device_work():
    d = NetDesc(3, 4, 8, 64, (0, 1, 2))
    s = _spec(NS, d).c_struct()
    # spec: NULL, unknown residual, a role outside the outputs, a direction the network does not carry
    assert _call(d, None, 16)[0] == ERR_INVALID
    bad = _spec(NS, d).c_struct(); bad.residual_id = 9
    rc, msg = _call(d, C.byref(bad), 16); assert rc == ERR_INVALID and "residual_id" in msg
    bad = _spec(NS, d).c_struct(); bad.out_col[3] = 4
    rc, msg = _call(d, C.byref(bad), 16); assert rc == ERR_INVALID and "out_col[3]" in msg
    d2 = NetDesc(3, 4, 8, 64, (0, 1))
    bad = _spec(NS, d).c_struct()
    rc, msg = _call(d2, C.byref(bad), 16); assert rc == ERR_INVALID and "dir_of[2]" in msg
    # K1 against the residual: a two-direction residual on a three-direction network
    d6 = NetDesc(3, 6, 4, 20, (0, 1, 2))
    pe = ResidualSpec.from_names(PE[0], ("x", "y", "t"), d6.grad_cols, PE[2]).c_struct()
    rc, msg = _call(d6, C.byref(pe), 16); assert rc == ERR_UNSUPPORTED and "k = 3" in msg
    assert _query(d6, ResidualSpec.from_names(PE[0], ("x", "y", "t"), d6.grad_cols, PE[2]), 16)[0] == ERR_UNSUPPORTED
    # pointers and sizes
    rc, msg = _call(d, C.byref(s), 16, fields=0); assert rc == ERR_INVALID and "NULL" in msg
    assert _call(d, C.byref(s), 16, params=0)[0] == ERR_INVALID
    assert _call(d, C.byref(s), 16, X=0)[0] == ERR_INVALID
    for N in (0, -3):
        rc, msg = _call(d, C.byref(s), N); assert rc == ERR_INVALID and "at least one point" in msg
        assert _query(d, _spec(NS, d), N)[0] == ERR_INVALID
    rc, need, _ = _query(d, _spec(NS, d), 1000)
    assert rc == 0
    rc, msg = _call(d, C.byref(s), 1000, ws_bytes=need - 1); assert rc == ERR_WORKSPACE and str(need) in msg
    rc, msg = _call(d, C.byref(s), 1000, ws=0); assert rc == ERR_WORKSPACE
    lib = _lib.load()
    assert lib.pinn_query_fields_workspace(C.byref(d.c_struct()), C.byref(s), 16, None) == ERR_INVALID


def test_engine_rules_are_refusals_with_reasons():
    wide = NetDesc(3, 4, 3, 100, (0, 1, 2))
    for e in (ENGINE_FUSED, ENGINE_FUSED_TILE):
        rc, _, msg = _query(wide.with_(engine=e), _spec(NS, wide), 64)
        assert rc == ERR_UNSUPPORTED and "width above 64" in msg
    drop = NetDesc(3, 4, 3, 64, (0, 1, 2), dropout_p=0.2)
    rc, _, msg = _query(drop.with_(engine=ENGINE_FUSED), _spec(NS, drop), 64)
    assert rc == ERR_UNSUPPORTED and "dropout" in msg
    assert _query(drop, _spec(NS, drop), 64)[0] == 0                      # AUTO: the staged path on the generic engine
    assert _query(wide, _spec(NS, wide), 64)[0] == 0                      # AUTO: the staged path on the wide engine
    assert _query(wide.with_(engine=ENGINE_WIDE), _spec(NS, wide), 64)[0] == 0
    narrow = NetDesc(3, 4, 3, 20, (0, 1, 2))
    assert _query(narrow.with_(engine=ENGINE_WIDE), _spec(NS, narrow), 64)[0] == ERR_UNSUPPORTED
    assert _query(narrow.with_(engine=ENGINE_GENERIC), _spec(NS, narrow), 64)[0] == 0


@pytest.mark.parametrize("desc,fam", [
    (NetDesc(3, 4, 8, 64, (0, 1, 2)), NS),                                  # fused tile kernel
    (NetDesc(2, 6, 10, 10, (0, 1), engine=ENGINE_GENERIC), PE),             # staged, generic engine
    (NetDesc(3, 4, 12, 256, (0, 1, 2)), NS),                                # staged, wide engine
], ids=["fused", "generic", "12x256"])
def test_fields_workspace_positive_and_non_decreasing(desc, fam):
    spec = _spec(fam, desc)
    prev = 0
    for N in (1, 15, 16, 17, 777, 4096, 65536, 65537, 1 << 20, 1 << 24):
        rc, need, msg = _query(desc, spec, N)
        assert rc == 0, msg
        assert need > 0 and need >= prev, (N, need, prev)
        prev = need
    # chunked staging: past one chunk the answer no longer grows
    assert _query(desc, spec, 1 << 24)[1] == _query(desc, spec, 1 << 17)[1]
    # ... and the main workspace query answers what it always did (no field staging in it)
    lib = _lib.load()
    main = C.c_int64()
    assert lib.pinn_query_workspace(C.byref(desc.c_struct()), 1 << 20, C.byref(main)) == 0 and main.value > 0


# ---- the sampler ---------------------------------------------------------------------------------------------------
def _cdf_indices(score, u):
    """The definition, in numpy float64: the i with cdf[i-1] <= u * total < cdf[i]."""
    cdf = np.cumsum(np.asarray(score, dtype=np.float64))
    v = np.asarray(u, dtype=np.float64) * cdf[-1]
    return np.minimum(np.array([int(np.sum(cdf <= x)) for x in v]), len(cdf) - 1)


def test_rad_indices_follow_the_float64_cdf():
    from pinn_depthestimation_amd.trainer import rad_indices
    score = torch.tensor([1.0, 0.0, 3.0])
    u = torch.arange(0, 1000, dtype=torch.float64) / 1000
    idx = rad_indices(score, u)
    assert idx.dtype == torch.int64
    assert np.array_equal(idx.numpy(), _cdf_indices(score.numpy(), u.numpy()))
    assert not bool((idx == 1).any()), "a zero-score point owns an empty interval"
    assert int((idx == 0).sum()) == 250 and int((idx == 2).sum()) == 750
    # leading zero score and u = 0: still never drawn
    assert rad_indices(torch.tensor([0.0, 2.0, 0.0, 2.0]), torch.tensor([0.0, 0.5, 0.999999], dtype=torch.float64)).tolist() == [1, 3, 3]
    # float32 scores whose float32 running sum would stall: the CDF is float64
    big = torch.full((1 << 16,), 1.0e-3)
    big[0] = 1.0e5
    got = rad_indices(big, torch.tensor([0.9999999], dtype=torch.float64))
    assert np.array_equal(got.numpy(), _cdf_indices(big.numpy(), [0.9999999]))
    assert int(got) > 0


def test_rad_indices_never_return_N():
    from pinn_depthestimation_amd.trainer import rad_indices
    score = torch.rand(1000, generator=torch.Generator().manual_seed(1)) + 0.1
    u = torch.tensor([1.0, 1.0 - 2.0 ** -53, np.nextafter(np.float32(1.0), np.float32(0.0)).item()], dtype=torch.float64)
    idx = rad_indices(score, u)
    assert idx.tolist()[:2] == [999, 999] and int(idx.max()) == 999
    assert rad_indices(score, torch.tensor([1.0], dtype=torch.float32)).tolist() == [999]


def test_rad_score_constant_residual_draws_uniformly():
    from pinn_depthestimation_amd.trainer import rad_indices, rad_score
    N = 64
    fields = torch.full((3, N), 0.25)                     # eps constant
    s = rad_score(fields, 2.0, 1.0)
    assert s.dtype == torch.float64 and torch.equal(s, torch.full((N,), 2.0, dtype=torch.float64))
    u = (torch.arange(0, 64 * N, dtype=torch.float64) + 0.5) / (64 * N)
    counts = torch.bincount(rad_indices(s, u), minlength=N)
    assert counts.tolist() == [64] * N
    # the definition: eps^k / mean(eps^k) + c with eps = sqrt(sum_f f^2)
    f = torch.tensor([[3.0, 0.0, 1.0], [4.0, 0.0, 0.0]])
    eps = np.array([5.0, 0.0, 1.0])
    want = eps ** 2 / np.mean(eps ** 2) + 0.5
    assert np.allclose(rad_score(f, 2.0, 0.5).numpy(), want, rtol=1e-15)
    # an identically zero residual: the constant alone (uniform), not 0 / 0
    assert torch.equal(rad_score(torch.zeros(2, 5), 1.0, 1.0), torch.ones(5, dtype=torch.float64))


# ---- trainer -------------------------------------------------------------------------------------------------------
CFG = {"layers": {"input_features": 2, "hidden_layers": 3, "hidden_width": 20, "output_features": 3},
       "adam_optimizer": {"max_it": 12, "learning_rate": 1e-3, "scheduler_step_size": 10000, "scheduler_gamma": 0.8},
       "lbfgs_optimizer": {"max_it": 0}, "loss": {"weight_fid_loss": 1, "weight_res_loss": 1},
       "data_fidelity": {"inputs": ["x", "y"], "outputs": []},
       "data_residual": {"inputs": {k: {"requires_grad": ["true"]} for k in "xy"}, "outputs": ["U", "V", "h"]}}


class StubEvaluator:
    """Records the mini-batches it is handed; residual_fields is zero except on `hot` rows."""

    def __init__(self, hot, n_fields=2):
        self.hot, self.n_fields, self.batches, self.scored = hot, n_fields, [], 0

    def __call__(self, theta, Xf, Tf, fid_scale, Xr, res_scale, grad, fid_sums, res_sums):
        self.batches.append(Xr.clone())
        fid_sums.zero_(); res_sums.fill_(1.0)

    def adam_step(self, theta, grad, m, v, step, lr):
        pass

    def residual_fields(self, theta, X):
        self.scored += 1
        f = torch.zeros(self.n_fields, X.shape[0], device=X.device)
        f[0, self.hot.to(X.device)] = 2.0
        return f


def _trainer(**kw):
    from pinn_depthestimation_amd.dnn import DNN
    from pinn_depthestimation_amd.trainer import PINN
    torch.manual_seed(3)
    Xr = torch.rand(4096, 2, generator=torch.Generator().manual_seed(5)) * 2 - 1
    kw.setdefault("evaluator", StubEvaluator(torch.arange(0, 4096, 64)))
    return PINN(None, None, Xr.numpy(), CFG, device="cpu", dnn=DNN([2, 20, 20, 20, 3], 0.0, "xavier"),
                checkpoint_every=0, **kw), Xr


def test_rad_needs_a_minibatch_and_refuses_continuity_only():
    with pytest.raises(PinnError, match="residual_batch"):
        _trainer(resample="rad")
    with pytest.raises(PinnError, match="continuity_only"):
        _trainer(resample="rad", residual="continuity_only")
    with pytest.raises(PinnError, match="continuity_only"):
        _trainer(resample="rad", residual="continuity_only", residual_batch=512)
    with pytest.raises(PinnError, match="uniform"):
        _trainer(resample="adaptive", residual_batch=512)
    tr, _ = _trainer(residual_batch=512)
    assert tr.resample == "uniform"


def test_rad_draws_only_scored_rows_and_rescoring_follows_rad_every():
    tr, Xr = _trainer(residual_batch=512, resample="rad", rad_every=5, rad_c=0.0)
    for _ in range(12):
        tr.adam_step()
    ev = tr.evaluator
    assert ev.scored == 3                                   # iterations 0, 5 and 10
    hot = {tuple(r) for r in Xr[ev.hot].tolist()}
    assert len(ev.batches) == 12
    for b in ev.batches:
        assert b.shape == (512, 2)
        assert all(tuple(r) in hot for r in b.tolist())
    assert not torch.equal(ev.batches[0], ev.batches[1])    # a fresh draw per closure
    assert float(tr._res_unit[0]) == pytest.approx(1.0 / 512)   # no re-weighting: the uniform mini-batch's normaliser


def test_uniform_resampling_draws_what_it_drew_before():
    a, _ = _trainer(residual_batch=512)
    b, _ = _trainer(residual_batch=512, resample="uniform", rad_every=7, rad_k=2.0, rad_c=0.0)
    for _ in range(4):
        a.adam_step(); b.adam_step()
    assert b.evaluator.scored == 0
    assert all(torch.equal(x, y) for x, y in zip(a.evaluator.batches, b.evaluator.batches))
    g = torch.Generator().manual_seed(1234)
    first = torch.randint(0, 4096, (512,), generator=g)
    assert torch.equal(a.evaluator.batches[0], a.Xr.index_select(0, first))
