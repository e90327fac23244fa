"""The host layer's shared rules, without a device: Engine's workspace cache on a counting fake query, the packed-weights
token on CPU tensors, which Engine call each HipEvaluator request reaches (and with which dropout seed) on recording
stand-ins, and the StepLR factor against the expression it replaces."""
import pytest
import torch

from pinn_depthestimation_amd import Engine, NetDesc, ResidualSpec

DESC = NetDesc(3, 6, 2, 16, (0, 1, 2))


# ---- the workspace cache ---------------------------------------------------------------------------------------------
def _fake(asked, rc, nbytes):
    def query():
        asked.append((rc, nbytes))
        return rc, nbytes
    return query


def test_workspace_cache_one_query_per_need_key_and_buffers_only_grow():
    eng, asked = Engine(DESC, "cpu"), []
    rc, a = eng._workspace("buf", ("k", 33), _fake(asked, 0, 0))
    assert rc == 0 and a.numel() == 256 and a.dtype == torch.uint8 and a.device.type == "cpu"      # a need of 0: 256 bytes
    rc, b = eng._workspace("buf", ("k", 33), _fake(asked, 0, 10 ** 6))
    assert rc == 0 and b is a and asked == [(0, 0)]                  # the need key is known: not asked again
    rc, b = eng._workspace("buf", ("k", 34), _fake(asked, 0, 256))
    assert rc == 0 and b is a and asked == [(0, 0), (0, 256)]        # a second need key on the same buffer asks; it fits
    rc, c = eng._workspace("buf", ("k", 1000), _fake(asked, 0, 257))
    assert rc == 0 and c is not a and c.numel() == 257 and len(asked) == 3      # replaced only when the need exceeds it
    for key in (("k", 33), ("k", 34), ("k", 1000)):
        rc, d = eng._workspace("buf", key, _fake(asked, 0, 1))
        assert rc == 0 and d is c                                    # never shrinks, the same object while it fits
    assert len(asked) == 3 and eng._ws["buf"] is c
    rc, o = eng._workspace("other", ("o", 33), _fake(asked, 0, 300))
    assert rc == 0 and o is not c and o.numel() == 300 and eng._ws["buf"] is c and len(asked) == 4      # one buffer per kind


@pytest.mark.parametrize("code", [-2, -1])
def test_workspace_cache_never_remembers_a_failed_query(code):
    eng, asked = Engine(DESC, "cpu"), []
    _, a = eng._workspace("buf", ("k", 33), _fake(asked, 0, 100))
    rc, none = eng._workspace("buf", ("k", 1000), _fake(asked, code, 10 ** 6))
    assert rc == code and none is None and eng._ws["buf"] is a and dict(eng._ws_need) == {("k", 33): 100}
    rc, none = eng._workspace("buf", ("k", 1000), _fake(asked, code, 10 ** 6))
    assert rc == code and none is None and eng._ws["buf"] is a and len(asked) == 3      # asked again
    rc, b = eng._workspace("buf", ("k", 1000), _fake(asked, 0, 1000))
    assert rc == 0 and b.numel() == 1000 and len(asked) == 4
    rc, c = eng._workspace("buf", ("k", 1000), _fake(asked, code, 1))
    assert rc == 0 and c is b and len(asked) == 4                    # a good answer IS remembered
    rc, none = eng._workspace("new", ("k", 1), _fake(asked, code, 1))
    assert rc == code and none is None and "new" not in eng._ws      # no buffer comes out of a failed query


def test_replacing_the_ensemble_buffer_forgets_its_packed_copies():
    eng, asked = Engine(DESC, "cpu"), []
    eng._ens_packed_tok = eng._packed_tok = ("armed",)
    eng._workspace("ens", ("ens", 2, 33), _fake(asked, 0, 100))
    assert eng._ens_packed_tok is None and eng._packed_tok == ("armed",)
    eng._ens_packed_tok = ("armed",)
    eng._workspace("ens", ("ens", 2, 33), _fake(asked, 0, 100))
    eng._workspace("ens", ("ens", 2, 20), _fake(asked, 0, 50))
    eng._workspace("adamext", ("adamext", 33), _fake(asked, 0, 10 ** 4))
    assert eng._ens_packed_tok == ("armed",)                         # it fits / another buffer: the copies are still there
    eng._workspace("ens", ("ens", 2, 1000), _fake(asked, 0, 1000))
    assert eng._ens_packed_tok is None


# ---- the packed-weights token ------------------------------------------------------------------------------------------
def test_packed_token_is_valid_only_when_all_five_agree():
    from pinn_depthestimation_amd.engine import _packed_token, _packed_valid
    ws, params = torch.empty(256, dtype=torch.uint8), torch.zeros(10)
    req = ("ext", "coef", 33, 4, 1, 2, False)
    tok = _packed_token(ws, params, ("t", 1), req)
    assert _packed_valid(tok, ws, params, ("t", 1), req)
    assert not _packed_valid(None, ws, params, ("t", 1), req)
    assert not _packed_valid(tok, torch.empty(256, dtype=torch.uint8), params, ("t", 1), req)      # another workspace OBJECT
    assert not _packed_valid(tok, ws.view(torch.uint8), params, ("t", 1), req)                     # ... even on the same bytes
    assert not _packed_valid(tok, ws, torch.zeros(10), ("t", 1), req)                               # another storage
    assert not _packed_valid(tok, ws, params, ("t", 2), req) and not _packed_valid(tok, ws, params, None, req)
    for other in (("ens", "coef", 33, 4, 1, 2, False), ("ext", "w", 33, 4, 1, 2, False), ("ext", "coef", 34, 4, 1, 2, False),
                  ("ext", "coef", 33, 5, 1, 2, False), ("ext", "coef", 33, 4, 0, 2, False), ("ext", "coef", 33, 4, 1, 1, False),
                  ("ext", "coef", 33, 4, 1, 2, True)):                                              # a request differing in one field
        assert not _packed_valid(tok, ws, params, ("t", 1), other)
    assert _packed_valid(tok, ws, params, ("t", 1), req)             # (nothing above wrote anything)
    params.add_(1)                                                   # a version bump
    assert not _packed_valid(tok, ws, params, ("t", 1), req)
    assert _packed_valid(_packed_token(ws, params, ("t", 1), req), ws, params, ("t", 1), req)


# ---- HipEvaluator: which call each request reaches -------------------------------------------------------------------------
class Rec:
    """Stands in for an Engine: records (its name, the method, the dropout seed it holds at that moment) of every call."""

    def __init__(self, name, log):
        self.name, self.log, self.dropout_seed = name, log, "unset"

    def __getattr__(self, method):
        def f(*a, **kw):
            self.log.append((self.name, method, self.dropout_seed))
            return False
        return f


RESIDUAL_CALL = {"plain": "residual_loss_grad", "nu": "residual2_loss_grad", "coef": "residual_coef_loss_grad",
                 "weighted": "residual_weighted_loss_grad"}
# (Xf, Xr) -> (calls, sums zeroed), RES the mode's residual call: the two terms as a pass each
TWO_PASSES = {
    ("none", "none"): ([], "fr"), ("none", "zero"): ([], "fr"), ("none", "8"): (["RES"], "f"),
    ("zero", "none"): ([], "fr"), ("zero", "zero"): ([], "fr"), ("zero", "8"): (["RES"], "f"),
    ("same", "none"): ([], "fr"), ("same", "zero"): ([], "fr"), ("same", "8"): (["mse_loss_grad", "RES"], ""),
    ("4", "none"): (["mse_loss_grad"], "r"), ("4", "zero"): (["mse_loss_grad"], "r"), ("4", "8"): (["mse_loss_grad", "RES"], ""),
    ("big", "none"): (["mse_loss_grad"], "r"), ("big", "zero"): (["mse_loss_grad"], "r"), ("big", "8"): (["mse_loss_grad", "RES"], ""),
}
# what the plain mode does otherwise: one pass on a shared point set, with or without dropout; one launch for a small
# fidelity set behind the collocation points, without dropout and with merge_sets only
PLAIN_SHARED = (["residual_mse_loss_grad"], "")
PLAIN_MERGED = (["residual_mse_split_loss_grad"], "")
ENGINE_OF = {"none": "eng", "train": "eng_drop", "eval": "eng"}


def _evaluator(mode, dropout, merge, log):
    from pinn_depthestimation_amd.trainer import HipEvaluator
    ev = HipEvaluator.__new__(HipEvaluator)
    ev.eng, ev.eng_drop = Rec("eng", log), (None if dropout == "none" else Rec("eng_drop", log))
    ev.training, ev.fid_cols, ev.merge_sets = dropout != "eval", [0], merge
    ev._cat, ev._cat_src = None, (None, None)
    ev.spec = ResidualSpec("physics_equation", (0, 1, 2, 3, 4, 5), (0, 1), nu=0.1 if mode == "nu" else 0.0)
    if mode == "coef":
        ev.coef, ev.coef_grad = torch.ones(1), torch.ones(1)
    if mode == "weighted":
        ev.point_w = torch.ones(1, 8)
    return ev


@pytest.mark.parametrize("dropout", ["none", "train", "eval"])
@pytest.mark.parametrize("mode", ["plain", "nu", "coef", "weighted"])
def test_hip_evaluator_routing_seeds_and_zeroing(mode, dropout):
    from pinn_depthestimation_amd.trainer import HipEvaluator
    torch.manual_seed(0)
    draws = [int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) for _ in range(3)]
    z = torch.zeros(3)
    for xr in ("none", "zero", "8"):
        Xr = {"none": None, "zero": torch.zeros(0, 2), "8": torch.zeros(8, 2)}[xr]
        for xf in ("none", "zero", "same", "4", "big"):
            Xf = {"none": None, "zero": torch.zeros(0, 2), "same": Xr, "4": torch.zeros(4, 2),
                  "big": torch.zeros(HipEvaluator.MERGE_MAX_FID + 1, 2)}[xf]
            for merge in (True, False) if xf == "4" else (True,):
                calls, zeroed = TWO_PASSES[(xf, xr)]
                if mode == "plain" and (xf, xr) == ("same", "8"):
                    calls, zeroed = PLAIN_SHARED
                if mode == "plain" and (xf, xr) == ("4", "8") and merge and dropout != "train":
                    calls, zeroed = PLAIN_MERGED
                calls = [RESIDUAL_CALL[mode] if c == "RES" else c for c in calls]
                n_draws = len(calls) if dropout == "train" else 0
                log, fid_sums, res_sums = [], torch.ones(1), torch.ones(3)
                ev = _evaluator(mode, dropout, merge, log)
                torch.manual_seed(0)
                ev(z, Xf, z, z, Xr, z, z, fid_sums, res_sums)
                cell = (mode, dropout, xf, xr, merge)
                assert [(e, m) for e, m, _ in log] == [(ENGINE_OF[dropout], c) for c in calls], cell
                assert (("f" if not fid_sums.any() else "") + ("r" if not res_sums.any() else "")) == zeroed, cell
                # one draw immediately before each pass that is launched, fidelity first; none without dropout or in eval mode
                assert [s for _, _, s in log] == (draws[:n_draws] if n_draws else ["unset"] * len(calls)), cell
                assert int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) == draws[n_draws], cell
                if mode == "coef":
                    assert not ev.coef_grad.any(), cell              # zeroed before anything else, whatever is launched


# ---- StepLR ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("size", [3, 1000])
def test_steplr_factor_is_the_expression_it_replaces(size, k):
    from pinn_depthestimation_amd.trainer import steplr_factors
    a = {"learning_rate": 1e-4, "scheduler_gamma": 0.8, "scheduler_step_size": size}
    for s in (0, 1, size - 1, size, 3 * size + 2):
        want = [a["scheduler_gamma"] ** ((s + i) // a["scheduler_step_size"]) for i in range(k)]
        assert steplr_factors(a, s, k) == want
        assert [a["learning_rate"] * f for f in steplr_factors(a, s, k)] == \
            [a["learning_rate"] * a["scheduler_gamma"] ** ((s + i) // a["scheduler_step_size"]) for i in range(k)]
        assert a["learning_rate"] * steplr_factors(a, s)[0] == a["learning_rate"] * a["scheduler_gamma"] ** (s // a["scheduler_step_size"])
