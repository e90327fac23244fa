"""The trainer's call script, without a device: which Engine calls trainer.PINN makes, in which order and with which arguments,
over seven Adam iterations and two closure() calls, in every mode the constructor takes — against a recording made before the
trainer was reorganised (trainer_script_recorded.json, beside this file: plain data).  The engines are recording stand-ins, in
the manner of Rec in test_engine_host_cpu.py.  Every cell runs twice: once with the loop entries (loss_grad_adam_step,
adam_loop_ext, adam_loop_balanced) answering True — the folded path — and once answering False — the classic path.

A call is recorded as its method, its scalars verbatim and its tensors by the trainer attribute they alias (else by shape and a
hash of their bytes).  The stand-in writes a running call counter into every losses / sums / log tensor it is handed, so the
log shows which call filled which row.  After the cell: iter, _adam_step, _sched_steps, _folded_iters, the text of log.txt,
the files written and the iterations of every history.

Shapes: physics_equation, 2 -> 2 x 10 -> 6, N_res = 16, N_fid = 4; log_every = 2, log_flush_every = 3, checkpoint_every = 4,
mat_dump_iter = 5 — the smallest values at which every rule that cuts a run fires within seven iterations.
lbfgs_impl="device" is not here (its control block is read from device state): test_lbfgs_loop_gpu.py covers it.

`python tests/test_trainer_script_cpu.py --record` rewrites the recording from the tree it runs in."""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
RECORDED = os.path.join(HERE, "trainer_script_recorded.json")
PE_OUT = ("h", "U", "V", "eta_mean", "Hrms", "k")
N_RES, N_FID = 16, 4
LOOP_ENTRIES = ("loss_grad_adam_step", "adam_loop_ext", "adam_loop_balanced")
FILLED = ("losses", "sums", "term_sums", "col_sums", "coef_log", "lam_log")
# the trainer's own tensors, by the names other tests and tools read or the trainer's documents use
ATTRS = ("theta", "Xr", "Xf", "Tf", "buf", "_fid_scale", "_res_scale", "_loss_mat", "_adam_m", "_adam_v", "_ring", "_coef",
         "_lam", "_lam_m", "_lam_v", "_w_fixed", "_rad_score", "_last_idx")


def config(dropout=0.0, loss=None):
    return {
        "layers": {"input_features": 2, "hidden_layers": 2, "hidden_width": 10, "output_features": 6, "dropout_rate": dropout,
                   "init_type": "xavier"},
        "adam_optimizer": {"max_it": 7, "learning_rate": 1e-3, "scheduler_step_size": 3, "scheduler_gamma": 0.5,
                           "coefficient_learning_rate": 2e-3, "weight_learning_rate": 4e-3},
        "lbfgs_optimizer": {"max_it": 2, "learning_rate": 1, "max_evaluation": 3, "history_size": 4, "tolerance_grad": 1e-9,
                            "tolerance_change": 1e-12, "line_search_fn": "strong_wolfe"},
        "loss": {"weight_fid_loss": 2, "weight_res_loss": 3, **{f"weight_{k}_loss": 1 + i for i, k in enumerate(PE_OUT)},
                 **(loss or {})},
        "data_fidelity": {"inputs": ["x", "y"], "outputs": list(PE_OUT), "training_points": N_FID},
        "data_residual": {"inputs": {k: {"requires_grad": ["true"]} for k in ("x", "y")}, "outputs": list(PE_OUT)},
    }


def _weights():
    return 0.5 + np.arange(3 * N_RES, dtype=np.float32).reshape(3, N_RES) / 64


# name -> (point set, dropout, constructor keywords); every cell also runs with fold_extras=True where that is not refused
def cells():
    from pinn_depthestimation_amd.trainer import HipEvaluator
    c = {f"plain/{p}": (p, 0.0, {}) for p in ("separate", "shared", "none", "big")}
    c["dropout"] = ("separate", 0.25, {})
    c["eddy_viscosity"] = ("separate", 0.0, dict(eddy_viscosity=0.05))
    c["corrected"] = ("separate", 0.0, dict(corrected=True))
    c["coef/trainable"] = ("separate", 0.0, dict(coefficients={"Cd": 0.01}, trainable_coefficients=("Cd",)))
    c["coef/frozen"] = ("separate", 0.0, dict(coefficients={"Cd": 0.01}))
    c["fixed_weights"] = ("separate", 0.0, dict(residual_weights=_weights()))
    c["sa/square_per_term"] = ("separate", 0.0, dict(self_adaptive={"mask": "square", "per_term": True}))
    c["sa/linear_shared"] = ("separate", 0.0, dict(self_adaptive={"mask": "linear", "per_term": False, "init": 0.5}))
    c["batch/uniform"] = ("separate", 0.0, dict(residual_batch=8))
    c["batch/rad"] = ("separate", 0.0, dict(residual_batch=8, resample="rad", rad_every=3, rad_k=2.0))
    c["batch/rad_importance"] = ("separate", 0.0, dict(residual_batch=8, resample="rad", rad_every=3, rad_k=2.0, rad_importance=True))
    c["batch/rad_fixed_weights"] = ("separate", 0.0, dict(residual_batch=8, resample="rad", rad_every=3, rad_k=2.0,
                                                           residual_weights=_weights()))
    for groups in ("sets", "terms"):
        for mode in ("max_mean", "norm"):
            c[f"balance/{groups}/{mode}"] = ("separate", 0.0, dict(loss_balancing=mode, balance_groups=groups, balance_every=2,
                                                                   balance_alpha=0.25, balance_ref="fidelity"))
    assert HipEvaluator.MERGE_MAX_FID == 2048
    return c


def point_sets(kind):
    from pinn_depthestimation_amd.trainer import HipEvaluator
    g = torch.Generator().manual_seed(11)
    Xr = (torch.rand(N_RES, 2, generator=g) * 2 - 1).numpy()
    if kind == "none":
        return None, None, Xr
    if kind == "shared":
        return Xr, torch.rand(N_RES, 6, generator=g).numpy(), Xr
    n = N_FID if kind == "separate" else HipEvaluator.MERGE_MAX_FID + 1
    return (torch.rand(n, 2, generator=g) * 2 - 1).numpy(), torch.rand(n, 6, generator=g).numpy(), Xr


class Recorder:
    """Stands in for an Engine: records every call, answers the loop entries with `answer`, and writes the running call counter
    into every losses / sums / log tensor it is handed."""

    def __init__(self, name, script, answer):
        self.name, self.script, self.answer, self.dropout_seed, self.trainer = name, script, answer, "unset", None

    def describe(self, v):
        tr = self.trainer
        if torch.is_tensor(v):
            for a in ATTRS:
                t = getattr(tr, a, None)
                if torch.is_tensor(t) and t.numel() and v.numel() and v.untyped_storage().data_ptr() == t.untyped_storage().data_ptr():
                    if v.storage_offset() == t.storage_offset() and v.shape == t.shape:
                        return a
                    return f"{a}+{v.storage_offset() - t.storage_offset()}{list(v.shape)}"
            h = hashlib.sha256(v.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:10]
            return f"{str(v.dtype)[6:]}{list(v.shape)}#{h}"
        if v is tr.spec:
            return "spec"
        if isinstance(v, (list, tuple)):
            return [self.describe(x) for x in v]
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        return repr(v)

    def __getattr__(self, method):
        if method.startswith("__"):
            raise AttributeError(method)

        def call(*a, **kw):
            self.script["n"] += 1
            n = self.script["n"]
            named = {k: self.describe(x) for k, x in sorted(kw.items())}
            if "params_token" in kw:      # (it holds an object's id: recorded as whether it is the module's token of this moment)
                named["params_token"] = kw["params_token"] == self.trainer.dnn.write_token(self.trainer.theta)
            self.script["calls"].append([n, self.name, method, self.dropout_seed, [self.describe(x) for x in a], named])
            for k in FILLED:
                if torch.is_tensor(kw.get(k)):
                    kw[k].fill_(float(n))
            if method in LOOP_ENTRIES:
                return self.answer
            if method == "residual_fields":      # (n_fields, N) small integers: the RAD score is then exact arithmetic
                spec, X = a[0], a[2]
                return (torch.arange(spec.n_fields * X.shape[0], dtype=torch.float32).reshape(spec.n_fields, -1) * 7) % 5
            if method == "forward":
                return torch.zeros(a[1].shape[0], 6)
            return None
        return call


def run_cell(point_set, dropout, kw, fold_extras, answer, tmp):
    from pinn_depthestimation_amd._lib import PinnError
    from pinn_depthestimation_amd.dnn import DNN
    from pinn_depthestimation_amd.trainer import PINN
    Xf, Tf, Xr = point_sets(point_set)
    torch.manual_seed(3)
    model = DNN([2, 10, 10, 6], dropout, "xavier")
    try:
        tr = PINN(Xf, Tf, Xr, config(dropout), device="cpu", dnn=model, log_dir=tmp, log_every=2, log_flush_every=3,
                  checkpoint_every=4, mat_dump_iter=5, mat_dump_path=os.path.join(tmp, "dump.mat"), fold_extras=fold_extras, **kw)
    except PinnError as e:
        return {"refused": str(e)}
    script = {"n": 0, "calls": []}
    tr.evaluator.eng = Recorder("eng", script, answer)
    if tr.evaluator.eng_drop is not None:
        tr.evaluator.eng_drop = Recorder("eng_drop", script, answer)
    for e in (tr.evaluator.eng, tr.evaluator.eng_drop):
        if e is not None:
            e.trainer = tr
    torch.manual_seed(5)      # the dropout seeds come from the global generator
    tr.train_adam(7)
    marks = {"adam": dict(calls=script["n"], iter=tr.iter, folded=tr._folded_iters, adam_folded=bool(tr._adam_folded))}
    for _ in range(2):
        tr.closure()
    tr.flush_log()
    if tr._log_fh is not None:
        tr._log_fh.close()
    log = os.path.join(tmp, "log.txt")
    return {
        "why": [tr.fold_extras_why, tr.balance_why], "calls": script["calls"], "marks": marks,
        "state": dict(iter=tr.iter, adam_step=tr._adam_step, sched_steps=tr._sched_steps, folded_iters=tr._folded_iters,
                      last=[float(x) for x in tr.last]),
        "log": open(log).read() if os.path.exists(log) else None, "files": sorted(os.listdir(tmp)),
        "history": [h[0] for h in tr.history], "coef_history": [list(h) for h in tr._coef_history],
        "weight_history": [list(h) for h in tr.weight_history],
    }


def run_all():
    out = {}
    for name, (point_set, dropout, kw) in cells().items():
        for fold_extras in (False, True):
            for answer in (True, False):
                with tempfile.TemporaryDirectory() as tmp:
                    key = f"{name}|fold_extras={int(fold_extras)}|loops={int(answer)}"
                    out[key] = json.loads(json.dumps(run_cell(point_set, dropout, kw, fold_extras, answer, tmp)))
    return out


def pack(cells_out):
    """The recording as plain data: every distinct call once, in a table, a cell's calls as indices into it; and every
    distinct value of the other fields (log text, files, state, ...) once, a cell's fields as indices into those."""
    table, values, index = [], [], {}

    def ref(store, item):
        s = json.dumps(item)
        if (id(store), s) not in index:
            index[(id(store), s)] = len(store)
            store.append(item)
        return index[(id(store), s)]
    cells = {key: {f: [ref(table, c[1:]) for c in v] if f == "calls" else ref(values, v) for f, v in rec.items()}
             for key, rec in cells_out.items()}
    return {"table": table, "values": values, "cells": cells}


def unpack(recorded):
    """What run_all() returned when `recorded` was packed."""
    table, values = recorded["table"], recorded["values"]
    return {key: {f: [[i + 1] + table[j] for i, j in enumerate(v)] if f == "calls" else values[v] for f, v in rec.items()}
            for key, rec in recorded["cells"].items()}


@pytest.fixture(scope="module")
def script():
    return run_all()


def test_no_cell_was_dropped(script):
    with open(RECORDED) as fh:
        want = json.load(fh)
    assert sorted(script) == sorted(want["cells"]) and len(script) == 4 * len(cells())
    refused = [k for k, v in script.items() if "refused" in v]
    assert all("balance/terms" in k and "fold_extras=1" in k for k in refused), refused      # balance_refusal's last rule alone


def test_trainer_call_script_is_the_recorded_one(script):
    with open(RECORDED) as fh:
        want = unpack(json.load(fh))
    for key, rec in want.items():
        got = script[key]
        assert sorted(got) == sorted(rec), key
        if "refused" in rec:
            assert got == rec, key
            continue
        assert len(got["calls"]) == len(rec["calls"]), (key, [c[2] for c in got["calls"]], [c[2] for c in rec["calls"]])
        for g, w in zip(got["calls"], rec["calls"]):
            assert g == w, (key, g, w)
        for field in rec:
            assert got[field] == rec[field], (key, field, got[field], rec[field])


@pytest.mark.parametrize("log_every,flush_every", [(1, 100), (1, 4), (3, 2), (3, 100), (4, 1)])
def test_ring_writer_rows_of_a_run(log_every, flush_every):
    """_to_ring with the (k, 3) rows of a run of 11 iterations starting at iteration 6: every logged iteration's own row and its
    own row of the per-iteration extras — in one copy (every iteration logged), row by row (every third) and in pieces with a
    flush in between (a ring smaller than the run's logged iterations) — then the same rows beside ONE vector of current
    values.  The script above reaches none of these branches: its runs are of at most three iterations."""
    from pinn_depthestimation_amd.dnn import DNN
    from pinn_depthestimation_amd.trainer import PINN
    Xf, Tf, Xr = point_sets("separate")
    tr = PINN(Xf, Tf, Xr, config(), device="cpu", dnn=DNN([2, 10, 10, 6], 0.0, "xavier"), log_every=log_every,
              log_flush_every=flush_every, checkpoint_every=0, coefficients={"Cd": 0.01})
    k, first = 11, 6
    losses = torch.arange(3.0 * k).reshape(k, 3) + 100 * first
    extras = -torch.arange(1.0 * k).reshape(k, 1)
    logged = [i for i in range(k) if (first + i) % log_every == 0]
    tr._to_ring(first, losses, extras)
    assert len(tr._ring_iters) == len(logged) % tr._ring.shape[0]                 # flushed whenever full, the rest pending
    tr._to_ring(first + k, losses + 1000, tr._coef)
    logged2 = [i for i in range(k) if (first + k + i) % log_every == 0]
    want = [(first + i,) + tuple(losses[i].tolist()) for i in logged] + \
           [(first + k + i,) + tuple((losses[i] + 1000).tolist()) for i in logged2]
    assert tr.history == want
    assert tr._coef_history == [(first + i, float(extras[i])) for i in logged] + \
        [(first + k + i, float(tr._coef[0])) for i in logged2]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    if "--record" in sys.argv:
        with open(RECORDED, "w") as fh:
            json.dump(pack(run_all()), fh, separators=(",", ":"))
        print(f"wrote {RECORDED}: {os.path.getsize(RECORDED)} bytes")
