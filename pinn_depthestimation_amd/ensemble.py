"""ensemble — M networks of one configuration trained side by side: a deep ensemble (same data, different
initialisations) or a seed sweep, for the spread a single trained network of an ill-posed inverse problem cannot give.

The reference's problems fill a few workgroups of the chip (config_CMB.json: 243 collocation + 12 fidelity points on a
10 x 10 network), so M trainers run one after the other cost M times the launches while most of the chip idles.
EnsemblePINN keeps all members' parameters in ONE (M, P) buffer and runs an Adam iteration of all of them in two launches
(Engine.ensemble_adam_step -> pinn_ensemble_adam_loop): member i gets the arithmetic trainer.PINN applies to its own
network.  Same config schema, loss weights and StepLR schedule as trainer.PINN; one learning-rate schedule and one set of
loss weights for all members.

The L-BFGS stage (the reference's one LBFGS.step after Adam) runs for all members at once too: train_lbfgs() ->
lbfgs.EnsembleDeviceLBFGS -> pinn_ensemble_lbfgs_loop, the device-resident loop of trainer.PINN(lbfgs_impl="device") with
a member axis.  Every member runs its own strong-Wolfe line search, its own history ring and its own stopping tests; one
schedule of launches per evaluation advances them all, and a member that has stopped is inert while the others go on.
One set of L-BFGS options (config.lbfgs) for all members.  EnsemblePINN(lbfgs_stage=True).train() is the Adam stage
followed by train_lbfgs().  member(i) is a DNN whose parameters are views of row i — the row both stages write — ready
for inference.Tester, or for trainer.PINN(dnn=...) where one member is to be trained on its own.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from ._lib import PinnError
from .config import PinnConfig, load_config
from .dnn import DNN, activation_id_of, init_flat_params
from .engine import Engine, NetDesc, ResidualSpec
from .lbfgs import DeviceLBFGS, EnsembleDeviceLBFGS
from .parallel import Reducer
from .trainer import _as_f32, anchor_count, loss_arithmetic, steplr_factors

DEFAULT_SEED = 1234      # trainer.PINN's default seed: member i starts from DEFAULT_SEED + i


def member_seeds(members: int, seeds: Optional[Sequence[int]] = None) -> List[int]:
    """The members' initialisation seeds: `seeds` (one per member, all different) or DEFAULT_SEED + i."""
    if int(members) < 1:
        raise PinnError(f"members = {members}: an ensemble has at least one member")
    if seeds is None:
        return [DEFAULT_SEED + i for i in range(int(members))]
    seeds = [int(s) for s in seeds]
    if len(seeds) != int(members):
        raise PinnError(f"{len(seeds)} seeds for {members} members")
    if len(set(seeds)) != len(seeds):
        raise PinnError("two members share a seed: they would be the same network")
    return seeds


def init_ensemble_params(layers: Sequence[int], init_type: str, seeds: Sequence[int]) -> torch.Tensor:
    """(M, P) fp32 on the CPU: row i = dnn.init_flat_params(layers, init_type) drawn from a generator seeded with seeds[i]."""
    return torch.stack([init_flat_params(layers, init_type, torch.Generator().manual_seed(int(s))) for s in seeds])


class EnsemblePINN:
    """M physics-guided networks of one configuration, trained together (see the module docstring).

    fidelity_input / fidelity_true / residual_input as trainer.PINN takes them — shared by all members — or with a
    leading member axis, (M, N, d): one point set per member (bootstrap resamples, different collocation draws)."""

    MAX_RUN = 256      # iterations enqueued by one call (pinn_ensemble_adam_loop)

    def __init__(self, fidelity_input, fidelity_true, residual_input, config, members: int,
                 seeds: Optional[Sequence[int]] = None, residual: Optional[str] = None, device="cuda", engine: int = 0,
                 log_every: int = 1, coefficients=None, trainable_coefficients=(), lbfgs_stage: bool = False):
        cfg = config if isinstance(config, PinnConfig) else load_config(config)
        self.config, self.device = cfg, torch.device(device)
        self.lbfgs_stage = bool(lbfgs_stage)
        if self.lbfgs_stage:      # the options the device loop does not serve, in its own words, before the device is touched
            self._lbfgs_options()
        if coefficients or trainable_coefficients or cfg.raw.get("loss", {}).get("coefficients") \
                or cfg.raw.get("loss", {}).get("trainable_coefficients"):
            raise PinnError("EnsemblePINN has no runtime closure coefficients (loss.coefficients / loss.trainable_coefficients): "
                            "the ensemble kernels carry the constants; use trainer.PINN per member")
        self.seeds = member_seeds(members, seeds)
        self.members = M = len(self.seeds)
        if Reducer().active:
            raise PinnError("EnsemblePINN does not run under data parallelism (the members' gradients are finished on the "
                            "device, no all-reduce in between): train the ensemble in one process")
        residual = residual or cfg.default_residual()
        loss = cfg.raw.get("loss", {})
        if float(loss.get("eddy_viscosity", 0.0)) != 0.0:
            raise PinnError("EnsemblePINN has no second-order residual (loss.eddy_viscosity): use trainer.PINN per member")
        if loss.get("wave_period") is not None:
            raise PinnError("EnsemblePINN has no wave closure (loss.wave_period): the ensemble kernels do not carry the dispersion "
                            "and wave-energy terms; use trainer.PINN per member")
        self.spec = ResidualSpec.from_names(residual, cfg.residual_inputs, cfg.grad_cols, cfg.residual_outputs,
                                            corrected=bool(loss.get("corrected_radiation_stress", False)))
        Xr_in = residual_input
        own = [a is not None and getattr(a, "ndim", 0) == 3 for a in (fidelity_input, fidelity_true, residual_input)]
        if residual == "continuity_only" and own[2]:
            raise PinnError("continuity_only divides its anchor term by a data-dependent count (points with x < threshold): "
                            "with one collocation set per member the count differs by member, and the term scales are shared")
        same_set = fidelity_input is not None and Xr_in is not None and (fidelity_input is Xr_in or (
            cfg.variant == "newmethod" and tuple(fidelity_input.shape) == tuple(Xr_in.shape)
            and torch.equal(_as_f32(fidelity_input, "cpu"), _as_f32(Xr_in, "cpu"))))      # (as trainer.PINN decides it)
        fid_cols = list(range(len(cfg.fidelity_outputs)))
        has_fid = fidelity_input is not None and fidelity_input.shape[-2] > 0 and len(fid_cols) > 0
        self.fid_cols = fid_cols if has_fid else []
        nr = 0 if Xr_in is None else int(Xr_in.shape[-2])
        if nr < 1:
            raise PinnError("EnsemblePINN needs collocation points (residual_input)")
        nfp = int(fidelity_input.shape[-2]) if has_fid else 0
        # the request, as trainer.PINN's evaluator forms it: one point set for both terms / collocation points first, then
        # the fidelity points / the residual alone
        if has_fid and same_set:
            self._N, self._n_res = nr, -1
        elif has_fid:
            self._N, self._n_res = nr + nfp, nr
        else:
            self._N, self._n_res = nr, nr
        # (a sine first layer has no ensemble kernel: the engine's refusal below says so in its own words)
        act = activation_id_of(cfg.init_type, cfg.first_activation)
        self.eng = Engine(NetDesc.from_layers(cfg.layers, cfg.grad_cols, act, engine, 0, cfg.dropout_rate), self.device)
        why = self.eng.ensemble_refusal(self.spec, M, self._N, self._n_res, len(self.fid_cols))
        if why:
            raise PinnError(why)

        # ---- data (nothing above touched the device) ----
        dev = self.device
        Xf, Tf, Xr = (_as_f32(a, dev) for a in (fidelity_input if has_fid else None, fidelity_true if has_fid else None, Xr_in))

        def per_member(t):
            return t if t.dim() == 3 else t.unsqueeze(0).expand(M, *t.shape)
        for t, name in ((Xf, "fidelity_input"), (Tf, "fidelity_true"), (Xr, "residual_input")):
            if t is not None and t.dim() == 3 and t.shape[0] != M:
                raise PinnError(f"{name} has {t.shape[0]} member slices for {M} members")
        if has_fid and same_set:
            self.X = Xr
        elif has_fid:
            if Xf.dim() == 3 or Xr.dim() == 3:
                self.X = torch.cat([per_member(Xr), per_member(Xf)], 1).contiguous()
            else:
                self.X = torch.cat([Xr, Xf], 0).contiguous()
        else:
            self.X = Xr
        self.T = Tf
        self.n_res, self.n_fid = nr, nfp
        self.weight_fidelity, self.weight_residual = cfg.weight_fid, cfg.weight_res
        nf, nt = len(self.fid_cols), self.spec.n_terms
        # the trainer's loss arithmetic, one set of scales for all members
        self._fid_unit, self._res_unit, self._fid_scale, self._res_scale, self._loss_mat = loss_arithmetic(
            cfg, self.spec, nf, nfp, nr, dev, anchor_count(cfg, self.spec, Xr) if residual == "continuity_only" else None)

        # ---- parameters and optimiser state ----
        self.theta = init_ensemble_params(cfg.layers, cfg.init_type, self.seeds).to(dev).contiguous()
        P = self.theta.shape[1]
        self.grad = torch.zeros(M, P, dtype=torch.float32, device=dev)
        self._adam_m, self._adam_v = torch.zeros_like(self.grad), torch.zeros_like(self.grad)
        self._res_sums = torch.zeros(M, nt, dtype=torch.float32, device=dev)
        self._fid_sums = torch.zeros(M, nf, dtype=torch.float32, device=dev) if nf else None
        self._run_losses = torch.zeros(self.MAX_RUN, M, 3, dtype=torch.float32, device=dev)
        self._members = {}
        self.iter = self._adam_step = self._sched_steps = 0
        self.adam_maxit = cfg.adam["max_it"]
        self.log_every = max(int(log_every), 1)
        self._history: List[tuple] = []
        self._pending: List[Tuple[List[int], torch.Tensor]] = []      # (iterations, their (n, M, 3) rows on the device)
        self.device_lbfgs: Optional[EnsembleDeviceLBFGS] = None       # built by train_lbfgs(): it binds the point sets
        self._lbfgs_traces: List[torch.Tensor] = []                   # one (slots, M, LBFGS_TRACE_COLS) CPU tensor per run

    # ---- members ---------------------------------------------------------------------------------------------------
    def member(self, i: int) -> DNN:
        """Member i as a dnn.DNN whose Linear parameters are views of row i of `theta` — the row train_adam and train_lbfgs
        write: what it is told to do (inference.Tester, load_state_dict, trainer.PINN(dnn=...)) happens to the ensemble's
        own buffer."""
        i = int(i)
        if not 0 <= i < self.members:
            raise PinnError(f"member {i} of an ensemble of {self.members}")
        dnn = self._members.get(i)
        if dnn is None:
            with torch.random.fork_rng(devices=[]):      # (the module's own initial draw is thrown away: leave the caller's stream alone)
                dnn = DNN(self.config.layers, self.config.dropout_rate, self.config.init_type)
            row, off = self.theta[i], 0
            for p in dnn._ordered_params():
                n = p.numel()
                p.data = row[off:off + n].view_as(p)
                off += n
            dnn._flat = row
            self._members[i] = dnn
        return dnn

    def _write_token(self):
        """Changes when a member's module was written through torch (engine.py, packed-weights token)."""
        return tuple((i, d.write_token()) for i, d in sorted(self._members.items()))

    # ---- training ----------------------------------------------------------------------------------------------------
    def train_adam(self, n: int):
        """n Adam iterations of every member (train.py:188-193 with the StepLR schedule), in runs of at most MAX_RUN
        iterations enqueued by one call each: two launches per iteration, whatever the number of members."""
        a = self.config.adam
        n = int(n)
        while n > 0:
            k = min(n, self.MAX_RUN)
            lrs = [a["learning_rate"] * f for f in steplr_factors(a, self._sched_steps, k)]
            out = self._run_losses[:k]
            nf = len(self.fid_cols)
            ok = self.eng.ensemble_adam_step(self.spec, self._res_scale, self.theta, self.X, self._n_res, self.grad, self._adam_m,
                                             self._adam_v, self._adam_step + 1, lrs, T=self.T if nf else None,
                                             out_col=self.fid_cols, col_scale=self._fid_scale if nf else None,
                                             term_sums=self._res_sums, col_sums=self._fid_sums, loss_rows=self._loss_mat,
                                             losses=out, params_token=self._write_token())
            if not ok:
                raise PinnError(self.eng.last_error())
            its = [self.iter + 1 + i for i in range(k) if (self.iter + 1 + i) % self.log_every == 0]
            if its:
                idx = torch.tensor([it - self.iter - 1 for it in its], device=self.device)
                self._pending.append((its, out.index_select(0, idx)))
            self.iter += k
            self._adam_step += k
            self._sched_steps += k
            n -= k

    def _lbfgs_options(self):
        """config.lbfgs as lbfgs.DeviceLBFGS.check_options takes it (PinnError in its words for what the loop does not do)."""
        lb = self.config.lbfgs
        return DeviceLBFGS.check_options(lb["learning_rate"], lb["max_it"], lb.get("max_evaluation"), lb["history_size"],
                                         lb["tolerance_grad"], lb["tolerance_change"], lb["line_search_fn"])

    def train_lbfgs(self):
        """The L-BFGS stage of every member (train.py:200, one LBFGS.step each) through lbfgs.EnsembleDeviceLBFGS, with
        the options of config.lbfgs as trainer.PINN.train_lbfgs_device takes them: runs of up to RUN evaluations enqueued
        by one call each, until every member has stopped.  self.iter advances by the evaluations of the member that took
        the most; every evaluation's three losses are kept per member (lbfgs_history)."""
        o = self._lbfgs_options()
        nf = len(self.fid_cols)
        opt = self.device_lbfgs = EnsembleDeviceLBFGS(
            self.eng, self.spec, self.theta, self.X, self._n_res, self._res_scale, self._loss_mat, 2,
            T=self.T if nf else None, out_col=self.fid_cols, col_scale=self._fid_scale if nf else None,
            lr=o.lr, max_iter=o.max_iter, max_eval=o.max_eval, history_size=o.history_size,
            tolerance_grad=o.tolerance_grad, tolerance_change=o.tolerance_change)
        opt.step(after_run=self._lbfgs_traces.append)
        self.iter += max(opt.func_evals)
        return opt

    def train(self):
        """The Adam stage of the configuration (adam_optimizer.max_it iterations); with lbfgs_stage=True followed by the
        L-BFGS stage of all members (train_lbfgs) where lbfgs_optimizer.max_it > 0, as trainer.PINN.train does."""
        self.train_adam(self.adam_maxit)
        if self.lbfgs_stage and self.config.lbfgs["max_it"] > 0:
            self.train_lbfgs()

    @property
    def lbfgs_history(self) -> List[torch.Tensor]:
        """Per member, an (evaluations, 3) float32 CPU tensor: [fidelity, residual, total] of every evaluation of its
        L-BFGS stage, in order, from the loop's trace (inert slots — after the member's stop — left out)."""
        from ._lib import LBFGS_TRACE_COLS
        tr = torch.cat(self._lbfgs_traces) if self._lbfgs_traces else torch.zeros(0, self.members, LBFGS_TRACE_COLS, dtype=torch.float64)
        return [tr[tr[:, j, 2] != 0, j, 10:13].to(torch.float32) for j in range(self.members)]

    @property
    def history(self) -> List[tuple]:
        """(iteration, fidelity (M,), residual (M,), total (M,)) of every logged iteration: CPU tensors, formed on the
        device by the finishing kernel (loss_rows) and brought over here, one synchronisation per call."""
        for its, rows in self._pending:
            rows = rows.cpu()
            for j, it in enumerate(its):
                self._history.append((it, rows[j, :, 0].clone(), rows[j, :, 1].clone(), rows[j, :, 2].clone()))
        self._pending = []
        return self._history

    # ---- inference -------------------------------------------------------------------------------------------------------
    def predict(self, inputs) -> torch.Tensor:
        """Every member's outputs on a grid: (N, d_in) -> (M, N, d_out), M calls of Engine.forward."""
        X = _as_f32(inputs, self.device)
        return torch.stack([self.eng.forward(self.theta[i], X) for i in range(self.members)])

    def predict_stats(self, inputs) -> Tuple[torch.Tensor, torch.Tensor]:
        """(mean, unbiased standard deviation) over the members, each (N, d_out)."""
        Y = self.predict(inputs)
        return Y.mean(0), Y.std(0, unbiased=True)
