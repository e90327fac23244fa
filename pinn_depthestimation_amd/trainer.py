"""trainer — the `pinn` training harness of train.py:46-200 / train_newmethod.py:46-209 on the
HIP engine: same constructor arguments, same loss arithmetic, same Adam+StepLR then one
LBFGS.step(closure) schedule, same log.txt / model_{iter}.pth artefacts.

One closure evaluation =
    grad <- 0
    fidelity   : pinn_mse_loss_grad       (train.py:131-141)
    residual   : pinn_residual_loss_grad  (train.py:144-154 + loss.backward(), :191)
    all-reduce : [grad | loss sums] over the data-parallel group (parallel.py)
The reference logs every call (train.py:160-173), i.e. one host synchronisation per iteration.
Here the three loss values of a logged iteration are copied into a device-side ring and written
out `log_flush_every` entries at a time (one synchronisation per flush; `log_flush_every=1`
restores line-by-line behaviour): log.txt has the same lines, just written in batches.
"""
from __future__ import annotations

import math
import json
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import PinnError
from .config import PinnConfig, load_config, self_adaptive_options
from .dnn import DNN
from .engine import ACTIVATION_OF_INIT, RESIDUAL_ROLES, Engine, NetDesc, ResidualSpec
from .lbfgs import DeviceLBFGS, FlatLBFGS
from .parallel import Reducer


def rad_cdf(score: torch.Tensor) -> torch.Tensor:
    """Running sum of the scores in float64 (a float32 sum over a large pool stalls once it outgrows its addends)."""
    return torch.cumsum(score.to(torch.float64), 0)


def rad_indices(score: torch.Tensor, u: torch.Tensor, cdf: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Draw indices with probability proportional to `score` (N non-negative values) from uniforms `u` in [0, 1):
    inverse-CDF sampling, idx = searchsorted(cdf, u * cdf[-1]) with the CDF accumulated in float64, clamped to N - 1
    (u -> 1 may land on the last edge).  side='right': a zero-score point owns an empty interval and is never drawn.
    `cdf`: rad_cdf(score) kept from an earlier call (the trainer forms it once per re-scoring, not once per closure)."""
    if cdf is None:
        cdf = rad_cdf(score)
    idx = torch.searchsorted(cdf, u.to(torch.float64) * cdf[-1], right=True)
    return idx.clamp_(max=score.numel() - 1)


def rad_score(fields: torch.Tensor, k: float, c: float) -> torch.Tensor:
    """RAD's sampling density (Wu et al. 2023, eq. 2) up to normalisation: eps^k / mean(eps^k) + c with
    eps_n = sqrt(sum_f fields[f][n]^2), in float64.  An all-zero residual leaves the constant (uniform)."""
    eps = fields.to(torch.float64).square().sum(0).sqrt()
    ek = eps.pow(k)
    m = ek.mean()
    return torch.where(m > 0, ek / m, torch.zeros_like(ek)) + c


def rad_importance_weights(score: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """Importance weights of a mini-batch drawn at `idx` with probability proportional to `score` (rad_indices): one row
    w_b = mean(score) / score[idx_b], formed in float64 and cast to float32 once.  With p_n = score_n / sum(score) the batch
    mean of w f^2 is then an unbiased estimate of the pool mean of f^2: sum_n p_n w_n f_n^2 = mean(f^2).  Only drawn points
    are divided by, and a zero-score point is never drawn."""
    s64 = score.to(torch.float64)
    return (s64.mean() / s64.index_select(0, idx)).to(torch.float32).reshape(1, -1).contiguous()


def sa_weights(lam: torch.Tensor, mask: str) -> torch.Tensor:
    """The self-adaptive weights w = m(lambda): lambda^2 ("square") or lambda ("linear")."""
    return lam * lam if mask == "square" else lam.clone()


def sa_weight_grad(lam: torch.Tensor, fields: torch.Tensor, term_scale: torch.Tensor, mask: str) -> torch.Tensor:
    """The gradient Adam DESCENDS along so that lambda ASCENDS the weighted residual loss sum_t s_t sum_n m(lambda_t[n]) f_t[n]^2:
    -s_t m'(lambda) f^2, the shape of lambda.  lam is (rows, N): rows == 1 shares one multiplier among the weighted terms
    (its gradient sums over them), otherwise row t belongs to term t.  fields: the pass's unweighted signed fields
    (n_fields, N), of which the first n_w = min(len(term_scale), n_fields) are weighted terms."""
    n_w = min(int(term_scale.numel()), int(fields.shape[0]))
    sf = term_scale[:n_w].reshape(-1, 1) * fields[:n_w] * fields[:n_w]          # s_t f_t^2, (n_w, N)
    if lam.shape[0] == 1:
        sf = sf.sum(0, keepdim=True)
    elif lam.shape[0] != n_w:
        raise PinnError(f"sa_weight_grad: lambda has {lam.shape[0]} rows, the residual {n_w} weighted terms")
    return -(2.0 * lam * sf if mask == "square" else sf)


def weighted_refusal(residual_weights=False, self_adaptive=False, rad_importance=False, reducer_active=False, eddy_viscosity=0.0,
                     coefficients=False, corrected=False, lbfgs_impl="flat", custom_evaluator=False, residual_batch=None,
                     resample="uniform", wave=False):
    """Why trainer.PINN cannot run this configuration with point weights on the residual — fixed residual_weights, self_adaptive
    or rad_importance (None: it can, or none is asked for).  Pure host logic, evaluated before anything touches a device."""
    if not (residual_weights or self_adaptive or rad_importance):
        return None
    if reducer_active:
        return "point weights on the residual do not run under data parallelism (the weights are not sharded with the points)"
    if eddy_viscosity:
        return "point weights on the residual do not run with eddy_viscosity != 0 (the second-order residual has no weighted form)"
    if coefficients:
        return "point weights on the residual do not run with runtime closure coefficients (the coefficient kernels have no weights)"
    if wave:
        return "point weights on the residual do not run with the wave closure (wave_period: its kernels have no weights)"
    if corrected:
        return "point weights on the residual do not run with the corrected radiation stress (the corrected kernels have no weights)"
    if lbfgs_impl == "device":
        return "point weights on the residual do not run with lbfgs_impl=\"device\" (the device loop enqueues the unweighted loss entries); use lbfgs_impl=\"flat\""
    if custom_evaluator:
        return "point weights on the residual need the library's own evaluator, not a custom one"
    if rad_importance and resample != "rad":
        return "rad_importance re-weights the RAD mini-batch: it needs resample='rad'"
    if self_adaptive and (residual_batch is not None or resample == "rad"):
        return "self_adaptive does not run with residual_batch or resample='rad' (a multiplier belongs to a point of a fixed set)"
    if self_adaptive and residual_weights:
        return "self_adaptive and residual_weights are two sources of the same weights: give one"
    return None


def device_lbfgs_refusal(reducer_active, residual_batch, eddy_viscosity, custom_evaluator, line_search_fn, dropout_rate=0.0,
                         coefficients=False):
    """Why lbfgs_impl="device" cannot run this configuration (None: it can).  The device loop enqueues a fixed schedule of
    evaluations of ONE loss request; whatever needs the host, a second call or fresh randomness per evaluation is out."""
    flat = '; use lbfgs_impl="flat"'
    if reducer_active:
        return "lbfgs_impl=\"device\" does not run under data parallelism (the all-reduce of every evaluation is issued by the host)" + flat
    if residual_batch is not None:
        return "lbfgs_impl=\"device\" does not run with residual_batch (a mini-batch is drawn by the host for every evaluation)" + flat
    if eddy_viscosity:
        return "lbfgs_impl=\"device\" does not run with eddy_viscosity > 0 (the second-order residual is two calls per evaluation)" + flat
    if custom_evaluator:
        return "lbfgs_impl=\"device\" runs the library's own loss pass, not a custom evaluator" + flat
    if line_search_fn != "strong_wolfe":
        return f"lbfgs_impl=\"device\" runs the strong_wolfe line search only (line_search_fn={line_search_fn!r})" + flat
    if dropout_rate and dropout_rate > 0:
        return "lbfgs_impl=\"device\" does not run with dropout (a seed per forward pass has no place in a fixed schedule)" + flat
    if coefficients:
        return "lbfgs_impl=\"device\" does not run with runtime closure coefficients (the device loop enqueues the loss entries that carry the constants)" + flat
    return None


def coefficient_refusal(residual, coefficients, trainable, corrected=False, eddy_viscosity=0.0, reducer_active=False,
                        resample="uniform", custom_evaluator=False, wave=False):
    """Why trainer.PINN cannot run this configuration with runtime closure coefficients (None: it can, or none are asked
    for).  Pure host logic.  coefficients: {name: value}; trainable: names."""
    coefficients, trainable = dict(coefficients or {}), tuple(trainable or ())
    if not coefficients and not trainable:
        return None
    if residual not in RESIDUAL_ROLES:
        return f"unknown residual {residual!r}"
    if wave:
        return "the wave closure (wave_period) has no coefficient form (its kernels carry the constant Cd)"
    if corrected:
        return "the corrected radiation stress has no coefficient form (the corrected kernels carry the constant Cd)"
    have = _lib.RES_COEFS[RESIDUAL_ROLES[residual][0]]
    for name in list(coefficients) + list(trainable):
        if name not in have:
            return (f"residual {residual!r} has no coefficient {name!r}: " +
                    (f"it has {', '.join(have)}" if have else "it has no coefficient at all"))
    if eddy_viscosity:
        return "runtime coefficients do not run with eddy_viscosity != 0 (the second-order residual carries the constants)"
    if reducer_active:
        return "runtime coefficients do not run under data parallelism (the coefficient gradient has no place in the all-reduce)"
    if resample == "rad":
        return "runtime coefficients do not run with resample='rad' (the field kernels carry the constants)"
    if custom_evaluator:
        return "runtime coefficients need the library's own evaluator, not a custom one"
    return None


def fold_extras_refusal(fold_extras=False, coefficients=False, weighted=False, rad_importance=False, residual_batch=None,
                        resample="uniform", dropout_rate=0.0, reducer_active=False, eddy_viscosity=0.0, custom_evaluator=False,
                        fold_adam=True):
    """Why Adam iterations with runtime closure coefficients or point weights stay on the classic path although
    fold_extras is asked for (None: they run as device-enqueued runs, Engine.adam_loop_ext — or there is nothing to decide:
    the option is off, or the configuration has neither coefficients nor weights).  Nothing is refused outright: the classic
    path computes the same iteration.  Pure host logic."""
    if not fold_extras or not (coefficients or weighted or rad_importance):
        return None
    if not fold_adam:
        return "fold_adam is off: every Adam iteration takes the classic path"
    if reducer_active:
        return "data parallelism: the all-reduce of every iteration is issued by the host"
    if eddy_viscosity:
        return "eddy_viscosity != 0: the second-order residual is layer kernels per chunk, not one pass"
    if custom_evaluator:
        return "a custom evaluator: the device-enqueued runs are the library's own"
    if rad_importance or resample == "rad":
        return "resample='rad': the host draws and weights a mini-batch for every iteration"
    if residual_batch is not None:
        return "residual_batch: the host draws a mini-batch for every iteration"
    if dropout_rate and dropout_rate > 0:
        return "dropout: a fresh seed per forward pass has no place in an enqueued run"
    return None


def balance_refusal(loss_balancing=None, groups="sets", every=10, alpha=0.1, ref="residual", fold_extras=False, coefficients=False,
                    weighted=False, rad_importance=False, eddy_viscosity=0.0, reducer_active=False, custom_evaluator=False,
                    wave=False):
    """Why trainer.PINN cannot run this configuration with gradient-statistics loss balancing (None: it can, or none is asked
    for).  Pure host logic, evaluated before anything touches a device."""
    if loss_balancing is None:
        return None
    if loss_balancing not in ("max_mean", "norm"):
        return f"loss_balancing={loss_balancing!r}: use None, 'max_mean' or 'norm'"
    if groups not in ("sets", "terms"):
        return f"balance_groups={groups!r}: use 'sets' (residual, fidelity) or 'terms' (a group per weighted residual term, and fidelity)"
    if int(every) < 1:
        return f"balance_every={every} must be >= 1"
    if not (0.0 < float(alpha) <= 1.0):
        return f"balance_alpha={alpha} must lie in (0, 1]"
    if ref not in ("residual", "fidelity"):
        return f"balance_ref={ref!r}: use 'residual' or 'fidelity'"
    if coefficients:
        return "loss balancing does not run with runtime closure coefficients (their gradient belongs to no group)"
    if weighted or rad_importance:
        return ("loss balancing does not run with point weights on the residual (residual_weights, self_adaptive, rad_importance): "
                "two schemes would set the same weights")
    if eddy_viscosity:
        return "loss balancing does not run with eddy_viscosity != 0"
    if wave:
        return "loss balancing does not run with the wave closure (wave_period: the balanced loop has no pass for it)"
    if reducer_active:
        return "loss balancing does not run under data parallelism (the statistics are taken on one rank's gradients)"
    if custom_evaluator:
        return "loss balancing needs the library's own evaluator, not a custom one"
    if groups == "terms" and fold_extras:
        return "balance_groups='terms' does not run with fold_extras (the device-enqueued runs balance the two point sets; a group per term needs one-hot passes)"
    return None


def wave_refusal(wave_period, wave_gamma, residual, corrected, eddy_viscosity=0.0):
    """Why trainer.PINN cannot train with the wave closure as configured (None: it can, or no wave_period is given).  Pure
    host logic."""
    if wave_period is None:
        return None
    if residual != "physics_equation" or not corrected:
        return ("wave_period is the wave closure of physics_equation with the corrected radiation stress (corrected=True / "
                f"loss.corrected_radiation_stress): got residual {residual!r}, corrected={bool(corrected)}")
    if not (float(wave_period) > 0 and float(wave_gamma) > 0):
        return f"the wave closure needs wave_period > 0 and wave_gamma > 0 (got {wave_period}, {wave_gamma})"
    if eddy_viscosity:
        return "the wave closure (wave_period) does not run with eddy_viscosity != 0 (it has no second-order form)"
    return None


def balance_fold_refusal(residual_batch=None, resample="uniform", dropout_rate=0.0, fold_adam=True):
    """Why balanced Adam iterations stay on the classic path although fold_extras is on (None: they run as device-enqueued
    runs, Engine.adam_loop_balanced, where the engine serves them).  Nothing is refused: the classic path computes the same
    iteration.  Pure host logic."""
    if not fold_adam:
        return "fold_adam is off: every Adam iteration takes the classic path"
    if resample == "rad":
        return "resample='rad': the host draws a mini-batch for every iteration"
    if residual_batch is not None:
        return "residual_batch: the host draws a mini-batch for every iteration"
    if dropout_rate and dropout_rate > 0:
        return "dropout: a fresh seed per forward pass has no place in an enqueued run"
    return None


def _as_f32(a, device) -> Optional[torch.Tensor]:
    if a is None:
        return None
    t = torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a)
    return t.to(device=device, dtype=torch.float32).contiguous()


def _dropout_seed() -> int:
    """A fresh seed for one forward pass's dropout masks, from torch's global CPU generator."""
    return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())


def steplr_factors(adam: dict, sched_steps: int, k: int = 1) -> List[float]:
    """StepLR(step_size, gamma) stepped once per Adam iteration (train.py:109-113,193): the factor on the base learning
    rate at schedule steps sched_steps .. sched_steps + k - 1.  `adam`: the configuration's adam_optimizer section."""
    return [adam["scheduler_gamma"] ** ((sched_steps + i) // adam["scheduler_step_size"]) for i in range(k)]


def anchor_count(cfg: PinnConfig, spec: ResidualSpec, Xr: torch.Tensor) -> torch.Tensor:
    """continuity_only's data-dependent normaliser: how many of the points Xr have x < threshold, a (1,) float32 tensor."""
    xcol = cfg.grad_cols[spec.dir_of[0]]
    return (Xr[:, xcol] < spec.threshold).sum().to(torch.float32).reshape(1)


def loss_arithmetic(cfg: PinnConfig, spec: ResidualSpec, nf: int, n_fid: int, n_res: int, device, anchor=None):
    """The loss arithmetic of train.py:131-157 as (fid_unit, res_unit, fid_scale, res_scale, loss_mat): the sums of squares
    the kernels return become means with the units, weighted terms of the total with the scales (= hand-set weight x unit),
    and [fidelity, residual, total] = loss_mat @ [fid sums | res sums].  nf fidelity outputs on n_fid points; n_res: the
    residual's normaliser (the point count; a mini-batch's size x the world size); anchor: continuity_only's anchor_count,
    summed over the ranks — its second term's normaliser."""
    if cfg.variant == "newmethod":
        fid_w = [1.0] * nf                                                 # F.mse_loss, unweighted sum
    else:
        fid_w = [cfg.output_weight(k) for k in cfg.fidelity_outputs][:nf]  # train.py:94-95,140
    fid_unit = torch.tensor(fid_w, dtype=torch.float32, device=device) / max(n_fid, 1)
    if anchor is not None:
        res_unit = torch.cat([torch.tensor([1.0 / n_res], device=device), 1.0 / anchor, torch.zeros(1, device=device)])
    else:
        res_unit = torch.full((spec.n_terms,), 1.0 / max(n_res, 1), dtype=torch.float32, device=device)
    m = torch.zeros(3, nf + spec.n_terms, dtype=torch.float32, device=device)
    m[0, :nf] = fid_unit
    m[1, nf:] = res_unit
    m[2] = cfg.weight_fid * m[0] + cfg.weight_res * m[1]                   # train.py:157
    return fid_unit, res_unit, (cfg.weight_fid * fid_unit).contiguous(), (cfg.weight_res * res_unit).contiguous(), m.contiguous()


class HipEvaluator:
    """Local-shard loss sums and gradient through libpinn_hip.so."""

    def __init__(self, cfg_layers, init_type, grad_cols, spec: ResidualSpec, fid_cols: Sequence[int], device,
                 engine: int = 0, precision: int = 0, dropout_rate: float = 0.0, activation: Optional[int] = None):
        # (activation: DNN.activation_id — the sine first layer is no function of init_type)
        act = ACTIVATION_OF_INIT[init_type] if activation is None else int(activation)
        self.dropout_rate = float(dropout_rate)
        self.eng = Engine(NetDesc.from_layers(cfg_layers, grad_cols, act, engine, precision), device)
        # training-mode dropout (dnn.py:38 with train.py:186): its own engine (generic kernels carry the mask)
        self.eng_drop = Engine(NetDesc.from_layers(cfg_layers, grad_cols, act, 0, 0, self.dropout_rate), device) \
            if self.dropout_rate > 0.0 else None
        self.training = True
        self.spec, self.fid_cols = spec, list(fid_cols)
        self.merge_sets = True      # one launch for both loss terms when the fidelity set is small
        self._cat = None            # [collocation points ; fidelity points], allocated once
        self._cat_src = (None, None)   # the very tensor OBJECTS whose rows _cat currently holds

    MERGE_MAX_FID = 2048   # fidelity points ride through the jet kernel (4x their own work): only when few
    # runtime closure coefficients (PINN(coefficients=..., trainable_coefficients=...)): the device tensor the residual reads
    # them from, and where their gradient goes (None: values only — frozen, or nothing trainable); set by the trainer
    coef = None
    coef_grad = None
    # point weights on the residual (PINN(residual_weights=..., self_adaptive=..., rad_importance=...)): the device tensor
    # (w_rows, N) matching the collocation points of the call, and where the pass's unweighted signed fields go (None: not
    # wanted); set by the trainer
    point_w = None
    fields_out = None

    def _dropping(self) -> bool:
        return self.eng_drop is not None and self.training

    def _engine(self):
        """The engine of the next pass.  In training mode with dropout it is eng_drop, and a fresh seed is drawn for the
        pass's masks first: one draw immediately before every pass that IS launched (the reference runs the network twice
        per loss_func call, train.py:133,148: two forward passes, two masks)."""
        if not self._dropping():
            return self.eng
        self.eng_drop.dropout_seed = _dropout_seed()
        return self.eng_drop

    def _split_pass(self, theta, Xf, Tf, fid_scale, Xr, grad, fid_sums, res_sums, residual):
        """The two loss terms as a pass each: the fidelity term through mse_loss_grad, then residual(engine) on the
        collocation points; a term without points launches nothing and zeroes its sums."""
        if Xf is not None and Xf.shape[0] > 0:
            self._engine().mse_loss_grad(theta, Xf, Tf, self.fid_cols, fid_scale, grad, sums=fid_sums)
        else:
            fid_sums.zero_()
        if Xr is not None and Xr.shape[0] > 0:
            residual(self._engine())
        else:
            res_sums.zero_()

    def __call__(self, theta, Xf, Tf, fid_scale, Xr, res_scale, grad, fid_sums, res_sums):
        if self.point_w is not None:
            # point weights (self.point_w) on the residual; the pass's unweighted signed fields go to self.fields_out
            def residual(e):
                e.residual_weighted_loss_grad(self.spec, self.point_w, res_scale, theta, Xr, grad, sums=res_sums, fields=self.fields_out)
        elif self.coef is not None:
            # runtime closure coefficients (self.coef); self.coef_grad, when set, is overwritten with d loss / d coef
            if self.coef_grad is not None:
                self.coef_grad.zero_()

            def residual(e):
                e.residual_coef_loss_grad(self.spec, self.coef, res_scale, theta, Xr, grad, self.coef_grad, sums=res_sums)
        elif self.spec.nu != 0:
            # the lateral-mixing term: the second-order entry (also where both terms share one point set)
            def residual(e):
                e.residual2_loss_grad(self.spec, res_scale, theta, Xr, grad, sums=res_sums)
        else:
            if Xf is not None and Xf is Xr and Xr.shape[0] > 0:
                # one point set for both terms (train_newmethod.py:122-159): one pass, one forward, one dropout mask
                self._engine().residual_mse_loss_grad(self.spec, res_scale, Tf, self.fid_cols, fid_scale, theta, Xr, grad,
                                                      term_sums=res_sums, col_sums=fid_sums)
                return
            if (not self._dropping() and self.merge_sets and Xf is not None and Xr is not None
                    and 0 < Xf.shape[0] <= self.MERGE_MAX_FID and Xr.shape[0] > 0):
                # train.py:131-157 in ONE launch: collocation points first, fidelity points after them
                cat = self._merged(Xr, Xf)
                self.eng.residual_mse_split_loss_grad(self.spec, res_scale, Tf, self.fid_cols, fid_scale, theta, cat,
                                                      Xr.shape[0], grad, term_sums=res_sums, col_sums=fid_sums)
                return

            def residual(e):
                e.residual_loss_grad(self.spec, res_scale, theta, Xr, grad, sums=res_sums)
        self._split_pass(theta, Xf, Tf, fid_scale, Xr, grad, fid_sums, res_sums, residual)

    def group_passes(self, theta, Xf, Tf, fid_scale, Xr, res_scale, g_res, g_fid, fid_sums, res_sums):
        """Loss balancing's classic path: the residual's gradient ADDED to g_res and the fidelity term's to g_fid, a pass each
        (either may be None: that pass is not run and its sums are left alone) — the plain entries of whatever engine serves
        the network, with a fresh dropout seed per pass in training mode as _engine draws it."""
        if g_fid is not None:
            self._engine().mse_loss_grad(theta, Xf, Tf, self.fid_cols, fid_scale, g_fid, sums=fid_sums)
        if g_res is not None:
            self._engine().residual_loss_grad(self.spec, res_scale, theta, Xr, g_res, sums=res_sums)

    def adam_step(self, theta, grad, m, v, step, lr):
        self.eng.adam_step(theta, grad, m, v, step, lr)

    def request_points(self, Xf, Xr, force_merge: bool = False):
        """(X, n_res) of the request that runs both loss terms in ONE pass, as the engine's loop entries take them: the
        collocation points alone (n_res = their count) without fidelity points, the shared point set (n_res = -1,
        train_newmethod.py:122-159), else [collocation points ; fidelity points] (n_res = the collocation count).  None: not
        servable in one pass — merge_sets is off or the fidelity set is larger than MERGE_MAX_FID (force_merge: the
        caller has no second pass to fall back to, and merges all the same)."""
        if Xf is None or Xf.shape[0] == 0:
            return Xr, Xr.shape[0]
        if Xf is Xr:
            return Xr, -1
        if not force_merge and not (self.merge_sets and Xf.shape[0] <= self.MERGE_MAX_FID):
            return None
        return self._merged(Xr, Xf), Xr.shape[0]

    def adam_iteration(self, theta, Xf, Tf, fid_scale, Xr, res_scale, grad, fid_sums, res_sums, m, v, step, lr,
                       loss_rows=None, losses=None, params_token=None, extras=None, balance=None) -> bool:
        """loss_func + backward + Adam.step (train.py:189-193) in two launches where the engine can
        (Engine.loss_grad_adam_step); False — nothing done — otherwise: the caller then runs __call__ + adam_step.
        lr: a float, with losses (3,) — one iteration — or a list, with losses (k, 3): a device-enqueued run.
        extras (trainer.PINN(fold_extras=True)): with runtime coefficients or point weights set, the keyword arguments of
        Engine.adam_loop_ext that belong to them (moments, learning rates, coef_log / the multipliers) — the request then
        runs as a device-enqueued run of that entry; without it such requests take the classic path.
        balance (trainer.PINN(loss_balancing=..., fold_extras=True)): the keyword arguments of Engine.adam_loop_balanced that
        belong to gradient-statistics loss balancing — the two point sets as a pass each, the weights updated on the device."""
        if self._dropping() or Xr is None or Xr.shape[0] == 0:
            return False
        if self.spec.nu != 0:     # the second-order residual is layer kernels per chunk, not one pass: the classic path
            return False
        has_fid = Xf is not None and Xf.shape[0] > 0
        has_extras = self.coef is not None or self.point_w is not None
        if balance is None and not has_extras:     # the plain request (first: the path every small problem's iteration takes)
            request = None if not has_fid and fid_sums.numel() else self.request_points(Xf, Xr)
            if request is None:                    # (fidelity outputs but no fidelity points, or two passes: classic path)
                return False
            fid = dict(T=Tf, out_col=self.fid_cols, col_scale=fid_scale, col_sums=fid_sums) if has_fid else {}
            return self.eng.loss_grad_adam_step(self.spec, res_scale, theta, *request, grad, m, v, step, lr, term_sums=res_sums,
                                                loss_rows=loss_rows, losses=losses, params_token=params_token, **fid)
        # the other loop entries take runs only: one iteration is a run of one
        single = not isinstance(lr, (list, tuple))
        lrs = [lr] if single else lr
        out = dict(term_sums=res_sums, col_sums=fid_sums, loss_rows=loss_rows, params_token=params_token,
                   losses=losses.reshape(1, -1) if single and losses is not None else losses)
        if balance is not None:
            if has_extras or not has_fid:
                return False
            return self.eng.adam_loop_balanced(self.spec, res_scale, theta, Xr, grad, m, v, step, lrs, Xf, Tf, self.fid_cols,
                                               fid_scale, **out, **balance)
        # coefficients or point weights: the folded iteration above runs the entries that carry the constants and no weights,
        # so these requests have a loop entry of their own, taken only when the trainer asks for it
        if extras is None:
            return False
        own = dict(coef=self.coef, coef_grad=self.coef_grad) if self.coef is not None else \
            dict(point_w=self.point_w, fields=self.fields_out)
        return self.eng.adam_loop_ext(self.spec, res_scale, theta, Xr, grad, m, v, step, lrs, Xf=Xf if has_fid else None,
                                      T=Tf if has_fid else None, out_col=self.fid_cols, col_scale=fid_scale,
                                      **out, **extras, **own)

    def _merged(self, Xr, Xf):
        """[collocation points ; fidelity points] in one matrix, refreshed whenever either source is a different
        tensor OBJECT than the one it was filled from (held here, so its storage cannot be recycled under us): a
        resampled mini-batch is a new tensor every call and is copied in every call.  data_ptr() is no identity —
        the caching allocator hands a freed block to the next same-sized tensor."""
        nr, nf = Xr.shape[0], Xf.shape[0]
        if self._cat is None or self._cat.shape[0] != nr + nf:
            self._cat = torch.empty(nr + nf, Xr.shape[1], dtype=torch.float32, device=Xr.device)
            self._cat_src = (None, None)
        if self._cat_src[0] is not Xr:
            self._cat[:nr].copy_(Xr)
        if self._cat_src[1] is not Xf:
            self._cat[nr:].copy_(Xf)
        self._cat_src = (Xr, Xf)
        return self._cat

    def predict(self, theta, X):
        return self.eng.forward(theta, X)

    def residual_fields(self, theta, X):
        """(n_fields, N) signed residual fields at the rows of X, in eval mode: the engine without dropout, as predict."""
        if self.coef is not None:
            raise PinnError("residual_fields does not run with runtime closure coefficients: the field kernels carry the constants")
        if self.spec.nu != 0:     # the shifted fields, from the entry the loss runs on (no backward sweep)
            return self.eng.residual2_loss_grad(self.spec, None, theta, X, grad=None, fields=True)[1]
        return self.eng.residual_fields(self.spec, theta, X)


@dataclass(frozen=True)
class Options:
    """What PINN.__init__ makes of its arguments and the configuration, resolved ONCE (an argument wins over its config key):
    every refusal and every later use reads this record."""
    residual: str
    corrected: bool
    wave_period: Optional[float]     # seconds; None: no wave closure
    wave_gamma: float
    nu: float                        # eddy_viscosity
    coef_in: dict                    # coefficient values given, by name
    coef_tr: tuple                   # names of the trainable coefficients
    fixed_weights: bool              # residual_weights were given
    sa_opt: Optional[dict]           # self_adaptive's options (None: off)
    rad_imp: bool
    fold_adam: bool
    fold_extras: bool
    balancing: Optional[str]
    balance_every: int
    balance_alpha: float
    balance_ref: str
    balance_groups: str
    residual_batch: Optional[int]
    resample: str
    lbfgs_impl: str
    custom_evaluator: bool
    reducer_active: bool

    @property
    def wave(self) -> bool:
        return self.wave_period is not None

    @property
    def has_coef(self) -> bool:
        return bool(self.coef_in or self.coef_tr)

    @property
    def weighted(self) -> bool:
        """Fixed or self-adaptive weights on the collocation points (rad_imp: the mini-batch's importance weights beside them)."""
        return self.fixed_weights or self.sa_opt is not None


ADAM, LBFGS = "adam", "lbfgs"      # PINN._stage: which stage the next loss evaluation belongs to


class PINN:
    """The physics-guided network harness (reference `class pinn`, train.py:46)."""

    def __init__(self, fidelity_input, fidelity_true, residual_input, config, residual: Optional[str] = None,
                 device="cuda", log_dir: Optional[str] = None, log_every: int = 1, checkpoint_every: int = 1000,
                 reducer: Optional[Reducer] = None, evaluator: Optional[Callable] = None,
                 dnn: Optional[DNN] = None, engine: int = 0, mat_dump_iter: Optional[int] = None,
                 mat_dump_path: str = "data_at50k.mat", residual_batch: Optional[int] = None, seed: int = 1234,
                 log_flush_every: int = 100, lbfgs_impl: str = "flat", precision: int = 0, fold_adam: bool = True,
                 resample: str = "uniform", rad_every: int = 100, rad_k: float = 1.0, rad_c: float = 1.0,
                 corrected: bool = False, eddy_viscosity: float = 0.0, coefficients: Optional[dict] = None,
                 trainable_coefficients: Sequence[str] = (), residual_weights=None, self_adaptive=None,
                 rad_importance: Optional[bool] = None, fold_extras: bool = False, loss_balancing: Optional[str] = None,
                 balance_every: Optional[int] = None, balance_alpha: Optional[float] = None, balance_ref: Optional[str] = None,
                 balance_groups: Optional[str] = None, wave_period: Optional[float] = None, wave_gamma: Optional[float] = None):
        """loss_balancing (or the config key loss.balancing): "max_mean" (Wang, Teng & Perdikaris 2021) or "norm" (Wang et al.
        2023) — the weights of the loss groups are set from the groups' own gradients during the Adam stage
        (include/pinn_hip.h: pinn_balance_update): on every balance_every-th iteration, from the first, the statistics of the
        per-group gradients move the weights by a moving average of rate balance_alpha; every iteration steps along
        sum_j lam_j g_j.  balance_groups "sets": residual and fidelity (balance_ref, the max/mean rule's reference group:
        "residual" or "fidelity"); "terms": a group per weighted residual term (ResidualSpec.n_weighted_terms; "residual"
        then names the first term) and fidelity — on update iterations the residual runs once per term with a one-hot scale.
        The weights multiply the hand-set ones (weight_fid / weight_res and the per-output weights stay in the scales); the
        logged losses stay weighted by the hand-set ones alone, loss_weights() and the log's extra columns give the rest.
        The classic path — two loss calls into two rows of a (G, P) buffer, Engine.balance_update, pinn_adam_step, no host
        synchronisation — runs on every engine and with residual_batch and resample="rad"; with fold_extras and "sets" the
        iterations run as device-enqueued runs (Engine.adam_loop_balanced) where that entry serves the network
        (self.balance_why says why not).  The L-BFGS stage holds the weights frozen at their Adam-final values: they are
        folded into the scales once when it starts.  What is refused: balance_refusal decides.
        fold_extras (or the config key adam_optimizer.fold_extras; off unless asked for): Adam iterations with runtime
        coefficients, fixed residual_weights or self_adaptive weights run as device-enqueued runs (Engine.adam_loop_ext: three
        launches per iteration, no Python in between; the coefficients, the multipliers and their Adam moments are updated on
        the device) instead of the classic path.  Checkpoint iterations and mat_dump_iter keep the classic path, and so does
        whatever fold_extras_refusal names (self.fold_extras_why holds its answer); the L-BFGS stage is unchanged.
        residual_weights: fixed weights on the collocation points' squared residuals, (N_res,) or (n_w, N_res) with
        n_w = ResidualSpec.n_weighted_terms — a mask, a confidence map; set_residual_weights changes them later.  The
        normaliser stays the point count (res_scale = weight / N), not the sum of the weights.
        self_adaptive (or the config key loss.self_adaptive): True, or {"init": 1.0, "mask": "square" | "linear", "per_term":
        True} — one trainable multiplier lambda per collocation point (and weighted term), w = lambda^2 or lambda, raised by one
        Adam ASCENT step after every Adam pass (McClenny & Braga-Neto) with Adam moments of its own, the network's step count
        and StepLR factor and the rate adam_optimizer.weight_learning_rate (default the network's); the L-BFGS stage holds the
        weights frozen.  rad_importance (or loss.rad_importance) with resample="rad": the mini-batch gets the importance weights
        mean(score) / score[idx], which makes its loss an unbiased estimate of the pool mean.  With any of the three the residual
        runs on Engine.residual_weighted_loss_grad, the fidelity term as a separate call, and Adam iterations take the classic
        path.  What is refused: weighted_refusal decides.
        coefficients (or the config key loss.coefficients), e.g. {"Cd": 0.01}: values of the residual's closure coefficients
        (ResidualSpec.coef_names: gamma_b of Navier_Stokes, Cd of physics_equation) in place of the compiled-in constants.
        trainable_coefficients (or loss.trainable_coefficients), e.g. ("Cd",): those are unknowns learned with the network —
        a small device tensor with Adam state of its own, updated with the same step count and schedule (learning rate:
        adam_optimizer.coefficient_learning_rate, default the network's).  With either set the residual runs on
        Engine.residual_coef_loss_grad, the fidelity term as a separate call, Adam iterations take the classic path, and the
        L-BFGS stage holds the coefficients frozen at their Adam-final values.  What is refused: coefficient_refusal decides
        (and device_lbfgs_refusal for lbfgs_impl="device", weighted_refusal and balance_refusal for their options).
        corrected (or the config key loss.corrected_radiation_stress; physics_equation only): train on the corrected
        radiation stress, E = rho g Hrms^2 / 8, hard-wired in the kernels (ResidualSpec.corrected) — every path that takes
        the spec follows: the merged launch, the folded Adam runs, residual_fields and resample="rad".
        wave_period (or the config key loss.wave_period, seconds; with corrected only) and wave_gamma (loss.wave_gamma, default
        0.42): the wave closure — the dispersion relation and the wave-energy balance as a fourth and a fifth residual term at
        omega = 2 pi / wave_period (ResidualSpec.wave_omega, physics.physics_equation_wave), weight 1 each like the other
        terms.  Every path that takes the spec follows: the merged launch, the folded Adam runs, residual_fields,
        resample="rad", lbfgs_impl="device".  What is refused: wave_refusal decides, and the coefficient, weighted and
        balancing refusals name it.
        eddy_viscosity (or the config key loss.eddy_viscosity; Navier_Stokes and physics_equation): nu of the lateral-mixing
        term -nu lap(U) in the momentum equations (ResidualSpec.nu), in the units of the network's inputs — normalised to
        [-1, 1] in the reference's pipeline.  The residual then runs on Engine.residual2_loss_grad, the fidelity term
        as a separate call; Adam iterations take the classic path; residual_fields and resample="rad" see the shifted fields.
        lbfgs_impl "device": what is refused, device_lbfgs_refusal decides."""
        cfg = config if isinstance(config, PinnConfig) else load_config(config)
        self.config, self.device = cfg, torch.device(device)
        self.reducer = reducer or Reducer()
        if lbfgs_impl not in ("flat", "torch", "device"):
            raise PinnError(f"lbfgs_impl={lbfgs_impl!r}: use 'flat', 'torch' or 'device'")
        loss_cfg = cfg.raw.get("loss", {})

        def given(arg, from_cfg):
            return from_cfg if arg is None else arg
        o = self.options = Options(
            residual=residual or cfg.default_residual(),
            corrected=bool(corrected) or bool(loss_cfg.get("corrected_radiation_stress", False)),
            wave_period=given(wave_period, loss_cfg.get("wave_period")),
            wave_gamma=float(given(wave_gamma, loss_cfg.get("wave_gamma", 0.42))),
            nu=float(eddy_viscosity) if eddy_viscosity else float(loss_cfg.get("eddy_viscosity", 0.0)),
            coef_in=dict(coefficients) if coefficients else dict(loss_cfg.get("coefficients") or {}),
            coef_tr=tuple(trainable_coefficients) if trainable_coefficients else tuple(loss_cfg.get("trainable_coefficients") or ()),
            fixed_weights=residual_weights is not None,
            sa_opt=cfg.self_adaptive if self_adaptive is None else None if self_adaptive is False else self_adaptive_options(self_adaptive),
            rad_imp=bool(given(rad_importance, cfg.rad_importance)), fold_adam=bool(fold_adam),
            fold_extras=bool(fold_extras) or cfg.fold_extras,
            balancing=cfg.loss_balancing if loss_balancing is None else (None if loss_balancing == "none" else loss_balancing),
            balance_every=given(balance_every, cfg.balance_every), balance_alpha=given(balance_alpha, cfg.balance_alpha),
            balance_ref=given(balance_ref, cfg.balance_ref), balance_groups=given(balance_groups, cfg.balance_groups),
            residual_batch=residual_batch, resample=resample, lbfgs_impl=lbfgs_impl, custom_evaluator=evaluator is not None,
            reducer_active=self.reducer.active)

        def refuse(why):
            if why:
                raise PinnError(why)
        # every refusal is pure host logic on the record, decided before anything touches a device
        refuse(wave_refusal(o.wave_period, o.wave_gamma, o.residual, o.corrected, o.nu))
        refuse(coefficient_refusal(o.residual, o.coef_in, o.coef_tr, o.corrected, o.nu, o.reducer_active, o.resample,
                                   o.custom_evaluator, o.wave))
        refuse(weighted_refusal(o.fixed_weights, o.sa_opt is not None, o.rad_imp, o.reducer_active, o.nu, o.has_coef, o.corrected,
                                o.lbfgs_impl, o.custom_evaluator, o.residual_batch, o.resample, o.wave))
        refuse(balance_refusal(o.balancing, o.balance_groups, o.balance_every, o.balance_alpha, o.balance_ref, o.fold_extras,
                               o.has_coef, o.weighted, o.rad_imp, o.nu, o.reducer_active, o.custom_evaluator, o.wave))
        if o.balancing is not None and (fidelity_input is None or residual_input is None or
                                        len(fidelity_input) == 0 or len(residual_input) == 0):
            raise PinnError("loss balancing weighs the fidelity set against the collocation set: it needs points in both")
        if o.lbfgs_impl == "device":
            refuse(device_lbfgs_refusal(o.reducer_active, o.residual_batch, o.nu, o.custom_evaluator, cfg.lbfgs["line_search_fn"],
                                        cfg.dropout_rate, o.has_coef))
        self.loss_balancing, self.balance_every, self.balance_alpha = o.balancing, o.balance_every, o.balance_alpha
        self.balance_ref, self.balance_groups = o.balance_ref, o.balance_groups
        self.fold_adam, self._adam_folded, self._folded_iters, self._run_losses = o.fold_adam, False, 0, None
        self.fold_extras = o.fold_extras
        self.fold_extras_why = fold_extras_refusal(o.fold_extras, o.has_coef, o.weighted, o.rad_imp, o.residual_batch, o.resample,
                                                   cfg.dropout_rate, o.reducer_active, o.nu, o.custom_evaluator, o.fold_adam)
        # (balanced iterations: where fold_extras is on, why they keep the classic path all the same — None: they run as
        # device-enqueued runs wherever the engine serves the request)
        self.balance_why = None
        if o.balancing is not None:
            self.balance_why = ("fold_extras is off" if not o.fold_extras else
                                balance_fold_refusal(o.residual_batch, o.resample, cfg.dropout_rate, o.fold_adam))
        self._fold_refused = None   # key of the (evaluator, point sets) whose folded request the engine has refused
        self.layers = cfg.layers                                           # train.py:52-56
        self.dnn = dnn if dnn is not None else DNN(cfg.layers, cfg.dropout_rate, cfg.init_type,
                                                   first_activation=cfg.first_activation, fourier_sigma=cfg.fourier_sigma)
        self.dnn.to(self.device)
        self.theta = self.dnn.flat_params()
        self.reducer.broadcast_(self.theta)                                # replicas start identical
        P = self.theta.numel()

        self.corrected, self.eddy_viscosity = o.corrected, o.nu
        self.wave_period, self.wave_gamma = o.wave_period, o.wave_gamma
        self.spec = ResidualSpec.from_names(o.residual, cfg.residual_inputs, cfg.grad_cols, cfg.residual_outputs,
                                            corrected=o.corrected, nu=o.nu, wave_gamma=o.wave_gamma,
                                            wave_omega=2.0 * math.pi / float(o.wave_period) if o.wave else 0.0)   # (PinnError on any other residual)
        # i-th fidelity output is compared with output column i (train.py:137-138, train_newmethod.py:129-131)
        self.fid_cols = list(range(len(cfg.fidelity_outputs)))
        self.weight_fidelity, self.weight_residual = cfg.weight_fid, cfg.weight_res

        Xf, Tf, Xr = (_as_f32(a, self.device) for a in (fidelity_input, fidelity_true, residual_input))
        if Xf is not None and Xr is not None and (fidelity_input is residual_input or
                                                  (cfg.variant == "newmethod" and Xf.shape == Xr.shape and torch.equal(Xf, Xr))):
            Xf = Xr            # the same point set: the evaluator fuses both loss terms into one pass
        self.n_fid = 0 if Xf is None else Xf.shape[0]
        self.n_res = 0 if Xr is None else Xr.shape[0]
        self.Xr = self.reducer.shard(Xr)
        self.Xf = self.Xr if Xf is Xr else self.reducer.shard(Xf)
        self.Tf = self.reducer.shard(Tf)
        nf, nt = len(self.fid_cols), self.spec.n_terms
        dev = self.device
        self.buf = torch.zeros(P + nf + nt, dtype=torch.float32, device=dev)   # ONE all-reduce per closure
        self.grad = self.buf[:P]
        self._fid_sums, self._res_sums = self.buf[P:P + nf], self.buf[P + nf:]
        self.evaluator = evaluator or HipEvaluator(cfg.layers, cfg.init_type, cfg.grad_cols, self.spec,
                                                   self.fid_cols, dev, engine, precision, cfg.dropout_rate,
                                                   activation=self.dnn.activation_id)
        # the coefficients: every one of the residual's, given or default, in ResidualSpec.coef_names order
        self.coef_names: Tuple[str, ...] = self.spec.coef_names if o.has_coef else ()
        self.trainable_coefficients = tuple(n for n in self.coef_names if n in o.coef_tr)
        self._coef = self._coef_grad = self._coef_m = self._coef_v = self._coef_mask = None
        self._coef_history: List[tuple] = []
        if self.coef_names:
            vals = [float(o.coef_in.get(n, d)) for n, d in zip(self.coef_names, self.spec.coef_defaults)]
            self._coef = torch.tensor(vals, dtype=torch.float32, device=dev)
            self.evaluator.coef = self._coef
            if self.trainable_coefficients:
                self._coef_grad = torch.zeros_like(self._coef)
                self._coef_mask = torch.tensor([1.0 if n in o.coef_tr else 0.0 for n in self.coef_names], dtype=torch.float32, device=dev)

        # point weights on the residual: fixed (_w_fixed), self-adaptive (_lam -> _w_fixed = m(lambda) every pass) and / or the
        # RAD mini-batch's importance weights (formed per draw)
        self.self_adaptive, self.rad_importance = o.sa_opt, o.rad_imp
        self._w_fixed = self._lam = self._lam_m = self._lam_v = self._sa_fields = None
        self._last_idx = None
        if residual_weights is not None:
            self.set_residual_weights(residual_weights)
        if o.sa_opt is not None:
            rows = self.spec.n_weighted_terms if o.sa_opt["per_term"] else 1
            self._lam = torch.full((rows, self.n_res), o.sa_opt["init"], dtype=torch.float32, device=dev)
            self._w_fixed = sa_weights(self._lam, o.sa_opt["mask"]).contiguous()
            self._sa_fields = torch.zeros(self.spec.n_fields, self.n_res, dtype=torch.float32, device=dev)
            self.evaluator.point_w = self._w_fixed

        # optional resampled collocation mini-batch (the reference is full-batch only):
        # each closure draws `residual_batch` of this rank's points with a device-side generator
        self.residual_batch = residual_batch
        self._gen = None
        if residual_batch is not None:
            if o.residual == "continuity_only":
                raise PinnError("residual_batch is not supported with continuity_only's data-dependent mean")
            self._gen = torch.Generator(device=dev).manual_seed(seed + self.reducer.rank)
        # resample = "rad": residual-based adaptive distribution (Wu et al. 2023) — the mini-batch is drawn with
        # probability proportional to eps^k / mean(eps^k) + c over this rank's pool, eps the per-point residual
        # magnitude (Engine.residual_fields), re-scored every rad_every iterations.  A biased sampler by design: no
        # importance re-weighting, _res_unit as for the uniform mini-batch; each rank scores and samples its own shard.
        if resample not in ("uniform", "rad"):
            raise PinnError(f"resample={resample!r}: use 'uniform' or 'rad'")
        if resample == "rad":
            if o.residual == "continuity_only":
                raise PinnError("resample='rad' is not supported with continuity_only's data-dependent mean")
            if residual_batch is None:
                raise PinnError("resample='rad' draws a mini-batch of the collocation pool: it needs residual_batch")
            if int(rad_every) < 1 or rad_k < 0 or rad_c < 0:
                raise PinnError(f"rad_every={rad_every} must be >= 1, rad_k={rad_k} and rad_c={rad_c} must be >= 0")
        self.resample, self.rad_every, self.rad_k, self.rad_c = resample, int(rad_every), float(rad_k), float(rad_c)
        self._rad_score, self._rad_cdf, self._rad_at = None, None, None
        # the loss arithmetic: the residual's normaliser is the global point count, or the mini-batches' size over all ranks
        anchor = None
        if o.residual == "continuity_only":
            anchor = anchor_count(cfg, self.spec, self.Xr)
            self.reducer.allreduce_sum_(anchor)                            # global count of x < 25.5
        self._fid_unit, self._res_unit, self._fid_scale, self._res_scale, self._loss_mat = loss_arithmetic(
            cfg, self.spec, nf, self.n_fid, self.n_res if residual_batch is None else residual_batch * self.reducer.world, dev, anchor)
        self._loss_vec = torch.zeros(3, dtype=torch.float32, device=dev)       # the three losses of an iteration that is not logged
        self.mat_dump_iter, self.mat_dump_path = mat_dump_iter, mat_dump_path
        self.lbfgs_impl = lbfgs_impl     # "flat": lbfgs.FlatLBFGS (batched recursion); "torch": torch.optim.LBFGS;
                                         # "device": lbfgs.DeviceLBFGS (whole runs of evaluations decided on the device)
        self.device_lbfgs = None
        self.iter = 0                                                      # train.py:73
        self.adam_maxit = cfg.adam["max_it"]
        self.log_dir, self.log_every, self.checkpoint_every = log_dir, max(int(log_every), 1), checkpoint_every
        self._log_fh = None
        self._history: List[tuple] = []
        # loss balancing: the group weights and the (G, P) buffer of the per-group gradients
        self._bal_lam = self._bal_buf = self._bal_pair = None
        self._bal_frozen = False
        self.balance_names: Tuple[str, ...] = ()
        self._weight_history: List[tuple] = []
        if o.balancing is not None:
            nw = self.spec.n_weighted_terms
            self.balance_names = ("residual", "fidelity") if o.balance_groups == "sets" else \
                tuple(f"residual_term_{t}" for t in range(nw)) + ("fidelity",)
            G = len(self.balance_names)
            self._bal_ref = 0 if o.balance_ref == "residual" else G - 1
            self._bal_lam = torch.ones(G, dtype=torch.float32, device=dev)
            self._bal_buf = torch.zeros(G, P, dtype=torch.float32, device=dev)
            if o.balance_groups == "terms":
                self._bal_pair = torch.ones(2, dtype=torch.float32, device=dev)      # [1, lam_fidelity] between updates
                self._bal_onehot = torch.eye(nt, dtype=torch.float32, device=dev)[:nw].contiguous()
                self._bal_term_scale = torch.zeros(nt, dtype=torch.float32, device=dev)
        # the log's extra columns, beside the three losses: the coefficients or the balanced groups' weights (never both:
        # balance_refusal) — their names in log.txt's header, the device tensor that holds their current values, the history
        # their logged values go to, and (allocated at the first run) the rows a device-enqueued run logs them in
        self._extra_names = self.coef_names or tuple(f"weight_{n}" for n in self.balance_names)
        self._extra_vals = self._coef if self.coef_names else self._bal_lam
        self._extra_history = self._coef_history if self.coef_names else self._weight_history
        self._run_extras = None
        self._ring = torch.zeros(max(int(log_flush_every), 1), 3 + len(self._extra_names), dtype=torch.float32, device=dev)
        self._ring_iters: List[int] = []
        self.last = None
        self._stage = ADAM          # set by adam_step / _adam_run and closure / train_lbfgs_device; a bare loss_func() keeps the last
        self.init_optimizers()
        self._bind()

    # ---- optimisers (train.py:100-125) ----------------------------------------------------------
    def init_optimizers(self):
        a, lb = self.config.adam, self.config.lbfgs
        self._adam_m = torch.zeros_like(self.theta)
        self._adam_v = torch.zeros_like(self.theta)
        if self._coef_grad is not None:      # the coefficients' own Adam state
            self._coef_m, self._coef_v = torch.zeros_like(self._coef), torch.zeros_like(self._coef)
        if self._lam is not None:            # the self-adaptive multipliers' own Adam state
            self._lam_m, self._lam_v = torch.zeros_like(self._lam), torch.zeros_like(self._lam)
        self._adam_step = 0
        self._sched_steps = 0
        self.theta_param = torch.nn.Parameter(self.theta)       # shares storage with every Linear weight
        if self.lbfgs_impl == "device":      # built by train(): it binds the point sets and the loss rows
            self.optimizer_LBFGS = None
            DeviceLBFGS.check_options(lb["learning_rate"], lb["max_it"], lb.get("max_evaluation"), lb["history_size"],
                                      lb["tolerance_grad"], lb["tolerance_change"], lb["line_search_fn"])
            return
        lbfgs_cls = FlatLBFGS if self.lbfgs_impl == "flat" else torch.optim.LBFGS
        self.optimizer_LBFGS = lbfgs_cls(
            [self.theta_param], lr=lb["learning_rate"], max_iter=lb["max_it"], max_eval=lb.get("max_evaluation"),
            history_size=lb["history_size"], tolerance_grad=lb["tolerance_grad"],
            tolerance_change=lb["tolerance_change"], line_search_fn=lb["line_search_fn"])

    def current_lr(self) -> float:
        """StepLR(step_size, gamma) stepped once per Adam iteration (train.py:109-113,193)."""
        a = self.config.adam
        return a["learning_rate"] * steplr_factors(a, self._sched_steps)[0]

    def current_coefficient_lr(self) -> float:
        """The coefficients' learning rate: adam_optimizer.coefficient_learning_rate (default: the network's) on the same StepLR."""
        a = self.config.adam
        return float(a.get("coefficient_learning_rate", a["learning_rate"])) * steplr_factors(a, self._sched_steps)[0]

    def current_weight_lr(self) -> float:
        """The self-adaptive weights' learning rate: adam_optimizer.weight_learning_rate (default: the network's) on the same StepLR."""
        a = self.config.adam
        return self.config.weight_learning_rate * steplr_factors(a, self._sched_steps)[0]

    def set_residual_weights(self, weights):
        """Fixed weights on the collocation points: (N_res,) or (n_w, N_res) (None: back to the unweighted loss).  Not with
        self_adaptive, whose weights are m(lambda)."""
        if self._lam is not None:
            raise PinnError("set_residual_weights: the weights are the self-adaptive ones, m(lambda)")
        w = None
        if weights is not None:
            w = _as_f32(weights, self.device)
            w = w.reshape(1, -1) if w.dim() == 1 else w
            if w.dim() != 2 or w.shape[1] != self.n_res or w.shape[0] not in (1, self.spec.n_weighted_terms):
                raise PinnError(f"residual_weights must be ({self.n_res},) or ({self.spec.n_weighted_terms}, {self.n_res}), got {tuple(w.shape)}")
            w = w.contiguous()
        self._w_fixed = self.evaluator.point_w = w

    def residual_weights(self) -> Optional[torch.Tensor]:
        """The weights on the collocation points in use, (w_rows, N_res): the fixed ones, or m(lambda) of the self-adaptive
        multipliers; None for the unweighted loss."""
        if self._lam is not None:
            return sa_weights(self._lam, self.self_adaptive["mask"])
        return None if self._w_fixed is None else self._w_fixed.clone()

    def coefficients(self) -> Dict[str, float]:
        """The closure coefficients in use, by name (one synchronisation); {} when the compiled-in constants are."""
        if self._coef is None:
            return {}
        return dict(zip(self.coef_names, (float(x) for x in self._coef.cpu().tolist())))

    # ---- loss (train.py:128-181) ----------------------------------------------------------------------
    def _bind(self, idx: Optional[torch.Tensor] = None):
        """Tell the evaluator what the next pass carries — after construction and set_residual_weights the ONE place that
        writes evaluator.coef_grad, point_w and fields_out.  By the stage (self._stage): the Adam stage asks for the
        coefficients' gradient and the self-adaptive pass's fields, the L-BFGS stage holds coefficients and multipliers frozen
        at their Adam-final values and asks for neither.  idx: the mini-batch's indices into the collocation pool, where
        there is one — its weights are the importance weights x the fixed ones at those points."""
        ev = self.evaluator
        if hasattr(ev, "training"):
            ev.training = self.dnn.training          # dropout follows the module's mode (train.py:186)
        if self._coef is not None:
            ev.coef_grad = self._coef_grad if self._stage == ADAM else None      # (None too when nothing is trainable)
        if self._lam is not None:
            ev.fields_out = self._sa_fields if self._stage == ADAM else None
        if idx is not None and (self.rad_importance or self._w_fixed is not None):
            w = rad_importance_weights(self._rad_score, idx) if self.rad_importance else None
            if self._w_fixed is not None:
                wf = self._w_fixed.index_select(1, idx)
                w = wf if w is None else wf * w
            ev.point_w = w.contiguous()

    def _draw_batch(self) -> torch.Tensor:
        """The next mini-batch's indices into this rank's collocation pool: uniform, or by the RAD score (re-scored every
        rad_every iterations)."""
        if self.resample == "rad":
            if self._rad_score is None or self.iter - self._rad_at >= self.rad_every:
                self._rad_score = rad_score(self.evaluator.residual_fields(self.theta, self.Xr), self.rad_k, self.rad_c)
                self._rad_cdf = rad_cdf(self._rad_score)
                self._rad_at = self.iter
            u = torch.rand(self.residual_batch, device=self.device, generator=self._gen, dtype=torch.float64)
            self._last_idx = rad_indices(self._rad_score, u, self._rad_cdf)
        else:
            self._last_idx = torch.randint(0, self.Xr.shape[0], (self.residual_batch,), device=self.device, generator=self._gen)
        return self._last_idx

    def loss_func(self, _fold: bool = False) -> torch.Tensor:
        """Total loss (0-dim device tensor); self.grad holds d loss / d theta afterwards.  `_fold` (adam_step only): the
        evaluator may fold the Adam update into the pass's last kernel (`self._adam_folded` says whether it did)."""
        self.theta = self.dnn.flat_params()
        if self.mat_dump_iter is not None and self.iter == self.mat_dump_iter:
            self.dump_predictions(self.mat_dump_path)                      # train_newmethod.py:141-153
        Xr, idx = self.Xr, None
        if self.residual_batch is not None:
            idx = self._draw_batch()
            Xr = self.Xr.index_select(0, idx)
        elif self._lam is not None:      # w = m(lambda) of this pass (a device-enqueued run rewrites it itself: Engine.adam_loop_ext)
            self._w_fixed.copy_(sa_weights(self._lam, self.self_adaptive["mask"]))
        self._bind(idx)
        logged = self._logged(self.iter + 1)
        # loss balancing is the Adam stage's: the L-BFGS stage (closure) has folded the weights into the scales
        balancing = self.loss_balancing is not None and not self._bal_frozen
        # the three losses of a logged iteration are computed straight into the device-side ring
        row = self._ring[len(self._ring_iters)] if logged else None
        vec = row[:3] if logged else self._loss_vec
        if logged and self._extra_vals is not None and not balancing:
            row[3:].copy_(self._extra_vals)      # the values this evaluation RUNS with: a folded iteration moves the coefficients
        self._adam_folded = _fold and self._folded_request(Xr, vec)
        if not self._adam_folded:
            self.buf.zero_()
            if balancing:
                self._balanced_pass(Xr)
            else:
                self.evaluator(self.theta, self.Xf, self.Tf, self._fid_scale, Xr, self._res_scale, self.grad,
                               self._fid_sums, self._res_sums)
            self.reducer.allreduce_sum_(self.buf)
            torch.mv(self._loss_mat, self.buf[self.theta.numel():], out=vec)                  # one small mat-vec: the three losses
        self.iter += 1                                                                        # train.py:160
        self.last = (vec[0], vec[1], vec[2])
        if logged:      # (balancing: the weights this iteration stepped with — they are updated before they are used)
            self._to_ring(self.iter, None, (self._run_extras[0] if self._adam_folded else self._bal_lam) if balancing else None)
        if self._checkpoint_due(self.iter):
            self.save_checkpoint(f"model_{self.iter}.pth")                                    # train.py:175-179
        return self.last[2]

    def _balanced_pass(self, Xr):
        """One balanced evaluation on the classic path: the groups' gradients into the rows of the (G, P) buffer,
        Engine.balance_update — statistics and the rule on update iterations ((step - 1) % balance_every == 0), the
        combination sum_j lam_j g_j into self.grad on every one — and the sums of both terms.  No host synchronisation."""
        update = self._adam_step % self.balance_every == 0          # (this iteration is Adam step _adam_step + 1)
        ev, eng, buf, G = self.evaluator, self.evaluator.eng, self._bal_buf, self._bal_lam.numel()
        if self.balance_groups == "sets":
            buf.zero_()
            ev.group_passes(self.theta, self.Xf, self.Tf, self._fid_scale, Xr, self._res_scale, buf[0], buf[1],
                            self._fid_sums, self._res_sums)
            eng.balance_update(buf, self._bal_lam, self.loss_balancing if update else None, ref=self._bal_ref,
                               alpha=self.balance_alpha, out=self.grad)
            return
        nw = G - 1
        if update:       # the residual once per weighted term, its scale one-hot: row t = term t's gradient
            buf.zero_()
            for t in range(nw):
                torch.mul(self._res_scale, self._bal_onehot[t], out=self._bal_term_scale)
                ev.group_passes(self.theta, self.Xf, self.Tf, self._fid_scale, Xr, self._bal_term_scale, buf[t],
                                buf[nw] if t == 0 else None, self._fid_sums, self._res_sums)
            eng.balance_update(buf, self._bal_lam, self.loss_balancing, ref=self._bal_ref, alpha=self.balance_alpha, out=self.grad)
            return
        # between updates: ONE residual call with the scales lam_t * base, the fidelity term beside it, combined as [1, lam_fid]
        pair = buf[:2]
        pair.zero_()
        self._bal_term_scale.copy_(self._res_scale)
        self._bal_term_scale[:nw].mul_(self._bal_lam[:nw])
        self._bal_pair[1:].copy_(self._bal_lam[nw:])
        ev.group_passes(self.theta, self.Xf, self.Tf, self._fid_scale, Xr, self._bal_term_scale, pair[0], pair[1],
                        self._fid_sums, self._res_sums)
        eng.balance_update(pair, self._bal_pair, None, out=self.grad)

    def loss_weights(self) -> Dict[str, float]:
        """The balanced groups' weights by name (one synchronisation): "residual" and "fidelity", or "residual_term_<t>" and
        "fidelity"; {} without loss_balancing.  They multiply the hand-set weights."""
        if self._bal_lam is None:
            return {}
        return dict(zip(self.balance_names, (float(x) for x in self._bal_lam.cpu().tolist())))

    @property
    def weight_history(self) -> List[tuple]:
        """(iteration, weight of every group in balance_names order) of every logged iteration so far: the weights the
        iteration stepped with."""
        self.flush_log()
        return self._weight_history

    def freeze_loss_weights(self):
        """The L-BFGS stage holds the balanced weights at their Adam-final values: they are folded into the scales (and into
        the total's row of the loss matrix) once, on the device; from then on every evaluation is the plain weighted loss."""
        if self.loss_balancing is None or self._bal_frozen:
            return
        nw, nf = self._bal_lam.numel() - 1, self._fid_sums.numel()
        self._fid_scale = (self._fid_scale * self._bal_lam[nw]).contiguous()
        res = self._res_scale.clone()
        if self.balance_groups == "sets":
            res.mul_(self._bal_lam[0])
        else:
            res[:nw].mul_(self._bal_lam[:nw])
        self._res_scale = res.contiguous()
        self._loss_mat[2, :nf] = self._fid_scale          # (train.py:157: the total is [fid scale | res scale] . sums)
        self._loss_mat[2, nf:] = self._res_scale
        self._bal_frozen = True

    def _checkpoint_due(self, it: int) -> bool:
        if not self.checkpoint_every:
            return False
        every = self.checkpoint_every
        if self.config.variant == "newmethod" and self.checkpoint_every == 1000:
            every = 10000 if it <= 45000 else 1000                                            # train_newmethod.py:181-188
        return it % every == 0

    # ---- the log ring ---------------------------------------------------------------------------------
    def _logged(self, it: int) -> bool:
        """Iteration `it` (1-based) goes to the log."""
        return it % self.log_every == 0 or it % 1000 == 0

    def _to_ring(self, first: int, losses: Optional[torch.Tensor], extras: Optional[torch.Tensor]):
        """The logged ones among iterations first .. first + k - 1 into the log ring, flushed whenever it is full.
        losses: their (k, 3) loss rows; None: ONE logged iteration whose losses loss_func has computed into the next free row itself.
        extras, the columns beside the losses: (k, E), a row per iteration (what a device-enqueued run logged); (E,), the
        current values, the same for every row; None: there are none, or they are in the row already."""
        iters, size = self._ring_iters, self._ring.shape[0]
        if losses is None:       # (every logged loss_func call comes through here: kept short)
            if extras is not None:
                self._ring[len(iters), 3:].copy_(extras)
            iters.append(first)
            if len(iters) == size:
                self.flush_log()
            return
        picks = [i for i in range(losses.shape[0]) if self._logged(first + i)]
        while picks:
            r0 = len(self._ring_iters)
            now, picks = picks[:size - r0], picks[size - r0:]
            one_copy = now[-1] - now[0] + 1 == len(now)
            for cols, src in ((slice(0, 3), losses), (slice(3, None), extras)):
                if src is None:
                    continue
                dst = self._ring[r0:r0 + len(now), cols]
                if src.dim() == 1 or one_copy:       # the same values for every row / consecutive iterations: one copy
                    dst.copy_(src if src.dim() == 1 else src[now[0]:now[-1] + 1])
                else:
                    for j, i in enumerate(now):
                        dst[j].copy_(src[i])
            self._ring_iters.extend(first + i for i in now)
            if len(self._ring_iters) == size:
                self.flush_log()

    @property
    def history(self) -> List[tuple]:
        """(iteration, fidelity, residual, total) of every logged iteration so far."""
        self.flush_log()
        return self._history

    @history.setter
    def history(self, value):
        self._ring_iters = []
        self._history = list(value)

    def flush_log(self):
        """Bring the pending ring entries to the host (ONE synchronisation) and write them out."""
        if not self._ring_iters:
            return
        rows = self._ring[:len(self._ring_iters)].cpu().tolist()
        iters, self._ring_iters = self._ring_iters, []
        for it, row in zip(iters, rows):
            self._log(it, row[0], row[1], row[2], row[3:])
        if self._log_fh is not None:
            self._log_fh.flush()

    def _log(self, it: int, fid: float, res: float, tot: float, extras: Sequence[float] = ()):
        self._history.append((it, fid, res, tot))
        if extras:
            self._extra_history.append((it,) + tuple(extras))
        tail = "".join(f", {c:.6e}" for c in extras)      # the extra columns' values, appended to the log line
        if it % 1000 == 0 and self.reducer.rank == 0:
            print(f"Epoch {it}, Fidelity Loss: {fid:.5e}, Residual Loss: {res:.5e}, Total Loss: {tot:.5e}")
        if self.log_dir is None or self.reducer.rank != 0:
            return
        if self._log_fh is None:
            os.makedirs(self.log_dir, exist_ok=True)
            path = os.path.join(self.log_dir, "log.txt")
            new = not os.path.exists(path) or os.stat(path).st_size == 0
            self._log_fh = open(path, "a")
            if new:
                self._log_fh.write("Epoch, Fidelity Loss, Residual Loss, Total Loss" +
                                   "".join(f", {n}" for n in self._extra_names) + "\n")           # train.py:167
        self._log_fh.write(f"{it}, {fid:.5e}, {res:.5e}, {tot:.5e}{tail}\n")                  # train.py:170

    def dump_predictions(self, path: str):
        """savemat of pred_<key> (N,1) float32 for every network output on ALL residual points — the
        file format of the reference's data_at50k.mat (train_newmethod.py:141-153).  Under data
        parallelism every rank predicts its shard, the shards are gathered in rank order (= the
        original row order, parallel.shard_bounds) and rank 0 alone writes the file."""
        Y = self.reducer.gather_rows(self.predict(self.Xr).detach(), self.n_res)
        if self.reducer.rank != 0:
            return
        from scipy.io import savemat
        Y = Y.cpu().numpy().astype(np.float32)
        names = self.config.residual_outputs
        out = {f"pred_{k}": Y[:, i:i + 1] for i, k in enumerate(names)}
        if self._coef is not None:
            out["coefficients"] = self._coef.cpu().numpy().astype(np.float32).reshape(1, -1)      # in coef_names order
        if self.residual_weights() is not None:
            out["residual_weights"] = self.residual_weights().cpu().numpy().astype(np.float32)    # (w_rows, N_res)
        savemat(path, out)
        print(f"Data saved to {path} after {self.iter} iterations.")

    def save_checkpoint(self, name: str):
        self.flush_log()
        if self.log_dir is None or self.reducer.rank != 0:
            return
        os.makedirs(self.log_dir, exist_ok=True)
        torch.save(self.dnn, os.path.join(self.log_dir, name))                    # whole module, as train.py:179
        torch.save(self.dnn.state_dict(), os.path.join(self.log_dir, name.replace(".pth", ".state.pth")))
        if self._coef is not None:
            with open(os.path.join(self.log_dir, "coefficients.json"), "w") as fh:
                json.dump({"iteration": self.iter, "coefficients": self.coefficients(),
                           "trainable": list(self.trainable_coefficients)}, fh)
        if self.residual_weights() is not None:
            np.save(os.path.join(self.log_dir, "residual_weights.npy"), self.residual_weights().cpu().numpy().astype(np.float32))

    # ---- training (train.py:185-200) ------------------------------------------------------------------
    def adam_step(self):
        """zero_grad / loss_func / backward / Adam.step / StepLR.step (train.py:189-193)."""
        # One process, no checkpoint inside this iteration (the reference saves the PRE-update weights from inside
        # loss_func, train.py:175-179): the evaluator may fold the update into the pass's last kernel.
        fold = (self._may_fold() and not self._checkpoint_due(self.iter + 1))
        if fold and self._has_extras() and self.mat_dump_iter is not None and self.iter == self.mat_dump_iter:
            # the prediction dump's iteration takes the classic path.  The plain request folds it (the dump is written at the
            # start of loss_func either way); with extras the .mat also carries the coefficients / residual_weights, and the
            # iteration that hands them over is kept the one that has always written that file.  _foldable_run cuts runs here.
            fold = False
        self._stage = ADAM
        if self._bal_frozen:
            raise PinnError("loss balancing: the weights were frozen for the L-BFGS stage; Adam iterations after it are not balanced")
        loss = self.loss_func(fold)
        self._adam_step += 1
        if fold and not self._adam_folded:
            self._fold_refused = self._fold_key()      # remembered: no second refused C call per iteration from now on
        if not self._adam_folded:
            self.evaluator.adam_step(self.theta, self.grad, self._adam_m, self._adam_v, self._adam_step,
                                     self.current_lr())
            if self._coef_grad is not None:      # the coefficients: the same step count and schedule, their own state
                if len(self.trainable_coefficients) < len(self.coef_names):
                    self._coef_grad.mul_(self._coef_mask)
                self.evaluator.eng.adam_step(self._coef, self._coef_grad, self._coef_m, self._coef_v, self._adam_step,
                                             self.current_coefficient_lr(), count=self._coef.numel())
            if self._lam is not None:            # the multipliers' ascent step from this pass's fields: same step count and schedule
                g = sa_weight_grad(self._lam, self._sa_fields, self._res_scale, self.self_adaptive["mask"]).contiguous()
                self.evaluator.eng.adam_step(self._lam.view(-1), g.view(-1), self._lam_m.view(-1), self._lam_v.view(-1),
                                             self._adam_step, self.current_weight_lr(), count=self._lam.numel())
        else:
            self._folded_iters += 1
        self._sched_steps += 1
        return loss

    MAX_RUN = 256      # iterations enqueued by one call (pinn_adam_loop)

    def _fold_key(self):
        return (id(self.evaluator), id(self.Xr), id(self.Xf), self.residual_batch, self.dnn.training)   # (dropout folds in eval mode only)

    def _may_fold(self) -> bool:
        """The folded iteration is worth asking for: switched on, one process, an evaluator that has it, and the engine
        has not already refused this very request (wide / generic engine, a large split request: the refusal is remembered
        per evaluator and point sets instead of being re-discovered by two refused C calls every iteration)."""
        if self._has_extras() and not (self.fold_extras and self.fold_extras_why is None and self.residual_batch is None):
            return False      # coefficients / point weights: the classic path unless fold_extras is on and applies
        if self.loss_balancing is not None and not (self.balance_why is None and self.balance_groups == "sets"):
            return False      # balanced iterations: the classic path unless fold_extras is on and applies
        return (self.fold_adam and not self.reducer.active and hasattr(self.evaluator, "adam_iteration")
                and self._fold_refused != self._fold_key())

    def _has_extras(self) -> bool:
        """Runtime coefficients or point weights of any kind: the requests of Engine.adam_loop_ext."""
        return self._coef is not None or self._w_fixed is not None or self.rad_importance

    def _folded_request(self, Xr, losses: torch.Tensor) -> bool:
        """evaluator.adam_iteration for the next Adam iterations, with the keywords of the loop entry the configuration needs:
        ONE iteration whose three losses go to `losses` (3,) — from loss_func — or a device-enqueued run of k with losses
        (k, 3) — from _adam_run.  Learning rates on the StepLR schedule (current_lr / current_coefficient_lr /
        current_weight_lr at each iteration).  The extra columns each iteration ran with go to self._run_extras[:k]; a single
        iteration's coefficients are in its ring row already (loss_func) and are not asked for.  False: not served, nothing done."""
        single = losses.dim() == 1
        k = 1 if single else losses.shape[0]
        a = self.config.adam
        sched = steplr_factors(a, self._sched_steps, k)
        lr = a["learning_rate"] * sched[0] if single else [a["learning_rate"] * f for f in sched]
        if self._extra_names and (self._run_extras is None or self._run_extras.shape[0] < k):
            self._run_extras = torch.zeros(max(k, self.MAX_RUN), len(self._extra_names), dtype=torch.float32, device=self.device)
        kw = {}
        if self.loss_balancing is not None:      # Engine.adam_loop_balanced
            kw["balance"] = {"lam": self._bal_lam, "mode": self.loss_balancing, "every": self.balance_every, "ref": self._bal_ref,
                             "alpha": self.balance_alpha, "lam_log": self._run_extras[:k]}
        elif self._coef is not None:             # Engine.adam_loop_ext: the coefficients' Adam state and learning rates
            ext = kw["extras"] = {"coef_log": None if single else self._run_extras[:k]}
            if self._coef_grad is not None:
                base = float(a.get("coefficient_learning_rate", a["learning_rate"]))
                ext.update(coef_m=self._coef_m, coef_v=self._coef_v, lr_coef=[base * f for f in sched])
                if len(self.trainable_coefficients) < len(self.coef_names):
                    ext["coef_mask"] = self._coef_mask
        elif self._lam is not None:              # ... or the multipliers'
            kw["extras"] = {"lam": self._lam, "lam_m": self._lam_m, "lam_v": self._lam_v, "sa_mask": self.self_adaptive["mask"],
                            "lr_w": [self.config.weight_learning_rate * f for f in sched]}
        elif self._w_fixed is not None or self.rad_importance:      # ... or fixed weights: nothing of their own
            kw["extras"] = {}
        return self.evaluator.adam_iteration(
            self.theta, self.Xf, self.Tf, self._fid_scale, Xr, self._res_scale, self.grad, self._fid_sums, self._res_sums,
            self._adam_m, self._adam_v, self._adam_step + 1, lr, loss_rows=self._loss_mat, losses=losses,
            params_token=self.dnn.write_token(self.theta), **kw)

    def _foldable_run(self, n: int) -> int:
        """How many of the next n Adam iterations can be enqueued by ONE call: full batch, one process, nothing the
        host must do in between (a checkpoint is saved from inside loss_func with pre-update weights, train.py:175-179;
        the prediction dump of train_newmethod.py:141-153 happens at the start of its iteration)."""
        if not (self._may_fold() and self.residual_batch is None):
            return 0
        k = min(n, self.MAX_RUN)
        for i in range(1, k + 1):
            if self._checkpoint_due(self.iter + i):
                k = i - 1
                break
        if self.mat_dump_iter is not None and self.iter <= self.mat_dump_iter < self.iter + k:
            k = self.mat_dump_iter - self.iter
        free, logged = self._ring.shape[0] - len(self._ring_iters), 0
        for i in range(1, k + 1):
            if self._logged(self.iter + i):
                logged += 1
                if logged > free:
                    k = i - 1
                    break
        return k

    def train_adam(self, n: int):
        """n Adam iterations (train.py:188-193).  Runs of iterations that need nothing from the host are enqueued by one
        call (two launches per iteration, no Python in between); the rest go through adam_step()."""
        while n > 0:
            k = self._foldable_run(n)
            if k > 1:
                if self._adam_run(k):
                    n -= k
                    continue
                self._fold_refused = self._fold_key()
            self.adam_step()
            n -= 1

    def _adam_run(self, k: int) -> bool:
        self.theta = self.dnn.flat_params()
        self._stage = ADAM
        self._bind()
        if self._run_losses is None or self._run_losses.shape[0] < k:
            self._run_losses = torch.zeros(max(k, self.MAX_RUN), 3, dtype=torch.float32, device=self.device)
        out = self._run_losses[:k]
        if not self._folded_request(self.Xr, out):
            return False
        # (the run was cut so that its logged iterations fit the ring: _foldable_run)
        self._to_ring(self.iter + 1, out, self._run_extras[:k] if self._extra_names else None)
        self.iter += k
        self._adam_step += k
        self._sched_steps += k
        self._folded_iters += k
        self._adam_folded = True
        last = out[k - 1].clone()
        self.last = (last[0], last[1], last[2])
        return True

    def closure(self):
        """train.py:195-199.  The L-BFGS stage holds the coefficients and the self-adaptive weights frozen at their
        Adam-final values (_bind), and the balanced group weights, folded into the scales once."""
        self._stage = LBFGS
        self.freeze_loss_weights()
        loss = self.loss_func()
        self.theta_param.grad = self.grad.clone()
        return loss

    def train(self):
        self.dnn.train()
        self.train_adam(self.adam_maxit)
        if self.config.lbfgs["max_it"] > 0:
            self.freeze_loss_weights()
            if self.lbfgs_impl == "device":
                self.train_lbfgs_device()
            else:
                self.optimizer_LBFGS.step(self.closure)                            # ONE step, train.py:200
        self.flush_log()

    def train_lbfgs_device(self):
        """The L-BFGS stage (train.py:200) through lbfgs.DeviceLBFGS: runs of up to DeviceLBFGS.RUN evaluations enqueued by
        one call each.  self.iter advances by one per evaluation (train.py:160) and every evaluation's three losses go
        into the log ring from the trace.  A run is cut so that an evaluation due a checkpoint (or the prediction dump) is
        its LAST slot: x_trial then still holds that evaluation's weights and the host saves from there — the
        reference's "weights of the evaluation, saved from inside loss_func" (train.py:175-179)."""
        self.theta = self.dnn.flat_params()
        self._stage = LBFGS
        lb = self.config.lbfgs
        has_fid = self.Xf is not None and self.Xf.shape[0] > 0
        nc = self._fid_sums.numel()
        X, n_res = self.evaluator.request_points(self.Xf, self.Xr, force_merge=True)      # (the loop is ONE request)
        opt = self.device_lbfgs = DeviceLBFGS(
            self.evaluator.eng, self.spec, self.theta, X, n_res, self._res_scale, self._loss_mat, 2,
            T=self.Tf if has_fid else None, out_col=self.fid_cols if nc else (), col_scale=self._fid_scale if nc else None,
            lr=lb["learning_rate"], max_iter=lb["max_it"], max_eval=lb.get("max_evaluation"), history_size=lb["history_size"],
            tolerance_grad=lb["tolerance_grad"], tolerance_change=lb["tolerance_change"], line_search_fn=lb["line_search_fn"])

        def due(it):       # evaluation number `it` (1-based, self.iter after it) needs the host right after it
            return self._checkpoint_due(it) or (self.mat_dump_iter is not None and it - 1 == self.mat_dump_iter)

        def before_run(_evals):
            for i in range(1, DeviceLBFGS.RUN + 1):
                if due(self.iter + i):
                    return i
            return DeviceLBFGS.RUN

        def after_run(tr):
            acts = tr[:, 2]
            k = int((acts != 0).sum())               # evaluations of this run: inert slots follow a stop
            rows = tr[:k, 10:13].to(torch.float32)
            self._to_ring(self.iter + 1, rows, self._extra_vals)      # (the frozen group weights, in their columns)
            self.iter += k
            if k:
                self.last = tuple(rows[k - 1].to(self.device))
            if k == tr.shape[0] and due(self.iter):      # the run's last slot was this evaluation: x_trial holds its weights
                keep = self.theta.clone()
                self.theta.copy_(opt.x_trial)
                if self.mat_dump_iter is not None and self.iter - 1 == self.mat_dump_iter:
                    self.dump_predictions(self.mat_dump_path)
                if self._checkpoint_due(self.iter):
                    self.save_checkpoint(f"model_{self.iter}.pth")
                self.theta.copy_(keep)

        opt.step(before_run, after_run)

    def residual_fields(self, X=None) -> torch.Tensor:
        """The residual's signed per-point fields (n_fields, N) at X (default: this rank's collocation shard), in
        eval mode: Navier_Stokes (fc, fm_x, fm_y), physics_equation (fc, fx, fy), continuity (fc, da)."""
        if self._coef is not None:
            raise PinnError("residual_fields does not run with runtime closure coefficients: the field kernels carry the constants")
        X = self.Xr if X is None else _as_f32(X, self.device)
        return self.evaluator.residual_fields(self.dnn.flat_params(), X)

    def predict(self, inputs) -> torch.Tensor:
        """Forward on a grid (test.py:76): (N, d_in) -> (N, d_out)."""
        X = _as_f32(inputs, self.device)
        return self.evaluator.predict(self.dnn.flat_params(), X)


pinn = PINN   # the reference's class name (train.py:46)
