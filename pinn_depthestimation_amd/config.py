"""config — reads the reference's JSON configs verbatim (config_CMB.json, config_CMB_h.json and
the older-schema config.json / config_txyz.json) and exposes the few facts the hot path needs.

Reference behaviour kept: sections and key names; `requires_grad` is a LIST OF
STRINGS tested with `"true" in info["requires_grad"]` (train.py:87); float-typed iteration
counts (config.json:17 `5.00e4`, config_CMB.json:21 `6.25e4`) are coerced to int for loops.
Defaults for keys the old schema lacks: dropout_rate 0.0, init_type "xavier"
(train.py:59,62 would raise KeyError there).  Unknown extra keys (e.g. "engine") are ignored.
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple


def _names(section) -> List[str]:
    """A variable list may be a JSON list (config_CMB.json:42) or a dict keyed by name
    (config_CMB.json:48-51, config.json:40-45)."""
    if section is None:
        return []
    return list(section.keys()) if isinstance(section, dict) else list(section)


def _grad_cols(inputs) -> Tuple[int, ...]:
    if not isinstance(inputs, dict):
        return ()
    cols = []
    for i, (_, info) in enumerate(inputs.items()):
        if isinstance(info, dict) and "true" in info.get("requires_grad", []):   # train.py:87
            cols.append(i)
    return tuple(cols)


@dataclass
class PinnConfig:
    raw: dict
    layers: List[int]
    dropout_rate: float
    init_type: str
    adam: Dict[str, float]
    lbfgs: Dict[str, object]
    loss_weights: Dict[str, float]
    variant: str                           # "train" (train.py) or "newmethod" (train_newmethod.py)
    fidelity_inputs: List[str] = field(default_factory=list)
    fidelity_outputs: List[str] = field(default_factory=list)
    residual_inputs: List[str] = field(default_factory=list)
    residual_outputs: List[str] = field(default_factory=list)
    grad_cols: Tuple[int, ...] = ()
    trues: List[str] = field(default_factory=list)
    unknowns: List[str] = field(default_factory=list)
    # layers.first_activation ("sin": a Fourier-feature first layer, dnn.DNN) and layers.fourier_sigma (the standard deviation
    # of its weights, in the units of the normalised inputs); absent keys mean the reference's network
    first_activation: Optional[str] = None
    fourier_sigma: float = 1.0

    @property
    def weight_fid(self) -> float:
        return float(self.loss_weights.get("weight_fid_loss", 1))

    @property
    def weight_res(self) -> float:
        return float(self.loss_weights.get("weight_res_loss", 1))

    def output_weight(self, key: str) -> float:
        """config.loss.weight_<key>_loss (train.py:94-95); 1 when the old schema omits it."""
        return float(self.loss_weights.get(f"weight_{key}_loss", 1))

    @property
    def self_adaptive(self) -> Optional[dict]:
        """loss.self_adaptive: None (absent or false), or {"init", "mask", "per_term"} with the defaults filled in."""
        return self_adaptive_options(self.raw.get("loss", {}).get("self_adaptive"))

    @property
    def rad_importance(self) -> bool:
        """loss.rad_importance: importance weights on the RAD mini-batch."""
        return bool(self.raw.get("loss", {}).get("rad_importance", False))

    @property
    def weight_learning_rate(self) -> float:
        """adam_optimizer.weight_learning_rate: the self-adaptive weights' rate, default the network's."""
        return float(self.adam.get("weight_learning_rate", self.adam["learning_rate"]))

    @property
    def fold_extras(self) -> bool:
        """adam_optimizer.fold_extras: run Adam iterations with closure coefficients or point weights in device-enqueued
        runs (trainer.PINN(fold_extras=True)); off unless asked for."""
        return bool(self.adam.get("fold_extras", False))

    # gradient-statistics loss balancing (trainer.PINN(loss_balancing=...)): the weights of the loss groups set from the run
    @property
    def loss_balancing(self) -> Optional[str]:
        """loss.balancing: None (absent, null or "none"), "max_mean" or "norm"."""
        v = self.raw.get("loss", {}).get("balancing")
        return None if v in (None, False, "none") else str(v)

    @property
    def balance_every(self) -> int:
        """loss.balance_every: the weights are updated on every balance_every-th Adam iteration, from the first."""
        return int(self.raw.get("loss", {}).get("balance_every", 10))

    @property
    def balance_alpha(self) -> float:
        """loss.balance_alpha: the moving average's rate, in (0, 1]."""
        return float(self.raw.get("loss", {}).get("balance_alpha", 0.1))

    @property
    def balance_ref(self) -> str:
        """loss.balance_ref: the max/mean rule's reference group, "residual" or "fidelity"."""
        return str(self.raw.get("loss", {}).get("balance_ref", "residual"))

    @property
    def balance_groups(self) -> str:
        """loss.balance_groups: "sets" (residual, fidelity) or "terms" (a group per weighted residual term, and fidelity)."""
        return str(self.raw.get("loss", {}).get("balance_groups", "sets"))

    def default_residual(self) -> str:
        """The reference hard-codes the residual by import (train.py:17, train_newmethod.py:18);
        pick the one whose argument names the config's variables satisfy."""
        if self.variant == "newmethod":
            return "continuity_only"
        if "t" in self.residual_inputs:
            return "Navier_Stokes"
        if "eta_mean" in self.residual_outputs:
            return "physics_equation"
        return "continuity_ftemp"


SELF_ADAPTIVE_DEFAULTS = {"init": 1.0, "mask": "square", "per_term": True}


def self_adaptive_options(value) -> Optional[dict]:
    """The self-adaptive weights' options from `true` or an object {"init": 1.0, "mask": "square" | "linear",
    "per_term": true}; None for an absent or false key.  ValueError on an unknown key or mask."""
    if value is None or value is False:
        return None
    if value is True:
        return dict(SELF_ADAPTIVE_DEFAULTS)
    if not isinstance(value, dict):
        raise ValueError(f"self_adaptive = {value!r}: use true or an object with the keys {sorted(SELF_ADAPTIVE_DEFAULTS)}")
    unknown = sorted(set(value) - set(SELF_ADAPTIVE_DEFAULTS))
    if unknown:
        raise ValueError(f"self_adaptive: unknown key(s) {unknown}; known: {sorted(SELF_ADAPTIVE_DEFAULTS)}")
    out = {**SELF_ADAPTIVE_DEFAULTS, **value}
    if out["mask"] not in ("square", "linear"):
        raise ValueError(f"self_adaptive.mask = {out['mask']!r}: use 'square' or 'linear'")
    out["init"], out["per_term"] = float(out["init"]), bool(out["per_term"])
    return out


def load_config(src) -> PinnConfig:
    raw = src if isinstance(src, dict) else json.load(open(src, "r"))
    L = raw["layers"]
    layers = [int(L["input_features"])] + [int(L["hidden_width"])] * int(L["hidden_layers"]) + \
        [int(L["output_features"])]                                            # train.py:52-56
    adam = dict(raw.get("adam_optimizer", {}))
    adam["max_it"] = int(adam.get("max_it", 0))
    adam.setdefault("learning_rate", 1e-4)
    adam["scheduler_step_size"] = int(adam.get("scheduler_step_size", 10000))
    adam.setdefault("scheduler_gamma", 0.8)
    lb = dict(raw.get("lbfgs_optimizer", {}))
    lb["max_it"] = int(lb.get("max_it", 0))
    if "max_evaluation" in lb and lb["max_evaluation"] is not None:
        lb["max_evaluation"] = int(lb["max_evaluation"])
    lb.setdefault("learning_rate", 1)
    lb.setdefault("history_size", 100)
    lb.setdefault("tolerance_grad", 1e-5)
    lb.setdefault("tolerance_change", 1e-7)
    lb.setdefault("line_search_fn", "strong_wolfe")
    cfg = PinnConfig(raw=raw, layers=layers, dropout_rate=float(L.get("dropout_rate", 0.0)),
                     init_type=L.get("init_type", "xavier"), adam=adam, lbfgs=lb,
                     loss_weights=dict(raw.get("loss", {})), variant="train")
    cfg.first_activation = L.get("first_activation")
    if cfg.first_activation not in (None, "sin"):
        raise ValueError(f"layers.first_activation = {cfg.first_activation!r}: use \"sin\" or leave the key out")
    cfg.fourier_sigma = float(L.get("fourier_sigma", 1.0))
    if "data" in raw and "data_residual" not in raw:          # config_CMB_h.json:33-41
        d = raw["data"]
        cfg.variant = "newmethod"
        cfg.residual_inputs = _names(d["inputs"])
        cfg.grad_cols = _grad_cols(d["inputs"])
        cfg.trues, cfg.unknowns = _names(d.get("trues")), _names(d.get("unknowns"))
        cfg.fidelity_inputs = list(cfg.residual_inputs)
        cfg.fidelity_outputs = list(cfg.trues)
        cfg.residual_outputs = cfg.trues + cfg.unknowns          # train_newmethod.py:136-139
    else:
        df, dr = raw.get("data_fidelity", {}), raw.get("data_residual", {})
        cfg.fidelity_inputs = _names(df.get("inputs"))
        cfg.fidelity_outputs = _names(df.get("outputs"))
        cfg.residual_inputs = _names(dr.get("inputs"))
        cfg.residual_outputs = _names(dr.get("outputs"))
        cfg.grad_cols = _grad_cols(dr.get("inputs"))
    return cfg
