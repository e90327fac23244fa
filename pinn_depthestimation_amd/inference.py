"""inference — the reference's test.py / test_newmethod.py on the HIP engine: forward on the full
ny x nx grid and the optional physics-only L-BFGS fine-tune.

Reference behaviour kept (test.py:10-106): LBFGS(max_iter=1, max_eval=2, history_size=10) with the
config's lr/tolerances/line search (:44-54); inputs become one (N,1) tensor per config variable
with requires_grad from the config strings (:60-65); predictions are reshaped to (ny, nx) as
`plot_pred_<key>` and inputs denormalised to `plot_input_<key>` (:67-84); when
config['perform_optimization'] is true ONE optimizer_LBFGS.step(closure) runs on the residual
alone and the grid is predicted again (:92-104).  Differences: the model may be given as a DNN,
a whole-module file or a state_dict file; the residual follows the config's variable names
(the reference hard-wires Navier_Stokes at test.py:6 while its config_CMB.json has no `t`).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from . import operations as op
from . import physics
from .config import PinnConfig, load_config
from ._lib import PinnError
from .dnn import DNN
from .engine import RESIDUAL_ROLES, Engine, NetDesc, ResidualSpec


FIELD_NAMES = {"Navier_Stokes": ("fc", "fm_x", "fm_y"), "physics_equation": ("fc", "fx", "fy"),
               "continuity_ftemp": ("fc", "da"), "continuity_only": ("fc", "da")}


class Tester:
    def __init__(self, model, config, device="cuda", residual: Optional[str] = None, corrected: bool = False,
                 eddy_viscosity: float = 0.0, wave_period: Optional[float] = None, wave_gamma: Optional[float] = None):
        """wave_period (seconds) and wave_gamma, or the config keys loss.wave_period / loss.wave_gamma (with a wave period
        from either source loss.corrected_radiation_stress is read as well): the wave closure of the corrected physics_equation, five fields
        (fc, fx, fy, f_d, f_E) and five terms in the fine-tune (physics.physics_equation_wave).
        corrected (physics_equation only): residual_fields and the physics-only fine-tune use the corrected radiation
        stress (ResidualSpec.corrected, physics.physics_equation_corrected).
        eddy_viscosity (Navier_Stokes, physics_equation): nu of the lateral-mixing term -nu lap(U) in the momentum
        equations, in the units of the network's inputs (normalised to [-1, 1] in the reference's pipeline); residual_fields
        and the fine-tune residual both carry it."""
        self.config: PinnConfig = config if isinstance(config, PinnConfig) else load_config(config)
        self.device = torch.device(device)
        self.model = self.load_model(model)
        raw = self.config.raw
        dt = raw.get("data_test", {})
        ins = dt.get("inputs", raw.get("data_residual", {}).get("inputs", raw.get("data", {}).get("inputs", {})))
        self.test_input_vars: Dict[str, dict] = ins if isinstance(ins, dict) else {k: {"requires_grad": []} for k in ins}
        outs = dt.get("outputs", self.config.residual_outputs)
        self.test_output_vars = list(outs.keys()) if isinstance(outs, dict) else list(outs)
        self.nx, self.ny = dt.get("nx"), dt.get("ny")
        self.residual = residual or self.config.default_residual()
        self.corrected = bool(corrected)
        loss_cfg = raw.get("loss", {}) or {}
        if wave_period is None:
            wave_period = loss_cfg.get("wave_period")
        if wave_period is not None:      # (with a wave period in effect, from either source, the config's corrected key counts)
            self.corrected = self.corrected or bool(loss_cfg.get("corrected_radiation_stress", False))
        self.wave_period = None if wave_period is None else float(wave_period)
        self.wave_gamma = float(loss_cfg.get("wave_gamma", 0.42) if wave_gamma is None else wave_gamma)
        if self.wave_period is not None:
            if self.residual != "physics_equation" or not self.corrected:
                raise PinnError("wave_period is the wave closure of physics_equation with corrected=True; got residual "
                                f"{self.residual!r}, corrected={self.corrected}")
            if not (self.wave_period > 0 and self.wave_gamma > 0):
                raise PinnError(f"the wave closure needs wave_period > 0 and wave_gamma > 0 (got {self.wave_period}, {self.wave_gamma})")
            if eddy_viscosity:
                raise PinnError("the wave closure (wave_period) does not run with eddy_viscosity != 0")
        if self.corrected and self.residual != "physics_equation":
            raise PinnError(f"corrected=True is the radiation stress of physics_equation; residual {self.residual!r} has none")
        self.eddy_viscosity = float(eddy_viscosity)
        if not (self.eddy_viscosity >= 0.0 and self.eddy_viscosity != float("inf")):
            raise PinnError(f"eddy_viscosity = {self.eddy_viscosity}: must be finite and >= 0")
        if self.eddy_viscosity != 0 and self.residual not in ("Navier_Stokes", "physics_equation"):
            raise PinnError(f"eddy_viscosity is the lateral mixing of a momentum equation; residual {self.residual!r} has none")
        self.init_optimizers()
        self.last_loss = None

    @property
    def wave_omega(self) -> float:
        """2 pi / wave_period, 0 without the wave closure."""
        return 0.0 if self.wave_period is None else 2.0 * math.pi / self.wave_period

    def load_model(self, model) -> DNN:
        if isinstance(model, DNN):
            m = model
        else:
            try:
                obj = torch.load(model, map_location="cpu", weights_only=True)       # a state_dict file
            except Exception:
                obj = torch.load(model, map_location="cpu", weights_only=False)      # whole-module pickle (test.py:37)
            if isinstance(obj, DNN):
                m = obj
            else:
                m = DNN(self.config.layers, self.config.dropout_rate, self.config.init_type,
                        first_activation=self.config.first_activation, fourier_sigma=self.config.fourier_sigma)
                m.load_state_dict(obj)
        m.to(self.device)
        m.eval()
        return m

    def init_optimizers(self):
        lb = self.config.lbfgs
        self.optimizer_LBFGS = torch.optim.LBFGS(                                   # test.py:44-54
            self.model.parameters(), lr=lb["learning_rate"], max_iter=1, max_eval=2, history_size=10,
            tolerance_grad=lb["tolerance_grad"], tolerance_change=lb["tolerance_change"],
            line_search_fn=lb["line_search_fn"])

    def _residual_loss(self):
        _, out_roles, dir_roles = RESIDUAL_ROLES[self.residual]
        args = [getattr(self, k) for k in dir_roles] + [getattr(self, k) for k in out_roles]
        if self.eddy_viscosity != 0:
            kw = {"corrected": True} if self.corrected else {}
            return getattr(physics, self.residual)(*args, nu=self.eddy_viscosity, **kw)
        if self.wave_period is not None:
            return physics.physics_equation_wave(*args, omega=self.wave_omega, gamma=self.wave_gamma)
        fn = physics.physics_equation_corrected if self.corrected else getattr(physics, self.residual)
        return fn(*args)

    def test(self, test_input_data, input_min_max: Optional[dict] = None, perform_optimization: Optional[bool] = None):
        data = torch.as_tensor(np.asarray(test_input_data)).float().to(self.device)
        cols = []
        for i, (key, info) in enumerate(self.test_input_vars.items()):
            t = data[:, i:i + 1].clone().detach()
            if "true" in info.get("requires_grad", []):
                t = t.requires_grad_()
            setattr(self, key, t)
            cols.append(t)
            if self.nx and self.ny and t.numel() == self.nx * self.ny:
                grid = t.detach().cpu().numpy().reshape(self.ny, self.nx)
                if input_min_max is not None and key in input_min_max:
                    grid = op.denormalize(grid, input_min_max[key][0], input_min_max[key][1])
                setattr(self, f"plot_input_{key}", grid)
        pred = self.model(torch.cat(cols, dim=-1))
        self._publish(pred)
        if perform_optimization is None:
            perform_optimization = bool(self.config.raw.get("perform_optimization", False))
        if perform_optimization:
            def closure():                                                           # test.py:94-99
                self.optimizer_LBFGS.zero_grad()
                loss = self._residual_loss()
                if loss.requires_grad:
                    loss.backward()
                self.last_loss = loss.detach()
                return loss
            self.optimizer_LBFGS.step(closure)
            with torch.no_grad():
                pred = self.model(torch.cat(cols, dim=-1))
            self._publish(pred)
        return pred.detach().cpu().numpy()

    def residual_fields(self, test_input_data, input_min_max: Optional[dict] = None):
        """Residual maps beside test(): the residual's signed per-point fields on the test grid, one array per field
        (Navier_Stokes: fc, fm_x, fm_y; physics_equation: fc, fx, fy; continuity: fc, da), computed by the engine in
        eval mode (Engine.residual_fields).  Returns (n_fields, N); when the grid is ny x nx each field is also
        published as `plot_res_<name>` (ny, nx), and the inputs as `plot_input_<key>` exactly as test() does."""
        cfg = self.config
        data = torch.as_tensor(np.asarray(test_input_data)).float().to(self.device).contiguous()
        names = list(self.test_input_vars)
        grad_cols = tuple(i for i, k in enumerate(names) if "true" in self.test_input_vars[k].get("requires_grad", []))
        spec = ResidualSpec.from_names(self.residual, names, grad_cols, self.test_output_vars, corrected=self.corrected,
                                       nu=self.eddy_viscosity, wave_omega=self.wave_omega, wave_gamma=self.wave_gamma)
        key = (tuple(self.model.layer_sizes), grad_cols, self.model.activation_id)
        if getattr(self, "_fields_engine_key", None) != key:
            self._fields_engine = Engine(NetDesc.from_layers(self.model.layer_sizes, grad_cols,
                                                             self.model.activation_id), self.device)
            self._fields_engine_key = key
        if spec.nu != 0:
            F = self._fields_engine.residual2_loss_grad(spec, None, self.model.flat_params(), data, grad=None, fields=True)[1]
        else:
            F = self._fields_engine.residual_fields(spec, self.model.flat_params(), data)
        out = F.cpu().numpy()
        if self.nx and self.ny and data.shape[0] == self.nx * self.ny:
            for i, k in enumerate(names):
                grid = data[:, i].cpu().numpy().reshape(self.ny, self.nx)
                if input_min_max is not None and k in input_min_max:
                    grid = op.denormalize(grid, input_min_max[k][0], input_min_max[k][1])
                setattr(self, f"plot_input_{k}", grid)
            for name, row in zip(FIELD_NAMES[self.residual] + (("f_d", "f_E") if spec.wave else ()), out):
                setattr(self, f"plot_res_{name}", row.reshape(self.ny, self.nx))
        return out

    def _publish(self, pred):
        for i, key in enumerate(self.test_output_vars):
            t = pred[:, i:i + 1]
            setattr(self, key, t)
            if self.nx and self.ny and t.numel() == self.nx * self.ny:
                setattr(self, f"plot_pred_{key}", t.detach().cpu().numpy().reshape(self.ny, self.nx))
