"""dnn — drop-in for the reference's dnn.py (class DNN), running on the HIP engine.

Same constructor, same state_dict keys (layers.layer_{i}.weight / .bias), same
initialisation (dnn.py:42-52), nn.Module semantics.  Differences, all deliberate:
  * the Linear weights are views into ONE flat fp32 buffer [W0,b0,W1,b1,...] — the layout
    the C-ABI takes — so optimisers updating the Parameters in place update it too;
  * forward() runs on libpinn_hip.so and REQUIRES a GPU tensor: there is no CPU path;
  * Dropout(p>0) in training mode (dnn.py:38, train.py:186) uses the engine's counter-based mask (one fresh
    seed per forward call, drawn from torch's CPU generator; include/pinn_hip.h pinn_desc.dropout_p): same
    distribution as nn.Dropout, not torch's random stream.
One addition the reference does not have: first_activation="sin" makes the FIRST hidden layer a Fourier-feature layer,
a_1 = sin(W_0 x + b_0) with W_0 ~ N(0, fourier_sigma^2) and b_0 ~ U[0, 2 pi) (include/pinn_hip.h, PINN_ACT_SIN_TANH); W_0 and
b_0 stay ordinary trained parameters under the same state_dict keys.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import List, Optional, Sequence

import torch
import torch.nn as nn

from ._lib import ACT_SIN_TANH, PinnError
from .engine import ACTIVATION_OF_INIT


def _check_init_type(init_type: str):
    if init_type not in ACTIVATION_OF_INIT:
        # same exception type and text as dnn.py:23 / :49
        raise ValueError(f"Invalid init_type: {init_type}. Use 'kaiming' or 'xavier'.")


def _check_first_activation(first_activation, init_type: str, fourier_sigma):
    if first_activation is None:
        return
    if first_activation != "sin":
        raise ValueError(f"Invalid first_activation: {first_activation!r}. Use None or 'sin'.")
    if init_type != "xavier":
        raise ValueError("first_activation='sin' needs init_type='xavier' (the other hidden layers are tanh layers), "
                         f"got init_type={init_type!r}")
    if not (float(fourier_sigma) > 0.0 and math.isfinite(float(fourier_sigma))):
        raise ValueError(f"fourier_sigma must be a positive finite number, got {fourier_sigma!r}")


class Sin(nn.Module):
    """sin(x): the activation of a Fourier-feature first layer (no parameters)."""

    def forward(self, x):
        return torch.sin(x)


def activation_id_of(init_type: str, first_activation=None) -> int:
    """The ACT_* value of the engine (include/pinn_hip.h) for a network built with these constructor arguments."""
    return ACT_SIN_TANH if first_activation == "sin" else ACTIVATION_OF_INIT[init_type]


def init_flat_params(layers: Sequence[int], init_type: str = "xavier", generator=None, first_activation=None,
                     fourier_sigma: float = 1.0) -> torch.Tensor:
    """Flat [W0,b0,...] fp32 vector drawn from the distributions of dnn.py:42-52
    (Xavier/Kaiming-uniform weights; zero bias except the last layer's nn.Linear default).
    first_activation="sin": layer 0 is W_0 ~ N(0, fourier_sigma^2), b_0 ~ U[0, 2 pi) from the same generator."""
    _check_init_type(init_type)
    _check_first_activation(first_activation, init_type, fourier_sigma)
    parts = []
    n_lin = len(layers) - 1
    for i in range(n_lin):
        fan_in, fan_out = layers[i], layers[i + 1]
        if i == 0 and first_activation == "sin":
            parts.append(torch.empty(fan_out * fan_in).normal_(0.0, float(fourier_sigma), generator=generator))
            parts.append(torch.empty(fan_out).uniform_(0.0, 2.0 * math.pi, generator=generator))
            continue
        if init_type == "xavier":
            bound = math.sqrt(6.0 / (fan_in + fan_out))
        else:
            # kaiming_uniform_(w, nonlinearity='leaky_relu') leaves a at its default 0: gain sqrt(2/(1+0^2))
            # (dnn.py:45 — NOT the 0.01 slope of the LeakyReLU it then applies)
            bound = math.sqrt(2.0) * math.sqrt(3.0 / fan_in)
        parts.append(torch.empty(fan_out * fan_in).uniform_(-bound, bound, generator=generator))
        if i < n_lin - 1:
            parts.append(torch.zeros(fan_out))
        else:
            b = 1.0 / math.sqrt(fan_in)
            parts.append(torch.empty(fan_out).uniform_(-b, b, generator=generator))
    return torch.cat(parts)


class DNN(nn.Module):
    """The deep neural network (reference dnn.py:5-55)."""

    def __init__(self, layers, dropout_rate, init_type, first_activation=None, fourier_sigma=1.0):
        super().__init__()
        _check_init_type(init_type)
        _check_first_activation(first_activation, init_type, fourier_sigma)
        self.first_activation = first_activation
        self.fourier_sigma = float(fourier_sigma)
        if first_activation == "sin" and len(layers) < 3:
            raise ValueError("first_activation='sin' needs at least one hidden layer")
        self.activation = nn.Tanh() if init_type == "xavier" else nn.LeakyReLU(negative_slope=0.01)
        self.layer_sizes: List[int] = [int(v) for v in layers]
        self.dropout_rate = float(dropout_rate)
        self.init_type = init_type
        mods = []
        n = len(self.layer_sizes)
        for i in range(n - 1):
            lin = nn.Linear(self.layer_sizes[i], self.layer_sizes[i + 1])
            if init_type == "kaiming":
                nn.init.kaiming_uniform_(lin.weight, nonlinearity="leaky_relu")
            else:
                nn.init.xavier_uniform_(lin.weight)
            if i < n - 2:
                nn.init.zeros_(lin.bias)
            if i == 0 and first_activation == "sin":        # Fourier features: B ~ N(0, sigma^2), a random phase
                nn.init.normal_(lin.weight, 0.0, self.fourier_sigma)
                nn.init.uniform_(lin.bias, 0.0, 2.0 * math.pi)
            mods.append((f"layer_{i}", lin))
            if i < n - 2:
                mods.append((f"activation_{i}", Sin() if i == 0 and first_activation == "sin" else self.activation))
                mods.append((f"dropout_{i}", nn.Dropout(self.dropout_rate)))
        self.layers = nn.Sequential(OrderedDict(mods))
        self._flat: Optional[torch.Tensor] = None
        self._grad_cols_override = None
        self._flatten()

    # ---- flat parameter storage -----------------------------------------------------------
    def _linears(self):
        return [m for m in self.layers if isinstance(m, nn.Linear)]

    def _ordered_params(self):
        # cached: the trainer asks for this list (write_token, flat_params) on every iteration of a host-bound loop
        ps = self.__dict__.get("_plist")
        if ps is None:
            ps = []
            for lin in self._linears():
                ps += [lin.weight, lin.bias]
            self.__dict__["_plist"] = ps
        return ps

    def _flatten(self):
        self.__dict__.pop("_plist", None)      # the slow path re-reads the module tree (a layer replaced since the last time)
        ps = self._ordered_params()
        flat = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in ps])
        off = 0
        for p in ps:
            n = p.numel()
            p.data = flat[off:off + n].view_as(p)
            off += n
        self._flat = flat

    def _aliased(self) -> bool:
        flat = self._flat
        if flat is None:
            return False
        off = 0
        for p in self._ordered_params():
            if p.device != flat.device or p.dtype != torch.float32 or \
               p.data_ptr() != flat.data_ptr() + 4 * off or not p.is_contiguous():
                return False
            off += p.numel()
        return True

    def flat_params(self) -> torch.Tensor:
        """The (P,) fp32 buffer every Linear parameter aliases; rebuilt after .to()/.cuda()."""
        if not self._aliased():
            self._flatten()
        return self._flat

    def write_token(self, flat=None):
        """Changes whenever a Parameter of this module (or the flat buffer) is written in place through torch
        (optimizer.step, load_state_dict, clipping, p.mul_()): the version counters of every alias family of the flat
        buffer.  `p.data = flat[...]` gives each Parameter a counter of its own, so the flat buffer's alone would miss
        those writes (Engine.loss_grad_adam_step's packed-weights token)."""
        flat = self._flat if flat is None else flat     # (the caller's flat_params() result: already validated)
        if flat is None:
            flat = self.flat_params()
        return (id(flat), flat._version) + tuple([p._version for p in self._ordered_params()])

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.pop("_plist", None)
        if "layer_sizes" not in self.__dict__:          # a pickle written by the reference's class
            lins = self._linears()
            self.layer_sizes = [lins[0].in_features] + [l.out_features for l in lins]
            self.init_type = "xavier" if isinstance(self.activation, nn.Tanh) else "kaiming"
            drops = [m for m in self.layers if isinstance(m, nn.Dropout)]
            self.dropout_rate = float(drops[0].p) if drops else 0.0
            self._grad_cols_override = None
        if "first_activation" not in self.__dict__:     # the reference's class, or this one before it had the attribute
            self.first_activation = None
            self.fourier_sigma = 1.0
        self._flat = None

    @property
    def activation_id(self) -> int:
        """The engine's ACT_* value for this network (include/pinn_hip.h)."""
        return activation_id_of(self.init_type, self.__dict__.get("first_activation"))

    def set_grad_columns(self, cols: Optional[Sequence[int]]):
        """Name the differentiated input columns explicitly instead of reading them off the
        torch.cat graph (train.py:87-88, 148)."""
        self._grad_cols_override = None if cols is None else tuple(int(c) for c in cols)

    # ---- forward ----------------------------------------------------------------------------
    def forward(self, x):
        if not x.is_cuda:
            raise PinnError("DNN.forward needs a GPU tensor: pinn_depthestimation_amd has no CPU path "
                            "(move the model and its inputs to cuda)")
        from .autograd import dnn_forward
        drop = (0.0, 0)
        if self.training and self.dropout_rate > 0.0:       # a new mask per forward pass, as nn.Dropout draws one
            drop = (self.dropout_rate, int(torch.randint(0, 2 ** 31 - 1, (1,)).item()))
        return dnn_forward(self, x, drop)
