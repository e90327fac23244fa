"""Engine — thin host wrapper that hands torch device tensors to the C-ABI.

PyTorch is plumbing here: device memory, the current HIP stream, and (in
parallel.py) torch.distributed.  All arithmetic of the hot path runs in
libpinn_hip.so.  Nothing in this file synchronises the device.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import (ACT_LEAKY_RELU, ACT_TANH, ENGINE_AUTO, ENGINE_FUSED, ENGINE_FUSED_BATCH, ENGINE_FUSED_COOP, ENGINE_FUSED_TILE, ENGINE_GENERIC,
                   ENGINE_WIDE, RES_CONTINUITY_FTEMP,
                   RES_CONTINUITY_ONLY, RES_FIELDS, RES_NAVIER_STOKES, RES_PHYSICS_EQUATION, RES_TERMS, PinnDesc, PinnError,
                   PinnResidualSpec, check)

ACTIVATION_OF_INIT = {"xavier": ACT_TANH, "kaiming": ACT_LEAKY_RELU}  # dnn.py:18-21

# residual name -> (id, output role names, direction role names)
RESIDUAL_ROLES = {
    "Navier_Stokes": (RES_NAVIER_STOKES, ("h", "z", "u", "v"), ("t", "x", "y")),          # physics.py:50
    "physics_equation": (RES_PHYSICS_EQUATION, ("h", "U", "V", "eta_mean", "Hrms", "k"), ("x", "y")),  # :91
    "continuity_ftemp": (RES_CONTINUITY_FTEMP, ("h", "U", "V"), ("x", "y")),               # physics.py:37
    "continuity_only": (RES_CONTINUITY_ONLY, ("h", "U", "V"), ("x", "y")),                 # physics.py:18
}


@dataclass(frozen=True)
class NetDesc:
    """Network geometry: layers = [d_in] + [width]*n_hidden + [d_out] (train.py:56)."""
    d_in: int
    d_out: int
    n_hidden: int
    width: int
    grad_cols: Tuple[int, ...] = ()      # X columns whose inputs have requires_grad "true" (train.py:87)
    activation: int = ACT_TANH
    engine: int = ENGINE_AUTO
    precision: int = 0                   # _lib.PREC_F32 / PREC_BF16 (bf16 MFMA operands, wide engine only)
    dropout_p: float = 0.0               # nn.Dropout rate applied after every hidden activation (training mode)

    @property
    def k(self) -> int:
        return len(self.grad_cols)

    @property
    def layers(self) -> List[int]:
        return [self.d_in] + [self.width] * self.n_hidden + [self.d_out]

    @property
    def n_params(self) -> int:
        ls = self.layers
        return sum(ls[i] * ls[i + 1] + ls[i + 1] for i in range(len(ls) - 1))

    def with_(self, **kw) -> "NetDesc":
        return dataclasses.replace(self, **kw)

    def c_struct(self) -> PinnDesc:
        if self.k > _lib.PINN_MAX_DIRS:
            raise PinnError(f"{self.k} differentiated inputs; the engine carries at most {_lib.PINN_MAX_DIRS}")
        d = PinnDesc()
        d.d_in, d.d_out, d.n_hidden, d.width = self.d_in, self.d_out, self.n_hidden, self.width
        d.k = self.k
        for j in range(_lib.PINN_MAX_DIRS):
            d.dir_col[j] = self.grad_cols[j] if j < self.k else -1
        d.activation, d.engine, d.precision = self.activation, self.engine, self.precision
        d.dropout_p, d.dropout_seed = float(self.dropout_p), 0
        return d

    @staticmethod
    def from_layers(layers: Sequence[int], grad_cols=(), activation=ACT_TANH, engine=ENGINE_AUTO, precision=0,
                    dropout_p=0.0) -> "NetDesc":
        if len(layers) < 3 or len(set(layers[1:-1])) != 1:
            raise PinnError(f"layers {list(layers)} are not [d_in] + [width]*n + [d_out] (train.py:56)")
        return NetDesc(layers[0], layers[-1], len(layers) - 2, layers[1], tuple(grad_cols), activation, engine, precision,
                       dropout_p)


@dataclass(frozen=True)
class ResidualSpec:
    """Which output column plays which role in a residual (physics.py signatures)."""
    name: str
    out_col: Tuple[int, ...]
    dir_of: Tuple[int, ...]           # per direction role: index into NetDesc.grad_cols
    threshold: float = 25.5           # physics.py:26
    anchor: float = 0.75              # physics.py:27
    corrected: bool = False           # physics_equation only: the corrected radiation stress (pinn_residual_spec.flags bit 0)
    wave_omega: float = 0.0           # physics_equation with corrected=True only: > 0 adds the wave closure (flags bit 1): the
                                      # dispersion relation and the wave-energy balance at angular frequency omega (rad/s)
    wave_gamma: float = 0.42          # ... its breaker index (Thornton & Guza 1983)
    nu: float = 0.0                   # lateral mixing -nu lap(U) in the momentum equations (Navier_Stokes, physics_equation), in
                                      # the units of the network's inputs; travels BESIDE the C struct (pinn_residual2_loss_grad)

    def __post_init__(self):
        if self.wave_omega != 0:
            if self.name != "physics_equation" or not self.corrected:
                raise PinnError("wave_omega is the wave closure of physics_equation with corrected=True (the dispersion and "
                                f"wave-energy terms close the corrected radiation stress); got residual {self.name!r}, "
                                f"corrected={self.corrected}")
            if not (self.wave_omega > 0 and self.wave_gamma > 0):
                raise PinnError(f"the wave closure needs wave_omega > 0 and wave_gamma > 0 (got {self.wave_omega}, {self.wave_gamma})")
            if self.nu != 0:
                raise PinnError("the wave closure has no second-order form: nu must be 0 with wave_omega")

    @property
    def residual_id(self) -> int:
        return RESIDUAL_ROLES[self.name][0]

    @property
    def closure_key(self):
        """What the workspace cache keys and the packed-copy token carry for the residual's closure, in `corrected`'s place:
        `corrected` itself, or "wave" with the wave closure (one entry, so that the token keeps its shape)."""
        return "wave" if self.wave else self.corrected

    @property
    def wave(self) -> bool:
        """The wave closure is on (pinn_residual_spec.flags bit 1)."""
        return self.wave_omega != 0

    def first_order(self, what: str) -> "ResidualSpec":
        """self, for a first-order entry: raises instead of silently dropping the second-order term."""
        if self.nu != 0:
            raise PinnError(f"{what} evaluates the first-order residual and would drop nu = {self.nu}: use residual2_loss_grad")
        return self

    @property
    def n_terms(self) -> int:
        return _lib.PEW_TERMS if self.wave else RES_TERMS[self.residual_id]

    @property
    def n_fields(self) -> int:
        """Rows of Engine.residual_fields: (fc, fm_x, fm_y) / (fc, fx, fy) / (fc, da); (fc, fx, fy, f_d, f_E) with the wave
        closure."""
        return _lib.PEW_TERMS if self.wave else RES_FIELDS[self.residual_id]

    @property
    def n_weighted_terms(self) -> int:
        """The terms residual_weighted_loss_grad weights, min(n_terms, n_fields): 3, 3, 1, 2 (continuity_only's third term,
        the count of points below the threshold, is a normaliser and never weighted)."""
        return min(self.n_terms, self.n_fields)

    @property
    def coef_names(self) -> Tuple[str, ...]:
        """The residual's closure coefficients, in the order of residual_coef_loss_grad's coef array: ("gamma_b",) for
        Navier_Stokes, ("Cd",) for the plain physics_equation, () for everything else (pinn_residual_coef_count)."""
        return () if self.corrected else _lib.RES_COEFS[self.residual_id]

    @property
    def n_coefs(self) -> int:
        return len(self.coef_names)

    @property
    def coef_defaults(self) -> Tuple[float, ...]:
        """The constants the other entries have compiled in (pinn_residual_coef_default): 0.78 / 0.002."""
        out = []
        for j in range(self.n_coefs):
            v = C.c_float()
            check(_lib.load().pinn_residual_coef_default(self.residual_id, j, C.byref(v)), "pinn_residual_coef_default")
            out.append(float(v.value))
        return tuple(out)

    def c_struct(self) -> PinnResidualSpec:
        s = PinnResidualSpec()
        s.residual_id = self.residual_id
        for r in range(_lib.PINN_MAX_ROLES):
            s.out_col[r] = self.out_col[r] if r < len(self.out_col) else 0
        for d in range(_lib.PINN_MAX_DIRS):
            s.dir_of[d] = self.dir_of[d] if d < len(self.dir_of) else 0
        s.flags = 3 if self.wave else (1 if self.corrected else 0)
        s.param[0], s.param[1] = (self.wave_omega, self.wave_gamma) if self.wave else (self.threshold, self.anchor)
        return s

    @staticmethod
    def from_names(name: str, input_names: Sequence[str], grad_cols: Sequence[int],
                   output_names: Sequence[str], corrected: bool = False, nu: float = 0.0,
                   wave_omega: float = 0.0, wave_gamma: float = 0.42) -> "ResidualSpec":
        """Map config variable names (config data_residual.inputs / outputs) onto roles.  corrected=True (physics_equation
        only): E = rho g Hrms^2 / 8 in place of the reference's E == 0, as physics.physics_equation(corrected=True).
        nu (Navier_Stokes, physics_equation): the lateral-mixing term -nu lap(U) in the momentum equations.
        wave_omega > 0 (with corrected=True): the wave closure, as physics.physics_equation(wave_omega=, wave_gamma=)."""
        if name not in RESIDUAL_ROLES:
            raise PinnError(f"unknown residual {name!r}; known: {sorted(RESIDUAL_ROLES)}")
        if corrected and name != "physics_equation":
            raise PinnError(f"corrected=True is the radiation stress of physics_equation; residual {name!r} has none")
        nu = float(nu)
        if not (nu >= 0.0 and nu != float("inf")):
            raise PinnError(f"nu = {nu}: the eddy viscosity must be finite and >= 0")
        if nu != 0 and name not in ("Navier_Stokes", "physics_equation"):
            raise PinnError(f"nu is the lateral mixing of a momentum equation; residual {name!r} has none")
        _, out_roles, dir_roles = RESIDUAL_ROLES[name]
        out_col = []
        for r in out_roles:
            if r not in output_names:
                raise PinnError(f"residual {name} needs output {r!r}; network outputs are {list(output_names)}")
            out_col.append(list(output_names).index(r))
        dir_of = []
        for r in dir_roles:
            if r not in input_names:
                raise PinnError(f"residual {name} needs input {r!r}; network inputs are {list(input_names)}")
            col = list(input_names).index(r)
            if col not in grad_cols:
                raise PinnError(f"input {r!r} must have requires_grad 'true' for residual {name}")
            dir_of.append(list(grad_cols).index(col))
        return ResidualSpec(name, tuple(out_col), tuple(dir_of), corrected=bool(corrected), nu=nu,
                            wave_omega=float(wave_omega or 0.0), wave_gamma=float(wave_gamma))


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk(t: torch.Tensor, name: str, shape=None):
    if not t.is_cuda:
        raise PinnError(f"{name} must live on the GPU (got {t.device}); this engine has no CPU path")
    if t.dtype != torch.float32:
        raise PinnError(f"{name} must be float32 (got {t.dtype})")
    if not t.is_contiguous():
        raise PinnError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise PinnError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")


def _out_cols(out_col: Sequence[int]):
    """The fidelity columns as the C-ABI's int32 array (never of length zero: ctypes would have no address for it)."""
    return (C.c_int32 * max(len(out_col), 1))(*out_col)


def _lr_list(lr, sequence: bool = False) -> Optional[List[float]]:
    """A list or tuple of learning rates (sequence=True: any iterable) as floats, one per enqueued iteration; None for one
    scalar rate."""
    return [float(x) for x in lr] if sequence or isinstance(lr, (list, tuple)) else None


def _balance_mode(mode) -> int:
    """A balancing mode by name (None / "none", "max_mean", "norm") or by its PINN_BALANCE_* number."""
    if isinstance(mode, int) and not isinstance(mode, bool):
        return mode
    if mode not in _lib.BALANCE_MODES:
        raise PinnError(f"loss balancing mode {mode!r}: use None, 'max_mean' or 'norm'")
    return _lib.BALANCE_MODES[mode]


def _adam_state(m, v, step, lr, beta1, beta2, eps, packed_valid: bool, n_rows: int, loss_rows, losses) -> _lib.PinnAdamState:
    """pinn_adam_state of a folded-Adam call; lr None: the rates travel beside it, one per iteration."""
    return _lib.PinnAdamState(_ptr(m), _ptr(v), int(step), 0.0 if lr is None else float(lr), float(beta1), float(beta2),
                              float(eps), 1 if packed_valid else 0, n_rows, _ptr(loss_rows), _ptr(losses))


# ---- the packed-weights token ------------------------------------------------------------------------------------------
# A folded-Adam call leaves the packed copy of the weights it trained in its workspace; the next one may skip the packing
# kernel only if that copy is still what it would pack: the same workspace tensor, the same `params` storage and torch
# version counter, the same caller's token and the same request (which picks the kernel, and with it the packed layout).
# A rule that forgot one of the five would train on stale weights without an error: it lives here, once.
def _packed_token(ws: torch.Tensor, params: torch.Tensor, params_token, req: tuple) -> tuple:
    """What a successful folded-Adam call stores: read AFTER the call, so the version is the one the call left."""
    return (ws, params.data_ptr(), params._version, params_token, req)


def _packed_valid(tok: Optional[tuple], ws: torch.Tensor, params: torch.Tensor, params_token, req: tuple) -> bool:
    """Whether the packed copy described by the stored token `tok` serves this call (the workspace by identity)."""
    return tok is not None and tok[0] is ws and tok[1:] == _packed_token(ws, params, params_token, req)[1:]


_NO_GUARD = contextlib.nullcontext()


class Engine:
    """One network geometry bound to one device; owns the workspace cache."""

    def __init__(self, desc: NetDesc, device: torch.device | str = "cuda"):
        self.lib = _lib.load()
        self.desc = desc
        self.device = torch.device(device)
        self._cdesc: Dict[int, PinnDesc] = {}
        self._ws: Dict[object, torch.Tensor] = {}      # buffer key -> workspace (_workspace)
        self._ws_need: Dict[tuple, int] = {}           # need key -> bytes the query answered
        self._packed_tok = None      # _packed_token after loss_grad_adam_step / adam_loop_ext
        self._ens_packed_tok = None  # ... after ensemble_adam_step, for the M packed copies in the ensemble workspace
        self.dropout_seed = 0        # training-mode dropout: the caller sets a fresh seed per forward pass; the
                                     # reverse sweep of that pass must run under the same one (include/pinn_hip.h)
        cnt = C.c_int64()
        check(self.lib.pinn_param_count(C.byref(desc.c_struct()), C.byref(cnt)), "pinn_param_count")
        self.n_params = cnt.value

    # ---- plumbing -------------------------------------------------------------------
    def _e(self, engine: Optional[int]) -> int:
        return self.desc.engine if engine is None else engine

    def _d(self, engine: Optional[int] = None) -> PinnDesc:
        e = self._e(engine)
        if e not in self._cdesc:
            self._cdesc[e] = self.desc.with_(engine=e).c_struct()
        d = self._cdesc[e]
        d.dropout_seed = int(self.dropout_seed) & 0xFFFFFFFF
        return d

    def _chk(self, t: torch.Tensor, name: str, shape=None):
        _chk(t, name, shape)
        if t.device.index != self._index():
            raise PinnError(f"{name} lives on {t.device} but this engine is bound to {self.device}")

    def _chk_px(self, params: torch.Tensor, X: torch.Tensor) -> int:
        """Checks the flat parameter vector and the points; returns N."""
        N = X.shape[0]
        self._chk(params, "params", (self.n_params,)); self._chk(X, "X", (N, self.desc.d_in))
        return N

    def _sums(self, sums: Optional[torch.Tensor], name: str, shape, like: torch.Tensor) -> torch.Tensor:
        """The caller's buffer for loss sums, checked like every other argument, or a new one on `like`'s device."""
        if sums is None:
            return torch.empty(shape, dtype=torch.float32, device=like.device)
        self._chk(sums, name, shape)
        return sums

    def _chk_losses(self, loss_rows: Optional[torch.Tensor], losses, n_in: int, lead: tuple) -> int:
        """Checks loss_rows (rows, n_in) and losses (*lead, rows); returns rows, 0 without loss_rows."""
        if loss_rows is None:
            return 0
        n_rows = loss_rows.shape[0]
        self._chk(loss_rows, "loss_rows", (n_rows, n_in)); self._chk(losses, "losses", (*lead, n_rows))
        return n_rows

    @staticmethod
    def _unsupported(rc: int, what: str) -> bool:
        """True where the library refused the request (the caller returns False, the reason is in last_error()); any other
        failure is raised."""
        if rc == _lib.ERR_UNSUPPORTED:
            return True
        check(rc, what)
        return False

    def _index(self) -> int:
        """Ordinal of this engine's GPU ("cuda" without an index binds to the device current at first use)."""
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        return self.device.index

    def _guard(self):
        """A context in which this engine's device is current; nothing is exchanged where it already is."""
        idx = self._index()
        return _NO_GUARD if torch.cuda.current_device() == idx else torch.cuda.device(idx)

    def _stream(self):
        """The current stream of this engine's device, as the last argument of a C-ABI call."""
        return C.c_void_p(torch.cuda.current_stream(self._index()).cuda_stream)

    def _run(self, what: str, fn, *args):
        """Call one C-ABI entry point on THIS engine's device and on that device's current stream
        (appended as the last argument), whatever device the calling thread has current: launch
        geometry (CU count) and the stream both belong to the device the tensors live on."""
        self._packed_tok = None      # any other call may re-pack the workspace from ITS params argument
        self._ens_packed_tok = None  # (the ensemble calls' token: the same rule)
        with self._guard():
            check(fn(*args, self._stream()), what)

    # ---- the workspace cache ----------------------------------------------------------------------------------------
    def _workspace(self, buf_key, need_key, query) -> Tuple[int, Optional[torch.Tensor]]:
        """(0, the buffer `buf_key`, of at least the bytes the query answers for `need_key`), or (rc, None) where the
        query fails.  query() -> (rc, bytes) runs once per need key; a failed one is not remembered and touches no buffer.
        One uint8 buffer per buf_key on this engine's device, of at least 256 bytes: it only grows, and a request that
        fits gets the very tensor the last one got.  Kinds never share a buffer: what one call leaves in its workspace
        (the packed weights) survives calls of another kind."""
        need = self._ws_need.get(need_key)
        if need is None:
            rc, need = query()
            if rc != 0:
                return rc, None
            self._ws_need[need_key] = need
        ws = self._ws.get(buf_key)
        if ws is None or ws.numel() < need:
            self._ws[buf_key] = ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
            if buf_key == "ens":      # the members' packed copies went with the old buffer
                self._ens_packed_tok = None
        return 0, ws

    def _query(self, symbol: str, *args) -> Tuple[int, int]:
        """(rc, bytes) of the workspace query `symbol`, asked with this engine's device current (the answer depends on
        that device's CU count wherever the query reads it)."""
        need = C.c_int64()
        with self._guard():
            rc = getattr(self.lib, symbol)(*args, C.byref(need))
        return rc, need.value

    def _checked_workspace(self, kind, symbol: str, spec: Optional[ResidualSpec], N: int, engine, *key) -> torch.Tensor:
        """The buffer (kind, engine) — kind None: workspace()'s own, keyed by the engine alone — sized by `symbol`
        (desc[, spec], N), one query per (kind, engine, *key, N); a failed query is raised."""
        e = self._e(engine)
        buf_key, need_key = (e, (e, N)) if kind is None else ((kind, e), (kind, e, *key, N))

        def query():
            of = (C.byref(self._d(e)),) if spec is None else (C.byref(self._d(e)), C.byref(spec.c_struct()))
            return self._query(symbol, *of, N)
        rc, ws = self._workspace(buf_key, need_key, query)
        check(rc, symbol)
        return ws

    def workspace(self, N: int, engine: Optional[int] = None) -> torch.Tensor:
        return self._checked_workspace(None, "pinn_query_workspace", None, N, engine)

    def jet2_workspace(self, N: int, engine: Optional[int] = None) -> torch.Tensor:
        """Workspace of the second-order calls (pinn_query_jet2_workspace), cached apart from workspace()'s."""
        return self._checked_workspace("jet2", "pinn_query_jet2_workspace", None, N, engine)

    # ---- calls ------------------------------------------------------------------------------------
    def forward(self, params: torch.Tensor, X: torch.Tensor, engine=None) -> torch.Tensor:
        N = self._chk_px(params, X)
        Y = torch.empty(N, self.desc.d_out, dtype=torch.float32, device=X.device)
        ws = self.workspace(N, engine)
        self._run("pinn_forward", self.lib.pinn_forward, C.byref(self._d(engine)), _ptr(params), _ptr(X), N, _ptr(Y), _ptr(ws),
                  ws.numel())
        return Y

    def forward_jet(self, params: torch.Tensor, X: torch.Tensor, engine=None):
        N = self._chk_px(params, X)
        Y = torch.empty(N, self.desc.d_out, dtype=torch.float32, device=X.device)
        dY = torch.empty(self.desc.k, N, self.desc.d_out, dtype=torch.float32, device=X.device)
        ws = self.workspace(N, engine)
        self._run("pinn_forward_jet", self.lib.pinn_forward_jet, C.byref(self._d(engine)), _ptr(params), _ptr(X), N, _ptr(Y), _ptr(dY),
                                        _ptr(ws), ws.numel())
        return Y, dY

    def jet_backward(self, params, X, gY: Optional[torch.Tensor], gdY: Optional[torch.Tensor],
                     grad: torch.Tensor, engine=None) -> torch.Tensor:
        """grad += d/d params [sum(gY*Y) + sum(gdY*dY)] (pinn_jet_backward); either adjoint may be None.  engine=None
        is the descriptor's engine: AUTO runs an MFMA kernel where one serves the request (width <= 64, no dropout,
        k != 1 when gdY is given; the batch kernel for narrow tanh networks from 4096 points on, else the tile kernel)
        and the generic engine otherwise; FUSED is refused where AUTO would fall back.  jet_backward_kernel() tells which."""
        N = self._chk_px(params, X)
        self._chk(grad, "grad", (self.n_params,))
        if gY is not None: self._chk(gY, "gY", (N, self.desc.d_out))
        if gdY is not None: self._chk(gdY, "gdY", (self.desc.k, N, self.desc.d_out))
        ws = self.workspace(N, engine)
        self._run("pinn_jet_backward", self.lib.pinn_jet_backward, C.byref(self._d(engine)), _ptr(params), _ptr(X), N, _ptr(gY),
                                         _ptr(gdY), _ptr(grad), _ptr(ws), ws.numel())
        return grad

    def jet_backward_kernel(self, N: int, with_gdY: bool = True, engine: Optional[int] = None) -> int:
        """The kernel a jet_backward call on N points would run (pinn_jet_backward_kernel): ENGINE_GENERIC,
        ENGINE_FUSED_TILE or ENGINE_FUSED_BATCH.  Raises PinnError where the call itself would be refused.  Host logic
        only: no device is touched."""
        kern = C.c_int32()
        check(self.lib.pinn_jet_backward_kernel(C.byref(self._d(engine)), int(N), 1 if with_gdY else 0, C.byref(kern)),
              "pinn_jet_backward_kernel")
        return kern.value

    @property
    def n_pairs(self) -> int:
        """Second-order pairs (i, j), i <= j, of the differentiated inputs: the rows of d2Y."""
        return self.desc.k * (self.desc.k + 1) // 2

    def forward_jet2(self, params: torch.Tensor, X: torch.Tensor, engine=None):
        """(Y, dY, d2Y): Y (N, d_out), dY (k, N, d_out), d2Y (P, N, d_out) with row p = pair (i, j) of the
        differentiated columns, upper triangle row-major (pinn_forward_jet2)."""
        N = self._chk_px(params, X)
        Y = torch.empty(N, self.desc.d_out, dtype=torch.float32, device=X.device)
        dY = torch.empty(self.desc.k, N, self.desc.d_out, dtype=torch.float32, device=X.device)
        d2Y = torch.empty(self.n_pairs, N, self.desc.d_out, dtype=torch.float32, device=X.device)
        ws = self.jet2_workspace(N, engine)
        self._run("pinn_forward_jet2", self.lib.pinn_forward_jet2, C.byref(self._d(engine)), _ptr(params), _ptr(X), N,
                  _ptr(Y), _ptr(dY), _ptr(d2Y), _ptr(ws), ws.numel())
        return Y, dY, d2Y

    def jet2_backward(self, params, X, gY: Optional[torch.Tensor], gdY: Optional[torch.Tensor],
                      gd2Y: Optional[torch.Tensor], grad: torch.Tensor, engine=None) -> torch.Tensor:
        """grad += d/d params [sum(gY*Y) + sum(gdY*dY) + sum(gd2Y*d2Y)] (pinn_jet2_backward); any adjoint may be None."""
        N = self._chk_px(params, X)
        self._chk(grad, "grad", (self.n_params,))
        if gY is not None: self._chk(gY, "gY", (N, self.desc.d_out))
        if gdY is not None: self._chk(gdY, "gdY", (self.desc.k, N, self.desc.d_out))
        if gd2Y is not None: self._chk(gd2Y, "gd2Y", (self.n_pairs, N, self.desc.d_out))
        ws = self.jet2_workspace(N, engine)
        self._run("pinn_jet2_backward", self.lib.pinn_jet2_backward, C.byref(self._d(engine)), _ptr(params), _ptr(X), N,
                  _ptr(gY), _ptr(gdY), _ptr(gd2Y), _ptr(grad), _ptr(ws), ws.numel())
        return grad

    def residual_loss(self, spec: ResidualSpec, params, X, engine=None) -> torch.Tensor:
        spec.first_order("residual_loss")
        N = self._chk_px(params, X)
        sums = self._sums(None, "sums", (spec.n_terms,), X)
        ws = self.workspace(N, engine)
        self._run("pinn_residual_loss", self.lib.pinn_residual_loss, C.byref(self._d(engine)), C.byref(spec.c_struct()), _ptr(params),
                                          _ptr(X), N, _ptr(sums), _ptr(ws), ws.numel())
        return sums

    def fields_workspace(self, spec: ResidualSpec, N: int, engine: Optional[int] = None) -> torch.Tensor:
        """Workspace of residual_fields (pinn_query_fields_workspace), cached apart from workspace()'s."""
        spec.first_order("fields_workspace")
        return self._checked_workspace("fields", "pinn_query_fields_workspace", spec, N, engine, spec.residual_id, spec.closure_key)

    def residual_fields(self, spec: ResidualSpec, params, X, engine=None) -> torch.Tensor:
        """The residual's signed per-point fields, (n_fields, N): row f is field f at every row of X
        (pinn_residual_fields); sum over points of row t squared is residual_loss's term_sums[t].  engine=None is the
        descriptor's engine: AUTO runs the MFMA tile kernel's field instances where they exist (width <= 64, fp32, no
        dropout) and the forward jet plus a point-wise kernel otherwise; FUSED is refused where AUTO would fall back."""
        spec.first_order("residual_fields")
        N = self._chk_px(params, X)
        out = torch.empty(spec.n_fields, N, dtype=torch.float32, device=X.device)
        ws = self.fields_workspace(spec, N, engine)
        self._run("pinn_residual_fields", self.lib.pinn_residual_fields, C.byref(self._d(engine)), C.byref(spec.c_struct()),
                  _ptr(params), _ptr(X), N, _ptr(out), _ptr(ws), ws.numel())
        return out

    def residual_loss_grad(self, spec: ResidualSpec, term_scale: torch.Tensor, params, X, grad: torch.Tensor,
                           engine=None, sums: Optional[torch.Tensor] = None) -> torch.Tensor:
        """grad += sum_t term_scale[t] * d(term_sums[t])/d(params); returns term_sums (device)."""
        spec.first_order("residual_loss_grad")
        N = self._chk_px(params, X)
        self._chk(grad, "grad", (self.n_params,)); self._chk(term_scale, "term_scale", (spec.n_terms,))
        sums = self._sums(sums, "sums", (spec.n_terms,), X)
        ws = self.workspace(N, engine)
        self._run("pinn_residual_loss_grad", self.lib.pinn_residual_loss_grad, C.byref(self._d(engine)), C.byref(spec.c_struct()),
                                               _ptr(term_scale), _ptr(params), _ptr(X), N, _ptr(sums),
                                               _ptr(grad), _ptr(ws), ws.numel())
        return sums

    def residual_coef_workspace(self, spec: ResidualSpec, N: int, engine: Optional[int] = None) -> torch.Tensor:
        """Workspace of residual_coef_loss_grad (pinn_query_residual_coef_workspace), cached apart from the others."""
        spec.first_order("residual_coef_workspace")
        return self._checked_workspace("coef", "pinn_query_residual_coef_workspace", spec, N, engine, spec.residual_id, spec.closure_key)

    def residual_coef_loss_grad(self, spec: ResidualSpec, coef: torch.Tensor, term_scale: Optional[torch.Tensor], params, X,
                                grad: Optional[torch.Tensor] = None, coef_grad: Optional[torch.Tensor] = None,
                                sums: Optional[torch.Tensor] = None, engine=None) -> torch.Tensor:
        """residual_loss_grad with the residual's closure coefficients read from the device tensor `coef` (spec.coef_names:
        gamma_b of Navier_Stokes, Cd of physics_equation) instead of the compiled-in constants (pinn_residual_coef_loss_grad).
        Returns term_sums; with `grad`, grad += sum_t term_scale[t] d term_sums[t] / d params, and with `coef_grad` as well,
        coef_grad += the same derivative with respect to coef.  grad=None: forward only (term_scale may then be None).
        coef_grad=None: the coefficients are values only.  Their VALUES are not checked: they never leave the device.
        engine=None is the descriptor's: AUTO runs the tile kernel's coefficient instances where they exist (fp32, tanh,
        width <= 64, no dropout) and the generic engine otherwise."""
        spec.first_order("residual_coef_loss_grad")
        N = self._chk_px(params, X)
        if coef is None:
            raise PinnError("residual_coef_loss_grad: coef is None (use residual_loss_grad for the compiled-in constants)")
        self._chk(coef, "coef", (max(spec.n_coefs, 1),))
        if grad is not None:
            self._chk(grad, "grad", (self.n_params,)); self._chk(term_scale, "term_scale", (spec.n_terms,))
        if coef_grad is not None:
            if grad is None:
                raise PinnError("residual_coef_loss_grad: coef_grad without grad (the coefficient gradient comes out of the gradient pass)")
            self._chk(coef_grad, "coef_grad", (max(spec.n_coefs, 1),))
        sums = self._sums(sums, "sums", (spec.n_terms,), X)
        ws = self.residual_coef_workspace(spec, N, engine)
        self._run("pinn_residual_coef_loss_grad", self.lib.pinn_residual_coef_loss_grad, C.byref(self._d(engine)),
                  C.byref(spec.c_struct()), _ptr(coef), _ptr(term_scale) if grad is not None else None, _ptr(params), _ptr(X), N,
                  _ptr(sums), _ptr(grad), _ptr(coef_grad), _ptr(ws), ws.numel())
        return sums

    def residual_weighted_workspace(self, spec: ResidualSpec, N: int, engine: Optional[int] = None) -> torch.Tensor:
        """Workspace of residual_weighted_loss_grad (pinn_query_residual_weighted_workspace), cached apart from the others."""
        spec.first_order("residual_weighted_workspace")
        return self._checked_workspace("weighted", "pinn_query_residual_weighted_workspace", spec, N, engine, spec.residual_id,
                                       spec.closure_key)

    def residual_weighted_loss_grad(self, spec: ResidualSpec, weights: torch.Tensor, scale: Optional[torch.Tensor], theta, X,
                                    grad: Optional[torch.Tensor] = None, sums: Optional[torch.Tensor] = None, fields=None,
                                    engine=None):
        """residual_loss_grad with a weight on every point's squared fields (pinn_residual_weighted_loss_grad):
        term_sums[t] = sum_n w_t[n] f_t[n]^2 for the spec.n_weighted_terms first terms.  `weights` is (N,) — one weight per
        point for every term — or (w_rows, N) with w_rows 1 or spec.n_weighted_terms, contiguous fp32 on the device; its
        VALUES are not checked.  With `grad`, grad += sum_t scale[t] d term_sums[t] / d theta; grad=None: forward only
        (scale may then be None).  fields: None, a (n_fields, N) tensor to overwrite with the unweighted signed fields, or
        True to allocate one.  Returns term_sums, or (term_sums, fields) when fields were asked for."""
        spec.first_order("residual_weighted_loss_grad")
        N = self._chk_px(theta, X)
        if weights is None:
            raise PinnError("residual_weighted_loss_grad: weights is None (use residual_loss_grad for the unweighted sums)")
        if weights.dim() not in (1, 2) or weights.shape[-1] != N:
            raise PinnError(f"residual_weighted_loss_grad: weights must be (N,) or (w_rows, N) with N = {N}, got {tuple(weights.shape)}")
        w_rows = 1 if weights.dim() == 1 else int(weights.shape[0])
        self._chk(weights, "weights", tuple(weights.shape))
        if grad is not None:
            self._chk(grad, "grad", (self.n_params,)); self._chk(scale, "term_scale", (spec.n_terms,))
        sums = self._sums(sums, "sums", (spec.n_terms,), X)
        if fields is True:
            fields = torch.empty(spec.n_fields, N, dtype=torch.float32, device=X.device)
        elif fields is not None and fields is not False:
            self._chk(fields, "fields", (spec.n_fields, N))
        else:
            fields = None
        ws = self.residual_weighted_workspace(spec, N, engine)
        # (an empty tensor has no address, and a NULL point_w is refused whatever N: at N = 0, where nothing is read, the sums'
        # address stands in)
        wp = _ptr(weights) if N > 0 else _ptr(sums)
        self._run("pinn_residual_weighted_loss_grad", self.lib.pinn_residual_weighted_loss_grad, C.byref(self._d(engine)),
                  C.byref(spec.c_struct()), _ptr(scale) if grad is not None else None, wp, w_rows, _ptr(theta), _ptr(X), N,
                  _ptr(sums), _ptr(fields), _ptr(grad), _ptr(ws), ws.numel())
        return sums if fields is None else (sums, fields)

    def residual2_workspace(self, spec: ResidualSpec, N: int, engine: Optional[int] = None) -> torch.Tensor:
        """Workspace of residual2_loss_grad (pinn_query_residual2_workspace), cached apart from the others."""
        return self._checked_workspace("res2", "pinn_query_residual2_workspace", spec, N, engine, spec.residual_id)

    def residual2_loss_grad(self, spec: ResidualSpec, term_scale: Optional[torch.Tensor], params, X,
                            grad: Optional[torch.Tensor] = None, fields: bool = False,
                            sums: Optional[torch.Tensor] = None, engine=None):
        """The residual with the lateral-mixing term -spec.nu lap(U) in its momentum equations, on the second-order jets
        (pinn_residual2_loss_grad): returns term_sums, or (term_sums, fields (n_fields, N)) with fields=True; with `grad`
        also grad += sum_t term_scale[t] * d(term_sums[t])/d(params).  grad=None runs no backward sweep (term_scale may
        then be None).  spec.nu == 0 gives the first-order residual.  engine=None is the descriptor's: AUTO runs the MFMA
        kernels where every layer is at most 64 wide (fp32, no dropout) and the generic ones otherwise."""
        N = self._chk_px(params, X)
        if grad is not None:
            self._chk(grad, "grad", (self.n_params,)); self._chk(term_scale, "term_scale", (spec.n_terms,))
        sums = self._sums(sums, "sums", (spec.n_terms,), X)
        out = torch.empty(spec.n_fields, N, dtype=torch.float32, device=X.device) if fields else None
        ws = self.residual2_workspace(spec, N, engine)
        self._run("pinn_residual2_loss_grad", self.lib.pinn_residual2_loss_grad, C.byref(self._d(engine)),
                  C.byref(spec.c_struct()), C.c_float(spec.nu), _ptr(term_scale) if grad is not None else None, _ptr(params),
                  _ptr(X), N, _ptr(sums), _ptr(out), _ptr(grad), _ptr(ws), ws.numel())
        return (sums, out) if fields else sums

    def mse_loss_grad(self, params, X, T: torch.Tensor, out_col: Sequence[int],
                      col_scale: Optional[torch.Tensor], grad: Optional[torch.Tensor], engine=None,
                      sums: Optional[torch.Tensor] = None) -> torch.Tensor:
        N, nc = self._chk_px(params, X), len(out_col)
        self._chk(T, "T", (N, nc))
        if grad is not None:
            self._chk(grad, "grad", (self.n_params,)); self._chk(col_scale, "col_scale", (nc,))
        sums = self._sums(sums, "sums", (nc,), X)
        ws = self.workspace(N, engine)
        self._run("pinn_mse_loss_grad", self.lib.pinn_mse_loss_grad, C.byref(self._d(engine)), _ptr(params), _ptr(X), _ptr(T), N, nc,
                                          _out_cols(out_col), _ptr(col_scale), _ptr(sums), _ptr(grad), _ptr(ws), ws.numel())
        return sums

    def residual_mse_loss_grad(self, spec: ResidualSpec, term_scale, T: torch.Tensor, out_col: Sequence[int],
                               col_scale, params, X, grad, engine=None, term_sums=None, col_sums=None):
        """One pass over one point set: PDE residual + fidelity columns (train_newmethod.py:122-159)."""
        spec.first_order("residual_mse_loss_grad")
        N, nc = self._chk_px(params, X), len(out_col)
        self._chk(T, "T", (N, nc))
        self._chk(grad, "grad", (self.n_params,)); self._chk(term_scale, "term_scale", (spec.n_terms,))
        self._chk(col_scale, "col_scale", (nc,))
        term_sums = self._sums(term_sums, "term_sums", (spec.n_terms,), X)
        col_sums = self._sums(col_sums, "col_sums", (nc,), X)
        ws = self.workspace(N, engine)
        self._run("pinn_residual_mse_loss_grad", self.lib.pinn_residual_mse_loss_grad, C.byref(self._d(engine)), C.byref(spec.c_struct()), _ptr(term_scale),
                                                   _ptr(T), nc, _out_cols(out_col), _ptr(col_scale), _ptr(params), _ptr(X), N,
                                                   _ptr(term_sums), _ptr(col_sums), _ptr(grad), _ptr(ws), ws.numel())
        return term_sums, col_sums

    def residual_mse_split_loss_grad(self, spec: ResidualSpec, term_scale, T: torch.Tensor, out_col: Sequence[int],
                                     col_scale, params, X, n_res: int, grad, engine=None, term_sums=None,
                                     col_sums=None):
        """train.py:131-157 in one launch: X = [n_res collocation points ; fidelity points], T = the
        fidelity targets (N - n_res, n_cols)."""
        spec.first_order("residual_mse_split_loss_grad")
        N, nc = self._chk_px(params, X), len(out_col)
        self._chk(T, "T", (N - n_res, nc))
        self._chk(grad, "grad", (self.n_params,)); self._chk(term_scale, "term_scale", (spec.n_terms,))
        self._chk(col_scale, "col_scale", (nc,))
        term_sums = self._sums(term_sums, "term_sums", (spec.n_terms,), X)
        col_sums = self._sums(col_sums, "col_sums", (nc,), X)
        ws = self.workspace(N, engine)
        self._run("pinn_residual_mse_split_loss_grad", self.lib.pinn_residual_mse_split_loss_grad,
            C.byref(self._d(engine)), C.byref(spec.c_struct()), _ptr(term_scale), _ptr(T), nc, _out_cols(out_col), _ptr(col_scale),
            _ptr(params), _ptr(X), N, int(n_res), _ptr(term_sums), _ptr(col_sums), _ptr(grad), _ptr(ws), ws.numel())
        return term_sums, col_sums

    def loss_grad_adam_step(self, spec: ResidualSpec, term_scale, params, X, n_res: int, grad, m, v, step: int, lr,
                            T: Optional[torch.Tensor] = None, out_col: Sequence[int] = (), col_scale=None,
                            term_sums=None, col_sums=None, beta1=0.9, beta2=0.999, eps=1e-8,
                            loss_rows: Optional[torch.Tensor] = None, losses: Optional[torch.Tensor] = None,
                            params_token=None) -> bool:
        """train.py:189-193 in two launches (pinn_loss_grad_adam_step): loss + gradient at `params`, then ONE kernel
        that finishes sums and gradient, applies Adam to params / m / v and refreshes the packed weights of this N's
        workspace; with `loss_rows` (rows x (len(out_col) + n_terms)) it also writes losses = loss_rows @ [col sums | term sums].
        `lr` a sequence of n learning rates: n consecutive iterations (steps step .. step + n - 1) enqueued by ONE call
        (pinn_adam_loop), iteration i writing losses[i].
        Returns False — nothing launched — when the request is not a one-pass request of the fused engine.
        The packing kernel is skipped when the previous call on this engine was this method and `params` has not
        been written since: same workspace, same storage, same torch version counter of `params` AND the same
        `params_token` (_packed_valid).  torch's version counter is per alias family: tensors that share `params`' storage
        through `.data` (dnn.DNN's Linear weights, `p.data = flat[...]`) have counters of their own, so a caller whose buffer
        is aliased that way passes a token that changes whenever any alias is written (DNN.write_token(): the
        Parameters' version counters); writes no counter sees (`p.data.mul_()`) need invalidate_packed()."""
        spec.first_order("loss_grad_adam_step")
        lrs = _lr_list(lr)
        N, nc = self._chk_px(params, X), len(out_col)
        for t, nme in ((grad, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
            self._chk(t, nme, (self.n_params,))
        self._chk(term_scale, "term_scale", (spec.n_terms,)); self._chk(term_sums, "term_sums", (spec.n_terms,))
        if nc:
            self._chk(col_scale, "col_scale", (nc,)); self._chk(col_sums, "col_sums", (nc,))
            if n_res != N:
                self._chk(T, "T", (N - n_res if n_res >= 0 else N, nc))
        n_rows = self._chk_losses(loss_rows, losses, nc + spec.n_terms, () if lrs is None else (len(lrs),))
        ws = self.workspace(N)
        req = (N, int(n_res), nc, spec.residual_id, spec.closure_key)
        st = _adam_state(m, v, step, None if lrs is not None else lr, beta1, beta2, eps,
                         _packed_valid(self._packed_tok, ws, params, params_token, req), n_rows, loss_rows, losses)
        self._packed_tok = None
        head = (C.byref(self._d()), C.byref(spec.c_struct()), _ptr(term_scale), _ptr(T), nc, _out_cols(out_col), _ptr(col_scale),
                _ptr(params), _ptr(X), N, int(n_res), _ptr(term_sums), _ptr(col_sums), _ptr(grad), C.byref(st))
        with self._guard():
            tail = (_ptr(ws), ws.numel(), self._stream())
            if lrs is None:
                rc = self.lib.pinn_loss_grad_adam_step(*head, *tail)
            else:
                rc = self.lib.pinn_adam_loop(*head, len(lrs), (C.c_double * len(lrs))(*lrs), *tail)
        if self._unsupported(rc, "pinn_loss_grad_adam_step" if lrs is None else "pinn_adam_loop"):
            return False
        self._packed_tok = _packed_token(ws, params, params_token, req)
        return True

    def adam_loop_ext(self, spec: ResidualSpec, term_scale, params, X, grad, m, v, step: int, lr: Sequence[float],
                      Xf: Optional[torch.Tensor] = None, T: Optional[torch.Tensor] = None, out_col: Sequence[int] = (),
                      col_scale=None, term_sums=None, col_sums=None,
                      coef=None, coef_m=None, coef_v=None, coef_grad=None, coef_mask=None, coef_log=None, lr_coef=None,
                      point_w=None, fields=None, lam=None, lam_m=None, lam_v=None, sa_mask: str = "square", lr_w=None,
                      beta1=0.9, beta2=0.999, eps=1e-8, loss_rows: Optional[torch.Tensor] = None,
                      losses: Optional[torch.Tensor] = None, params_token=None) -> bool:
        """len(lr) Adam iterations of the residual with closure coefficients (`coef`) or with point weights (`point_w`)
        enqueued by ONE call (pinn_adam_loop_ext): per iteration the residual pass on X, the fidelity pass on (Xf, T) when Xf
        is given (Xf may be X itself), and one finishing kernel — gradient, Adam on params / m / v, the sums, the weighted
        losses (losses[i] = loss_rows @ [col sums | term sums]) and
          coefficients: coef_log[i] <- coef as iteration i ran with it, coef_grad <- its gradient (times coef_mask), Adam
            with lr_coef[i] on coef / coef_m / coef_v; coef_grad=None: the coefficients are values only;
          weights: lam=None — point_w (N,) or (w_rows, N) is fixed and read only (fields, if given, gets every pass's
            unweighted signed fields); lam given — the self-adaptive multipliers: Adam with lr_w[i] raises lam / lam_m /
            lam_v (w_rows, N) along the weighted loss and point_w = lam^2 (sa_mask "square") or lam ("linear") is rewritten.
        grad is OVERWRITTEN with the last iteration's gradient.  Returns False — nothing launched, the reason in
        last_error() — where the request is not served (engine, precision, activation, width, dropout, corrected, the
        continuity residuals with coef, both groups).  The packing kernel is skipped under loss_grad_adam_step's rules."""
        spec.first_order("adam_loop_ext")
        lrs = _lr_list(lr, sequence=True)
        k = len(lrs)
        N, nc = self._chk_px(params, X), len(out_col)
        for t, nme in ((grad, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
            self._chk(t, nme, (self.n_params,))
        self._chk(term_scale, "term_scale", (spec.n_terms,)); self._chk(term_sums, "term_sums", (spec.n_terms,))
        n_fid = 0 if Xf is None else Xf.shape[0]
        if nc:
            self._chk(col_sums, "col_sums", (nc,))
        if n_fid:
            self._chk(Xf, "Xf", (n_fid, self.desc.d_in)); self._chk(T, "T", (n_fid, nc)); self._chk(col_scale, "col_scale", (nc,))
        n_rows = self._chk_losses(loss_rows, losses, nc + spec.n_terms, (k,))
        ex = _lib.PinnAdamExtras()
        kind = ("coef" if coef is not None else "") + ("w" if point_w is not None else "") + ("sa" if lam is not None else "")
        keep = []          # ctypes arrays must outlive the call
        if coef is not None:
            nco = max(spec.n_coefs, 1)
            for t, nme in ((coef, "coef"), (coef_m, "coef_m"), (coef_v, "coef_v"), (coef_grad, "coef_grad"), (coef_mask, "coef_mask")):
                if t is not None:
                    self._chk(t, nme, (nco,))
            if coef_log is not None:
                self._chk(coef_log, "coef_log", (k, nco))
            ex.coef, ex.coef_m, ex.coef_v, ex.coef_grad = (t.data_ptr() if t is not None else None for t in (coef, coef_m, coef_v, coef_grad))
            ex.coef_mask = coef_mask.data_ptr() if coef_mask is not None else None
            ex.coef_log = coef_log.data_ptr() if coef_log is not None else None
        if point_w is not None:
            if point_w.dim() not in (1, 2) or point_w.shape[-1] != N:
                raise PinnError(f"adam_loop_ext: point_w must be (N,) or (w_rows, N) with N = {N}, got {tuple(point_w.shape)}")
            self._chk(point_w, "point_w", tuple(point_w.shape))
            ex.point_w, ex.w_rows = point_w.data_ptr(), (1 if point_w.dim() == 1 else int(point_w.shape[0]))
            if fields is not None:
                self._chk(fields, "fields", (spec.n_fields, N)); ex.fields = fields.data_ptr()
            if lam is not None:
                if sa_mask not in ("square", "linear"):
                    raise PinnError(f"adam_loop_ext: sa_mask = {sa_mask!r}: use 'square' or 'linear'")
                for t, nme in ((lam, "lam"), (lam_m, "lam_m"), (lam_v, "lam_v")):
                    if t is not None:
                        self._chk(t, nme, (ex.w_rows, N))
                ex.lam, ex.lam_m, ex.lam_v = (t.data_ptr() if t is not None else None for t in (lam, lam_m, lam_v))
                ex.sa_mask = 0 if sa_mask == "square" else 1

        def darr(xs):
            if xs is None:
                return None
            xs = [float(x) for x in xs]
            if len(xs) != k:
                raise PinnError(f"adam_loop_ext: {len(xs)} learning rates for {k} iterations")
            a = (C.c_double * max(k, 1))(*xs); keep.append(a)
            return a

        rc, ws = self._workspace("adamext", ("adamext", kind, spec.residual_id, spec.closure_key, N, n_fid), lambda: self._query(
            "pinn_query_adam_ext_workspace", C.byref(self._d()), C.byref(spec.c_struct()), C.byref(ex), N, n_fid))
        if self._unsupported(rc, "pinn_query_adam_ext_workspace"):
            return False
        req = ("ext", kind, N, n_fid, nc, spec.residual_id, spec.closure_key)
        st = _adam_state(m, v, step, None, beta1, beta2, eps, _packed_valid(self._packed_tok, ws, params, params_token, req),
                         n_rows, loss_rows, losses)
        self._packed_tok = None
        self._ens_packed_tok = None
        with self._guard():
            rc = self.lib.pinn_adam_loop_ext(
                C.byref(self._d()), C.byref(spec.c_struct()), _ptr(term_scale), _ptr(Xf) if n_fid else None,
                _ptr(T) if n_fid else None, n_fid, nc, _out_cols(out_col), _ptr(col_scale) if n_fid else None, _ptr(params), _ptr(X), N,
                _ptr(term_sums), _ptr(col_sums) if nc else None, _ptr(grad), C.byref(st), C.byref(ex), k, darr(lrs),
                darr(lr_coef), darr(lr_w), _ptr(ws), ws.numel(), self._stream())
        if self._unsupported(rc, "pinn_adam_loop_ext"):
            return False
        if k > 0:
            self._packed_tok = _packed_token(ws, params, params_token, req)
        return True

    # ---- gradient-statistics loss balancing (pinn_balance_*) ------------------------------------------------------------
    def balance_weights_host(self, stats, lam, mode, ref: int = 0, alpha: float = 0.1, P: int = 1):
        """The update rule alone, on host arrays (pinn_balance_weights_host; no device): stats (G, 3) float64 rows
        [max|g|, sum|g|, sum g^2], lam (G,) float32 -> the new weights, a float32 numpy array."""
        import numpy as np
        st = np.ascontiguousarray(stats, dtype=np.float64)
        lam_in = np.ascontiguousarray(lam, dtype=np.float32)
        G = lam_in.shape[0]
        if st.shape != (G, _lib.BALANCE_STATS):
            raise PinnError(f"balance_weights_host: stats has shape {st.shape}, expected {(G, _lib.BALANCE_STATS)}")
        out = np.empty_like(lam_in)
        check(self.lib.pinn_balance_weights_host(
            _balance_mode(mode), G, int(ref), float(alpha), int(P), st.ctypes.data_as(C.POINTER(C.c_double)),
            lam_in.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float))), "pinn_balance_weights_host")
        return out

    def balance_update(self, grads: torch.Tensor, lam: torch.Tensor, mode, ref: int = 0, alpha: float = 0.1,
                       stats: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, P: Optional[int] = None):
        """pinn_balance_update on G flat gradients, the rows of grads (G, ld): the statistics of the first P (default ld)
        entries of every row into stats (G, 3) float64 if given, the rule on lam (G,) in place, and with `out` (P,) the
        combination out = sum_j lam[j] grads[j] with the new weights.  mode None / "none": combination only."""
        if grads.dim() != 2:
            raise PinnError(f"balance_update: grads must be (G, ld), got {tuple(grads.shape)}")
        G, ld = int(grads.shape[0]), int(grads.shape[1])
        P = ld if P is None else int(P)
        self._chk(grads, "grads", (G, ld)); self._chk(lam, "lam", (G,))
        if out is not None:
            self._chk(out, "out", (P,))
        if stats is not None:
            if stats.dtype != torch.float64 or not stats.is_contiguous() or tuple(stats.shape) != (G, _lib.BALANCE_STATS) or stats.device != grads.device:
                raise PinnError(f"balance_update: stats must be a contiguous float64 ({G}, {_lib.BALANCE_STATS}) tensor on {grads.device}")
        rc, ws = self._workspace("balance", ("balance", P, G), lambda: self._query("pinn_query_balance_workspace", P, G))
        check(rc, "pinn_query_balance_workspace")
        tok = self._packed_tok, self._ens_packed_tok      # (this call touches no packed weights: the tokens survive it)
        self._run("pinn_balance_update", self.lib.pinn_balance_update, _balance_mode(mode), G, int(ref), float(alpha), _ptr(grads),
                  P, ld, _ptr(lam), _ptr(stats), _ptr(out), _ptr(ws), ws.numel())
        self._packed_tok, self._ens_packed_tok = tok
        return out

    def adam_loop_balanced(self, spec: ResidualSpec, term_scale, params, X, grad, m, v, step: int, lr: Sequence[float],
                           Xf: torch.Tensor, T: torch.Tensor, out_col: Sequence[int], col_scale, lam: torch.Tensor, mode,
                           every: int = 10, ref: int = 0, alpha: float = 0.1, term_sums=None, col_sums=None,
                           lam_log=None, stats_log=None, group_grads=None, beta1=0.9, beta2=0.999, eps=1e-8,
                           loss_rows: Optional[torch.Tensor] = None, losses: Optional[torch.Tensor] = None,
                           params_token=None) -> bool:
        """len(lr) Adam iterations with two balanced loss groups enqueued by ONE call (pinn_adam_loop_balanced): per iteration
        the plain residual pass on X, the fidelity pass on (Xf, T), on iterations with (step + i - 1) % every == 0 the
        statistics of the two gradients and the rule on lam (2,) = [residual, fidelity], and one finishing kernel:
        grad = lam[0] g_res + lam[1] g_fid, Adam on params / m / v, the sums, the weighted losses (by the caller's scales,
        not by lam).  lam_log (k, 2): the weights each iteration stepped with; stats_log (k, 2, 3) float64: the statistics of
        the update iterations; group_grads (2, P): the last iteration's two gradients.  Returns False — nothing launched,
        the reason in last_error() — where the request is not served.  The packing kernel is skipped under
        loss_grad_adam_step's rules."""
        spec.first_order("adam_loop_balanced")
        lrs = _lr_list(lr, sequence=True)
        k = len(lrs)
        N, nc = self._chk_px(params, X), len(out_col)
        for t, nme in ((grad, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
            self._chk(t, nme, (self.n_params,))
        self._chk(term_scale, "term_scale", (spec.n_terms,)); self._chk(term_sums, "term_sums", (spec.n_terms,))
        n_fid = Xf.shape[0]
        self._chk(col_sums, "col_sums", (nc,)); self._chk(col_scale, "col_scale", (nc,))
        self._chk(Xf, "Xf", (n_fid, self.desc.d_in)); self._chk(T, "T", (n_fid, nc))
        self._chk(lam, "lam", (2,))
        if lam_log is not None:
            self._chk(lam_log, "lam_log", (k, 2))
        if group_grads is not None:
            self._chk(group_grads, "group_grads", (2, self.n_params))
        if stats_log is not None and (stats_log.dtype != torch.float64 or not stats_log.is_contiguous() or
                                      tuple(stats_log.shape) != (k, 2, _lib.BALANCE_STATS) or stats_log.device != params.device):
            raise PinnError(f"adam_loop_balanced: stats_log must be a contiguous float64 ({k}, 2, {_lib.BALANCE_STATS}) tensor on {params.device}")
        n_rows = self._chk_losses(loss_rows, losses, nc + spec.n_terms, (k,))
        bal = _lib.PinnBalance(_balance_mode(mode), int(every), int(ref), float(alpha), lam.data_ptr(),
                               None if lam_log is None else lam_log.data_ptr(), None if stats_log is None else stats_log.data_ptr(),
                               None if group_grads is None else group_grads.data_ptr())
        # (the extended loop's buffer: the same layout with the statistics' partials behind it, one packed copy for both)
        rc, ws = self._workspace("adamext", ("adambal", spec.residual_id, spec.closure_key, N, n_fid), lambda: self._query(
            "pinn_query_adam_balanced_workspace", C.byref(self._d()), C.byref(spec.c_struct()), N, n_fid))
        if self._unsupported(rc, "pinn_query_adam_balanced_workspace"):
            return False
        req = ("bal", N, n_fid, nc, spec.residual_id, spec.closure_key)
        st = _adam_state(m, v, step, None, beta1, beta2, eps, _packed_valid(self._packed_tok, ws, params, params_token, req),
                         n_rows, loss_rows, losses)
        self._packed_tok = None
        self._ens_packed_tok = None
        lr_arr = (C.c_double * max(k, 1))(*lrs)
        with self._guard():
            rc = self.lib.pinn_adam_loop_balanced(
                C.byref(self._d()), C.byref(spec.c_struct()), _ptr(term_scale), _ptr(Xf), _ptr(T), n_fid, nc, _out_cols(out_col),
                _ptr(col_scale), _ptr(params), _ptr(X), N, _ptr(term_sums), _ptr(col_sums), _ptr(grad), C.byref(st),
                C.byref(bal), k, lr_arr, _ptr(ws), ws.numel(), self._stream())
        if self._unsupported(rc, "pinn_adam_loop_balanced"):
            return False
        if k > 0:
            self._packed_tok = _packed_token(ws, params, params_token, req)
        return True

    # ---- the device-resident L-BFGS loop (pinn_lbfgs_loop) ------------------------------------------------------------
    def lbfgs_loop_query(self, N: int, history_size: int) -> Tuple[int, int]:
        """(workspace bytes, state bytes) of lbfgs_loop on N points with this history size (pinn_query_lbfgs_loop)."""
        ws, st = C.c_int64(), C.c_int64()
        with self._guard():      # the pass's workspace depends on the device's CU count
            check(self.lib.pinn_query_lbfgs_loop(C.byref(self._d()), int(N), int(history_size), C.byref(ws), C.byref(st)),
                  "pinn_query_lbfgs_loop")
        return ws.value, st.value

    def lbfgs_loop_init(self, state: torch.Tensor, lr, max_iter, max_eval, history_size, tolerance_grad, tolerance_change):
        """Zeroes `state` (uint8, at least the query's state bytes) and arms its control block (pinn_lbfgs_loop_init)."""
        o = _lib.PinnLbfgsOpts(float(lr), float(tolerance_grad), float(tolerance_change), int(max_iter), int(max_eval),
                               int(history_size))
        self._run("pinn_lbfgs_loop_init", self.lib.pinn_lbfgs_loop_init, _ptr(state), state.numel(), self.n_params, C.byref(o))

    def lbfgs_loop(self, spec: ResidualSpec, term_scale, params, X, n_res: int, loss_rows: torch.Tensor, total_row: int,
                   state: torch.Tensor, n_slots: int, trace: Optional[torch.Tensor] = None, T: Optional[torch.Tensor] = None,
                   out_col: Sequence[int] = (), col_scale=None, ws: Optional[torch.Tensor] = None):
        """n_slots slots of the device-resident L-BFGS loop (pinn_lbfgs_loop): every slot one loss + gradient evaluation
        and one step of the strong-Wolfe state machine, decided on the device.  X, n_res, T, out_col and the scales as
        loss_grad_adam_step; loss_rows (rows x (len(out_col) + n_terms)), total_row the objective's row.  `params` holds the
        accepted iterate whenever the enqueued work has run; trace (n_slots, LBFGS_TRACE_COLS) float64, optional."""
        spec.first_order("lbfgs_loop")
        N, nc = self._chk_px(params, X), len(out_col)
        self._chk(term_scale, "term_scale", (spec.n_terms,))
        self._chk(loss_rows, "loss_rows", (loss_rows.shape[0], nc + spec.n_terms))
        if nc:
            self._chk(col_scale, "col_scale", (nc,))
            if n_res != N:
                self._chk(T, "T", (N - n_res if n_res >= 0 else N, nc))
        if trace is not None and (trace.dtype != torch.float64 or not trace.is_contiguous()
                                  or tuple(trace.shape) != (n_slots, _lib.LBFGS_TRACE_COLS) or trace.device != params.device):
            raise PinnError(f"trace must be a contiguous float64 ({n_slots}, {_lib.LBFGS_TRACE_COLS}) tensor on {params.device}")
        if state.dtype != torch.uint8 or not state.is_contiguous() or state.device != params.device:
            raise PinnError("state must be a contiguous uint8 tensor on the engine's device")
        if ws is None:
            ws = self.workspace(N)
        self._run("pinn_lbfgs_loop", self.lib.pinn_lbfgs_loop, C.byref(self._d()), C.byref(spec.c_struct()), _ptr(term_scale),
                  _ptr(T), nc, _out_cols(out_col), _ptr(col_scale), _ptr(params), _ptr(X), N, int(n_res), loss_rows.shape[0],
                  _ptr(loss_rows), int(total_row), _ptr(state), state.numel(), int(n_slots), _ptr(trace), _ptr(ws), ws.numel())

    # ---- ensembles: M networks of this geometry in one launch (pinn_ensemble_*) ---------------------------------------------
    def _ensemble_workspace(self, M: int, N: int) -> Tuple[int, Optional[torch.Tensor]]:
        """(rc, workspace) of the ensemble calls: _workspace on pinn_ensemble_query_workspace, the one buffer "ens"."""
        return self._workspace("ens", ("ens", int(M), int(N)), lambda: self._query(
            "pinn_ensemble_query_workspace", C.byref(self._d()), int(M), int(N)))

    def ensemble_workspace(self, M: int, N: int) -> torch.Tensor:
        """Workspace of the ensemble calls for M members on N points (pinn_ensemble_query_workspace), cached apart from
        workspace()'s.  Raises PinnError with the engine's reason where the ensemble calls are refused."""
        rc, ws = self._ensemble_workspace(M, N)
        check(rc, "pinn_ensemble_query_workspace")
        return ws

    def ensemble_plan(self, M: int, N: int) -> Tuple[int, bool]:
        """(workgroups per member, whether a workgroup's gradient copy lives in LDS) of an ensemble pass of M members on N
        points (pinn_ensemble_plan).  Raises PinnError where the ensemble calls are refused.  Host logic only."""
        gx, lds = C.c_int32(), C.c_int32()
        with self._guard():
            check(self.lib.pinn_ensemble_plan(C.byref(self._d()), int(M), int(N), C.byref(gx), C.byref(lds)), "pinn_ensemble_plan")
        return gx.value, bool(lds.value)

    def ensemble_refusal(self, spec: ResidualSpec, M: int, N: int, n_res: int, n_cols: int) -> Optional[str]:
        """Why the ensemble calls would refuse this request (None: they serve it), in the engine's own words: the
        descriptor's part from pinn_ensemble_plan, the request's part (corrected radiation stress, the split request at
        hidden width 33..64) from pinn_ensemble_loss_grad called WITHOUT arrays — it decides its refusals before it
        looks at a pointer (pinn_hip.h) and then stops at the NULL arguments.  Host logic only: nothing is launched."""
        gx, lds = C.c_int32(), C.c_int32()
        with self._guard():
            rc = self.lib.pinn_ensemble_plan(C.byref(self._d()), int(M), int(N), C.byref(gx), C.byref(lds))
            if rc == 0:
                rc = self.lib.pinn_ensemble_loss_grad(C.byref(self._d()), C.byref(spec.c_struct()), int(M), None, None, int(n_cols),
                                                      _out_cols(range(n_cols)), None, None, None, int(N), int(n_res), 0, None, None,
                                                      None, None, 0, None)
        if rc == _lib.ERR_UNSUPPORTED:
            return self.last_error()
        if rc not in (0, _lib.ERR_INVALID):
            check(rc, "pinn_ensemble_loss_grad")
        if rc == _lib.ERR_INVALID and "NULL pointer" not in self.last_error():
            raise PinnError(f"ensemble request is invalid: {self.last_error()}")
        return None

    def _ensemble_args(self, spec, term_scale, params, X, n_res, grad, T, out_col, col_scale, term_sums, col_sums):
        """Shapes of an ensemble request: (M, N, nc, flags, term_sums, col_sums)."""
        if params.dim() != 2:
            raise PinnError(f"params must be (M, {self.n_params}), got {tuple(params.shape)}")
        M, nc = params.shape[0], len(out_col)
        own_x = X.dim() == 3
        N = X.shape[1] if own_x else X.shape[0]
        self._chk(params, "params", (M, self.n_params)); self._chk(grad, "grad", (M, self.n_params))
        self._chk(X, "X", (M, N, self.desc.d_in) if own_x else (N, self.desc.d_in))
        self._chk(term_scale, "term_scale", (spec.n_terms,))
        flags = _lib.ENSEMBLE_OWN_X if own_x else 0
        term_sums = self._sums(term_sums, "term_sums", (M, spec.n_terms), params)
        if nc:
            self._chk(col_scale, "col_scale", (nc,))
            col_sums = self._sums(col_sums, "col_sums", (M, nc), params)
            if n_res != N:
                rows = N - n_res if n_res >= 0 else N
                if T is not None and T.dim() == 3:
                    flags |= _lib.ENSEMBLE_OWN_T
                    self._chk(T, "T", (M, rows, nc))
                else:
                    self._chk(T, "T", (rows, nc))
        return M, N, nc, flags, term_sums, col_sums

    def ensemble_loss_grad(self, spec: ResidualSpec, term_scale, params, X, n_res: int, grad, T: Optional[torch.Tensor] = None,
                           out_col: Sequence[int] = (), col_scale=None, term_sums=None, col_sums=None):
        """Loss sums and gradients of M networks in one pass (pinn_ensemble_loss_grad).  params, grad (M, P); X (N, d_in)
        shared by the members or (M, N, d_in) one point set each; n_res as loss_grad_adam_step (== N residual only, 0 <=
        n_res < N split, < 0 both terms on every point); T (rows, nc) shared or (M, rows, nc).  grad += the weighted
        gradient of each member; returns (term_sums (M, n_terms), col_sums (M, nc) or None).  Raises PinnError with the
        engine's reason, nothing launched, where the request has no ensemble kernel."""
        spec.first_order("ensemble_loss_grad")
        M, N, nc, flags, term_sums, col_sums = self._ensemble_args(spec, term_scale, params, X, n_res, grad, T, out_col, col_scale,
                                                                   term_sums, col_sums)
        ws = self.ensemble_workspace(M, N)
        self._run("pinn_ensemble_loss_grad", self.lib.pinn_ensemble_loss_grad, C.byref(self._d()), C.byref(spec.c_struct()), M,
                  _ptr(term_scale), _ptr(T), nc, _out_cols(out_col), _ptr(col_scale), _ptr(params), _ptr(X), N, int(n_res), flags,
                  _ptr(term_sums), _ptr(col_sums), _ptr(grad), _ptr(ws), ws.numel())
        return term_sums, col_sums

    def ensemble_adam_step(self, spec: ResidualSpec, term_scale, params, X, n_res: int, grad, m, v, step: int, lr,
                           T: Optional[torch.Tensor] = None, out_col: Sequence[int] = (), col_scale=None,
                           term_sums=None, col_sums=None, beta1=0.9, beta2=0.999, eps=1e-8,
                           loss_rows: Optional[torch.Tensor] = None, losses: Optional[torch.Tensor] = None,
                           params_token=None) -> bool:
        """loss_grad_adam_step for M networks: two launches per iteration whatever M is (pinn_ensemble_adam_step; `lr` a
        sequence: pinn_ensemble_adam_loop, one call for len(lr) iterations).  params, grad, m, v (M, P); term_sums
        (M, n_terms), col_sums (M, nc); losses (M, rows), with an lr sequence (len(lr), M, rows).  One step count and one
        learning-rate schedule for all members.  Returns False — nothing launched, the reason in last_error() — where the
        request has no ensemble kernel.  The packed-weights token is this method's own, under loss_grad_adam_step's rules."""
        spec.first_order("ensemble_adam_step")
        lrs = _lr_list(lr)
        M, N, nc, flags, term_sums, col_sums = self._ensemble_args(spec, term_scale, params, X, n_res, grad, T, out_col, col_scale,
                                                                   term_sums, col_sums)
        for t, nme in ((m, "exp_avg"), (v, "exp_avg_sq")):
            self._chk(t, nme, (M, self.n_params))
        n_rows = self._chk_losses(loss_rows, losses, nc + spec.n_terms, (M,) if lrs is None else (len(lrs), M))
        rc, ws = self._ensemble_workspace(M, N)
        if self._unsupported(rc, "pinn_ensemble_query_workspace"):
            return False
        req = (M, N, int(n_res), nc, flags, spec.residual_id, spec.closure_key)
        st = _adam_state(m, v, step, None if lrs is not None else lr, beta1, beta2, eps,
                         _packed_valid(self._ens_packed_tok, ws, params, params_token, req), n_rows, loss_rows, losses)
        self._ens_packed_tok = None
        head = (C.byref(self._d()), C.byref(spec.c_struct()), M, _ptr(term_scale), _ptr(T), nc, _out_cols(out_col), _ptr(col_scale),
                _ptr(params), _ptr(X), N, int(n_res), flags, _ptr(term_sums), _ptr(col_sums), _ptr(grad), C.byref(st))
        with self._guard():
            tail = (_ptr(ws), ws.numel(), self._stream())
            if lrs is None:
                rc = self.lib.pinn_ensemble_adam_step(*head, *tail)
            else:
                rc = self.lib.pinn_ensemble_adam_loop(*head, len(lrs), (C.c_double * len(lrs))(*lrs), *tail)
        if self._unsupported(rc, "pinn_ensemble_adam_step" if lrs is None else "pinn_ensemble_adam_loop"):
            return False
        self._ens_packed_tok = _packed_token(ws, params, params_token, req)
        return True

    # ---- the ensemble's device-resident L-BFGS loop (pinn_ensemble_lbfgs_loop) ------------------------------------------
    def ensemble_lbfgs_loop_query(self, M: int, N: int, history_size: int) -> Tuple[int, int]:
        """(workspace bytes, state bytes) of ensemble_lbfgs_loop for M members on N points with this history size
        (pinn_ensemble_query_lbfgs_loop).  Raises PinnError with the engine's reason where the ensemble calls are refused."""
        ws, st = C.c_int64(), C.c_int64()
        with self._guard():
            check(self.lib.pinn_ensemble_query_lbfgs_loop(C.byref(self._d()), int(M), int(N), int(history_size), C.byref(ws),
                                                          C.byref(st)), "pinn_ensemble_query_lbfgs_loop")
        return ws.value, st.value

    def ensemble_lbfgs_loop_init(self, state: torch.Tensor, M: int, lr, max_iter, max_eval, history_size, tolerance_grad,
                                 tolerance_change):
        """Zeroes `state` (uint8, at least the query's state bytes) and arms its M control blocks, one set of options
        for all members (pinn_ensemble_lbfgs_loop_init)."""
        o = _lib.PinnLbfgsOpts(float(lr), float(tolerance_grad), float(tolerance_change), int(max_iter), int(max_eval),
                               int(history_size))
        self._run("pinn_ensemble_lbfgs_loop_init", self.lib.pinn_ensemble_lbfgs_loop_init, _ptr(state), state.numel(), int(M),
                  self.n_params, C.byref(o))

    def ensemble_lbfgs_loop(self, spec: ResidualSpec, term_scale, params, X, n_res: int, loss_rows: torch.Tensor, total_row: int,
                            history_size: int, state: torch.Tensor, n_slots: int, trace: Optional[torch.Tensor] = None,
                            T: Optional[torch.Tensor] = None, out_col: Sequence[int] = (), col_scale=None,
                            ws: Optional[torch.Tensor] = None):
        """n_slots slots of the device-resident L-BFGS loop of M networks (pinn_ensemble_lbfgs_loop): lbfgs_loop's slot for
        every member — its own line search, ring and stopping tests — in one schedule of launches.  params (M, P): row j
        holds member j's accepted iterate whenever the enqueued work has run.  X (N, d_in) or (M, N, d_in), T (rows, nc)
        or (M, rows, nc), n_res, out_col and the scales as ensemble_loss_grad; loss_rows, total_row as lbfgs_loop, shared;
        history_size the one `state` was initialised with; trace (n_slots, M, LBFGS_TRACE_COLS) float64, optional.  Like
        every other call it leaves no packed weights to trust: an ensemble_adam_step after it packs again."""
        spec.first_order("ensemble_lbfgs_loop")
        if params.dim() != 2:
            raise PinnError(f"params must be (M, {self.n_params}), got {tuple(params.shape)}")
        M, nc = params.shape[0], len(out_col)
        own_x = X.dim() == 3
        N = X.shape[1] if own_x else X.shape[0]
        self._chk(params, "params", (M, self.n_params))
        self._chk(X, "X", (M, N, self.desc.d_in) if own_x else (N, self.desc.d_in))
        self._chk(term_scale, "term_scale", (spec.n_terms,))
        self._chk(loss_rows, "loss_rows", (loss_rows.shape[0], nc + spec.n_terms))
        flags = _lib.ENSEMBLE_OWN_X if own_x else 0
        if nc:
            self._chk(col_scale, "col_scale", (nc,))
            if n_res != N:
                rows = N - n_res if n_res >= 0 else N
                if T is not None and T.dim() == 3:
                    flags |= _lib.ENSEMBLE_OWN_T
                    self._chk(T, "T", (M, rows, nc))
                else:
                    self._chk(T, "T", (rows, nc))
        if trace is not None and (trace.dtype != torch.float64 or not trace.is_contiguous()
                                  or tuple(trace.shape) != (n_slots, M, _lib.LBFGS_TRACE_COLS) or trace.device != params.device):
            raise PinnError(f"trace must be a contiguous float64 ({n_slots}, {M}, {_lib.LBFGS_TRACE_COLS}) tensor on {params.device}")
        if state.dtype != torch.uint8 or not state.is_contiguous() or state.device != params.device:
            raise PinnError("state must be a contiguous uint8 tensor on the engine's device")
        if ws is None:
            ws = self.ensemble_workspace(M, N)
        self._run("pinn_ensemble_lbfgs_loop", self.lib.pinn_ensemble_lbfgs_loop, C.byref(self._d()), C.byref(spec.c_struct()), M,
                  _ptr(term_scale), _ptr(T), nc, _out_cols(out_col), _ptr(col_scale), _ptr(params), _ptr(X), N, int(n_res), flags,
                  loss_rows.shape[0], _ptr(loss_rows), int(total_row), int(history_size), _ptr(state), state.numel(),
                  int(n_slots), _ptr(trace), _ptr(ws), ws.numel())

    def last_error(self) -> str:
        """The library's message for the last refused or failed call of this thread (pinn_last_error)."""
        msg = self.lib.pinn_last_error()
        return msg.decode() if msg else ""

    def invalidate_packed(self):
        """Forget the packed copy of the parameters left in the workspace by loss_grad_adam_step: the next call re-packs.
        For writers torch's version counters cannot see (a `.data` view written in place, a raw pointer)."""
        self._packed_tok = None
        self._ens_packed_tok = None

    def adam_step(self, params, grad, m, v, step: int, lr: float, beta1=0.9, beta2=0.999, eps=1e-8, count: Optional[int] = None):
        """torch.optim.Adam.step on the flat parameter vector; count: the length of another flat vector to update instead
        (the trainer's closure coefficients: same kernel, same step count)."""
        n = self.n_params if count is None else int(count)
        for t, nme in ((params, "params"), (grad, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
            self._chk(t, nme, (n,))
        self._run("pinn_adam_step", self.lib.pinn_adam_step, _ptr(params), _ptr(grad), _ptr(m), _ptr(v), n, step, lr, beta1,
                                      beta2, eps)

