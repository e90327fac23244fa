"""ctypes binding of libpinn_hip.so (include/pinn_hip.h).  No torch extension headers,
no pybind: the shared library is a plain C-ABI and this file is the whole binding."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PINN_HIP_LIB", os.path.join(_HERE, "libpinn_hip.so"))  # override: kernel experiments
CSRC = os.path.join(_HERE, "csrc")

PINN_MAX_DIRS = 3
PINN_MAX_ROLES = 8
PINN_MAX_COEFS = 4

ACT_TANH, ACT_LEAKY_RELU = 0, 1
ACT_SIN_TANH = 2      # sine on the first hidden layer, tanh on the others (pinn_hip.h: PINN_ACT_SIN_TANH)
ENGINE_AUTO, ENGINE_GENERIC, ENGINE_FUSED, ENGINE_WIDE = 0, 1, 2, 3
ENGINE_FUSED_TILE, ENGINE_FUSED_COOP, ENGINE_FUSED_BATCH = 4, 5, 6     # sub-values of ENGINE_FUSED: force one of its kernels (pinn_hip.h)
ABI_VERSION = 4
PREC_F32, PREC_BF16 = 0, 1

RES_NAVIER_STOKES, RES_PHYSICS_EQUATION, RES_CONTINUITY_FTEMP, RES_CONTINUITY_ONLY = 1, 2, 3, 4
RES_TERMS = {RES_NAVIER_STOKES: 3, RES_PHYSICS_EQUATION: 3, RES_CONTINUITY_FTEMP: 1, RES_CONTINUITY_ONLY: 3}
PEW_TERMS = 5      # pinn_hip.h: PINN_PEW_TERMS, the terms and fields of physics_equation with the wave closure (flags = 3)
RES_COEFS = {RES_NAVIER_STOKES: ("gamma_b",), RES_PHYSICS_EQUATION: ("Cd",), RES_CONTINUITY_FTEMP: (), RES_CONTINUITY_ONLY: ()}   # pinn_residual_coef_*: names, in coef[] order
RES_FIELDS = {RES_NAVIER_STOKES: 3, RES_PHYSICS_EQUATION: 3, RES_CONTINUITY_FTEMP: 2, RES_CONTINUITY_ONLY: 2}   # pinn_residual_fields' rows


class PinnDesc(C.Structure):
    _fields_ = [
        ("d_in", C.c_int32), ("d_out", C.c_int32), ("n_hidden", C.c_int32), ("width", C.c_int32),
        ("k", C.c_int32), ("dir_col", C.c_int32 * PINN_MAX_DIRS),
        ("activation", C.c_int32), ("engine", C.c_int32), ("precision", C.c_int32),
        ("dropout_p", C.c_float), ("dropout_seed", C.c_uint32),
    ]


class PinnResidualSpec(C.Structure):
    _fields_ = [
        ("residual_id", C.c_int32), ("out_col", C.c_int32 * PINN_MAX_ROLES),
        ("dir_of", C.c_int32 * PINN_MAX_DIRS), ("flags", C.c_int32), ("param", C.c_float * 4),
    ]


class PinnAdamState(C.Structure):
    _fields_ = [
        ("m", C.c_void_p), ("v", C.c_void_p), ("step", C.c_int64), ("lr", C.c_double), ("beta1", C.c_double),
        ("beta2", C.c_double), ("eps", C.c_double), ("packed_valid", C.c_int32), ("n_loss_rows", C.c_int32),
        ("loss_rows", C.c_void_p), ("losses", C.c_void_p),
    ]


class PinnAdamExtras(C.Structure):
    """pinn_adam_extras (pinn_adam_loop_ext): the coefficient group or the weight group, the other left NULL."""
    _fields_ = [
        ("coef", C.c_void_p), ("coef_m", C.c_void_p), ("coef_v", C.c_void_p), ("coef_grad", C.c_void_p),
        ("coef_mask", C.c_void_p), ("coef_log", C.c_void_p),
        ("point_w", C.c_void_p), ("w_rows", C.c_int32), ("fields", C.c_void_p),
        ("lam", C.c_void_p), ("lam_m", C.c_void_p), ("lam_v", C.c_void_p), ("sa_mask", C.c_int32),
    ]


class PinnBalance(C.Structure):
    """pinn_balance (pinn_adam_loop_balanced): the rule, the two device weights [residual, fidelity] and the optional logs."""
    _fields_ = [
        ("mode", C.c_int32), ("every", C.c_int32), ("ref", C.c_int32), ("alpha", C.c_double),
        ("lam", C.c_void_p), ("lam_log", C.c_void_p), ("stats_log", C.c_void_p), ("group_grads", C.c_void_p),
    ]


BALANCE_NONE, BALANCE_MAX_MEAN, BALANCE_NORM = 0, 1, 2      # pinn_hip.h: PINN_BALANCE_*
BALANCE_MODES = {None: BALANCE_NONE, "none": BALANCE_NONE, "max_mean": BALANCE_MAX_MEAN, "norm": BALANCE_NORM}
BALANCE_MAX_GROUPS, BALANCE_STATS = 8, 3


class PinnLsState(C.Structure):
    """pinn_ls_state: torch's _strong_wolfe as a resumable state machine (csrc/lbfgs_line_search.h)."""
    _fields_ = [
        ("f0", C.c_double), ("gtd0", C.c_double), ("d_norm", C.c_double), ("t", C.c_double),
        ("t_prev", C.c_double), ("f_prev", C.c_double), ("gtd_prev", C.c_double),
        ("br_t", C.c_double * 2), ("br_f", C.c_double * 2), ("br_gtd", C.c_double * 2),
        ("t_acc", C.c_double), ("f_acc", C.c_double),
        ("phase", C.c_int32), ("ls_iter", C.c_int32), ("max_ls", C.c_int32), ("n_evals", C.c_int32),
        ("low_pos", C.c_int32), ("high_pos", C.c_int32), ("insuf_progress", C.c_int32), ("br_n", C.c_int32),
        ("g_prev_slot", C.c_int32), ("br_slot", C.c_int32 * 2), ("g_slot_for_new", C.c_int32), ("g_acc_slot", C.c_int32),
    ]


class PinnLbfgsOpts(C.Structure):
    _fields_ = [("lr", C.c_double), ("tolerance_grad", C.c_double), ("tolerance_change", C.c_double),
                ("max_iter", C.c_int32), ("max_eval", C.c_int32), ("history_size", C.c_int32)]


class PinnLbfgsCtrl(C.Structure):
    """pinn_lbfgs_ctrl: the first bytes of the device L-BFGS loop's state."""
    _fields_ = [
        ("phase", C.c_int32), ("done", C.c_int32), ("reason", C.c_int32), ("action", C.c_int32),
        ("head", C.c_int32), ("k", C.c_int32), ("slot", C.c_int32), ("m", C.c_int32),
        ("n_iter", C.c_int32), ("n_evals", C.c_int32), ("max_iter", C.c_int32), ("max_eval", C.c_int32),
        ("push", C.c_int32), ("file_row", C.c_int32), ("acc_row", C.c_int32), ("n_slots", C.c_int32),
        ("P", C.c_int64),
        ("t", C.c_double), ("f", C.c_double), ("gtd", C.c_double), ("d_norm", C.c_double), ("H", C.c_double),
        ("f_prev", C.c_double), ("t_acc", C.c_double), ("gmax", C.c_double),
        ("lr", C.c_double), ("tolerance_grad", C.c_double), ("tolerance_change", C.c_double),
        ("ls", PinnLsState),
    ]


LS_EVALUATE, LS_DONE, LS_POOL_ROWS = 0, 1, 4
LBFGS_ACT_INERT, LBFGS_ACT_CONTINUE, LBFGS_ACT_ACCEPT, LBFGS_ACT_INITIAL = 0, 1, 2, 3
LBFGS_STOP_REASONS = {0: None, 1: "gradient", 2: "step", 3: "loss change", 4: "max_iter", 5: "max_eval", 6: "direction"}
LBFGS_TRACE_COLS = 18


def _a256(v: int) -> int:
    return (int(v) + 255) // 256 * 256


def ensemble_lbfgs_ctrl_stride() -> int:
    """Bytes from one member's control block to the next in the ensemble L-BFGS state (pinn_hip.h)."""
    return _a256(C.sizeof(PinnLbfgsCtrl))


def ensemble_lbfgs_state_bytes(M: int, P: int, history_size: int) -> int:
    """pinn_ensemble_query_lbfgs_loop's state_bytes by the formula pinn_hip.h documents."""
    a, m = _a256, int(history_size)
    member = a(4 * LS_POOL_ROWS * P) + 4 * a(4 * P) + a(8 * 256 * 8) + a(32) + a(8 * 4 * 256) + a(4 * 2 * 256) \
        + 2 * a(4 * m * P) + a(8 * m * m)
    return M * ensemble_lbfgs_ctrl_stride() + 3 * a(4 * M * P) + 2 * a(4 * M * PINN_MAX_ROLES) + M * member

ERR_INVALID, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -2, -3


class PinnError(RuntimeError):
    pass


_P = C.c_void_p
_SIGNATURES = {
    "pinn_version": (C.c_int32, []),
    "pinn_last_error": (C.c_char_p, []),
    "pinn_dropout_keep": (C.c_int32, [C.c_uint32, C.c_int32, C.c_int32, C.c_int64, C.c_float]),
    "pinn_pe_corrected_point": (C.c_int32, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "pinn_pe_wave_point": (C.c_int32, [C.POINTER(C.c_float), C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                       C.POINTER(C.c_float)]),
    "pinn_param_count": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(C.c_int64)]),
    "pinn_query_workspace": (C.c_int32, [C.POINTER(PinnDesc), C.c_int64, C.POINTER(C.c_int64)]),
    "pinn_forward": (C.c_int32, [C.POINTER(PinnDesc), _P, _P, C.c_int64, _P, _P, C.c_int64, _P]),
    "pinn_forward_jet": (C.c_int32, [C.POINTER(PinnDesc), _P, _P, C.c_int64, _P, _P, _P, C.c_int64, _P]),
    "pinn_jet_backward": (C.c_int32, [C.POINTER(PinnDesc), _P, _P, C.c_int64, _P, _P, _P, _P, C.c_int64, _P]),
    "pinn_jet_backward_kernel": (C.c_int32, [C.POINTER(PinnDesc), C.c_int64, C.c_int32, C.POINTER(C.c_int32)]),
    "pinn_query_jet2_workspace": (C.c_int32, [C.POINTER(PinnDesc), C.c_int64, C.POINTER(C.c_int64)]),
    "pinn_forward_jet2": (C.c_int32, [C.POINTER(PinnDesc), _P, _P, C.c_int64, _P, _P, _P, _P, C.c_int64, _P]),
    "pinn_jet2_backward": (C.c_int32, [C.POINTER(PinnDesc), _P, _P, C.c_int64, _P, _P, _P, _P, _P, C.c_int64, _P]),
    "pinn_residual_loss": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), _P, _P, C.c_int64, _P,
                                       _P, C.c_int64, _P]),
    "pinn_query_fields_workspace": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), C.c_int64, C.POINTER(C.c_int64)]),
    "pinn_residual_fields": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), _P, _P, C.c_int64, _P,
                                         _P, C.c_int64, _P]),
    "pinn_residual2_point": (C.c_int32, [C.c_int32, C.c_int32, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                         C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "pinn_query_residual2_workspace": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), C.c_int64, C.POINTER(C.c_int64)]),
    "pinn_residual2_loss_grad": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), C.c_float, _P, _P, _P,
                                             C.c_int64, _P, _P, _P, _P, C.c_int64, _P]),
    "pinn_residual_coef_count": (C.c_int32, [C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "pinn_residual_coef_default": (C.c_int32, [C.c_int32, C.c_int32, C.POINTER(C.c_float)]),
    "pinn_residual_coef_point": (C.c_int32, [C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                             C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "pinn_query_residual_coef_workspace": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), C.c_int64, C.POINTER(C.c_int64)]),
    "pinn_residual_coef_loss_grad": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), _P, _P, _P, _P,
                                                 C.c_int64, _P, _P, _P, _P, C.c_int64, _P]),
    "pinn_query_residual_weighted_workspace": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), C.c_int64, C.POINTER(C.c_int64)]),
    "pinn_residual_weighted_loss_grad": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), _P, _P, C.c_int32, _P, _P,
                                                     C.c_int64, _P, _P, _P, _P, C.c_int64, _P]),
    "pinn_residual_loss_grad": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), _P, _P, _P,
                                            C.c_int64, _P, _P, _P, C.c_int64, _P]),
    "pinn_mse_loss_grad": (C.c_int32, [C.POINTER(PinnDesc), _P, _P, _P, C.c_int64, C.c_int32,
                                       C.POINTER(C.c_int32), _P, _P, _P, _P, C.c_int64, _P]),
    "pinn_residual_mse_loss_grad": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), _P, _P, C.c_int32,
                                                C.POINTER(C.c_int32), _P, _P, _P, C.c_int64, _P, _P, _P, _P,
                                                C.c_int64, _P]),
    "pinn_residual_mse_split_loss_grad": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), _P, _P, C.c_int32,
                                                      C.POINTER(C.c_int32), _P, _P, _P, C.c_int64, C.c_int64, _P, _P, _P,
                                                      _P, C.c_int64, _P]),
    "pinn_lbfgs_push": (C.c_int32, [_P, _P, _P, C.c_int32, C.c_int64, C.c_int32, _P, _P, _P]),
    "pinn_lbfgs_direction": (C.c_int32, [_P, _P, _P, C.c_int32, C.c_int64, C.c_int32, C.c_int32, _P, C.c_double, _P,
                                         _P, _P, _P, _P]),
    "pinn_lbfgs_ls_init": (C.c_int32, [C.POINTER(PinnLsState), C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32]),
    "pinn_lbfgs_ls_step": (C.c_int32, [C.POINTER(PinnLsState), C.c_double, C.c_double]),
    "pinn_query_lbfgs_loop": (C.c_int32, [C.POINTER(PinnDesc), C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "pinn_lbfgs_loop_init": (C.c_int32, [_P, C.c_int64, C.c_int64, C.POINTER(PinnLbfgsOpts), _P]),
    "pinn_lbfgs_loop": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), _P, _P, C.c_int32, C.POINTER(C.c_int32),
                                    _P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, C.c_int32, _P, C.c_int64, C.c_int32,
                                    _P, _P, C.c_int64, _P]),
    "pinn_ensemble_query_lbfgs_loop": (C.c_int32, [C.POINTER(PinnDesc), C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int64),
                                                   C.POINTER(C.c_int64)]),
    "pinn_ensemble_lbfgs_loop_init": (C.c_int32, [_P, C.c_int64, C.c_int32, C.c_int64, C.POINTER(PinnLbfgsOpts), _P]),
    "pinn_ensemble_lbfgs_loop": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), C.c_int32, _P, _P, C.c_int32,
                                             C.POINTER(C.c_int32), _P, _P, _P, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _P,
                                             C.c_int32, C.c_int32, _P, C.c_int64, C.c_int32, _P, _P, C.c_int64, _P]),
    "pinn_nanminmax_f64": (C.c_int32, [_P, C.c_int64, _P, _P, C.c_int64, _P]),
    "pinn_stage_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "pinn_stage_grid_columns": (C.c_int32, [C.POINTER(_P), C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _P, _P, _P, _P,
                                            C.c_int64, _P]),
    "pinn_adam_step": (C.c_int32, [_P, _P, _P, _P, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_double,
                                   C.c_double, _P]),
    "pinn_loss_grad_adam_step": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), _P, _P, C.c_int32,
                                             C.POINTER(C.c_int32), _P, _P, _P, C.c_int64, C.c_int64, _P, _P, _P,
                                             C.POINTER(PinnAdamState), _P, C.c_int64, _P]),
    "pinn_adam_loop": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), _P, _P, C.c_int32,
                                   C.POINTER(C.c_int32), _P, _P, _P, C.c_int64, C.c_int64, _P, _P, _P,
                                   C.POINTER(PinnAdamState), C.c_int32, C.POINTER(C.c_double), _P, C.c_int64, _P]),
    "pinn_query_adam_ext_workspace": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), C.POINTER(PinnAdamExtras),
                                                  C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    "pinn_adam_loop_ext": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), _P, _P, _P, C.c_int64, C.c_int32,
                                       C.POINTER(C.c_int32), _P, _P, _P, C.c_int64, _P, _P, _P, C.POINTER(PinnAdamState),
                                       C.POINTER(PinnAdamExtras), C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double), _P, C.c_int64, _P]),
    "pinn_balance_weights_host": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int64, C.POINTER(C.c_double),
                                              C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "pinn_query_balance_workspace": (C.c_int32, [C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    "pinn_balance_update": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_double, _P, C.c_int64, C.c_int64, _P, _P, _P,
                                        _P, C.c_int64, _P]),
    "pinn_query_adam_balanced_workspace": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), C.c_int64, C.c_int64,
                                                       C.POINTER(C.c_int64)]),
    "pinn_adam_loop_balanced": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), _P, _P, _P, C.c_int64, C.c_int32,
                                            C.POINTER(C.c_int32), _P, _P, _P, C.c_int64, _P, _P, _P, C.POINTER(PinnAdamState),
                                            C.POINTER(PinnBalance), C.c_int32, C.POINTER(C.c_double), _P, C.c_int64, _P]),
    "pinn_ensemble_query_workspace": (C.c_int32, [C.POINTER(PinnDesc), C.c_int32, C.c_int64, C.POINTER(C.c_int64)]),
    "pinn_ensemble_plan": (C.c_int32, [C.POINTER(PinnDesc), C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "pinn_ensemble_loss_grad": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), C.c_int32, _P, _P, C.c_int32,
                                            C.POINTER(C.c_int32), _P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P,
                                            _P, C.c_int64, _P]),
    "pinn_ensemble_adam_step": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), C.c_int32, _P, _P, C.c_int32,
                                            C.POINTER(C.c_int32), _P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P,
                                            C.POINTER(PinnAdamState), _P, C.c_int64, _P]),
    "pinn_ensemble_adam_loop": (C.c_int32, [C.POINTER(PinnDesc), C.POINTER(PinnResidualSpec), C.c_int32, _P, _P, C.c_int32,
                                            C.POINTER(C.c_int32), _P, _P, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P,
                                            C.POINTER(PinnAdamState), C.c_int32, C.POINTER(C.c_double), _P, C.c_int64, _P]),
}
ENSEMBLE_OWN_X, ENSEMBLE_OWN_T, ENSEMBLE_MAX_MEMBERS = 1, 2, 65535      # pinn_hip.h: PINN_ENSEMBLE_*

_lib = None


def build(verbose: bool = False) -> str:
    """Compile libpinn_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    out = subprocess.run(["make", "-C", CSRC, "-j4"], capture_output=True, text=True)
    if verbose or out.returncode != 0:
        print(out.stdout[-4000:])
        print(out.stderr[-4000:])
    if out.returncode != 0:
        raise PinnError("building libpinn_hip.so failed (see output above)")
    return LIB_PATH


def load():
    """Load the HIP library.  There is no CPU fallback: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PinnError(
            f"{LIB_PATH} is missing: the MI355X engine has not been built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (or `make -C "
            f"{CSRC}`) first; this package has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.pinn_version() != ABI_VERSION:
        raise PinnError(f"{LIB_PATH} has ABI version {lib.pinn_version()}, this package binds version {ABI_VERSION}: rebuild it")
    _lib = lib
    return lib


def exported_symbols():
    return list(_SIGNATURES)


def check(rc: int, what: str):
    if rc != 0:
        msg = load().pinn_last_error()
        raise PinnError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")
