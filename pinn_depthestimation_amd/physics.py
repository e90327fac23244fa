"""physics — drop-in for the reference's physics.py: same function names, argument order and
return value (a 0-dim loss tensor that supports .backward() and .item()).

Each residual first tries the FUSED path: if its arguments are the input columns and the
output columns of one DNN.forward call (what train.py:144-154 / train_newmethod.py:122-156
pass), the whole loss and d loss / d theta come from one pinn_residual_loss_grad kernel.
Otherwise it evaluates the same formulas through compute_gradient, whose derivatives come
from the forward-mode jet (autograd.py) — still the HIP engine, never a CPU path.
compute_gradient nests once: compute_gradient(compute_gradient(u, x), y) comes from the
second-order jet (pinn_forward_jet2); a third derivative raises PinnError.
"""
from __future__ import annotations

import math

import torch

from ._lib import PinnError
from .autograd import fused_residual


def compute_gradient(pred, var):
    """d pred / d var per collocation point, differentiable w.r.t. the network parameters
    (reference physics.py:6-15).  Applied to its own result it gives second derivatives (u_xx, u_xy),
    still differentiable w.r.t. the parameters; applied a third time it raises PinnError."""
    (grad,) = torch.autograd.grad(pred, var, grad_outputs=torch.ones_like(pred),
                                  retain_graph=True, create_graph=True)
    return grad


def _mean_sq(*fields):
    total = 0
    for f in fields:
        total = total + torch.mean(f ** 2)
    return total


def _continuity_field(x, y, h, U, V):
    # mass flux divergence d(hU)/dx + d(hV)/dy  (physics.py:20-23, 39-42)
    return compute_gradient(h * U, x) + compute_gradient(h * V, y)


def continuity_only(x, y, h, U, V):
    """physics.py:18-33 — continuity plus the depth anchor h = 0.75 where x < 25.5."""
    fused = fused_residual("continuity_only", (x, y), (h, U, V))
    if fused is not None:
        return fused
    fc = _continuity_field(x, y, h, U, V)
    sel = torch.where(x < 25.5)
    return torch.mean(fc ** 2) + torch.mean((h[sel] - 0.75) ** 2)


def continuity_ftemp(x, y, h, U, V):
    """physics.py:37-47"""
    fused = fused_residual("continuity_ftemp", (x, y), (h, U, V))
    if fused is not None:
        return fused
    return _mean_sq(_continuity_field(x, y, h, U, V))


def _laplacian(a, x, y):
    d = compute_gradient
    return d(d(a, x), x) + d(d(a, y), y)


def Navier_Stokes(t, x, y, h, z, u, v, nu=0.0, gamma_b=None):
    """physics.py:50-88 — unsteady shallow-water continuity + x/y momentum with the
    wave-breaking force 3/16 g gamma_b^2 d(h+z)/dx (h+z); friction terms are zero.

    nu > 0 (an extension, not reference behaviour) adds lateral mixing, -nu (u_xx + u_yy) and -nu (v_xx + v_yy), to the two
    momentum equations.  The derivatives are with respect to the network's inputs as it sees them: in the reference's
    pipeline those are normalised to [-1, 1], so nu is in those units.  Where the arguments are the columns of one
    DNN.forward call the term is hard-wired (pinn_residual2_loss_grad); otherwise nested compute_gradient evaluates it.

    gamma_b (an extension too): the breaker index, a float or a tensor, in place of the reference's 0.78.  When given, the
    formula below runs with that value (the forward jet and the parameter gradient still on the engine) and, for a tensor
    that requires grad, torch autograd supplies d loss / d gamma_b.  The kernel-speed route for a trainable gamma_b is
    Engine.residual_coef_loss_grad (trainer.PINN(trainable_coefficients=("gamma_b",)))."""
    if gamma_b is None:
        fused = fused_residual("Navier_Stokes", (t, x, y), (h, z, u, v), nu=nu)
        if fused is not None:
            return fused
    d = compute_gradient
    depth = h + z
    g = 9.81
    if gamma_b is None:
        gamma_b = 0.78
    cb = 3.0 / 16.0 * g * gamma_b ** 2
    mass = d(z, t) + d(depth * u, x) + d(depth * v, y)
    mom_x = d(u, t) + u * d(u, x) + v * d(u, y) + g * d(z, x) + cb * d(depth, x) * depth
    mom_y = d(v, t) + u * d(v, x) + v * d(v, y) + g * d(z, y) + cb * d(depth, y) * depth
    if nu != 0:
        mom_x = mom_x - nu * _laplacian(u, x, y)
        mom_y = mom_y - nu * _laplacian(v, x, y)
    return _mean_sq(mass, mom_x, mom_y)


def physics_equation(x, y, h, U, V, eta_mean, Hrms, k, corrected=False, nu=0.0, Cd=None, wave_omega=None, wave_gamma=0.42):
    """physics.py:91-120 — steady wave-averaged continuity + momentum with quadratic bottom
    friction.  Default is bug-compatible: the reference's E = 1/8**rho*g*Hrms**2 (physics.py:106)
    is exactly 0.0, so the radiation-stress gradients vanish and Hrms, k do not enter.

    corrected=True (an extension, not reference behaviour) evaluates what the line evidently
    meant, E = 1/8 * rho * g * Hrms**2, with Sxx = E (2kh/sinh(2kh) + 1/2), Syy = E kh/sinh(2kh)
    (physics.py:107-109); it is written with compute_gradient like any user residual: the forward jet and the
    parameter gradient (pinn_jet_backward) both run on the MFMA tile kernel, torch autograd evaluates the formula between.

    nu > 0 (an extension as well) adds lateral mixing, -nu (U_xx + U_yy) and -nu (V_xx + V_yy), to the two momentum
    equations, plain or corrected: the standard closure of the wave-averaged balance.  nu is in the units of the network's
    inputs (normalised to [-1, 1] in the reference's pipeline).  Hard-wired (pinn_residual2_loss_grad) where the arguments
    are the columns of one DNN.forward call, nested compute_gradient otherwise.

    Cd (an extension too): the drag coefficient, a float or a tensor, in place of the reference's 0.002.  When given, the
    formula below runs with that value and, for a tensor that requires grad, torch autograd supplies d loss / d Cd; the
    kernel-speed route is Engine.residual_coef_loss_grad (trainer.PINN(trainable_coefficients=("Cd",))).

    wave_omega (an extension, with corrected=True only): the wave closure — two more terms that tie k and Hrms to the depth,
    at the waves' angular frequency omega (rad/s) and the breaker index wave_gamma, with s = k h:
        f_d = g k tanh(s) / omega^2 - 1                                    (linear dispersion, dimensionless)
        f_E = d/dx (Hrms^2 c_g) + eps,   c_g = (omega / k) (1/2 + s / sinh 2s)
        eps = (3 sqrt(pi) / 2) (omega / 2 pi) Hrms^5 / (gamma^2 h^3) [1 - (1 + (Hrms / (gamma h))^2)^(-5/2)]
    (wave-energy flux balance divided by rho g / 8; dissipation of Thornton & Guza 1983 with B = 1; waves travel along +x,
    as the residual's Sxy = 0 has it).  k > 0 and h > 0 are the caller's to ensure.  This function evaluates them through
    compute_gradient like any user residual; physics_equation_wave is the hard-wired route."""
    if wave_omega is not None:
        if not corrected:
            raise PinnError("wave_omega is the wave closure of physics_equation(corrected=True): the dispersion and "
                            "wave-energy terms close the corrected radiation stress")
        if nu != 0 or Cd is not None:
            raise PinnError("the wave closure (wave_omega) has no form with nu or Cd")
        if not (wave_omega > 0 and wave_gamma > 0):
            raise PinnError(f"the wave closure needs wave_omega > 0 and wave_gamma > 0 (got {wave_omega}, {wave_gamma})")
    if Cd is not None:
        pass      # the formula route: the hard-wired kernels carry the constant
    elif nu != 0:
        fused = fused_residual("physics_equation", (x, y), (h, U, V, eta_mean, Hrms, k), corrected=corrected, nu=nu)
        if fused is not None:
            return fused
    elif not corrected:
        fused = fused_residual("physics_equation", (x, y), (h, U, V, eta_mean, Hrms, k))
        if fused is not None:
            return fused
    d = compute_gradient
    g, rho, cd = 9.81, 1025, (0.002 if Cd is None else Cd)
    inv_depth = 1 / (rho * (eta_mean + h))
    mass = d(U, x) + d(V, y)
    mom_x = U * d(U, x) + V * d(U, y) + g * d(eta_mean, x) + inv_depth * (rho * cd * U * abs(U))
    mom_y = U * d(V, x) + V * d(V, y) + g * d(eta_mean, y) + inv_depth * (rho * cd * V * abs(V))
    if corrected:
        E = (1.0 / 8.0) * rho * g * Hrms ** 2
        ratio = k * h / torch.sinh(2 * k * h)
        mom_x = mom_x + inv_depth * d(E * (2 * ratio + 0.5), x)
        mom_y = mom_y + inv_depth * d(E * ratio, y)
    if nu != 0:
        mom_x = mom_x - nu * _laplacian(U, x, y)
        mom_y = mom_y - nu * _laplacian(V, x, y)
    if wave_omega is not None:
        s = k * h
        disp = g * k * torch.tanh(s) / wave_omega ** 2 - 1
        cg = (wave_omega / k) * (0.5 + s / torch.sinh(2 * s))
        q = Hrms / (wave_gamma * h)
        eps = (1.5 * math.sqrt(math.pi)) * (wave_omega / (2 * math.pi)) * Hrms ** 5 / (wave_gamma ** 2 * h ** 3) \
            * (1 - (1 + q ** 2) ** (-2.5))
        energy = d(Hrms ** 2 * cg, x) + eps
        return _mean_sq(mass, mom_x, mom_y, disp, energy)
    return _mean_sq(mass, mom_x, mom_y)


def physics_equation_corrected(x, y, h, U, V, eta_mean, Hrms, k):
    """physics_equation(..., corrected=True) hard-wired: where the arguments are the input and output columns of one
    DNN.forward call (and the engine serves it: tanh, width <= 64), loss and d loss / d theta come from ONE kernel with
    the corrected radiation stress in its epilogue (ResidualSpec.corrected) instead of forward jet + torch autograd +
    jet_backward.  Otherwise the formula itself, physics_equation(..., corrected=True): the same loss.  One difference:
    at kh = 0 the kernels take the limit of kh / sinh 2kh and its derivatives, where the formula gives NaN."""
    fused = fused_residual("physics_equation", (x, y), (h, U, V, eta_mean, Hrms, k), corrected=True)
    if fused is not None:
        return fused
    return physics_equation(x, y, h, U, V, eta_mean, Hrms, k, corrected=True)


def physics_equation_wave(x, y, h, U, V, eta_mean, Hrms, k, omega, gamma=0.42):
    """physics_equation(..., corrected=True, wave_omega=omega, wave_gamma=gamma) hard-wired: where the arguments are the
    input and output columns of one DNN.forward call (and the engine serves it: tanh, width <= 64), the five-term loss and
    d loss / d theta come from ONE kernel with the wave closure in its epilogue (ResidualSpec.wave_omega).  Otherwise the
    formula itself: the same loss.  One difference: at kh -> 0 the kernels take the limits of kh / sinh 2kh and tanh kh
    from their series, where the formula loses digits (and gives NaN at kh = 0)."""
    if not (omega > 0 and gamma > 0):
        raise PinnError(f"the wave closure needs omega > 0 and gamma > 0 (got {omega}, {gamma})")
    fused = fused_residual("physics_equation", (x, y), (h, U, V, eta_mean, Hrms, k), corrected=True, wave_omega=omega,
                           wave_gamma=gamma)
    if fused is not None:
        return fused
    return physics_equation(x, y, h, U, V, eta_mean, Hrms, k, corrected=True, wave_omega=omega, wave_gamma=gamma)
