"""Shared inputs of the L-BFGS recursion tests (tests/test_lbfgs_cpu.py, tests/test_lbfgs_gpu.py): the synthetic
(s, y) families and a replay of torch.optim.LBFGS's own history, one iteration per `.step`."""
import torch

BAR = 5e-6          # device direction / M-entry bar: ~10x the fp32 torch-operator formulation's own error


def rel_l2(a, b):
    """|a - b| / |b| in float64 (b: the reference)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def synthetic_pair(family, P, gen):
    """One (s, y, g) of the synthetic families, fp32 on the CPU: s = 1e-2 randn, y = s c (0.5 + rand) + 1e-3 randn with
    c = 1 ("well") or c = 10^U(-2, 2) per coordinate ("spread"), redrawn until y.s > 1e-10 (torch.optim.LBFGS stores
    no other pair); g = randn."""
    while True:
        s = torch.randn(P, generator=gen) * 1e-2
        c = 1.0 if family == "well" else 10.0 ** (torch.rand(P, generator=gen) * 4 - 2)
        y = s * c * (0.5 + torch.rand(P, generator=gen)) + 1e-3 * torch.randn(P, generator=gen)
        if float(y.double().dot(s.double())) > 1e-10 and float(y.dot(s)) > 1e-10:
            return s, y, torch.randn(P, generator=gen)


def check_points(m, pushes):
    """Pushes (1-based) after which a case is checked: the first, k = m-1, k = m before the wrap, the first
    overwrite, the last, and every 37th in between."""
    pts = {1, m - 1, m, m + 1, pushes} | set(range(37, pushes, 37))
    return sorted(p for p in pts if 1 <= p <= pushes)


def m_entry_error(M, phys_s, phys_y):
    """max over the used rows and columns of |M_ij - s_i . y_j| / (|s_i| |y_j|), the product in fp64; phys_s, phys_y:
    the fp32 rows in PHYSICAL order (rows 0 .. k-1 of the ring)."""
    Sp, Yp = torch.stack(phys_s).double(), torch.stack(phys_y).double()
    k = Sp.shape[0]
    ref = Sp @ Yp.t()
    scale = Sp.norm(dim=1).unsqueeze(1) * Yp.norm(dim=1).unsqueeze(0)
    return float(((M.detach().cpu()[:k, :k] - ref).abs() / scale).max())


def run_case(make_history, device, m, P, pushes, family, seed, points=None, check_M=False):
    """Pushes `pushes` synthetic pairs into make_history(m, zeros(P)) and, after each push in `points` (default:
    check_points), compares direction(g, H = y.s / y.y) with oracle.lbfgs_two_loop on the fp32 values the history
    received, and (check_M: the history keeps a ring that starts at slot 0 and its M, as _HipHistory does) M with
    the fp64 products of the rows in physical order.  Returns (worst direction error, worst M-entry error or None, number of points checked)."""
    from oracle import pinn_oracle as O
    gen = torch.Generator().manual_seed(seed)
    hist = make_history(m, torch.zeros(P, dtype=torch.float32, device=device))
    points = set(check_points(m, pushes) if points is None else points)
    rows_s, rows_y = [], []
    worst_d, worst_m = 0.0, None
    for n in range(1, pushes + 1):
        s, y, g = synthetic_pair(family, P, gen)
        rows_s.append(s); rows_y.append(y)
        del rows_s[:-m], rows_y[:-m]
        hist.push(s.to(device), y.to(device))
        if n not in points:
            continue
        H = float(y.double().dot(s.double()) / y.double().dot(y.double()))
        ref = O.lbfgs_two_loop(torch.stack(rows_s), torch.stack(rows_y), g, H)
        worst_d = max(worst_d, rel_l2(hist.direction(g.to(device), H), ref))
        if check_M:
            # after n pushes the ring (started at slot 0) holds push j (0-based) in row j % m
            first = n - len(rows_s)
            phys_s, phys_y = [None] * len(rows_s), [None] * len(rows_s)
            for j in range(first, n):
                phys_s[j % m], phys_y[j % m] = rows_s[j - first], rows_y[j - first]
            worst_m = max(worst_m or 0.0, m_entry_error(hist.M, phys_s, phys_y))
    return worst_d, worst_m, len(points)


# ---------------------------------------------------------------------------------------------------------------------
# A real trajectory.  Chained Rosenbrock valleys with an uneven scaling: smooth, not quadratic, and far from converged
# after 170 quasi-Newton iterations, so the history fills to 100 and keeps rolling.

REPLAY_P, REPLAY_STEPS, REPLAY_MIN_PAIRS = 300, 170, 130


def replay_loss(x):
    a = torch.linspace(0.5, 3.0, x.numel() - 1, dtype=x.dtype)
    return (a * (x[1:] - x[:-1] ** 2) ** 2).sum() * 10 + ((1 - x[:-1]) ** 2).sum()


def torch_lbfgs_replay(steps=REPLAY_STEPS, P=REPLAY_P):
    """Drives torch.optim.LBFGS (float64, history 100, strong Wolfe, tolerances 0) one iteration per `.step` and
    yields after each one a dict: S, Y (lists, oldest first: torch's old_stps / old_dirs), g (prev_flat_grad), H
    (H_diag), d (torch's own direction), new (the pair stored by this step, or None) and stored (pairs stored so far)."""
    gen = torch.Generator().manual_seed(11)
    x = torch.nn.Parameter(-1.2 + 0.4 * torch.rand(P, generator=gen, dtype=torch.float64))
    opt = torch.optim.LBFGS([x], lr=1.0, max_iter=1, max_eval=25, history_size=100, tolerance_grad=0.0,
                            tolerance_change=0.0, line_search_fn="strong_wolfe")

    def closure():
        opt.zero_grad()
        loss = replay_loss(x)
        loss.backward()
        return loss

    last, stored = None, 0
    for it in range(steps):
        opt.step(closure)
        st = opt.state[x]
        S, Y = st.get("old_stps") or [], st.get("old_dirs") or []
        new = None
        if Y and Y[-1] is not last:
            last, stored = Y[-1], stored + 1
            new = (S[-1], Y[-1])
        yield dict(it=it, S=list(S), Y=list(Y), g=st["prev_flat_grad"].clone(), H=float(st["H_diag"]), d=st["d"].clone(),
                   new=new, stored=stored)
