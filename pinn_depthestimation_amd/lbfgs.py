"""lbfgs — torch.optim.LBFGS semantics (the optimiser of train.py:116-125, one `.step(closure)`,
train.py:200) with the two-loop recursion done in six matrix-vector products.

torch.optim.LBFGS walks its history with two Python loops: at history_size = 100 that is ~400
tiny kernels (dot, axpy) per iteration — 2.3 ms of launches around a 0.15 ms closure at the
reference's problem sizes (measured, tools/lbfgs_latency.py).  The recursion is a pair of
triangular solves in disguise.  With S, Y the (k x P) matrices of steps and gradient
differences (oldest first), M = S Y^T and q0 = -g:

    first loop :  al_i = ro_i (s_i . q_i),  q_{i} = q0 - sum_{j>i} al_j y_j,  ro_i = 1 / M_ii
                  <=>  triu(M) al = S q0
    q  = q0 - Y^T al,           r0 = H q
    second loop:  be_i = ro_i (y_i . r_i),  r_i = r0 + sum_{j<i} (al_j - be_j) s_j
                  <=>  tril(M^T) w = diag(M) al - H (Y q),     w = al - be
    d  = r0 + S^T w

i.e. four (k x P) matrix-vector products, two k x k triangular solves (fp64), and two more
products to extend M when a pair is stored.  On the GPU that is six launches of csrc/pinn_lbfgs.hip
(`_HipHistory`); `_History` is the same formulation in torch operators (CPU, or no library).  Same arithmetic up to summation order; everything else
(memory update rule, step-size initialisation, strong-Wolfe line search, stopping tests, state
counters) is torch.optim.LBFGS's own: this class subclasses it, re-uses its helpers and its
`_strong_wolfe`, and falls back to its `step` when it cannot apply.
"""
from __future__ import annotations

import torch
from torch.optim import LBFGS as _TorchLBFGS

try:                                     # private helper of torch.optim.lbfgs: same line search, same decisions
    from torch.optim.lbfgs import _strong_wolfe
except Exception:                        # pragma: no cover
    _strong_wolfe = None


class _History:
    """(s, y) pairs as two (m x P) matrices, oldest first, plus M = S Y^T in fp64.  Unused rows are zero
    with a unit diagonal in M, so every product and both triangular solves run over the full m without
    gathering; when the history is full the oldest row is rolled out (24 MB of copies at m = 100,
    P = 30 k: cheaper than the index bookkeeping it replaces)."""

    def __init__(self, m: int, like: torch.Tensor):
        self.m, self.k = m, 0
        self.S = torch.zeros(m, like.numel(), dtype=like.dtype, device=like.device)
        self.Y = torch.zeros_like(self.S)
        self.M = torch.eye(m, dtype=torch.float64, device=like.device)

    def push(self, s: torch.Tensor, y: torch.Tensor):
        if self.k == self.m:
            self.S = torch.roll(self.S, -1, 0)
            self.Y = torch.roll(self.Y, -1, 0)
            self.M = torch.roll(self.M, (-1, -1), (0, 1))
            self.k -= 1
        i = self.k
        self.S[i].copy_(s)
        self.Y[i].copy_(y)
        self.M[i, :] = torch.mv(self.Y, s)      # s_new . y_j   (zero beyond the used rows)
        self.M[:, i] = torch.mv(self.S, y)      # s_i . y_new   (M[i, i] = s . y either way)
        self.k += 1

    def direction(self, g: torch.Tensor, H) -> torch.Tensor:
        """-(inverse-Hessian approximation) g by the recursion written as two triangular solves."""
        q0 = g.neg()
        if self.k == 0:
            return q0 * H
        M = self.M
        b = torch.mv(self.S, q0).double()
        al = torch.linalg.solve_triangular(torch.triu(M), b.unsqueeze(1), upper=True).squeeze(1)
        q = torch.addmv(q0, self.Y.t(), al.to(g.dtype), alpha=-1.0)
        c = torch.mv(self.Y, q).double()
        rhs = torch.diagonal(M) * al - c * H
        w = torch.linalg.solve_triangular(torch.tril(M.t()), rhs.unsqueeze(1), upper=False).squeeze(1)
        return torch.addmv(q * H, self.S.t(), w.to(g.dtype))


class _HipHistory:
    """The same history on the device through libpinn_hip.so (csrc/pinn_lbfgs.hip): S, Y are rings
    (no roll), the recursion is six launches (two row-dot passes, two one-wave triangular solves in
    fp64, two combines) instead of ~25 torch operators."""

    def __init__(self, m: int, like: torch.Tensor):
        from . import _lib
        import ctypes
        self._C, self.lib = ctypes, _lib.load()
        self.m, self.k, self.head, self.P = m, 0, 0, like.numel()
        dev = like.device
        self.S = torch.zeros(m, self.P, dtype=torch.float32, device=dev)
        self.Y = torch.zeros_like(self.S)
        self.M = torch.zeros(m, m, dtype=torch.float64, device=dev)
        self.tmp = torch.zeros(4 * m, dtype=torch.float64, device=dev)
        self.coef = torch.zeros(2 * m, dtype=torch.float32, device=dev)
        self.q = torch.empty(self.P, dtype=torch.float32, device=dev)

    def _p(self, t):
        return self._C.c_void_p(t.data_ptr())

    def _check(self, rc, what):
        if rc != 0:
            from ._lib import PinnError
            raise PinnError(f"{what}: {self.lib.pinn_last_error().decode()}")

    def push(self, s: torch.Tensor, y: torch.Tensor):
        if self.k == self.m:
            slot, self.head = self.head, (self.head + 1) % self.m      # overwrite the oldest pair
        else:
            slot = (self.head + self.k) % self.m
            self.k += 1
        s, y = s.contiguous(), y.contiguous()
        st = self._C.c_void_p(torch.cuda.current_stream(s.device).cuda_stream)
        self._check(self.lib.pinn_lbfgs_push(self._p(self.S), self._p(self.Y), self._p(self.M), self.m, self.P, slot,
                                             self._p(s), self._p(y), st), "pinn_lbfgs_push")

    def direction(self, g: torch.Tensor, H) -> torch.Tensor:
        if self.k == 0:
            return g.neg() * H
        g = g.contiguous()
        d = torch.empty_like(g)
        st = self._C.c_void_p(torch.cuda.current_stream(g.device).cuda_stream)
        self._check(self.lib.pinn_lbfgs_direction(self._p(self.S), self._p(self.Y), self._p(self.M), self.m, self.P,
                                                  self.head, self.k, self._p(g), float(H), self._p(d), self._p(self.tmp),
                                                  self._p(self.coef), self._p(self.q), st), "pinn_lbfgs_direction")
        return d


def _make_history(m: int, like: torch.Tensor):
    # fp32 parameters on the GPU (the product path): csrc/pinn_lbfgs.hip, and a missing library is an error, not a
    # reason to run something else.  _History (torch operators) serves CPU tensors and float64 — the CPU tests of the
    # optimizer's semantics against torch.optim.LBFGS — and history sizes beyond the kernels' 256 (the reference: 100).
    if like.is_cuda and like.dtype == torch.float32 and m <= 256:
        return _HipHistory(m, like)
    return _History(m, like)


class FlatLBFGS(_TorchLBFGS):
    """torch.optim.LBFGS over ONE flat parameter tensor with the batched recursion above."""

    @torch.no_grad()
    def step(self, closure):
        group = self.param_groups[0]
        if _strong_wolfe is None or len(self._params) != 1 or group["line_search_fn"] not in (None, "strong_wolfe"):
            return super().step(closure)
        closure = torch.enable_grad()(closure)
        lr, max_iter, max_eval = float(group["lr"]), group["max_iter"], group["max_eval"]
        tol_grad, tol_change = group["tolerance_grad"], group["tolerance_change"]
        line_search, m = group["line_search_fn"], group["history_size"]
        state = self.state[self._params[0]]
        state.setdefault("func_evals", 0)
        state.setdefault("n_iter", 0)

        orig_loss = closure()
        loss = float(orig_loss)
        evals = 1
        state["func_evals"] += 1
        g = self._gather_flat_grad()
        if float(g.abs().max()) <= tol_grad:
            return orig_loss

        d, t = state.get("d"), state.get("t")
        hist: _History = state.get("hist")
        H = state.get("H_diag")
        prev_g, prev_loss = state.get("prev_flat_grad"), state.get("prev_loss")

        n_iter = 0
        pending = None      # (y, s, y.s, y.y) of the step just taken, fetched with the stopping tests' values
        while n_iter < max_iter:
            n_iter += 1
            state["n_iter"] += 1
            if state["n_iter"] == 1:
                d = g.neg()
                hist = _make_history(m, g)
                H = 1.0
            else:
                if pending is None:                                       # (first iteration of a later .step call)
                    y, s = g.sub(prev_g), d.mul(t)
                    pending = (y, s) + tuple(torch.stack((y.dot(s), y.dot(y))).tolist())
                y, s, ys, yy = pending
                pending = None
                if ys > 1e-10:
                    hist.push(s, y)
                    H = ys / yy
                d = hist.direction(g, H)
            if prev_g is None:
                prev_g = g.clone(memory_format=torch.contiguous_format)
            else:
                prev_g.copy_(g)
            prev_loss = loss

            gd = g.dot(d)
            gtd_l1 = torch.stack((gd, g.abs().sum())).tolist()           # one synchronisation for both
            t = min(1.0, 1.0 / gtd_l1[1]) * lr if state["n_iter"] == 1 else lr
            if gtd_l1[0] > -tol_change:
                break

            ls_evals = 0
            if line_search is not None:
                x_init = self._clone_param()

                def obj_func(x, step, direction):
                    return self._directional_evaluate(closure, x, step, direction)

                # The line-search budget is whatever the INSTALLED torch.optim.LBFGS.step gives it: torch 2.10
                # (this image) passes max_ls = max_eval - current_evals; older releases used _strong_wolfe's
                # default of 25.  tests/test_lbfgs_cpu.py::test_line_search_budget_is_torchs compares
                # evaluation counts with torch.optim.LBFGS itself, so a torch upgrade that changes the rule
                # shows up there.
                loss, g, t, ls_evals = _strong_wolfe(obj_func, x_init, t, d, loss, g, gd, max_ls=max_eval - evals)
                self._add_grad(t, d)
            else:
                self._add_grad(t, d)
                if n_iter != max_iter:
                    with torch.enable_grad():
                        loss = float(closure())
                    g = self._gather_flat_grad()
                    ls_evals = 1
            evals += ls_evals
            state["func_evals"] += ls_evals

            if n_iter == max_iter or evals >= max_eval:
                break
            # one synchronisation: the stopping tests' maxima and the next memory update's y.s, y.y
            y, s = g.sub(prev_g), d.mul(t)
            gmax, smax, ys, yy = torch.stack((g.abs().max(), s.abs().max(), y.dot(s), y.dot(y))).tolist()
            pending = (y, s, ys, yy)
            if gmax <= tol_grad:
                break
            if smax <= tol_change:
                break
            if abs(loss - prev_loss) < tol_change:
                break

        state.update(d=d, t=t, hist=hist, H_diag=H, prev_flat_grad=prev_g, prev_loss=prev_loss)
        return orig_loss


class DeviceLBFGS:
    """torch.optim.LBFGS.step(closure) with strong-Wolfe line search, run on the device (Engine.lbfgs_loop,
    pinn_lbfgs_loop): runs of RUN evaluations enqueued by one call, every decision — line search, stopping tests, ring
    bookkeeping, direction — taken by kernels.  Not a torch.optim.Optimizer: there is no closure to call; the loss request
    (point set, scales, loss rows) is fixed at construction.  The host reads the control block once per run and stops
    when the done flag is up.  `params` (the flat fp32 parameter tensor) holds the accepted iterate after every run."""

    RUN = 64

    @staticmethod
    def check_options(lr, max_iter, max_eval, history_size, tolerance_grad, tolerance_change, line_search_fn):
        """The options as torch.optim.LBFGS takes them, or PinnError with what the device loop does not do."""
        from types import SimpleNamespace
        from ._lib import PinnError
        flat = '; use lbfgs_impl="flat"'
        if line_search_fn != "strong_wolfe":
            raise PinnError(f"the device L-BFGS loop runs the strong_wolfe line search only (line_search_fn={line_search_fn!r})" + flat)
        if not 1 <= int(history_size) <= 256:
            raise PinnError(f"the device L-BFGS loop serves history_size 1..256 (got {history_size})" + flat)
        if int(max_iter) < 0:
            raise PinnError(f"max_iter={max_iter} must be >= 0" + flat)
        if max_eval is None:
            max_eval = int(max_iter) * 5 // 4          # torch.optim.LBFGS.__init__
        return SimpleNamespace(lr=float(lr), max_iter=int(max_iter), max_eval=int(max_eval), history_size=int(history_size),
                               tolerance_grad=float(tolerance_grad), tolerance_change=float(tolerance_change))

    def __init__(self, engine, spec, params, X, n_res, term_scale, loss_rows, total_row, T=None, out_col=(), col_scale=None,
                 lr=1.0, max_iter=20, max_eval=None, history_size=100, tolerance_grad=1e-7, tolerance_change=1e-9,
                 line_search_fn="strong_wolfe"):
        from . import _lib
        self._lib = _lib
        self.opts = self.check_options(lr, max_iter, max_eval, history_size, tolerance_grad, tolerance_change, line_search_fn)
        self.engine, self.spec, self.params, self.X, self.n_res = engine, spec, params, X, int(n_res)
        self.term_scale, self.loss_rows, self.total_row = term_scale, loss_rows, int(total_row)
        self.T, self.out_col, self.col_scale = T, tuple(out_col), col_scale
        ws_bytes, state_bytes = engine.lbfgs_loop_query(X.shape[0], self.opts.history_size)
        self.ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=params.device)
        self.state = torch.empty(state_bytes, dtype=torch.uint8, device=params.device)
        self.traces = []             # one (slots, LBFGS_TRACE_COLS) float64 CPU tensor per run
        self.reset()

    def reset(self):
        o = self.opts
        self.engine.lbfgs_loop_init(self.state, o.lr, o.max_iter, o.max_eval, o.history_size, o.tolerance_grad, o.tolerance_change)
        self.traces = []
        self._ctrl = None

    def enqueue(self, n_slots: int) -> torch.Tensor:
        """n_slots more slots; returns their trace (device tensor; nothing is synchronised)."""
        trace = torch.empty(n_slots, self._lib.LBFGS_TRACE_COLS, dtype=torch.float64, device=self.params.device)
        self.engine.lbfgs_loop(self.spec, self.term_scale, self.params, self.X, self.n_res, self.loss_rows, self.total_row,
                               self.state, n_slots, trace, T=self.T, out_col=self.out_col, col_scale=self.col_scale, ws=self.ws)
        self._ctrl = None
        return trace

    def run(self, n_slots: int) -> torch.Tensor:
        """enqueue(n_slots), then the trace on the host (one synchronisation) with the control block re-read."""
        tr = self.enqueue(n_slots).cpu()
        self.traces.append(tr)
        self.ctrl()
        return tr

    def ctrl(self):
        """The control block (pinn_lbfgs_ctrl) as the device holds it now (synchronises)."""
        if self._ctrl is None:
            import ctypes
            n = ctypes.sizeof(self._lib.PinnLbfgsCtrl)
            self._ctrl = self._lib.PinnLbfgsCtrl.from_buffer_copy(self.state[:n].cpu().numpy().tobytes())
        return self._ctrl

    @property
    def x_trial(self) -> torch.Tensor:
        """The weights of the last evaluation (x + t d), a view into the state: d and x_trial follow the control block,
        each region on a 256-byte boundary (include/pinn_hip.h, pinn_query_lbfgs_loop)."""
        import ctypes
        a = lambda v: (v + 255) // 256 * 256
        P = self.params.numel()
        off = a(ctypes.sizeof(self._lib.PinnLbfgsCtrl)) + a(4 * P)
        return self.state[off:off + 4 * P].view(torch.float32)

    def step(self, before_run=None, after_run=None):
        """Runs until the done flag is up.  before_run(evaluations so far) -> an upper limit for the slots of the next run;
        after_run(trace of the run, CPU) is called after each."""
        while not self.done:
            # an inert slot still runs its pass, so a run never holds more slots than the iterations left need at the
            # least (one evaluation each) nor more than the evaluation budget allows (a line search may overrun it by one)
            c, o = self.ctrl(), self.opts
            n = max(1, min(self.RUN, o.max_iter - c.n_iter + 1, o.max_eval + 1 - c.n_evals))
            if before_run is not None:
                n = max(1, min(n, int(before_run(self.func_evals))))
            tr = self.run(n)
            if after_run is not None:
                after_run(tr)
        return self

    @property
    def done(self) -> bool:
        return bool(self.ctrl().done)

    @property
    def n_iter(self) -> int:
        return self.ctrl().n_iter

    @property
    def func_evals(self) -> int:
        return self.ctrl().n_evals

    @property
    def stop_reason(self):
        return self._lib.LBFGS_STOP_REASONS[self.ctrl().reason]

    @property
    def trace(self) -> torch.Tensor:
        """Every slot run so far, (slots, LBFGS_TRACE_COLS) float64 on the CPU."""
        return torch.cat(self.traces) if self.traces else torch.zeros(0, self._lib.LBFGS_TRACE_COLS, dtype=torch.float64)


class EnsembleDeviceLBFGS:
    """DeviceLBFGS for the M networks of an ensemble (Engine.ensemble_lbfgs_loop, pinn_ensemble_lbfgs_loop): every member
    its own strong-Wolfe search, ring and stopping tests, all advanced by one schedule of launches per slot.  `params`
    (M, P): row j holds member j's accepted iterate after every run.  One set of options for all members.  The host reads
    the M control blocks once per run (one copy) and stops when every done flag is up; a member that has stopped is inert
    in the slots the others still need."""

    RUN = DeviceLBFGS.RUN

    def __init__(self, engine, spec, params, X, n_res, term_scale, loss_rows, total_row, T=None, out_col=(), col_scale=None,
                 lr=1.0, max_iter=20, max_eval=None, history_size=100, tolerance_grad=1e-7, tolerance_change=1e-9,
                 line_search_fn="strong_wolfe"):
        from . import _lib
        self._lib = _lib
        self.opts = DeviceLBFGS.check_options(lr, max_iter, max_eval, history_size, tolerance_grad, tolerance_change, line_search_fn)
        self.engine, self.spec, self.params, self.X, self.n_res = engine, spec, params, X, int(n_res)
        self.term_scale, self.loss_rows, self.total_row = term_scale, loss_rows, int(total_row)
        self.T, self.out_col, self.col_scale = T, tuple(out_col), col_scale
        self.members = int(params.shape[0])
        N = X.shape[1] if X.dim() == 3 else X.shape[0]
        ws_bytes, state_bytes = engine.ensemble_lbfgs_loop_query(self.members, N, self.opts.history_size)
        self.ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=params.device)
        self.state = torch.empty(state_bytes, dtype=torch.uint8, device=params.device)
        self.traces = []             # one (slots, M, LBFGS_TRACE_COLS) float64 CPU tensor per run
        self.reset()

    def reset(self):
        o = self.opts
        self.engine.ensemble_lbfgs_loop_init(self.state, self.members, o.lr, o.max_iter, o.max_eval, o.history_size,
                                             o.tolerance_grad, o.tolerance_change)
        self.traces = []
        self._ctrls = None

    def enqueue(self, n_slots: int) -> torch.Tensor:
        """n_slots more slots; returns their trace (device tensor; nothing is synchronised)."""
        trace = torch.empty(n_slots, self.members, self._lib.LBFGS_TRACE_COLS, dtype=torch.float64, device=self.params.device)
        self.engine.ensemble_lbfgs_loop(self.spec, self.term_scale, self.params, self.X, self.n_res, self.loss_rows,
                                        self.total_row, self.opts.history_size, self.state, n_slots, trace, T=self.T,
                                        out_col=self.out_col, col_scale=self.col_scale, ws=self.ws)
        self._ctrls = None
        return trace

    def run(self, n_slots: int) -> torch.Tensor:
        """enqueue(n_slots), then the trace on the host (one synchronisation) with the control blocks re-read."""
        tr = self.enqueue(n_slots).cpu()
        self.traces.append(tr)
        self.ctrls()
        return tr

    def ctrls(self):
        """The M control blocks (pinn_lbfgs_ctrl) as the device holds them now: one copy, one synchronisation."""
        if self._ctrls is None:
            stride = self._lib.ensemble_lbfgs_ctrl_stride()
            raw = self.state[:self.members * stride].cpu().numpy().tobytes()
            self._ctrls = [self._lib.PinnLbfgsCtrl.from_buffer_copy(raw, j * stride) for j in range(self.members)]
        return self._ctrls

    @property
    def x_trial(self) -> torch.Tensor:
        """(M, P): the members' weights of the last evaluation (x + t d), a view into the state: the control blocks, d
        (M, P) and x_trial (M, P), each region on a 256-byte boundary (include/pinn_hip.h)."""
        a = lambda v: (v + 255) // 256 * 256
        M, P = self.params.shape
        off = M * self._lib.ensemble_lbfgs_ctrl_stride() + a(4 * M * P)
        return self.state[off:off + 4 * M * P].view(torch.float32).view(M, P)

    def step(self, before_run=None, after_run=None):
        """Runs until every member's done flag is up.  Each run is sized by the member that still needs the most slots,
        under DeviceLBFGS.step's rule; before_run(most evaluations of a member so far) -> an upper limit for the slots of
        the next run; after_run(trace of the run, CPU) is called after each."""
        while not self.done:
            o = self.opts
            need = max(min(o.max_iter - c.n_iter + 1, o.max_eval + 1 - c.n_evals) for c in self.ctrls() if not c.done)
            n = max(1, min(self.RUN, need))
            if before_run is not None:
                n = max(1, min(n, int(before_run(max(self.func_evals)))))
            tr = self.run(n)
            if after_run is not None:
                after_run(tr)
        return self

    @property
    def done(self) -> bool:
        return all(c.done for c in self.ctrls())

    @property
    def n_iter(self):
        return [c.n_iter for c in self.ctrls()]

    @property
    def func_evals(self):
        return [c.n_evals for c in self.ctrls()]

    @property
    def stop_reason(self):
        return [self._lib.LBFGS_STOP_REASONS[c.reason] for c in self.ctrls()]

    @property
    def trace(self) -> torch.Tensor:
        """Every slot run so far, (slots, M, LBFGS_TRACE_COLS) float64 on the CPU."""
        if not self.traces:
            return torch.zeros(0, self.members, self._lib.LBFGS_TRACE_COLS, dtype=torch.float64)
        return torch.cat(self.traces)
