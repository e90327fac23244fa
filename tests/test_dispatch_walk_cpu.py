"""The C-ABI's host-side dispatch over a grid of descriptors (dispatch_walk_util.py): every entry agrees with its own query.

  - Where the query refuses, the call refuses with the same code and the same text (the entry's own name aside).
  - Where the query answers, the call without a workspace returns PINN_ERR_WORKSPACE naming exactly the query's bytes.
    The ensemble calls may refuse instead with "corrected" or "split" (their request-level refusals), or with the spec's own
    fault: their query sees no spec.
  - pinn_forward, pinn_forward_jet, pinn_residual_loss_grad and pinn_jet_backward never need more than pinn_query_workspace
    answers, where both succeed.  (The converse is NOT asserted: for some descriptors the general query refuses although
    pinn_forward or pinn_jet_backward would be served.)

The probes with non-NULL arrays are host logic only while no GPU is visible, and what needs them is skipped where one is;
the probes with NULL arrays run everywhere, for the entries that decide their refusals before they look at a pointer.
Every descriptor of the grid is walked at one N of the list, rotating, so that every N meets every value of every axis."""
import re

import pytest
import torch

from tests import dispatch_walk_util as W
from pinn_depthestimation_amd import _lib

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
NO_GPU = not torch.cuda.is_available()

# query -> the calls it answers for (matched on the probe's context; the ensemble's on its "M=" part)
PAIRS = {
    "pinn_query_fields_workspace": ("pinn_residual_fields",),
    "pinn_query_residual_coef_workspace": ("pinn_residual_coef_loss_grad",),
    "pinn_query_residual_weighted_workspace": ("pinn_residual_weighted_loss_grad",),
    "pinn_query_residual2_workspace": ("pinn_residual2_loss_grad",),
    "pinn_query_jet2_workspace": ("pinn_forward_jet2", "pinn_jet2_backward"),
    "pinn_query_adam_ext_workspace": ("pinn_adam_loop_ext",),
    "pinn_ensemble_query_workspace": ("pinn_ensemble_loss_grad", "pinn_ensemble_adam_step", "pinn_ensemble_adam_loop"),
    "pinn_ensemble_plan": ("pinn_ensemble_loss_grad", "pinn_ensemble_adam_step", "pinn_ensemble_adam_loop"),
    "pinn_jet_backward_kernel": ("pinn_jet_backward",),
}
ENSEMBLE = ("pinn_ensemble_query_workspace", "pinn_ensemble_plan")
# pinn_jet_backward looks at its pointers before it picks the engine: its refusals show with non-NULL arrays only
NULLS_FIRST = ("pinn_jet_backward",)
GENERAL = ("pinn_forward", "pinn_forward_jet", "pinn_residual_loss_grad", "pinn_jet_backward")


def need_of(p):
    m = re.search(r"workspace too small: need (\d+) bytes", p.err)
    return int(m.group(1)) if m else None


def unnamed(err):
    """the message without the entry's own name in front (a loop reports as the step it calls)"""
    return re.sub(r"^pinn_\w+", "@", err)


def spec_fault(p):
    return p.rc == INVALID and ("out_col[" in p.err or "dir_of[" in p.err)


def check_block(label, probes, counts):
    calls = {}
    for p in probes:
        if p.probe != "query":
            calls.setdefault(p.entry, []).append(p)
    bad_specs = {p.ctx for p in probes if p.entry == "pinn_query_fields_workspace" and spec_fault(p)}
    for q in probes:
        if q.probe != "query" or q.entry not in PAIRS:
            continue
        for entry in PAIRS[q.entry]:
            for c in calls[entry]:
                if q.entry in ENSEMBLE:
                    if not c.ctx.endswith(q.ctx):
                        continue
                elif c.ctx != q.ctx:
                    continue
                where = (label, q.entry, c.entry, c.ctx, c.probe, q, c)
                if q.rc != OK:      # the query refuses: so does the call, in the same words
                    if c.probe == "null" and entry in NULLS_FIRST:
                        continue
                    assert c.rc == q.rc and unnamed(c.err) == unnamed(q.err), where
                    counts["refused alike"] += 1
                elif c.probe == "dummy":      # the query answers: the call gets as far as its workspace, of that size
                    if q.entry in ENSEMBLE and c.rc != WORKSPACE:
                        spec_ctx = " ".join(c.ctx.split()[:2])
                        assert (c.rc == UNSUPPORTED and ("corrected" in c.err or "split" in c.err)) or \
                               (spec_ctx in bad_specs and spec_fault(c)), where
                        counts["ensemble request refused"] += 1
                        continue
                    assert c.rc == WORKSPACE, where
                    if q.entry == "pinn_ensemble_plan" or q.entry == "pinn_jet_backward_kernel":
                        continue      # (they answer a grid / a kernel, not a size)
                    assert need_of(c) == q.value[0], where
                    counts["workspace as queried"] += 1
    general = next(p for p in probes if p.entry == "pinn_query_workspace")
    if general.rc == OK:
        for entry in GENERAL:
            for c in calls[entry]:
                if c.probe == "dummy" and c.rc == WORKSPACE:
                    assert need_of(c) <= general.value[0], (label, entry, c, general)
                    counts["within the general query"] += 1


@pytest.mark.parametrize("shape", W.SHAPES, ids=["x".join(map(str, s)) for s in W.SHAPES])
def test_every_entry_agrees_with_its_query(shape):
    lib = _lib.load()
    counts = dict.fromkeys(("refused alike", "workspace as queried", "ensemble request refused", "within the general query"), 0)
    for i, key in enumerate(W.descriptors((shape,))):
        N = W.NS[(i + i // 4 + i // 28 + i // 84) % len(W.NS)]
        w = W._Walker(lib, with_dummy=NO_GPU)
        check_block("%s N=%d" % (W.desc_label(key), N), w.block(key, N), counts)
    print(shape, counts)
    assert counts["refused alike"] > 0
    if NO_GPU and shape[0] <= 16 and shape[1] <= 16:      # (beyond 16 inputs or outputs the spec entries serve nothing fused)
        assert counts["workspace as queried"] > 0 and counts["within the general query"] > 0


def test_the_walk_reaches_every_kind_of_answer():
    """one descriptor in full: queries answer, calls stop at the workspace, and the dump has a line per probe"""
    lib = _lib.load()
    key = ((3, 4, 8, 64), 3, 0, 0, 0, 0.0)
    probes = W._Walker(lib, with_dummy=NO_GPU).block(key, 243)
    by = {(p.entry, p.ctx, p.probe): p for p in probes}
    assert len(by) == len(probes)                                       # (entry, context, probe) names a probe
    assert by[("pinn_param_count", "", "query")].value == (3 * 64 + 64 + 7 * (64 * 64 + 64) + 64 * 4 + 4,)
    assert by[("pinn_query_workspace", "", "query")].rc == OK
    assert by[("pinn_ensemble_plan", "M=3", "query")].value == (4, 1)
    assert by[("pinn_residual_loss_grad", "res=1 flags=0", "null")].rc == INVALID
    if NO_GPU:
        assert by[("pinn_residual_loss_grad", "res=1 flags=0", "dummy")].rc == WORKSPACE
        assert by[("pinn_ensemble_loss_grad", "res=1 flags=0 n_res=split M=3", "dummy")].rc == UNSUPPORTED      # width 64: no split
    lines = list(W.dump_lines(lib, ns=(243,), with_dummy=NO_GPU, shapes=((2, 3, 2, 10),)))
    assert len(lines) == len(set(lines)) and all(" | rc=" in x for x in lines)
