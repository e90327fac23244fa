"""The second sweep's draw is fit for purpose (tests/sweep2_util.py), checked on the reference alone: no GPU.

  conditions  every committed seed: fp64 sums, fields and gradient finite, the gradient non-zero in every block the formula
              leaves non-zero, the reference's own fp32-vs-fp64 gap at most GAP_MARGIN < GAP_CAP per block, no tiny point set on
              a cancellation (sweep2_util.small_set_noise)
  power       every mis-reading a wrong kernel might make (sweep2_util.mutants: roles or directions swapped, the corrected
              flag or nu ignored, term scales exchanged, fidelity rows from the front, the next member's points or targets),
              evaluated through the fp64 reference, fails the field bound and the block-wise gradient bound that
              test_sweep2_gpu.py applies — the committed proof that the GPU module would notice
  census      each family's seed range holds at least 3 cases of every bucket it can reach
  served      sweep2_util.served agrees with the library's host-only queries (pinn_jet_backward_kernel, pinn_ensemble_plan)

The library is called through host-only queries alone: no entry that takes a data pointer."""
import ctypes as C

import pytest
import torch

from pinn_depthestimation_amd import NetDesc, _lib
from pinn_depthestimation_amd._lib import ENGINE_FUSED_BATCH, ENGINE_FUSED_TILE
from tests import sweep2_util as S
from tests.trained_state_util import GAP_CAP, assert_blocks_close, block_errors, param_blocks

CASES = [(f, s) for f in S.FAMILIES for s in S.SEEDS[f]]


def runs(family, seed):
    """Whether the case has a reference (the ensemble draws that must be refused have none)."""
    return family != "ens" or S.served(family, S.draw(family, seed), "auto")


def test_the_draw_is_deterministic_and_inside_its_lists():
    for f, s in CASES:
        c = S.draw(f, s)
        assert c == S.draw(f, s)
        assert c.W in S.WIDTHS and (c.L in S.DEPTHS or (c.L == 40 and c.W <= 24))
        assert c.N in (S.ADJ_POINTS if f == "adj" else S.POINTS + [9600]) and 2 <= c.k <= 3 and c.d_in <= 8 and c.d_out <= 16
        if c.res:
            out_roles, dir_roles = S.ROLES[c.res]
            assert set(out_roles) <= set(c.outn) and all(c.inn.index(r) in c.gc for r in dir_roles)
            assert c.n_res >= 1 and c.n_res + (c.n_fid if c.kind == "split" else 0) == c.N
        if c.corrected or f in ("fields", "res2"):
            assert not c.extra_dir
    assert len(CASES) == sum(len(S.SEEDS[f]) for f in S.FAMILIES) and all(24 <= len(S.SEEDS[f]) <= 40 for f in S.FAMILIES)


@pytest.mark.parametrize("family", S.FAMILIES)
def test_conditions_on_every_committed_seed(family):
    worst_gap, worst_noise = (0.0, ""), (0.0, "")
    for seed in S.SEEDS[family]:
        if not runs(family, seed):
            continue
        c = S.draw(family, seed)
        for m, (r64, r32) in enumerate(S.reference(family, seed)):
            what = f"{c.tag()} member {m}"
            for name in ("sums", "cols", "fields", "grad"):
                if hasattr(r64, name):
                    assert bool(torch.isfinite(getattr(r64, name)).all()), (what, name)
            assert float(r64.grad.norm()) > 0, what
            gaps = block_errors(r32.grad, r64.grad, c.layers)
            for name, a, b in param_blocks(c.layers):
                # no block is idle, but the output bias under gdY alone: dY does not depend on it
                idle = family == "adj" and c.mode == "gdY" and name == f"b{c.L}"
                assert (float(r64.grad[a:b].norm()) > 0) != idle, (what, name)
                assert gaps[name] <= S.GAP_MARGIN < GAP_CAP, (what, name, gaps[name])
            worst_gap = max(worst_gap, (max(gaps.values()), what))
            if hasattr(r64, "fields"):
                assert hasattr(r64, "noise") == (family in ("fields", "res2") or c.n_res < S.SMALL_SET)
                assert S.small_set_noise(c, r64) <= S.SMALL_SET_NOISE, (what, S.small_set_noise(c, r64))
                assert r64.fields.shape == (S.N_FIELDS[c.res], c.n_res)
                noise = float(((r32.fields - r64.fields).abs().amax(1) / r64.fields.abs().amax(1).clamp_min(1e-300)).max())
                worst_noise = max(worst_noise, (noise, what))
    print(f"SWEEP2 {family}: worst block gap {worst_gap[0]:.1e} ({worst_gap[1]}); worst relative field noise {worst_noise[0]:.1e} ({worst_noise[1]})")


def gradient_fails(got, r64, r32, layers):
    """(whether assert_blocks_close rejects `got`, its worst block error)."""
    errs = block_errors(got, r64.grad, layers)
    try:
        assert_blocks_close(got, r64.grad, r32.grad, layers, "mutant")
    except AssertionError:
        return True, max(errs.values())
    return False, max(errs.values())


@pytest.mark.parametrize("family", S.FAMILIES)
def test_power_every_misreading_fails_the_bounds(family):
    """Per mutant the weakest margin over the family's seeds.  Fields: (a)-(d) change them and must fail the field bound in
    at least one member; (e)-(g) leave the fields alone (scales, fidelity rows) or are checked per member.  Gradient: must
    fail assert_blocks_close in at least one block, for every member whose request the mis-reading changes."""
    weakest = {}
    for seed in S.SEEDS[family]:
        if not runs(family, seed):
            continue
        c = S.draw(family, seed)
        ref = S.reference(family, seed)
        for name, per_member in S.mutants(family, seed).items():
            w = weakest.setdefault(name, dict(grad=(float("inf"), ""), field=(float("inf"), ""), n=0))
            w["n"] += 1
            for m, mut in enumerate(per_member):
                r64, r32 = ref[m]
                what = f"{c.tag()} member {m}"
                if family != "fields":
                    failed, err = gradient_fails(mut.grad, r64, r32, c.layers)
                    assert failed, (name, what, err)
                    w["grad"] = min(w["grad"], (err, what))
                if name[0] in "abcd" and family in ("fields", "res2"):
                    ratio = max(S.field_ratios(mut.fields, r64))
                    assert ratio > S.FIELD_BOUND, (name, what, ratio)
                    rel = float(((mut.fields - r64.fields).abs().amax(1) / r64.fields.abs().amax(1).clamp_min(1e-300)).max())
                    w["field"] = min(w["field"], (rel, what))
                if name[0] == "f":                    # the column sums move too
                    assert S.sum_ratio(mut.cols, r64.cols, r32.cols) > 1.0, (name, what)
    for name, w in weakest.items():
        parts = [f"weakest worst-block gradient error {w['grad'][0]:.1e} ({w['grad'][1]})"] if w["grad"][1] else []
        parts += [f"weakest field error {w['field'][0]:.1e} ({w['field'][1]})"] if w["field"][1] else []
        print(f"SWEEP2 power {family} / {name}: {w['n']} cases; " + "; ".join(parts))
    need = {"pec": "abcef", "fields": "abc", "res2": "abcde", "ens": "abefg", "adj": "b"}[family]
    assert {n[0] for n in weakest} == set(need), sorted(weakest)


@pytest.mark.parametrize("family", S.FAMILIES)
def test_census(family):
    cnt = S.census(family)
    print(f"SWEEP2 census {family} ({len(S.SEEDS[family])} seeds): " + ", ".join(f"{k}: {v}" for k, v in cnt.items()))
    assert all(v >= 3 for v in cnt.values()), {k: v for k, v in cnt.items() if v < 3}
    cases = [S.draw(family, s) for s in S.SEEDS[family]]
    assert any(c.N == 1 for c in cases) and not set(S.SKIPPED[family]) & set(S.SEEDS[family])
    if family == "pec":
        plain = sum(not c.corrected for c in cases)
        assert 3 <= plain <= len(cases) // 2 and {c.kind for c in cases} == {"residual", "onepass", "split"}
        assert sum("batch" in S.engines(family, c) for c in cases) >= 6
    if family == "fields":
        assert {c.res + "+c" * c.corrected for c in cases} == set(S.RESIDUALS["fields"])
    if family == "res2":
        assert {c.nu for c in cases} == {0.05, 1.0} and {c.res + "+c" * c.corrected for c in cases} == set(S.RESIDUALS["res2"])
    if family == "adj":
        assert {c.mode for c in cases} == {"gY", "gdY", "both"} and sum(c.L == 40 for c in cases) >= 1
        assert {c.N for c in cases} == set(S.ADJ_POINTS)
    if family == "ens":
        assert {c.M for c in cases} == set(S.MEMBERS) and {c.kind for c in cases} == {"residual", "onepass", "split"}
        assert any(c.own_x for c in cases) and any(c.own_t for c in cases) and any(not c.own_x for c in cases)
        refused = [c for c in cases if not S.served(family, c, "auto")]
        assert any(c.corrected for c in refused) and any(c.kind == "split" and c.wp == 64 for c in refused)


# ---- served() against the library's host-only queries -------------------------------------------------------------------
def test_served_agrees_with_the_jet_backward_kernel_query():
    lib = _lib.load()
    for seed in S.SEEDS["adj"]:
        c = S.draw("adj", seed)
        desc = NetDesc(c.d_in, c.d_out, c.L, c.W, c.gc, engine=ENGINE_FUSED_BATCH)
        kern = C.c_int32(-1)
        rc = lib.pinn_jet_backward_kernel(C.byref(desc.c_struct()), c.N, 0 if c.mode == "gY" else 1, C.byref(kern))
        assert (rc == 0) == S.served("adj", c, "batch"), (c.tag(), lib.pinn_last_error().decode())
        assert kern.value == (ENGINE_FUSED_BATCH if S.adj_runs_on_batch(c) else ENGINE_FUSED_TILE), c.tag()
    assert sum(S.adj_runs_on_batch(S.draw("adj", s)) for s in S.SEEDS["adj"]) >= 16


def test_the_ensemble_draw_reaches_several_workgroups_and_a_clamped_grid():
    """pinn_ensemble_plan on a 256-CU device (its answer without one): the family holds members with one workgroup, with
    several, and a grid clamped by M (fewer workgroups per member than a single member gets at the same N)."""
    lib = _lib.load()
    gx, lds = C.c_int32(), C.c_int32()

    def plan(c, M):
        desc = NetDesc(c.d_in, c.d_out, c.L, c.W, c.gc)
        assert lib.pinn_ensemble_plan(C.byref(desc.c_struct()), M, c.N, C.byref(gx), C.byref(lds)) == 0, lib.pinn_last_error().decode()
        return gx.value, lds.value
    one = several = clamped = in_ws = 0
    for seed in S.SEEDS["ens"]:
        c = S.draw("ens", seed)
        if not S.served("ens", c, "auto"):
            continue
        g, in_lds = plan(c, c.M)
        one += g == 1; several += g > 1; in_ws += not in_lds
        clamped += g < plan(c, 1)[0]
    print(f"SWEEP2 ens plan: one workgroup {one}, several {several}, clamped {clamped}, gradient copy in the workspace {in_ws}")
    assert one >= 3 and several >= 3 and clamped >= 1
