"""Admissibility of every case of tests/switch_cases.py, on the CPU oracle alone.  These are conditions on the test
inputs, not measurements of the library: a case that fails one has the wrong inputs.

  sensitivity   the oracle with the case's settings differs from the oracle on the bare base (same inputs) by at least
                1e-6 -- four orders above TOL_TRAJ = TOL_SIZE = 1e-10 -- in a berg field, an accumulator plane or an
                output plane (a counter for the counter-only cases): a case that moves nothing tests nothing;
  health        everything finite, error_count 0, and for the bonded base some bond breaks;
  conditioning  with every berg moved one ulp the oracle gives the same survivors, cells and broken bonds, and agrees
                with itself within a tenth of the tolerance compare / compare_mts applies to each field: parity is
                then not decided by rounding.
"""
import numpy as np
import pytest

import parity as P
import switch_cases as SC
from icebergs_amd import types as T

SENSITIVITY = 1.0e-6
FIELDS = P.TRAJ_FIELDS + P.SIZE_FIELDS


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


def _scalar(run, name):
    return run[3][T.SCALAR_NAMES[name]]


def test_tables_are_well_formed():
    ids = [SC.case_id(c) for c in SC.PER_BERG + SC.BONDED]
    assert len(ids) == len(set(ids))
    p = T.Params()
    for c in SC.PER_BERG + SC.BONDED:
        assert c.settings and all(hasattr(p, k) for k in c.settings), c
        assert "tidal_drift" not in c.settings   # the stochastic stream is FMS's
    # every member of KID_SWITCHES outside the families existing tests cover is moved alone on both bases, unless
    # it cannot act there
    alone = {(c.base, SC.moves_one_switch(c)) for c in SC.PER_BERG}
    left_out = {("plain", "internal_bergs_for_drag"), ("flprof", "internal_bergs_for_drag"),   # read with iceberg_bonds_on only
                ("flprof", "use_new_predictive_corrective"),    # read by the Runge-Kutta scheme only
                ("flprof", "use_f_plane"),                      # read on a latitude-longitude grid only
                ("plain", "use_operator_splitting"),            # without bergy bits only the diagnostics see it: run with them
                ("flprof", "use_operator_splitting"),           # footloose refuses use_operator_splitting = F (FW:1476)
                ("flprof", "find_melt_using_spread_mass"),      # not implemented together with footloose (KID_EUNSUPPORTED)
                ("plain", "use_mixed_melting"), ("flprof", "use_mixed_melting")}   # needs static bergs, which select K = 0 themselves
    # the footloose profile spreads no mass onto the ocean: these run there together with add_weight_to_ocean
    left_out |= {("flprof", n) for n in ("grounding_fraction", "clipping_depth", "hexagonal_icebergs", "use_old_spreading",
                                         "time_average_weight")}
    for name in SC.KID_SWITCHES:
        if name in ("mts", "dem", "footloose", "iceberg_bonds_on"):
            continue
        for base in ("plain", "flprof"):
            assert ((base, name) in alone) != ((base, name) in left_out), (base, name)


def test_every_member_the_library_reads_is_moved_or_excluded_by_name():
    read, moved = SC.members_read_by_the_library(), SC.members_moved_by_a_case()
    assert len(read) > 100    # the scan finds the sources
    print("kid_params: %d members, %d read by icebergs_amd/csrc, %d of them moved by a case, %d excluded by name"
          % (len(T.Params._fields_), len(read), len([m for m in read if m in moved]), len([m for m in read if m in SC.EXCLUDED])))
    for m in read:
        assert (m in moved) != (m in SC.EXCLUDED), m + (": moved and excluded" if m in moved else ": neither moved by a case nor excluded")
    assert "tidal_drift" in SC.EXCLUDED and not (set(SC.EXCLUDED) - set(read))


@pytest.mark.parametrize("case", SC.PER_BERG, ids=SC.case_id)
def test_per_berg_case_is_admissible(case):
    """Branches of find_basal_melt taken by the plain ice-shelf cases, counted with a scratch copy of the oracle (six
    steps of 5000 bergs = 30000 calls each; the first two columns count passes of the salinity iteration, up to 20 a
    call, the other two count calls):
      case                     wB_flux > 0   wB_flux <= 0   convergence break   two-equation form
      ice_shelf                     154435          78354               27102                   0
      ice_shelf_var_gamma           177758          57258               30000                   0
      ice_shelf_two_eq                   0              0                   0               30000
      ice_shelf_ml_salinity         152871          78354               27186                   0
      ice_shelf_tide                154435          78354               27102                   0
      ice_shelf_cutoff              154435          78354               27102                   0
      ice_shelf_gamma_t             154435          78354               27102                   0
      ice_shelf_ustar               157172          57028               30000                   0
      mixed_melting (static)        154434          78354               27102                   0
    On its first pass a call has wB_flux > 0 for the 2736 berg-steps in the band of water below the freezing point and
    <= 0 for the other 27264.  With constant gamma 2898 calls run all 20 passes without converging (the band again).  The
    out-of-bounds fall-back to the two-equation form is not taken by any call on these grids (0 of 30000 in every
    case): that branch of the device copy is still read against the oracle's only."""
    base = SC.oracle_run(case.base, case.also or {}, case.inputs, keep=True)
    ref = SC.oracle_run(case.base, SC.all_settings(case), case.inputs)
    # health
    assert SC.finite(ref), "not finite"
    assert _scalar(ref, "error_count") == 0
    assert _scalar(ref, "nbergs_alive") > 0
    # sensitivity
    if case.name in SC.COUNTER_ONLY:
        name = SC.COUNTER_ONLY[case.name]
        assert _scalar(ref, name) != _scalar(base, name), "the counter %s does not move" % name
    else:
        d = SC.differences(base, ref, FIELDS)
        worst = max(d, key=d.get)
        print("%s: sensitivity %.1e (%s)" % (SC.case_id(case), d[worst], worst))
        assert d[worst] >= SENSITIVITY, "moves the oracle by %.1e only (%s)" % (d[worst], worst)
    # conditioning
    nud = SC.oracle_run(case.base, SC.all_settings(case), case.inputs, nudge=True)
    rows, nrows = SC.by_id(ref[0]), SC.by_id(nud[0])
    assert np.array_equal(ref[0]["id"][rows], nud[0]["id"][nrows]), "an ulp changes the set of survivors"
    for f in ("ine", "jne"):
        assert np.array_equal(ref[0][f][rows], nud[0][f][nrows]), "an ulp changes " + f
    d = SC.differences(ref, nud, FIELDS + P.ENV_FIELDS)
    for k, e in d.items():
        tol = P.TOL_GRID if k.startswith(("acc", "out")) else P.TOL_TRAJ
        assert e <= 0.1 * tol, "an ulp moves %s by %.1e" % (k, e)
    for name in ("nbergs_melted", "nbergs_calved_fl", "nspeeding_tickets", "nbergs_alive"):
        assert _scalar(ref, name) == _scalar(nud, name), name


def _mts_errors(ref, refbd, got, gotbd):
    """(error, tolerance of compare_mts) per compared quantity"""
    stiff = {"axn", "ayn", "bxn", "byn", "axn_fast", "ayn_fast", "bxn_fast", "byn_fast", "ang_accel"}
    out = {}
    for f in P.TRAJ_FIELDS + P.MTS_FIELDS + P.SIZE_FIELDS:
        out[f] = (P.rel_err(got[0][f], ref[0][f]), 1.0e-4 if f in stiff else (1.0e-6 if f in ("ang_vel", "rot") else 1.0e-9))
    live = (np.arange(refbd["max_bonds"])[:, None] < refbd["count"][None, :]).ravel()
    for f in P.BOND_STATE + ["f_x", "f_y", "fd_x", "fd_y", "t", "t_d"]:
        out["bond_" + f] = (P.rel_err(gotbd[f][live], refbd[f][live]), 1.0e-9 if f == "length" else 1.0e-4)
    sc = P.acc_scales(ref[1])
    for k in range(ref[1].shape[0]):
        out["acc%d" % k] = (P.acc_err(got[1], ref[1], k, sc), 10 * P.TOL_GRID)
    solid = np.abs(ref[2][T.OUT_NAMES["spread_area"]]) > 1.0e-9
    for k in range(ref[2].shape[0]):
        a, b = (got[2][k][solid], ref[2][k][solid]) if k == T.OUT_NAMES["ustar_iceberg"] else (got[2][k], ref[2][k])
        out["out%d" % k] = (P.rel_err(a, b), 10 * P.TOL_GRID)
    return out


@pytest.mark.parametrize("case", SC.BONDED, ids=SC.case_id)
def test_bonded_case_is_admissible(case):
    (base, basebd) = SC.oracle_run("bonded", case.also or {}, keep=True)
    (ref, refbd) = SC.oracle_run("bonded", SC.all_settings(case))
    # health
    assert SC.finite(ref) and all(np.isfinite(refbd[f]).all() for f in P.BOND_STATE), "not finite"
    assert _scalar(ref, "error_count") == 0
    if case.name not in SC.NO_FRACTURE:
        assert (refbd["broken"] != 0).sum() > 0, "no bond breaks"
    # sensitivity
    d = {k: e for k, (e, _) in _mts_errors(base, basebd, ref, refbd).items()}
    worst = max(d, key=d.get)
    print("%s: sensitivity %.1e (%s)" % (SC.case_id(case), d[worst], worst))
    assert d[worst] >= SENSITIVITY or not np.array_equal(basebd["broken"], refbd["broken"]), \
        "moves the oracle by %.1e only (%s)" % (d[worst], worst)
    # conditioning
    (nud, nudbd) = SC.oracle_run("bonded", SC.all_settings(case), nudge=True)
    assert np.array_equal(refbd["count"], nudbd["count"]) and np.array_equal(refbd["other_id"], nudbd["other_id"])
    assert np.array_equal(refbd["broken"], nudbd["broken"]), "an ulp changes the set of broken bonds"
    for f in ("ine", "jne", "conglom_id", "n_bonds"):
        assert np.array_equal(ref[0][f], nud[0][f]), f
    for k, (e, tol) in _mts_errors(ref, refbd, nud, nudbd).items():
        assert e <= 0.1 * tol, "an ulp moves %s by %.1e (tolerance %.1e)" % (k, e, tol)
