"""Case tables of the namelist-switch tests (test_namelist_switches_cpu.py, test_namelist_switches_gpu.py): every
member of kid_params that the device code reads and that the BASELINE namelists leave at one value, moved off that
value on a base configuration whose forcing gives the switch something to act on.

A case is (name, base, settings, inputs, also): `settings` are the kid_params members the case moves, `inputs` names a
variant of the base's berg population ("" = the base as it is), and `also` holds settings the switch needs in order to
act; the run a case's sensitivity is measured against has them too.  Three bases:

  plain   config_c2(n=5000, seed=7, continents=True): RK4, old order of the phases, the plain namelist (build K = 1);
          5000 > the 4096 thresholds of the host code and no multiple of 256.  Sea ice, ice velocity, salinity, a
          variable ocean depth and a band of water below the freezing point are added here.
  flprof  config_c3(n=600, fl_style="new_bergs", displace=True): Verlet, new order, the footloose profile (K = 2),
          with the same additions on its Cartesian grid (sst stays the profile's -0.5 outside the cold band) and a coast
          along the south of the channel.
  bonded  config_c4(), 55 bonded DEM elements grounding on a seamount, 200 sub-steps, every diagnostic on.

Input variants: "static" -- every fourth berg carries static_berg = 1 (N_bonds = N_max in the mixed-melting blend; a
population with static bergs is stepped by the general build K = 0, so the bare bases carry none); "narrow" -- every
third berg is narrower than it is thick, around the rolling thresholds of the three schemes (no berg of the bare bases
rolls within six steps).
"""
import collections
import functools

import numpy as np

import parity as P
from icebergs_amd import synthetic as S
from icebergs_amd import types as T

NSTEPS = 6
Case = collections.namedtuple("Case", "name base settings inputs also", defaults=("", None))


# ---------------------------------------------------------------------------------------------------------
# bases
# ---------------------------------------------------------------------------------------------------------
def _scrub(grid):
    st, f = grid["static"], grid["forcing"]
    land = st["msk"] < 0.5
    for k in ("ua", "va", "uo", "vo", "ui", "vi", "sst", "sss", "cn", "hi"):
        f[k][land] = 0.0


@functools.lru_cache(maxsize=None)
def _plain():
    grid, p, b = S.config_c2(n=5000, seed=7, continents=True)
    st, f = grid["static"], grid["forcing"]
    rad = np.pi / 180.0
    lonc, latc = st["lonc"], st["latc"]
    f["cn"][:] = 0.9 * np.clip((np.abs(latc) - 55.0) / 15.0, 0.0, 1.0) * (0.5 + 0.5 * np.cos(2.0 * lonc * rad))
    f["hi"][:] = 1.5 * f["cn"]
    f["ui"][:] = 0.1
    f["vi"][:] = -0.05
    f["sss"][:] = 33.0 + 2.0 * np.cos(latc * rad)
    st["ocean_depth"][:] = 150.0 + 3000.0 * np.cos(lonc * rad) ** 2
    f["sst"][(np.abs(latc) > 60.0) & (np.abs(latc) < 66.0)] = -2.2   # below the freezing point at depth: ice accretes
    _scrub(grid)
    return grid, p, b


@functools.lru_cache(maxsize=None)
def _flprof():
    grid, p, b = S.config_c3(n=600, fl_style="new_bergs", displace=True)
    st, f = grid["static"], grid["forcing"]
    xc, yc = st["lonc"], st["latc"]
    f["cn"][:] = 0.9 * np.clip((yc - 8.0e3) / 8.0e3, 0.0, 1.0) * (0.5 + 0.5 * np.cos(2.0 * np.pi * xc / 16.0e3))
    f["hi"][:] = 1.5 * f["cn"]
    f["ui"][:] = 0.1
    f["vi"][:] = -0.05
    f["sss"][:] = 33.0 + 2.0 * np.cos(2.0 * np.pi * yc / 20.0e3)
    st["ocean_depth"][:] = 150.0 + 3000.0 * np.cos(np.pi * xc / 16.0e3) ** 2
    # sst stays the profile's -0.5 outside the band: between 0 and about 3 degrees the convective melt of these 3-6 km wide
    # bergs takes 1e-7 of their mass a step, and the diagnostic of it (a difference of two masses) is then good to 1e-9 of
    # itself in the oracle's own double arithmetic -- the tolerance of the planes
    f["sst"][(yc > 4.0e3) & (yc < 7.0e3)] = -2.2
    st["msk"][yc < 4.0e3] = 0.0   # a coast along the south of the channel, next to the southernmost bergs (coastal_drift)
    _scrub(grid)
    return grid, p, b


@functools.lru_cache(maxsize=None)
def _bonded():
    grid, p, b, bd = S.config_c4()
    S.set_diag_all(p)
    return grid, p, b, bd


def _vary(base, b, inputs):
    n = int(b.get("_n", len(b["lon"])))
    if inputs == "static":
        b["static_berg"][0:n:4] = 1.0
    elif inputs == "narrow":
        k = np.arange(0, n, 3)
        rng = np.random.default_rng(11)
        b["width"][k] = b["thickness"][k] * rng.uniform(0.3, 1.4, len(k))
        b["length"][k] = b["width"][k] * rng.uniform(1.0, 1.5, len(k))
        b["mass"][k] = b["thickness"][k] * b["width"][k] * b["length"][k] * S.RHO_BERGS
        b["start_mass"][k] = b["mass"][k]
    else:
        assert inputs == "", inputs
    return b


def build(base, inputs=""):
    """Fresh copies of (grid, params, bergs[, bonds]) of a base; the grid's arrays are shared and never written."""
    if base == "bonded":
        grid, p, b, bd = _bonded()
        assert inputs == ""
        return grid, S.params_copy(p), S.copy_bergs(b), S.copy_bonds(bd)
    grid, p, b = {"plain": _plain, "flprof": _flprof}[base]()
    return grid, S.params_copy(p), _vary(base, S.copy_bergs(b), inputs)


def with_settings(p, settings):
    q = S.params_copy(p)
    for k, v in settings.items():
        assert hasattr(q, k), k
        setattr(q, k, v)
    return q


def nudged(b):
    """Every berg one ulp further north-east: what the conditioning check of a case runs the oracle on again."""
    q = S.copy_bergs(b)
    for f in ("lon", "lat", "lon_old", "lat_old"):
        q[f] = np.nextafter(b[f], np.inf)
    return q


# ---------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------
_ISM = dict(melt_icebergs_as_ice_shelf=1, Use_three_equation_model=1, const_gamma=1)
_DIAG_ALL = (1 << 20) - 1


_SPREAD = dict(add_weight_to_ocean=1)   # the footloose profile spreads no mass onto the ocean by itself


def _both(name, settings, inputs="", also_fl=None):
    return [Case(name, "plain", settings, inputs), Case(name, "flprof", settings, inputs, also_fl)]


def _per_berg_cases():
    c = []
    c += _both("ice_shelf", dict(_ISM))
    # the variants of the ice-shelf melt: `also` switches it on, so that the sensitivity is the variant's own
    for name, st in (("ice_shelf_var_gamma", dict(const_gamma=0)),
                     ("ice_shelf_two_eq", dict(Use_three_equation_model=0)),
                     ("ice_shelf_ml_salinity", dict(use_mixed_layer_salinity_for_thermo=1)),
                     ("ice_shelf_tide", dict(utide_icebergs=0.05)),
                     ("ice_shelf_cutoff", dict(melt_cutoff=50.0, apply_thickness_cutoff_to_bergs_melt=1)),
                     ("ice_shelf_gamma_t", dict(Gamma_T_3EQ=0.03)),
                     ("ice_shelf_ustar", dict(const_gamma=0, cdrag_icebergs=3.0e-3, ustar_icebergs_bg=0.004))):
        c += [Case(name, b, dict(st, melt_cutoff=500.0) if (b, name) == ("flprof", "ice_shelf_cutoff") else st, "", dict(_ISM))
              for b in ("plain", "flprof")]   # (flprof has the cutoff on at 10 m: 50 m reaches the same cells of its 1 km grid)
    c += _both("mixed_melting", dict(use_mixed_melting=1), inputs="static")
    # (without static bergs the blend only moves the convective melt into the erosion term, which leaves the new dimensions
    # what they were up to rounding)
    c += _both("sicn_shift", dict(sicn_shift=0.1))
    c += _both("coastal_drift", dict(coastal_drift=0.05))
    c += _both("velocity_override", dict(override_iceberg_velocities=1, u_override=0.2, v_override=-0.1))
    c += _both("ocean_drag_scale", dict(ocean_drag_scale=2.5))
    # cdrag_grounding = 1e-3 moves the oracle by 1e-9 only: the drag is raised until the case is sensitive
    c += _both("grounding", dict(cdrag_grounding=1.0, h_to_init_grounding=50.0))
    c += _both("grounding_fraction", dict(grounding_fraction=0.5), also_fl=_SPREAD)
    c += _both("clipping_depth", dict(clipping_depth=0.05), also_fl=_SPREAD)
    # the two forms give the same new dimensions up to rounding; what differs is how the loss is divided between the
    # three melt terms, which without bergy bits and footloose only the diagnostics see
    # (footloose refuses use_operator_splitting = F, FW:1476: no flprof case)
    c += [Case("no_operator_splitting", "plain", dict(use_operator_splitting=0), "", dict(diag_mask=_DIAG_ALL))]
    c += _both("no_rolling", dict(allow_bergs_to_roll=0), inputs="narrow")
    # tip_parameter = 0.5 is read by the updated rolling scheme only, = 999 selects scheme 2 of the old one
    c += [Case("tip_0.5", "plain", dict(tip_parameter=0.5), "narrow", dict(use_updated_rolling_scheme=1)),
          Case("tip_0.5", "flprof", dict(tip_parameter=0.5), "narrow"),
          Case("tip_999", "plain", dict(tip_parameter=999.0), "narrow"),
          Case("tip_999", "flprof", dict(tip_parameter=999.0), "narrow", dict(use_updated_rolling_scheme=0))]
    c += _both("bergy_bits", dict(bergy_bit_erosion_fraction=0.5))
    # the remaining members of KID_SWITCHES, each by itself at its other value
    c += [Case("old_bug_bilin", "plain", dict(old_bug_bilin=0), ""), Case("old_bug_bilin", "flprof", dict(old_bug_bilin=1), "")]
    c += [Case("new_predictive_corrective", "plain", dict(use_new_predictive_corrective=1), "")]
    c += _both("hexagonal", dict(hexagonal_icebergs=1), also_fl=_SPREAD)
    c += _both("speed_limit", dict(speed_limit=0.01))
    c += [Case("f_plane", "plain", dict(use_f_plane=1), "")]
    c += [Case("updated_rolling", "plain", dict(use_updated_rolling_scheme=1), "narrow"),
          Case("updated_rolling", "flprof", dict(use_updated_rolling_scheme=0), "narrow")]
    c += _both("melt_rates_zero", dict(set_melt_rates_to_zero=1))
    c += _both("diag_all", dict(diag_mask=_DIAG_ALL))
    c += _both("melt_without_decay", dict(Iceberg_melt_without_decay=1))
    c += [Case("old_spreading", "plain", dict(use_old_spreading=0), ""), Case("old_spreading", "flprof", dict(use_old_spreading=1), "", _SPREAD)]
    c += [Case("weight_to_ocean", "plain", dict(add_weight_to_ocean=0), ""), Case("weight_to_ocean", "flprof", dict(add_weight_to_ocean=1), "")]
    c += [Case("time_average_weight", "plain", dict(time_average_weight=1), ""),
          Case("time_average_weight", "flprof", dict(time_average_weight=1), "", _SPREAD)]
    # (with footloose the library refuses it, KID_EUNSUPPORTED: no flprof case)
    c += [Case("melt_using_spread_mass", "plain", dict(find_melt_using_spread_mass=1), "")]
    # read at run time inside the folded builds
    # (the gridded cutoff reads the spread area, which only a diagnostic or the ocean model asks for)
    # (flprof has the cutoff on at 10 m, which no cell of its grid reaches)
    c += [Case("gridded_melt_cutoff", b, dict(melt_cutoff=m, apply_thickness_cutoff_to_gridded_melt=1), "",
               dict(diag_mask=_DIAG_ALL, add_weight_to_ocean=1)) for b, m in (("plain", 50.0), ("flprof", 500.0))]
    c += _both("rho_bergs", dict(rho_bergs=900.0))
    c += _both("dt", dict(dt=900.0))
    c += [Case("lat_ref", "plain", dict(lat_ref=-60.0), "", dict(use_f_plane=1)), Case("lat_ref", "flprof", dict(lat_ref=-50.0), "")]
    # outside KID_SWITCHES, but read by the host where it selects the build and the schedule
    c += _both("static_icebergs", dict(static_icebergs=1))
    c += _both("pass_fields_to_ocean_model", dict(pass_fields_to_ocean_model=1), also_fl=_SPREAD)
    c += [Case("initial_orientation", "plain", dict(initial_orientation=15.0), "", dict(hexagonal_icebergs=1)),
          Case("initial_orientation", "flprof", dict(initial_orientation=15.0), "", dict(_SPREAD, hexagonal_icebergs=1))]
    return c


PER_BERG = _per_berg_cases()

BONDED = [Case(n[0], "bonded", n[1], "", n[2] if len(n) > 2 else None) for n in (
    ("ignore_tangential_force", dict(ignore_tangential_force=1)),
    ("use_grounding_torque", dict(use_grounding_torque=1)),
    ("radius_based_drag", dict(radius_based_drag=1)),
    ("rev_mind", dict(rev_mind=1)),
    # the two forms differ by sin(theta) - theta of neighbouring elements: softer bonds bend enough for 1e-6
    ("orig_dem_moment_of_inertia", dict(orig_dem_moment_of_inertia=1), dict(dem_spring_coef=1.0e6)),
    ("no_broken_bonds_for_contact", dict(use_broken_bonds_for_substep_contact=0)),
    # the stresses at the end of a long step stay under the base's thresholds: lower ones, so that break_bonds_dem deletes bonds
    # (ice_bergs_framework_init clears use_broken_bonds_for_substep_contact with it, FW:1438-1447)
    ("no_break_on_sub_steps", dict(break_bonds_on_sub_steps=0, use_broken_bonds_for_substep_contact=0),
     dict(frac_thres_n=200.0, frac_thres_t=100.0)),
    ("no_short_step_grounding", dict(short_step_mts_grounding=0)),
    ("no_internal_bergs_for_drag", dict(internal_bergs_for_drag=0)),
    ("tang_crit_int_damp", dict(tang_crit_int_damp_on=1)),
    ("ice_shelf", dict(melt_icebergs_as_ice_shelf=1)),
    ("mixed_melting", dict(use_mixed_melting=1)),
    ("ocean_drag_scale", dict(ocean_drag_scale=2.5)),
    # a conglomerate in rigid translation keeps its bonds at exact multiples of 60 degrees, where the orientation from the
    # bonds (an average of angles modulo pi/3, IB:3829-3892) jumps with the last bit: spread with the initial orientation
    ("velocity_override", dict(override_iceberg_velocities=1, u_override=0.1, v_override=0.02), dict(rotate_icebergs_for_mass_spreading=0)),
    ("grounding_fraction", dict(grounding_fraction=0.5)),
    ("no_rotation_for_spreading", dict(rotate_icebergs_for_mass_spreading=0)),
)]

# Cases whose only effect on the oracle is a counter (the sensitivity condition compares that scalar instead of a field)
COUNTER_ONLY = {"speed_limit": "nspeeding_tickets"}
# bonded cases that exist to keep bonds from breaking: (broken != 0).sum() > 0 is not asked of them
NO_FRACTURE = set()

# The members of KID_SWITCHES (kid_device.hpp) with their (plain, footloose profile) values: a case that moves one of them
# off its base's value must leave the folded build.
KID_SWITCHES = dict(
    old_bug_bilin=(1, 0), coastal_drift=(0., 0.), cdrag_grounding=(0., 0.), use_new_predictive_corrective=(0, 1),
    iceberg_bonds_on=(0, 0), internal_bergs_for_drag=(0, 0), hexagonal_icebergs=(0, 0), speed_limit=(0., 0.),
    override_iceberg_velocities=(0, 0), use_f_plane=(0, 1), use_updated_rolling_scheme=(0, 1), tip_parameter=(0., 0.),
    use_mixed_melting=(0, 0), melt_icebergs_as_ice_shelf=(0, 0), set_melt_rates_to_zero=(0, 0), use_operator_splitting=(1, 1),
    footloose=(0, 1), bergy_bit_erosion_fraction=(0., 1.), diag_mask=(0, 0), allow_bergs_to_roll=(1, 1),
    Iceberg_melt_without_decay=(0, 0), grounding_fraction=(0., 0.), clipping_depth=(0., 0.), use_old_spreading=(1, 0),
    add_weight_to_ocean=(1, 0), time_average_weight=(0, 0), find_melt_using_spread_mass=(0, 0), mts=(0, 0), dem=(0, 0))


# Members of kid_params the library reads that no case above moves, and why (DESIGN.md section 4 lists them too).
_FAMILY = "selects a code family the existing parity tests run on both sides (BASELINE configs 1-4, the beam and collision runs)"
_MTS = "a number of the MTS/DEM interaction, varied between config_c4's variants and the beam runs of the existing tests"
_FL = "footloose calving: varied between the fl_bits / new_bergs / displaced / by_pe runs of test_c3_footloose*"
EXCLUDED = dict(
    pi="pinned FMS constant (SURVEY 8c)", omega="pinned FMS constant (SURVEY 8c)", HLF="pinned FMS constant (SURVEY 8c)",
    Rearth="pinned constant of the reference (FW:44)", tidal_drift="must stay 0: the stochastic stream is FMS's (SURVEY 8c)",
    current_year="a time stamp: only copied into start_year of new bergs (calving and footloose tests)",
    current_yearday="a time stamp: only copied into start_day of new bergs (calving and footloose tests)",
    initial_mass_s="the class table of the melt-by-class diagnostic and of calving (test_calving, diag_all runs)",
    initial_mass_n="the class table of the melt-by-class diagnostic and of calving (test_calving, diag_all runs)",
    use_roundoff_fix="acts only on a berg that sits on a cell edge to the last bit: no conditioned case exists",
    Runge_not_Verlet=_FAMILY, old_interp_flds_order=_FAMILY, iceberg_bonds_on=_FAMILY, dem=_FAMILY, mts=_FAMILY, footloose=_FAMILY,
    interactive_icebergs_on=_FAMILY, only_interactive_forces=_FAMILY, explicit_inner_mts=_FAMILY, dem_beam_test=_FAMILY,
    periodic_reentry=_FAMILY, fracture_criterion_stress=_FAMILY, constant_interaction_LW=_FAMILY, max_bonds=_FAMILY,
    fl_style=_FL, displace_fl_bergs=_FL, fl_init_child_xy_by_pe=_FL, fl_rng_seed=_FL, fl_youngs=_FL, fl_strength=_FL,
    new_berg_from_fl_bits_mass_thres=_FL,
    spring_coef=_MTS, contact_spring_coef=_MTS, contact_distance=_MTS, radial_damping_coef=_MTS, tangental_damping_coef=_MTS,
    convergence_tolerance=_MTS, constant_length=_MTS, constant_width=_MTS, dem_damping_coef=_MTS, poisson=_MTS,
    dem_tests_start_lon=_MTS, dem_tests_end_lon=_MTS, mts_sub_steps=_MTS, force_convergence=_MTS,
    critical_interaction_damping_on=_MTS, scale_damping_by_pmag=_MTS, contact_cells_lon=_MTS, contact_cells_lat=_MTS)


def members_read_by_the_library():
    """The members of kid_params that the sources under icebergs_amd/csrc name."""
    import glob
    import os
    import re
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "icebergs_amd", "csrc")
    src = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(here, "*"))) if f.endswith((".hip", ".hpp", ".inc")))
    return [m for m, _ in T.Params._fields_ if re.search(r"(\bp\.|\bpp->|\bp->|params\.|Sw<K>::)%s\b" % re.escape(m), src)]


def members_moved_by_a_case():
    out = set()
    for c in PER_BERG + BONDED:
        out |= set(all_settings(c))
    return out


def all_settings(case):
    """`also` (inputs the switch needs, shared with the run the sensitivity is measured against) and the case's own"""
    return dict(case.also or {}, **case.settings)


def stays_folded(case):
    """True when the case leaves every KID_SWITCHES member at its base's value and adds no static berg: the host then
    still selects the folded build (K = 1 for plain, K = 2 for flprof), and the case is run once more with
    KID_NO_PLAIN_BUILD so that the general build K = 0 is held to the oracle at the same value."""
    col = {"plain": 0, "flprof": 1}[case.base]
    st = all_settings(case)
    return case.inputs != "static" and not st.get("pass_fields_to_ocean_model") and \
        all(k not in KID_SWITCHES or v == KID_SWITCHES[k][col] for k, v in st.items())


def moves_one_switch(case):
    """The KID_SWITCHES member a case moves alone (None when it moves none or more than one)."""
    col = {"plain": 0, "flprof": 1}[case.base]
    moved = [k for k, v in case.settings.items() if k in KID_SWITCHES and v != KID_SWITCHES[k][col]]
    return moved[0] if len(moved) == 1 and case.inputs != "static" and not case.also else None


def runs_phase_by_phase(case):
    """The phase entry points do not gather grd%spread_mass_old (IB:5490-5503): kid_thermodynamics refuses the switch."""
    return not all_settings(case).get("find_melt_using_spread_mass")


def case_id(c):
    return "%s-%s" % (c.base, c.name)


# ---------------------------------------------------------------------------------------------------------
# oracle runs, shared by the tests of one session and never written to
# ---------------------------------------------------------------------------------------------------------
_ORACLE = collections.OrderedDict()   # the runs of the bases stay; of the others the last few (a plain run holds ~40 MB of planes)


def oracle_run(base, settings, inputs="", nudge=False, keep=False):
    key = (base, tuple(sorted(settings.items())), inputs, nudge)
    if key in _ORACLE:
        _ORACLE.move_to_end(key)
        _ORACLE[key][1] |= keep
        return _ORACLE[key][0]
    if base == "bonded":
        grid, p, b, bd = build(base)
        run = P.run_oracle_mts(grid, with_settings(p, settings), nudged(b) if nudge else b, bd, NSTEPS)
    else:
        grid, p, b = build(base, inputs)
        run = P.run_oracle(grid, with_settings(p, settings), nudged(b) if nudge else b, NSTEPS)
    _ORACLE[key] = [run, keep]
    loose = [k for k, v in _ORACLE.items() if not v[1]]
    for k in loose[:-4]:
        del _ORACLE[k]
    return run


def by_id(b):
    """Rows of the live bergs in the order of their ids."""
    n = int(b.get("_n", len(b["lon"])))   # (an oracle run with footloose calving counts the children it appended)
    live = np.nonzero(b["alive"][:n] != 0)[0]
    return live[np.argsort(b["id"][live], kind="stable")]


def differences(ref, got, fields):
    """Largest relative difference between two runs (berg tuple, acc, out, scalars) per compared quantity: the berg
    fields matched by id, every accumulator plane over its acc_scales, every output plane.  inf where the sets of
    surviving bergs differ."""
    rb, gb = ref[0], got[0]
    ro, go = by_id(rb), by_id(gb)
    rep = {}
    if not np.array_equal(rb["id"][ro], gb["id"][go]):
        rep["survivors"] = float("inf")
    else:
        for f in fields:
            rep[f] = P.rel_err(gb[f][go].astype(np.float64), rb[f][ro].astype(np.float64))
    sc = P.acc_scales(ref[1])
    for k in range(ref[1].shape[0]):
        rep["acc%d" % k] = P.acc_err(got[1], ref[1], k, sc)
    for k in range(ref[2].shape[0]):
        rep["out%d" % k] = P.rel_err(got[2][k], ref[2][k])
    return rep


def finite(run):
    b = run[0]
    rows = by_id(b)
    ok = all(np.isfinite(b[f][rows]).all() for f in T.BERG_F64_NAMES)
    return bool(ok and np.isfinite(run[1]).all() and np.isfinite(run[2]).all() and np.isfinite(run[3]).all())
