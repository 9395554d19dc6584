"""Device-side budgets: kid_budget, kid_stock, kid_incr_mass (include/kid.h, icebergs_amd/csrc/kid_budget.inc).

Expected values are independent sums: the test downloads the bergs and the calving state, keeps the live rows whose cell is on
the computational domain, forms the terms of sum_mass / sum_heat (icebergs_framework.F90:6606-6666) in numpy and adds them with
math.fsum, which is exactly rounded.

Tolerance.  The device adds non-negative terms in a tree of fixed shape; a sum whose longest chain of additions has `depth`
links differs from the exact sum by at most about depth * 2^-53 * sum|x|.  The chain of the berg sums is 6 (wave butterfly) +
2 (four waves) + ceil(blocks / 256) (the finishing thread's serial adds) + 8 (finishing block), blocks = ceil(rows / 256): 17
below 2^16 rows.  The stored-ice sum adds 9 class additions in front and has 282 blocks of cells on the 360 x 200 grid: 27.
Forming a term costs at most 4 more roundings, identical on both sides.  All of that is below the 64 the assertions use:
|got - fsum| <= 64 * 2^-53 * sum|x|, the bound computed from the data of each case.

What the reference's expressions do and do not depend on (icebergs.F90:8102-8133): both stocks are built from sum_mass(bergs)
without optional argument, i.e. bergs, bergy bits, footloose bits and footloose bergy bits together, always; no switch selects
a branch and the heat stock is -(mass) * HLF, not heat_density * mass.  The stock tests therefore run one population that
carries bits and one that carries none against that one expression; the justbergs / justbits / justflbits branches of
sum_mass are members of kid_budget and are checked there."""
import ctypes as C
import math

import numpy as np
import pytest

from icebergs_amd import synthetic as S
from icebergs_amd import types as T

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
KID_EINVAL = -1
WATER, HEAT = T.ENUMS["KID_STOCK_WATER"], T.ENUMS["KID_STOCK_HEAT"]
SUMS = ("floating_mass", "icebergs_mass", "bergy_mass", "fl_bits_mass", "floating_heat")


def _depth(rows, lead=0):
    blocks = -(-rows // 256)
    return lead + 8 + -(-blocks // 256) + 8


def _close(got, terms, label, scale=1.0, depth=0):
    """|got - scale * fsum(terms)| <= 64 * 2^-53 * sum|terms| * |scale|"""
    terms = np.asarray(terms, dtype=np.float64).ravel()
    exact = math.fsum(terms) * scale
    bound = 64.0 * U * math.fsum(np.abs(terms)) * abs(scale)
    print("%-28s got %.17g exact %.17g |diff| %.3g bound %.3g depth %d" % (label, got, exact, abs(got - exact), bound, depth))
    assert depth + 6 <= 64, (label, depth)
    assert abs(got - exact) <= bound, (label, got, exact, bound)


def _on_domain(d, b):
    return (b["alive"] != 0) & (b["ine"] >= d.isc) & (b["ine"] <= d.iec) & (b["jne"] >= d.jsc) & (b["jne"] <= d.jec)


def _terms(d, b):
    """the per-berg terms of sum_mass / sum_heat for the rows that count, in the reference's operation order"""
    on = _on_domain(d, b)
    m, ms, bits = b["mass"][on], b["mass_scaling"][on], b["mass_of_bits"][on]
    flb, flbb, hd = b["mass_of_fl_bits"][on], b["mass_of_fl_bergy_bits"][on], b["heat_density"][on]
    dm = (m + bits + flb + flbb) * ms                   # FW:6627
    return {"floating_mass": dm, "icebergs_mass": m * ms, "bergy_mass": (bits + flbb) * ms, "fl_bits_mass": flb * ms,   # FW:6621-6625
            "floating_heat": dm * hd, "nbergs": int(on.sum())}                                                            # FW:6661


def _stored_terms(ib):
    d = ib.grid["desc"]
    if getattr(ib, "_calv_params", None) is None:
        return np.zeros(0), np.zeros(0)
    st = ib.get_calving_state()
    js, je, i_s, ie = d.jsc - d.jsd, d.jec - d.jsd + 1, d.isc - d.isd, d.iec - d.isd + 1
    return st["stored_ice"][:, js:je, i_s:ie].copy(), st["stored_heat"][js:je, i_s:ie].copy()


def _snapshot(ib):
    """every answer of the feature, then the independent data they are checked against (the downloads come last)"""
    r = {"budget": ib.budget(), "budget2": ib.budget(), "water": ib.stock(WATER), "heat": ib.stock(HEAT)}
    r["slots"] = ib.num_bergs()[0]
    r["scalars"] = ib.fetch()[2].copy()
    r["bergs"] = ib.download_bergs()
    r["alive"] = int((r["bergs"]["alive"] != 0).sum())
    r["ice"], r["sheat"] = _stored_terms(ib)
    r["desc"], r["HLF"] = ib.grid["desc"], ib.params.HLF
    return r


def _check_snapshot(r, label):
    t = _terms(r["desc"], r["bergs"])
    bud = r["budget"]
    assert bud == r["budget2"], (label, "two calls in a row differ")
    assert bud["nbergs"] == t["nbergs"], (label, bud["nbergs"], t["nbergs"])
    dep = _depth(max(r["slots"], 1))
    for name in SUMS:
        _close(bud[name], t[name], label + "/" + name, depth=dep)
    ncomp = (r["desc"].iec - r["desc"].isc + 1) * (r["desc"].jec - r["desc"].jsc + 1)
    dep_c = _depth(ncomp, lead=9)
    _close(bud["stored"], r["ice"], label + "/stored", depth=dep_c)
    _close(bud["stored_heat"], r["sheat"], label + "/stored_heat", depth=dep_c)
    sc = r["scalars"]
    assert bud["net_heat_to_ocean"] == sc[T.SCALAR_NAMES["net_heat_to_ocean"]]
    assert bud["nbergs_melted"] == int(sc[T.SCALAR_NAMES["nbergs_melted"]])
    assert bud["nbergs_calved_fl"] == int(sc[T.SCALAR_NAMES["nbergs_calved_fl"]])
    assert bud["nspeeding_tickets"] == int(sc[T.SCALAR_NAMES["nspeeding_tickets"]])
    # the stocks: IB:8121, 8126, from the same sweep
    assert r["water"] == bud["stored"] + bud["floating_mass"], label
    assert r["heat"] == -(bud["stored"] + bud["floating_mass"]) * r["HLF"], label
    both = np.concatenate([np.ravel(r["ice"]), t["floating_mass"]])
    _close(r["water"], both, label + "/stock water", depth=max(dep, dep_c) + 1)
    _close(r["heat"], both, label + "/stock heat", scale=-r["HLF"], depth=max(dep, dep_c) + 2)
    return t


def _calving_state(grid, seed=5, cells=40):
    """non-zero buckets in a few dozen cells of the computational domain and in some halo cells, which must not count"""
    d = grid["desc"]
    nj, ni = d.jed - d.jsd + 1, d.ied - d.isd + 1
    rng = np.random.default_rng(seed)
    ice, heat = np.zeros((10, nj, ni)), np.zeros((nj, ni))
    jj = rng.integers(d.jsc - d.jsd, d.jec - d.jsd + 1, cells)
    ii = rng.integers(d.isc - d.isd, d.iec - d.isd + 1, cells)
    ice[:, jj, ii] = rng.uniform(1.0e6, 8.0e10, (10, cells))
    heat[jj, ii] = -rng.uniform(1.0e10, 5.0e15, cells)
    for (j, i) in ((0, 0), (1, 5), (nj - 1, ni - 1), (d.jsc - d.jsd + 3, 1), (nj - 2, d.isc - d.isd + 7), (d.jsc - d.jsd - 1, d.isc - d.isd)):
        ice[:, j, i] = 7.0e10
        heat[j, i] = -3.0e15
    return ice, heat


def _c2_run(n, bits, nsteps=3, calving=True, seed=11):
    from icebergs_amd.framework import Icebergs
    grid, p, b = S.config_c2(n=n, seed=seed, continents=True)
    b["heat_density"][:] = 3.0e5
    if bits:
        p.bergy_bit_erosion_fraction = 0.5
        b["mass_of_bits"][:] = 0.03 * b["mass"] * (1.0 + (np.arange(n) % 7))
    ib = Icebergs(grid, p, capacity=max(n, 1))
    try:
        if calving:
            ib.set_calving_params(S.calving_params(p))
            ib.set_calving_state(*_calving_state(grid))
        ib.upload_bergs(b)
        ib.run(nsteps)
        return _snapshot(ib)
    finally:
        ib.close()


@pytest.fixture(scope="module")
def with_bits():
    return _c2_run(5000, bits=True)


def test_stocks_with_bits(with_bits):
    t = _check_snapshot(with_bits, "c2-5000-bits")
    assert math.fsum(t["bergy_mass"]) > 0.0 and with_bits["budget"]["stored"] > 0.0 and with_bits["water"] > 0.0
    assert with_bits["heat"] < 0.0


def test_stocks_without_bits():
    r = _c2_run(5000, bits=False)
    _check_snapshot(r, "c2-5000-nobits")
    assert r["budget"]["bergy_mass"] == 0.0 and r["budget"]["fl_bits_mass"] == 0.0
    assert r["budget"]["floating_mass"] == r["budget"]["icebergs_mass"]


def test_budget_members(with_bits):
    r = with_bits
    _check_snapshot(r, "c2-5000-bits")
    bud = r["budget"]
    assert set(bud) == {name for name, _ in T.BudgetOut._fields_}
    assert bud["nbergs"] == r["alive"] > 0          # config 2 keeps its bergs inside the computational domain
    assert bud["floating_heat"] > 0.0 and bud["stored_heat"] < 0.0 and bud["net_heat_to_ocean"] != 0.0


@pytest.mark.parametrize("n", [5001, 1])
def test_budget_ragged_and_single(n):
    r = _c2_run(n, bits=True, nsteps=2, calving=False)
    _check_snapshot(r, "c2-%d" % n)
    assert r["budget"]["stored"] == 0.0 and r["budget"]["stored_heat"] == 0.0   # no calving state: zero stored ice
    assert r["budget"]["nbergs"] == r["alive"]


def test_budget_empty_handle():
    from icebergs_amd.framework import Icebergs
    grid, p, b = S.config_c2(n=4, seed=1)
    ib = Icebergs(grid, p, capacity=16)
    try:
        bud = ib.budget()
        assert all(v == 0 for v in bud.values()), bud
        assert ib.stock(WATER) == 0.0 and ib.stock(HEAT) == 0.0
        ib.set_calving_params(S.calving_params(p))
        ib.set_calving_state(*_calving_state(grid))
        _check_snapshot(_snapshot(ib), "empty+stored")   # stored ice alone
    finally:
        ib.close()


def test_budget_dead_rows_and_halo_rows():
    """dead rows before compaction do not count; live rows planted in halo cells do not count either"""
    from icebergs_amd.framework import Icebergs
    grid, p, b = S.config_c2(n=3000, seed=4)
    d = grid["desc"]
    b["heat_density"][:] = 3.0e5
    b["mass_of_bits"][:] = 0.1 * b["mass"]
    b["mass_of_fl_bits"][:] = 0.02 * b["mass"]
    b["mass_of_fl_bergy_bits"][:] = 0.005 * b["mass"]
    b["alive"][::7] = 0
    b["mass"][::14] = np.nan                                   # what a dead row holds is never read as a term
    halo = np.arange(3, 3000, 11)
    halo = halo[b["alive"][halo] != 0]
    b["ine"][halo[0::4]] = d.isc - 1
    b["ine"][halo[1::4]] = d.iec + 1
    b["jne"][halo[2::4]] = d.jsc - 1
    b["jne"][halo[3::4]] = d.jec + 1
    b["halo_berg"][halo] = 1.0
    ib = Icebergs(grid, p, capacity=3000)
    try:
        ib.set_resort_interval(0)
        ib.upload_bergs(b)
        r = _snapshot(ib)
    finally:
        ib.close()
    t = _check_snapshot(r, "dead+halo")
    assert t["nbergs"] == int((b["alive"] != 0).sum()) - len(halo)
    assert r["budget"]["nbergs"] < r["alive"] < 3000


def test_budget_footloose_members():
    from icebergs_amd.framework import Icebergs
    grid, p, b = S.config_c3(n=300, fl_style="fl_bits")
    ib = Icebergs(grid, p, capacity=len(b["lon"]))
    try:
        ib.upload_bergs(b)
        ib.run(20)
        r = _snapshot(ib)
    finally:
        ib.close()
    on = _on_domain(r["desc"], r["bergs"])
    assert (r["bergs"]["mass_of_fl_bits"][on] > 0.0).any() and (r["bergs"]["mass_of_fl_bergy_bits"][on] > 0.0).any()
    _check_snapshot(r, "c3-fl_bits")
    assert r["budget"]["fl_bits_mass"] > 0.0 and r["budget"]["bergy_mass"] > 0.0


def _c2_weight(n=5000, seed=13):
    grid, p, b = S.config_c2(n=n, seed=seed, continents=True)
    p.add_weight_to_ocean = 1
    return grid, p, b


def test_incr_mass():
    import torch
    from icebergs_amd.framework import Icebergs
    grid, p, b = _c2_weight()
    d = grid["desc"]
    nic, njc = d.iec - d.isc + 1, d.jec - d.jsc + 1
    ib = Icebergs(grid, p, capacity=len(b["lon"]))
    try:
        ib.upload_bergs(b)
        ib.run(1)
        _, out, _ = ib.fetch()
        spread = out[T.OUT_NAMES["spread_mass"]][d.jsc - d.jsd:d.jec - d.jsd + 1, d.isc - d.isd:d.iec - d.isd + 1].copy()
        assert spread.max() > 0.0
        ramp = 1.0e3 + 0.125 * np.arange(nic * njc, dtype=np.float64).reshape(njc, nic)
        want = ramp + spread                                   # IB:6067, one add per cell
        dev = torch.from_numpy(ramp.copy()).to("cuda:%d" % ib.device)
        ib.incr_mass(dev)
        got = dev.cpu().numpy()
        print("incr_mass max |got - want| %.3g, plane max %.6g" % (np.abs(got - want).max(), np.abs(want).max()))
        assert np.abs(got - want).max() <= 1.0e-15 * np.abs(want).max()
        host = ramp.copy()
        ib.incr_mass(host)
        assert np.array_equal(host, got), "host-pointer route and device route differ"
        # a wrong shape
        bad = np.zeros((njc, nic + 1))
        assert ib.lib.kid_incr_mass(ib.h, bad.ctypes.data, 0, nic + 1, njc) == KID_EINVAL
        assert ib.lib.kid_incr_mass(ib.h, host.ctypes.data, 0, njc, nic) == KID_EINVAL
        assert ib.lib.kid_incr_mass(ib.h, dev.data_ptr(), 1, nic, njc - 1) == KID_EINVAL
        assert np.array_equal(dev.cpu().numpy(), got)
        # without add_weight_to_ocean the routine returns before the loop (IB:6057): the plane is unchanged
        q = S.params_copy(p)
        q.add_weight_to_ocean = 0
        ib.set_params(q)
        dev2 = torch.from_numpy(ramp.copy()).to("cuda:%d" % ib.device)
        host2 = ramp.copy()
        ib.incr_mass(dev2)
        ib.incr_mass(host2)
        assert np.array_equal(dev2.cpu().numpy(), ramp) and np.array_equal(host2, ramp)
    finally:
        ib.close()


def _state(ib):
    """live bergs in id order (the order of the rows inside a cell after a re-binning is the order its atomics arrived in:
    include/kid.h, results never depend on it), planes, scalars"""
    acc, out, scal = ib.fetch()
    got = ib.download_bergs()
    live = np.nonzero(got["alive"] != 0)[0]
    live = live[np.argsort(got["id"][live], kind="stable")]
    return {k: v[live].copy() for k, v in got.items()}, acc.copy(), out.copy(), scal.copy()


def test_no_side_effects_and_repeatability():
    from icebergs_amd.framework import Icebergs
    grid, p, b = S.config_c2(n=5000, seed=17, continents=True)
    S.set_diag_all(p)
    b["heat_density"][:] = 3.0e5
    res = []
    for with_budget in (False, True):
        ib = Icebergs(grid, p, capacity=len(b["lon"]))
        try:
            ib.set_resort_interval(3)
            ib.set_reproducible_sums(True)
            ib.upload_bergs(b)
            for _ in range(8):
                ib.run(1)
                if with_budget:
                    a, c = ib.budget(), ib.budget()
                    assert a == c and a["nbergs"] > 0
                    assert ib.stock(WATER) == ib.stock(WATER)
            res.append(_state(ib))
        finally:
            ib.close()
    (b0, acc0, out0, sc0), (b1, acc1, out1, sc1) = res
    for k in b0:
        assert np.array_equal(b0[k], b1[k], equal_nan=True), k
    assert np.array_equal(acc0, acc1) and np.array_equal(out0, out1) and np.array_equal(sc0, sc1)


def test_default_mode_repeatable_and_steps_unchanged():
    """default sums: two calls give the same bits, and the berg state after budget calls is that of a run without them"""
    from icebergs_amd.framework import Icebergs
    grid, p, b = S.config_c2(n=5000, seed=19, continents=True)
    res = []
    for with_budget in (False, True):
        ib = Icebergs(grid, p, capacity=len(b["lon"]))
        try:
            ib.set_resort_interval(2)
            ib.upload_bergs(b)
            for _ in range(5):
                ib.run(1)
                if with_budget:
                    assert ib.budget() == ib.budget()
            got = ib.download_bergs()
            o = np.argsort(got["id"], kind="stable")
            res.append({k: v[o] for k, v in got.items()})
        finally:
            ib.close()
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k], equal_nan=True), k


def test_row_order_unchanged(monkeypatch):
    """The calls do not change the order of rows.  Two runs in the default mode, one with the budget calls
    after every step, compared row for row: KID_STABLE_RESORT (read at kid_create) makes every re-binning a stable sort, so the two
    handles order their rows alike.  With a re-binning interval of 2, steps 2 and 4 leave the permutation pending for the hot
    build that follows; in the observed run the budget call applies it instead (rebin_flush), which kid_rebin_fused_count shows:
    the plain run fuses both re-binnings, the observed run none.  Then on one handle: download, every call of the feature,
    download again -- the same rows."""
    from icebergs_amd.framework import Icebergs
    monkeypatch.setenv("KID_STABLE_RESORT", "1")
    grid, p, b = S.config_c2(n=5001, seed=29)
    b["alive"][np.random.default_rng(3).choice(5001, 250, replace=False)] = 0
    d = grid["desc"]
    res, fused = [], []
    for with_budget in (False, True):
        ib = Icebergs(grid, p, capacity=5001)
        try:
            ib.set_resort_interval(2)
            ib.upload_bergs(b)
            for _ in range(5):
                ib.run(1)
                if with_budget:
                    ib.budget()
                    ib.stock(WATER)
                    ib.stock(HEAT)
            fused.append(ib.rebin_fused_count())
            got = ib.download_bergs()
            if with_budget:
                ib.budget()
                ib.stock(WATER)
                ib.stock(HEAT)
                ib.incr_mass(np.zeros((d.jec - d.jsc + 1, d.iec - d.isc + 1)))
                again = ib.download_bergs()
                for k in got:
                    assert np.array_equal(got[k], again[k], equal_nan=True), k
            res.append(got)
        finally:
            ib.close()
    assert fused == [2, 0], fused
    assert 0 < int((res[0]["alive"] != 0).sum()) <= 5001 - 250       # (the download's count drops the dead a re-binning sorted last)
    assert not np.array_equal(res[0]["id"], b["id"][:len(res[0]["id"])])        # the rows did move
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k], equal_nan=True), k


def _permuted(b, perm):
    return {k: (v[perm].copy() if isinstance(v, np.ndarray) and v.shape[:1] == b["lon"].shape else v) for k, v in b.items()}


def test_layout_invariance_in_reproducible_mode():
    from icebergs_amd.framework import Icebergs
    grid, p, b = S.config_c2(n=40000, seed=21, continents=True)
    b["heat_density"][:] = 3.0e5
    p.bergy_bit_erosion_fraction = 0.5
    b["mass_of_bits"][:] = 0.03 * b["mass"]
    ice, heat = _calving_state(grid)
    layouts = ((_permuted(b, np.lexsort((b["id"], b["ine"], b["jne"]))), 3, None),
               (_permuted(b, np.random.default_rng(99).permutation(len(b["lon"]))), 0, 2))
    res = []
    for bb, resort, compact_at in layouts:
        ib = Icebergs(grid, p, capacity=len(b["lon"]))
        try:
            ib.set_resort_interval(resort)
            ib.set_reproducible_sums(True)
            ib.set_calving_params(S.calving_params(p))
            ib.set_calving_state(ice, heat)
            ib.upload_bergs(bb)
            for step in range(4):
                ib.run(1)
                if compact_at == step:
                    ib.compact()
            res.append((ib.budget(), ib.stock(WATER), ib.stock(HEAT)))
        finally:
            ib.close()
    assert res[0][0]["nbergs"] > 0 and res[0][0]["bergy_mass"] > 0.0
    for name in res[0][0]:
        assert res[0][0][name] == res[1][0][name], (name, res[0][0][name], res[1][0][name])
    assert res[0][1] == res[1][1] and res[0][2] == res[1][2]


def test_mass_closure():
    """floating mass lost over one step = the area-weighted floating_melt plane times dt (thermodynamics IB:3114-3117), to the
    1e-9 tests/test_properties_gpu.py uses for the same balance"""
    from icebergs_amd.framework import Icebergs
    grid, p, b = S.config_c2(n=5000, seed=23)
    p.bergy_bit_erosion_fraction = 0.5
    b["mass_of_bits"][:] = 0.03 * b["mass"]
    ib = Icebergs(grid, p, capacity=len(b["lon"]))
    try:
        ib.upload_bergs(b)
        before = ib.budget()
        ib.run(1)
        after = ib.budget()
        acc, _, _ = ib.fetch()
    finally:
        ib.close()
    assert before["nbergs"] == 5000 and after["nbergs"] == 5000 and after["nbergs_melted"] == 0   # nobody left, nobody melted away
    lost = before["floating_mass"] - after["floating_mass"]
    received = float(np.sum(acc[T.ACC_NAMES["floating_melt"]] * grid["static"]["area"])) * p.dt
    print("mass closure: lost %.17g received %.17g rel %.3g (floating mass %.6g)" % (lost, received, abs(lost - received) / lost, before["floating_mass"]))
    assert lost > 0.0
    assert abs(received - lost) <= 1.0e-9 * lost, (lost, received)


def test_bad_arguments():
    from icebergs_amd.framework import Icebergs
    grid, p, b = S.config_c2(n=64, seed=1)
    d = grid["desc"]
    nic, njc = d.iec - d.isc + 1, d.jec - d.jsc + 1
    ib = Icebergs(grid, p, capacity=64)
    lib = ib.lib
    v, out, plane = C.c_double(1.5), T.BudgetOut(), np.zeros((njc, nic))
    try:
        ib.upload_bergs(b)
        for index in (0, 3, -1, 99):
            v.value = 1.5
            assert lib.kid_stock(ib.h, index, C.byref(v)) == KID_EINVAL
            assert v.value == 0.0                                  # the reference's `case default`, IB:8128-8129
        assert lib.kid_stock(ib.h, WATER, None) == KID_EINVAL
        assert lib.kid_budget(ib.h, None) == KID_EINVAL
        assert lib.kid_incr_mass(ib.h, None, 0, nic, njc) == KID_EINVAL
        assert lib.kid_stock(None, WATER, C.byref(v)) == KID_EINVAL
        assert lib.kid_budget(None, C.byref(out)) == KID_EINVAL
        assert lib.kid_incr_mass(None, plane.ctypes.data, 0, nic, njc) == KID_EINVAL
        assert lib.kid_stock(ib.h, WATER, C.byref(v)) == 0 and v.value > 0.0    # the handle is still usable
    finally:
        ib.close()
    # after close() the host layer holds None, so this is the null-handle check above once more: a pointer to a destroyed handle
    # is freed memory and cannot be passed in safely
    assert ib.h is None
    assert lib.kid_stock(ib.h, WATER, C.byref(v)) == KID_EINVAL
    assert lib.kid_budget(ib.h, C.byref(out)) == KID_EINVAL
    assert lib.kid_incr_mass(ib.h, plane.ctypes.data, 0, nic, njc) == KID_EINVAL
