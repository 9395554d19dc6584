"""kid_icebergs_stock_pe and kid_icebergs_incr_mass of the Fortran glue (icebergs_stock_pe IB:8102-8133, icebergs_incr_mass
IB:6046-6074 behind their argument lists): namelist -> kid_icebergs_init -> three kid_icebergs_run -> both stocks and the
increment of a zero plane, against the Python host driving the same library through the same calls on the same population.

The two hosts are two handles in two processes, and their rows are not in the same order (the glue flattens per-cell lists, the
re-binning places the rows of a cell in the order its atomics arrive).  In the default mode that would leave the last bits of
grd%spread_mass (fp64 atomics across waves) and of the tree sums (their bits follow the row layout) free to differ
between the two.  Both sides therefore turn reproducible sums on (kid_set_reproducible_sums; config 1 sets none of mts,
interactive_icebergs_on, footloose): every per-cell sum and every budget sum is then a function of the set of bergs only
(kid_repro.inc), each berg's own arithmetic never depends on its row, and the library, the kernels and the shape of
the reduction are the same -- so the numbers must be equal bit for bit."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from icebergs_amd import synthetic as S
from icebergs_amd import types as T
from test_fortran_gpu import icebergs_nml_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET = os.path.join(ROOT, "icebergs_amd", "fortran", "kid_budget_test")
MAGIC = 1263093767


def _write_case(path, gni, gnj, nsteps, gridres, dt, sst, sss, cap, b):
    n = len(b["lon"])
    with open(path, "wb") as f:
        f.write(struct.pack("<5i", MAGIC, gni, gnj, 0, nsteps))
        f.write(struct.pack("<4d", gridres, dt, sst, sss))
        f.write(struct.pack("<qq", cap, n))
        for name in T.BERG_F64_NAMES:
            f.write(np.ascontiguousarray(b[name], dtype=np.float64).tobytes())
        for name in T.BERG_I32_NAMES:
            f.write(np.ascontiguousarray(b[name], dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(b["id"], dtype=np.int64).tobytes())


def _read_result(path, gni, gnj):
    with open(path, "rb") as f:
        d = T.GridDesc.from_buffer_copy(f.read(C.sizeof(T.GridDesc)))
        p = T.Params.from_buffer_copy(f.read(C.sizeof(T.Params)))
        ni, nj = d.ied - d.isd + 1, d.jed - d.jsd + 1
        st = {name: np.frombuffer(f.read(8 * ni * nj), dtype=np.float64).reshape(nj, ni).copy() for name in T.GRID_STATIC_NAMES}
        water, heat, total = struct.unpack("<3d", f.read(24))
        plane = np.frombuffer(f.read(8 * gni * gnj), dtype=np.float64).reshape(gnj, gni).copy()
        assert f.read() == b""
    return d, p, st, water, heat, total, plane


@pytest.mark.gpu
def test_glue_stock_pe_and_incr_mass(tmp_path):
    from icebergs_amd.framework import Icebergs
    gni = gnj = 20
    nsteps, sst, sss, gridres = 3, 2.0, 34.0, 1000.0
    grid, p, b = S.config_c1(n=300, seed=5)
    p.bergy_bit_erosion_fraction = 0.5
    b["heat_density"][:] = 3.0e5
    b["mass_of_bits"][:] = 0.05 * b["mass"]
    n = len(b["lon"])
    (tmp_path / "input.nml").write_text(icebergs_nml_text(p, grid["desc"], halo=4, debug=".false."))
    perm = np.random.default_rng(8).permutation(n)                 # file order is not list order
    sh = {k: (v[perm].copy() if hasattr(v, "dtype") and len(v) == n else v) for k, v in b.items()}
    case, res = str(tmp_path / "budget.bin"), str(tmp_path / "budget.out")
    _write_case(case, gni, gnj, nsteps, gridres, p.dt, sst, sss, n, sh)
    r = subprocess.run([BUDGET, case, res], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    d, fp, st, water, heat, total, plane = _read_result(res, gni, gnj)
    printed = [float(x) for x in re.findall(r"kid_budget_test: \S+ \S+\s+=\s*(\S+)", r.stdout)]
    assert printed[:2] == [water, heat], r.stdout                  # 17 digits after the point: the text round-trips
    assert printed[2] == total
    # the Python host: the grid and the parameters kid_icebergs_init derived, the bergs in the order the glue flattens its lists
    # in (place_bergs returns them in that order), the calls of kid_icebergs_run in its order
    ib = Icebergs({"desc": d, "static": st, "forcing": {k: np.zeros_like(st["lon"]) for k in T.FORCING_NAMES}}, fp, capacity=n)
    try:
        ib.set_reproducible_sums(True)                             # as kid_budget_test.F90 does after kid_icebergs_init
        ib.set_calving_params(S.calving_params(fp))
        ib.upload_bergs(b)
        zero_h = np.zeros((gnj + 2, gni + 2))
        zero_c = np.zeros((gnj, gni))
        args = {"uo": zero_h, "vo": zero_h, "ui": zero_h, "vi": zero_h, "tauxa": zero_c, "tauya": zero_c, "ssh": zero_h, "cn": zero_h, "hi": zero_h,
                "sst": zero_c + sst, "sss": zero_c + sss}
        for s in range(nsteps):
            fp.current_year, fp.current_yearday = 1, s * fp.dt / 86400.0
            ib.set_params(fp)
            ib.ingest_forcing(args, "B", "B", tau_is_velocity=False, cyclic_x=d.Lx > 0.0)
            ib.calving(zero_c.copy(), zero_c.copy())
            ib.step_local()
            ib.step_gather()
            ib.fetch()
        want_water, want_heat = ib.stock(T.ENUMS["KID_STOCK_WATER"]), ib.stock(T.ENUMS["KID_STOCK_HEAT"])
        want_plane = ib.incr_mass(np.zeros((gnj, gni)))
        bud = ib.budget()
    finally:
        ib.close()
    print("fortran water %.17g heat %.17g; python water %.17g heat %.17g; plane max |diff| %.3g of %.6g" %
          (water, heat, want_water, want_heat, np.abs(plane - want_plane).max(), want_plane.max()))
    assert bud["nbergs"] == n and want_water > 0.0 and want_plane.max() > 0.0
    assert water == want_water and heat == want_heat
    assert np.array_equal(plane, want_plane)
    assert abs(total - float(want_plane.sum())) <= 1.0e-12 * total   # Fortran's sum() and numpy's add in their own orders
