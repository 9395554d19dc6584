"""The growable capacity through the Fortran glue (icebergs_amd/fortran/kid_reserve_test.F90): lists of 500 bergs, a handle
created for exactly 500, the calving source on and auto_reserve_growth handed to kid_icebergs_init; 20 kid_icebergs_run calve
several hundred bergs, the handle grows ahead of each of them and the staging arrays of the glue follow in kid_glue_unflatten.
The lists rebuilt at the end hold more than 500 bergs and are, berg for berg and bit for bit, those of the same run on a handle
whose capacity was given up front.  Bergs are matched by id: two bergs a cell calves from the same class in the same step
have equal `inorder` keys, and their order in the list follows the rows, which follow the order atomics arrive in."""
import os
import struct
import subprocess

import numpy as np
import pytest

from icebergs_amd import synthetic as S
from icebergs_amd import types as T
from test_fortran_gpu import icebergs_nml_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESERVE = os.path.join(ROOT, "icebergs_amd", "fortran", "kid_reserve_test")
MAGIC = 1263093768


def _write_case(path, gni, gnj, nsteps, gridres, dt, sst, sss, rate, growth, cap_tight, cap_roomy, min_free, b):
    n = len(b["lon"])
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", MAGIC, gni, gnj, nsteps))
        f.write(struct.pack("<6d", gridres, dt, sst, sss, rate, growth))
        f.write(struct.pack("<4q", cap_tight, cap_roomy, min_free, n))
        for name in T.BERG_F64_NAMES:
            f.write(np.ascontiguousarray(b[name], dtype=np.float64).tobytes())
        for name in T.BERG_I32_NAMES:
            f.write(np.ascontiguousarray(b[name], dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(b["id"], dtype=np.int64).tobytes())


def _read_run(f):
    cap_end, staging, m = struct.unpack("<3q", f.read(24))
    b = {name: np.frombuffer(f.read(8 * m), dtype=np.float64).copy() for name in T.BERG_F64_NAMES}
    for name in T.BERG_I32_NAMES:
        b[name] = np.frombuffer(f.read(4 * m), dtype=np.int32).copy()
    b["id"] = np.frombuffer(f.read(8 * m), dtype=np.int64).copy()
    return cap_end, staging, m, b


@pytest.mark.gpu
def test_glue_grows_with_the_calving_source(tmp_path):
    gni = gnj = 20
    n, nsteps, sst, sss, gridres, growth, roomy = 500, 20, 2.0, 34.0, 1000.0, 1.5, 6000
    grid, p, b = S.config_c1(n=n, seed=5)
    cp = S.calving_params(p)
    # a uniform flux (kg m-2 s-1) that fills the quickest bucket of a northern cell two and a half times in the 20 steps:
    # at least two bergs per cell, 800 in all, none of them before the third step
    need = min(p.initial_mass_n[k] * cp.mass_scaling_n[k] / cp.distribution_n[k] for k in range(10))
    rate = 2.5 * need / (gridres * gridres * p.dt * nsteps)
    (tmp_path / "input.nml").write_text(icebergs_nml_text(p, grid["desc"], halo=4, debug=".false."))
    perm = np.random.default_rng(8).permutation(n)                 # file order is not list order
    sh = {k: (v[perm].copy() if hasattr(v, "dtype") and len(v) == n else v) for k, v in b.items()}
    case, res = str(tmp_path / "reserve.bin"), str(tmp_path / "reserve.out")
    _write_case(case, gni, gnj, nsteps, gridres, p.dt, sst, sss, rate, growth, n, roomy, 0, sh)
    r = subprocess.run([RESERVE, case, res], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    with open(res, "rb") as f:
        cap_a, staging_a, m_a, ba = _read_run(f)
        cap_b, staging_b, m_b, bb = _read_run(f)
        assert f.read() == b""
    print(r.stdout.strip(), "| staging rows", staging_a, staging_b)
    assert m_b > n + 2 * gni * gnj - 1 and m_b <= roomy, m_b       # the roomy run itself never ran out
    assert m_a == m_b
    assert cap_b == roomy and staging_b == roomy
    assert n < m_a <= cap_a < roomy and staging_a >= m_a           # the handle grew by the rule, not to the roomy size; the staging followed
    oa, ob = np.argsort(ba["id"], kind="stable"), np.argsort(bb["id"], kind="stable")
    assert len(np.unique(ba["id"])) == m_a
    for k in ba:
        assert np.array_equal(ba[k][oa], bb[k][ob]), k
    assert set(b["id"]) <= set(ba["id"])                           # the 500 are still there, the rest was calved
