"""The bonded pair force of the DEM sub-steps as the device computes it (pair_const, then pair_force_dem of
icebergs_amd/csrc/kid_mts.inc, unchanged, through the test-only libkid_dem_probe.so: tests/dem_pair_probe.hip, one lane per pair)
against the 50-digit restatement of IB:959-1242 in tests/dem_pair_ref.py -- element by element, every output relative to its own
condition scale, never to a field maximum.

Bounds.  |computed - exact| <= C u S with u = 2^-53, S the condition scale the reference carries along and C the count of
roundings through pair_const, pair_geom and pair_finish, each form at the bound DESIGN section 4 states for it (kid_rcp 1 ulp and
the product with it 1.5, kid_div 0.6, kid_sqrt 1, kid_cube 1, ocml sin / cos 1, IEEE +, -, *, /, sqrt 0.5).  The rules that turn
the expression tree into C and S are the docstring of tests/dem_pair_ref.py; the constants they give are its DERIVED_C (Cartesian /
lat-lon: len 4 / 13, tangential displacement 46.6 / 118.6, nstress 30 / 46, sstress 130.8 / 274.8, forces 92.6 / 200.6, torques
109.6 / 238.6, damping forces 8, half_delta 5 / 14, L 18 / 36, Thick 16 / 34), with one of them read aloud in the comment there.
tests/test_dem_pair_cpu.py holds the oracle to the same reference with IEEE roundings counted instead: the bound is attainable.
What is asserted is the derived bound; the measured worst ratio is printed per output and family (DESIGN section 4 records both).

Sensitivity.  Each mechanism family leaves one term of the force non-zero; against the same reference with that mechanism's
coefficient (dem_spring_coef, 2 (1 + poisson), the 12 of r12l0, the 2/3 of the original moment, dem_damping_coef, the 0.5 L lever)
off by 1e-9 relative the device's outputs must violate the bound, by a factor of 10 at least.

The probe library is test-only: icebergs_amd/lib.py never loads it."""
import ctypes as C
import os

import numpy as np
import pytest

import dem_pair_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "icebergs_amd", "csrc", "libkid_dem_probe.so")
PLANES = ("len", "tg1", "tg2", "relrot", "nstress", "sstress", "Fx", "Fy", "Fdx", "Fdy", "Tq", "Tdq", "To_q", "half_delta", "L", "Thick")


class Probe:
    def __init__(self):
        import torch
        assert os.path.exists(PROBE), "libkid_dem_probe.so is not built (build() makes it)"
        self.torch = torch
        self.lib = C.CDLL(PROBE)
        from icebergs_amd import types as T
        vp, d = C.c_void_p, C.c_double
        self.lib.kid_probe_dem_pair.argtypes = [C.POINTER(T.Params), C.c_int, d, d, d] + [vp] * 14 + [C.c_longlong]
        assert self.lib.kid_probe_dem_pair_outputs() == len(PLANES)

    def __call__(self, p, latlon, x):
        """{output: n doubles, "status", "broke": n int32} of the n pairs of x (tests/dem_pair_ref.py: empty_inputs)"""
        t = self.torch
        n = len(x["dt"])

        def dev(a, dtype=np.float64):
            return t.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")
        rows = {f: dev(x[f].reshape(2 * n)) for f in ("fl_k", "thickness", "mass", "length", "width")}   # row 2e evaluates, 2e+1 is its partner
        ids = dev(x["id"].reshape(2 * n), np.int64)
        rec = dev(np.stack([x[f].reshape(2 * n) for f in ("lon", "lat", "u", "v", "w", "rot")], axis=1))
        assert rec.shape == (2 * n, 6) and rec.is_contiguous()
        pair = {f: dev(x[f]) for f in ("t1", "t2", "relrot0", "dt")}
        status = t.full((n,), -1, dtype=t.int32, device="cuda:0")
        broke = t.full((n,), -1, dtype=t.int32, device="cuda:0")
        out = t.full((len(PLANES), n), float("nan"), dtype=t.float64, device="cuda:0")
        area, radius, kd = R.derived(p)
        t.cuda.synchronize()
        rc = self.lib.kid_probe_dem_pair(C.byref(p), int(latlon), area, radius, kd, ids.data_ptr(), rows["fl_k"].data_ptr(), rows["thickness"].data_ptr(),
                                         rows["mass"].data_ptr(), rows["length"].data_ptr(), rows["width"].data_ptr(), rec.data_ptr(), pair["t1"].data_ptr(),
                                         pair["t2"].data_ptr(), pair["relrot0"].data_ptr(), pair["dt"].data_ptr(), status.data_ptr(), broke.data_ptr(),
                                         out.data_ptr(), n)
        assert rc == 0, rc
        o = out.cpu().numpy()
        r = {name: o[k].copy() for k, name in enumerate(PLANES)}
        r["status"], r["broke"] = status.cpu().numpy(), broke.cpu().numpy()
        return r


@pytest.fixture(scope="module")
def probe():
    return Probe()


@pytest.mark.parametrize("index", range(len(R.families())), ids=[f[0] for f in R.families()])
def test_device_pair_force_within_the_derived_bounds(probe, index):
    name, p, latlon, x, coefs, outs = R.families()[index]
    got = probe(p, latlon, x)
    R.check_family(index, got, got["status"], got["broke"], "device", "MEASURED device")
    if coefs:
        R.check_sensitivity(index, got, "device", "CONTROL device")


def test_device_pair_force_edges(probe):
    """same id, a footloose child, zero separation, nothing tangential, stresses at and one ulp above their thresholds, broken in
    compression and in tension, fracture without the stress criterion: each with its exact outcome (tests/dem_pair_ref.py)"""
    R.check_edges(probe, "device")
