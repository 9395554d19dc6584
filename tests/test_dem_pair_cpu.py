"""The oracle's calculate_force_dem (through ko_dem_pair: one pair by value on a two-berg context) against the 50-digit restatement of
IB:959-1242 in tests/dem_pair_ref.py, on every input family and edge that tests/test_dem_pair_gpu.py puts to the device, with the
same per-output bounds |computed - exact| <= C u S -- C counted with IEEE roundings in place of the device's forms.  The oracle and
the reference are two independent restatements of the routine (one in C doubles as the sub-step loop calls it, one in mpmath with
the error analysis carried along): that they agree inside the bound says that the bound is attainable and that the reference is
the routine.  Each mechanism family is run a second time against a reference with its coefficient off by 1e-9: it must fail.

The derivation of the bounds (rules, rounding costs of each form, one line read aloud) is the docstring of tests/dem_pair_ref.py
and the comment at its DERIVED_C.  The probe library and ko_dem_pair are test-only; the product path loads neither."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import dem_pair_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BOND_ORDER = ("len", "tg1", "tg2", "nstress", "sstress", "relrot", "Fx", "Fy", "Fdx", "Fdy", "Tq", "Tdq")   # KID_BOND_*
NOUT = 40


def pack(x, e):
    xin = np.zeros(26)
    for k in range(2):
        for q, f in enumerate(R.PER_BERG):
            xin[11 * k + q] = x[f][e, k]
    xin[22:26] = x["t1"][e], x["t2"][e], x["relrot0"][e], x["dt"][e]
    return np.ascontiguousarray(x["id"][e], dtype=np.int64), xin


def oracle_raw(lib, p, latlon, x):
    import oracle_lib
    n = len(x["dt"])
    out = np.zeros((n, NOUT))
    for e in range(n):
        ids, xin = pack(x, e)
        lib.ko_dem_pair(C.byref(p), int(latlon), ids.ctypes.data_as(C.POINTER(C.c_int64)), oracle_lib._dp(xin), oracle_lib._dp(out[e]))
    return out


def unpack(p, out):
    """the columns of ko_dem_pair as the outputs of the pair function; status as the routine shows it: 1 nothing written and no
    error, 2 / 3 the two FATALs (error_count) told apart by the length"""
    r = {o: out[:, q].copy() for q, o in enumerate(BOND_ORDER)}
    r["To_q"] = out[:, 12 + BOND_ORDER.index("Tq")].copy()
    err, brk = out[:, 34], out[:, 30]
    r["status"] = np.where(err > 0, np.where(r["len"] == 0.0, 2, 3), np.where(r["len"] == 0.0, 1, 0)).astype(np.int32)
    r["broke"] = (brk != 0).astype(np.int32)
    # the partner's side mirrors the primary's (IB:1180-1190, 1218-1230), the caller's sums are the stored forces of an unbroken bond
    done = r["status"] == 0   # (the FATAL of IB:1200 stops before the mirroring)
    for q, o in enumerate(BOND_ORDER):
        sign = 1.0 if o in ("len", "nstress", "sstress") else -1.0
        if o != "Tq":
            assert np.array_equal(out[done, 12 + q], sign * out[done, q]), o
    assert np.array_equal(out[:, 31], out[:, 30]) and np.array_equal(out[:, 35], 2.0 * out[:, 30]) and np.array_equal(out[:, 36], out[:, 30])
    assert np.array_equal(out[:, 32], 2.0 - out[:, 30]) and np.array_equal(out[:, 33], 2.0 - out[:, 30])   # n_bonds (use_broken_bonds_for_substep_contact)
    whole = (r["status"] == 0) & (r["broke"] == 0)
    for q, o in ((24, "Fx"), (25, "Fy"), (26, "Tq"), (27, "Fdx"), (28, "Fdy"), (29, "Tdq")):
        assert np.array_equal(out[whole, q], r[o][whole]), o
    area, radius, kd = R.derived(p)
    assert np.all(out[:, 37] == area) and np.all(out[:, 38] == radius) and np.all(out[:, 39] == kd), "the derived constants"
    return r


@pytest.mark.parametrize("index", range(len(R.families())), ids=[f[0] for f in R.families()])
def test_oracle_pair_force_within_the_derived_bounds(oracle, index):
    name, p, latlon, x, coefs, outs = R.families()[index]
    got = unpack(p, oracle_raw(oracle, p, latlon, x))
    R.check_family(index, got, got["status"], got["broke"], "ieee", "oracle")
    if coefs:
        R.check_sensitivity(index, got, "ieee", "oracle")


def test_derived_constants_are_the_table():
    """DERIVED_C is what the rules give on the families' expression trees, for both arithmetic models: no entry is exceeded and every
    entry is reached (C never depends on the values, so a few pairs per family do)"""
    for model in ("device", "ieee"):
        worst = {o: [0.0, 0.0] for o in R.DERIVED_C[model]}
        for name, p, latlon, x, _, _ in R.families():
            few = {f: v[:3] for f, v in x.items()}
            _, _, cc, _, _ = R.reference(p, latlon, few, model)
            for o in worst:
                worst[o][1 if latlon else 0] = max(worst[o][1 if latlon else 0], float(cc[o].max()))
        for o, (cart, ll) in R.DERIVED_C[model].items():
            assert abs(worst[o][0] - cart) < 0.05 and abs(worst[o][1] - ll) < 0.05, (model, o, worst[o], (cart, ll))


def test_oracle_pair_force_edges_and_sanitizers(oracle, tmp_path):
    """every edge with its exact outcome on the oracle; then the same calls again in a stand-alone program built with the oracle's
    sources under AddressSanitizer and UndefinedBehaviorSanitizer: clean, and the same bits"""
    calls = []

    def evaluate(p, latlon, x):
        from icebergs_amd import synthetic as S
        out = oracle_raw(oracle, p, latlon, x)
        calls.append((S.params_copy(p), int(latlon), {f: v.copy() for f, v in x.items()}, out))
        return unpack(p, out)
    R.check_edges(evaluate, "oracle")
    assert len(calls) >= 12
    cc = next((c for c in (os.environ.get("CC"), "gcc", "clang", "/opt/rocm/llvm/bin/clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    exe, cases, results = str(tmp_path / "dem_pair_host"), str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    src = [os.path.join(ROOT, "oracle", f) for f in sorted(os.listdir(os.path.join(ROOT, "oracle"))) if f.endswith(".c")]
    build = subprocess.run([cc, "-std=c11", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-o", exe, os.path.join(HERE, "dem_pair_host.c")] + src + ["-lm"], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    with open(cases, "wb") as f:
        for p, latlon, x, _ in calls:
            for e in range(len(x["dt"])):
                ids, xin = pack(x, e)
                f.write(bytes(p)); f.write(np.array([latlon, ids[0], ids[1]], dtype=np.int64).tobytes()); f.write(xin.tobytes())
    run = subprocess.run([exe, cases, results], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1] == "ok"
    again = np.fromfile(results, dtype=np.float64).reshape(-1, NOUT)
    first = np.concatenate([out for _, _, _, out in calls])
    assert again.shape == first.shape and np.array_equal(again.view(np.int64), first.view(np.int64))
