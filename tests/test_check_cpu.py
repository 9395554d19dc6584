"""The debug-mode invariants without a GPU: the host restatement (tests/check_ref.py) against brute-force definitions and against
the planted populations of tests/check_cases.py, the HIP-free decisions of the kernels (icebergs_amd/csrc/kid_check_plan.hpp)
under the sanitizers, TileExchange.check_duplicates over gloo ranks of numpy tiles, and the new calls in every host layer."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import check_cases as CC
import check_ref as CR
from icebergs_amd import synthetic as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the restatement against brute-force definitions ----
def _random_population(n, seed):
    """rows whose keys, members and ids come from small sets, so that groups of every kind occur; NaNs and both zeros among them;
    some rows dead, some in halo cells"""
    rng = np.random.Generator(np.random.PCG64(seed))
    b = S.empty_bergs(n)
    b["ine"][:], b["jne"][:] = rng.integers(0, 5, size=n), rng.integers(1, 4, size=n)       # the domain below is 1..3 x 1..3
    b["start_year"][:] = rng.integers(0, 2, size=n)
    for f, values in (("start_day", (1.0, 2.0)), ("start_mass", (5.0, np.nan, 7.0)), ("start_lon", (-0.0, 0.0, 3.0)), ("start_lat", (10.0, 20.0))):
        b[f][:] = rng.choice(values, size=n, p=(0.45, 0.1, 0.45) if len(values) == 3 and np.isnan(values[1]) else None)
    for f in CR.MEMBERS + CR.MEMBERS_MTS:
        b[f][:] = rng.choice((0.0, -0.0, 1.0), size=n, p=(0.6, 0.3, 0.1)) if f in ("lon", "axn_fast") else 0.0
    b["alive"][:] = rng.choice((0, 1), size=n, p=(0.15, 0.85))
    b["halo_berg"][:] = rng.choice((0.0, 1.0), size=n)
    b["id"] = rng.integers(1, max(2, n // 2), size=n).astype(np.int64)
    return b


class _Dom:
    isc, iec, jsc, jec = 1, 3, 1, 3


def _eq(x, y):
    return bool(x == y)        # IEEE: a NaN equals nothing, the two zeros are equal


def _brute(b, d, mts):
    """the definitions of include/kid_types.h, row by row and pair by pair, with no cell traversal and no sorting"""
    rows = [k for k in range(CR.nrows(b)) if b["alive"][k] != 0 and d.isc <= b["ine"][k] <= d.iec and d.jsc <= b["jne"][k] <= d.jec]
    same_keys = lambda p, q: all(_eq(b[f][p], b[f][q]) for f in CR.KEYS)      # noqa: E731
    members = CR.MEMBERS + (CR.MEMBERS_MTS if mts else ())
    n_id = n_same = 0
    for p, q in itertools.combinations(rows, 2):
        if same_keys(p, q):
            n_id += 1
            n_same += all(_eq(b[f][p], b[f][q]) for f in members)
    # a row is an identical when an earlier row of its cell has its keys
    n_identical = sum(any(b["ine"][p] == b["ine"][q] and b["jne"][p] == b["jne"][q] and same_keys(p, q) for p in rows[:a]) for a, q in enumerate(rows))
    ids = [int(b["id"][k]) for k in rows]
    n_dup = len(ids) - len(set(ids))
    n_halo = sum(1 for k in range(CR.nrows(b)) if b["alive"][k] != 0 and b["halo_berg"][k] < 0.5
                 and not (d.isc <= b["ine"][k] <= d.iec and d.jsc <= b["jne"][k] <= d.jec))
    return {"n_in_halo": n_halo, "n_identical": n_identical, "n_same_id": n_id, "n_same_berg": n_same, "n_dup_ids": n_dup}


@pytest.mark.parametrize("n", [0, 1, 2, 300])
@pytest.mark.parametrize("mts", [False, True])
def test_restatement_against_brute_force(n, mts):
    seen = {k: 0 for k in ("n_in_halo", "n_identical", "n_same_id", "n_same_berg", "n_dup_ids")}
    for seed in range(3):
        b = _random_population(n, 100 + seed)
        got, want = CR.report(b, _Dom, mts), _brute(b, _Dom, mts)
        assert got == want, (seed, got, want)
        for k in seen:
            seen[k] += want[k]
    if n == 300:
        assert all(v > 0 for v in seen.values()), seen        # every count is exercised
    if n < 2:
        assert not any(seen.values())


def test_members_of_sameberg_differ_between_mts_and_not():
    b = _random_population(300, 7)
    assert CR.report(b, _Dom, False)["n_same_berg"] > CR.report(b, _Dom, True)["n_same_berg"] > 0


# ---- the planted populations ----
def test_planted_duplicates_give_the_planted_numbers():
    g = CC.box_grid()
    d = g["desc"]
    b = CC.box_bergs()
    clean = CR.report(b, d)
    assert clean == {"n_in_halo": 0, "n_identical": 0, "n_same_id": 0, "n_same_berg": 0, "n_dup_ids": 0}
    want = CC.plant_duplicates(b, d)
    for mts in (False, True):
        got = CR.report(b, d, mts)
        assert got["n_same_id"] == want["n_same_id"] == 2086
        assert got["n_same_berg"] == (want["n_same_berg_mts"] if mts else want["n_same_berg"])
        assert got["n_identical"] == want["n_identical"] and got["n_dup_ids"] == want["n_dup_ids"] == 1 and got["n_in_halo"] == want["n_in_halo"] == 1
    # the 65 sit on rows of three waves and in two cells
    keys = np.stack([b[f] for f in CR.KEYS])
    c = [k for k in want["rows_same_id"] if np.array_equal(keys[:, k], keys[:, want["rows_same_id"][0]])]
    assert len(c) == 65 and len({k // 64 for k in c}) == 3 and len({(int(b["ine"][k]), int(b["jne"][k])) for k in c}) == 2


def test_shapes_of_the_box_are_clean():
    g = CC.box_grid()
    for n in CC.SHAPES:
        b = CC.box_bergs(n)
        assert int((b["alive"] != 0).sum()) == n - n // 7
        assert not any(CR.report(b, g["desc"]).values())


def test_planted_positions_give_the_planted_numbers():
    """on the state whose xi, yj are the oracle's own pos_within_cell: nothing before the plants, the planted numbers after"""
    import oracle_lib
    oracle_lib.build()
    g = CC.box_grid(mask=True)
    d = g["desc"]
    ref = CR.PositionRef(g, CC.box_params())
    b = CC.box_bergs()
    for k in range(CC.N):
        b["xi"][k], b["yj"][k] = ref.recompute(b, k)
    clean = ref.check(b)
    assert (clean["n_rows"], clean["n_xiyj"], clean["n_land"], clean["max_dxi"], clean["max_dyj"]) == (CC.N - CC.N // 7, 0, 0, 0.0, 0.0)
    want = CC.plant_positions(b, d)
    got = ref.check(b)
    assert got["n_rows"] == CC.N - CC.N // 7
    assert got["n_xiyj"] == want["n_xiyj"] == 6 and got["rows_xiyj"] == want["rows_xiyj"]
    assert got["n_land"] == 1 and got["rows_land"] == want["rows_land"]
    assert CR.count_out_of_order(b, d)[0] == want["n_in_halo"] == 1
    assert got["max_dxi"] == want["max_dxi"] and got["max_dyj"] == want["max_dyj"]          # not poisoned by the NaN
    assert 0.0 < got["max_dxi"] <= 2.0 ** -52 and 0.0 < got["max_dyj"] <= 2.0 ** -52
    # a cell outside the data domain: -999, -999, hence a mismatch
    b["ine"][1] = d.ied + 3
    assert ref.recompute(b, 1) == (-999.0, -999.0) and ref.check(b)["n_xiyj"] == 7


# ---- the HIP-free decisions of the kernels under the sanitizers ----
def test_check_plan_under_sanitizers(tmp_path):
    cxx = None
    for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            cxx = shutil.which(c)
            break
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "check_plan_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-o", exe, os.path.join(HERE, "check_plan_host.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().splitlines()[-1] == "ok"


# ---- TileExchange.check_duplicates over gloo ranks ----
class _NumpyTile:
    """all that check_duplicates asks of a tile"""

    def __init__(self, ids):
        self.ids = np.sort(np.asarray(ids, dtype=np.int64))

    def sorted_ids(self):
        return self.ids


def _ids_case(case, rank, world):
    """the lists of test_check_for_duplicate_ids_in_list (FW:7455-7486): five ids a rank, k + 5 pe; the root's last id made its
    fourth; then made 7 + 5 pe, which the next rank owns -- and two more: a rank with nothing, nobody with anything"""
    ids = [k + 5 * rank for k in range(1, 6)]
    if case == "clean":
        return ids
    if case == "twice-on-one-rank":
        if rank == 0:
            ids[4] = ids[3]
        return ids
    if case == "on-two-ranks":
        if rank == 0:
            ids[4] = 7 + 5 * rank
        return ids
    if case == "empty-rank":
        return [] if rank == world - 1 else ids
    if case == "all-empty":
        return []
    raise KeyError(case)


CASES = {"clean": (0, 0), "twice-on-one-rank": (1, 0), "on-two-ranks": (0, 1), "empty-rank": (0, 0), "all-empty": (0, 0)}


def _worker(rank, world, port, out_dir):
    from icebergs_amd.decomposed import TileExchange
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ex = TileExchange(world, 1, dist)
    got = {case: ex.check_duplicates(_NumpyTile(_ids_case(case, rank, world))) for case in CASES}
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array([got[c] for c in CASES], dtype=np.int64))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_check_duplicates_over_gloo_ranks(tmp_path, world):
    port = 31300 + (os.getpid() % 2000) + world
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    for rank in range(world):
        got = np.load(os.path.join(str(tmp_path), "rank%d.npy" % rank))
        for q, case in enumerate(CASES):
            lists = [_ids_case(case, r, world) for r in range(world)]
            assert tuple(got[q]) == CASES[case] == CR.check_duplicates_parallel(lists), (rank, case, got[q])     # the same on every rank


# ---- the new calls in every host layer ----
def test_entry_points_are_declared_in_every_host_layer():
    from icebergs_amd import lib as L
    from icebergs_amd import types as T
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kid.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+kid_check_bergs\s*\(\s*kid_handle\s*\*\s*h\s*,\s*uint32_t\s+what\s*,\s*kid_check_report\s*\*\s*rep\s*\)\s*;", hdr)
    assert re.search(r"\bint\s+kid_sorted_ids\s*\(\s*kid_handle\s*\*\s*h\s*,\s*int64_t\s*\*\s*ids\s*,\s*int64_t\s+capacity\s*,\s*int64_t\s*\*\s*n\s*\)\s*;", hdr)
    assert "kid_check_bergs" in L.SYMBOLS and "kid_sorted_ids" in L.SYMBOLS
    assert [T.ENUMS[k] for k in ("KID_CHECK_POSITION", "KID_CHECK_ORDER", "KID_CHECK_DUPLICATES", "KID_CHECK_IDS", "KID_CHECK_ALL")] == [1, 2, 4, 8, 15]
    names = [f for f, _ in T.CheckReport._fields_]
    assert names == ["n_rows", "n_xiyj", "n_land", "n_in_halo", "n_identical", "n_same_id", "n_same_berg", "n_dup_ids", "max_dxi", "max_dyj", "first_id", "first_row"]
    import ctypes as C
    assert C.sizeof(T.CheckReport) == 8 * 8 + 2 * 8 + 8 * 8
    mod = open(os.path.join(ROOT, "icebergs_amd", "fortran", "kid_hip_mod.F90")).read()
    public = set()
    for m in re.finditer(r"^\s*public ::(.*)$", mod, re.M):
        public |= {x.strip() for x in m.group(1).split(",")}
    for name in ("kid_check_bergs", "kid_sorted_ids"):
        assert "bind(C, name='%s')" % name in mod and name in public
    assert "kid_check_report" in public
    inc = open(os.path.join(ROOT, "icebergs_amd", "fortran", "kid_types_gen.inc")).read()
    assert re.search(r"type, bind\(C\) :: kid_check_report", inc) and re.search(r"KID_CHECK_ALL = 15\b", inc)
    from icebergs_amd.decomposed import HipTile, TileExchange
    from icebergs_amd.framework import Icebergs
    assert all(hasattr(c, m) for c in (Icebergs, HipTile) for m in ("check_bergs", "sorted_ids")) and hasattr(TileExchange, "check_duplicates")
