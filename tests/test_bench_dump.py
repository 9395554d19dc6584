"""bench.py --dump-outputs without a GPU: dump_outputs against a stand-in handle whose population has lost and reordered
bergs, in a child process (importing bench.py sets its runtime environment)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import bench
from icebergs_amd import types as T
from icebergs_amd.synthetic import empty_bergs

n = 100000
rng = np.random.default_rng(5)
b0 = empty_bergs(n)
b0["id"][:] = rng.permutation(np.arange(1, n + 1))
for name in T.BERG_F64_NAMES:
    b0[name][:] = rng.uniform(-1.0, 1.0, n)

class Handle:
    ni, nj = 7, 5
    def fetch(self):
        return (np.ones((T.NACC, self.nj, self.ni)), np.full((T.NOUT, self.nj, self.ni), 2.0), np.arange(T.NSCALAR, dtype=np.float64))
    def download_bergs(self):
        # the population after a run: rows reordered, 1000 bergs gone (dropped rows), 1000 more dead but still in their rows
        order = rng.permutation(n)[1000:]
        b = {k: v[order].copy() for k, v in b0.items()}
        b["alive"][:1000] = 0
        return b

bench.dump_outputs(sys.argv[2], np, T, Handle(), b0["id"])
np.save(sys.argv[2] + "_lon_by_id.npy", b0["lon"][np.argsort(b0["id"])])
"""


def test_dump_outputs_absent_bergs_are_zero(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    arrays = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    lon_by_id = np.load(str(out) + "_lon_by_id.npy")                  # the population's lon, row k = id k + 1
    assert sum(os.path.getsize(out / (f + ".npy")) for f in arrays) <= 64 << 20
    for name, a in arrays.items():
        assert a.dtype == np.float64 and np.isfinite(a).all(), name
    ids = arrays["berg_id"]
    assert len(ids) == 65536 and np.all(np.diff(ids) > 0)
    assert arrays["out_spread_mass"].shape == (5, 7) and np.all(arrays["acc_floating_melt"] == 1.0)
    alive = arrays["berg_alive"] != 0
    assert 0 < np.count_nonzero(~alive) < 0.1 * len(ids)
    for name in ("lon", "mass", "ine", "alive"):
        assert np.all(arrays["berg_" + name][~alive] == 0), name      # an absent berg: every member 0
    assert np.array_equal(arrays["berg_lon"][alive], lon_by_id[ids[alive].astype(np.int64) - 1])   # a present berg: its own row, by id
