"""grd_chksum2 / grd_chksum3 (icebergs_framework.F90:6832-6886, 6761-6829) restated in numpy, from the cited lines.

A field is the data-domain array (nj, ni) -- grd%fld(isd:ied, jsd:jed) with the first Fortran index last -- or (nk, nj, ni) for
the 3-d fields.  Both routines loop over the computational domain only, j outer / i inner (3-d: k outermost), and

  mean = sum(fld) / icount                      (FW:6852, 6864)      sequential, in loop order
  rms  = sqrt(sum(fld**2) / icount)             (FW:6853, 6865)
  sd   = sqrt(sum((fld - mean)**2) / icount)    (FW:6866-6872)       second pass, about the mean just formed
  min, max                                      (FW:6847-6855)
  chksum  = mpp_chksum(fld)                     (FW:6873)            wrap-around sum of the IEEE bit patterns, kept as a default
  chksum2 = mpp_chksum(fld * float(i + 2*j))    (FW:6856, 6874)      integer (the low 32 bits, signed: kid_chksum.inc)
            3-d: float(i + 2*j + 3*(k-1)), k from 1 (FW:6792), i, j the data-domain indices (io, jo of FW:6782-6783)

np.add.accumulate adds one element after the other, which is the order of the Fortran loops on the flattened array.
`sums` carries what the tests need to bound another summation order: the three sequential sums, sum|x|, the terms."""
import numpy as np


def _i32(u):
    u = int(u) & 0xFFFFFFFF
    return u - (1 << 32) if u >= (1 << 31) else u


def mpp_chksum(a):
    return _i32(int(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).sum(dtype=np.uint64)))


def _seq_sum(x):
    return float(np.add.accumulate(x)[-1]) if x.size else 0.0


def grd_chksum(desc, fld):
    """the record of one field as a dict: chksum, chksum2, minv, maxv, mean, rms, sd, present = 1, and `sums`"""
    d = desc
    fld = np.asarray(fld, dtype=np.float64)
    f3 = fld[None] if fld.ndim == 2 else fld
    nk = f3.shape[0]
    assert f3.shape[1:] == (d.jed - d.jsd + 1, d.ied - d.isd + 1), f3.shape
    comp = f3[:, d.jsc - d.jsd:d.jec - d.jsd + 1, d.isc - d.isd:d.iec - d.isd + 1]
    i = np.arange(d.isc, d.iec + 1, dtype=np.int64)[None, None, :]
    j = np.arange(d.jsc, d.jec + 1, dtype=np.int64)[None, :, None]
    k = np.arange(nk, dtype=np.int64)[:, None, None]            # k - 1
    w = (i + 2 * j + 3 * k).astype(np.float64)
    x = np.ascontiguousarray(comp).ravel()                        # k outer, j, i inner: the loop order
    n = x.size
    s1, s2 = _seq_sum(x), _seq_sum(x * x)
    mean = s1 / float(n)
    rms = float(np.sqrt(s2 / float(n)))
    dev = (x - mean) * (x - mean)
    ssd = _seq_sum(dev)
    sd = float(np.sqrt(ssd / float(n)))
    return {"chksum": mpp_chksum(comp), "chksum2": mpp_chksum(comp * w), "minv": float(x.min()), "maxv": float(x.max()),
            "mean": mean, "rms": rms, "sd": sd, "present": 1,
            "sums": {"n": n, "s1": s1, "s2": s2, "ssd": ssd, "abs1": float(np.abs(x).sum()), "abs2": float((x * x).sum()), "x": x}}


def absent():
    return {"chksum": 0, "chksum2": 0, "minv": 0.0, "maxv": 0.0, "mean": 0.0, "rms": 0.0, "sd": 0.0, "present": 0}


U = 2.0 ** -53


def bounds(ref):
    """How far mean, rms and sd of another summation order may lie from `ref`'s: every sum of N terms within
    2 (N-1) u sum|term| of the sequential one (a bound on either order is (N-1) u sum|term|; u = 2**-53).
      mean: B1 / N, and the rounding of the two divisions.
      rms:  S2 within B2 -> the interval of sqrt(S2' / N), widened by the roundings of division and root (3 u relative).
      sd:   the other mean differs by dm <= tol(mean), so every term (x - m)**2 moves by at most 2 |x - m| dm + dm**2; both
            sides round the difference and the square (3 u relative each); then the order bound on the sum of the terms.
    Returns {"mean": tol, "rms": (lo, hi), "sd": (lo, hi)}."""
    s = ref["sums"]
    n, x = s["n"], s["x"]
    b1 = 2.0 * (n - 1) * U * s["abs1"]
    b2 = 2.0 * (n - 1) * U * s["abs2"]
    tol_mean = b1 / n + 2.0 * U * (abs(ref["mean"]) + b1 / n)
    a = np.abs(x - ref["mean"])
    pert = float((2.0 * a * tol_mean + tol_mean ** 2 + 6.0 * U * (a + tol_mean) ** 2).sum())
    b3 = 2.0 * (n - 1) * U * (s["ssd"] + pert) + pert

    def interval(total, b):
        lo, hi = np.sqrt(max(0.0, total - b) / n), np.sqrt((total + b) / n)
        return lo * (1.0 - 3.0 * U), hi * (1.0 + 3.0 * U)
    return {"mean": tol_mean, "rms": interval(s["s2"], b2), "sd": interval(s["ssd"], b3)}
