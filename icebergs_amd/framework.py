"""Host-side mirror of the reference's `ice_bergs` surface for the evolve-loop path.

The reference host is Fortran (icebergs_init / icebergs_run, src/icebergs.F90:92-178, 5074-5887) and the
Fortran binding lives in icebergs_amd/fortran/.  This module is the same thin host layer in Python, used by
the tests, bench.py and the multi-GPU driver: it owns no numerics, it only moves arrays across the C ABI
(include/kid.h) and calls the phases in the order icebergs_run does (IB:5423-5512).
"""
import atexit
import ctypes as C
import weakref

import numpy as np

from . import lib as _lib
from . import types as T


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _chk_record(rec):
    return {name: getattr(rec, name) for name, _ in T.GrdChksum._fields_ if name != "pad_"}


def _a18(txt):
    """Fortran's a18: the leftmost 18 characters, or the text right-justified in 18 columns"""
    return txt[:18].rjust(18)


def _es16_9(x):
    """Fortran's es16.9 (a three-digit exponent drops the letter: 1.000000000+100)"""
    if x != x:
        return "NaN".rjust(16)
    if x in (float("inf"), float("-inf")):
        return ("Infinity" if x > 0 else "-Infinity").rjust(16)
    mant, exp = ("%.9E" % x).split("E")
    return (mant + ("E" + exp if len(exp) == 3 else exp)).rjust(16)


def format_bergs_chksum(label, six):
    """FW:6975: '("KID, bergs_chksum: ",a18,6(x,a,"=",i22))'"""
    names = ("chksum", "chksum2", "chksum3", "chksum4", "chksum5", "#")
    return "KID, bergs_chksum: " + _a18(label) + "".join(" %s=%22d" % (n, v) for n, v in zip(names, six))


def format_grd_chksum(label, rec, three_d=False):
    """FW:6876 (grd_chksum2) and FW:6817 (grd_chksum3); the i8 group that ends grd_chksum2's format has no item and prints nothing"""
    head = "KID, grd_chksum%d: " % (3 if three_d else 2)
    ints = "".join(" %s=%22d" % (n, rec[n]) for n in ("chksum", "chksum2"))
    reals = "".join(" %s=%s" % (n, _es16_9(rec[k])) for n, k in (("min", "minv"), ("max", "maxv"), ("mean", "mean"), ("rms", "rms"), ("sd", "sd")))
    return head + _a18(label) + ints + reals


_LIVE = weakref.WeakSet()


@atexit.register
def _close_live_handles():
    """Handles still open when the interpreter exits are destroyed here, while the HIP runtime (and a profiler attached to it)
    is still up: a handle left to `__del__` during interpreter shutdown -- or never finalised at all -- used to keep its
    streams, captured graphs and the cooperative launch's buffers alive into the runtime's own exit handlers."""
    for ib in list(_LIVE):
        try:
            ib.close()
        except Exception:
            pass


class Icebergs:
    """One handle == one `type(icebergs)` container bound to one GPU (and one HIP stream)."""

    def __init__(self, grid, params, capacity, device=0):
        """icebergs_init (IB:92-178): grid + parameters -> device-resident state."""
        self.lib = _lib.load()
        self.grid = grid
        self.params = params
        self.device = int(device)
        d = grid["desc"]
        self.ni, self.nj = d.ied - d.isd + 1, d.jed - d.jsd + 1
        self.ncell = self.ni * self.nj
        self.h = C.c_void_p()
        rc = self.lib.kid_create(C.byref(d), C.byref(params), int(capacity), int(device), C.byref(self.h))
        if rc != 0:
            msg = self.lib.kid_last_error(self.h).decode() if self.h else "kid_create failed"
            if self.h:
                self.lib.kid_destroy(self.h)
                self.h = None
            raise _lib.KidError("kid_create: rc=%d %s" % (rc, msg))
        arr = (C.POINTER(C.c_double) * T.ENUMS["KID_NGRID_STATIC"])()
        keep = []
        for k, name in enumerate(T.GRID_STATIC_NAMES):
            a = np.ascontiguousarray(grid["static"][name], dtype=np.float64)
            assert a.shape == (self.nj, self.ni), (name, a.shape)
            keep.append(a)
            arr[k] = _dp(a)
        self._check(self.lib.kid_set_static_grid(self.h, arr), "kid_set_static_grid")
        self.set_forcing(grid["forcing"])
        self.acc = np.zeros((T.NACC, self.nj, self.ni))
        self.out = np.zeros((T.NOUT, self.nj, self.ni))
        self.scalars = np.zeros(T.NSCALAR)
        _LIVE.add(self)

    def _check(self, rc, what):
        if rc != 0:
            raise _lib.KidError("%s: rc=%d %s" % (what, rc, self.lib.kid_last_error(self.h).decode()))

    def close(self):
        if getattr(self, "h", None):
            self.lib.kid_destroy(self.h)
            self.h = None
        _LIVE.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- forcing (what icebergs_run's ingest block leaves in grd%*, IB:5236-5383) ----
    def set_forcing(self, forcing):
        arr = (C.POINTER(C.c_double) * T.ENUMS["KID_NFORCING"])()
        keep = []
        for k, name in enumerate(T.FORCING_NAMES):
            a = np.ascontiguousarray(forcing[name], dtype=np.float64)
            assert a.shape == (self.nj, self.ni), (name, a.shape)
            keep.append(a)
            arr[k] = _dp(a)
        self._check(self.lib.kid_set_forcing(self.h, arr), "kid_set_forcing")

    def ingest_forcing(self, args, vel_stagger="B", stress_stagger="B", tau_is_velocity=False, cyclic_x=False, on_device=False):
        """icebergs_run's ingest block on the device (kid_ingest_forcing, IB:5236-5383).  `args`: dict with uo, vo, ui, vi,
        tauxa, tauya, ssh, sst, cn, hi and optionally sss -- numpy arrays of shape (n2, n1) holding the Fortran array
        a(n1, n2), or with on_device (device address, (n2, n1)) pairs."""
        if on_device:   # resident arrays: the argument block is rebuilt only when an address or a switch changes
            key = (tuple(sorted((k, int(v[0]), tuple(v[1])) for k, v in args.items() if v is not None)), vel_stagger, stress_stagger, bool(tau_is_velocity), bool(cyclic_x))
            if getattr(self, "_ingest_key", None) == key:
                self._check(self.lib.kid_ingest_forcing(self.h, self._ingest_ref), "kid_ingest_forcing")
                return
        st = {"B": T.ENUMS["KID_BGRID_NE"], "C": T.ENUMS["KID_CGRID_NE"], "A": T.ENUMS["KID_AGRID"]}
        fin, keep, shape = T.ForcingIn(), [], {}
        for name in ("uo", "vo", "ui", "vi", "tauxa", "tauya", "ssh", "sst", "cn", "hi", "sss"):
            v = args.get(name)
            if v is None:
                setattr(fin, name, None)
                continue
            if on_device:
                ptr, shp = v
                setattr(fin, name, C.cast(C.c_void_p(int(ptr)), C.POINTER(C.c_double)))
            else:
                a = np.ascontiguousarray(v, dtype=np.float64)
                keep.append(a)
                shp = a.shape
                setattr(fin, name, _dp(a))
            shape[name] = shp
        for name, other in (("uo", "ui"), ("vo", "vi")):
            assert shape[name] == shape[other], (name, other)
        d = self.grid["desc"]
        nic, njc = d.iec - d.isc + 1, d.jec - d.jsc + 1
        for name in ("ssh", "cn", "hi"):
            assert shape[name] == (njc + 2, nic + 2), (name, shape[name])
        for name in ("sst", "sss"):
            assert name not in shape or shape[name] == (njc, nic), (name, shape[name])
        fin.u_nj, fin.u_ni = shape["uo"]
        fin.v_nj, fin.v_ni = shape["vo"]
        fin.taux_nj, fin.taux_ni = shape["tauxa"]
        fin.tauy_nj, fin.tauy_ni = shape["tauya"]
        fin.vel_stagger, fin.stress_stagger = st[vel_stagger], st[stress_stagger]
        fin.tau_is_velocity, fin.cyclic_x, fin.on_device = int(tau_is_velocity), int(cyclic_x), int(on_device)
        self._check(self.lib.kid_ingest_forcing(self.h, C.byref(fin)), "kid_ingest_forcing")
        if on_device:
            self._ingest_key, self._ingest_fin, self._ingest_ref = key, fin, C.byref(fin)

    def get_forcing(self):
        """grd%uo .. grd%hi as the handle holds them (after set_forcing or ingest_forcing)"""
        out = {name: np.empty((self.nj, self.ni)) for name in T.FORCING_NAMES}
        arr = (C.POINTER(C.c_double) * T.ENUMS["KID_NFORCING"])(*[_dp(out[name]) for name in T.FORCING_NAMES])
        self._check(self.lib.kid_get_forcing(self.h, arr), "kid_get_forcing")
        return out

    # ---- trajectories (record_posn FW:5328-5498, write_trajectory IO2:1631-2103) ----
    def set_traj_params(self, tp):
        self._check(self.lib.kid_set_traj_params(self.h, C.byref(tp)), "kid_set_traj_params")

    def record_posn(self):
        self._check(self.lib.kid_record_posn(self.h), "kid_record_posn")

    def num_traj_records(self):
        n = C.c_int64()
        self._check(self.lib.kid_num_traj_records(self.h, C.byref(n)), "kid_num_traj_records")
        return n.value

    def write_trajectories(self, path):
        self._check(self.lib.kid_write_trajectories(self.h, str(path).encode()), "kid_write_trajectories")

    def num_bond_traj_records(self):
        n = C.c_int64()
        self._check(self.lib.kid_num_bond_traj_records(self.h, C.byref(n)), "kid_num_bond_traj_records")
        return n.value

    def write_bond_trajectories(self, path):
        """write_bond_trajectory, IO2:2106-2331 (needs TrajParams.save_bond_traj and uploaded bonds)"""
        self._check(self.lib.kid_write_bond_trajectories(self.h, str(path).encode()), "kid_write_bond_trajectories")

    # ---- migration between the handles of a decomposed domain (send_bergs_to_other_pes FW:2997-3247) ----
    def buffer_width(self):
        w = C.c_int32()
        self._check(self.lib.kid_buffer_width(self.h, C.byref(w)), "kid_buffer_width")
        return w.value

    def pack_emigrants(self, direction):
        """bergs that left through `direction` (types.ENUMS['KID_DIR_E'] ...) as rows of the reference's wire format
        (pack_berg_into_buffer2 FW:3250-3301); they are gone from the handle afterwards"""
        n = C.c_int64()
        if getattr(self, "_mig_buf", None) is None:
            self._mig_buf = np.empty((4096, self.buffer_width()))
        rc = self.lib.kid_pack_emigrants(self.h, direction, _dp(self._mig_buf), self._mig_buf.shape[0], C.byref(n))
        if rc == -4 and n.value > self._mig_buf.shape[0]:        # KID_ECAPACITY: nothing was packed, n says how many wait
            self._mig_buf = np.empty((2 * n.value, self._mig_buf.shape[1]))
            rc = self.lib.kid_pack_emigrants(self.h, direction, _dp(self._mig_buf), self._mig_buf.shape[0], C.byref(n))
        self._check(rc, "kid_pack_emigrants")
        return self._mig_buf[:n.value].copy()

    def pack_emigrants_pair(self, axis):
        """east + west (axis 0) or north + south (axis 1) in one launch; returns the two record arrays"""
        na, nb = C.c_int64(), C.c_int64()
        if getattr(self, "_mig_buf2", None) is None:
            self._mig_buf2 = [np.empty((4096, self.buffer_width())) for _ in range(2)]
        for attempt in range(2):
            a, b = self._mig_buf2
            rc = self.lib.kid_pack_emigrants_pair(self.h, axis, _dp(a), a.shape[0], C.byref(na), _dp(b), b.shape[0], C.byref(nb))
            if rc != -4 or attempt:
                break
            self._mig_buf2 = [np.empty((max(2 * n.value, x.shape[0]), x.shape[1])) for n, x in ((na, a), (nb, b))]   # KID_ECAPACITY: nothing was packed
        self._check(rc, "kid_pack_emigrants_pair")
        return self._mig_buf2[0][:na.value].copy(), self._mig_buf2[1][:nb.value].copy()

    def unpack_immigrants_pair(self, buf_a, buf_b):
        a, b = (np.ascontiguousarray(x, dtype=np.float64) for x in (buf_a, buf_b))
        if a.size or b.size:
            self._check(self.lib.kid_unpack_immigrants_pair(self.h, _dp(a) if a.size else None, a.shape[0] if a.size else 0,
                                                            _dp(b) if b.size else None, b.shape[0] if b.size else 0), "kid_unpack_immigrants_pair")

    def pack_halo_bergs_pair(self, axis, width=0, sides=(True, True)):
        """copies of the bergs next to the two edges of `axis` for the neighbours' halos (update_halo_icebergs FW:1800-2131), as
        records with halo_berg = 1: (for the east / north neighbour, for the west / south one); the rows stay as they are.
        width 0: the grid's halo; sides: False where there is no neighbour (nothing is selected for it)"""
        n = [C.c_int64(), C.c_int64()]
        if getattr(self, "_halo_berg_buf", None) is None:
            self._halo_berg_buf = [np.empty((4096, 34)) for _ in range(2)]
        for attempt in range(2):
            a, b = self._halo_berg_buf
            rc = self.lib.kid_pack_halo_bergs_pair(self.h, int(axis), int(width), _dp(a) if sides[0] else None, a.shape[0], C.byref(n[0]),
                                                   _dp(b) if sides[1] else None, b.shape[0], C.byref(n[1]))
            if rc != -4 or attempt:
                break
            self._halo_berg_buf = [np.empty((max(2 * q.value, x.shape[0]), 34)) for q, x in zip(n, (a, b))]   # KID_ECAPACITY: nothing was packed
        self._check(rc, "kid_pack_halo_bergs_pair")
        return self._halo_berg_buf[0][:n[0].value].copy(), self._halo_berg_buf[1][:n[1].value].copy()

    def halo_berg_count(self):
        """resident halo rows: more than 0 only between an unpack of halo records and the next kid_evolve_icebergs"""
        n = C.c_int64()
        self._check(self.lib.kid_halo_berg_count(self.h, C.byref(n)), "kid_halo_berg_count")
        return n.value

    def unpack_immigrants(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.float64)
        if buf.size:
            self._check(self.lib.kid_unpack_immigrants(self.h, _dp(buf), buf.shape[0]), "kid_unpack_immigrants")

    # ---- halo update of the on-ocean planes of a decomposed domain (mpp_update_domains in sum_up_spread_fields, IB:6106-6107) ----
    def calculate_mass_on_ocean(self):
        """the spreading half of kid_create_gridded_icebergs_fields (no gather); step_gather is the other half"""
        self._check(self.lib.kid_calculate_mass_on_ocean(self.h), "kid_calculate_mass_on_ocean")

    def halo_plane_count(self):
        n = C.c_int32()
        self._check(self.lib.kid_halo_plane_count(self.h, C.byref(n)), "kid_halo_plane_count")
        return n.value

    def halo_buffer_count(self, axis, width=1):
        """doubles per direction of pack_halo_pair / unpack_halo_pair (include/kid.h has the layout)"""
        n = C.c_int64()
        self._check(self.lib.kid_halo_buffer_count(self.h, int(axis), int(width), C.byref(n)), "kid_halo_buffer_count")
        return n.value

    def _halo_buffers(self, bufs, count, what):
        """addresses of a (hi, lo) / (lo, hi) pair of flat float64 buffers: numpy arrays, or torch tensors on the handle's device
        (on_device = 1); None stands for a missing side"""
        ptrs, dev = [], None
        for b in bufs:
            if b is None:
                ptrs.append(None)
                continue
            on_dev = not isinstance(b, np.ndarray)
            assert dev is None or dev == on_dev, what + ": both buffers on the host or both on the device"
            dev = on_dev
            if on_dev:
                import torch
                assert isinstance(b, torch.Tensor) and b.is_cuda and b.device.index == self.device and b.dtype == torch.float64 and b.is_contiguous(), what
                assert b.numel() == count, (what, b.numel(), count)
                ptrs.append(b.data_ptr())
            else:
                assert b.dtype == np.float64 and b.flags.c_contiguous and b.size == count, (what, b.shape, count)
                ptrs.append(b.ctypes.data)
        return ptrs, bool(dev)

    def _halo_order_in(self, bufs):
        import torch
        torch.cuda.current_stream(next(b for b in bufs if b is not None).device).synchronize()

    def pack_halo_pair(self, axis, width=1, out=None):
        """the edge strips of the live on-ocean planes for the east / north neighbour (hi) and the west / south one (lo).
        out: (hi, lo), each a flat float64 numpy array, a torch tensor on the handle's device, or None for a side without a
        neighbour; default two new numpy arrays.  Returns (hi, lo).  Device tensors: their pending work is waited for and
        the strips are in them on return (nothing crosses the bus)."""
        count = self.halo_buffer_count(axis, width)
        if out is None:
            out = (np.empty(count), np.empty(count))
        ptrs, dev = self._halo_buffers(out, count, "pack_halo_pair")
        if dev:
            self._halo_order_in(out)
        self._check(self.lib.kid_pack_halo_pair(self.h, int(axis), int(width), ptrs[0], ptrs[1], int(dev)), "kid_pack_halo_pair")
        if dev:
            self.sync()
        return tuple(out)

    def unpack_halo_pair(self, axis, from_lo, from_hi, width=1):
        """the neighbours' strips into this handle's halo: from_lo (what the west / south neighbour packed as hi) and from_hi,
        numpy arrays, torch device tensors or None for a missing side (that halo keeps its zeros)"""
        count = self.halo_buffer_count(axis, width)
        bufs = (from_lo, from_hi)
        if from_lo is None and from_hi is None:
            return
        ptrs, dev = self._halo_buffers(bufs, count, "unpack_halo_pair")
        if dev:
            self._halo_order_in(bufs)
        self._check(self.lib.kid_unpack_halo_pair(self.h, int(axis), int(width), ptrs[0], ptrs[1], int(dev)), "kid_unpack_halo_pair")
        if dev:
            self.sync()             # the tensors may be reused on return

    # ---- the tripolar north fold (IB:6110-6122; include/kid.h has the mapping) ----
    def unpack_halo_fold(self, from_fold, width=1, swap_slots=True):
        """the strip the mirror partner packed for the north (its pack_halo_pair(1, width)[0]) into this handle's rows beyond the
        fold, turned by 180 degrees; swap_slots: mirror the nine slots of every group as well (False: old_bug_rotated_weights).
        from_fold: a numpy array or a torch tensor on the handle's device"""
        count = self.halo_buffer_count(1, width)
        assert from_fold is not None, "unpack_halo_fold: a fold tile always has a partner"
        ptrs, dev = self._halo_buffers((from_fold,), count, "unpack_halo_fold")
        if dev:
            self._halo_order_in((from_fold,))
        self._check(self.lib.kid_unpack_halo_fold(self.h, int(width), ptrs[0], int(bool(swap_slots)), int(dev)), "kid_unpack_halo_fold")
        if dev:
            self.sync()             # the tensor may be reused on return

    def fold_halo_self(self, width=1, swap_slots=True):
        """the same for a handle that owns the whole zonal width and so is its own partner: planes to planes, no buffer"""
        self._check(self.lib.kid_fold_halo_self(self.h, int(width), int(bool(swap_slots))), "kid_fold_halo_self")

    # ---- restart files (icebergs_fms2io.F90:124-631, 663-1049) ----
    def write_restart(self, directory):
        self._check(self.lib.kid_write_restart(self.h, str(directory).encode()), "kid_write_restart")

    def read_restart(self, directory):
        self._check(self.lib.kid_read_restart(self.h, str(directory).encode()), "kid_read_restart")

    # ---- cells from positions: ignore_ij_restart / use_slow_find (IO2:876-891; include/kid.h) ----
    LOCATE_MODES = {"search": 1, "scan": 2}

    def locate_bergs(self, mode="search"):
        """the cell and xi, yj of every live resident berg from its lon, lat: "search" is find_cell_by_search (FW:5710-5842),
        "scan" is find_cell (FW:6011-6041).  Bergs no cell of the computational domain holds, or whose cell has no area, become
        dead rows.  Returns {"found", "lost", "grounded"}."""
        if mode not in self.LOCATE_MODES:
            raise ValueError("locate_bergs: mode is 'search' or 'scan', not %r" % (mode,))
        c = (C.c_int64 * 3)()
        self._check(self.lib.kid_locate_bergs(self.h, self.LOCATE_MODES[mode], c), "kid_locate_bergs")
        return {"found": int(c[0]), "lost": int(c[1]), "grounded": int(c[2])}

    def set_restart_locate(self, mode):
        """read_restart with ignore_ij_restart: None (the default) trusts the file's ine, jne; "search" or "scan" finds every
        berg's cell from its position, so a handle keeps the bergs of its own computational domain out of any file"""
        if mode is not None and mode not in self.LOCATE_MODES:
            raise ValueError("set_restart_locate: mode is None, 'search' or 'scan', not %r" % (mode,))
        self._check(self.lib.kid_set_restart_locate(self.h, 0 if mode is None else self.LOCATE_MODES[mode]), "kid_set_restart_locate")

    # ---- calving source (IB:5203-5231, accumulate_calving IB:6153, calve_icebergs IB:6225) ----
    def set_calving_params(self, cp):
        self._calv_params = cp
        self._check(self.lib.kid_set_calving_params(self.h, C.byref(cp)), "kid_set_calving_params")

    def set_calving_state(self, stored_ice=None, stored_heat=None, rmean_calving=None, rmean_calving_hflx=None):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (stored_ice, stored_heat, rmean_calving, rmean_calving_hflx)]
        if arrs[0] is not None:
            assert arrs[0].shape == (T.ENUMS["KID_NCLASSES"], self.nj, self.ni)
        self._check(self.lib.kid_set_calving_state(self.h, *[None if a is None else _dp(a) for a in arrs]), "kid_set_calving_state")

    def get_calving_state(self):
        nk = T.ENUMS["KID_NCLASSES"]
        out = {"stored_ice": np.empty((nk, self.nj, self.ni)), "stored_heat": np.empty((self.nj, self.ni)),
               "rmean_calving": np.empty((self.nj, self.ni)), "rmean_calving_hflx": np.empty((self.nj, self.ni)),
               "real_calving": np.empty((nk, self.nj, self.ni)), "calving": np.empty((self.nj, self.ni)), "calving_hflx": np.empty((self.nj, self.ni))}
        self._check(self.lib.kid_get_calving_state(self.h, _dp(out["stored_ice"]), _dp(out["stored_heat"]), _dp(out["rmean_calving"]),
                                                   _dp(out["rmean_calving_hflx"]), _dp(out["real_calving"])), "kid_get_calving_state")
        self._check(self.lib.kid_get_calving(self.h, _dp(out["calving"]), _dp(out["calving_hflx"])), "kid_get_calving")
        return out

    def calving(self, calving, calving_hflx, on_device=False):
        """kid_calving; arrays cover (isc:iec, jsc:jec) as (njc, nic) numpy, or device addresses with on_device.
        Returns the KID_CS_* scalar increments."""
        cin = T.CalvingIn()
        if on_device:
            cin.calving = C.cast(C.c_void_p(int(calving)), C.POINTER(C.c_double))
            cin.calving_hflx = C.cast(C.c_void_p(int(calving_hflx)), C.POINTER(C.c_double))
        else:
            d = self.grid["desc"]
            a = np.ascontiguousarray(calving, dtype=np.float64)
            b = np.ascontiguousarray(calving_hflx, dtype=np.float64)
            assert a.shape == b.shape == (d.jec - d.jsc + 1, d.iec - d.isc + 1), a.shape
            cin.calving, cin.calving_hflx = _dp(a), _dp(b)
        cin.on_device = int(on_device)
        scal = np.zeros(T.ENUMS["KID_NCALV_SCALARS"])
        self._check(self.lib.kid_calving(self.h, C.byref(cin), _dp(scal)), "kid_calving")
        return scal

    def set_forcing_device(self, dev_ptrs):
        """dev_ptrs: KID_NFORCING device addresses (0 keeps a plane); asynchronous on the handle's stream."""
        arr = (C.c_void_p * T.ENUMS["KID_NFORCING"])(*[C.c_void_p(int(x)) if x else None for x in dev_ptrs])
        self._check(self.lib.kid_set_forcing_device(self.h, arr), "kid_set_forcing_device")

    def step_prepare(self, dev_ptrs=None):
        """forcing prepass + accumulator zeroing of the coming step in one launch (dev_ptrs as set_forcing_device)"""
        if dev_ptrs is None:
            self._check(self.lib.kid_step_prepare(self.h, None), "kid_step_prepare")
            return
        key = tuple(int(x) if x else 0 for x in dev_ptrs)
        if getattr(self, "_prep_key", None) != key:   # the pointer table is rebuilt only when the addresses change
            self._prep_key = key
            self._prep_arr = (C.c_void_p * T.ENUMS["KID_NFORCING"])(*[C.c_void_p(x) if x else None for x in key])
        self._check(self.lib.kid_step_prepare(self.h, self._prep_arr), "kid_step_prepare")

    def set_params(self, params):
        self.params = params
        self._check(self.lib.kid_set_params(self.h, C.byref(params)), "kid_set_params")

    def set_side_stream(self, stream_ptr, enable=True):
        """enable: False/0 off, True/1 two half launches, 2 the slow-lane schedule (include/kid.h)"""
        self._check(self.lib.kid_set_side_stream(self.h, C.c_void_p(stream_ptr), int(enable)), "kid_set_side_stream")

    def set_stream(self, stream_ptr):
        self._check(self.lib.kid_set_stream(self.h, C.c_void_p(stream_ptr)), "kid_set_stream")

    # ---- berg population ----
    @staticmethod
    def _soa(bergs, n=None):
        s = T.BergSoA()
        s.n = len(bergs["lon"]) if n is None else n
        for k, name in enumerate(T.BERG_F64_NAMES):
            a = bergs[name]
            assert a.dtype == np.float64 and a.flags.c_contiguous
            s.f64[k] = _dp(a)
        for k, name in enumerate(T.BERG_I32_NAMES):
            a = bergs[name]
            assert a.dtype == np.int32 and a.flags.c_contiguous
            s.i32[k] = a.ctypes.data_as(C.POINTER(C.c_int32))
        s.id = bergs["id"].ctypes.data_as(C.POINTER(C.c_int64))
        return s

    def upload_bergs(self, bergs):
        """bergs["_n"] (optional) = number of live rows when the arrays carry spare rows"""
        s = self._soa(bergs, bergs.get("_n"))
        self._check(self.lib.kid_upload_bergs(self.h, C.byref(s)), "kid_upload_bergs")

    # ---- bonds (mts / dem) ----
    @staticmethod
    def _bond_soa(bonds, n):
        s = T.BondSoA()
        s.n, s.max_bonds = n, int(bonds["max_bonds"])
        assert len(bonds["count"]) == n and bonds["count"].dtype == np.int32
        s.count = bonds["count"].ctypes.data_as(C.POINTER(C.c_int32))
        s.other_id = bonds["other_id"].ctypes.data_as(C.POINTER(C.c_int64))
        s.broken = bonds["broken"].ctypes.data_as(C.POINTER(C.c_int32))
        for k, name in enumerate(T.BOND_F64_NAMES):
            a = bonds[name]
            assert a.dtype == np.float64 and len(a) == s.max_bonds * n
            s.f64[k] = _dp(a)
        return s

    def upload_bonds(self, bonds):
        n, _ = self.num_bergs()
        self._check(self.lib.kid_upload_bonds(self.h, C.byref(self._bond_soa(bonds, n))), "kid_upload_bonds")
        self._max_bonds = int(bonds["max_bonds"])

    def _bond_slots(self):
        """slots per berg of the handle's bond tables: those of the last upload_bonds, else the namelist's max_bonds (at least one)"""
        return getattr(self, "_max_bonds", None) or max(1, int(self.params.max_bonds))

    def download_bonds(self, max_bonds):
        from .synthetic import empty_bonds
        n, _ = self.num_bergs()
        bd = empty_bonds(n, max_bonds)
        self._check(self.lib.kid_download_bonds(self.h, C.byref(self._bond_soa(bd, n))), "kid_download_bonds")
        return bd

    def initialize_bonds(self, from_radii=True, length=None):
        """initialize_iceberg_bonds (IB:356-441) on the resident bergs: bonds every pair closer than 1.25 x the sum of its radii
        (from_radii) or than `length` metres; returns the number of bond records added (both ends counted).  include/kid.h has
        the ordering rules."""
        if not from_radii and length is None:
            raise ValueError("initialize_bonds: give a length or use from_radii")
        n = C.c_int64()
        self._check(self.lib.kid_initialize_bonds(self.h, 1 if from_radii else 0, 0.0 if length is None else float(length), C.byref(n)),
                    "kid_initialize_bonds")
        return n.value

    def count_bonds(self):
        """count_bonds (FW:5172-5285): (bond records on the computational domain, records without a matching partner)"""
        a, b = C.c_int64(), C.c_int64()
        self._check(self.lib.kid_count_bonds(self.h, C.byref(a), C.byref(b)), "kid_count_bonds")
        return a.value, b.value

    def set_conglom_ids(self):
        self._check(self.lib.kid_set_conglom_ids(self.h), "kid_set_conglom_ids")

    def evolve_icebergs_mts(self):
        self._check(self.lib.kid_evolve_icebergs_mts(self.h), "kid_evolve_icebergs_mts")

    def num_bergs(self):
        a, b = C.c_int64(), C.c_int64()
        self._check(self.lib.kid_num_bergs(self.h, C.byref(a), C.byref(b)), "kid_num_bergs")
        return a.value, b.value

    def download_bergs(self):
        from .synthetic import empty_bergs
        n, _ = self.num_bergs()
        b = empty_bergs(n)
        s = self._soa(b)
        self._check(self.lib.kid_download_bergs(self.h, C.byref(s)), "kid_download_bergs")
        return b

    def set_store_environment(self, on):
        self._check(self.lib.kid_set_store_environment(self.h, 1 if on else 0), "kid_set_store_environment")

    def set_reproducible_sums(self, on):
        """Bitwise-reproducible per-cell sums (the device side of parallel_reprod, include/kid.h); off by default."""
        self._check(self.lib.kid_set_reproducible_sums(self.h, 1 if on else 0), "kid_set_reproducible_sums")

    def bergs_chksum(self):
        """(chksum, chksum2, chksum3, chksum4, chksum5, #) of bergs_chksum (FW:6889-6987), as the reference prints them"""
        out = (C.c_int64 * 6)()
        self._check(self.lib.kid_bergs_chksum(self.h, out), "kid_bergs_chksum")
        return tuple(int(v) for v in out)

    def bergs_chksum_device(self, per_cell=False):
        """the same six integers from the resident state without the download (kid_bergs_chksum_device, include/kid.h); with
        per_cell: (integers, record of the '# of bergs/cell' line as a dict of the members of kid_grd_chksum)"""
        out, rec = (C.c_int64 * 6)(), T.GrdChksum()
        self._check(self.lib.kid_bergs_chksum_device(self.h, out, C.byref(rec) if per_cell else None), "kid_bergs_chksum_device")
        six = tuple(int(v) for v in out)
        return (six, _chk_record(rec)) if per_cell else six

    def checksum_gridded(self):
        """checksum_gridded (FW:6685-6758) on the device: {label: record} in the reference's order (types.CHK_LABELS), a record
        being the members of kid_grd_chksum as a dict"""
        recs = (T.GrdChksum * T.NCHK)()
        self._check(self.lib.kid_checksum_gridded(self.h, recs, T.NCHK), "kid_checksum_gridded")
        return {label: _chk_record(recs[k]) for k, label in enumerate(T.CHK_LABELS)}

    def checksum_report(self, label):
        """the lines the reference prints under `debug` at one point of icebergs_run (bergs_chksum, its '# of bergs/cell' record,
        then checksum_gridded: FW:6975, 6876, 6691, 6817), for the fields the handle holds"""
        six, per_cell = self.bergs_chksum_device(per_cell=True)
        lines = [format_bergs_chksum(label, six), format_grd_chksum("# of bergs/cell", per_cell), "KID: checksumming gridded data @ " + label.rstrip()]
        for name, rec in self.checksum_gridded().items():
            if rec["present"]:
                lines.append(format_grd_chksum(name, rec, three_d=name in T.CHK_3D))
        return lines

    # ---- the debug-mode invariants (check_position FW:6576, count_out_of_order FW:4039, check_for_duplicates FW:4118) ----
    CHECKS = {"position": T.ENUMS["KID_CHECK_POSITION"], "order": T.ENUMS["KID_CHECK_ORDER"], "duplicates": T.ENUMS["KID_CHECK_DUPLICATES"],
              "ids": T.ENUMS["KID_CHECK_IDS"], "all": T.ENUMS["KID_CHECK_ALL"]}

    def check_bergs(self, what="all"):
        """kid_check_bergs (include/kid.h) on the resident rows: the members of kid_check_report as a dict (first_id, first_row: lists
        of four, for xiyj, land, same_id, dup_ids).  what: a name of CHECKS, several of them, or the mask itself.  Offenders are
        reported, never raised."""
        if isinstance(what, str):
            what = (what,)
        mask = int(what) if isinstance(what, (int, np.integer)) else sum(self.CHECKS[w] for w in set(what))
        rep = T.CheckReport()
        self._check(self.lib.kid_check_bergs(self.h, mask, C.byref(rep)), "kid_check_bergs")
        out = {}
        for name, ct in T.CheckReport._fields_:
            v = getattr(rep, name)
            out[name] = [int(x) for x in v] if hasattr(ct, "_length_") else (float(v) if ct is C.c_double else int(v))
        return out

    def sorted_ids(self):
        """the ids of the live rows on the computational domain, ascending, duplicates kept (kid_sorted_ids): a numpy int64 array"""
        n = C.c_int64()
        self._check(self.lib.kid_sorted_ids(self.h, None, 0, C.byref(n)), "kid_sorted_ids")
        ids = np.empty(int(n.value), dtype=np.int64)
        if ids.size:
            self._check(self.lib.kid_sorted_ids(self.h, ids.ctypes.data_as(C.POINTER(C.c_int64)), ids.size, C.byref(n)), "kid_sorted_ids")
        return ids

    # ---- budgets (icebergs_stock_pe IB:8102-8133, icebergs_incr_mass IB:6046-6074, the budget block IB:5702-5727) ----
    def stock(self, index):
        """icebergs_stock_pe: index = types.ENUMS['KID_STOCK_WATER'] (kg) or ['KID_STOCK_HEAT'] (J); include/kid.h has the expression"""
        v = C.c_double()
        self._check(self.lib.kid_stock(self.h, int(index), C.byref(v)), "kid_stock")
        return v.value

    def budget(self):
        """the members of kid_budget_out (include/kid_types.h) as a dict: one device sweep, one 96-byte read"""
        out = T.BudgetOut()
        self._check(self.lib.kid_budget(self.h, C.byref(out)), "kid_budget")
        return {name: getattr(out, name) for name, _ in T.BudgetOut._fields_}

    def incr_mass(self, plane):
        """icebergs_incr_mass: adds the spread mass of the last gather (kg m-2) to `plane` in place.  `plane` covers the
        computational domain, shape (njc, nic): a C-contiguous float64 numpy array, or a torch tensor on the handle's device
        (then nothing crosses the bus: the tensor's pending work is waited for, the add runs on the handle's stream and is
        complete on return)."""
        if isinstance(plane, np.ndarray):
            assert plane.dtype == np.float64 and plane.flags.c_contiguous and plane.ndim == 2, "float64, C-contiguous, 2-d"
            self._check(self.lib.kid_incr_mass(self.h, plane.ctypes.data, 0, plane.shape[1], plane.shape[0]), "kid_incr_mass")
            return plane
        import torch
        assert isinstance(plane, torch.Tensor) and plane.is_cuda and plane.dtype == torch.float64 and plane.is_contiguous() and plane.dim() == 2
        assert plane.device.index == self.device, "the tensor lives on another device than the handle"
        torch.cuda.current_stream(plane.device).synchronize()
        self._check(self.lib.kid_incr_mass(self.h, plane.data_ptr(), 1, plane.shape[1], plane.shape[0]), "kid_incr_mass")
        self.sync()
        return plane

    def set_footloose_step(self, step):
        """continue the child-placement sequence of a restarted run (include/kid_rng.h)"""
        self._check(self.lib.kid_set_footloose_step(self.h, int(step)), "kid_set_footloose_step")

    def get_footloose_step(self):
        s = C.c_int64(0)
        self._check(self.lib.kid_get_footloose_step(self.h, C.byref(s)), "kid_get_footloose_step")
        return int(s.value)

    def adjust_fl_berg_interactivity(self):
        """adjust_fl_berg_interactivity (IB:5486): footloose children (fl_k = -1) that no other berg is in contact range of become
        interactive (fl_k = -2); returns how many did.  Nothing happens unless footloose and interactive_icebergs_on are both on."""
        n = C.c_int64(0)
        self._check(self.lib.kid_adjust_fl_berg_interactivity(self.h, C.byref(n)), "kid_adjust_fl_berg_interactivity")
        return int(n.value)

    def set_iceberg_counter(self, counter):
        a = np.ascontiguousarray(counter, dtype=np.int32)
        assert a.shape == (self.nj, self.ni)
        self._check(self.lib.kid_set_iceberg_counter(self.h, a.ctypes.data_as(C.POINTER(C.c_int32))), "kid_set_iceberg_counter")

    def get_iceberg_counter(self):
        a = np.zeros((self.nj, self.ni), dtype=np.int32)
        self._check(self.lib.kid_get_iceberg_counter(self.h, a.ctypes.data_as(C.POINTER(C.c_int32))), "kid_get_iceberg_counter")
        return a

    def move_berg_between_cells(self):
        """IB:5437: re-bin (stable sort by cell, dead bergs dropped)."""
        self._check(self.lib.kid_move_berg_between_cells(self.h), "kid_move_berg_between_cells")

    def set_resort_interval(self, steps):
        self._check(self.lib.kid_set_resort_interval(self.h, int(steps)), "kid_set_resort_interval")

    def compact(self):
        self._check(self.lib.kid_compact_bergs(self.h), "kid_compact_bergs")

    def set_bonds_follow_rows(self, on=True):
        """bond tables follow their rows through compact() and move_berg_between_cells() (True) or make both refuse (False, the
        default); kid_set_bonds_follow_rows in include/kid.h.  An int other than 0 or 1 is passed through and refused there."""
        self._check(self.lib.kid_set_bonds_follow_rows(self.h, int(on)), "kid_set_bonds_follow_rows")

    def bond_partner_rows(self):
        """(rows, slots), each (max_bonds, n) int32: where the kernels find the other end of every bond, -1 past a list's end and
        where no partner row is known (kid_bond_partner_rows, a hook for tests)"""
        n, _ = self.num_bergs()
        mb = self._bond_slots()
        rows, slots = np.full((mb, n), -1, dtype=np.int32), np.full((mb, n), -1, dtype=np.int32)
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.kid_bond_partner_rows(self.h, rows.ctypes.data_as(ip), slots.ctypes.data_as(ip), n), "kid_bond_partner_rows")
        return rows, slots

    # ---- growable capacity (include/kid.h): host buffers are sized from num_bergs(), never from the capacity of __init__ ----
    @property
    def capacity(self):
        """the handle's current row capacity: what __init__ was given, or what reserve / auto-reserve have made of it since"""
        n = C.c_int64()
        self._check(self.lib.kid_capacity(self.h, C.byref(n)), "kid_capacity")
        return n.value

    def reserve(self, rows):
        """make the capacity at least `rows` (never shrinks); rows keep their numbers, so bonds and halo rows survive"""
        self._check(self.lib.kid_reserve(self.h, int(rows)), "kid_reserve")

    def set_auto_reserve(self, min_free, growth=1.5, max_capacity=0):
        """the calls that append rows grow the handle before they write: to max(need, ceil(capacity * growth)), at most
        max_capacity (0: 2^29); a footloose launch is given `min_free` free rows.  growth=0 switches it off (the default)."""
        self._check(self.lib.kid_set_auto_reserve(self.h, int(min_free), float(growth), int(max_capacity)), "kid_set_auto_reserve")

    # ---- icebergs_run, the hot-path part (IB:5423-5512) ----
    def run(self, nsteps=1):
        """Fused path: per step one per-berg launch (evolve + thermodynamics + spreading) and one gather."""
        self._check(self.lib.kid_run_step(self.h, int(nsteps)), "kid_run_step")

    def step_local(self):
        self._check(self.lib.kid_step_local(self.h), "kid_step_local")

    def step_gather(self):
        self._check(self.lib.kid_step_gather(self.h), "kid_step_gather")

    def run_phases(self, nsteps=1):
        """Phase-by-phase path: exactly the reference's call sequence inside icebergs_run."""
        p = self.params
        for _ in range(nsteps):
            self._check(self.lib.kid_zero_accumulators(self.h), "kid_zero_accumulators")          # IB:5125-5156
            if not p.mts and not p.old_interp_flds_order:
                self._check(self.lib.kid_interp_gridded_fields_to_bergs(self.h), "interp")          # IB:5423
            self._check(self.lib.kid_evolve_icebergs(self.h), "kid_evolve_icebergs")               # IB:5433
            if p.footloose:
                self._check(self.lib.kid_footloose_calving(self.h), "kid_footloose_calving")       # IB:5453
            if not p.old_interp_flds_order:
                self._check(self.lib.kid_interp_gridded_fields_to_bergs(self.h), "interp")          # IB:5473
            self._check(self.lib.kid_thermodynamics(self.h), "kid_thermodynamics")                 # IB:5505
            self._check(self.lib.kid_create_gridded_icebergs_fields(self.h), "kid_create_gridded") # IB:5512

    def fetch(self):
        self._check(self.lib.kid_get_accumulators(self.h, _dp(self.acc), _dp(self.out), _dp(self.scalars)), "kid_get_accumulators")
        return self.acc, self.out, self.scalars

    def sync(self):
        self._check(self.lib.kid_sync(self.h), "kid_sync")

    def accum_device_ptr(self):
        p, n = C.c_void_p(), C.c_int64()
        self._check(self.lib.kid_accum_device_ptr(self.h, C.byref(p), C.byref(n)), "kid_accum_device_ptr")
        return p.value, n.value

    def accum_live_count(self):
        """doubles from the start of the accumulator block that a sharded run sums across GPUs (include/kid.h)"""
        n = C.c_int64()
        self._check(self.lib.kid_accum_live_count(self.h, C.byref(n)), "kid_accum_live_count")
        return n.value

    def bind_accum_buffer(self, ptr, count):
        self._check(self.lib.kid_bind_accum_buffer(self.h, C.c_void_p(ptr), int(count)), "kid_bind_accum_buffer")

    def bind_spread_mass_old(self, ptr, count):
        """find_melt_using_spread_mass in a sharded run: the two planes the ranks must sum (include/kid.h)"""
        self._check(self.lib.kid_bind_spread_mass_old(self.h, ptr, int(count)), "kid_bind_spread_mass_old")

    def last_redo_count(self):
        c = C.c_int64()
        self._check(self.lib.kid_last_redo_count(self.h, C.byref(c)), "kid_last_redo_count")
        return c.value

    def rebin_fused_count(self):
        """re-binnings whose copy the following plain hot build took over (include/kid.h); 0 with KID_REBIN_EAGER=1"""
        c = C.c_int64()
        self._check(self.lib.kid_rebin_fused_count(self.h, C.byref(c)), "kid_rebin_fused_count")
        return c.value

    def hot_zero_mask(self):
        """fields the last hot-build launch neither loaded nor stored, as a set of member names (include/kid.h); empty with KID_NO_ZERO_SKIP=1"""
        m = C.c_uint64()
        self._check(self.lib.kid_hot_zero_mask(self.h, C.byref(m)), "kid_hot_zero_mask")
        return {name for f, name in enumerate(T.BERG_F64_NAMES) if (m.value >> f) & 1}

    def cold_state(self):
        """(deferred, materialised): are cold fields waiting behind a row permutation now, and how many times have they been
        gathered into row order so far (kid_cold_state, a hook for tests; nothing deferred ever with KID_COLD_EAGER=1)"""
        d, m = C.c_int32(), C.c_int64()
        self._check(self.lib.kid_cold_state(self.h, C.byref(d), C.byref(m)), "kid_cold_state")
        return bool(d.value), m.value

    def mts_fused_launches(self):
        """how many times the MTS sub-step loop went out as the one cooperative launch so far (kid_mts_fused_launches, a hook
        for tests; stays 0 with KID_MTS_NO_FUSED=1 or when the population does not fit)"""
        c = C.c_int64()
        self._check(self.lib.kid_mts_fused_launches(self.h, C.byref(c)), "kid_mts_fused_launches")
        return c.value

    def profile(self, on=True):
        self._check(self.lib.kid_profile_enable(self.h, 1 if on else 0), "kid_profile_enable")

    def profile_get(self):
        a, n, b = C.c_double(), C.c_int64(), C.c_double()
        self._check(self.lib.kid_profile_get(self.h, C.byref(a), C.byref(n), C.byref(b)), "kid_profile_get")
        return a.value, n.value, b.value
