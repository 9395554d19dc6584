"""Domain-decomposed runs: one tile of the ocean grid and one handle per rank, bergs migrating between ranks.

This is the reference's own parallel layout (send_bergs_to_other_pes, icebergs_framework.F90:2997-3247) with
`torch.distributed` point-to-point messages where the reference has mpp_send / mpp_recv: per exchange pass the two counts,
then the records in the reference's wire format (pack_berg_into_buffer2, FW:3250-3301).  East/west first, then north/south
(FW:3022-3230), so a berg that leaves through a corner hops twice.  Inside one node `distributed.py` replicates the grid and
shards the bergs by index instead (no exchange at all); this module is for grids that should not be replicated, or for
several nodes.

The tile only needs `pack_pair(axis)` -> (records for the east/north neighbour, records for the west/south neighbour) and
`unpack_pair(from_west_or_south, from_east_or_north)`: `HipTile` wraps an `Icebergs` handle; the CPU tests plug the oracle
in the same way.

The second exchange of a step is the halo update of the on-ocean planes before the 9-point gather (mpp_update_domains in
sum_up_spread_fields, IB:6106-6107): `TileExchange.update_halos`, with fixed-size messages, east/west then north/south so that
a diagonal neighbour's corner arrives in two hops.  `TileExchange.step` is one step of icebergs_run for a tile with both
exchanges in their places; for it the tile also offers the phases (`zero_accumulators`, `interp`, `evolve`, `thermodynamics`,
`calculate_mass_on_ocean`, `gather`), its `params`, and `halo_buffer_count(axis, width)`, `pack_halo_pair(axis, width, sides)`
-> (strip for the east/north neighbour, strip for the west/south one; None where `sides` says there is no neighbour) and
`unpack_halo_pair(axis, from_lo, from_hi, width)`.

The third exchange is for interacting bergs: `TileExchange.update_halo_bergs` brings copies of the neighbours' bergs next to the
shared edges (update_halo_icebergs, FW:1800-2131) so that contact forces cross tile edges, and `TileExchange.step_interactive`
is the step that uses it.  The tile offers `pack_halo_bergs_pair(axis, width, sides)` -> (records for the east/north neighbour,
for the west/south one) and `set_conglom_ids()`; the records come in through `unpack_pair`.

A tripolar grid closes its north edge on itself (FOLD_NORTH_EDGE): `TileExchange(..., fold_north=True)` gives a tile of the top
row its mirror tile as the partner beyond the fold (grd%pe_N of FW:3138-3195).  The partner's north strip of the on-ocean planes
arrives turned by 180 degrees (`unpack_halo_fold`, or `fold_halo_self` where the tile is its own partner; IB:6110-6122), and a
berg that walks north over the fold arrives on the partner with its cell index mirrored.  For this the tile also offers
`comp_domain()` -> (isc, iec, jsc, jec), `unpack_halo_fold(from_fold, width, swap_slots)` and `fold_halo_self(width, swap_slots)`.
"""
import numpy as np
import torch

WIDTH = 34  # buffer_width without bonds, FW:21
W_INE, W_JNE = 23, 24  # reals 24 and 25 of the wire record (pack_berg_into_buffer2, FW:3291-3292), 0-based


class HipTile:
    """the migration calls of one handle (kid_pack_emigrants_pair / kid_unpack_immigrants_pair), its halo calls
    (kid_pack_halo_pair / kid_unpack_halo_pair, host buffers: the messages of TileExchange leave from the host, as the berg
    records do) and the phases of a step"""

    def __init__(self, icebergs):
        self.ib = icebergs
        self._halo_out = {}

    @property
    def params(self):
        return self.ib.params

    def _call(self, name):
        self.ib._check(getattr(self.ib.lib, name)(self.ib.h), name)

    def zero_accumulators(self):
        self._call("kid_zero_accumulators")

    def interp(self):
        self._call("kid_interp_gridded_fields_to_bergs")

    def evolve(self):
        self._call("kid_evolve_icebergs")

    def thermodynamics(self):
        self._call("kid_thermodynamics")

    def calculate_mass_on_ocean(self):
        self.ib.calculate_mass_on_ocean()

    def gather(self):
        self.ib.step_gather()

    def halo_buffer_count(self, axis, width=1):
        return self.ib.halo_buffer_count(axis, width)

    def pack_halo_pair(self, axis, width=1, sides=(True, True)):
        count = self.halo_buffer_count(axis, width)
        if (axis, count) not in self._halo_out:       # the send buffers are kept: a step packs the same sizes every time
            self._halo_out[(axis, count)] = (np.empty(count), np.empty(count))
        out = tuple(b if on else None for b, on in zip(self._halo_out[(axis, count)], sides))
        if out[0] is None and out[1] is None:
            return out
        return self.ib.pack_halo_pair(axis, width, out=out)

    def unpack_halo_pair(self, axis, from_lo, from_hi, width=1):
        self.ib.unpack_halo_pair(axis, from_lo, from_hi, width)

    def unpack_halo_fold(self, from_fold, width=1, swap_slots=True):
        self.ib.unpack_halo_fold(from_fold, width, swap_slots)

    def fold_halo_self(self, width=1, swap_slots=True):
        self.ib.fold_halo_self(width, swap_slots)

    def comp_domain(self):
        d = self.ib.grid["desc"]
        return d.isc, d.iec, d.jsc, d.jec

    def pack_pair(self, axis):
        return self.ib.pack_emigrants_pair(axis)

    def pack_halo_bergs_pair(self, axis, width=0, sides=(True, True)):
        return self.ib.pack_halo_bergs_pair(axis, width, sides)

    def set_conglom_ids(self):
        self.ib.set_conglom_ids()

    def unpack_pair(self, from_lo, from_hi):
        self.ib.unpack_immigrants_pair(from_lo, from_hi)

    # growable capacity, per tile: a TileExchange run opts in for the tiles that need it
    @property
    def capacity(self):
        return self.ib.capacity

    def reserve(self, rows):
        self.ib.reserve(rows)

    def set_auto_reserve(self, min_free, growth=1.5, max_capacity=0):
        self.ib.set_auto_reserve(min_free, growth, max_capacity)

    # cells from positions, per tile: a tile that reads a global file keeps the bergs of its own computational domain
    def locate_bergs(self, mode="search"):
        return self.ib.locate_bergs(mode)

    def set_restart_locate(self, mode):
        self.ib.set_restart_locate(mode)

    # the debug-mode invariants, per tile (halo copies may be resident)
    def check_bergs(self, what="all"):
        return self.ib.check_bergs(what)

    def sorted_ids(self):
        return self.ib.sorted_ids()


class TileExchange:
    """ranks laid out as an ntx x nty array of tiles, rank = ty * ntx + tx (x fastest, like the reference's domain layout);
    a tile on the edge of the box has no neighbour there (NULL_PE: its leavers are packed and dropped, FW:3050) unless
    cyclic_x closes the zonal direction or fold_north the north edge: the partner of tile (tx, nty-1) beyond the fold is
    (ntx-1-tx, nty-1), the tile itself for ntx == 1 and for the middle tile of an odd ntx.  fold_north needs tiles of one width
    (tile_widths: the computational columns of every tile column, where the caller knows them; they must all be equal), since
    only then is a tile's mirror image one tile"""

    def __init__(self, ntx, nty, dist, rank=None, cyclic_x=False, device="cpu", fold_north=False, tile_widths=None):
        self.ntx, self.nty, self.dist, self.device = int(ntx), int(nty), dist, device
        self.rank = dist.get_rank() if rank is None else int(rank)
        assert dist.get_world_size() == self.ntx * self.nty, "one rank per tile"
        self.tx, self.ty = self.rank % self.ntx, self.rank // self.ntx
        self.cyclic_x = bool(cyclic_x)
        self.fold_north = bool(fold_north)
        if self.fold_north and tile_widths is not None:
            assert len(tile_widths) == self.ntx and len(set(int(w) for w in tile_widths)) == 1, "fold_north needs tiles that are uniform in x"
        self._fold_nic = None if tile_widths is None else int(tile_widths[0])
        self._fold_checked = False
        self.sent = 0          # records handed to neighbours so far
        self.received = 0
        self.fold_records = np.empty((0, WIDTH))   # what the last exchange brought over the fold, cell indices already mirrored

    def neighbour(self, dx, dy):
        tx, ty = self.tx + dx, self.ty + dy
        if self.cyclic_x and self.ntx > 1:
            tx %= self.ntx
        if tx < 0 or tx >= self.ntx or ty < 0 or ty >= self.nty:
            return None
        return ty * self.ntx + tx

    def fold_partner(self):
        """the rank beyond the north fold (grd%pe_N of a top-row PE, FW:3138-3195); None for a tile below the top row or without fold_north"""
        if not self.fold_north or self.ty != self.nty - 1:
            return None
        return self.ty * self.ntx + (self.ntx - 1 - self.tx)

    def _fold_width_check(self, tile):
        """uniform in x: this tile has the width the caller gave (tile_widths) and, asked of the partner once, the partner's"""
        isc, iec, _, _ = tile.comp_domain()
        nic = iec - isc + 1
        assert self._fold_nic is None or nic == self._fold_nic, "fold_north needs tiles that are uniform in x"
        self._fold_nic = nic
        partner = self.fold_partner()
        if self._fold_checked or partner == self.rank:
            return
        dist = self.dist
        mine = torch.tensor([nic], dtype=torch.int64, device=self.device)
        theirs = torch.zeros(1, dtype=torch.int64, device=self.device)
        for w in dist.batch_isend_irecv([dist.P2POp(dist.isend, mine, partner), dist.P2POp(dist.irecv, theirs, partner)]):
            w.wait()
        assert int(theirs.item()) == nic, "fold_north needs tiles that are uniform in x"
        self._fold_checked = True

    def _swap(self, to_hi, hi, to_lo, lo):
        """send `to_hi` to rank `hi` and `to_lo` to rank `lo`; returns (from_lo, from_hi).  Counts first, then the records
        (FW:3050-3097: mpp_send of nbergs_to_send, then of the buffer)"""
        dist = self.dist
        if hi is not None and hi == lo:        # two tiles across a cyclic direction: both neighbours are the same rank
            return self._swap_same_peer(to_hi, to_lo, hi)
        out = {hi: to_hi, lo: to_lo}
        counts_in = {}
        ops, keep = [], []
        for peer, recs in ((hi, to_hi), (lo, to_lo)):
            if peer is None:
                continue
            c = torch.tensor([len(recs)], dtype=torch.int64, device=self.device)
            r = torch.zeros(1, dtype=torch.int64, device=self.device)
            keep.append(c)
            counts_in[peer] = r
            ops += [dist.P2POp(dist.isend, c, peer), dist.P2POp(dist.irecv, r, peer)]
        if ops:
            for w in dist.batch_isend_irecv(ops):
                w.wait()
        ops, got = [], {}
        for peer in (hi, lo):
            if peer is None:
                continue
            if len(out[peer]):
                t = torch.from_numpy(np.ascontiguousarray(out[peer])).to(self.device)
                keep.append(t)
                ops.append(dist.P2POp(dist.isend, t, peer))
            n_in = int(counts_in[peer].item())
            if n_in:
                got[peer] = torch.empty((n_in, WIDTH), dtype=torch.float64, device=self.device)
                ops.append(dist.P2POp(dist.irecv, got[peer], peer))
        if ops:
            for w in dist.batch_isend_irecv(ops):
                w.wait()
        empty = np.empty((0, WIDTH))
        from_lo = got[lo].cpu().numpy() if lo in got else empty
        from_hi = got[hi].cpu().numpy() if hi in got else empty
        self.sent += (len(to_hi) if hi is not None else 0) + (len(to_lo) if lo is not None else 0)
        self.received += len(from_lo) + len(from_hi)
        return from_lo, from_hi

    def _swap_same_peer(self, to_hi, to_lo, peer):
        """ntx == 2 with cyclic_x: the east and the west neighbour are the same rank.  One message each way carrying both
        groups, the first row saying how many belong to the first group."""
        dist = self.dist
        mine = np.concatenate([np.full((1, WIDTH), float(len(to_hi))), to_hi, to_lo]) if len(to_hi) + len(to_lo) else np.full((1, WIDTH), 0.0)
        c = torch.tensor([len(mine)], dtype=torch.int64, device=self.device)
        r = torch.zeros(1, dtype=torch.int64, device=self.device)
        for w in dist.batch_isend_irecv([dist.P2POp(dist.isend, c, peer), dist.P2POp(dist.irecv, r, peer)]):
            w.wait()
        t = torch.from_numpy(np.ascontiguousarray(mine)).to(self.device)
        g = torch.empty((int(r.item()), WIDTH), dtype=torch.float64, device=self.device)
        for w in dist.batch_isend_irecv([dist.P2POp(dist.isend, t, peer), dist.P2POp(dist.irecv, g, peer)]):
            w.wait()
        theirs = g.cpu().numpy()
        k = int(theirs[0, 0])
        # what the peer sent east arrives here from the west, and the other way round
        from_lo, from_hi = theirs[1:1 + k], theirs[1 + k:]
        self.sent += len(to_hi) + len(to_lo)
        self.received += len(from_lo) + len(from_hi)
        return from_lo, from_hi

    def check_duplicates(self, tile):
        """check_for_duplicates_in_parallel (FW:7344-7379) with the cross-PE half of check_for_duplicate_ids_in_list (FW:7424-7450):
        every rank contributes `tile.sorted_ids()` (ascending int64, duplicates kept) -- the counts first, then the ids padded to the
        longest list.  Returns (duplicates on a rank, summed over the ranks; ids that more than one rank owns), the same pair on every
        rank.  Nothing is raised: the reference stops on either being non-zero, here the caller decides."""
        dist = self.dist
        ids = np.ascontiguousarray(np.asarray(tile.sorted_ids(), dtype=np.int64))
        world = dist.get_world_size()
        mine = torch.tensor([len(ids)], dtype=torch.int64, device=self.device)
        counts = [torch.zeros(1, dtype=torch.int64, device=self.device) for _ in range(world)]
        dist.all_gather(counts, mine)
        counts = [int(c.item()) for c in counts]
        longest = max(counts)
        if longest == 0:      # FW:7358: no bergs anywhere
            return 0, 0
        padded = torch.zeros(longest, dtype=torch.int64, device=self.device)
        padded[:len(ids)] = torch.from_numpy(ids).to(self.device)
        lists = [torch.empty(longest, dtype=torch.int64, device=self.device) for _ in range(world)]
        dist.all_gather(lists, padded)
        per_rank = [t.cpu().numpy()[:c] for t, c in zip(lists, counts)]
        on_a_rank = sum(int(np.count_nonzero(a[1:] == a[:-1])) for a in per_rank)    # FW:7418-7423
        owners = np.concatenate([np.unique(a) for a in per_rank])                    # one entry per (rank, id)
        _, seen = np.unique(owners, return_counts=True)
        return on_a_rank, int(np.count_nonzero(seen > 1))                            # FW:7444: ii > 1

    def exchange(self, tile):
        """send_bergs_to_other_pes for this rank's tile: call it between evolve_icebergs and thermodynamics (IB:5447)"""
        partner = self.fold_partner()
        self.fold_records = np.empty((0, WIDTH))
        for axis, (dx, dy) in enumerate(((1, 0), (0, 1))):
            to_hi, to_lo = tile.pack_pair(axis)
            hi, lo = self.neighbour(dx, dy), self.neighbour(-dx, -dy)
            if axis == 1 and partner is not None:
                # over the fold: what a top-row tile sends north goes to its mirror tile, and what that tile sent north arrives
                # here from the north.  The partner sits in this tile's own row, so nothing else travels between the two in
                # this pass, and the east/west pass has been waited for: the messages cannot be taken for one another
                # (the reference gives them tags of their own, COMM_TAG_9/10, FW:3138-3195).
                self._fold_width_check(tile)
                if partner == self.rank:
                    from_lo, _ = self._swap(to_hi[:0], None, to_lo, lo)
                    from_hi = to_hi.copy()                    # straight back
                    self.sent += len(to_hi)
                    self.received += len(from_hi)
                else:
                    from_lo, from_hi = self._swap(to_hi, partner, to_lo, lo)
                if len(from_hi):
                    # the sender's cell (i, jec+k) beyond its north edge is this tile's cell (isc+iec-i, jec+1-k): with it the
                    # first guess of the unpack holds (the reference scans for the cell and finds the same one)
                    isc, iec, _, jec = tile.comp_domain()
                    from_hi = np.array(from_hi, dtype=np.float64)
                    from_hi[:, W_INE] = (isc + iec) - from_hi[:, W_INE]
                    from_hi[:, W_JNE] = (2 * jec + 1) - from_hi[:, W_JNE]
                    self.fold_records = from_hi
            else:
                from_lo, from_hi = self._swap(to_hi, hi, to_lo, lo)
            if len(from_lo) or len(from_hi):
                tile.unpack_pair(from_lo, from_hi)            # from the west / south first, FW:3064, 3160

    def update_halo_bergs(self, tile, width=None):
        """update_halo_icebergs (FW:1800-2131) for this rank's tile: copies of the neighbours' bergs next to the shared edges
        arrive as halo rows, force sources for the evolve that follows and retires them.  East/west, then north/south over the
        columns of the whole data domain, which carry what the first pass has brought: a diagonal neighbour's bergs arrive in
        two hops.  Counts, then records, as the migration.  width None: the grid's halo."""
        if self.cyclic_x:
            raise ValueError("TileExchange.update_halo_bergs does not cover cyclic_x (update_latlon, IB:5467; DESIGN 7.6, out of scope)")
        if self.fold_north:
            raise ValueError("TileExchange.update_halo_bergs does not cover fold_north (halo bergs across the fold; DESIGN 7.6, out of scope)")
        w = 0 if width is None else int(width)
        for axis, (dx, dy) in enumerate(((1, 0), (0, 1))):
            hi, lo = self.neighbour(dx, dy), self.neighbour(-dx, -dy)
            if hi is None and lo is None:
                continue
            to_hi, to_lo = tile.pack_halo_bergs_pair(axis, w, (hi is not None, lo is not None))
            from_lo, from_hi = self._swap(to_hi, hi, to_lo, lo)
            if len(from_lo) or len(from_hi):
                tile.unpack_pair(from_lo, from_hi)

    def step_interactive(self, tile, width=1, halo_width=None):
        """one step of icebergs_run for a tile of unbonded interacting bergs under the single-time-step Verlet scheme.
        The halo bergs are taken right before the evolve (the reference takes them before the thermodynamics of the step
        before, IB:5462, so that a copy carries its owner's size of one melt earlier): a tile run sees what the undivided run sees."""
        p = tile.params
        if self.fold_north:
            raise ValueError("TileExchange.step_interactive does not cover fold_north (halo bergs across the fold; DESIGN 7.6, out of scope)")
        if not p.interactive_icebergs_on:
            raise ValueError("TileExchange.step_interactive needs interactive_icebergs_on; TileExchange.step covers the rest")
        for switch in ("find_melt_using_spread_mass", "mts", "iceberg_bonds_on", "footloose", "Runge_not_Verlet"):
            if getattr(p, switch):
                raise ValueError("TileExchange.step_interactive does not cover %s on tiles (DESIGN 7.6, out of scope)" % switch)
        tile.zero_accumulators()                 # IB:5125-5156
        if not p.old_interp_flds_order:
            tile.interp()                        # IB:5423
        self.update_halo_bergs(tile, halo_width)  # IB:5462, moved here
        if p.contact_distance > 0.0 or p.contact_spring_coef != p.spring_coef:
            tile.set_conglom_ids()               # IB:5470-5471, with the halo rows resident
        tile.evolve()                            # IB:5433; retires the halo rows
        self.exchange(tile)                      # IB:5447
        if not p.old_interp_flds_order:
            tile.interp()                        # IB:5473
        tile.thermodynamics()                    # IB:5505
        tile.calculate_mass_on_ocean()           # IB:5512 -> IB:4984
        self.update_halos(tile, width)           # IB:6106-6107
        tile.gather()                            # IB:6126-6150, 3419-3488

    def _swap_halo(self, to_hi, hi, to_lo, lo, count):
        """the strips of one axis (numpy, `count` doubles each): `to_hi` to rank `hi`, `to_lo` to rank `lo`; returns
        (from_lo, from_hi), None where there is no neighbour.  Both sides know `count`, so there is no count message."""
        dist = self.dist
        if hi is None and lo is None:
            return None, None
        if hi == lo:
            # two tiles across a cyclic direction: one message each way, the strip sent east first.  What the peer sent east
            # arrives here from the west, and the other way round.
            mine = torch.from_numpy(np.concatenate([to_hi, to_lo])).to(self.device)
            theirs = torch.empty(2 * count, dtype=torch.float64, device=self.device)
            for w in dist.batch_isend_irecv([dist.P2POp(dist.isend, mine, hi), dist.P2POp(dist.irecv, theirs, hi)]):
                w.wait()
            theirs = theirs.cpu().numpy()
            return theirs[:count].copy(), theirs[count:].copy()
        ops, keep, got = [], [], {}
        for peer, strip in ((hi, to_hi), (lo, to_lo)):
            if peer is None:
                continue
            t = torch.from_numpy(strip).to(self.device)
            got[peer] = torch.empty(count, dtype=torch.float64, device=self.device)
            keep.append(t)
            ops += [dist.P2POp(dist.isend, t, peer), dist.P2POp(dist.irecv, got[peer], peer)]
        for w in dist.batch_isend_irecv(ops):
            w.wait()
        return (got[lo].cpu().numpy() if lo is not None else None), (got[hi].cpu().numpy() if hi is not None else None)

    def update_halos(self, tile, width=1):
        """mpp_update_domains(var_on_ocean) of sum_up_spread_fields (IB:6106-6107) for this rank's tile: call it between
        calculate_mass_on_ocean and the gather.  East/west over the computational rows, then north/south over the columns
        isc-width .. iec+width, which carry the corners the first pass has filled.  With fold_north a top-row tile sends its north
        strip to its mirror tile and takes that tile's strip turned by 180 degrees (IB:6110-6122), slots swapped unless
        old_bug_rotated_weights."""
        partner = self.fold_partner()
        for axis, (dx, dy) in enumerate(((1, 0), (0, 1))):
            hi, lo = self.neighbour(dx, dy), self.neighbour(-dx, -dy)
            if axis == 1 and partner is not None:
                self._fold_width_check(tile)
                swap_slots = not tile.params.old_bug_rotated_weights
                count = tile.halo_buffer_count(axis, width)
                own = partner == self.rank
                to_hi, to_lo = tile.pack_halo_pair(axis, width, (not own, lo is not None))
                from_lo, from_fold = self._swap_halo(to_hi, None if own else partner, to_lo, lo, count)   # (ordering: see exchange)
                if own:
                    tile.fold_halo_self(width, swap_slots)
                else:
                    tile.unpack_halo_fold(from_fold, width, swap_slots)
                tile.unpack_halo_pair(axis, from_lo, None, width)
                continue
            if hi is None and lo is None:
                continue
            count = tile.halo_buffer_count(axis, width)
            to_hi, to_lo = tile.pack_halo_pair(axis, width, (hi is not None, lo is not None))
            from_lo, from_hi = self._swap_halo(to_hi, hi, to_lo, lo, count)
            tile.unpack_halo_pair(axis, from_lo, from_hi, width)

    def step(self, tile, width=1):
        """one step of icebergs_run for this rank's tile in the reference's order (IB:5125-5512): both exchanges in place"""
        p = tile.params
        for switch in ("find_melt_using_spread_mass", "mts", "interactive_icebergs_on", "footloose"):
            if getattr(p, switch):
                raise ValueError("TileExchange.step does not cover %s on tiles (DESIGN 7.5, out of scope)" % switch)
        tile.zero_accumulators()                 # IB:5125-5156
        if not p.old_interp_flds_order:
            tile.interp()                        # IB:5423
        tile.evolve()                            # IB:5433
        self.exchange(tile)                      # IB:5447
        if not p.old_interp_flds_order:
            tile.interp()                        # IB:5473
        tile.thermodynamics()                    # IB:5505
        tile.calculate_mass_on_ocean()           # IB:5512 -> IB:4984
        self.update_halos(tile, width)           # IB:6106-6107
        tile.gather()                            # IB:6126-6150, 3419-3488
