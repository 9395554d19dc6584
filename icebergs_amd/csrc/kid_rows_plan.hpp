// kid_rows_plan.hpp -- what the host decides about berg rows, as plain C++17: no HIP header, no handle.  The wire record of a
// berg (kid_migrate.inc packs and decodes it, kid_halo_bergs.inc packs it) and the skip rule of the row permutation
// (kid_rows.inc) are written down here once; tests/rows_plan_host.cpp enumerates both on the host.  So are the cold fields
// (tests/cold_rows_host.cpp) and what a row permutation does to a bond's reference to its partner (tests/bond_rows_host.cpp).
#pragma once
#include "../../include/kid_types.h"

namespace kid {

// pack_berg_into_buffer2 without bonds, FW:3268-3301: buffer_width reals per berg, integers as reals.  One entry per word,
// in wire order: its kind and, where there is one, the member of the SoA it carries.
enum WireKind { WIRE_F64, WIRE_I32, WIRE_INE, WIRE_JNE, WIRE_ID_HI, WIRE_ID_LO };   // fp64 member; int32 member as a real; the cell; the two halves of split_id (FW:3297-3299)
struct WireWord { WireKind kind; int field; };
constexpr WireWord WIRE_RECORD[] = {
  {WIRE_F64, KID_B_LON}, {WIRE_F64, KID_B_LAT}, {WIRE_F64, KID_B_UVEL}, {WIRE_F64, KID_B_VVEL},
  {WIRE_F64, KID_B_UVEL_PREV}, {WIRE_F64, KID_B_VVEL_PREV}, {WIRE_F64, KID_B_XI}, {WIRE_F64, KID_B_YJ},
  {WIRE_F64, KID_B_START_LON}, {WIRE_F64, KID_B_START_LAT}, {WIRE_I32, KID_BI_START_YEAR}, {WIRE_F64, KID_B_START_DAY},
  {WIRE_F64, KID_B_START_MASS}, {WIRE_F64, KID_B_MASS}, {WIRE_F64, KID_B_THICKNESS}, {WIRE_F64, KID_B_WIDTH},
  {WIRE_F64, KID_B_LENGTH}, {WIRE_F64, KID_B_FL_K}, {WIRE_F64, KID_B_MASS_SCALING}, {WIRE_F64, KID_B_MASS_OF_BITS},
  {WIRE_F64, KID_B_MASS_OF_FL_BITS}, {WIRE_F64, KID_B_MASS_OF_FL_BERGY_BITS}, {WIRE_F64, KID_B_HEAT_DENSITY},
  {WIRE_INE, KID_BI_INE}, {WIRE_JNE, KID_BI_JNE},
  {WIRE_F64, KID_B_AXN}, {WIRE_F64, KID_B_AYN}, {WIRE_F64, KID_B_BXN}, {WIRE_F64, KID_B_BYN},
  {WIRE_F64, KID_B_HALO_BERG}, {WIRE_F64, KID_B_STATIC_BERG}, {WIRE_ID_HI, -1}, {WIRE_ID_LO, -1},
  {WIRE_F64, KID_B_OD},
};
constexpr int MIG_WIDTH = (int)(sizeof(WIRE_RECORD) / sizeof(WIRE_RECORD[0]));
static_assert(MIG_WIDTH == 34, "buffer_width without bonds, mts and dem (FW:21)");

// the word that carries a member (or, for the kinds that occur once, the word of that kind)
constexpr int wire_word(WireKind kind, int field) {
  for (int w = 0; w < MIG_WIDTH; ++w)
    if (WIRE_RECORD[w].kind == kind && (WIRE_RECORD[w].field == field || kind >= WIRE_INE)) return w;
  return -1;
}
constexpr int WIRE_W_LON = wire_word(WIRE_F64, KID_B_LON), WIRE_W_LAT = wire_word(WIRE_F64, KID_B_LAT);
constexpr int WIRE_W_UVEL = wire_word(WIRE_F64, KID_B_UVEL), WIRE_W_VVEL = wire_word(WIRE_F64, KID_B_VVEL);
constexpr int WIRE_W_INE = wire_word(WIRE_INE, 0), WIRE_W_JNE = wire_word(WIRE_JNE, 0);
constexpr int WIRE_W_HALO_BERG = wire_word(WIRE_F64, KID_B_HALO_BERG), WIRE_W_STATIC_BERG = wire_word(WIRE_F64, KID_B_STATIC_BERG);
constexpr int WIRE_W_ID_HI = wire_word(WIRE_ID_HI, 0), WIRE_W_ID_LO = wire_word(WIRE_ID_LO, 0), WIRE_W_OD = wire_word(WIRE_F64, KID_B_OD);
static_assert(WIRE_W_INE == 23 && WIRE_W_JNE == 24 && WIRE_W_HALO_BERG == 29 && WIRE_W_ID_HI == 31 && WIRE_W_OD == 33, "the layout of FW:3268-3301");

// A non-zero word of these members switches the optional paths of the per-berg kernels on (Flags::has_static, Flags::has_fl;
// kid_upload_bergs applies the same rule to the arrays it is given).
constexpr bool marks_has_static(int f) { return f == KID_B_STATIC_BERG || f == KID_B_HALO_BERG; }
constexpr bool marks_has_fl(int f) { return f == KID_B_MASS_OF_FL_BITS || f == KID_B_MASS_OF_FL_BERGY_BITS || f == KID_B_FL_K; }

// Fields no kernel of the current configuration ever stores to: if such a field was uploaded as zeros it is zeros
// forever and a permutation of the rows need not move it (config 2: 32 of the 52 fp64 fields).  Conservative: anything that
// can append bergs (footloose, calving) or the MTS path writes everything.
struct NeverWrittenIn { bool footloose, mts, calving_on, periodic_reentry, runge_not_verlet, has_fl, env_ever_stored; };
constexpr bool field_never_written(const NeverWrittenIn &s, int f) {
  if (s.footloose || s.mts || s.calving_on) return false;
  switch (f) {
    case KID_B_AXN_FAST: case KID_B_AYN_FAST: case KID_B_BXN_FAST: case KID_B_BYN_FAST: case KID_B_ANG_VEL: case KID_B_ANG_ACCEL: case KID_B_ROT:
    case KID_B_UVEL_OLD: case KID_B_VVEL_OLD: case KID_B_LON_OLD: case KID_B_LAT_OLD:
      return !s.periodic_reentry;   // a berg that re-enters across the seam gets them reset (FW:3573-3577)
    case KID_B_HALO_BERG: case KID_B_STATIC_BERG: case KID_B_START_LON: case KID_B_START_LAT: case KID_B_START_MASS: case KID_B_HEAT_DENSITY:
      return true;
    case KID_B_UVEL_PREV: case KID_B_VVEL_PREV:
      return s.runge_not_verlet;
    case KID_B_MASS_OF_FL_BITS: case KID_B_MASS_OF_FL_BERGY_BITS: case KID_B_FL_K: case KID_B_START_DAY: case KID_B_MASS_SCALING:
      return !s.has_fl;
    case KID_B_UO: case KID_B_VO: case KID_B_UI: case KID_B_VI: case KID_B_UA: case KID_B_VA: case KID_B_SSH_X: case KID_B_SSH_Y:
    case KID_B_SST: case KID_B_SSS: case KID_B_CN: case KID_B_HI: case KID_B_OD:
      return !s.env_ever_stored;
    default:
      return false;
  }
}

// Fields that hold only zeros (== 0.) in every row of [0, n): a plain hot build neither loads nor stores them, a row
// permutation does not move them.  Two sticky words per field, cleared only by an upload that proves zeros:
//   uploaded_nonzero: the field held something else at the last upload, or in a row appended since (a record that carries it,
//                     or rows a kernel wrote: those may hold anything)
//   launched_nonzero: a launch that can write it non-zero has been enqueued since the last upload
// kid_rows.inc calls the row events, kid_launch.inc (and the MTS / interactive / footloose entry points) the launch events;
// tests/zero_fields_host.cpp enumerates the rule and runs scripted sequences of the events.
struct ZeroState {
  bool uploaded_nonzero[KID_NB_F64] = {};
  bool launched_nonzero[KID_NB_F64] = {};
  constexpr void uploaded(int f, bool nonzero) { uploaded_nonzero[f] = nonzero; launched_nonzero[f] = false; }
  constexpr void appended_by_kernel() { for (bool &nz : uploaded_nonzero) nz = true; }
  constexpr void appended_word(int f) { uploaded_nonzero[f] = true; }   // a non-zero word of an immigrant's record
  constexpr void launched_accel() { launched_nonzero[KID_B_AXN] = true; launched_nonzero[KID_B_AYN] = true; }
  // one launch of the per-berg kernel.  Under RK accel ends with axn = ayn = 0 (IB:2286) and the sums of the four stages stay
  // +0; Verlet stores the explicit part there.  The thermodynamics changes mass_of_bits only with bergy_bit_erosion_fraction > 0
  // or when footloose bits take the place of a parent that melted (IB:3289)
  constexpr void launched_berg(bool evolve, bool thermo, bool rk, bool erosion_zero, bool has_fl, bool footloose) {
    if ((evolve && !rk) || footloose) launched_accel();
    if ((thermo && (!erosion_zero || has_fl)) || footloose) launched_nonzero[KID_B_MASS_OF_BITS] = true;
  }
  // the MTS and the interacting evolve and the footloose calving pass: they write any of the three
  constexpr void launched_other() { launched_accel(); launched_nonzero[KID_B_MASS_OF_BITS] = true; }
};
// what a launch (or the plan of a row permutation) knows about field f now.  never_written: field_never_written above
struct KnownZeroIn { bool uploaded_nonzero, launched_nonzero, never_written, rk, erosion_zero; };
constexpr bool field_known_zero(const KnownZeroIn &s, int f) {
  if (s.uploaded_nonzero) return false;
  switch (f) {
    case KID_B_AXN: case KID_B_AYN: return !s.launched_nonzero && s.rk;
    case KID_B_MASS_OF_BITS: return !s.launched_nonzero && s.erosion_zero;
    case KID_B_HEAT_DENSITY: return s.never_written;
    default: return false;
  }
}
// the fields a plain hot build asks about: its mask has one bit per KID_B_* field, and only these are ever set
constexpr unsigned long long KID_ZERO_FIELDS = (1ull << KID_B_AXN) | (1ull << KID_B_AYN) | (1ull << KID_B_MASS_OF_BITS) | (1ull << KID_B_HEAT_DENSITY);
static_assert(KID_B_AXN < 64 && KID_B_AYN < 64 && KID_B_MASS_OF_BITS < 64 && KID_B_HEAT_DENSITY < 64, "one bit per fp64 field");
// the mask of a launch enqueued now.  heat_density_never_written: field_never_written of that field
constexpr unsigned long long known_zero_mask(const ZeroState &z, bool heat_density_never_written, bool rk, bool erosion_zero) {
  unsigned long long m = 0ull;
  for (int f = 0; f < KID_NB_F64; ++f)
    if (((KID_ZERO_FIELDS >> f) & 1ull) &&
        field_known_zero(KnownZeroIn{z.uploaded_nonzero[f], z.launched_nonzero[f], f == KID_B_HEAT_DENSITY && heat_density_never_written, rk, erosion_zero}, f))
      m |= 1ull << f;
  // the two components of one vector: known together or not at all
  constexpr unsigned long long accel = (1ull << KID_B_AXN) | (1ull << KID_B_AYN);
  if ((m & accel) != accel) m &= ~accel;
  return m;
}

// Cold fields: the members no kernel of a step the handle can currently run reads or writes by row.  A row permutation leaves
// them in the array they are in and moves one int32 per row instead, `origin`: field f of row k is cold[f][origin[k]] until a
// reader asks for the rows (kid_rows.inc, cold_materialise).  Only a handle whose step is one plain fused launch defers
// anything (`fusable`: rebin_fusable of kid_rows.inc -- RK4, old interpolation order, no mts / interactions / footloose /
// static_icebergs / find_melt_using_spread_mass, plain namelist): its step is berg_kernel<RK, OLD, PH_STEP> as hot build
// (K = 1 or 3) and as general build (K = 0), the forcing prepass and the gather, and of these only berg_kernel looks at rows.
// step_touches_* follows that kernel (kid_berg_kernel.hpp) load by load and store by store; a member it does not know is touched.
// The guard that decides today is `fusable`: it implies the plain namelist (diag_mask 0, iceberg_bonds_on 0, RK4) and neither
// has_static nor has_fl, so of the conditions below only periodic_reentry can take its other value on a handle that defers
// anything; the rest are what the kernel's own conditions say, kept so that a wider `fusable` cannot make a field cold that the
// step then reads.  tests/cold_rows_host.cpp enumerates the rule (against its statement in words, not against the kernel) and
// the composition of `origin`.
struct ColdIn { bool fusable, runge_not_verlet, periodic_reentry, has_static, has_fl, bonds_on, melt_by_class; };
constexpr bool step_touches_f64(const ColdIn &s, int f) {
  switch (f) {
    case KID_B_START_LON: case KID_B_START_LAT:   // no load, no store
    case KID_B_AXN_FAST: case KID_B_AYN_FAST: case KID_B_BXN_FAST: case KID_B_BYN_FAST: case KID_B_ANG_VEL: case KID_B_ANG_ACCEL: case KID_B_ROT:   // the MTS / DEM kernels only
      return false;
    case KID_B_UVEL_PREV: case KID_B_VVEL_PREV:
      return !s.runge_not_verlet;   // stored by the Verlet evolve
    case KID_B_UVEL_OLD: case KID_B_VVEL_OLD: case KID_B_LON_OLD: case KID_B_LAT_OLD:
      return s.periodic_reentry;    // stored for a berg that re-enters across the seam (general build)
    case KID_B_HALO_BERG: case KID_B_STATIC_BERG:
      return s.has_static;          // loaded at the head of the kernel under Flags::has_static
    case KID_B_MASS_OF_FL_BITS: case KID_B_MASS_OF_FL_BERGY_BITS: case KID_B_FL_K:
    case KID_B_START_DAY:           // stored when a berg turns into a footloose child
      return s.has_fl;
    case KID_B_START_MASS:
      return s.melt_by_class;       // loaded for the melt-by-class diagnostic
    default:
      return true;                  // position, velocity, accelerations, size, mass_scaling, bits, heat density, the environment
  }
}
constexpr bool step_touches_i32(const ColdIn &s, int f) {
  switch (f) {
    case KID_BI_START_YEAR: return s.has_fl;     // stored with start_day
    case KID_BI_N_BONDS: return s.bonds_on;      // loaded under iceberg_bonds_on
    case KID_BI_CONGLOM_ID: return false;
    default: return true;                        // the cell, alive
  }
}
static_assert(KID_NB_I32 <= 32, "one bit per int32 field");
struct ColdSet {
  unsigned long long f64 = 0ull; unsigned i32 = 0u; bool id = false;
  constexpr bool empty() const { return f64 == 0ull && i32 == 0u && !id; }
  constexpr bool within(const ColdSet &o) const { return (f64 & ~o.f64) == 0ull && (i32 & ~o.i32) == 0u && (!id || o.id); }
  constexpr int bytes_per_row() const {
    int b = id ? 8 : 0;
    for (int f = 0; f < KID_NB_F64; ++f) b += ((f64 >> f) & 1ull) ? 8 : 0;
    for (int f = 0; f < KID_NB_I32; ++f) b += ((i32 >> f) & 1u) ? 4 : 0;
    return b;
  }
};
// the id is never looked at by the step
constexpr ColdSet cold_set(const ColdIn &s) {
  ColdSet c;
  if (!s.fusable) return c;
  for (int f = 0; f < KID_NB_F64; ++f) if (!step_touches_f64(s, f)) c.f64 |= 1ull << f;
  for (int f = 0; f < KID_NB_I32; ++f) if (!step_touches_i32(s, f)) c.i32 |= 1u << f;
  c.id = true;
  return c;
}
// `origin` through a permutation (perm[k]: the source row of destination row k): what permute_all_kernel and the re-binning
// instance do to it as one more 4-byte field.  Composing again never looks at cold data.
constexpr void origin_compose(const int32_t *origin_src, const unsigned *perm, long long n, int32_t *origin_dst) {
  for (long long k = 0; k < n; ++k) origin_dst[k] = origin_src[perm[k]];
}

// Bond tables through a row permutation (kid_set_bonds_follow_rows; permute_bonds_kernel of kid_rows.inc).  The tables are
// slot-major, x[s * stride + k], and a list is the slots s < count[k] of its row.  A list moves with its row, in list order.
// What it holds of its partners is an id (kept as it is) and a reference, (row, slot) of the partner's end of the bond; the row
// is a number of the OLD population, so it goes through the inverse permutation.  A partner that the permutation does not keep
// -- a compaction drops it, a re-binning sorts it to the tail that the next count cuts off -- or that is dead leaves no row to
// point at: the reference becomes (-1, -1), which is what kid_upload_bonds leaves for a partner it does not find among the live
// rows; the slot stays in the list with its id, its fields and the list's count.
// The values the tables are born with (mts_ensure): what a slot past a list's end holds, before and after.
constexpr int32_t BOND_FILL_COUNT = 0, BOND_FILL_BROKEN = 0, BOND_FILL_REF = -1;   // (-1: the 0xff bytes of bother_row / bother_slot)
constexpr long long BOND_FILL_ID = 0;
constexpr double BOND_FILL_F64 = 0.;
struct BondRef { int32_t row, slot; };
// o, slot: the reference as the source list holds it.  partner_stays: row o is kept by the permutation and alive; inv_o: its new
// row.  Neither is looked at when o < 0 (the caller need not look them up then)
constexpr BondRef bond_ref_moved(int32_t o, int32_t slot, bool partner_stays, int32_t inv_o) {
  return (o >= 0 && partner_stays) ? BondRef{inv_o, slot} : BondRef{BOND_FILL_REF, BOND_FILL_REF};
}
// the whole of it on the host, for the reference tables of a list (count, row, slot): destination row k < n_dst takes the list
// of source row perm[k]; keep / alive / inv are indexed by source row (inv only where keep).  Strides may differ.
constexpr void bond_refs_compose(const int32_t *count_src, const int32_t *row_src, const int32_t *slot_src, long long stride_src, const unsigned *perm,
                                 long long n_dst, const int32_t *keep, const int32_t *alive, const int32_t *inv, int mb,
                                 int32_t *count_dst, int32_t *row_dst, int32_t *slot_dst, long long stride_dst) {
  for (long long k = 0; k < n_dst; ++k) {
    const long long p = perm[k];
    const int32_t cnt = keep[p] != 0 ? count_src[p] : BOND_FILL_COUNT;   // (a source row that is not kept: the tail a re-binning leaves to be cut off)
    count_dst[k] = cnt;
    for (int s = 0; s < mb; ++s) {
      BondRef r{BOND_FILL_REF, BOND_FILL_REF};
      if (s < cnt) {
        const int32_t o = row_src[s * stride_src + p];
        r = bond_ref_moved(o, slot_src[s * stride_src + p], o >= 0 && keep[o] != 0 && alive[o] != 0, o >= 0 && keep[o] != 0 ? inv[o] : -1);
      }
      row_dst[s * stride_dst + k] = r.row; slot_dst[s * stride_dst + k] = r.slot;
    }
  }
}

}  // namespace kid
