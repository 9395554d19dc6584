// kid_rows_plan.hpp -- what the host decides about berg rows, as plain C++17: no HIP header, no handle.  The wire record of a
// berg (kid_migrate.inc packs and decodes it, kid_halo_bergs.inc packs it) and the skip rule of the row permutation
// (kid_rows.inc) are written down here once; tests/rows_plan_host.cpp enumerates both on the host.
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

}  // namespace kid
