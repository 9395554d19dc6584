// Host-side check of the rule that takes bond tables through a row permutation (icebergs_amd/csrc/kid_rows_plan.hpp:
// bond_ref_moved, the BOND_FILL_* values, bond_refs_compose; the kernel that calls it is permute_bonds_kernel of kid_rows.inc).
//   * the rule itself over the four kinds of partner: none (-1), kept and alive, kept but dead, not kept;
//   * whole populations (rings with lists from empty to full, max_bonds 1, 4 and 6, strides that are not the row count) through
//     the identity, a reversal, a shuffle and a compaction, checked BY ID: after the permutation every reference that is left
//     points at the row that holds the partner's id, and at the slot of that row's list that names this berg;
//   * one table of eight rows with hand-written expected values, against a plain double loop over (row, slot).
// No HIP, no GPU; built with -fsanitize=address,undefined by tests/test_bond_rows_cpu.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "../icebergs_amd/csrc/kid_rows_plan.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                              \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d %s -- ", __FILE__, __LINE__, #cond);  \
      std::printf(__VA_ARGS__);                                       \
      std::printf("\n");                                              \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static_assert(kid::BOND_FILL_COUNT == 0 && kid::BOND_FILL_BROKEN == 0 && kid::BOND_FILL_ID == 0 && kid::BOND_FILL_F64 == 0. && kid::BOND_FILL_REF == -1,
              "what mts_ensure fills the tables with: zeros, and 0xff bytes for the partner rows and slots");
static_assert(kid::bond_ref_moved(3, 1, true, 7).row == 7 && kid::bond_ref_moved(3, 1, true, 7).slot == 1, "constexpr");

static void check_rule() {
  for (int slot = -1; slot < 6; ++slot)
    for (int inv = -1; inv < 9; ++inv)
      for (int stays = 0; stays < 2; ++stays) {
        // no partner row known: nothing is looked at, nothing appears
        const kid::BondRef none = kid::bond_ref_moved(-1, slot, stays != 0, inv);
        CHECK(none.row == -1 && none.slot == -1, "partner -1, slot %d inv %d stays %d: (%d, %d)", slot, inv, stays, none.row, none.slot);
        for (int o : {0, 1, 5, 1 << 20}) {
          const kid::BondRef r = kid::bond_ref_moved(o, slot, stays != 0, inv);
          if (stays) CHECK(r.row == inv && r.slot == slot, "partner %d kept and alive: (%d, %d), expected (%d, %d)", o, r.row, r.slot, inv, slot);
          else CHECK(r.row == -1 && r.slot == -1, "partner %d dead or not kept: (%d, %d), the slot must lose its row AND its slot", o, r.row, r.slot);
        }
      }
}

// a population of n rows, row k with id 100 + k, bonded in a ring to its next `reach` neighbours on either side as far as
// `len[k]` slots go: mutual bonds only (a bond is entered at both ends or not at all)
struct Tables {
  int mb; long long n, stride;
  std::vector<int32_t> count, row, slot;
  std::vector<long long> id, other;
  Tables(int mb_, long long n_, long long stride_) : mb(mb_), n(n_), stride(stride_), count((size_t)stride_, -77), row((size_t)(mb_ * stride_), -77),
                                                     slot((size_t)(mb_ * stride_), -77), id((size_t)stride_, -77), other((size_t)(mb_ * stride_), -77) {}
  size_t at(int s, long long k) const { return (size_t)(s * stride + k); }
};
static Tables ring(int mb, long long n, long long stride, int want) {   // want: bonds per berg asked for (0: none; mb: full lists where n allows)
  Tables t(mb, n, stride);
  for (long long k = 0; k < n; ++k) { t.id[(size_t)k] = 100 + k; t.count[(size_t)k] = 0; }
  for (long long k = 0; k < n; ++k)
    for (long long d = 1; d <= n / 2; ++d) {
      const long long o = (k + d) % n;
      if (o == k || t.count[(size_t)k] >= want || t.count[(size_t)o] >= want) continue;
      bool dup = false;
      for (int s = 0; s < t.count[(size_t)k]; ++s) dup = dup || t.row[t.at(s, k)] == (int32_t)o;
      if (dup) continue;
      const int sk = t.count[(size_t)k]++, so = t.count[(size_t)o]++;
      t.row[t.at(sk, k)] = (int32_t)o; t.slot[t.at(sk, k)] = so; t.other[t.at(sk, k)] = t.id[(size_t)o];
      t.row[t.at(so, o)] = (int32_t)k; t.slot[t.at(so, o)] = sk; t.other[t.at(so, o)] = t.id[(size_t)k];
    }
  return t;
}
// through perm (destination k < n_dst takes source perm[k]); keep / alive by source row.  Checked by id.
static void through(const Tables &src, const std::vector<unsigned> &perm, const std::vector<int32_t> &keep, const std::vector<int32_t> &alive, long long stride_dst, const char *what) {
  const long long n_dst = (long long)perm.size();
  std::vector<int32_t> inv((size_t)src.n, -5);
  for (long long k = 0; k < n_dst; ++k) inv[perm[(size_t)k]] = (int32_t)k;
  Tables dst(src.mb, n_dst, stride_dst);
  for (long long k = 0; k < n_dst; ++k) {   // what permute_all_kernel / permute_bonds_kernel do to the id and to other_id
    dst.id[(size_t)k] = src.id[perm[(size_t)k]];
    for (int s = 0; s < src.mb; ++s) dst.other[dst.at(s, k)] = s < src.count[perm[(size_t)k]] ? src.other[src.at(s, perm[(size_t)k])] : kid::BOND_FILL_ID;
  }
  kid::bond_refs_compose(src.count.data(), src.row.data(), src.slot.data(), src.stride, perm.data(), n_dst, keep.data(), alive.data(), inv.data(), src.mb,
                         dst.count.data(), dst.row.data(), dst.slot.data(), dst.stride);
  for (long long k = 0; k < n_dst; ++k) {
    const long long p = perm[(size_t)k];
    const int32_t cnt = keep[(size_t)p] ? src.count[(size_t)p] : 0;   // a row that is not kept sits in the tail that is cut off: no list
    CHECK(dst.count[(size_t)k] == cnt, "%s: row %lld count", what, k);
    for (int s = 0; s < src.mb; ++s) {
      const int32_t r = dst.row[dst.at(s, k)], q = dst.slot[dst.at(s, k)];
      if (s >= cnt) { CHECK(r == -1 && q == -1, "%s: row %lld slot %d past the list's end holds (%d, %d)", what, k, s, r, q); continue; }
      const int32_t o = src.row[src.at(s, p)];
      const bool stays = o >= 0 && keep[(size_t)o] && alive[(size_t)o];
      if (!stays) { CHECK(r == -1 && q == -1, "%s: row %lld slot %d names a partner that is gone, and holds (%d, %d)", what, k, s, r, q); continue; }
      CHECK(r >= 0 && r < n_dst, "%s: row %lld slot %d points at row %d of %lld", what, k, s, r, n_dst);
      if (r < 0 || r >= n_dst) continue;
      CHECK(dst.id[(size_t)r] == dst.other[dst.at(s, k)], "%s: row %lld slot %d: the row it points at holds another id", what, k, s);
      CHECK(q >= 0 && q < dst.count[(size_t)r] && dst.other[dst.at(q, r)] == dst.id[(size_t)k], "%s: row %lld slot %d: the partner's slot %d does not name it back", what, k, s, q);
    }
  }
}
static void check_populations() {
  unsigned long long seed = 88172645463325252ull;
  auto rnd = [&]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
  for (int mb : {1, 4, 6})
    for (long long n : {1ll, 2ll, 8ll, 65ll, 257ll})
      for (int want : {0, 1, mb}) {   // empty lists, one bond, full lists
        const Tables t = ring(mb, n, n + 37, want);
        if (want == mb && n > mb) CHECK(*std::max_element(t.count.begin(), t.count.begin() + n) == mb, "mb %d n %lld: no list is full", mb, n);
        if (want == 0) for (long long k = 0; k < n; ++k) CHECK(t.count[(size_t)k] == 0, "empty lists");
        std::vector<int32_t> all((size_t)n, 1);
        std::vector<unsigned> perm((size_t)n);
        std::iota(perm.begin(), perm.end(), 0u);
        through(t, perm, all, all, n + 37, "identity");
        std::reverse(perm.begin(), perm.end());
        through(t, perm, all, all, n + 5, "reversal");
        for (long long k = n - 1; k > 0; --k) std::swap(perm[(size_t)k], perm[(size_t)(rnd() % (unsigned long long)(k + 1))]);
        through(t, perm, all, all, n, "shuffle");
        // a re-binning with dead rows: they are kept out (sorted to the tail that is cut off) though they are destinations
        std::vector<int32_t> alive((size_t)n, 1);
        for (long long k = 0; k < n; k += 7) alive[(size_t)k] = 0;
        through(t, perm, alive, alive, n + 37, "shuffle with dead rows");
        // a compaction: the live rows, in order
        std::vector<unsigned> live;
        for (long long k = 0; k < n; ++k) if (alive[(size_t)k]) live.push_back((unsigned)k);
        through(t, live, alive, alive, n + 37, "compaction");
        // everything dead: no destination row at all
        std::fill(alive.begin(), alive.end(), 0);
        through(t, std::vector<unsigned>(), alive, alive, n + 37, "compaction of the dead");
      }
}

// eight rows, two slots, source stride 11, destination stride 9.  Rows 2 and 5 are dead and dropped, row 6 is dead but kept (a
// row that waits to be packed), row 7 was uploaded with a second partner nobody held.  Slots past the ends hold rubbish.
static void check_table() {
  const int mb = 2; const long long S = 11, D = 9;
  const int32_t X = 40;   // rubbish past a list's end
  const int32_t count[8] = {1, 2, 2, 2, 1, 0, 1, 2};
  const int32_t row0[8] = {1, 0, 1, 2, 3, X, 7, 6}, slot0[8] = {0, 0, 1, 1, 1, X, 0, 0};
  const int32_t row1[8] = {X, 2, 3, 4, X, X, X, -1}, slot1[8] = {X, 0, 0, 0, X, X, X, -1};
  const int32_t keep[8] = {1, 1, 0, 1, 1, 0, 1, 1}, alive[8] = {1, 1, 0, 1, 1, 0, 0, 1};
  const unsigned perm[6] = {0, 1, 3, 4, 6, 7};
  const int32_t inv[8] = {0, 1, -9, 2, 3, -9, 4, 5};
  // by hand: row 1 loses its partner 2, row 3 (now 2) loses its partner 2 and keeps 4 (now 3), row 7 (now 5) loses the dead row 6
  const int32_t want_count[6] = {1, 2, 2, 1, 1, 2};
  const int32_t want_row0[6] = {1, 0, -1, 2, 5, -1}, want_slot0[6] = {0, 0, -1, 1, 0, -1};
  const int32_t want_row1[6] = {-1, -1, 3, -1, -1, -1}, want_slot1[6] = {-1, -1, 0, -1, -1, -1};
  std::vector<int32_t> srow((size_t)(mb * S), X), sslot((size_t)(mb * S), X), scount((size_t)S, X);
  for (int k = 0; k < 8; ++k) { scount[(size_t)k] = count[k]; srow[(size_t)k] = row0[k]; sslot[(size_t)k] = slot0[k]; srow[(size_t)(S + k)] = row1[k]; sslot[(size_t)(S + k)] = slot1[k]; }
  // the plain double loop over (destination row, slot), with the rule
  std::vector<int32_t> lrow((size_t)(mb * D), X), lslot((size_t)(mb * D), X);
  for (int k = 0; k < 6; ++k)
    for (int s = 0; s < mb; ++s) {
      const unsigned p = perm[k];
      kid::BondRef r{kid::BOND_FILL_REF, kid::BOND_FILL_REF};
      if (s < count[p]) {
        const int32_t o = srow[(size_t)(s * S + p)];
        r = kid::bond_ref_moved(o, sslot[(size_t)(s * S + p)], o >= 0 && keep[o] && alive[o], o >= 0 ? inv[o] : -1);
      }
      lrow[(size_t)(s * D + k)] = r.row; lslot[(size_t)(s * D + k)] = r.slot;
    }
  std::vector<int32_t> drow((size_t)(mb * D), X), dslot((size_t)(mb * D), X), dcount((size_t)D, X);
  kid::bond_refs_compose(scount.data(), srow.data(), sslot.data(), S, perm, 6, keep, alive, inv, mb, dcount.data(), drow.data(), dslot.data(), D);
  for (int k = 0; k < 6; ++k) {
    CHECK(dcount[(size_t)k] == want_count[k], "row %d: count %d", k, dcount[(size_t)k]);
    for (int s = 0; s < mb; ++s) {
      const int32_t wr = s ? want_row1[k] : want_row0[k], ws = s ? want_slot1[k] : want_slot0[k];
      CHECK(lrow[(size_t)(s * D + k)] == wr && lslot[(size_t)(s * D + k)] == ws, "double loop, row %d slot %d: (%d, %d), by hand (%d, %d)", k, s, lrow[(size_t)(s * D + k)], lslot[(size_t)(s * D + k)], wr, ws);
      CHECK(drow[(size_t)(s * D + k)] == wr && dslot[(size_t)(s * D + k)] == ws, "bond_refs_compose, row %d slot %d: (%d, %d), by hand (%d, %d)", k, s, drow[(size_t)(s * D + k)], dslot[(size_t)(s * D + k)], wr, ws);
    }
  }
  // nothing was written beyond the destination rows
  for (long long k = 6; k < D; ++k) CHECK(dcount[(size_t)k] == X && drow[(size_t)k] == X && drow[(size_t)(D + k)] == X && dslot[(size_t)k] == X, "row %lld was written", k);
}

int main() {
  check_rule();
  check_populations();
  check_table();
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
