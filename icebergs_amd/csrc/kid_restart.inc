// kid_restart.inc -- restart files straight from the structure of arrays (SURVEY.md 8f N2):
//   icebergs.res.nc   write_restart_bergs /root/reference/src/icebergs_fms2io.F90:124-420, read_restart_bergs IO2:663-1049
//   bonds_iceberg.res.nc  IO2:466-583 (write), read_restart_bonds IO2:1190-1481
//   calving.res.nc    IO2:583-631 (write), read_restart_calving IO2:1483ff
// The reference goes through FMS fms2_io and libnetcdf, neither of which exists here; the files are netCDF classic
// (CDF-2, 64-bit offset), whose published layout is short enough to write and read directly: header = magic, numrecs,
// dimension / attribute / variable lists; fixed-size variables at their `begin`, record variables interleaved record by
// record.  Variable names, order, types, dimensions ("i" unlimited) and the long_name / units attributes follow the
// reference's register_restart_field_wrap calls.  Files of the netCDF-4 (HDF5) flavour are refused with a message
// (convert with `nccopy -k cdf2`).
namespace ncfile {
enum { NC_BYTE = 1, NC_CHAR = 2, NC_SHORT = 3, NC_INT = 4, NC_FLOAT = 5, NC_DOUBLE = 6, TAG_DIM = 10, TAG_VAR = 11, TAG_ATT = 12 };
struct Att { std::string name; int type; std::vector<char> raw; long long n; };   // raw: big-endian values
struct Var {
  std::string name; std::vector<int> dims; std::vector<Att> atts; int type; bool record = false;
  long long vsize = 0, begin = 0; std::vector<char> data;   // data: big-endian, whole variable (all records)
};
struct File { std::vector<std::pair<std::string, long long>> dims; int unlimited = -1; long long numrecs = 0; std::vector<Att> gatts; std::vector<Var> vars; };
static inline int tsize(int t) { return t == NC_DOUBLE ? 8 : (t == NC_INT || t == NC_FLOAT) ? 4 : t == NC_SHORT ? 2 : 1; }
static inline long long pad4(long long n) { return (n + 3) & ~3ll; }
template <class T> static void put_be(std::vector<char> &o, T v) {
  char b[sizeof(T)]; std::memcpy(b, &v, sizeof(T));
  for (size_t k = 0; k < sizeof(T); ++k) o.push_back(b[sizeof(T) - 1 - k]);
}
static void put_i32(std::vector<char> &o, long long v) { put_be<int32_t>(o, (int32_t)v); }
static void put_name(std::vector<char> &o, const std::string &s) { put_i32(o, (long long)s.size()); o.insert(o.end(), s.begin(), s.end()); while (o.size() & 3) o.push_back(0); }
static Att att_text(const std::string &name, const std::string &text) { Att a{name, NC_CHAR, {}, (long long)text.size()}; a.raw.assign(text.begin(), text.end()); return a; }
static Att att_int(const std::string &name, int v) { Att a{name, NC_INT, {}, 1}; put_be<int32_t>(a.raw, v); return a; }
static void put_atts(std::vector<char> &o, const std::vector<Att> &atts) {
  if (atts.empty()) { put_i32(o, 0); put_i32(o, 0); return; }
  put_i32(o, TAG_ATT); put_i32(o, (long long)atts.size());
  for (const Att &a : atts) { put_name(o, a.name); put_i32(o, a.type); put_i32(o, a.n); o.insert(o.end(), a.raw.begin(), a.raw.end()); while (o.size() & 3) o.push_back(0); }
}
template <class T> static void set_data(Var &v, const T *src, long long n) { v.data.clear(); v.data.reserve((size_t)n * sizeof(T)); for (long long k = 0; k < n; ++k) put_be<T>(v.data, src[k]); }

static int write(const File &f, const char *path) {
  // sizes first: the header length fixes every `begin`
  std::vector<Var> vars = f.vars;
  long long recsize = 0;
  for (Var &v : vars) {
    long long cnt = 1;
    for (size_t d = 0; d < v.dims.size(); ++d) if (!(v.record && d == 0)) cnt *= f.dims[v.dims[d]].second;
    v.vsize = pad4(cnt * tsize(v.type));
    if (v.record) recsize += v.vsize;
  }
  auto header = [&](std::vector<char> &o) {
    o.clear(); o.push_back('C'); o.push_back('D'); o.push_back('F'); o.push_back(2);
    put_i32(o, f.numrecs);
    if (f.dims.empty()) { put_i32(o, 0); put_i32(o, 0); }
    else { put_i32(o, TAG_DIM); put_i32(o, (long long)f.dims.size()); for (size_t d = 0; d < f.dims.size(); ++d) { put_name(o, f.dims[d].first); put_i32(o, (int)d == f.unlimited ? 0 : f.dims[d].second); } }
    put_atts(o, f.gatts);
    if (vars.empty()) { put_i32(o, 0); put_i32(o, 0); }
    else {
      put_i32(o, TAG_VAR); put_i32(o, (long long)vars.size());
      for (const Var &v : vars) {
        put_name(o, v.name); put_i32(o, (long long)v.dims.size()); for (int d : v.dims) put_i32(o, d);
        put_atts(o, v.atts); put_i32(o, v.type); put_i32(o, v.vsize > 0x7fffffffll ? -1 : v.vsize); put_be<int64_t>(o, (int64_t)v.begin);
      }
    }
  };
  std::vector<char> hdr; header(hdr);
  long long off = (long long)hdr.size();
  for (Var &v : vars) if (!v.record) { v.begin = off; off += v.vsize; }
  const long long rec0 = off;
  for (Var &v : vars) if (v.record) { v.begin = off; off += v.vsize; }
  header(hdr);
  FILE *fp = std::fopen(path, "wb");
  if (!fp) return -1;
  bool ok = std::fwrite(hdr.data(), 1, hdr.size(), fp) == hdr.size();
  for (const Var &v : vars) if (!v.record) {
    std::vector<char> b(v.data); b.resize((size_t)v.vsize, 0);
    ok = ok && std::fwrite(b.data(), 1, b.size(), fp) == b.size();
  }
  if (recsize > 0 && f.numrecs > 0) {
    std::vector<char> rec((size_t)(recsize * f.numrecs), 0);
    long long voff = 0;
    for (const Var &v : vars) if (v.record) {
      const long long per = v.vsize;
      for (long long r = 0; r < f.numrecs; ++r) {
        const long long have = std::min<long long>(per, (long long)v.data.size() - r * per);
        if (have > 0) std::memcpy(rec.data() + r * recsize + voff, v.data.data() + r * per, (size_t)have);
      }
      voff += per;
    }
    ok = ok && std::fwrite(rec.data(), 1, rec.size(), fp) == rec.size();
    (void)rec0;
  }
  ok = (std::fclose(fp) == 0) && ok;
  return ok ? 0 : -1;
}

struct Reader {
  std::vector<char> buf; size_t pos = 0; int version = 0; std::string err;
  bool need(size_t n) { if (pos + n > buf.size()) { err = "truncated netCDF header"; return false; } return true; }
  long long i32() { if (!need(4)) return 0; uint32_t v = 0; for (int k = 0; k < 4; ++k) v = (v << 8) | (unsigned char)buf[pos + k]; pos += 4; return (int32_t)v; }
  long long i64() { if (!need(8)) return 0; uint64_t v = 0; for (int k = 0; k < 8; ++k) v = (v << 8) | (unsigned char)buf[pos + k]; pos += 8; return (long long)v; }
  std::string name() { const long long n = i32(); if (n < 0 || !need((size_t)pad4(n))) return ""; std::string s(buf.data() + pos, (size_t)n); pos += (size_t)pad4(n); return s; }
  bool atts(std::vector<Att> &out) {
    const long long tag = i32(), n = i32();
    if (tag == 0 && n == 0) return true;
    if (tag != TAG_ATT) { err = "bad attribute list"; return false; }
    for (long long k = 0; k < n; ++k) {
      Att a; a.name = name(); a.type = (int)i32(); a.n = i32();
      const long long bytes = pad4(a.n * tsize(a.type));
      if (!need((size_t)bytes)) return false;
      a.raw.assign(buf.data() + pos, buf.data() + pos + a.n * tsize(a.type)); pos += (size_t)bytes;
      out.push_back(a);
    }
    return err.empty();
  }
};
// header + data of a classic file; values stay big-endian in Var::data (as_double / as_int convert)
static int read(const char *path, File &f, std::string &err) {
  FILE *fp = std::fopen(path, "rb");
  if (!fp) { err = std::string("cannot open ") + path; return -1; }
  Reader r;
  std::fseek(fp, 0, SEEK_END); const long sz = std::ftell(fp); std::fseek(fp, 0, SEEK_SET);
  r.buf.resize((size_t)sz);
  const bool got = std::fread(r.buf.data(), 1, (size_t)sz, fp) == (size_t)sz; std::fclose(fp);
  if (!got || sz < 8) { err = "short read"; return -1; }
  if (r.buf[0] == (char)0x89 && r.buf[1] == 'H' && r.buf[2] == 'D' && r.buf[3] == 'F') { err = "netCDF-4 / HDF5 file: convert it with `nccopy -k cdf2`"; return -1; }
  if (r.buf[0] != 'C' || r.buf[1] != 'D' || r.buf[2] != 'F' || (r.buf[3] != 1 && r.buf[3] != 2)) { err = "not a netCDF classic (CDF-1/2) file"; return -1; }
  r.version = r.buf[3]; r.pos = 4;
  f.numrecs = r.i32();
  { const long long tag = r.i32(), n = r.i32();
    if (tag == TAG_DIM) for (long long k = 0; k < n; ++k) { std::string nm = r.name(); const long long len = r.i32(); if (len == 0) f.unlimited = (int)k; f.dims.emplace_back(nm, len == 0 ? f.numrecs : len); }
    else if (!(tag == 0 && n == 0)) { err = "bad dimension list"; return -1; } }
  if (!r.atts(f.gatts)) { err = r.err; return -1; }
  long long recsize = 0;
  { const long long tag = r.i32(), n = r.i32();
    if (tag == TAG_VAR) for (long long k = 0; k < n; ++k) {
      Var v; v.name = r.name(); const long long nd = r.i32();
      for (long long d = 0; d < nd; ++d) v.dims.push_back((int)r.i32());
      if (!r.atts(v.atts)) { err = r.err; return -1; }
      v.type = (int)r.i32(); v.vsize = r.i32(); v.begin = r.version == 2 ? r.i64() : r.i32();
      v.record = !v.dims.empty() && v.dims[0] == f.unlimited;
      long long cnt = 1; for (size_t d = 0; d < v.dims.size(); ++d) if (!(v.record && d == 0)) { if (v.dims[d] < 0 || v.dims[d] >= (int)f.dims.size()) { err = "bad dimension id"; return -1; } cnt *= f.dims[v.dims[d]].second; }
      v.vsize = pad4(cnt * tsize(v.type));   // recomputed: the stored value saturates for huge variables
      if (v.record) recsize += v.vsize;
      f.vars.push_back(v);
    } else if (!(tag == 0 && n == 0)) { err = "bad variable list"; return -1; } }
  if (!r.err.empty()) { err = r.err; return -1; }
  int nrecvars = 0; for (const Var &v : f.vars) nrecvars += v.record ? 1 : 0;
  for (Var &v : f.vars) {
    long long cnt = 1; for (size_t d = 0; d < v.dims.size(); ++d) if (!(v.record && d == 0)) cnt *= f.dims[v.dims[d]].second;
    const long long per = cnt * tsize(v.type);
    if (!v.record) {
      if (v.begin < 0 || (size_t)(v.begin + per) > r.buf.size()) { err = "variable " + v.name + " runs past the end of the file"; return -1; }
      v.data.assign(r.buf.data() + v.begin, r.buf.data() + v.begin + per);
    } else {
      // a single record variable is stored without padding between its records (the format's one special case)
      const long long stride = nrecvars == 1 ? per : recsize;
      v.data.resize((size_t)(per * f.numrecs));
      for (long long q = 0; q < f.numrecs; ++q) {
        const long long at = v.begin + q * stride;
        if (at < 0 || (size_t)(at + per) > r.buf.size()) { err = "record variable " + v.name + " runs past the end of the file"; return -1; }
        std::memcpy(v.data.data() + q * per, r.buf.data() + at, (size_t)per);
      }
    }
  }
  return 0;
}
static const Var *find(const File &f, const std::string &name) { for (const Var &v : f.vars) if (v.name == name) return &v; return nullptr; }
static long long count(const File &f, const Var &v) { long long c = 1; for (int d : v.dims) c *= f.dims[d].second; return c; }
static double value(const Var &v, long long k) {
  const char *p = v.data.data() + k * tsize(v.type);
  unsigned char b[8]; const int ts = tsize(v.type);
  for (int q = 0; q < ts; ++q) b[q] = (unsigned char)p[ts - 1 - q];
  if (v.type == NC_DOUBLE) { double d; std::memcpy(&d, b, 8); return d; }
  if (v.type == NC_FLOAT) { float d; std::memcpy(&d, b, 4); return d; }
  if (v.type == NC_INT) { int32_t d; std::memcpy(&d, b, 4); return d; }
  if (v.type == NC_SHORT) { int16_t d; std::memcpy(&d, b, 2); return d; }
  return (signed char)b[0];
}
}  // namespace ncfile

namespace {
struct RestartField { const char *name; int field; const char *longname, *units; int when; };  // when: 0 always, 1 Verlet, 2 footloose, 3 mts, 4 dem
// order, names and attributes of IO2:316-407 (ine, jne, start_year, id_cnt, id_ij are integers and handled apart)
static const RestartField kRestartF64[] = {
  {"lon", KID_B_LON, "longitude", "degrees_E", 0}, {"lat", KID_B_LAT, "latitude", "degrees_N", 0},
  {"uvel", KID_B_UVEL, "zonal velocity", "m/s", 0}, {"vvel", KID_B_VVEL, "meridional velocity", "m/s", 0},
  {"mass", KID_B_MASS, "mass", "kg", 0},
  {"axn", KID_B_AXN, "explicit zonal acceleration", "m/s^2", 1}, {"ayn", KID_B_AYN, "explicit meridional acceleration", "m/s^2", 1},
  {"bxn", KID_B_BXN, "implicit zonal acceleration", "m/s^2", 1}, {"byn", KID_B_BYN, "implicit meridional acceleration", "m/s^2", 1},
  {"ine", -1, "i index", "none", 0}, {"jne", -2, "j index", "none", 0},
  {"thickness", KID_B_THICKNESS, "thickness", "m", 0}, {"width", KID_B_WIDTH, "width", "m", 0}, {"length", KID_B_LENGTH, "length", "m", 0},
  {"start_lon", KID_B_START_LON, "longitude of calving location", "degrees_E", 0}, {"start_lat", KID_B_START_LAT, "latitude of calving location", "degrees_N", 0},
  {"start_year", -3, "calendar year of calving event", "years", 0},
  {"id_cnt", -4, "counter component of iceberg id", "dimensionless", 0}, {"id_ij", -5, "position component of iceberg id", "dimensionless", 0},
  {"start_day", KID_B_START_DAY, "year day of calving event", "days", 0}, {"start_mass", KID_B_START_MASS, "initial mass of calving berg", "kg", 0},
  {"mass_scaling", KID_B_MASS_SCALING, "scaling factor for mass of calving berg", "none", 0},
  {"mass_of_bits", KID_B_MASS_OF_BITS, "mass of bergy bits", "kg", 0}, {"heat_density", KID_B_HEAT_DENSITY, "heat density", "J/kg", 0},
  {"fl_k", KID_B_FL_K, "footloose calving k", "m", 2}, {"mass_of_fl_bits", KID_B_MASS_OF_FL_BITS, "mass of footloose bits", "kg", 2},
  {"mass_of_fl_bergy_bits", KID_B_MASS_OF_FL_BERGY_BITS, "mass of bergy bits associated with footloose bits", "kg", 2},
  {"axn_fast", KID_B_AXN_FAST, "sub-step explicit zonal acceleration", "m/s^2", 3}, {"ayn_fast", KID_B_AYN_FAST, "sub-step explicit meridional acceleration", "m/s^2", 3},
  {"bxn_fast", KID_B_BXN_FAST, "sub-step implicit zonal acceleration", "m/s^2", 3}, {"byn_fast", KID_B_BYN_FAST, "sub-step implicit meridional acceleration", "m/s^2", 3},
  {"ang_vel", KID_B_ANG_VEL, "dem angular velocity", "rad/s", 4}, {"ang_accel", KID_B_ANG_ACCEL, "dem angular acceleration", "rad/s^2", 4},
  {"rot", KID_B_ROT, "dem accumulated rotation", "rad", 4},
};
static bool restart_wanted(const kid_params &p, int when) {
  return when == 0 || (when == 1 && !p.Runge_not_Verlet) || (when == 2 && p.footloose) || (when == 3 && p.mts) || (when == 4 && p.dem);
}
}  // namespace

extern "C" {

// icebergs.res.nc from a host SoA: the bergs of `host` that are alive (halo copies excluded, IO2:191); no device involved
int kid_restart_write_bergs(const char *path, const kid_params *p, const kid_berg_soa *host) {
  if (!path || !p || !host || host->n < 0) return KID_EINVAL;
  for (int f : {KID_B_LON, KID_B_LAT, KID_B_MASS}) if (!host->f64[f]) return KID_EINVAL;
  if (!host->i32[KID_BI_INE] || !host->i32[KID_BI_JNE] || !host->id) return KID_EINVAL;
  std::vector<long long> rows;
  for (long long k = 0; k < host->n; ++k) {
    if (host->i32[KID_BI_ALIVE] && !host->i32[KID_BI_ALIVE][k]) continue;
    if (host->f64[KID_B_HALO_BERG] && host->f64[KID_B_HALO_BERG][k] >= 0.5) continue;
    rows.push_back(k);
  }
  const long long n = (long long)rows.size();
  ncfile::File f;
  f.dims.emplace_back("i", n); f.unlimited = 0; f.numrecs = n;
  f.gatts = {ncfile::att_int("file_format_major_version", 0), ncfile::att_int("file_format_minor_version", 1), ncfile::att_int("time_axis", 0)};  // IO2:65-66, 310-312
  auto add = [&](const char *name, int type, const char *longname, const char *units) -> ncfile::Var & {
    ncfile::Var v; v.name = name; v.dims = {0}; v.type = type; v.record = true;
    v.atts = {ncfile::att_text("long_name", longname), ncfile::att_text("units", units)};
    f.vars.push_back(v); return f.vars.back();
  };
  std::vector<double> col((size_t)std::max<long long>(n, 1));
  std::vector<int32_t> icol((size_t)std::max<long long>(n, 1));
  double n_static = 0.;
  for (const RestartField &rf : kRestartF64) {
    if (!restart_wanted(*p, rf.when)) continue;
    if (rf.field >= 0) {
      for (long long q = 0; q < n; ++q) col[(size_t)q] = host->f64[rf.field] ? host->f64[rf.field][rows[(size_t)q]] : 0.;
      ncfile::set_data(add(rf.name, ncfile::NC_DOUBLE, rf.longname, rf.units), col.data(), n);
    } else {
      for (long long q = 0; q < n; ++q) {
        const long long k = rows[(size_t)q];
        int32_t v = 0;
        if (rf.field == -1) v = host->i32[KID_BI_INE][k];
        else if (rf.field == -2) v = host->i32[KID_BI_JNE][k];
        else if (rf.field == -3) v = host->i32[KID_BI_START_YEAR] ? host->i32[KID_BI_START_YEAR][k] : 0;
        else if (rf.field == -4) v = (int32_t)(host->id[k] >> 32);                  // split_id FW:7285-7296
        else v = (int32_t)(host->id[k] & 0xffffffffll);
        icol[(size_t)q] = v;
      }
      ncfile::set_data(add(rf.name, ncfile::NC_INT, rf.longname, rf.units), icol.data(), n);
    }
  }
  if (host->f64[KID_B_STATIC_BERG]) for (long long q = 0; q < n; ++q) n_static += host->f64[KID_B_STATIC_BERG][rows[(size_t)q]];
  if (n_static > 0.) {  // IO2:387-399
    for (long long q = 0; q < n; ++q) col[(size_t)q] = host->f64[KID_B_STATIC_BERG][rows[(size_t)q]];
    ncfile::set_data(add("static_berg", ncfile::NC_DOUBLE, "static_berg", "dimensionless"), col.data(), n);
  }
  { ncfile::Var v; v.name = "i"; v.dims = {0}; v.type = ncfile::NC_INT; v.record = true;   // IO2:401-405
    for (long long q = 0; q < n; ++q) icol[(size_t)q] = (int32_t)(q + 1);
    ncfile::set_data(v, icol.data(), n); f.vars.push_back(v); }
  return ncfile::write(f, path) == 0 ? KID_OK : KID_EINVAL;
}

int kid_restart_count_bergs(const char *path, int64_t *n) {
  if (!path || !n) return KID_EINVAL;
  ncfile::File f; std::string err;
  if (ncfile::read(path, f, err)) return KID_EINVAL;
  const ncfile::Var *lon = ncfile::find(f, "lon");
  if (!lon) return KID_EINVAL;
  *n = ncfile::count(f, *lon);
  return KID_OK;
}

// icebergs.res.nc into a host SoA with room for `capacity` rows: every berg of the file, the fields the file does not
// hold zero, uvel_old / lon_old = current values and halo_berg = 0 as read_restart_bergs sets them (IO2:895-925);
// xi, yj are left to kid_read_restart (they need the grid)
int kid_restart_read_bergs(const char *path, kid_berg_soa *host, int64_t capacity) {
  if (!path || !host) return KID_EINVAL;
  ncfile::File f; std::string err;
  if (ncfile::read(path, f, err)) return KID_EINVAL;
  const ncfile::Var *lon = ncfile::find(f, "lon");
  if (!lon) return KID_EINVAL;
  const long long n = ncfile::count(f, *lon);
  if (n > capacity) return KID_ECAPACITY;
  for (int q = 0; q < KID_NB_F64; ++q) if (host->f64[q]) for (long long k = 0; k < n; ++k) host->f64[q][k] = 0.;
  for (int q = 0; q < KID_NB_I32; ++q) if (host->i32[q]) for (long long k = 0; k < n; ++k) host->i32[q][k] = (q == KID_BI_ALIVE) ? 1 : 0;
  std::vector<int32_t> cnt((size_t)std::max<long long>(n, 1), 0), ij((size_t)std::max<long long>(n, 1), 0);
  bool have_id = false;
  for (const RestartField &rf : kRestartF64) {
    const ncfile::Var *v = ncfile::find(f, rf.name);
    if (!v || ncfile::count(f, *v) != n) continue;
    for (long long k = 0; k < n; ++k) {
      const double x = ncfile::value(*v, k);
      if (rf.field >= 0) { if (host->f64[rf.field]) host->f64[rf.field][k] = x; }
      else if (rf.field == -1) host->i32[KID_BI_INE][k] = (int32_t)x;
      else if (rf.field == -2) host->i32[KID_BI_JNE][k] = (int32_t)x;
      else if (rf.field == -3) { if (host->i32[KID_BI_START_YEAR]) host->i32[KID_BI_START_YEAR][k] = (int32_t)x; }
      else if (rf.field == -4) { cnt[(size_t)k] = (int32_t)x; have_id = true; }
      else ij[(size_t)k] = (int32_t)x;
    }
  }
  if (const ncfile::Var *v = ncfile::find(f, "static_berg")) if (host->f64[KID_B_STATIC_BERG] && ncfile::count(f, *v) == n)
    for (long long k = 0; k < n; ++k) host->f64[KID_B_STATIC_BERG][k] = ncfile::value(*v, k);
  // files with the old 32-bit `iceberg_num` carry no id_cnt / id_ij: the ids are then made by generate_id on the grid
  // (IO2:917-918), which needs the per-cell counters: id = 0 here, kid_read_restart fills them in
  for (long long k = 0; k < n; ++k) {
    if (host->id) host->id[k] = have_id ? (int64_t)cnt[(size_t)k] * ((int64_t)1 << 32) + (int64_t)ij[(size_t)k] : 0;   // id_from_2_ints FW:7276
    if (host->f64[KID_B_UVEL_OLD]) host->f64[KID_B_UVEL_OLD][k] = host->f64[KID_B_UVEL][k];
    if (host->f64[KID_B_VVEL_OLD]) host->f64[KID_B_VVEL_OLD][k] = host->f64[KID_B_VVEL][k];
    if (host->f64[KID_B_LON_OLD]) host->f64[KID_B_LON_OLD][k] = host->f64[KID_B_LON][k];
    if (host->f64[KID_B_LAT_OLD]) host->f64[KID_B_LAT_OLD][k] = host->f64[KID_B_LAT][k];
  }
  host->n = n;
  return KID_OK;
}

}  // extern "C"

extern "C" {

// bonds_iceberg.res.nc (IO2:466-583): one record per bond SIDE, in the order of the loop over bergs and their bond
// lists; the dem group (tangd1 .. broken) only with dem=T.  `bergs` supplies ids and cells of both ends.
int kid_restart_write_bonds(const char *path, const kid_params *p, const kid_berg_soa *bergs, const kid_bond_soa *bonds) {
  if (!path || !p || !bergs || !bonds || !bergs->id || !bonds->count || !bonds->other_id || bonds->n < bergs->n) return KID_EINVAL;
  const long long n = bergs->n, stride = bonds->n;
  std::unordered_map<int64_t, long long> row;
  for (long long k = 0; k < n; ++k) if (!bergs->i32[KID_BI_ALIVE] || bergs->i32[KID_BI_ALIVE][k]) row[bergs->id[k]] = k;
  std::vector<int32_t> c[8]; std::vector<double> dv[6];
  for (long long k = 0; k < n; ++k) {
    if (bergs->i32[KID_BI_ALIVE] && !bergs->i32[KID_BI_ALIVE][k]) continue;
    for (int sl = 0; sl < bonds->count[k] && sl < bonds->max_bonds; ++sl) {
      const int64_t oid = bonds->other_id[sl * stride + k];
      const auto it = row.find(oid);
      if (it == row.end()) return KID_EINVAL;   // the reference stops on a bond whose partner is missing (count_bonds, check_bond_quality)
      c[0].push_back(bergs->i32[KID_BI_INE][k]); c[1].push_back(bergs->i32[KID_BI_JNE][k]);
      c[2].push_back((int32_t)(bergs->id[k] >> 32)); c[3].push_back((int32_t)(bergs->id[k] & 0xffffffffll));
      c[4].push_back(bergs->i32[KID_BI_INE][it->second]); c[5].push_back(bergs->i32[KID_BI_JNE][it->second]);
      c[6].push_back((int32_t)(oid >> 32)); c[7].push_back((int32_t)(oid & 0xffffffffll));
      const int fields[5] = {KID_BOND_TANGD1, KID_BOND_TANGD2, KID_BOND_NSTRESS, KID_BOND_SSTRESS, KID_BOND_REL_ROTATION};
      for (int q = 0; q < 5; ++q) dv[q].push_back(bonds->f64[fields[q]] ? bonds->f64[fields[q]][sl * stride + k] : 0.);
      dv[5].push_back(bonds->broken ? (double)bonds->broken[sl * stride + k] : 0.);
    }
  }
  const long long nb = (long long)c[0].size();
  ncfile::File f;
  f.dims.emplace_back("i", nb); f.unlimited = 0; f.numrecs = nb;
  f.gatts = {ncfile::att_int("file_format_major_version", 0), ncfile::att_int("file_format_minor_version", 1), ncfile::att_int("time_axis", 0)};
  static const char *iname[8] = {"first_berg_ine", "first_berg_jne", "first_id_cnt", "first_id_ij", "other_berg_ine", "other_berg_jne", "other_id_cnt", "other_id_ij"};
  static const char *ilong[8] = {"iceberg ine of first berg in bond", "iceberg jne of first berg in bond", "counter component of iceberg id first berg in bond",
                                 "position component of iceberg id first berg in bond", "iceberg ine of second berg in bond", "iceberg jne of second berg in bond",
                                 "counter component of iceberg id second berg in bond", "position component of iceberg id second berg in bond"};
  static const char *dname[6] = {"tangd1", "tangd2", "nstress", "sstress", "rel_rotation", "broken"};
  static const char *dlong[6] = {"zonal tangential displacement", "meridional tangential displacement", "normal stress", "shear stress", "relative rotation", "broken status"};
  static const char *dunit[6] = {"m", "m", "Pa", "Pa", "rad", "none"};
  for (int q = 0; q < 8; ++q) {
    ncfile::Var v; v.name = iname[q]; v.dims = {0}; v.type = ncfile::NC_INT; v.record = true;
    v.atts = {ncfile::att_text("long_name", ilong[q]), ncfile::att_text("units", "dimensionless")};
    c[q].resize((size_t)std::max<long long>(nb, 1)); ncfile::set_data(v, c[q].data(), nb); f.vars.push_back(v);
  }
  if (p->dem) for (int q = 0; q < 6; ++q) {
    ncfile::Var v; v.name = dname[q]; v.dims = {0}; v.type = ncfile::NC_DOUBLE; v.record = true;
    v.atts = {ncfile::att_text("long_name", dlong[q]), ncfile::att_text("units", dunit[q])};
    dv[q].resize((size_t)std::max<long long>(nb, 1)); ncfile::set_data(v, dv[q].data(), nb); f.vars.push_back(v);
  }
  return ncfile::write(f, path) == 0 ? KID_OK : KID_EINVAL;
}

// read_restart_bonds (IO2:1190-1481) into a host bond SoA shaped (bonds->n rows, bonds->max_bonds slots) for the bergs
// of `bergs`: form_a_bond puts every new bond at the HEAD of the first berg's list, so a berg's slots come out in the
// reverse of the file's order.  A bond whose first berg is not among `bergs` is another rank's; a missing partner is the
// reference's FATAL (KID_EINVAL); more bonds than slots is KID_ECAPACITY.
int kid_restart_read_bonds(const char *path, const kid_berg_soa *bergs, kid_bond_soa *bonds) {
  if (!path || !bergs || !bonds || !bergs->id || !bonds->count || !bonds->other_id || bonds->n < bergs->n) return KID_EINVAL;
  ncfile::File f; std::string err;
  if (ncfile::read(path, f, err)) return KID_EINVAL;
  const ncfile::Var *fc = ncfile::find(f, "first_id_cnt"), *fi = ncfile::find(f, "first_id_ij"), *oc = ncfile::find(f, "other_id_cnt"), *oi = ncfile::find(f, "other_id_ij");
  if (!fc || !fi || !oc || !oi) return KID_EINVAL;
  const long long nb = ncfile::count(f, *fc), n = bergs->n, stride = bonds->n;
  const int mb = bonds->max_bonds;
  std::unordered_map<int64_t, long long> row;
  for (long long k = 0; k < n; ++k) row[bergs->id[k]] = k;
  for (long long k = 0; k < stride; ++k) bonds->count[k] = 0;
  for (long long q = 0; q < (long long)mb * stride; ++q) {
    bonds->other_id[q] = 0; if (bonds->broken) bonds->broken[q] = 0;
    for (int g = 0; g < KID_NBOND_F64; ++g) if (bonds->f64[g]) bonds->f64[g][q] = 0.;
  }
  static const char *dname[5] = {"tangd1", "tangd2", "nstress", "sstress", "rel_rotation"};
  const int dfield[5] = {KID_BOND_TANGD1, KID_BOND_TANGD2, KID_BOND_NSTRESS, KID_BOND_SSTRESS, KID_BOND_REL_ROTATION};
  const ncfile::Var *dvar[5]; for (int q = 0; q < 5; ++q) { dvar[q] = ncfile::find(f, dname[q]); if (dvar[q] && ncfile::count(f, *dvar[q]) != nb) dvar[q] = nullptr; }
  const ncfile::Var *bvar = ncfile::find(f, "broken"); if (bvar && ncfile::count(f, *bvar) != nb) bvar = nullptr;
  for (long long r = 0; r < nb; ++r) {
    const int64_t first = (int64_t)ncfile::value(*fc, r) * ((int64_t)1 << 32) + (int64_t)ncfile::value(*fi, r);
    const int64_t other = (int64_t)ncfile::value(*oc, r) * ((int64_t)1 << 32) + (int64_t)ncfile::value(*oi, r);
    const auto it = row.find(first);
    if (it == row.end()) continue;
    if (row.find(other) == row.end()) return KID_EINVAL;
    const long long k = it->second;
    if (bonds->count[k] >= mb) return KID_ECAPACITY;
    for (int sl = bonds->count[k]; sl > 0; --sl) {   // make room at the head of the list
      bonds->other_id[sl * stride + k] = bonds->other_id[(sl - 1) * stride + k];
      if (bonds->broken) bonds->broken[sl * stride + k] = bonds->broken[(sl - 1) * stride + k];
      for (int g = 0; g < KID_NBOND_F64; ++g) if (bonds->f64[g]) bonds->f64[g][sl * stride + k] = bonds->f64[g][(sl - 1) * stride + k];
    }
    bonds->other_id[k] = other;
    if (bonds->broken) bonds->broken[k] = bvar ? (int32_t)ncfile::value(*bvar, r) : 0;
    for (int g = 0; g < KID_NBOND_F64; ++g) if (bonds->f64[g]) bonds->f64[g][k] = 0.;
    for (int q = 0; q < 5; ++q) if (dvar[q] && bonds->f64[dfield[q]]) bonds->f64[dfield[q]][k] = ncfile::value(*dvar[q], r);
    bonds->count[k] += 1;
  }
  return KID_OK;
}

}  // extern "C"

// xi, yj of restored bergs: pos_within_cell on (lon, lat, ine, jne) as read_restart_bergs does (IO2:945)
__global__ void __launch_bounds__(256) restart_locate_kernel(const DevGrid g, const kid_params *pp, const BergPtrs b, long long n) {
  const long long k = (long long)blockIdx.x * 256ll + threadIdx.x;
  if (k >= n) return;
  const int i = b.i[KID_BI_INE][k], j = b.i[KID_BI_JNE][k];
  double xi = 0., yj = 0.;
  int err = 0; bool bail = false;
  const GlbCell cell{g, g.idx(i, j)};
  (void)pos_within_cell<false>(g, *pp, cell, b.f[KID_B_LON][k], b.f[KID_B_LAT][k], i, j, xi, yj, err, bail);
  b.f[KID_B_XI][k] = xi; b.f[KID_B_YJ][k] = yj;
}

extern "C" {

static void restart_calving_file(const kid_handle *h, const std::vector<double> &stored_ice, const std::vector<double> &stored_heat,
                                 const std::vector<int32_t> &counter, const std::vector<double> &rm, const std::vector<double> &rmh, ncfile::File &f) {
  const kid_grid_desc &d = h->gd;
  const int nic = d.iec - d.isc + 1, njc = d.jec - d.jsc + 1, ni = h->ni;
  f.dims = {{"xaxis_1", nic}, {"yaxis_1", njc}, {"zaxis_1", KID_NCLASSES}, {"Time", 1}};   // IO2:598-601
  f.unlimited = 3; f.numrecs = 1;
  auto axis = [&](const char *name, int dim, int n, const char *ax) {
    ncfile::Var v; v.name = name; v.dims = {dim}; v.type = ncfile::NC_DOUBLE; v.record = dim == 3; v.atts = {ncfile::att_text("axis", ax)};
    std::vector<double> x((size_t)n); for (int q = 0; q < n; ++q) x[(size_t)q] = q + 1.0;
    ncfile::set_data(v, x.data(), n); f.vars.push_back(v);
  };
  axis("xaxis_1", 0, nic, "X"); axis("yaxis_1", 1, njc, "Y"); axis("zaxis_1", 2, KID_NCLASSES, "Z"); axis("Time", 3, 1, "T");
  auto comp = [&](const double *plane, std::vector<double> &out) {  // computational domain of a data-domain plane
    for (int j = 0; j < njc; ++j) for (int i = 0; i < nic; ++i) out.push_back(plane[(size_t)(i + d.isc - d.isd) + (size_t)(j + d.jsc - d.jsd) * ni]);
  };
  auto field = [&](const char *name, const char *longname, std::vector<int> dims, int type) -> ncfile::Var & {
    ncfile::Var v; v.name = name; v.dims = dims; v.type = type; v.record = true;
    v.atts = {ncfile::att_text("long_name", longname), ncfile::att_text("units", "none")};
    f.vars.push_back(v); return f.vars.back();
  };
  { std::vector<double> x; for (int k = 0; k < KID_NCLASSES; ++k) comp(stored_ice.data() + (size_t)k * h->ncell, x);
    ncfile::set_data(field("stored_ice", "STORED_ICE", {3, 2, 1, 0}, ncfile::NC_DOUBLE), x.data(), (long long)x.size()); }
  { std::vector<double> x; comp(stored_heat.data(), x);
    ncfile::set_data(field("stored_heat", "STORED_HEAT", {3, 1, 0}, ncfile::NC_DOUBLE), x.data(), (long long)x.size()); }
  { std::vector<int32_t> x; for (int j = 0; j < njc; ++j) for (int i = 0; i < nic; ++i) x.push_back(counter[(size_t)(i + d.isc - d.isd) + (size_t)(j + d.jsc - d.jsd) * ni]);
    ncfile::set_data(field("iceberg_counter_grd", "ICEBERG_COUNTER_GRD", {3, 1, 0}, ncfile::NC_INT), x.data(), (long long)x.size()); }
  if (h->calv_params.tau_calving > 0.) {
    { std::vector<double> x; comp(rm.data(), x); ncfile::set_data(field("rmean_calving", "RMEAN_CALVING", {3, 1, 0}, ncfile::NC_DOUBLE), x.data(), (long long)x.size()); }
    { std::vector<double> x; comp(rmh.data(), x); ncfile::set_data(field("rmean_calving_hflx", "RMEAN_CALVING_HFLX", {3, 1, 0}, ncfile::NC_DOUBLE), x.data(), (long long)x.size()); }
  }
}

// write_restart_bergs (IO2:124-631) from the resident state: <dir>/icebergs.res.nc and, when the calving source is on,
// <dir>/calving.res.nc (buckets, stored heat, the id counters, the running means)
int kid_write_restart(kid_handle *h, const char *dir) {
  if (!h || !dir) return KID_EINVAL;
  { const int rc_h = halo_rows_refuse(h, "kid_write_restart"); if (rc_h) return rc_h; }
  int64_t n_slots = 0, n_alive = 0;
  int rc = kid_num_bergs(h, &n_slots, &n_alive);
  if (rc) return rc;
  const size_t n = (size_t)std::max<int64_t>(n_slots, 1);
  std::vector<std::vector<double>> f64(KID_NB_F64, std::vector<double>(n));
  std::vector<std::vector<int32_t>> i32(KID_NB_I32, std::vector<int32_t>(n));
  std::vector<int64_t> id(n);
  kid_berg_soa soa{};
  soa.n = n_slots;
  for (int q = 0; q < KID_NB_F64; ++q) soa.f64[q] = f64[(size_t)q].data();
  for (int q = 0; q < KID_NB_I32; ++q) soa.i32[q] = i32[(size_t)q].data();
  soa.id = id.data();
  rc = kid_download_bergs(h, &soa);
  if (rc) return rc;
  const std::string base(dir);
  if (kid_restart_write_bergs((base + "/icebergs.res.nc").c_str(), &h->params, &soa)) { h->err = "cannot write " + base + "/icebergs.res.nc"; return KID_EINVAL; }
  if (h->have_bonds) {  // bonds_iceberg.res.nc, IO2:466-583
    const size_t mb = (size_t)h->mb;
    std::vector<int32_t> bcount(n), bbroken(n * mb);
    std::vector<int64_t> bother(n * mb);
    std::vector<std::vector<double>> bf(KID_NBOND_F64, std::vector<double>(n * mb));
    kid_bond_soa bs{};
    bs.n = n_slots; bs.max_bonds = h->mb; bs.count = bcount.data(); bs.other_id = bother.data(); bs.broken = bbroken.data();
    for (int g = 0; g < KID_NBOND_F64; ++g) bs.f64[g] = bf[(size_t)g].data();
    rc = kid_download_bonds(h, &bs);
    if (rc) return rc;
    if (kid_restart_write_bonds((base + "/bonds_iceberg.res.nc").c_str(), &h->params, &soa, &bs)) { h->err = "cannot write " + base + "/bonds_iceberg.res.nc (a bond whose partner is gone?)"; return KID_EINVAL; }
  }
  if (h->calving_on) {
    std::vector<double> ice((size_t)KID_NCLASSES * h->ncell), heat(h->ncell), rm(h->ncell), rmh(h->ncell);
    std::vector<int32_t> counter(h->ncell);
    rc = kid_get_calving_state(h, ice.data(), heat.data(), rm.data(), rmh.data(), nullptr);
    if (rc) return rc;
    rc = kid_get_iceberg_counter(h, counter.data());
    if (rc) return rc;
    ncfile::File f;
    restart_calving_file(h, ice, heat, counter, rm, rmh, f);
    if (ncfile::write(f, (base + "/calving.res.nc").c_str())) { h->err = "cannot write " + base + "/calving.res.nc"; return KID_EINVAL; }
  }
  return KID_OK;
}

// read_restart_bergs (IO2:663-1049) + read_restart_calving into the handle: bergs whose (ine, jne) lies outside the
// computational domain are not this rank's (IO2:880-884), bergs in cells of zero area are dropped as grounded
// (IO2:948-955); xi, yj are recomputed on the device.  calving.res.nc is read when it exists and the calving source is on.
// With kid_set_restart_locate (ignore_ij_restart) the cells come from the positions instead (kid_locate.inc); the rest is the same.
int kid_read_restart(kid_handle *h, const char *dir) {
  if (!h || !dir) return KID_EINVAL;
  if (need_static(h)) return KID_EINVAL;
  KID_HIP(h, hipSetDevice(h->device));
  { const int rc_f = rebin_flush(h); if (rc_f) return rc_f; }
  const std::string base(dir), path = base + "/icebergs.res.nc";
  int64_t nfile = 0;
  if (kid_restart_count_bergs(path.c_str(), &nfile)) {
    ncfile::File f; std::string err; (void)ncfile::read(path.c_str(), f, err);
    h->err = "cannot read " + path + (err.empty() ? "" : ": " + err); return KID_EINVAL;
  }
  const size_t n = (size_t)std::max<int64_t>(nfile, 1);
  std::vector<std::vector<double>> f64(KID_NB_F64, std::vector<double>(n));
  std::vector<std::vector<int32_t>> i32(KID_NB_I32, std::vector<int32_t>(n));
  std::vector<int64_t> id(n);
  kid_berg_soa soa{};
  for (int q = 0; q < KID_NB_F64; ++q) soa.f64[q] = f64[(size_t)q].data();
  for (int q = 0; q < KID_NB_I32; ++q) soa.i32[q] = i32[(size_t)q].data();
  soa.id = id.data();
  int rc = kid_restart_read_bergs(path.c_str(), &soa, nfile);
  if (rc) { h->err = "cannot read " + path; return rc; }
  if (h->restart_locate) {   // ignore_ij_restart (IO2:885-890): the file's ine, jne are not read; each berg's cell is searched from lon, lat
    rc = restart_locate_cells(h, f64[KID_B_LON].data(), f64[KID_B_LAT].data(), i32[KID_BI_INE].data(), i32[KID_BI_JNE].data(), nfile);
    if (rc) return rc;
  }
  std::vector<double> area(h->ncell);
  KID_HIP(h, hipMemcpy(area.data(), h->d_static[KID_G_AREA], h->ncell * sizeof(double), hipMemcpyDeviceToHost));
  const kid_grid_desc &d = h->gd;
  // a file of the 32-bit era carries iceberg_num instead of id_cnt / id_ij: every id reads as 0 (a real id is 0 only with
  // cnt = ij = 0, which generate_id never hands out).  replace_iceberg_num (IO2:743): generate_id for every berg of the
  // computational domain in file order (IO2:917-918) -- BEFORE the grounded-cell filter (IO2:948), so a grounded berg still
  // takes a value of its cell's counter, as in the reference.
  bool legacy_ids = nfile > 0;
  for (long long k = 0; k < nfile && legacy_ids; ++k) legacy_ids = id[(size_t)k] == 0;
  std::vector<int32_t> counter;
  if (legacy_ids) {
    counter.resize(h->ncell);
    rc = kid_get_iceberg_counter(h, counter.data());
    if (rc) return rc;
  }
  const int iNg = id_iNg(d), ij0 = id_ij0(d);   // (a tile of a decomposed grid hashes the GLOBAL cell, FW:4233-4236)
  long long m = 0;
  for (long long k = 0; k < nfile; ++k) {
    const int i = i32[KID_BI_INE][(size_t)k], j = i32[KID_BI_JNE][(size_t)k];
    if (i < d.isc || i > d.iec || j < d.jsc || j > d.jec) continue;
    if (legacy_ids) {
      const int32_t c = ++counter[(size_t)(i - d.isd) + (size_t)(j - d.jsd) * h->ni];
      id[(size_t)k] = (int64_t)c * ((int64_t)1 << 32) + (int64_t)(i + iNg * (j - 1) + ij0);      // FW:4165-4179, 4224-4239
    }
    if (area[(size_t)(i - d.isd) + (size_t)(j - d.jsd) * h->ni] == 0.) continue;
    if (m != k) {
      for (int q = 0; q < KID_NB_F64; ++q) f64[(size_t)q][(size_t)m] = f64[(size_t)q][(size_t)k];
      for (int q = 0; q < KID_NB_I32; ++q) i32[(size_t)q][(size_t)m] = i32[(size_t)q][(size_t)k];
      id[(size_t)m] = id[(size_t)k];
    }
    ++m;
  }
  soa.n = m;
  if (legacy_ids) {
    rc = kid_set_iceberg_counter(h, counter.data());
    if (rc) return rc;
  }
  rc = kid_upload_bergs(h, &soa);
  if (rc) return rc;
  if (m > 0) {
    rc = refresh_tables(h);
    if (rc) return rc;
    hipLaunchKernelGGL(restart_locate_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, h->stream, dev_grid(h), h->d_params, h->bp, (long long)m);
    KID_HIP(h, hipGetLastError());
  }
  if (h->params.iceberg_bonds_on && m > 0) {  // read_restart_bonds, IO2:1190-1481
    const std::string bpath = base + "/bonds_iceberg.res.nc";
    FILE *probe = std::fopen(bpath.c_str(), "rb");
    if (probe) {
      std::fclose(probe);
      const size_t mm = (size_t)m, mb = (size_t)(h->params.max_bonds > 0 ? h->params.max_bonds : KID_MAX_BONDS);
      std::vector<int32_t> bcount(mm), bbroken(mm * mb);
      std::vector<int64_t> bother(mm * mb);
      std::vector<std::vector<double>> bf(KID_NBOND_F64, std::vector<double>(mm * mb));
      kid_bond_soa bs{};
      bs.n = m; bs.max_bonds = (int32_t)mb; bs.count = bcount.data(); bs.other_id = bother.data(); bs.broken = bbroken.data();
      for (int g = 0; g < KID_NBOND_F64; ++g) bs.f64[g] = bf[(size_t)g].data();
      rc = kid_restart_read_bonds(bpath.c_str(), &soa, &bs);
      if (rc) { h->err = rc == KID_ECAPACITY ? "more bonds on a berg than max_bonds" : "cannot read " + bpath + " (or a bond partner is missing)"; return rc; }
      rc = kid_upload_bonds(h, &bs);
      if (rc) return rc;
    }
  }
  if (h->calving_on) {
    ncfile::File f; std::string err;
    if (ncfile::read((base + "/calving.res.nc").c_str(), f, err) == 0) {
      const int nic = d.iec - d.isc + 1, njc = d.jec - d.jsc + 1;
      auto plane = [&](const ncfile::Var &v, long long off, double *out) {  // computational-domain values into a zeroed data-domain plane
        for (int j = 0; j < njc; ++j) for (int i = 0; i < nic; ++i)
          out[(size_t)(i + d.isc - d.isd) + (size_t)(j + d.jsc - d.jsd) * h->ni] = ncfile::value(v, off + (long long)j * nic + i);
      };
      const ncfile::Var *ice = ncfile::find(f, "stored_ice"), *heat = ncfile::find(f, "stored_heat"), *cnt = ncfile::find(f, "iceberg_counter_grd");
      const ncfile::Var *rm = ncfile::find(f, "rmean_calving"), *rmh = ncfile::find(f, "rmean_calving_hflx");
      if (!ice || !heat || ncfile::count(f, *ice) != (long long)KID_NCLASSES * nic * njc || ncfile::count(f, *heat) != (long long)nic * njc) {
        h->err = "calving.res.nc does not match the grid"; return KID_EINVAL;
      }
      std::vector<double> pice((size_t)KID_NCLASSES * h->ncell, 0.), pheat(h->ncell, 0.), prm(h->ncell, 0.), prmh(h->ncell, 0.);
      for (int k = 0; k < KID_NCLASSES; ++k) plane(*ice, (long long)k * nic * njc, pice.data() + (size_t)k * h->ncell);
      plane(*heat, 0, pheat.data());
      if (rm) plane(*rm, 0, prm.data());
      if (rmh) plane(*rmh, 0, prmh.data());
      rc = kid_set_calving_state(h, pice.data(), pheat.data(), rm ? prm.data() : nullptr, rmh ? prmh.data() : nullptr);
      if (rc) return rc;
      if (cnt && ncfile::count(f, *cnt) == (long long)nic * njc) {
        std::vector<double> pc(h->ncell, 0.); plane(*cnt, 0, pc.data());
        std::vector<int32_t> ic(h->ncell); for (size_t q = 0; q < h->ncell; ++q) ic[q] = (int32_t)pc[q];
        rc = kid_set_iceberg_counter(h, ic.data());
        if (rc) return rc;
      }
    }
  }
  KID_HIP(h, hipStreamSynchronize(h->stream));
  return KID_OK;
}

}  // extern "C"
