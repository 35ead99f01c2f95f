// cooler_reader.cpp -- the cooler (v3) reader behind include/modle_cooler_read.h (host side, HDF5 C API):
// opens the root of a .cool or one /resolutions/<bin size> group of an .mcool, validates what the kernels rely
// on (fixed bins, integer counts, indexes of the right length) and hands over a chromosome's slice of the pixel
// table as it lies in the file.
//
// This file is the second half of cooler_writer.cpp's translation unit (it is included at that file's end and is
// not compiled on its own): it shares read_all / read_slice and set_err with modle_cool_read_band instead of
// copying them, and the build recipe of libmodle_cooler.so stays as it is.
#include <new>

#include "modle_cooler_read.h"

struct modle_cool_reader {
  hid_t file = -1;
  hid_t group = -1;  // the cooler's location: the root group or /resolutions/<bin size>
  std::string uri;
  uint32_t bin_size = 0;
  std::vector<std::string> names;
  std::vector<int64_t> sizes, chrom_offset, bin1_offset;
  std::vector<int64_t> bin1, bin2;  // the slice of the last modle_cool_reader_pixels
  std::vector<int32_t> count;
};

namespace {

// a string attribute, of fixed or variable length; false when it is missing or no string
bool read_attr_string(hid_t loc, const char* name, std::string& out) {
  if (H5Aexists(loc, name) <= 0) return false;
  const hid_t a = H5Aopen(loc, name, H5P_DEFAULT);
  if (a < 0) return false;
  const hid_t t = H5Aget_type(a);
  bool ok = false;
  if (t >= 0 && H5Tget_class(t) == H5T_STRING) {
    if (H5Tis_variable_str(t) > 0) {
      char* p = nullptr;
      const hid_t mt = H5Tcopy(H5T_C_S1);
      H5Tset_size(mt, H5T_VARIABLE);
      H5Tset_cset(mt, H5Tget_cset(t));
      if (H5Aread(a, mt, &p) >= 0 && p != nullptr) {
        out = p;
        H5free_memory(p);
        ok = true;
      }
      H5Tclose(mt);
    } else {
      std::vector<char> buf(H5Tget_size(t) + 1, 0);
      if (H5Aread(a, t, buf.data()) >= 0) {
        out = std::string(buf.data(), strnlen(buf.data(), buf.size() - 1));
        ok = true;
      }
    }
  }
  if (t >= 0) H5Tclose(t);
  H5Aclose(a);
  return ok;
}

herr_t collect_name(hid_t, const char* name, const H5L_info_t*, void* data) {
  static_cast<std::vector<std::string>*>(data)->push_back(name);
  return 0;
}

// "10000, 50000" of the groups below /resolutions; "none" for a file without them
std::string list_resolutions(hid_t file) {
  std::vector<std::string> found;
  if (H5Lexists(file, "resolutions", H5P_DEFAULT) > 0) {
    const hid_t g = H5Gopen2(file, "resolutions", H5P_DEFAULT);
    if (g >= 0) {
      hsize_t idx = 0;
      H5Literate(g, H5_INDEX_NAME, H5_ITER_INC, &idx, collect_name, &found);
      H5Gclose(g);
    }
  }
  if (found.empty()) return "none";
  std::string s;
  for (const auto& f : found) s += (s.empty() ? "" : ", ") + f;
  return s;
}

// whether every component of the absolute path `group` exists (H5Lexists wants them checked one by one)
bool group_exists(hid_t file, const std::string& group) {
  size_t pos = 0;
  while (pos < group.size()) {
    while (pos < group.size() && group[pos] == '/') ++pos;
    if (pos >= group.size()) break;
    size_t end = group.find('/', pos);
    if (end == std::string::npos) end = group.size();
    if (H5Lexists(file, group.substr(0, end).c_str(), H5P_DEFAULT) <= 0) return false;
    pos = end;
  }
  return true;
}

bool read_names(hid_t loc, std::vector<std::string>& out) {
  const hid_t d = H5Dopen2(loc, "chroms/name", H5P_DEFAULT);
  if (d < 0) return false;
  const hid_t ft = H5Dget_type(d);
  const hid_t sp = H5Dget_space(d);
  const hssize_t n = H5Sget_simple_extent_npoints(sp);
  bool ok = ft >= 0 && n >= 0 && H5Tget_class(ft) == H5T_STRING && H5Tis_variable_str(ft) <= 0;
  if (ok) {
    const size_t mlen = H5Tget_size(ft) + 1;  // room for the terminator of the memory type
    std::vector<char> buf(static_cast<size_t>(n) * mlen + 1, 0);
    const hid_t mt = H5Tcopy(H5T_C_S1);
    H5Tset_size(mt, mlen);
    ok = n == 0 || H5Dread(d, mt, H5S_ALL, H5S_ALL, H5P_DEFAULT, buf.data()) >= 0;
    H5Tclose(mt);
    for (hssize_t i = 0; ok && i < n; ++i) {
      const char* p = buf.data() + static_cast<size_t>(i) * mlen;
      out.emplace_back(p, strnlen(p, mlen));
    }
  }
  if (sp >= 0) H5Sclose(sp);
  if (ft >= 0) H5Tclose(ft);
  H5Dclose(d);
  return ok;
}

int fail(modle_cool_reader* r, int rc, char* err, size_t errlen, const std::string& msg) {
  set_err(err, errlen, msg);
  modle_cool_reader_close(r);
  return rc;
}

}  // namespace

namespace {
int open_impl(const char* uri, modle_cool_reader** out, char* err, size_t errlen) {
  const std::string u(uri);
  const size_t sep = u.find("::");
  const std::string path = u.substr(0, sep);
  std::string group = sep == std::string::npos ? "/" : u.substr(sep + 2);
  if (group.empty() || group[0] != '/') group = "/" + group;
  auto* r = new (std::nothrow) modle_cool_reader;
  if (r == nullptr) {
    set_err(err, errlen, "modle_cool_reader_open: out of memory");
    return MODLE_COOL_ERR_IO;
  }
  r->uri = u;
  const std::string what = "\"" + u + "\"";
  r->file = H5Fopen(path.c_str(), H5F_ACC_RDONLY, H5P_DEFAULT);
  if (r->file < 0) return fail(r, MODLE_COOL_ERR_IO, err, errlen, "unable to open \"" + path + "\" as an HDF5 file");
  if (!group_exists(r->file, group) || (r->group = H5Gopen2(r->file, group.c_str(), H5P_DEFAULT)) < 0)
    return fail(r, MODLE_COOL_ERR_ARG, err, errlen,
                "\"" + path + "\" has no group " + group + " (resolutions of the file: " + list_resolutions(r->file) + ")");
  const hid_t g = r->group;
  if (H5Lexists(g, "pixels", H5P_DEFAULT) <= 0 || H5Lexists(g, "chroms", H5P_DEFAULT) <= 0 ||
      H5Lexists(g, "indexes", H5P_DEFAULT) <= 0)
    return fail(r, MODLE_COOL_ERR_ARG, err, errlen,
                what + " is no cooler: the group " + group + " has no chroms, pixels and indexes (resolutions of the file: " +
                    list_resolutions(r->file) + ")");
  std::string bin_type = "fixed";  // (what a file without the attribute is taken to be, as cooler does)
  if (read_attr_string(g, "bin-type", bin_type) && bin_type != "fixed")
    return fail(r, MODLE_COOL_ERR_ARG, err, errlen,
                what + " has bin-type \"" + bin_type + "\": only fixed-width bins are read");
  {
    const hid_t a = H5Aexists(g, "bin-size") > 0 ? H5Aopen(g, "bin-size", H5P_DEFAULT) : -1;
    int64_t bs = 0;
    const bool ok = a >= 0 && H5Aread(a, H5T_NATIVE_INT64, &bs) >= 0;
    if (a >= 0) H5Aclose(a);
    if (!ok || bs <= 0 || bs > 0xFFFFFFFFll)
      return fail(r, MODLE_COOL_ERR_ARG, err, errlen, what + " has no usable bin-size attribute");
    r->bin_size = static_cast<uint32_t>(bs);
  }
  {
    const hid_t d = H5Dopen2(g, "pixels/count", H5P_DEFAULT);
    const hid_t t = d >= 0 ? H5Dget_type(d) : -1;
    const bool integer = t >= 0 && H5Tget_class(t) == H5T_INTEGER;
    if (t >= 0) H5Tclose(t);
    if (d >= 0) H5Dclose(d);
    if (d < 0) return fail(r, MODLE_COOL_ERR_IO, err, errlen, what + ": cannot open pixels/count");
    if (!integer)
      return fail(r, MODLE_COOL_ERR_ARG, err, errlen,
                  what + ": pixels/count is no integer type: only raw integer counts are read");
  }
  if (!read_names(g, r->names) || !read_all(g, "chroms/length", H5T_NATIVE_INT64, r->sizes) ||
      !read_all(g, "indexes/chrom_offset", H5T_NATIVE_INT64, r->chrom_offset) ||
      !read_all(g, "indexes/bin1_offset", H5T_NATIVE_INT64, r->bin1_offset))
    return fail(r, MODLE_COOL_ERR_IO, err, errlen, "HDF5 error while reading the chromosomes and indexes of " + what);
  const size_t nc = r->names.size();
  bool ok = r->sizes.size() == nc && r->chrom_offset.size() == nc + 1 && r->chrom_offset[0] == 0;
  for (size_t c = 0; ok && c < nc; ++c) {
    const int64_t bins = (r->sizes[c] + r->bin_size - 1) / r->bin_size;
    ok = r->sizes[c] >= 0 && r->chrom_offset[c + 1] - r->chrom_offset[c] == bins;
  }
  if (!ok)
    return fail(r, MODLE_COOL_ERR_ARG, err, errlen,
                what + ": indexes/chrom_offset does not match the chromosomes at the bin size " + std::to_string(r->bin_size));
  const uint64_t n_bins = static_cast<uint64_t>(r->chrom_offset[nc]);
  if (r->bin1_offset.size() != n_bins + 1)
    return fail(r, MODLE_COOL_ERR_ARG, err, errlen,
                what + ": indexes/bin1_offset has " + std::to_string(r->bin1_offset.size()) + " entries, the " +
                    std::to_string(n_bins) + " bins need " + std::to_string(n_bins + 1));
  for (size_t b = 0; b + 1 < r->bin1_offset.size(); ++b)
    if (r->bin1_offset[b] < 0 || r->bin1_offset[b] > r->bin1_offset[b + 1])
      return fail(r, MODLE_COOL_ERR_ARG, err, errlen, what + ": indexes/bin1_offset does not ascend from 0");
  *out = r;
  return MODLE_COOL_OK;
}
}  // namespace

extern "C" int modle_cool_reader_open(const char* uri, modle_cool_reader** out, char* err, size_t errlen) {
  if (out != nullptr) *out = nullptr;
  if (uri == nullptr || out == nullptr) {
    set_err(err, errlen, "modle_cool_reader_open: invalid argument");
    return MODLE_COOL_ERR_ARG;
  }
  // a probe that fails is a return code here, not text on stderr: HDF5's printing is off for the call
  H5E_auto2_t print = nullptr;
  void* print_data = nullptr;
  H5Eget_auto2(H5E_DEFAULT, &print, &print_data);
  H5Eset_auto2(H5E_DEFAULT, nullptr, nullptr);
  const int rc = open_impl(uri, out, err, errlen);
  H5Eset_auto2(H5E_DEFAULT, print, print_data);
  return rc;
}

extern "C" int modle_cool_reader_info(const modle_cool_reader* r, uint32_t* bin_size, size_t* n_chroms) {
  if (r == nullptr) return MODLE_COOL_ERR_ARG;
  if (bin_size != nullptr) *bin_size = r->bin_size;
  if (n_chroms != nullptr) *n_chroms = r->names.size();
  return MODLE_COOL_OK;
}

extern "C" int modle_cool_reader_chrom(const modle_cool_reader* r, size_t chrom_id, const char** name, uint64_t* size,
                                       int64_t* first_bin, uint64_t* n_bins) {
  if (r == nullptr || chrom_id >= r->names.size()) return MODLE_COOL_ERR_ARG;
  if (name != nullptr) *name = r->names[chrom_id].c_str();
  if (size != nullptr) *size = static_cast<uint64_t>(r->sizes[chrom_id]);
  if (first_bin != nullptr) *first_bin = r->chrom_offset[chrom_id];
  if (n_bins != nullptr) *n_bins = static_cast<uint64_t>(r->chrom_offset[chrom_id + 1] - r->chrom_offset[chrom_id]);
  return MODLE_COOL_OK;
}

extern "C" int modle_cool_reader_indexes(const modle_cool_reader* r, const int64_t** chrom_offset,
                                         const int64_t** bin1_offset, uint64_t* n_bins) {
  if (r == nullptr) return MODLE_COOL_ERR_ARG;
  if (chrom_offset != nullptr) *chrom_offset = r->chrom_offset.data();
  if (bin1_offset != nullptr) *bin1_offset = r->bin1_offset.data();
  if (n_bins != nullptr) *n_bins = r->bin1_offset.size() - 1;
  return MODLE_COOL_OK;
}

extern "C" int modle_cool_reader_pixels(modle_cool_reader* r, size_t chrom_id, const int64_t** bin1,
                                        const int64_t** bin2, const int32_t** count, uint64_t* n, int64_t* first_bin,
                                        char* err, size_t errlen) {
  if (r == nullptr || bin1 == nullptr || bin2 == nullptr || count == nullptr || n == nullptr ||
      chrom_id >= r->names.size()) {
    set_err(err, errlen, "modle_cool_reader_pixels: invalid argument");
    return MODLE_COOL_ERR_ARG;
  }
  const int64_t b0 = r->chrom_offset[chrom_id], b1 = r->chrom_offset[chrom_id + 1];
  const hsize_t p0 = static_cast<hsize_t>(r->bin1_offset[static_cast<size_t>(b0)]);
  const hsize_t p1 = static_cast<hsize_t>(r->bin1_offset[static_cast<size_t>(b1)]);
  if (!read_slice(r->group, "pixels/bin1_id", H5T_NATIVE_INT64, p0, p1 - p0, r->bin1) ||
      !read_slice(r->group, "pixels/bin2_id", H5T_NATIVE_INT64, p0, p1 - p0, r->bin2) ||
      !read_slice(r->group, "pixels/count", H5T_NATIVE_INT32, p0, p1 - p0, r->count)) {
    *bin1 = *bin2 = nullptr, *count = nullptr, *n = 0;
    set_err(err, errlen, "HDF5 error while reading the pixels " + std::to_string(p0) + " .. " + std::to_string(p1) +
                             " of \"" + r->uri + "\" (is indexes/bin1_offset beyond the pixel table?)");
    return MODLE_COOL_ERR_IO;
  }
  *bin1 = r->bin1.data(), *bin2 = r->bin2.data(), *count = r->count.data();
  *n = p1 - p0;
  if (first_bin != nullptr) *first_bin = b0;
  return MODLE_COOL_OK;
}

extern "C" void modle_cool_reader_close(modle_cool_reader* r) {
  if (r == nullptr) return;
  if (r->group >= 0) H5Gclose(r->group);
  if (r->file >= 0) H5Fclose(r->file);
  delete r;
}
