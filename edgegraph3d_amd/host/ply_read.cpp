// ply_read.cpp — eg3d_host_read_ply_points (include/eg3d/host_nearest.hpp): the `element vertex` of an ASCII or binary
// little-endian PLY file as points. The file comes from outside the project: it is read whole into one buffer with a NUL
// behind it, every read of the buffer is checked against its end, and no count of the header sizes an allocation before
// it has been held against the bytes that are there.
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/eg3d/host_nearest.hpp"

namespace eg3d {
namespace nearest {
extern thread_local std::string g_host_err;
}
}  // namespace eg3d

namespace {

int refuse(int code, const std::string& text) {
  eg3d::nearest::g_host_err = "eg3d_host_read_ply_points: " + text;
  return code;
}

// the size of a scalar PLY type, 0 = unknown; *is_float: float / float32
size_t scalar_size(const std::string& t, bool* is_float) {
  *is_float = t == "float" || t == "float32";
  if (t == "char" || t == "uchar" || t == "int8" || t == "uint8") return 1;
  if (t == "short" || t == "ushort" || t == "int16" || t == "uint16") return 2;
  if (t == "int" || t == "uint" || t == "int32" || t == "uint32" || *is_float) return 4;
  if (t == "double" || t == "float64") return 8;
  return 0;
}

std::vector<std::string> words(const std::string& line) {
  std::vector<std::string> w;
  size_t i = 0;
  while (i < line.size()) {
    while (i < line.size() && (line[i] == ' ' || line[i] == '\t')) i++;
    size_t j = i;
    while (j < line.size() && line[j] != ' ' && line[j] != '\t') j++;
    if (j > i) w.push_back(line.substr(i, j - i));
    i = j;
  }
  return w;
}

bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v'; }

}  // namespace

extern "C" void eg3d_host_free_points(float* X) { free(X); }

extern "C" int eg3d_host_read_ply_points(const char* path, float** X_out, uint64_t* n_out) {
  if (!path || !X_out || !n_out) return refuse(EG3D_NEAREST_ERR_ARG, "bad arguments");
  FILE* f = fopen(path, "rb");
  if (!f) return refuse(EG3D_NEAREST_ERR_FILE, std::string("cannot open ") + path);
  std::vector<char> buf;
  {
    char chunk[1 << 16];
    size_t got;
    while ((got = fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) return refuse(EG3D_NEAREST_ERR_FILE, std::string("cannot read ") + path);
  }
  const size_t size = buf.size();
  buf.push_back('\0');  // (strtod below stops here at the latest)
  const char* p = buf.data();

  // ---- header: lines up to end_header
  size_t pos = 0;
  bool ended = false, first = true, in_vertex = false, seen_vertex = false, after_vertex = false;
  int format = 0;  // 1 ascii, 2 binary little-endian
  uint64_t n_vertex = 0;
  struct Prop {
    size_t size, offset;
    bool is_float;
  };
  std::vector<Prop> props;
  int at[3] = {-1, -1, -1};
  size_t stride = 0;
  while (pos < size) {
    size_t e = pos;
    while (e < size && p[e] != '\n') e++;
    if (e == size) break;  // (a last line without a newline cannot be end_header followed by a body)
    std::string line(p + pos, e - pos);
    pos = e + 1;
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
    const std::vector<std::string> w = words(line);
    if (first) {
      if (w.size() != 1 || w[0] != "ply") return refuse(EG3D_NEAREST_ERR_PLY, "not a PLY file (no \"ply\" in the first line)");
      first = false;
      continue;
    }
    if (w.empty() || w[0] == "comment" || w[0] == "obj_info") continue;
    if (w[0] == "end_header") {
      ended = true;
      break;
    }
    if (w[0] == "format") {
      if (w.size() >= 2 && w[1] == "binary_big_endian") return refuse(EG3D_NEAREST_ERR_PLY, "big-endian files are not read");
      if (w.size() != 3 || w[2] != "1.0" || (w[1] != "ascii" && w[1] != "binary_little_endian"))
        return refuse(EG3D_NEAREST_ERR_PLY, "unknown format line: " + line);
      format = w[1] == "ascii" ? 1 : 2;
    } else if (w[0] == "element") {
      if (w.size() != 3) return refuse(EG3D_NEAREST_ERR_PLY, "malformed element line: " + line);
      if (in_vertex) after_vertex = true;
      in_vertex = false;
      if (w[1] == "vertex" && !seen_vertex) {
        errno = 0;
        char* end = nullptr;
        const unsigned long long v = strtoull(w[2].c_str(), &end, 10);
        if (errno || !end || *end || w[2][0] == '-') return refuse(EG3D_NEAREST_ERR_PLY, "malformed vertex count: " + line);
        n_vertex = v;
        in_vertex = seen_vertex = true;
      } else if (!seen_vertex) {
        return refuse(EG3D_NEAREST_ERR_PLY, "an element before `vertex` is not read: " + line);
      }
    } else if (w[0] == "property") {
      if (!in_vertex) {
        if (!after_vertex) return refuse(EG3D_NEAREST_ERR_PLY, "a property outside an element: " + line);
        continue;  // (elements after vertex are ignored)
      }
      if (w.size() >= 2 && w[1] == "list") return refuse(EG3D_NEAREST_ERR_PLY, "a list property inside `vertex`: " + line);
      if (w.size() != 3) return refuse(EG3D_NEAREST_ERR_PLY, "malformed property line: " + line);
      bool is_float = false;
      const size_t sz = scalar_size(w[1], &is_float);
      if (!sz) return refuse(EG3D_NEAREST_ERR_PLY, "unknown property type: " + line);
      if (props.size() >= 4096) return refuse(EG3D_NEAREST_ERR_PLY, "more than 4096 properties in `vertex`");
      for (int a = 0; a < 3; a++)
        if (w[2] == (a == 0 ? "x" : a == 1 ? "y" : "z")) {
          if (!is_float) return refuse(EG3D_NEAREST_ERR_PLY, "property " + w[2] + " is not a float");
          if (at[a] >= 0) return refuse(EG3D_NEAREST_ERR_PLY, "property " + w[2] + " is declared twice");
          at[a] = (int)props.size();
        }
      props.push_back(Prop{sz, stride, is_float});
      stride += sz;
    } else {
      return refuse(EG3D_NEAREST_ERR_PLY, "the header does not end (no end_header before the line: " + line.substr(0, 80) + ")");
    }
  }
  if (first) return refuse(EG3D_NEAREST_ERR_PLY, "not a PLY file (no \"ply\" in the first line)");
  if (!ended) return refuse(EG3D_NEAREST_ERR_PLY, "the header does not end (no end_header line)");
  if (!format) return refuse(EG3D_NEAREST_ERR_PLY, "the header has no format line");
  if (!seen_vertex) return refuse(EG3D_NEAREST_ERR_PLY, "the header has no `element vertex`");
  for (int a = 0; a < 3; a++)
    if (at[a] < 0) return refuse(EG3D_NEAREST_ERR_PLY, std::string("`vertex` has no float property ") + (a == 0 ? "x" : a == 1 ? "y" : "z"));

  // ---- body: the count is held against the bytes that are there before anything is allocated
  const size_t left = size - pos;
  const size_t need_each = format == 2 ? stride : 2 * props.size() - 1;  // ASCII: a character per value, one between two
  if (n_vertex && n_vertex > left / need_each) return refuse(EG3D_NEAREST_ERR_PLY, "the body is shorter than the header promises");
  float* X = (float*)malloc(n_vertex ? (size_t)n_vertex * 3 * sizeof(float) : 1);
  if (!X) return refuse(EG3D_NEAREST_ERR_FILE, "out of memory");
  if (format == 2) {
    for (uint64_t i = 0; i < n_vertex; i++)
      for (int a = 0; a < 3; a++) memcpy(&X[3 * i + a], p + pos + (size_t)i * stride + props[at[a]].offset, 4);  // (little-endian hosts)
  } else {
    size_t q = pos;
    for (uint64_t i = 0; i < n_vertex; i++)
      for (size_t k = 0; k < props.size(); k++) {
        while (q < size && is_space(p[q])) q++;
        if (q >= size) {
          free(X);
          return refuse(EG3D_NEAREST_ERR_PLY, "the body is shorter than the header promises");
        }
        size_t e = q;
        while (e < size && !is_space(p[e])) e++;
        for (int a = 0; a < 3; a++)
          if ((int)k == at[a]) {
            char* end = nullptr;
            const double v = strtod(p + q, &end);  // (stops at white space or at the NUL behind the buffer)
            if (end != p + e) {
              free(X);
              return refuse(EG3D_NEAREST_ERR_PLY, "a coordinate that is no number: " + std::string(p + q, e - q));
            }
            X[3 * i + a] = (float)v;
          }
        q = e;
      }
  }
  *X_out = X;
  *n_out = n_vertex;
  return 0;
}
