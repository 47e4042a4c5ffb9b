// eg3d_point_cloud.hpp — header-only C++ seam that offers the reference's point-cloud writers on the types of
// eg3d_refapi.hpp (include/edgegraph3d/io/output/output_point_cloud.hpp), name for name:
//
//   output_point_cloud(sfmd, file)                                        white points
//   output_point_cloud(sfmd, folder, name)
//   output_point_cloud(sfmd, inliers, folder, name)                       only the inliers
//   output_colored_point_cloud(sfmd, images_folder, file)                 coloured from the source images
//   output_colored_point_cloud(sfmd, images_folder, folder, name)
//   output_colored_point_cloud(sfmd, images_folder, inliers, folder, name)
//
// The bytes are those of eg3d_host_write_ply (include/eg3d_host_colour.h); the colours are those of include/eg3d_colour.h.
// With the reference's signatures the colours come from the host statement (libeg3d_host.so, no GPU); the overloads that
// take an eg3d_ctx* first colour on that context's device (eg3d_upload_images + eg3d_colour_points; the context keeps the
// images afterwards). Images are found as the reference finds them — images_folder + the base name of camerasPaths_[v],
// no separator added — and read with eg3d_host_png_read_rgb: PNG only, JPEG is not read.
//
// Error behaviour: the reference's writers have no error channel, and its image loader CONSTRUCTS an exception for an
// unreadable image without throwing it. That is not reproduced: a missing or unreadable image, a file that cannot be
// written and a refused cloud throw eg3d_ref::Eg3dError with a message. The *_highlight writers are not offered.
#pragma once
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "eg3d_colour.h"
#include "eg3d_host_colour.h"
#include "eg3d_refapi.hpp"

namespace eg3d_ref {
namespace detail {

inline std::string opc_base_name(const std::string& s) {  // (npos + 1 == 0: a name without a separator stays whole)
  return s.substr(s.find_last_of("/\\") + 1);
}

struct OpcImages {
  std::vector<int32_t> w, h;
  std::vector<const uint8_t*> rgb;
  std::vector<std::unique_ptr<uint8_t, void (*)(void*)>> own;
};
inline OpcImages opc_read_images(const char* images_folder, const SfMData& sfmd) {
  OpcImages im;
  for (const std::string& s : sfmd.camerasPaths_) {
    const std::string path = std::string(images_folder) + opc_base_name(s);
    int w = 0, h = 0;
    uint8_t* p = nullptr;
    const int rc = eg3d_host_png_read_rgb(path.c_str(), &w, &h, &p);
    if (rc != 0) throw Eg3dError(rc, "output_colored_point_cloud: cannot read " + path + " as a PNG image (code " + std::to_string(rc) + ")");
    im.own.emplace_back(p, eg3d_host_free);
    im.w.push_back(w);
    im.h.push_back(h);
    im.rgb.push_back(p);
  }
  return im;
}

struct OpcCloud {
  std::vector<float> X;
  std::vector<uint32_t> off;
  std::vector<int32_t> view;
  std::vector<float> xy;
  std::vector<uint8_t> keep;
};
inline OpcCloud opc_cloud(const SfMData& sfmd, const std::vector<bool>* inliers) {
  OpcCloud c;
  const size_t n = (size_t)sfmd.numPoints_;
  if (sfmd.points_.size() < n || sfmd.camViewingPointN_.size() < n || sfmd.point2DoncamViewingPoint_.size() < n ||
      (inliers && inliers->size() < n))
    throw Eg3dError(EG3D_ERR_ARG, "output_point_cloud: the SfMData arrays are shorter than numPoints_");
  c.off.push_back(0);
  for (size_t i = 0; i < n; i++) {
    c.X.insert(c.X.end(), {sfmd.points_[i].x, sfmd.points_[i].y, sfmd.points_[i].z});
    const std::vector<int>& cams = sfmd.camViewingPointN_[i];
    const std::vector<vec2>& at = sfmd.point2DoncamViewingPoint_[i];
    if (at.size() < cams.size()) throw Eg3dError(EG3D_ERR_ARG, "output_point_cloud: a point has fewer 2-D positions than cameras");
    for (size_t k = 0; k < cams.size(); k++) {
      c.view.push_back(cams[k]);
      c.xy.push_back(at[k].x);
      c.xy.push_back(at[k].y);
    }
    if (c.view.size() > 0xffffffffull) throw Eg3dError(EG3D_ERR_CAPACITY, "output_point_cloud: more than 2^32 observations");
    c.off.push_back((uint32_t)c.view.size());
    if (inliers) c.keep.push_back((*inliers)[i] ? 1 : 0);
  }
  return c;
}

inline void opc_write(const std::string& file, const OpcCloud& c, const uint8_t* rgb) {
  const int rc = eg3d_host_write_ply(file.c_str(), c.off.size() - 1, c.X.data(), rgb, c.keep.empty() ? nullptr : c.keep.data());
  if (rc != 0) throw Eg3dError(rc, "output_point_cloud: cannot write " + file);
}

// ctx == nullptr: the host statement
inline void opc_coloured(eg3d_ctx* ctx, const SfMData& sfmd, const char* images_folder, const std::vector<bool>* inliers,
                         const std::string& file) {
  const OpcCloud c = opc_cloud(sfmd, inliers);
  const OpcImages im = opc_read_images(images_folder, sfmd);
  const uint64_t n = c.off.size() - 1;
  std::vector<uint8_t> rgb(3 * n + 1);
  const uint8_t* keep = c.keep.empty() ? nullptr : c.keep.data();
  if (ctx) {
    int rc = eg3d_upload_images(ctx, (int)im.rgb.size(), im.w.data(), im.h.data(), im.rgb.data());
    if (rc == EG3D_OK) rc = eg3d_colour_points(ctx, n, c.off.data(), c.view.data(), c.xy.data(), keep, rgb.data(), nullptr, nullptr);
    if (rc != EG3D_OK) throw Eg3dError(rc, std::string("output_colored_point_cloud: ") + eg3d_last_error());
  } else if (eg3d_host_colour_points((int)im.rgb.size(), im.w.data(), im.h.data(), im.rgb.data(), n, c.off.data(), c.view.data(),
                                     c.xy.data(), keep, 0, rgb.data(), nullptr, nullptr) != 0) {
    throw Eg3dError(EG3D_ERR_ARG, "output_colored_point_cloud: the cloud is refused (a view without an image, a view id outside "
                                  "the cameras, a position that is not finite or not below 1e7, or more than 32 767 observations)");
  }
  opc_write(file, c, rgb.data());
}

}  // namespace detail

inline void output_point_cloud(const SfMData& sfmd, const char* output_file) {
  detail::opc_write(output_file, detail::opc_cloud(sfmd, nullptr), nullptr);
}
inline void output_point_cloud(const SfMData& sfmd, const char* out_folder, const std::string& output_filename) {
  output_point_cloud(sfmd, (std::string(out_folder) + output_filename).c_str());
}
inline void output_point_cloud(const SfMData& sfmd, const std::vector<bool>& inliers, const char* out_folder,
                               const std::string& output_filename) {
  detail::opc_write(std::string(out_folder) + output_filename, detail::opc_cloud(sfmd, &inliers), nullptr);
}

inline void output_colored_point_cloud(const SfMData& sfmd, const char* images_folder, const char* output_file) {
  detail::opc_coloured(nullptr, sfmd, images_folder, nullptr, output_file);
}
inline void output_colored_point_cloud(const SfMData& sfmd, const char* images_folder, const char* out_folder,
                                       const std::string& output_filename) {
  detail::opc_coloured(nullptr, sfmd, images_folder, nullptr, std::string(out_folder) + output_filename);
}
inline void output_colored_point_cloud(const SfMData& sfmd, const char* images_folder, const std::vector<bool>& inliers,
                                       const char* out_folder, const std::string& output_filename) {
  detail::opc_coloured(nullptr, sfmd, images_folder, &inliers, std::string(out_folder) + output_filename);
}

// ... and on the device of `ctx`, whose rig must be the SfMData's cameras
inline void output_colored_point_cloud(eg3d_ctx* ctx, const SfMData& sfmd, const char* images_folder, const char* output_file) {
  detail::opc_coloured(ctx, sfmd, images_folder, nullptr, output_file);
}
inline void output_colored_point_cloud(eg3d_ctx* ctx, const SfMData& sfmd, const char* images_folder, const std::vector<bool>& inliers,
                                       const char* out_folder, const std::string& output_filename) {
  detail::opc_coloured(ctx, sfmd, images_folder, &inliers, std::string(out_folder) + output_filename);
}

}  // namespace eg3d_ref
