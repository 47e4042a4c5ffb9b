// eg3d_transform_coordinate_system.hpp — header-only C++ seam that offers the reference's coordinate alignment
// (include/coordinate_system_transform/transform_coordinate_system.hpp) on the types of eg3d_refapi.hpp:
//
//   update_sfmd_from_real_camera_positions(sfmd, cameras_file)   fit to the file's centres, print, transform everything
//   update_sfmd_transform(sfmd, transformation)                  cameras and all points through a given 4 x 4
//
// The reference's CameraType carries rotation, translation, center and intrinsics; the shim's (eg3d_refapi.hpp) carries
// the cameraMatrix alone, which is all the hot path reads. The alignment needs the pose, so these functions take
// PosedSfMData: the shim's SfMData plus one CameraPose per camera. Everything else is the reference's signature. The
// arithmetic is that of include/eg3d_host_transform.h (the fit FP64 and unpinned, everything after it FP32 and pinned to
// the reference's glm); cameraMatrix is rewritten with the other three fields, as the reference does.
//
// With the reference's signatures everything runs on the host (libeg3d_host.so, no GPU); the overloads that take an
// eg3d_ctx* first transform the points on that context's device (eg3d_transform_points, K16). The printed lines are the
// reference's: "Transforming coordinate system ...", the "Ignoring camera" lines, "T:" and the matrix, the camera position
// errors before and after (divided by ALL cameras: DESIGN.md 3, Q16).
//
// Error behaviour: the reference has no error channel and fits to whatever a short or unreadable file leaves in its
// variables. That is not reproduced: an unusable poses file, fewer than 3 posed cameras, coincident centres, a non-finite
// value and a refused device call throw eg3d_ref::Eg3dError with a message.
#pragma once
#include <algorithm>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "eg3d_host_transform.h"
#include "eg3d_refapi.hpp"
#include "eg3d_transform.h"

namespace eg3d_ref {

struct CameraPose {  // the fields of the reference's CameraType the shim's does not hold; [i][j] as glm indexes them
  float rotation[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  float translation[3] = {0, 0, 0};
  float center[3] = {0, 0, 0};
  float intrinsics[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // [0][0] = [1][1] = focal, [0][2], [1][2] = principal point
};
struct PosedSfMData : SfMData {
  std::vector<CameraPose> poses_;  // one per camera, in camera order
};
struct mat4d {  // Eigen::Matrix<double, 4, 4> of the reference's signature, row-major
  double m[16];
};

namespace detail {

inline void cst_check(const PosedSfMData& s) {
  const size_t V = (size_t)std::max(s.numCameras_, 0);
  if (s.poses_.size() < V || s.camerasList_.size() < V || s.points_.size() < (size_t)std::max(s.numPoints_, 0))
    throw Eg3dError(EG3D_ERR_ARG, "update_sfmd_transform: the SfM data arrays are shorter than numCameras_ / numPoints_");
}
inline std::vector<uint8_t> cst_null_mask(const PosedSfMData& s) {
  std::vector<uint8_t> mask((size_t)s.numCameras_);
  for (int v = 0; v < s.numCameras_; v++)
    eg3d_host_null_cameras(1, &s.poses_[(size_t)v].rotation[0][0], s.poses_[(size_t)v].center, &mask[(size_t)v]);
  return mask;
}
inline float cst_error(const PosedSfMData& s, const std::vector<uint8_t>& mask, const std::vector<double>& target) {
  std::vector<float> c;
  for (int v = 0; v < s.numCameras_; v++) c.insert(c.end(), s.poses_[(size_t)v].center, s.poses_[(size_t)v].center + 3);
  float e = 0;
  eg3d_host_camera_errors(s.numCameras_, c.data(), mask.data(), target.data(), &e);
  return e;
}
inline void cst_cameras(PosedSfMData& s, const mat4d& T) {
  for (int v = 0; v < s.numCameras_; v++) {
    CameraPose& p = s.poses_[(size_t)v];
    const float fpp[3] = {p.intrinsics[0][0], p.intrinsics[0][2], p.intrinsics[1][2]};
    // (a null camera is left as it is, its cameraMatrix included)
    const int rc = eg3d_host_transform_cameras(T.m, 1, fpp, &p.rotation[0][0], p.center, p.translation,
                                               &s.camerasList_[(size_t)v].cameraMatrix[0][0]);
    if (rc != 0) throw Eg3dError(rc, "update_sfmd_transform: the transformation holds a value that is not finite");
  }
}
inline void cst_points(eg3d_ctx* ctx, PosedSfMData& s, const mat4d& T) {
  static_assert(sizeof(vec3) == 3 * sizeof(float), "points_ is a flat float array");
  const uint64_t n = (uint64_t)std::max(s.numPoints_, 0);
  if (!n) return;
  float* X = &s.points_[0].x;
  if (!ctx) {
    eg3d_host_transform_points(T.m, X, n, X);
    return;
  }
  std::vector<float> out(3 * (size_t)n);
  const int rc = eg3d_transform_points(ctx, T.m, X, n, out.data(), nullptr);
  if (rc != EG3D_OK) throw Eg3dError(rc, std::string("update_sfmd_transform: ") + eg3d_last_error());
  std::copy(out.begin(), out.end(), X);
}
inline void cst_print(const mat4d& T) {  // `cout << Matrix4d`: coefficients right-aligned to the widest, one space apart
  std::string text[16];
  size_t width = 0;
  for (int k = 0; k < 16; k++) {
    std::ostringstream os;
    os << T.m[k];
    text[k] = os.str();
    width = std::max(width, text[k].size());
  }
  for (int r = 0; r < 4; r++) {
    for (int c = 0; c < 4; c++) std::cout << (c ? " " : "") << std::string(width - text[4 * r + c].size(), ' ') << text[4 * r + c];
    std::cout << std::endl;
  }
}

inline void cst_update(eg3d_ctx* ctx, PosedSfMData& s, const mat4d& T) {
  cst_check(s);
  cst_cameras(s, T);
  cst_points(ctx, s, T);
}
inline void cst_from_file(eg3d_ctx* ctx, PosedSfMData& s, const std::string& cameras_file) {
  cst_check(s);
  const int V = s.numCameras_;
  std::cout << "Transforming coordinate system to adapt it to real camera poses..." << std::endl;
  std::vector<double> target((size_t)V * 3), centres;
  int rc = eg3d_host_read_camera_poses(cameras_file.c_str(), V, target.data());
  if (rc != 0)
    throw Eg3dError(rc, "update_sfmd_from_real_camera_positions: " + cameras_file +
                            (rc == EG3D_TRANSFORM_ERR_SHORT ? " holds fewer than three numbers per camera" : " cannot be read"));
  const std::vector<uint8_t> mask = cst_null_mask(s);
  for (int v = 0; v < V; v++) {
    for (int k = 0; k < 3; k++) centres.push_back((double)s.poses_[(size_t)v].center[k]);
    if (mask[(size_t)v]) std::cout << "Ignoring camera " << v << " in computing the Umeyama transformation" << std::endl;
  }
  mat4d T;
  rc = eg3d_host_similarity_fit(V, centres.data(), target.data(), mask.data(), T.m, nullptr);
  if (rc != 0)
    throw Eg3dError(rc, std::string("update_sfmd_from_real_camera_positions: no fit: ") +
                            (rc == EG3D_TRANSFORM_ERR_FEW          ? "fewer than 3 cameras with a pose"
                             : rc == EG3D_TRANSFORM_ERR_DEGENERATE ? "all camera centres are equal"
                                                                   : "a camera centre is not finite"));
  std::cout << "T:" << std::endl;
  cst_print(T);
  std::cout << "Camera position errors before: " << cst_error(s, mask, target) << std::endl;
  cst_update(ctx, s, T);
  std::cout << "Camera position errors after: " << cst_error(s, mask, target) << std::endl;
}

}  // namespace detail

// transform_coordinate_system.hpp: void update_sfmd_transform(SfMData&, const glm::mat4&) — here the FP64 matrix the fit
// returns; it is converted to FP32 element by element exactly as the reference fills its glm::mat4
inline void update_sfmd_transform(PosedSfMData& sfmd, const mat4d& transformation) { detail::cst_update(nullptr, sfmd, transformation); }
inline void update_sfmd_transform(eg3d_ctx* ctx, PosedSfMData& sfmd, const mat4d& transformation) {
  detail::cst_update(ctx, sfmd, transformation);
}
// transform_coordinate_system.hpp: void update_sfmd_from_real_camera_positions(SfMData&, const std::string&)
inline void update_sfmd_from_real_camera_positions(PosedSfMData& sfmd, const std::string& cameras_file) {
  detail::cst_from_file(nullptr, sfmd, cameras_file);
}
inline void update_sfmd_from_real_camera_positions(eg3d_ctx* ctx, PosedSfMData& sfmd, const std::string& cameras_file) {
  detail::cst_from_file(ctx, sfmd, cameras_file);
}

}  // namespace eg3d_ref
