// gn_cam.hpp -- the pinhole intrinsics as the pose-only Gauss-Newton rows read them (pose_gn_dev.hpp) and as the loop-closure
// check's argument record carries them (lc_plan.hpp).  No HIP header: the host planner and its CPU test compile this.
#pragma once

namespace plslam {

struct GnCam { double fx, fy, cx, cy; };

}  // namespace plslam
