// facade_wide_tracking.cpp — a recorded sequence through PoseEstimator::estimateBodyPose with setWideFrames(true): the
// tracked branch on frames whose ROI holds 65 .. 256 detections (glare), which the tracker behind the class answers with
// its wide records.
//
//   facade_wide_tracking --markers <yaml> --frames <file.raw> --rows R --cols C --n N --dt s --camera "fx fy cx cy"
//                        [--dist "k1 k2 p1 p2 k3"] [--border b] [--tol t] [--wide 0|1]
//
// Per frame one line "frame k updated U roi x y w h points N rows R", then "frame k pose ..." (16 values, as
// getPredictedPose stores them) and "frame k cov ..." (36) when the pose was updated; "frame k exception <what>" when
// estimateBodyPose threw.  Returns 0 unless the arguments or files are unusable.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "marker_yaml.h"
#include "monocular_pose_estimator_lib/pose_estimator.h"

using namespace monocular_pose_estimator;

int main(int argc, char** argv) {
  const char *markers = 0, *frames = 0;
  int rows = 0, cols = 0, n = 0, wide = 1;
  double cam[4] = {0, 0, 0, 0}, dist[5] = {0, 0, 0, 0, 0}, dt = 0.02, tol = 5, border = 20;
  for (int i = 1; i + 1 < argc; i += 2) {
    if (!std::strcmp(argv[i], "--markers")) markers = argv[i + 1];
    else if (!std::strcmp(argv[i], "--frames")) frames = argv[i + 1];
    else if (!std::strcmp(argv[i], "--rows")) rows = std::atoi(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--cols")) cols = std::atoi(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--n")) n = std::atoi(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--wide")) wide = std::atoi(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--dt")) dt = std::atof(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--tol")) tol = std::atof(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--border")) border = std::atof(argv[i + 1]);
    else if (!std::strcmp(argv[i], "--camera")) std::sscanf(argv[i + 1], "%lf %lf %lf %lf", cam, cam + 1, cam + 2, cam + 3);
    else if (!std::strcmp(argv[i], "--dist")) std::sscanf(argv[i + 1], "%lf %lf %lf %lf %lf", dist, dist + 1, dist + 2, dist + 3, dist + 4);
  }
  List4DPoints pts;
  if (!markers || !frames || rows < 1 || cols < 1 || n < 1 || !read_markers(markers, pts)) return 2;
  std::vector<uint8_t> buf((size_t)n * rows * cols);
  std::FILE* fp = std::fopen(frames, "rb");
  if (!fp || std::fread(buf.data(), 1, buf.size(), fp) != buf.size()) return 2;
  std::fclose(fp);
  try {
    PoseEstimator pe;
    pe.camera_matrix_K_(0, 0) = cam[0];
    pe.camera_matrix_K_(1, 1) = cam[1];
    pe.camera_matrix_K_(0, 2) = cam[2];
    pe.camera_matrix_K_(1, 2) = cam[3];
    pe.camera_matrix_K_(2, 2) = 1.0;
    pe.camera_distortion_coeffs_.assign(dist, dist + 5);
    pe.detection_threshold_value_ = 140;  // demo.launch
    pe.gaussian_sigma_ = 0.6;
    pe.min_blob_area_ = 10;
    pe.max_blob_area_ = 200;
    pe.max_width_height_distortion_ = 0.5;
    pe.max_circular_distortion_ = 0.5;
    pe.roi_border_thickness_ = (unsigned)border;
    pe.setBackProjectionPixelTolerance(tol);
    pe.setNearestNeighbourPixelTolerance(7);
    pe.setCertaintyThreshold(0.75);
    pe.setValidCorrespondenceThreshold(0.7);
    pe.setMarkerPositions(pts);
    pe.setWideFrames(wide != 0);
    for (int k = 0; k < n; ++k) {
      const ImageView img(buf.data() + (size_t)k * rows * cols, rows, cols, (size_t)cols);
      try {
        const bool ok = pe.estimateBodyPose(img, k * dt);
        const Rect r = pe.getRegionOfInterest();
        std::printf("frame %d updated %d roi %d %d %d %d points %d rows %d\n", k, (int)ok, r.x, r.y, r.width, r.height,
                    (int)pe.getImagePoints().size(), (int)pe.getCorrespondences().size());
        if (!ok) continue;
        std::printf("frame %d pose", k);
        const Matrix4d T = pe.getPredictedPose();
        for (int i = 0; i < 16; ++i) std::printf(" %.17g", T(i));
        std::printf("\nframe %d cov", k);
        const Matrix6d C = pe.getPoseCovariance();
        for (int i = 0; i < 36; ++i) std::printf(" %.17g", C(i));
        std::printf("\n");
      } catch (const std::exception& e) {
        std::printf("frame %d exception %s\n", k, e.what());
      }
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
  return 0;
}
