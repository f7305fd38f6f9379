// mpe_body_ba_dev.h — what the host side of mpe_body_calibrate (mpe_body.cpp) shares with the steps of mpe_body_ba.h:
// the sizes of a view's record and the table of pointers every step works on.  Needs include/mpe.h in front; included
// inside namespace mpe (mpe_internal.h) and by the CPU tier.
#pragma once
#define MPE_BODY_BA_MAX_N (3 * MPE_MAX_MARKERS)
#define MPE_BODY_BA_HEAD 8
#define MPE_BODY_BA_SLOT 45  // W 18 | Y 18 | V 6 | h 3
#define MPE_BODY_BA_TRI (MPE_BODY_BA_MAX_N * (MPE_BODY_BA_MAX_N + 1) / 2)
#define MPE_BODY_BA_MAX_GAUGE 7
// what solve leaves for the covariance: [w | number of constraints | sum |d|^2 | the rotations' 3 x 3 block of N^T N (9)
// | n7 . u | pad to 16] then N, one row of MPE_BODY_BA_MAX_N per constraint, then u = M^-1 n7 (n7 the scale column)
#define MPE_BODY_BA_GAUGE (16 + (MPE_BODY_BA_MAX_GAUGE + 1) * MPE_BODY_BA_MAX_N)

// everything the steps read and write (device memory on the GPU, plain memory in the CPU tier)
struct BodyBaDev {
  const mpe_rig_camera* cams;    // n_cam: K and the extrinsics (fixed)
  const int* free_marker;        // n_free: the caller's index of free marker i (held markers bring no row)
  int n_cam, n_free, n_views;    // n_views: the USED views
  int scale_held;                // 1: the seventh constraint
  const int* view_begin;         // n_views + 1
  const unsigned* view_mask;     // per view: bit i = free marker i has a row in it
  const long long* view_cum;     // n_views + 1: doubles of the records in front of view f
  const int* row_cam;
  const int* row_free;           // per row: index of its marker among the free ones
  const double* row_uv;
  double* markers;               // n_markers x 3: the CURRENT positions (finish updates the free ones in place)
  double* T_view;                // n_views x 16, updated in place
  double* rec;                   // the records of the views of one chunk
  double* sse;                   // n_views
  double* step;                  // n_views
  double* Sacc;                  // per block (i <= j): accS 9, accV 9
  double* racc;                  // per free marker: acch 3, accz 3
  double* Lf;                    // MPE_BODY_BA_TRI: the factor of M (unit lower triangle, D on the diagonal)
  double* delta;                 // MPE_BODY_BA_MAX_N
  double* gauge;                 // MPE_BODY_BA_GAUGE
  double* cov;                   // n_free x 9
  double* out;                   // [largest |step|, sum of sse]
};
