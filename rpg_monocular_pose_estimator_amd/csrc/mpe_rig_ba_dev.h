// mpe_rig_ba_dev.h — what the host side of mpe_rig_calibrate (mpe_rig.cpp) shares with the steps of mpe_rig_ba.h: the
// sizes of a view's record and the table of pointers every step works on.  Needs include/mpe.h in front; included inside
// namespace mpe (mpe_internal.h) and by the CPU tier.
#pragma once
#define MPE_RIG_BA_MAX_FREE (MPE_RIG_MAX_CAMERAS - 1)
#define MPE_RIG_BA_MAX_N (6 * MPE_RIG_BA_MAX_FREE)
#define MPE_RIG_BA_HEAD 8
#define MPE_RIG_BA_SLOT 99
#define MPE_RIG_BA_TRI (MPE_RIG_BA_MAX_N * (MPE_RIG_BA_MAX_N + 1) / 2)
#define MPE_RIG_BA_CHUNK 64  // views staged per pass of the reduction

// everything the steps read and write (device memory on the GPU, plain memory in the CPU tier)
struct RigBaDev {
  mpe_rig_camera* cams;          // n_cam: K and the CURRENT extrinsics (finish updates the free ones in place)
  const int* cam_free;           // n_cam: index among the free cameras, -1 for the reference camera (held ones bring no row)
  int n_cam, n_free, n_views;    // n_views: the USED views
  const int* view_begin;         // n_views + 1
  const unsigned* view_mask;     // per view: bit i = free camera i has a row in it
  const long long* view_cum;     // n_views + 1: doubles of the records in front of view f
  const int* row_cam;
  const double* row_xyz;
  const double* row_uv;
  double* T_view;                // n_views x 16, updated in place
  double* rec;                   // the records of the views of one chunk
  double* sse;                   // n_views
  double* step;                  // n_views
  double* Sacc;                  // per block (i <= j): accS 36, accV 36
  double* racc;                  // per free camera: acch 6, accz 6
  double* Lf;                    // MPE_RIG_BA_TRI: the factor of S (unit lower triangle, D on the diagonal)
  double* eta;                   // MPE_RIG_BA_MAX_N
  double* cov;                   // n_free x 36
  double* out;                   // [largest |step|, sum of sse]
};

