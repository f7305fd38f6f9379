// mpe_rig_init.h — the logic of k_rig_init_vote / k_rig_init_winner / k_rig_init_finish (mpe_k3.hip): a body FOUND with the
// whole rig when no camera sees four LEDs.  initialise() (pose_estimator.cpp:544-702) takes a P3P hypothesis from every
// detection triple x marker permutation of ONE camera and scores it by reprojection in that camera; here the hypotheses
// come from every camera with at least three detections and are scored in ALL cameras, by steps 1 - 3 of the tracking
// step (mpe_rig_track.h: project, nearest detection within the tolerance, one marker per detection).  The acceptance
// rule is the project's own (include/mpe.h states it): the reference validates inside one camera that sees four LEDs,
// and such a camera does not exist here.
//
//   item        = off[c] + rank(detection triple i < j < k of camera c) * P(n_mk, 3) + rank(ordered marker triple), the
//                 cameras in ascending order, a camera with fewer than three detections has no item
//   hypothesis  h = 4 * item + root: bearings as calculateImageVectors, p3p_prepare (plain quartic) / p3p_solution, counted
//                 when rc_finite; T_h = E_c^-1 [R^T | -R^T C], both rigid inverses in closed form
//   score       the row set W_h at T_h with the vote tolerance, rows_h = |W_h|, s2_h = the kept squared distances summed in
//                 ascending (camera, marker) order
//   winner      the least key (rows descending, s2 ascending, h ascending): a total order, so no launch shape shows
//   runner-up   the most rows among the hypotheses that contradict the winner: some (c, m) has a row in W_h that is not
//                 the winner's
//
// The form: one item per lane.  What a lane scores with — the rig's cameras with their inverse extrinsics, the markers,
// the problem's detection lists, the vote tolerances — is staged once per block in LDS (RigInitLds), and so are the two
// tables a lane needs per camera (squared distance and slot per marker: indexed by marker at run time, they would be
// scratch memory as per-lane arrays), marker-major so that the lanes of a wave hit different banks.  A lane scores camera
// after camera, so the tables hold one camera.  39.4 KB: four blocks of 128 lanes on a compute unit.  Nothing is summed
// across lanes; blocks hand out one key (or one row count) each and a later launch reduces them in index order.
//
// No #include and no namespace of its own: the text goes behind mpe_rig_track.h inside namespace mpe and needs mpe_p3p.h
// and mpe_k2_head.h's unrank_combo3 / bearing / pick_root in front.
#define MPE_RIG_INIT_LANES 128
#define MPE_RIG_INIT_ITEMS_PER_LANE 1  // (4: a single problem 0.64 instead of 0.24 ms, 4 096 problems 2 % faster: profiles/rig_init*.jsonl)
#define MPE_RIG_INIT_CHUNK (MPE_RIG_INIT_LANES * MPE_RIG_INIT_ITEMS_PER_LANE)  // items per block
#define MPE_RIG_INIT_MAX_ITEMS (1 << 22)

struct RigInitKey {
  double s2;
  int rows;
  int h;  // < 0: no hypothesis
};
__device__ __forceinline__ RigInitKey rig_init_no_key() { return RigInitKey{0.0, -1, -1}; }
// a comes in front of b
__device__ __forceinline__ bool rig_init_better(const RigInitKey& a, const RigInitKey& b) {
  if (a.h < 0 || b.h < 0) return b.h < 0 && a.h >= 0;
  if (a.rows != b.rows) return a.rows > b.rows;
  if (a.s2 != b.s2) return a.s2 < b.s2;
  return a.h < b.h;
}

struct RigInitCam {
  double fx, fy, cx, cy;
  double R[3][3], t[3];  // E_c
  double Ei[3][4];       // E_c^-1 = [R^T | -R^T t]
};

struct RigInitLds {
  RigInitCam cam[MPE_RIG_MAX_CAMERAS];
  double mk[MPE_MAX_MARKERS][3];
  double tol[MPE_RIG_MAX_CAMERAS];
  double det[MPE_RIG_MAX_CAMERAS * MPE_MAX_DETECTIONS][2];  // the lists one behind the other, each cut at MPE_MAX_DETECTIONS
  double d2[MPE_MAX_MARKERS][MPE_RIG_INIT_LANES];           // per lane, one camera: squared distance of a marker
  unsigned char slot[MPE_MAX_MARKERS][MPE_RIG_INIT_LANES];  // ... and its detection, 1-based, 0 none
  unsigned char win[MPE_RIG_MAX_ROWS];                      // the winner's row set (runner-up pass)
  int beg[MPE_RIG_MAX_CAMERAS + 1];                         // list c = det[beg[c] .. beg[c + 1])
  int off[MPE_RIG_MAX_CAMERAS + 1];                         // camera c's items = [off[c], off[c + 1])
};

// items of a camera with n detections: C(n, 3) * P(n_mk, 3) (fits 32 bits: 41 664 * 3 360)
__device__ __forceinline__ int rig_init_camera_items(int n, int n_mk) {
  if (n < 3 || n_mk < 3) return 0;
  return (n * (n - 1) * (n - 2) / 6) * (n_mk * (n_mk - 1) * (n_mk - 2));
}

// Lane ln of n_lanes brings one problem into S (followed by a barrier on the device).  win: the winner's row set or null.
__device__ __forceinline__ void rig_init_stage(RigInitLds& S, int ln, int n_lanes, const mpe_rig_camera* cams, int n_cam,
                                               const double* markers, int n_mk, const int* det_begin, const double* det_xy,
                                               const double* tol, const unsigned char* win) {
  for (int c = ln; c < n_cam; c += n_lanes) {
    RigInitCam& o = S.cam[c];
    o.fx = cams[c].K[0];
    o.fy = cams[c].K[4];
    o.cx = cams[c].K[2];
    o.cy = cams[c].K[5];
    const double* E = cams[c].T_cam_rig;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) {
        o.R[i][j] = E[4 * i + j];
        o.Ei[i][j] = E[4 * j + i];
      }
      o.t[i] = E[4 * i + 3];
      o.Ei[i][3] = -(E[i] * E[3] + E[4 + i] * E[7] + E[8 + i] * E[11]);
    }
    S.tol[c] = tol[c];
  }
  for (int m = ln; m < n_mk; m += n_lanes) {
    S.mk[m][0] = markers[3 * m];
    S.mk[m][1] = markers[3 * m + 1];
    S.mk[m][2] = markers[3 * m + 2];
  }
  int base = 0, items = 0;
  for (int c = 0; c < n_cam; ++c) {
    const int b = det_begin[c];
    const int nd = det_begin[c + 1] - b < MPE_MAX_DETECTIONS ? det_begin[c + 1] - b : MPE_MAX_DETECTIONS;
    for (int j = ln; j < nd; j += n_lanes) {
      S.det[base + j][0] = det_xy[2 * (size_t)(b + j)];
      S.det[base + j][1] = det_xy[2 * (size_t)(b + j) + 1];
    }
    if (ln == 0) {
      S.beg[c] = base;
      S.off[c] = items;
    }
    base += nd > 0 ? nd : 0;
    items += rig_init_camera_items(nd, n_mk);
  }
  if (ln == 0) {
    S.beg[n_cam] = base;
    S.off[n_cam] = items;
  }
  for (int p = ln; p < MPE_RIG_MAX_ROWS; p += n_lanes) S.win[p] = (win && p < n_cam * n_mk) ? win[p] : 0;
}

struct RigInitItem {
  int cam, d[3], m[3];
};
// item -> its camera, detection triple (0-based within the list) and marker triple
__device__ __forceinline__ void rig_init_decode(const RigInitLds& S, int n_mk, int item, RigInitItem& it) {
  int c = 0;
  while (item >= S.off[c + 1]) ++c;
  const int rel = item - S.off[c];
  const int n1 = n_mk - 1, n2 = n_mk - 2, P = n_mk * n1 * n2;
  const int ci = rel / P, pj = rel - ci * P;
  it.cam = c;
  unrank_combo3(ci, S.beg[c + 1] - S.beg[c], it.d[0], it.d[1], it.d[2]);
  // the pj-th ordered triple of distinct markers, lexicographic
  const int p0 = pj / (n1 * n2), r1 = pj - p0 * (n1 * n2);
  const int i1 = r1 / n2, i2 = r1 - i1 * n2;
  const int p1 = i1 + (i1 >= p0 ? 1 : 0);
  const int lo = p0 < p1 ? p0 : p1, hi = p0 < p1 ? p1 : p0;
  int p2 = i2;
  p2 += p2 >= lo ? 1 : 0;
  p2 += p2 >= hi ? 1 : 0;
  it.m[0] = p0;
  it.m[1] = p1;
  it.m[2] = p2;
}

// the item's P3P up to the roots -> false: the marker triple is collinear, no hypothesis
__device__ __forceinline__ bool rig_init_prepare(const RigInitLds& S, const RigInitItem& it, P3PCtx& ctx) {
  const RigInitCam& C = S.cam[it.cam];
  const double(*d)[2] = S.det + S.beg[it.cam];
  const V3 fa = bearing(d[it.d[0]][0], d[it.d[0]][1], C.fx, C.fy, C.cx, C.cy),
           fb = bearing(d[it.d[1]][0], d[it.d[1]][1], C.fx, C.fy, C.cx, C.cy),
           fc = bearing(d[it.d[2]][0], d[it.d[2]][1], C.fx, C.fy, C.cx, C.cy);
  const V3 wa = {S.mk[it.m[0]][0], S.mk[it.m[0]][1], S.mk[it.m[0]][2]},
           wb = {S.mk[it.m[1]][0], S.mk[it.m[1]][1], S.mk[it.m[1]][2]},
           wc = {S.mk[it.m[2]][0], S.mk[it.m[2]][1], S.mk[it.m[2]][2]};
  return p3p_prepare(fa, fb, fc, wa, wb, wc, ctx, false);
}

// root -> T = E_c^-1 [R^T | -R^T C] (rig <- marker frame); false: not finite, no hypothesis
__device__ __forceinline__ bool rig_init_pose(const RigInitLds& S, int cam, const P3PCtx& ctx, int root, T34& T) {
  M3 R;
  V3 Cc;
  p3p_solution(ctx, pick_root(ctx, root), R, Cc);
  if (!rc_finite(R, Cc)) return false;
  const M3 Ri = transpose(R);
  const V3 ti = mul(Ri, Cc);
  const double Pm[3][4] = {{Ri.r0.x, Ri.r0.y, Ri.r0.z, -ti.x}, {Ri.r1.x, Ri.r1.y, Ri.r1.z, -ti.y}, {Ri.r2.x, Ri.r2.y, Ri.r2.z, -ti.z}};
  const RigInitCam& C = S.cam[cam];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double s = C.Ei[i][0] * Pm[0][j] + C.Ei[i][1] * Pm[1][j] + C.Ei[i][2] * Pm[2][j];
      T.m[i][j] = j == 3 ? s + C.Ei[i][3] : s;
    }
  }
  return true;
}

// The row set at T with the vote tolerances: steps 1 - 3 of rig_track (mpe_rig_track.h), statement by statement, camera
// after camera through lane ln's columns of S.d2 / S.slot.  -> rows, s2 (ascending (camera, marker) order), contra: a row
// that is not S.win's; W (optional): the row set, n_cam * n_mk bytes.
__device__ __forceinline__ void rig_init_score(RigInitLds& S, int ln, int n_cam, int n_mk, const T34& T, int& rows, double& s2,
                                               bool& contra, unsigned char* W) {
  rows = 0;
  s2 = 0.0;
  contra = false;
  for (int c = 0; c < n_cam; ++c) {
    const RigInitCam& C = S.cam[c];
    const double(*det)[2] = S.det + S.beg[c];
    const int nd = S.beg[c + 1] - S.beg[c];
    if (nd == 0) {  // (no detection, no row: what the steps below give)
      for (int m = 0; m < n_mk; ++m) {
        if (W) W[c * n_mk + m] = 0;
      }
      continue;
    }
    const double tol = S.tol[c];
    for (int m = 0; m < n_mk; ++m) {
      const double* pm = S.mk[m];
      unsigned char s = 0;
      double best = 0.0;
      const double X = T.m[0][0] * pm[0] + T.m[0][1] * pm[1] + T.m[0][2] * pm[2] + T.m[0][3];
      const double Y = T.m[1][0] * pm[0] + T.m[1][1] * pm[1] + T.m[1][2] * pm[2] + T.m[1][3];
      const double Z = T.m[2][0] * pm[0] + T.m[2][1] * pm[1] + T.m[2][2] * pm[2] + T.m[2][3];
      const double x = C.R[0][0] * X + C.R[0][1] * Y + C.R[0][2] * Z + C.t[0];
      const double y = C.R[1][0] * X + C.R[1][1] * Y + C.R[1][2] * Z + C.t[1];
      const double z = C.R[2][0] * X + C.R[2][1] * Y + C.R[2][2] * Z + C.t[2];
      const double u = (C.fx * x + C.cx * z) / z;
      const double v = (C.fy * y + C.cy * z) / z;
      const bool visible = z > 0 && fabs(u) <= 1.7976931348623157e308 && fabs(v) <= 1.7976931348623157e308;
      if (visible) {
        best = __builtin_inf();
        for (int j = 0; j < nd; ++j) {
          const double du = u - det[j][0], dv = v - det[j][1];
          const double dd = du * du + dv * dv;
          if (dd < best) {
            best = dd;
            s = (unsigned char)(j + 1);
          }
        }
        if (!(sqrt(best) <= tol)) s = 0;
      }
      S.slot[m][ln] = s;
      S.d2[m][ln] = best;
    }
    for (int m = 0; m < n_mk; ++m) {
      unsigned char s = S.slot[m][ln];
      const double mine = S.d2[m][ln];
      if (s != 0) {
        for (int k = 0; k < n_mk; ++k) {
          const double other = S.d2[k][ln];
          if (k != m && S.slot[k][ln] == S.slot[m][ln] && (other < mine || (other == mine && k < m))) s = 0;
        }
      }
      if (s != 0) {
        ++rows;
        s2 += mine;
        contra = contra || s != S.win[c * n_mk + m];
      }
      if (W) W[c * n_mk + m] = s;
    }
  }
}

// One lane's item.  mode 0: key <- the better of key and the item's hypotheses; mode 1: runner <- the larger of runner and
// the rows of those that contradict S.win.
__device__ __forceinline__ void rig_init_item(RigInitLds& S, int ln, int n_cam, int n_mk, int item, int mode, RigInitKey& key,
                                              int& runner) {
  RigInitItem it;
  rig_init_decode(S, n_mk, item, it);
  P3PCtx ctx;
  if (!rig_init_prepare(S, it, ctx)) return;
  for (int root = 0; root < 4; ++root) {
    T34 T;
    if (!rig_init_pose(S, it.cam, ctx, root, T)) continue;
    int rows;
    double s2;
    bool contra;
    rig_init_score(S, ln, n_cam, n_mk, T, rows, s2, contra, nullptr);
    if (mode == 0) {
      const RigInitKey k = {s2, rows, 4 * item + root};
      if (rig_init_better(k, key)) key = k;
    } else if (contra && rows > runner) {
      runner = rows;
    }
  }
}

// The winner again, on ONE lane (ln's table columns), for everything the other launches need of it: its row set -> W
// (n_cam * n_mk bytes) and the head of the info record.  S staged with win = null.
__device__ __forceinline__ void rig_init_winner(RigInitLds& S, int ln, int n_cam, int n_mk, const RigInitKey& key,
                                                unsigned char* W, mpe_rig_init_info* info) {
  info->reason = 6;
  info->camera = -1;
  for (int k = 0; k < 3; ++k) info->detection[k] = info->marker[k] = -1;
  info->root = -1;
  info->best_rows = info->runner_rows = info->best_markers = 0;
  info->n_items = S.off[n_cam];
  info->best_sum2 = 0.0;
  for (int i = 0; i < 16; ++i) info->T_hyp[i] = (i % 5 == 0) ? 1.0 : 0.0;
  for (int p = 0; p < n_cam * n_mk; ++p) W[p] = 0;
  if (key.h < 0) return;
  RigInitItem it;
  rig_init_decode(S, n_mk, key.h >> 2, it);
  P3PCtx ctx;
  T34 T;
  if (!rig_init_prepare(S, it, ctx) || !rig_init_pose(S, it.cam, ctx, key.h & 3, T)) return;  // (cannot be: it was counted)
  int rows;
  double s2;
  bool contra;
  rig_init_score(S, ln, n_cam, n_mk, T, rows, s2, contra, W);
  unsigned seen = 0;
  for (int p = 0; p < n_cam * n_mk; ++p)
    if (W[p] != 0) seen |= 1u << (p % n_mk);
  int distinct = 0;
  for (int k = 0; k < MPE_MAX_MARKERS; ++k) distinct += (int)((seen >> k) & 1u);
  info->reason = 0;
  info->camera = it.cam;
  for (int k = 0; k < 3; ++k) {
    info->detection[k] = it.d[k];
    info->marker[k] = it.m[k];
  }
  info->root = key.h & 3;
  info->best_rows = rows;
  info->best_markers = distinct;
  info->best_sum2 = s2;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) info->T_hyp[4 * i + j] = T.m[i][j];
}

// 6 no hypothesis, 1 too few rows, 2 too few markers, 5 ambiguous, 0 go on to the tracking rounds
__device__ __forceinline__ int rig_init_decide(const mpe_rig_init_info& w, int runner, int min_rows, int min_markers,
                                               int min_margin) {
  if (w.camera < 0) return 6;
  if (w.best_rows < min_rows) return 1;
  if (w.best_markers < min_markers) return 2;
  if (w.best_rows - runner < min_margin) return 5;
  return 0;
}

// One problem on one wave of MPE_RIG_LANES lanes, behind the winner and the runner-up: the decision, then the tracking
// rounds of rig_track from T_pred = info->T_hyp with match tolerance = vote tolerance.  W: the winner's row set.  A record
// without a pose has T = I and cov = 0.
__device__ __forceinline__ void rig_init_finish(RigTrackLds& S, const mpe_rig_camera* cams, int n_cam, const double* markers,
                                                int n_mk, const int* det_begin, const double* det_xy, const double* tol_vote,
                                                const double* tol_accept, const unsigned char* W, int runner, int max_rounds,
                                                int min_rows, int min_markers, int min_margin, mpe_result* res, uint32_t* match,
                                                mpe_rig_init_info* info) {
  const int early = rig_init_decide(*info, runner, min_rows, min_markers, min_margin);
  int reason = early;
  if (early == 0) {
    rig_track(S, cams, n_cam, markers, n_mk, det_begin, det_xy, tol_vote, tol_accept, info->T_hyp, max_rounds, min_rows,
              min_markers, res, match, &info->track);
    reason = info->track.reason;
  }
  unsigned cams_seen = 0;
  int n_seen = 0;
  for (int p = 0; p < n_cam * n_mk; ++p)
    if (W[p] != 0 && !(cams_seen & (1u << (p / n_mk)))) {
      cams_seen |= 1u << (p / n_mk);
      ++n_seen;
    }
  RIG_EACH_LANE(l) {
    if (early != 0) {
      for (int p = l; p < n_cam * n_mk; p += MPE_RIG_LANES) match[p] = W[p];
      if (l < 36) res->cov[l] = 0.0;
      if (l == 0) {
        res->status = MPE_FRAME_NO_POSE;
        res->n_det = n_seen;
        res->n_corr = info->best_rows;
        res->gn_iterations = 0;
        info->track.rounds = info->track.rows = info->track.distinct_markers = info->track.reason = 0;
        info->track.max_residual = info->track.rms = 0.0;
      }
    }
    if (reason != 0 && l < 16) res->T[l] = (l % 5 == 0) ? 1.0 : 0.0;
    if (l == 0) {
      info->reason = reason;
      info->runner_rows = runner;
    }
  }
}
