// mpe_rig_track.h — the logic of k_rig_track (mpe_k3.hip): one time step of a rig that tracks ONE body whose LEDs are
// spread over the cameras — a camera that sees two or three of them counts.  From a predicted pose T_pred (rig <- marker
// frame) the markers are projected into every camera, every camera's detections are matched to them by the rule of the
// tracking branch (findCorrespondences, pose_estimator.cpp:372-392: nearest detection, du*du + dv*dv, strict <, first
// minimum wins, kept when sqrt(best) <= tolerance), ONE pose is refined over all rows (rig_gn_iterate, mpe_rig_gn.h) and
// the pose is believed when every row's residual is within the camera's accept tolerance.  The reference validates a
// camera's rows with a P3P triple inside that camera (checkCorrespondences); a camera with two rows has none, so the
// acceptance rule here is the project's own.
//
// Round r = 0, 1, .. from pose T_r (T_0 = T_pred):
//   1 project   pair (camera c, marker m) = p, p = c * n_markers + m, lanes take p = l, l + 64, ..: q = E_c T_r p_m and
//               (u, v) in rig_row's arithmetic; visible when q_z > 0 and u, v finite
//   2 match     the nearest detection of camera c within tol_c (match tolerance in round 0, accept tolerance later)
//   3 unique    of several markers of a camera on one detection the smallest squared distance keeps it, a tie goes to
//               the lowest marker; the others get no row (no second-nearest search)
//   4 rows      in ascending (camera, marker) order; fewer than min_rows: NO_POSE reason 1; fewer than min_markers
//               distinct markers: reason 2
//   5 stable    r > 0 and the row set is the previous round's: stop, the result is the previous refinement
//   6 refine    rig_gn_iterate from T_r -> T_{r+1}; a non-finite pose: reason 3; stop when r + 1 == max_rounds
// accept: at the final pose every final row's residual length <= its camera's accept tolerance, else reason 4.
// Every NO_POSE hands back T_pred and a zero covariance; the info record carries what was computed all the same.
//
// The form is mpe_rig_gn.h's: one 64-lane wave per problem, phases written RIG_EACH_LANE(l) { .. }, what crosses a phase
// in LDS (RigTrackLds = RigGnLds + 4.5 KB: the markers, the tolerances, a squared distance and two match slots per pair),
// what is wave-uniform read from LDS between phases.  The detection lists stay in global memory (a list is read by the
// <= 16 pairs of its camera).  No atomics, every sum and every prefix count in a fixed order.
//
// No #include and no namespace of its own: the text goes behind mpe_rig_gn.h inside namespace mpe.
#define MPE_RIG_TRACK_CHUNK (MPE_RIG_MAX_ROWS / MPE_RIG_LANES)  // consecutive pairs per lane when the rows are counted

struct RigTrackLds {
  RigGnLds G;
  double mk[MPE_MAX_MARKERS][3];
  double tol_match[MPE_RIG_MAX_CAMERAS], tol_accept[MPE_RIG_MAX_CAMERAS];
  double d2[MPE_RIG_MAX_ROWS];           // per pair: squared distance to its nearest detection; at the end per ROW: residual^2
  unsigned char slot[MPE_RIG_MAX_ROWS];  // per pair: its detection (1-based within the camera's list), 0 none
  unsigned char keep[MPE_RIG_MAX_ROWS];  // per pair: slot behind the uniqueness rule = the row set of this round
  unsigned char prev[MPE_RIG_MAX_ROWS];  // the row set of the round before
  unsigned char cnt[MPE_RIG_LANES];      // per lane: rows among its MPE_RIG_TRACK_CHUNK pairs
  unsigned char dif[MPE_RIG_LANES];      // per lane: one of its pairs differs from the round before
  unsigned short mseen[MPE_RIG_LANES];   // per lane: the markers of its rows
};

// One problem on one wave.  cams: the rig's n_cam cameras (1 .. 16); markers: n_mk x 3 (1 .. 16); det_begin: n_cam + 1
// offsets into det_xy (pairs of doubles), a list of at most MPE_MAX_DETECTIONS points (the caller has checked all of
// these); T_pred: 16 doubles.  Writes res, match (n_cam * n_mk words) and info.
__device__ __forceinline__ void rig_track(RigTrackLds& S, const mpe_rig_camera* cams, int n_cam, const double* markers,
                                          int n_mk, const int* det_begin, const double* det_xy, const double* tol_match,
                                          const double* tol_accept, const double* T_pred, int max_rounds, int min_rows,
                                          int min_markers, mpe_result* res, uint32_t* match, mpe_rig_track_info* info) {
  RigGnLds& G = S.G;
  const int n_pairs = n_cam * n_mk;
  RIG_EACH_LANE(l) {
    if (l < n_cam) {
      rig_stage_camera(cams[l], G.cam[l]);
      S.tol_match[l] = tol_match[l];
      S.tol_accept[l] = tol_accept[l];
    }
    if (l < n_mk) {
      S.mk[l][0] = markers[3 * l];
      S.mk[l][1] = markers[3 * l + 1];
      S.mk[l][2] = markers[3 * l + 2];
    }
    if (l < 12) G.T[l] = T_pred[l];
    if (l < 36) G.L[l / 6][l % 6] = 0.0;
    if (l < 6) G.D[l] = 0.0;
    for (int p = l; p < MPE_RIG_MAX_ROWS; p += MPE_RIG_LANES) S.prev[p] = 0;
  }
  int reason = 0, rounds = 0, iters = 0, n_rows = 0, n_distinct = 0;
  for (int r = 0;; ++r) {
    T34 T;
    for (int i = 0; i < 3; ++i)
      for (int c = 0; c < 4; ++c) T.m[i][c] = G.T[i * 4 + c];
    // (1, 2) project and match: lane l <- pairs l, l + 64, ...
    RIG_EACH_LANE(l) {
      for (int p = l; p < MPE_RIG_MAX_ROWS; p += MPE_RIG_LANES) {
        unsigned char s = 0;
        double best = 0.0;
        if (p < n_pairs) {
          const int c = p / n_mk, m = p - c * n_mk;
          const RigCam& C = G.cam[c];
          const double* pm = S.mk[m];
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
            const int b = det_begin[c];
            const int nd = det_begin[c + 1] - b < MPE_MAX_DETECTIONS ? det_begin[c + 1] - b : MPE_MAX_DETECTIONS;
            best = __builtin_inf();
            for (int j = 0; j < nd; ++j) {
              const double du = u - det_xy[2 * (size_t)(b + j)], dv = v - det_xy[2 * (size_t)(b + j) + 1];
              const double dd = du * du + dv * dv;
              if (dd < best) {
                best = dd;
                s = (unsigned char)(j + 1);
              }
            }
            const double tol = r == 0 ? S.tol_match[c] : S.tol_accept[c];
            if (!(sqrt(best) <= tol)) s = 0;
          }
        }
        S.slot[p] = s;
        S.d2[p] = best;
      }
    }
    // (3) one marker per detection: a pair loses to a marker of its camera on the same detection that is nearer, or as
    // near and lower
    RIG_EACH_LANE(l) {
      for (int p = l; p < MPE_RIG_MAX_ROWS; p += MPE_RIG_LANES) {
        unsigned char s = S.slot[p];
        if (s != 0) {
          const int c = p / n_mk, m = p - c * n_mk;
          const double mine = S.d2[p];
          for (int k = 0; k < n_mk; ++k) {
            const int q = c * n_mk + k;
            if (k != m && S.slot[q] == S.slot[p] && (S.d2[q] < mine || (S.d2[q] == mine && k < m))) s = 0;
          }
        }
        S.keep[p] = s;
      }
    }
    // (4, 5) count: lane l <- pairs 4 l .. 4 l + 3
    RIG_EACH_LANE(l) {
      int n = 0, d = 0;
      unsigned ms = 0;
      for (int k = 0; k < MPE_RIG_TRACK_CHUNK; ++k) {
        const int p = MPE_RIG_TRACK_CHUNK * l + k;
        if (S.keep[p] != 0) {
          ++n;
          ms |= 1u << (p % n_mk);
        }
        d |= (S.keep[p] != S.prev[p]) ? 1 : 0;
      }
      S.cnt[l] = (unsigned char)n;
      S.dif[l] = (unsigned char)d;
      S.mseen[l] = (unsigned short)ms;
    }
    n_rows = 0;
    int changed = 0;
    unsigned seen = 0;
    for (int k = 0; k < MPE_RIG_LANES; ++k) {
      n_rows += S.cnt[k];
      changed |= S.dif[k];
      seen |= S.mseen[k];
    }
    n_distinct = 0;
    for (int k = 0; k < MPE_MAX_MARKERS; ++k) n_distinct += (int)((seen >> k) & 1u);
    // the rows into G.P / G.rc, ascending pair order: a lane's first row sits behind the rows of the lanes below it
    RIG_EACH_LANE(l) {
      int j = 0;
      for (int k = 0; k < l; ++k) j += S.cnt[k];
      for (int k = 0; k < MPE_RIG_TRACK_CHUNK; ++k) {
        const int p = MPE_RIG_TRACK_CHUNK * l + k;
        const int s = S.keep[p];
        if (s != 0) {
          const int c = p / n_mk, m = p - c * n_mk;
          const size_t at = 2 * (size_t)(det_begin[c] + s - 1);
          G.P[j][0] = S.mk[m][0];
          G.P[j][1] = S.mk[m][1];
          G.P[j][2] = S.mk[m][2];
          G.P[j][3] = det_xy[at];
          G.P[j][4] = det_xy[at + 1];
          G.rc[j] = (unsigned char)c;
          ++j;
        }
      }
    }
    if (n_rows < min_rows) {
      reason = 1;
      break;
    }
    if (n_distinct < min_markers) {
      reason = 2;
      break;
    }
    if (r > 0 && !changed) break;  // (G.T, G.L, G.D and iters are the previous refinement's)
    RIG_EACH_LANE(l) {
      for (int p = l; p < MPE_RIG_MAX_ROWS; p += MPE_RIG_LANES) S.prev[p] = S.keep[p];
    }
    // (6)
    iters = rig_gn_iterate(G, n_rows, true);
    rounds = r + 1;
    bool finite = true;
    for (int i = 0; i < 12; ++i) finite = finite && (fabs(G.T[i]) <= 1.7976931348623157e308);
    if (!finite) {
      reason = 3;
      break;
    }
    if (rounds >= max_rounds) break;
  }
  // accept: the residual of every final row at the final pose (rig_row's e)
  double worst = 0.0, sum = 0.0;
  if (reason == 0) {
    T34 T;
    for (int i = 0; i < 3; ++i)
      for (int c = 0; c < 4; ++c) T.m[i][c] = G.T[i * 4 + c];
    RIG_EACH_LANE(l) {
      for (int j = l; j < n_rows; j += MPE_RIG_LANES) {
        rig_row(G, T, j);
        S.d2[j] = G.J[j][12] * G.J[j][12] + G.J[j][13] * G.J[j][13];
      }
    }
    for (int j = 0; j < n_rows; ++j) {
      const double len = sqrt(S.d2[j]);
      if (!(len <= S.tol_accept[G.rc[j]])) reason = 4;
      if (!(len <= worst)) worst = len;
      sum += S.d2[j];
    }
  }
  if (reason == 0) {
    rig_gn_finish(G, n_rows, true, iters, res);
  } else {
    unsigned cams_seen = 0;
    int n_seen = 0;
    for (int j = 0; j < n_rows; ++j) {
      const unsigned bit = 1u << G.rc[j];
      n_seen += (cams_seen & bit) ? 0 : 1;
      cams_seen |= bit;
    }
    RIG_EACH_LANE(l) {
      if (l < 36) res->cov[l] = 0.0;
      if (l < 12) res->T[l] = T_pred[l];
      if (l == 0) {
        res->T[12] = 0.0;
        res->T[13] = 0.0;
        res->T[14] = 0.0;
        res->T[15] = 1.0;
        res->status = MPE_FRAME_NO_POSE;
        res->n_det = n_seen;
        res->n_corr = n_rows;
        res->gn_iterations = iters;
      }
    }
  }
  RIG_EACH_LANE(l) {
    for (int p = l; p < n_pairs; p += MPE_RIG_LANES) match[p] = S.keep[p];
    if (l == 0) {
      info->rounds = rounds;
      info->rows = n_rows;
      info->distinct_markers = n_distinct;
      info->reason = reason;
      info->max_residual = worst;
      info->rms = n_rows > 0 ? sqrt(sum / n_rows) : 0.0;
    }
  }
}
