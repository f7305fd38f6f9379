// mpe_rig_gn.h — the logic of k_rig_refine (mpe_k3.hip): optimisePose (pose_estimator.cpp:733-792) over measurement rows
// that bring their own camera — the cameras of a calibrated rig see one body, and ONE pose T (rig <- marker frame) is
// refined over all their rows.  Camera c has K_c = (fx, fy, cx, cy) and a rigid extrinsic E_c = [R_c | t_c], camera <-
// rig.  Per iteration, for row j = (c, marker p, undistorted pixel uv), in row order:
//   X = T p (the first three lines of project_T),  q = R_c X + t_c,  (u, v) = ((fx q0 + cx q2) / q2, (fy q1 + cy q2) / q2),
//   e = uv - (u, v),  J = computeJacobian's 2 x 6 row pair (pose_estimator.cpp:945-957) at q with K_c, TIMES the adjoint
//   Ad = [[R_c, hat(t_c) R_c], [0, R_c]] of E_c (twist order (upsilon, omega)): the chain rule of q = E_c exp(xi) T p;
// A = sum J^T J, b = sum J^T e in row order, unpivoted LDL^T, T <- exp(dT) T, stop when max|dT| <= 1e-13 (tested behind
// the update) or after 500 iterations; cov = inverse of the last iteration's A: the covariance of a left twist in the
// rig frame.  With one camera and E = I every product with Ad and R_c multiplies by 1 or adds 0, and without contraction
// (-ffp-contract=off) the scalars are those of k3_gauss_newton / k3b_group_body: the same pose, covariance and count.
//
// The form is one 64-lane wave per problem, all state that crosses a phase in LDS (RigGnLds): lanes take rows l, l + 64,
// ..., 27 lanes sum the 21 + 6 entries of (A, b), the LDL^T runs column by column with a column's divisions on five
// lanes, lane 0 solves, the 3 x 3 matrices of the exponential map go one entry per lane — k3b_group_body's phases with
// a group of 64.  A phase is written `RIG_EACH_LANE(l) { ... }`: on the device the body runs once with l = the lane and
// is followed by wave_sync(); a host build runs it for l = 0 .. 63 one after the other, which is the same thing because
// no lane reads within a phase what another lane writes in it.  What is wave-uniform (the pose, the step, the stop
// test) is read from LDS between phases.  So the CPU tier runs THIS text (tests/host/rig_gn_host.cpp, plain and under
// ASan / UBSan).
//
// No #include and no namespace of its own: the text goes behind the tail helpers of mpe_k3.hip (T34, project_T's
// arithmetic, apply_exp's operation order) inside namespace mpe, and needs include/mpe.h (mpe_rig_camera) in front.
#define MPE_RIG_MAX_ROWS (MPE_RIG_MAX_CAMERAS * MPE_MAX_MARKERS)
#define MPE_RIG_LANES 64

#if defined(__HIPCC__)
#define RIG_EACH_LANE(l_) for (int l_ = (int)threadIdx.x, once_ = 0; once_ == 0; ++once_, wave_sync())
#else
#define RIG_EACH_LANE(l_) for (int l_ = 0; l_ < MPE_RIG_LANES; ++l_)
#endif

struct RigCam {
  double fx, fy, cx, cy;
  double R[3][3];
  double t[3];
  double M[3][3];  // hat(t) R: the upper right block of the adjoint
};

struct RigGnLds {
  double J[MPE_RIG_MAX_ROWS][14];  // per row: J0[6], J1[6] (already times Ad), e0, e1
  double P[MPE_RIG_MAX_ROWS][5];   // per row: marker xyz, pixel uv
  RigCam cam[MPE_RIG_MAX_CAMERAS];
  double Ab[27];  // upper triangle of A (21, row-major) then b (6)
  double L[6][6];
  double D[6];
  double dT[6];
  double O[9], Rm[9], Vm[9];
  double T[12], Tn[12];
  unsigned char rc[MPE_RIG_MAX_ROWS];  // per row: camera
};

// K and the extrinsic of one camera as the rows use them.  The extrinsic is trusted: its upper 3 x 4 is taken as
// [R | t], nothing is checked for orthonormality and its last row is not read.
__device__ __forceinline__ void rig_stage_camera(const mpe_rig_camera& c, RigCam& o) {
  o.fx = c.K[0];
  o.fy = c.K[4];
  o.cx = c.K[2];
  o.cy = c.K[5];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o.R[i][j] = c.T_cam_rig[4 * i + j];
    o.t[i] = c.T_cam_rig[4 * i + 3];
  }
  const double H[3][3] = {{0, -o.t[2], o.t[1]}, {o.t[2], 0, -o.t[0]}, {-o.t[1], o.t[0], 0}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) o.M[i][j] = H[i][0] * o.R[0][j] + H[i][1] * o.R[1][j] + H[i][2] * o.R[2][j];
}

// row j: residual and the two Jacobian rows times Ad -> G.J[j]
__device__ __forceinline__ void rig_row(RigGnLds& G, const T34& T, int j) {
  const RigCam& C = G.cam[G.rc[j]];
  const double* p = G.P[j];
  const double X = T.m[0][0] * p[0] + T.m[0][1] * p[1] + T.m[0][2] * p[2] + T.m[0][3];
  const double Y = T.m[1][0] * p[0] + T.m[1][1] * p[1] + T.m[1][2] * p[2] + T.m[1][3];
  const double Z = T.m[2][0] * p[0] + T.m[2][1] * p[1] + T.m[2][2] * p[2] + T.m[2][3];
  const double x = C.R[0][0] * X + C.R[0][1] * Y + C.R[0][2] * Z + C.t[0];
  const double y = C.R[1][0] * X + C.R[1][1] * Y + C.R[1][2] * Z + C.t[1];
  const double z = C.R[2][0] * X + C.R[2][1] * Y + C.R[2][2] * Z + C.t[2];
  const double fx = C.fx, fy = C.fy;
  const double u = (fx * x + C.cx * z) / z;
  const double v = (fy * y + C.cy * z) / z;
  const double z_2 = z * z;
  // computeJacobian, pose_estimator.cpp:945-957
  double a[6], b[6];
  a[0] = 1 / z * fx;
  a[1] = 0;
  a[2] = -x / z_2 * fx;
  a[3] = -x * y / z_2 * fx;
  a[4] = (1 + (x * x / z_2)) * fx;
  a[5] = -y / z * fx;
  b[0] = 0;
  b[1] = 1 / z * fy;
  b[2] = -y / z_2 * fy;
  b[3] = -(1 + y * y / z_2) * fy;
  b[4] = x * y / z_2 * fy;
  b[5] = x / z * fy;
  double* Jr = G.J[j];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    Jr[k] = a[0] * C.R[0][k] + a[1] * C.R[1][k] + a[2] * C.R[2][k];
    Jr[3 + k] = (a[0] * C.M[0][k] + a[1] * C.M[1][k] + a[2] * C.M[2][k]) +
                (a[3] * C.R[0][k] + a[4] * C.R[1][k] + a[5] * C.R[2][k]);
    Jr[6 + k] = b[0] * C.R[0][k] + b[1] * C.R[1][k] + b[2] * C.R[2][k];
    Jr[9 + k] = (b[0] * C.M[0][k] + b[1] * C.M[1][k] + b[2] * C.M[2][k]) +
                (b[3] * C.R[0][k] + b[4] * C.R[1][k] + b[5] * C.R[2][k]);
  }
  Jr[12] = p[3] - u;
  Jr[13] = p[4] - v;
}

// index of A[r][c], r <= c, in the packed upper triangle (k3g_tri)
__device__ __forceinline__ int rig_tri(int r, int c) { return r * 6 - (r * (r - 1)) / 2 + (c - r); }

// The three parts of a refinement: rig_gn_stage brings a problem into LDS, rig_gn_iterate runs the Gauss-Newton over
// the n_rows rows that are in G.P / G.rc from the pose in G.T (the rig's cameras in G.cam) and leaves the pose in G.T
// and the factors of the last iteration's A in G.L / G.D, rig_gn_finish writes the record.  rig_gn_refine is the three
// in a row; k_rig_track (mpe_rig_track.h) stages its rows itself and calls the last two.
__device__ __forceinline__ void rig_gn_stage(RigGnLds& G, const mpe_rig_camera* cams, int n_cam, const int* row_cam,
                                             const double* row_xyz, const double* row_uv, int n_rows,
                                             const double* T_init) {
  RIG_EACH_LANE(l) {
    if (l < n_cam) rig_stage_camera(cams[l], G.cam[l]);
    for (int j = l; j < n_rows; j += MPE_RIG_LANES) {
      G.P[j][0] = row_xyz[3 * j];
      G.P[j][1] = row_xyz[3 * j + 1];
      G.P[j][2] = row_xyz[3 * j + 2];
      G.P[j][3] = row_uv[2 * j];
      G.P[j][4] = row_uv[2 * j + 1];
      G.rc[j] = (unsigned char)row_cam[j];
    }
    if (l < 12) G.T[l] = T_init[l];
    if (l < 36) G.L[l / 6][l % 6] = 0.0;
    if (l < 6) G.D[l] = 0.0;
  }
}

// -> the iterations run (0 when !run)
__device__ __forceinline__ int rig_gn_iterate(RigGnLds& G, int n_rows, bool run) {
  int iters = 0;
  for (int it = 0; run && it < 500; ++it) {
    T34 T;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) T.m[r][c] = G.T[r * 4 + c];
    // (a) Jacobian rows: lane l <- rows l, l + 64, ...
    RIG_EACH_LANE(l) {
      for (int j = l; j < n_rows; j += MPE_RIG_LANES) rig_row(G, T, j);
    }
    // (b) A = sum J^T J (upper triangle), b = sum J^T e, each entry summed over the rows in row order
    RIG_EACH_LANE(l) {
      if (l < 27) {
        double acc = 0;
        if (l < 21) {
          int r = 0, base = 0;
          while (l >= base + (6 - r)) {
            base += 6 - r;
            ++r;
          }
          const int c = r + (l - base);
          for (int j = 0; j < n_rows; ++j) acc += G.J[j][r] * G.J[j][c] + G.J[j][6 + r] * G.J[j][6 + c];
        } else {
          const int r = l - 21;
          for (int j = 0; j < n_rows; ++j) acc += G.J[j][r] * G.J[j][12] + G.J[j][6 + r] * G.J[j][13];
        }
        G.Ab[l] = acc;
      }
    }
    // (c) unpivoted LDL^T (ldl6_factor), column by column: lane j the pivot, lanes j + 1 .. 5 the column's divisions
    for (int j = 0; j < 6; ++j) {
      RIG_EACH_LANE(l) {
        if (l == j) {
          double dd = G.Ab[rig_tri(j, j)];
          for (int k = 0; k < j; ++k) dd -= G.L[j][k] * G.L[j][k] * G.D[k];
          G.D[j] = dd;
        }
      }
      RIG_EACH_LANE(l) {
        if (l > j && l < 6) {
          double sacc = G.Ab[rig_tri(j, l)];  // A[l][j] = A[j][l]
          for (int k = 0; k < j; ++k) sacc -= G.L[l][k] * G.L[j][k] * G.D[k];
          G.L[l][j] = sacc / G.D[j];
        }
      }
    }
    // (d) ldl6_solve on lane 0 (a chain of 36 dependent operations: nothing to spread)
    RIG_EACH_LANE(l) {
      if (l == 0) {
        double yv[6], xv[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          double sacc = G.Ab[21 + i];
#pragma unroll
          for (int k = 0; k < i; ++k) sacc -= G.L[i][k] * yv[k];
          yv[i] = sacc;
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) yv[i] /= G.D[i];
#pragma unroll
        for (int i = 5; i >= 0; --i) {
          double sacc = yv[i];
#pragma unroll
          for (int k = i + 1; k < 6; ++k) sacc -= G.L[k][i] * xv[k];
          xv[i] = sacc;
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) G.dT[i] = xv[i];
      }
    }
    // (e) exponentialMap(dT) * T (apply_exp), the 3x3 matrices one entry per lane
    const double ux = G.dT[0], uy = G.dT[1], uz = G.dT[2], wx = G.dT[3], wy = G.dT[4], wz = G.dT[5];
    const double theta = sqrt(wx * wx + wy * wy + wz * wz);
    const double th2 = theta * theta;
    RIG_EACH_LANE(l) {
      if (l < 9) {
        const double Ov[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
        double o = Ov[0];
#pragma unroll
        for (int q = 1; q < 9; ++q) o = (l == q) ? Ov[q] : o;
        G.O[l] = o;
      }
    }
    RIG_EACH_LANE(l) {
      if (l < 9) {
        const int i = l / 3, j = l - 3 * i;
        const double o2 = G.O[3 * i] * G.O[j] + G.O[3 * i + 1] * G.O[3 + j] + G.O[3 * i + 2] * G.O[6 + j];
        const double o = G.O[l];
        const double I = (i == j) ? 1.0 : 0.0;
        double rm = I, vm = I;
        if (theta != 0) {
          double st, ct;
          sincos(theta, &st, &ct);
          rm = I + o / theta * st + o2 / th2 * (1 - ct);
          vm = I + (1 - ct) / th2 * o + (theta - st) / (th2 * theta) * o2;
        }
        G.Rm[l] = rm;
        G.Vm[l] = vm;
      }
    }
    RIG_EACH_LANE(l) {
      if (l < 12) {
        const int i = l >> 2, j = l & 3;
        double sacc = G.Rm[3 * i] * G.T[j] + G.Rm[3 * i + 1] * G.T[4 + j] + G.Rm[3 * i + 2] * G.T[8 + j];
        if (j == 3) sacc += G.Vm[3 * i] * ux + G.Vm[3 * i + 1] * uy + G.Vm[3 * i + 2] * uz;
        G.Tn[l] = sacc;
      }
    }
    RIG_EACH_LANE(l) {  // (every read of the old pose is done)
      if (l < 12) G.T[l] = G.Tn[l];
    }
    iters = it + 1;
    double mx = -1;  // norm_max, pose_estimator.cpp:1073-1085
    for (int r = 0; r < 6; ++r) {
      const double av = fabs(G.dT[r]);
      if (av > mx) mx = av;
    }
    if (mx <= 1e-13) break;
  }
  return iters;
}

// Fills res: T, cov, status, gn_iterations, n_corr = n_rows, n_det = cameras with a row.
__device__ __forceinline__ void rig_gn_finish(RigGnLds& G, int n_rows, bool run, int iters, mpe_result* res) {
  // the reference's isFinite on the final pose; the cameras that brought a row
  bool finite = true;
  for (int i = 0; i < 12; ++i) finite = finite && (fabs(G.T[i]) <= 1.7976931348623157e308);
  unsigned seen = 0;
  int n_seen = 0;
  for (int j = 0; j < n_rows; ++j) {
    const unsigned bit = 1u << G.rc[j];
    n_seen += (seen & bit) ? 0 : 1;
    seen |= bit;
  }
  // pose_covariance_ = A.inverse() with the A of the last iteration (pose_estimator.cpp:790): its factors are still in
  // G.L / G.D; column c of the inverse on lane c
  RIG_EACH_LANE(l) {
    if (run && l < 6) {
      double yv[6], xv[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        double sacc = (i == l) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k) sacc -= G.L[i][k] * yv[k];
        yv[i] = sacc;
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) yv[i] /= G.D[i];
#pragma unroll
      for (int i = 5; i >= 0; --i) {
        double sacc = yv[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) sacc -= G.L[k][i] * xv[k];
        xv[i] = sacc;
      }
#pragma unroll
      for (int r = 0; r < 6; ++r) res->cov[r * 6 + l] = xv[r];
    }
    if (!run && l < 36) res->cov[l] = 0.0;
    if (l < 12) res->T[l] = G.T[l];
    if (l == 0) {
      res->T[12] = 0.0;
      res->T[13] = 0.0;
      res->T[14] = 0.0;
      res->T[15] = 1.0;
      res->status = (run && finite) ? MPE_FRAME_POSE : MPE_FRAME_NO_POSE;
      res->n_det = n_seen;
      res->n_corr = n_rows;
      res->gn_iterations = iters;
    }
  }
}

// One problem on one wave.  cams: the rig's n_cam cameras; rows: n_rows of (camera, marker xyz, pixel uv), 0 <= n_rows <=
// MPE_RIG_MAX_ROWS and every camera index below n_cam (the caller has checked both); T_init: 16 doubles, row-major.
// Fills res: T, cov, status, gn_iterations, n_corr = n_rows, n_det = cameras with a row.
__device__ __forceinline__ void rig_gn_refine(RigGnLds& G, const mpe_rig_camera* cams, int n_cam, const int* row_cam,
                                              const double* row_xyz, const double* row_uv, int n_rows,
                                              const double* T_init, mpe_result* res) {
  rig_gn_stage(G, cams, n_cam, row_cam, row_xyz, row_uv, n_rows, T_init);
  const bool run = n_rows >= 3;  // fewer rows leave the 6x6 normal equations singular (mpe_optimise_pose's rule)
  const int iters = rig_gn_iterate(G, n_rows, run);
  rig_gn_finish(G, n_rows, run, iters, res);
}
