// mpe_rig_ba.h — the logic of the k_rig_ba_* kernels (mpe_k3.hip): the extrinsics of a rig calibrated from the body it
// tracks (mpe_rig_calibrate).  A bundle adjustment over views f = 0 .. n - 1 of ONE body: the unknowns are a left twist
// xi_f on every view pose T_f (rig <- marker frame) and a left twist eta_c on the extrinsic E_c (camera <- rig) of every
// FREE camera; the reference camera keeps its extrinsic (the gauge).  Row j of view f = (camera c, marker p, pixel uv):
//   q = E_c T_f p,  e = uv - project(K_c, q),  (a, b) = computeJacobian's row pair at q with K_c (mpe_rig_gn.h),
//   Je = (a, b)            = d e / d eta_c   (d q / d eta = [I | -hat(q)]),
//   Jp = (a, b) Ad(E_c)    = d e / d xi_f    (what rig_row stores).
// Gauss-Newton with a Schur complement over the view poses, per iteration four steps, each a launch of its own:
//   linearise (one wave per view)   U_f = sum Jp^T Jp, g_f = sum Jp^T e, per free camera c of the view W_fc = sum Jp^T Je,
//                                   V_fc = sum Je^T Je, h_fc = sum Je^T e — every entry summed over the rows in row order —,
//                                   LDL^T of U_f, Y_fc = U_f^-1 W_fc, z_f = U_f^-1 g_f, sse_f = sum e^2  -> the view's record
//   reduce (one wave per 6 x 6 block (i, j), i <= j, of the free cameras)
//                                   accS_ij = sum_f W_fi^T Y_fj, on the diagonal also accV_i = sum_f V_fi, acch_i = sum_f
//                                   h_fi, accz_i = sum_f W_fi^T z_f: every entry by ONE lane over the views in view order
//   solve (one wave)                S = V - accS, r = h - accz, unpivoted LDL^T of S (packed lower triangle), eta = S^-1 r
//   update (one lane per view)      xi_f = z_f - sum_c Y_fc eta_c, T_f <- exp(xi_f) T_f (apply_exp), the view's max |xi|
//   finish (one wave)               E_c <- exp(eta_c) E_c (apply_exp), the largest |step| of all eta and xi, the sum of
//                                   sse_f in view order -> the two doubles the host reads to decide whether to stop
// and once behind the last iteration: covariance (one wave per free camera) = the camera's 6 x 6 diagonal block of S^-1
// from the stored factor.  No atomics anywhere: an entry's value is fixed by the view order and the row order alone, not
// by the launch shape, and is the same bit for bit from run to run.
//
// The form is mpe_rig_gn.h's: 64-lane waves, state that crosses a phase in LDS, phases written RIG_EACH_LANE(l) { ... },
// so the CPU tier runs THIS text (tests/host/rig_ba_host.cpp).  No #include and no namespace of its own: the text goes
// behind mpe_rig_gn.h (RigCam, rig_stage_camera, rig_tri, T34, apply_exp) and needs mpe_rig_ba_dev.h (the sizes, RigBaDev:
// what the host side shares) in front.
//
// A view's record (doubles): [z 6 | sse | 0] then per free camera of the view, ascending, a slot [W 36 (W[a][b], a the
// pose component) | Y 36 | V 21 (rig_tri) | h 6].  View f's record starts at rec + (view_cum[f] - view_cum[first]).
__device__ __forceinline__ int rig_ba_pair(int i, int j, int n_free) { return i * n_free - (i * (i - 1)) / 2 + (j - i); }
__device__ __forceinline__ int rig_ba_low(int i, int j) { return (i * (i + 1)) / 2 + j; }  // j <= i
__device__ __forceinline__ int rig_ba_slot(unsigned mask, int fi) { return __builtin_popcount(mask & ((1u << fi) - 1u)); }

struct RigBaLinLds {
  double J[MPE_RIG_MAX_ROWS][26];  // per row: Jp0[6], Jp1[6], Je0[6], Je1[6], e0, e1
  RigCam cam[MPE_RIG_MAX_CAMERAS];
  double R[MPE_RIG_BA_HEAD + MPE_RIG_BA_MAX_FREE * MPE_RIG_BA_SLOT];  // the record as it grows
  double Ug[28];  // upper triangle of U (21), g (6), sse
  double L[6][6];
  double D[6];
  double T[12];
  unsigned char rs[MPE_RIG_MAX_ROWS];        // per row: slot of its camera, 255 = the reference camera
  unsigned char slot_of[MPE_RIG_MAX_CAMERAS];
};

// row (marker xyz at p, pixel at uv) of camera C under the view pose T: rig_row's arithmetic, the raw pair kept as well
__device__ __forceinline__ void rig_ba_row(const RigCam& C, const T34& T, const double* p, const double* uv, double* Jr) {
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
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    Jr[k] = a[0] * C.R[0][k] + a[1] * C.R[1][k] + a[2] * C.R[2][k];
    Jr[3 + k] = (a[0] * C.M[0][k] + a[1] * C.M[1][k] + a[2] * C.M[2][k]) +
                (a[3] * C.R[0][k] + a[4] * C.R[1][k] + a[5] * C.R[2][k]);
    Jr[6 + k] = b[0] * C.R[0][k] + b[1] * C.R[1][k] + b[2] * C.R[2][k];
    Jr[9 + k] = (b[0] * C.M[0][k] + b[1] * C.M[1][k] + b[2] * C.M[2][k]) +
                (b[3] * C.R[0][k] + b[4] * C.R[1][k] + b[5] * C.R[2][k]);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    Jr[12 + k] = a[k];
    Jr[18 + k] = b[k];
  }
  Jr[24] = uv[0] - u;
  Jr[25] = uv[1] - v;
}

// (r, c), r <= c, of index t of the packed upper triangle of a 6 x 6 (rig_tri's inverse)
__device__ __forceinline__ void rig_ba_untri(int t, int& r, int& c) {
  int base = 0;
  r = 0;
  while (t >= base + (6 - r)) {
    base += 6 - r;
    ++r;
  }
  c = r + (t - base);
}

// 6 x 6 solve with the factors in G.L / G.D (ldl6_solve's order); rhs and x may be the same array with any stride (Lds:
// RigBaLinLds, or mpe_body_ba.h's)
template <class Lds>
__device__ __forceinline__ void rig_ba_solve6(const Lds& G, const double* rhs, int rs, double* x, int xs) {
  double yv[6], xv[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double sacc = rhs[i * rs];
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
  for (int i = 0; i < 6; ++i) x[i * xs] = xv[i];
}

// ---- linearise: used view f on one wave ---------------------------------------------------------------------------
__device__ __forceinline__ void rig_ba_linearise(RigBaLinLds& G, const RigBaDev& d, int f, int chunk_first) {
  const int b0 = d.view_begin[f];
  int n_rows = d.view_begin[f + 1] - b0;
  n_rows = n_rows < 0 ? 0 : (n_rows > MPE_RIG_MAX_ROWS ? MPE_RIG_MAX_ROWS : n_rows);
  const unsigned mask = d.view_mask[f];
  const int n_slots = __builtin_popcount(mask);
  const int n_rec = MPE_RIG_BA_HEAD + n_slots * MPE_RIG_BA_SLOT;
  const int* row_cam = d.row_cam + b0;
  const double* row_xyz = d.row_xyz + 3 * (size_t)b0;
  const double* row_uv = d.row_uv + 2 * (size_t)b0;
  double* rec = d.rec + (d.view_cum[f] - d.view_cum[chunk_first]);
  RIG_EACH_LANE(l) {
    if (l < d.n_cam) {
      rig_stage_camera(d.cams[l], G.cam[l]);
      const int fi = d.cam_free[l];
      G.slot_of[l] = (unsigned char)((fi >= 0 && ((mask >> fi) & 1u)) ? rig_ba_slot(mask, fi) : 255);
    }
    if (l < 12) G.T[l] = d.T_view[16 * (size_t)f + l];
    if (l < 36) G.L[l / 6][l % 6] = 0.0;
    if (l < 6) G.D[l] = 0.0;
    for (int i = l; i < n_rec; i += MPE_RIG_LANES) G.R[i] = 0.0;
  }
  T34 T;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) T.m[r][c] = G.T[r * 4 + c];
  // (a) rows: lane l <- rows l, l + 64, ...
  RIG_EACH_LANE(l) {
    for (int j = l; j < n_rows; j += MPE_RIG_LANES) {
      const int c = row_cam[j];
      rig_ba_row(G.cam[c], T, row_xyz + 3 * j, row_uv + 2 * j, G.J[j]);
      G.rs[j] = G.slot_of[c];
    }
  }
  // (b) U, g, sse over all rows, and per camera slot W, V, h over the camera's rows: one entry per lane, rows in row order
  RIG_EACH_LANE(l) {
    if (l < 28) {
      double acc = 0;
      if (l < 21) {
        int r, c;
        rig_ba_untri(l, r, c);
        for (int j = 0; j < n_rows; ++j) acc += G.J[j][r] * G.J[j][c] + G.J[j][6 + r] * G.J[j][6 + c];
      } else if (l < 27) {
        const int r = l - 21;
        for (int j = 0; j < n_rows; ++j) acc += G.J[j][r] * G.J[j][24] + G.J[j][6 + r] * G.J[j][25];
      } else {
        for (int j = 0; j < n_rows; ++j) acc += G.J[j][24] * G.J[j][24] + G.J[j][25] * G.J[j][25];
      }
      G.Ug[l] = acc;
    }
  }
  RIG_EACH_LANE(l) {
    if (l < 63) {
      int i0, i1, off;  // the entry is J[i0] * J[i1] + J[6 + i0] * J[6 + i1]
      if (l < 36) {
        i0 = l / 6;
        i1 = 12 + l % 6;
        off = l;
      } else if (l < 57) {
        int r, c;
        rig_ba_untri(l - 36, r, c);
        i0 = 12 + r;
        i1 = 12 + c;
        off = 72 + (l - 36);
      } else {
        i0 = 12 + (l - 57);
        i1 = 24;
        off = 93 + (l - 57);
      }
      const int i0b = i0 + 6, i1b = (i1 == 24) ? 25 : i1 + 6;
      for (int j = 0; j < n_rows; ++j) {
        const int s = G.rs[j];
        if (s != 255) G.R[MPE_RIG_BA_HEAD + s * MPE_RIG_BA_SLOT + off] += G.J[j][i0] * G.J[j][i1] + G.J[j][i0b] * G.J[j][i1b];
      }
    }
  }
  // (c) unpivoted LDL^T of U, column by column (rig_gn_refine's phase (c))
  for (int j = 0; j < 6; ++j) {
    RIG_EACH_LANE(l) {
      if (l == j) {
        double dd = G.Ug[rig_tri(j, j)];
        for (int k = 0; k < j; ++k) dd -= G.L[j][k] * G.L[j][k] * G.D[k];
        G.D[j] = dd;
      }
    }
    RIG_EACH_LANE(l) {
      if (l > j && l < 6) {
        double sacc = G.Ug[rig_tri(j, l)];
        for (int k = 0; k < j; ++k) sacc -= G.L[l][k] * G.L[j][k] * G.D[k];
        G.L[l][j] = sacc / G.D[j];
      }
    }
  }
  // (d) z = U^-1 g and the columns of Y = U^-1 W, one right-hand side per lane
  RIG_EACH_LANE(l) {
    for (int r = l; r < 1 + 6 * n_slots; r += MPE_RIG_LANES) {
      if (r == 0) {
        rig_ba_solve6(G, G.Ug + 21, 1, G.R, 1);
        G.R[6] = G.Ug[27];
      } else {
        const int k = (r - 1) / 6, b = (r - 1) % 6;
        double* S = G.R + MPE_RIG_BA_HEAD + k * MPE_RIG_BA_SLOT;
        rig_ba_solve6(G, S + b, 6, S + 36 + b, 6);
      }
    }
  }
  RIG_EACH_LANE(l) {
    for (int i = l; i < n_rec; i += MPE_RIG_LANES) rec[i] = G.R[i];
    if (l == 0) d.sse[f] = G.Ug[27];
  }
}

// ---- reduce: block (ci, cj), ci <= cj, of the free cameras over the views [first, first + count) ---------------------
struct RigBaRedLds {
  double S[MPE_RIG_BA_CHUNK][105];  // per staged view: W_i 36, Y_j 36, and on the diagonal V_i 21, h_i 6, z 6
  double accS[36], accV[36], acch[6], accz[6];
  long long oi[MPE_RIG_BA_CHUNK], oj[MPE_RIG_BA_CHUNK], ob[MPE_RIG_BA_CHUNK];  // where the view's slots / record start
  unsigned char has[MPE_RIG_BA_CHUNK];
};

__device__ __forceinline__ void rig_ba_reduce(RigBaRedLds& G, const RigBaDev& d, int ci, int cj, int first, int count,
                                              int restart) {
  const bool diag = ci == cj;
  const int items = diag ? 105 : 72;
  double* Sacc = d.Sacc + 72 * (size_t)rig_ba_pair(ci, cj, d.n_free);
  double* racc = d.racc + 12 * (size_t)ci;
  const unsigned need = (1u << ci) | (1u << cj);
  RIG_EACH_LANE(l) {
    if (l < 36) {
      G.accS[l] = restart ? 0.0 : Sacc[l];
      G.accV[l] = restart ? 0.0 : Sacc[36 + l];
    } else if (l < 42) {
      G.acch[l - 36] = (restart || !diag) ? 0.0 : racc[l - 36];
      G.accz[l - 36] = (restart || !diag) ? 0.0 : racc[6 + l - 36];
    }
  }
  for (int f0 = first; f0 < first + count; f0 += MPE_RIG_BA_CHUNK) {
    const int nv = (first + count - f0) < MPE_RIG_BA_CHUNK ? (first + count - f0) : MPE_RIG_BA_CHUNK;
    // which of these views hold both cameras, and where their slots are: a view per lane
    RIG_EACH_LANE(l) {
      for (int v = l; v < nv; v += MPE_RIG_LANES) {
        const int f = f0 + v;
        const unsigned mask = d.view_mask[f];
        const long long base = d.view_cum[f] - d.view_cum[first];
        G.has[v] = (mask & need) == need ? 1 : 0;
        G.ob[v] = base;
        G.oi[v] = base + MPE_RIG_BA_HEAD + rig_ba_slot(mask, ci) * MPE_RIG_BA_SLOT;
        G.oj[v] = base + MPE_RIG_BA_HEAD + rig_ba_slot(mask, cj) * MPE_RIG_BA_SLOT;
      }
    }
    // stage what the block needs of them: consecutive lanes read consecutive doubles of a record, eight loads in flight
    // per lane (the addresses come from LDS, so nothing orders them)
    RIG_EACH_LANE(l) {
      for (int i0 = l; i0 < nv * items; i0 += 8 * MPE_RIG_LANES) {
        double val[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int idx = i0 + u * MPE_RIG_LANES;
          val[u] = 0.0;
          if (idx < nv * items) {
            const int v = idx / items, e = idx - v * items;
            if (G.has[v]) val[u] = e < 36 ? d.rec[G.oi[v] + e] : (e < 72 ? d.rec[G.oj[v] + e] : (e < 99 ? d.rec[G.oi[v] + e] : d.rec[G.ob[v] + (e - 99)]));
          }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int idx = i0 + u * MPE_RIG_LANES;
          if (idx < nv * items) {
            const int v = idx / items, e = idx - v * items;
            G.S[v][e] = val[u];
          }
        }
      }
    }
    // one entry per lane, the views in view order
    RIG_EACH_LANE(l) {
      if (l < 36) {
        const int a = l / 6, b = l % 6;
        const int t = a <= b ? rig_tri(a, b) : rig_tri(b, a);
        double s = G.accS[l], vv = G.accV[l];
        for (int v = 0; v < nv; ++v) {
          if (!G.has[v]) continue;
          double p = 0;
#pragma unroll
          for (int k = 0; k < 6; ++k) p += G.S[v][k * 6 + a] * G.S[v][36 + k * 6 + b];
          s += p;
          if (diag) vv += G.S[v][72 + t];
        }
        G.accS[l] = s;
        G.accV[l] = vv;
      } else if (l < 42 && diag) {
        const int a = l - 36;
        double hh = G.acch[a], zz = G.accz[a];
        for (int v = 0; v < nv; ++v) {
          if (!G.has[v]) continue;
          double p = 0;
#pragma unroll
          for (int k = 0; k < 6; ++k) p += G.S[v][k * 6 + a] * G.S[v][99 + k];
          hh += G.S[v][93 + a];
          zz += p;
        }
        G.acch[a] = hh;
        G.accz[a] = zz;
      }
    }
  }
  RIG_EACH_LANE(l) {
    if (l < 36) {
      Sacc[l] = G.accS[l];
      Sacc[36 + l] = G.accV[l];
    } else if (l < 42 && diag) {
      racc[l - 36] = G.acch[l - 36];
      racc[6 + l - 36] = G.accz[l - 36];
    }
  }
}

// ---- solve and covariance: the reduced system on one wave ------------------------------------------------------------
struct RigBaSolveLds {
  double L[MPE_RIG_BA_TRI];          // packed lower triangle: S, then its factor in place
  double X[6][MPE_RIG_BA_MAX_N];     // right-hand sides / solutions
};

// forward, diagonal and backward substitution of n_col right-hand sides in G.X with the factor in G.L: a column of L
// per phase, the (right-hand side, row) pairs spread over the lanes; row i subtracts k = 0 .. i - 1 ascending on the way
// down and k = n - 1 .. i + 1 descending on the way up
__device__ __forceinline__ void rig_ba_substitute(RigBaSolveLds& G, int n, int n_col) {
  for (int j = 0; j < n; ++j) {
    RIG_EACH_LANE(l) {
      for (int idx = l; idx < n_col * n; idx += MPE_RIG_LANES) {
        const int c = idx / n, i = idx - c * n;
        if (i > j) G.X[c][i] -= G.L[rig_ba_low(i, j)] * G.X[c][j];
      }
    }
  }
  RIG_EACH_LANE(l) {
    for (int idx = l; idx < n_col * n; idx += MPE_RIG_LANES) {
      const int c = idx / n, i = idx - c * n;
      G.X[c][i] /= G.L[rig_ba_low(i, i)];
    }
  }
  for (int j = n - 1; j >= 0; --j) {
    RIG_EACH_LANE(l) {
      for (int idx = l; idx < n_col * n; idx += MPE_RIG_LANES) {
        const int c = idx / n, i = idx - c * n;
        if (i < j) G.X[c][i] -= G.L[rig_ba_low(j, i)] * G.X[c][j];
      }
    }
  }
}

__device__ __forceinline__ void rig_ba_solve(RigBaSolveLds& G, const RigBaDev& d) {
  const int n = 6 * d.n_free;
  // S = V - accS (lower triangle from the stored upper blocks), r = h - accz
  RIG_EACH_LANE(l) {
    for (int idx = l; idx < (n * (n + 1)) / 2; idx += MPE_RIG_LANES) {
      int I = 0;
      while ((I + 1) * (I + 2) / 2 <= idx) ++I;
      const int Jc = idx - (I * (I + 1)) / 2;
      const int i = I / 6, a = I - 6 * i, j = Jc / 6, b = Jc - 6 * j;  // j <= i: block (j, i), its entry (b, a)
      const double* blk = d.Sacc + 72 * (size_t)rig_ba_pair(j, i, d.n_free);
      G.L[idx] = (i == j ? blk[36 + b * 6 + a] : 0.0) - blk[b * 6 + a];
    }
    for (int I = l; I < n; I += MPE_RIG_LANES) G.X[0][I] = d.racc[12 * (I / 6) + I % 6] - d.racc[12 * (I / 6) + 6 + I % 6];
  }
  // unpivoted LDL^T in place, column by column: one lane the pivot, the column's rows over the lanes
  for (int j = 0; j < n; ++j) {
    RIG_EACH_LANE(l) {
      if (l == 0) {
        double dd = G.L[rig_ba_low(j, j)];
        for (int k = 0; k < j; ++k) dd -= G.L[rig_ba_low(j, k)] * G.L[rig_ba_low(j, k)] * G.L[rig_ba_low(k, k)];
        G.L[rig_ba_low(j, j)] = dd;
      }
    }
    RIG_EACH_LANE(l) {
      for (int i = j + 1 + l; i < n; i += MPE_RIG_LANES) {
        double sacc = G.L[rig_ba_low(i, j)];
        for (int k = 0; k < j; ++k) sacc -= G.L[rig_ba_low(i, k)] * G.L[rig_ba_low(j, k)] * G.L[rig_ba_low(k, k)];
        G.L[rig_ba_low(i, j)] = sacc / G.L[rig_ba_low(j, j)];
      }
    }
  }
  rig_ba_substitute(G, n, 1);
  RIG_EACH_LANE(l) {
    for (int idx = l; idx < (n * (n + 1)) / 2; idx += MPE_RIG_LANES) d.Lf[idx] = G.L[idx];
    for (int I = l; I < n; I += MPE_RIG_LANES) d.eta[I] = G.X[0][I];
  }
}

// the 6 x 6 diagonal block of S^-1 of free camera ci, from the factor the last solve stored
__device__ __forceinline__ void rig_ba_covariance(RigBaSolveLds& G, const RigBaDev& d, int ci) {
  const int n = 6 * d.n_free;
  RIG_EACH_LANE(l) {
    for (int idx = l; idx < (n * (n + 1)) / 2; idx += MPE_RIG_LANES) G.L[idx] = d.Lf[idx];
    for (int idx = l; idx < 6 * n; idx += MPE_RIG_LANES) {
      const int c = idx / n, i = idx - c * n;
      G.X[c][i] = (i == 6 * ci + c) ? 1.0 : 0.0;
    }
  }
  rig_ba_substitute(G, n, 6);
  RIG_EACH_LANE(l) {
    if (l < 36) d.cov[36 * (size_t)ci + l] = G.X[l % 6][6 * ci + l / 6];
  }
}

// ---- update: view f on one lane --------------------------------------------------------------------------------------
__device__ __forceinline__ void rig_ba_update_view(const RigBaDev& d, int f, int chunk_first) {
  const double* rec = d.rec + (d.view_cum[f] - d.view_cum[chunk_first]);
  const unsigned mask = d.view_mask[f];
  double xi[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) xi[a] = rec[a];
  int k = 0;
  for (int fi = 0; fi < d.n_free; ++fi) {
    if (!((mask >> fi) & 1u)) continue;
    const double* Y = rec + MPE_RIG_BA_HEAD + k * MPE_RIG_BA_SLOT + 36;
    const double* eta = d.eta + 6 * fi;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) xi[a] -= Y[a * 6 + b] * eta[b];
    ++k;
  }
  double* Tv = d.T_view + 16 * (size_t)f;
  T34 T;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) T.m[r][c] = Tv[r * 4 + c];
  apply_exp(xi, T);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) Tv[r * 4 + c] = T.m[r][c];
  double mx = -1;  // norm_max, except that a NaN component makes the maximum NaN (and stays): the host stops on it
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double av = fabs(xi[a]);
    if (av > mx || av != av) mx = av;
  }
  d.step[f] = mx;
}

// ---- finish: the cameras' update, the largest step, the sum of squared residuals ------------------------------------------
struct RigBaFinLds {
  double buf[MPE_RIG_LANES];
  double mx[MPE_RIG_LANES];
  double sum;
};

__device__ __forceinline__ void rig_ba_finish(RigBaFinLds& G, const RigBaDev& d, int apply) {
  RIG_EACH_LANE(l) {
    double mx = -1;
    if (apply) {
      if (l < d.n_cam && d.cam_free[l] >= 0) {
        const double* eta = d.eta + 6 * d.cam_free[l];
        double* E = d.cams[l].T_cam_rig;
        T34 T;
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 4; ++c) T.m[r][c] = E[r * 4 + c];
        apply_exp(eta, T);
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 4; ++c) E[r * 4 + c] = T.m[r][c];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          const double av = fabs(eta[a]);
          if (av > mx || av != av) mx = av;
        }
      }
      for (int f = l; f < d.n_views; f += MPE_RIG_LANES) {
        const double av = d.step[f];
        if (av > mx || av != av) mx = av;
      }
    }
    G.mx[l] = mx;
    if (l == 0) G.sum = 0.0;
  }
  for (int f0 = 0; f0 < d.n_views; f0 += MPE_RIG_LANES) {
    RIG_EACH_LANE(l) {
      if (f0 + l < d.n_views) G.buf[l] = d.sse[f0 + l];
    }
    RIG_EACH_LANE(l) {
      if (l == 0) {
        double s = G.sum;
        const int nv = d.n_views - f0 < MPE_RIG_LANES ? d.n_views - f0 : MPE_RIG_LANES;
        for (int v = 0; v < nv; ++v) s += G.buf[v];
        G.sum = s;
      }
    }
  }
  RIG_EACH_LANE(l) {
    if (l == 0) {
      double mx = -1;
      for (int v = 0; v < MPE_RIG_LANES; ++v)
        if (G.mx[v] > mx || G.mx[v] != G.mx[v]) mx = G.mx[v];
      d.out[0] = mx;
      d.out[1] = G.sum;
    }
  }
}
