// mpe_body_ba.h — the logic of the k_body_ba_* kernels (mpe_k3.hip): the LED positions of a body calibrated from the
// sequences it was tracked in (mpe_body_calibrate).  The bundle adjustment of mpe_rig_ba.h with the other block of
// unknowns: a left twist xi_f on every view pose T_f (rig <- marker frame) and an additive delta_m on every FREE marker
// p_m; the extrinsics E_c = [R_c | t_c] (camera <- rig) are fixed.  Row j of view f = (camera c, marker m, pixel uv):
//   q = E_c T_f p_m,  e = uv - project(K_c, q),  (a, b) = rig_ba_row's pair at q with K_c,
//   Jp = (a, b) Ad(E_c)             = d e / d xi_f     (what rig_row stores),
//   Jm = (a, b)[:, 0:3] R_c R_f     = d e / d delta_m  (= Jp[:, 0:3] R_f).
// Gauss-Newton with a Schur complement over the view poses, per iteration five steps, each a launch of its own:
//   linearise (one wave per view)   U_f = sum Jp^T Jp, g_f = sum Jp^T e, per free marker m of the view W_fm = sum Jp^T Jm
//                                   (6 x 3), V_fm = sum Jm^T Jm (packed 6), h_fm = sum Jm^T e — every entry summed over
//                                   the rows in row order —, LDL^T of U_f, Y_fm = U_f^-1 W_fm, z_f = U_f^-1 g_f, sse_f
//   reduce (one wave per 3 x 3 block (i, j), i <= j, of the free markers)
//                                   accS_ij = sum_f W_fi^T Y_fj, on the diagonal also accV_i, acch_i, accz_i = sum_f
//                                   W_fi^T z_f: every entry by ONE lane over the views in view order
//   solve (one wave)                S = V - accS, r = h - accz.  S is singular: the body frame is arbitrary (and the size
//                                   too when no view holds two cameras).  Inner constraints: c = centroid of the free
//                                   markers, d_m = p_m - c, N = [translations (e_k)_m | rotations (e_k x d_m)_m | when
//                                   scale is held (d_m)_m], w = sum diag S / (3 n_free), M = S + w N N^T, unpivoted LDL^T
//                                   (packed lower triangle), delta = M^-1 r  (r is orthogonal to the null vectors of S, so
//                                   N^T delta = 0 for them; a scale that is held although the rig observes it takes one
//                                   more column: u = M^-1 n7, delta -= u (n7 . delta) / (n7 . u))
//   update (one lane per view)      xi_f = z_f - sum_m Y_fm delta_m, T_f <- exp(xi_f) T_f (apply_exp), the view's max |xi|
//   finish (one wave)               p_m <- p_m + delta_m, the largest |step| of all delta and xi, the sum of sse_f in
//                                   view order -> the two doubles the host reads to decide whether to stop
// and once behind the last iteration: covariance (one wave per free marker) = the marker's 3 x 3 diagonal block of
// M^-1 - M^-1 N (N^T M^-1 N)^-1 N^T M^-1 from the stored factor and gauge — for the null vectors of S that is S^+ = M^-1 -
// (1 / w) N (N^T N)^-2 N^T with N^T N block diagonal: n_free I_3, B = sum (|d|^2 I - d d^T); the scale column takes
// u u^T / (n7 . u), which is the same thing, n7 n7^T / (w (sum |d|^2)^2), while the size is unobservable.  No atomics
// anywhere: an entry's value is fixed by the view, row and marker order alone.
//
// The form is mpe_rig_gn.h's (RIG_EACH_LANE phases), so the CPU tier runs THIS text (tests/host/body_ba_host.cpp).  No
// #include and no namespace of its own: the text goes behind mpe_rig_ba.h (rig_ba_row, rig_ba_solve6, rig_ba_untri,
// rig_ba_pair, rig_ba_low, rig_ba_slot, rig_ba_substitute, RigBaSolveLds, RigBaFinLds) and needs mpe_body_ba_dev.h in front.
//
// A view's record (doubles): [z 6 | sse | 0] then per free marker of the view, ascending, a slot [W 18 (W[a][b], a the
// pose component) | Y 18 | V 6 (upper triangle, row-major) | h 3].  View f's record starts at rec + (view_cum[f] -
// view_cum[first]).
struct BodyBaLinLds {
  double J[MPE_RIG_MAX_ROWS][20];  // per row: Jp0[6], Jp1[6], Jm0[3], Jm1[3], e0, e1
  RigCam cam[MPE_RIG_MAX_CAMERAS];
  double R[MPE_BODY_BA_HEAD + MPE_MAX_MARKERS * MPE_BODY_BA_SLOT];  // the record as it grows
  double Ug[28];  // upper triangle of U (21), g (6), sse
  double L[6][6];
  double D[6];
  double T[12];
  unsigned char rs[MPE_RIG_MAX_ROWS];  // per row: slot of its marker
};
static_assert(sizeof(BodyBaLinLds) <= sizeof(RigBaLinLds), "the linearisation stays within the extrinsic one's LDS");

__device__ __forceinline__ int body_ba_tri3(int r, int c) { return r * 3 - (r * (r - 1)) / 2 + (c - r); }  // r <= c

// row (marker at p, pixel at uv) of camera C under the view pose T: rig_ba_row's arithmetic, then the marker's pair
__device__ __forceinline__ void body_ba_row(const RigCam& C, const T34& T, const double* p, const double* uv, double* Jr) {
  double t[26];
  rig_ba_row(C, T, p, uv, t);
#pragma unroll
  for (int k = 0; k < 12; ++k) Jr[k] = t[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    Jr[12 + k] = t[0] * T.m[0][k] + t[1] * T.m[1][k] + t[2] * T.m[2][k];
    Jr[15 + k] = t[6] * T.m[0][k] + t[7] * T.m[1][k] + t[8] * T.m[2][k];
  }
  Jr[18] = t[24];
  Jr[19] = t[25];
}

// ---- linearise: used view f on one wave ---------------------------------------------------------------------------
__device__ __forceinline__ void body_ba_linearise(BodyBaLinLds& G, const BodyBaDev& d, int f, int chunk_first) {
  const int b0 = d.view_begin[f];
  int n_rows = d.view_begin[f + 1] - b0;
  n_rows = n_rows < 0 ? 0 : (n_rows > MPE_RIG_MAX_ROWS ? MPE_RIG_MAX_ROWS : n_rows);
  const unsigned mask = d.view_mask[f] & 0xffffu;
  const int n_slots = __builtin_popcount(mask);
  const int n_rec = MPE_BODY_BA_HEAD + n_slots * MPE_BODY_BA_SLOT;
  const int* row_cam = d.row_cam + b0;
  const int* row_free = d.row_free + b0;
  const double* row_uv = d.row_uv + 2 * (size_t)b0;
  double* rec = d.rec + (d.view_cum[f] - d.view_cum[chunk_first]);
  RIG_EACH_LANE(l) {
    if (l < d.n_cam) rig_stage_camera(d.cams[l], G.cam[l]);
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
      const int fi = row_free[j];
      body_ba_row(G.cam[row_cam[j]], T, d.markers + 3 * (size_t)d.free_marker[fi], row_uv + 2 * j, G.J[j]);
      G.rs[j] = (unsigned char)rig_ba_slot(mask, fi);
    }
  }
  // (b) U, g, sse over all rows, and per marker slot W, V, h over the marker's rows: one entry per lane, rows in row order
  RIG_EACH_LANE(l) {
    if (l < 28) {
      double acc = 0;
      if (l < 21) {
        int r, c;
        rig_ba_untri(l, r, c);
        for (int j = 0; j < n_rows; ++j) acc += G.J[j][r] * G.J[j][c] + G.J[j][6 + r] * G.J[j][6 + c];
      } else if (l < 27) {
        const int r = l - 21;
        for (int j = 0; j < n_rows; ++j) acc += G.J[j][r] * G.J[j][18] + G.J[j][6 + r] * G.J[j][19];
      } else {
        for (int j = 0; j < n_rows; ++j) acc += G.J[j][18] * G.J[j][18] + G.J[j][19] * G.J[j][19];
      }
      G.Ug[l] = acc;
    }
  }
  RIG_EACH_LANE(l) {
    if (l < 54) {  // entry l % 27 of the even (l < 27) or the odd slots: the entry is J[i0] * J[i1] + J[i0b] * J[i1b]
      const int en = l % 27, half = l / 27;
      int i0, i0b, i1, i1b, off;
      if (en < 18) {
        i0 = en / 3, i0b = 6 + i0;
        i1 = 12 + en % 3, i1b = i1 + 3;
        off = en;
      } else if (en < 24) {
        const int t = en - 18;
        const int r = t < 3 ? 0 : (t < 5 ? 1 : 2), c = t < 3 ? t : (t < 5 ? t - 2 : 2);
        i0 = 12 + r, i0b = 15 + r;
        i1 = 12 + c, i1b = 15 + c;
        off = 36 + t;
      } else {
        i0 = 12 + (en - 24), i0b = i0 + 3;
        i1 = 18, i1b = 19;
        off = 42 + (en - 24);
      }
      for (int j = 0; j < n_rows; ++j) {
        const int s = G.rs[j];
        if ((s & 1) == half) G.R[MPE_BODY_BA_HEAD + s * MPE_BODY_BA_SLOT + off] += G.J[j][i0] * G.J[j][i1] + G.J[j][i0b] * G.J[j][i1b];
      }
    }
  }
  // (c) unpivoted LDL^T of U, column by column (rig_ba_linearise's phase (c))
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
    for (int r = l; r < 1 + 3 * n_slots; r += MPE_RIG_LANES) {
      if (r == 0) {
        rig_ba_solve6(G, G.Ug + 21, 1, G.R, 1);
        G.R[6] = G.Ug[27];
      } else {
        const int k = (r - 1) / 3, b = (r - 1) % 3;
        double* S = G.R + MPE_BODY_BA_HEAD + k * MPE_BODY_BA_SLOT;
        rig_ba_solve6(G, S + b, 3, S + 18 + b, 3);
      }
    }
  }
  RIG_EACH_LANE(l) {
    for (int i = l; i < n_rec; i += MPE_RIG_LANES) rec[i] = G.R[i];
    if (l == 0) d.sse[f] = G.Ug[27];
  }
}

// ---- reduce: block (mi, mj), mi <= mj, of the free markers over the views [first, first + count) ----------------------
struct BodyBaRedLds {
  double S[MPE_RIG_BA_CHUNK][51];  // per staged view: W_i 18, Y_j 18, and on the diagonal V_i 6, h_i 3, z 6
  double accS[9], accV[9], acch[3], accz[3];
  long long oi[MPE_RIG_BA_CHUNK], oj[MPE_RIG_BA_CHUNK], ob[MPE_RIG_BA_CHUNK];  // where the view's slots / record start
  unsigned char has[MPE_RIG_BA_CHUNK];
};

__device__ __forceinline__ void body_ba_reduce(BodyBaRedLds& G, const BodyBaDev& d, int mi, int mj, int first, int count,
                                               int restart) {
  const bool diag = mi == mj;
  const int items = diag ? 51 : 36;
  double* Sacc = d.Sacc + 18 * (size_t)rig_ba_pair(mi, mj, d.n_free);
  double* racc = d.racc + 6 * (size_t)mi;
  const unsigned need = (1u << mi) | (1u << mj);
  RIG_EACH_LANE(l) {
    if (l < 9) {
      G.accS[l] = restart ? 0.0 : Sacc[l];
      G.accV[l] = restart ? 0.0 : Sacc[9 + l];
    } else if (l < 12) {
      G.acch[l - 9] = (restart || !diag) ? 0.0 : racc[l - 9];
      G.accz[l - 9] = (restart || !diag) ? 0.0 : racc[3 + l - 9];
    }
  }
  for (int f0 = first; f0 < first + count; f0 += MPE_RIG_BA_CHUNK) {
    const int nv = (first + count - f0) < MPE_RIG_BA_CHUNK ? (first + count - f0) : MPE_RIG_BA_CHUNK;
    // which of these views hold both markers, and where their slots are: a view per lane
    RIG_EACH_LANE(l) {
      for (int v = l; v < nv; v += MPE_RIG_LANES) {
        const int f = f0 + v;
        const unsigned mask = d.view_mask[f] & 0xffffu;
        const long long base = d.view_cum[f] - d.view_cum[first];
        G.has[v] = (mask & need) == need ? 1 : 0;
        G.ob[v] = base;
        G.oi[v] = base + MPE_BODY_BA_HEAD + rig_ba_slot(mask, mi) * MPE_BODY_BA_SLOT;
        G.oj[v] = base + MPE_BODY_BA_HEAD + rig_ba_slot(mask, mj) * MPE_BODY_BA_SLOT;
      }
    }
    // stage what the block needs of them: consecutive lanes read consecutive doubles of a record, eight loads in flight
    // per lane (rig_ba_reduce's staging)
    RIG_EACH_LANE(l) {
      for (int i0 = l; i0 < nv * items; i0 += 8 * MPE_RIG_LANES) {
        double val[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int idx = i0 + u * MPE_RIG_LANES;
          val[u] = 0.0;
          if (idx < nv * items) {
            const int v = idx / items, e = idx - v * items;
            if (G.has[v]) val[u] = e < 18 ? d.rec[G.oi[v] + e] : (e < 36 ? d.rec[G.oj[v] + e] : (e < 45 ? d.rec[G.oi[v] + e] : d.rec[G.ob[v] + (e - 45)]));
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
      if (l < 9) {
        const int a = l / 3, b = l % 3;
        const int t = a <= b ? body_ba_tri3(a, b) : body_ba_tri3(b, a);
        double s = G.accS[l], vv = G.accV[l];
        for (int v = 0; v < nv; ++v) {
          if (!G.has[v]) continue;
          double p = 0;
#pragma unroll
          for (int k = 0; k < 6; ++k) p += G.S[v][k * 3 + a] * G.S[v][18 + k * 3 + b];
          s += p;
          if (diag) vv += G.S[v][36 + t];
        }
        G.accS[l] = s;
        G.accV[l] = vv;
      } else if (l < 12 && diag) {
        const int a = l - 9;
        double hh = G.acch[a], zz = G.accz[a];
        for (int v = 0; v < nv; ++v) {
          if (!G.has[v]) continue;
          double p = 0;
#pragma unroll
          for (int k = 0; k < 6; ++k) p += G.S[v][k * 3 + a] * G.S[v][45 + k];
          hh += G.S[v][42 + a];
          zz += p;
        }
        G.acch[a] = hh;
        G.accz[a] = zz;
      }
    }
  }
  RIG_EACH_LANE(l) {
    if (l < 9) {
      Sacc[l] = G.accS[l];
      Sacc[9 + l] = G.accV[l];
    } else if (l < 12 && diag) {
      racc[l - 9] = G.acch[l - 9];
      racc[3 + l - 9] = G.accz[l - 9];
    }
  }
}

// ---- solve and covariance: the reduced system with its inner constraints on one wave ---------------------------------------
struct BodyBaSolveLds {
  RigBaSolveLds S;                                    // the packed triangle and the right-hand sides (rig_ba_substitute)
  double N[MPE_BODY_BA_MAX_GAUGE][MPE_BODY_BA_MAX_N];  // the constraints, one per row
  double Dm[MPE_MAX_MARKERS][3];                      // d_m = p_m - c
  double c[3];
  double w, s2;
  double sa, sb;             // scale held: n7 . delta0 and n7 . u, u = M^-1 n7 (n7 the scale column)
  double B[9], Bi[9], Q[9];  // the rotations' block of N^T N, its inverse, its inverse squared
};
static_assert(MPE_BODY_BA_MAX_N <= MPE_RIG_BA_MAX_N && MPE_BODY_BA_TRI <= MPE_RIG_BA_TRI, "RigBaSolveLds holds the marker system");

__device__ __forceinline__ void body_ba_solve(BodyBaSolveLds& G, const BodyBaDev& d) {
  const int nf = d.n_free, n = 3 * nf;
  const int n_con = d.scale_held ? 7 : 6;
  // S = V - accS (lower triangle from the stored upper blocks), r = h - accz
  RIG_EACH_LANE(l) {
    for (int idx = l; idx < (n * (n + 1)) / 2; idx += MPE_RIG_LANES) {
      int I = 0;
      while ((I + 1) * (I + 2) / 2 <= idx) ++I;
      const int Jc = idx - (I * (I + 1)) / 2;
      const int i = I / 3, a = I - 3 * i, j = Jc / 3, b = Jc - 3 * j;  // j <= i: block (j, i), its entry (b, a)
      const double* blk = d.Sacc + 18 * (size_t)rig_ba_pair(j, i, nf);
      G.S.L[idx] = (i == j ? blk[9 + b * 3 + a] : 0.0) - blk[b * 3 + a];
    }
    for (int I = l; I < n; I += MPE_RIG_LANES) G.S.X[0][I] = d.racc[6 * (I / 3) + I % 3] - d.racc[6 * (I / 3) + 3 + I % 3];
  }
  // the centroid of the free markers and w: each summed by one lane, in marker order
  RIG_EACH_LANE(l) {
    if (l < 3) {
      double s = 0;
      for (int m = 0; m < nf; ++m) s += d.markers[3 * (size_t)d.free_marker[m] + l];
      G.c[l] = s / (double)nf;
    } else if (l == 3) {
      double s = 0;
      for (int I = 0; I < n; ++I) s += G.S.L[rig_ba_low(I, I)];
      G.w = s / (double)n;
    }
  }
  RIG_EACH_LANE(l) {
    if (l < n) G.Dm[l / 3][l % 3] = d.markers[3 * (size_t)d.free_marker[l / 3] + l % 3] - G.c[l % 3];
  }
  // N, and what the covariance needs of N^T N
  RIG_EACH_LANE(l) {
    for (int idx = l; idx < MPE_BODY_BA_MAX_GAUGE * n; idx += MPE_RIG_LANES) {
      const int k = idx / n, I = idx - k * n, m = I / 3, a = I - 3 * m;
      const double* dm = G.Dm[m];
      double v;
      if (k < 3) v = a == k ? 1.0 : 0.0;
      else if (k < 6) {
        const int e = k - 3;  // (e_e x d)_a
        v = a == e ? 0.0 : (a == (e + 1) % 3 ? dm[(e + 2) % 3] : -dm[(e + 1) % 3]);
      } else v = d.scale_held ? dm[a] : 0.0;
      G.N[k][I] = v;
    }
    if (l < 9) {
      const int j = l / 3, k = l % 3;
      double s = 0;
      for (int m = 0; m < nf; ++m) {
        const double* dm = G.Dm[m];
        const double q = dm[0] * dm[0] + dm[1] * dm[1] + dm[2] * dm[2];
        s += (j == k ? q : 0.0) - dm[j] * dm[k];
      }
      G.B[l] = s;
    } else if (l == 9) {
      double s = 0;
      for (int m = 0; m < nf; ++m) s += G.Dm[m][0] * G.Dm[m][0] + G.Dm[m][1] * G.Dm[m][1] + G.Dm[m][2] * G.Dm[m][2];
      G.s2 = s;
    }
  }
  // M = S + w N N^T
  RIG_EACH_LANE(l) {
    for (int idx = l; idx < (n * (n + 1)) / 2; idx += MPE_RIG_LANES) {
      int I = 0;
      while ((I + 1) * (I + 2) / 2 <= idx) ++I;
      const int Jc = idx - (I * (I + 1)) / 2;
      double s = 0;
      for (int k = 0; k < n_con; ++k) s += G.N[k][I] * G.N[k][Jc];
      G.S.L[idx] += G.w * s;
    }
    if (d.scale_held)
      for (int I = l; I < n; I += MPE_RIG_LANES) G.S.X[1][I] = G.N[6][I];
  }
  // unpivoted LDL^T in place, column by column: one lane the pivot, the column's rows over the lanes
  for (int j = 0; j < n; ++j) {
    RIG_EACH_LANE(l) {
      if (l == 0) {
        double dd = G.S.L[rig_ba_low(j, j)];
        for (int k = 0; k < j; ++k) dd -= G.S.L[rig_ba_low(j, k)] * G.S.L[rig_ba_low(j, k)] * G.S.L[rig_ba_low(k, k)];
        G.S.L[rig_ba_low(j, j)] = dd;
      }
    }
    RIG_EACH_LANE(l) {
      for (int i = j + 1 + l; i < n; i += MPE_RIG_LANES) {
        double sacc = G.S.L[rig_ba_low(i, j)];
        for (int k = 0; k < j; ++k) sacc -= G.S.L[rig_ba_low(i, k)] * G.S.L[rig_ba_low(j, k)] * G.S.L[rig_ba_low(k, k)];
        G.S.L[rig_ba_low(i, j)] = sacc / G.S.L[rig_ba_low(j, j)];
      }
    }
  }
  // delta0 = M^-1 r and, when scale is held, u = M^-1 n7.  The six columns of the frame are null vectors of S, r is
  // orthogonal to them and N^T delta0 = 0 there whatever w is.  The scale column is one only while the size is
  // unobservable; held on a rig that observes it, the constraint takes the step delta = delta0 - u (n7 . delta0) / (n7 . u)
  // (the same thing when it is a null vector: n7 . delta0 = 0 then).
  rig_ba_substitute(G.S, n, d.scale_held ? 2 : 1);
  RIG_EACH_LANE(l) {
    if (l < 2 && d.scale_held) {
      double s = 0;
      for (int I = 0; I < n; ++I) s += G.N[6][I] * G.S.X[l][I];
      if (l == 0) G.sa = s;
      else G.sb = s;
    }
  }
  RIG_EACH_LANE(l) {
    for (int idx = l; idx < (n * (n + 1)) / 2; idx += MPE_RIG_LANES) d.Lf[idx] = G.S.L[idx];
    for (int I = l; I < n; I += MPE_RIG_LANES) {
      d.delta[I] = d.scale_held ? G.S.X[0][I] - G.S.X[1][I] * (G.sa / G.sb) : G.S.X[0][I];
      d.gauge[16 + MPE_BODY_BA_MAX_GAUGE * MPE_BODY_BA_MAX_N + I] = d.scale_held ? G.S.X[1][I] : 0.0;
    }
    for (int idx = l; idx < MPE_BODY_BA_MAX_GAUGE * n; idx += MPE_RIG_LANES) {
      const int k = idx / n, I = idx - k * n;
      d.gauge[16 + k * MPE_BODY_BA_MAX_N + I] = G.N[k][I];
    }
    if (l < 16) d.gauge[l] = l == 0 ? G.w : (l == 1 ? (double)n_con : (l == 2 ? G.s2 : (l < 12 ? G.B[l - 3] : (l == 12 && d.scale_held ? G.sb : 0.0))));
  }
}

// the 3 x 3 diagonal block of S^+ of free marker mi, from the factor and the gauge the last solve stored
__device__ __forceinline__ void body_ba_covariance(BodyBaSolveLds& G, const BodyBaDev& d, int mi) {
  const int nf = d.n_free, n = 3 * nf;
  RIG_EACH_LANE(l) {
    for (int idx = l; idx < (n * (n + 1)) / 2; idx += MPE_RIG_LANES) G.S.L[idx] = d.Lf[idx];
    for (int idx = l; idx < 3 * n; idx += MPE_RIG_LANES) {
      const int c = idx / n, i = idx - c * n;
      G.S.X[c][i] = (i == 3 * mi + c) ? 1.0 : 0.0;
    }
    for (int idx = l; idx < MPE_BODY_BA_MAX_GAUGE * 3; idx += MPE_RIG_LANES) {
      const int k = idx / 3, a = idx - 3 * k;  // the marker's three rows of N only; u in the place of the scale column
      G.N[k][a] = d.gauge[16 + (k < 6 ? k : MPE_BODY_BA_MAX_GAUGE) * MPE_BODY_BA_MAX_N + 3 * mi + a];
    }
    if (l < 9) G.B[l] = d.gauge[3 + l];
    if (l == 9) G.w = d.gauge[0];
    if (l == 10) G.sb = d.gauge[12];
  }
  rig_ba_substitute(G.S, n, 3);
  RIG_EACH_LANE(l) {
    if (l < 9) {  // the inverse of B: cofactors over the determinant
      const int r = l / 3, c = l % 3;
      const double* B = G.B;
      const double det = B[0] * (B[4] * B[8] - B[5] * B[7]) - B[1] * (B[3] * B[8] - B[5] * B[6]) + B[2] * (B[3] * B[7] - B[4] * B[6]);
      const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
      G.Bi[c * 3 + r] = (B[r1 * 3 + c1] * B[r2 * 3 + c2] - B[r1 * 3 + c2] * B[r2 * 3 + c1]) / det;
    }
  }
  RIG_EACH_LANE(l) {
    if (l < 9) {
      const int r = l / 3, c = l % 3;
      G.Q[l] = G.Bi[r * 3] * G.Bi[c] + G.Bi[r * 3 + 1] * G.Bi[3 + c] + G.Bi[r * 3 + 2] * G.Bi[6 + c];
    }
  }
  RIG_EACH_LANE(l) {
    if (l < 9) {
      const int a = l / 3, b = l % 3;
      double corr = a == b ? 1.0 / ((double)nf * (double)nf) : 0.0;
      for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k) corr += G.N[3 + j][a] * G.Q[j * 3 + k] * G.N[3 + k][b];
      double val = G.S.X[b][3 * mi + a] - corr / G.w;
      if (d.scale_held) val -= G.N[6][a] * G.N[6][b] / G.sb;
      d.cov[9 * (size_t)mi + l] = val;
    }
  }
}

// ---- update: view f on one lane --------------------------------------------------------------------------------------
__device__ __forceinline__ void body_ba_update_view(const BodyBaDev& d, int f, int chunk_first) {
  const double* rec = d.rec + (d.view_cum[f] - d.view_cum[chunk_first]);
  const unsigned mask = d.view_mask[f] & 0xffffu;
  double xi[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) xi[a] = rec[a];
  int k = 0;
  for (int fi = 0; fi < d.n_free; ++fi) {
    if (!((mask >> fi) & 1u)) continue;
    const double* Y = rec + MPE_BODY_BA_HEAD + k * MPE_BODY_BA_SLOT + 18;
    const double* dl = d.delta + 3 * fi;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) xi[a] -= Y[a * 3 + b] * dl[b];
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

// ---- finish: the markers' update, the largest step, the sum of squared residuals ----------------------------------------
__device__ __forceinline__ void body_ba_finish(RigBaFinLds& G, const BodyBaDev& d, int apply) {
  RIG_EACH_LANE(l) {
    double mx = -1;
    if (apply) {
      if (l < d.n_free) {
        const double* dl = d.delta + 3 * l;
        double* p = d.markers + 3 * (size_t)d.free_marker[l];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          p[a] = p[a] + dl[a];
          const double av = fabs(dl[a]);
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
