// ccmp_row16_eval.inc — the function evaluation of a Newton round on the analytic mode's latency layout (sixteen lanes, one DPP
// row, per sample; ccmp_kernels_fast.hip says what each lane does): joint rotations, one row of each arm's chain and hand pose,
// the two world poses and the residual.  ONE text for project_row16_kernel and geodesic_row16_kernel, included into both loop
// bodies (the idiom of ccmp_geo_edge_body.inc / ccmp_fd_newton_phase1.inc): the two kernels cannot drift apart bit-wise, and the
// projector compiles to what it compiled to before (the same tokens in the same place).  The including scope provides: K, rec
// (the row's LDS record, layout q*), x (this lane's joint of the iterate), lj, ax, ap, ac, rc, cee, cRt, cd, cbp; this text
// declares T0, T1, f, dq, pc, which ccmp_row16_step.inc reads.
    // ---- function(x).  Joint lanes: sine, cosine, joint rotation (lanes 14, 15 shadow lane 13: same values, same words) ------
    {
      double s, c, Rj[9];
      ccmp_sincos(x, &s, &c);
      rot_sc(ax, ap, s, c, Rj);
#pragma unroll
      for (int k = 0; k < 9; k++) rec[qRJ + 9 * lj + k] = Rj[k];
    }
    // ---- chain lanes: one row of the arm's frame through the seven joints, then one row of the hand pose ---------------------
    {
      double R0 = rc == 0 ? 1.0 : 0.0, R1 = rc == 1 ? 1.0 : 0.0, R2 = rc == 2 ? 1.0 : 0.0, o = 0.0;
      // the arm's joint rotations in two batches (four joints, then three): two LDS latencies instead of seven
#pragma unroll
      for (int h = 0; h < 2; h++) {
        constexpr int kFirst[2] = {0, 4}, kCount[2] = {4, 3};
        double Rj[4][9];
#pragma unroll
        for (int i = 0; i < kCount[h]; i++)
#pragma unroll
          for (int k = 0; k < 9; k++) Rj[i][k] = rec[qRJ + 9 * (ac * 7 + kFirst[h] + i) + k];
#pragma unroll
        for (int ii = 0; ii < kCount[h]; ii++) {
          const int i = kFirst[h] + ii;
          const double *off = K.offset[ac][i], *a = K.axis[ac][i];
          o = dot3acc(o, R0, off[0], R1, off[1], R2, off[2]);
          const double zr = dot3(R0, a[0], R1, a[1], R2, a[2]);
          rec[qZO + (ac * 7 + i) * 6 + rc] = zr;
          rec[qZO + (ac * 7 + i) * 6 + 3 + rc] = o;
          const double n0 = dot3(R0, Rj[ii][0], R1, Rj[ii][3], R2, Rj[ii][6]);
          const double n1 = dot3(R0, Rj[ii][1], R1, Rj[ii][4], R2, Rj[ii][7]);
          const double n2 = dot3(R0, Rj[ii][2], R1, Rj[ii][5], R2, Rj[ii][8]);
          R0 = n0; R1 = n1; R2 = n2;
        }
      }
      // the hand frame in the arm's base frame (getTranslation / getRotation), one row
      const double pf = dot3acc(o, R0, cee[0], R1, cee[1], R2, cee[2]);
      const double f0 = dot3(R0, cRt[0], R1, cRt[3], R2, cRt[6]);
      const double f1 = dot3(R0, cRt[1], R1, cRt[4], R2, cRt[7]);
      const double f2 = dot3(R0, cRt[2], R1, cRt[5], R2, cRt[8]);
      double *T = rec + qT + 12 * ac;
      if (DIAG) { // t_wb * T with t_wb.linear() = diag(d): d_r * Rf[r][c], fma(d_r, pf[r], base_p[r]) (the general product adds exact zeros)
        T[3 * rc] = cd * f0;
        T[3 * rc + 1] = cd * f1;
        T[3 * rc + 2] = cd * f2;
        T[9 + rc] = CCMP_FMA(cd, pf, cbp);
      } else {
        T[3 * rc] = f0;
        T[3 * rc + 1] = f1;
        T[3 * rc + 2] = f2;
        T[9 + rc] = pf;
      }
    }
    // ---- all lanes: the two world poses, the residual, the loop condition ------------------------------------------------------
    double T0[12], T1[12], f[2], dq[4], pc[3];
    if (DIAG) {
#pragma unroll
      for (int k = 0; k < 12; k++) { T0[k] = rec[qT + k]; T1[k] = rec[qT + 12 + k]; }
    } else {
#pragma unroll
      for (int arm = 0; arm < 2; arm++) {
        double Rf[9], pf[3], *Tw = arm ? T1 : T0;
#pragma unroll
        for (int k = 0; k < 9; k++) Rf[k] = rec[qT + 12 * arm + k];
#pragma unroll
        for (int k = 0; k < 3; k++) pf[k] = rec[qT + 12 * arm + 9 + k];
        mul33(K.base_R[arm], Rf, Tw);
        Tw[9] = K.base_p[arm][0]; Tw[10] = K.base_p[arm][1]; Tw[11] = K.base_p[arm][2];
        mulvec_acc(K.base_R[arm], pf, Tw + 9);
      }
    }
    chain_residual(K, &T0[0], &T0[9], &T1[0], &T1[9], f, dq, pc);
