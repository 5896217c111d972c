// ccmp_row16_step.inc — the Newton update of a round on the analytic mode's latency layout: the probes, this lane's analytic
// Jacobian column, the 2x2 Gram step (orc_solve_gram) with the SVD-equivalent fallback, this lane's joint of x -= step J^T y.  ONE
// text for project_row16_kernel and geodesic_row16_kernel (see ccmp_row16_eval.inc).  The including scope provides, besides what
// the evaluation needs and declared: aj, sgn, l, cont (this row goes on iterating), updates.
    // ---- analytic Jacobian: probes (every lane, its joint's arm), then this lane's column --------------------------------------
    double J0, J1;
    {
      double u[3] = {0, 0, 0}, n[3] = {0, 0, 0}, aw[3], bw[3];
      if (f[0] > 0.0) {
        const double inv = 1.0 / f[0];
#pragma unroll
        for (int k = 0; k < 3; k++) u[k] = (pc[k] - K.init_p[k]) * inv;
      }
      const double vn = ccmp_sqrt(dot3(dq[0], dq[0], dq[1], dq[1], dq[2], dq[2]));
      if (vn > 0.0) {
        const double sg = (dq[3] < 0.0 ? -1.0 : 1.0) / vn;
#pragma unroll
        for (int k = 0; k < 3; k++) n[k] = dq[k] * sg;
      }
#pragma unroll
      for (int k = 0; k < 3; k++) {
        aw[k] = dot3(T1[3 * k], u[0], T1[3 * k + 1], u[1], T1[3 * k + 2], u[2]);
        bw[k] = dot3(T1[3 * k], n[0], T1[3 * k + 1], n[1], T1[3 * k + 2], n[2]);
      }
      double al[3], bl[3], pl[3], dp[3];
#pragma unroll
      for (int k = 0; k < 3; k++) dp[k] = T0[9 + k] - K.base_p[aj][k];
      mulTvec(K.base_R[aj], aw, al);
      mulTvec(K.base_R[aj], bw, bl);
      mulTvec(K.base_R[aj], dp, pl);
      const double *zo = rec + qZO + 6 * lj;
      const double z0 = zo[0], z1 = zo[1], z2 = zo[2];
      const double r0 = pl[0] - zo[3], r1 = pl[1] - zo[4], r2 = pl[2] - zo[5];
      const double cx = CCMP_FMA(z1, r2, -(z2 * r1));
      const double cy = CCMP_FMA(z2, r0, -(z0 * r2));
      const double cz = CCMP_FMA(z0, r1, -(z1 * r0));
      J0 = sgn * dot3(al[0], cx, al[1], cy, al[2], cz);
      J1 = sgn * dot3(bl[0], z0, bl[1], z1, bl[2], z2);
      rec[qJ + lj] = J0;
      rec[qJ + 14 + lj] = J1;
    }
    // ---- Newton update on the Gram matrix (orc_solve_gram): every lane the three sums, its own component of the step ----------
    {
      double Jr[28], a, d, b, y0, y1;
#pragma unroll
      for (int k = 0; k < 28; k++) Jr[k] = rec[qJ + k];
      gram_sums(Jr, a, d, b);
      const bool well = gram_coeffs(a, d, b, f[0], f[1], y0, y1);
      double dx = CCMP_FMA(y1, J1, y0 * J0);
      if (__builtin_amdgcn_ballot_w64(cont && !well) != 0ull) { // nearly parallel rows (or a NaN): the SVD-equivalent solve, through LDS
        double dxf[14];
        solve_minnorm(Jr, f[0], f[1], dxf);
        if (l == 0) {
#pragma unroll
          for (int k = 0; k < 14; k++) rec[qDX + k] = dxf[k];
        }
        const double own = rec[qDX + lj];
        if (!well) dx = own;
      }
      if (cont) {
        x = CCMP_FMA(-K.step, dx, x);
        updates++;
      }
    }
