// ccmp_fd_newton_phase2.inc — phase 2 of a Newton round on the throughput layout: OMPL's default Constraint::jacobian (one column per
// step, arm 0 then arm 1) and the update x -= 0.30 * J.jacobiSvd().solve(f).  ONE text for project_fd_kernel and
// geodesic_group_kernel (see ccmp_fd_newton_phase1.inc); the including loop provides K, rec, live, writer, r, plus, nstep, arm_l,
// row_l, d_lane, CCMP_FD_BP, x0, cont, f0, f1, updates.
    // ---- phase 2: OMPL's default Constraint::jacobian, one column per step --------------------
    // (STOCK: each piece of the round's kinematics exists twice — with the general joints' rotations in their short form where
    // phase 1 found that every angle of the round admits it (x0, wave-uniform: a scalar branch per piece), as they stand otherwise)
    if constexpr (STOCK) {
      if (x0) jacobian_columns<0, true, true>(K, rec, live, r, plus, nstep);
      else jacobian_columns<0, true, false>(K, rec, live, r, plus, nstep);
    } else jacobian_columns<0, false>(K, rec, live, r, plus, nstep);
    __syncthreads();
    stencil_combine<0>(rec, r, live);
    __syncthreads();
    if constexpr (STOCK) { // re-run by rows: arm 1's lanes stage ITS prefix frames
      if (CCMP_FD_X0_ROWS && x0) chain_rows<false, true>(K, rec, arm_l, row_l, live, 1, d_lane, CCMP_FD_BP);
      else chain_rows<false, false>(K, rec, arm_l, row_l, live, 1, d_lane, CCMP_FD_BP);
    } else {
      double T1[12];
      chain_at_x<1, true>(K, rec, writer, T1); // re-run arm 1's chain to stage ITS prefix frames
    }
    __syncthreads();
    if constexpr (STOCK) {
      if (x0) jacobian_columns<1, true, true>(K, rec, live, r, plus, nstep);
      else jacobian_columns<1, true, false>(K, rec, live, r, plus, nstep);
    } else jacobian_columns<1, false>(K, rec, live, r, plus, nstep);
    __syncthreads();
    stencil_combine<1>(rec, r, live);
    __syncthreads();

    // ---- Newton update: x -= 0.30 * J.jacobiSvd().solve(f) --------------------------------------
    // solve_minnorm (ccmp_solve.h) spread over the group's six lanes instead of run whole by each of them — its operations on
    // its operands in its order (the pieces are ccmp_solve.h's minnorm_*), hence its bits.  Lane r owns columns r, r + 6, r + 12
    // (< 14), the entries of x it updates: it keeps their (row 0, row 1) pairs in registers through both sweeps, rotates them, and
    // writes them back in place (kJ0 / arm 0's sin/cos slots) for the next pass of sums.  A serial sum over the 14 columns is ONE
    // chain in ONE lane, operands from LDS: lanes 0, 1, 2 form a, d, b (lanes 3..5 the same again), published to the group in the
    // prefix frames' region, dead until the next round — one slot per pass and sum, so no pass overwrites what a lane may still
    // read.  The scalar part (rotation angle, thresholds, quotients) is a serial chain with nothing to split: every lane runs it.
    {
      constexpr int kSums = kPre; // [3 passes][a, d, b]
      // (the lane's slots are formed here, every round, from an index the optimiser cannot see through: hoisted out of the Newton
      // loop they would be six more registers held across it, and the kernels are at their budget)
      int rq = r;
      asm volatile("" : "+v"(rq));
      const int kind = rq < 3 ? rq : rq - 3; // 0 pairs (r0, r0) into a, 1 pairs (r1, r1) into d, 2 pairs (r0, r1) into b
      const int e0 = kJ0 + 2 * rq, e1 = rq == 0 ? kJ0 + 12 : kSC + 2 * (rq - 1) /* column rq + 6 */, e2 = kSC + (rq == 0 ? 10 : 12) /* 12 or 13 */;
      const bool own2 = live && rq < 2; // lanes 2..5 carry column 13 along without ever storing it
      double v0[3], v1[3], g0 = f0, g1 = f1;
      v0[0] = rec[e0]; v1[0] = rec[e0 + 1];
      v0[1] = rec[e1]; v1[1] = rec[e1 + 1];
      v0[2] = rec[e2]; v1[2] = rec[e2 + 1];
      const double *px = rec + (kind == 1 ? 1 : 0), *py = rec + (kind != 0 ? 1 : 0);
#pragma unroll
      for (int pass = 0; pass < 3; pass++) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 14; j++) acc = minnorm_sum_step(px[minnorm_group_slot(j, kJ0, kSC)], py[minnorm_group_slot(j, kJ0, kSC)], acc);
        if (live && rq < 3) rec[kSums + 3 * pass + kind] = acc;
        __syncthreads();
        const double a = rec[kSums + 3 * pass], d = rec[kSums + 3 * pass + 1];
        if (pass < 2) {
          const double b = rec[kSums + 3 * pass + 2];
          if (b != 0.0) { // per group
            double c, s;
            minnorm_sweep_coeffs(a, d, b, c, s);
#pragma unroll
            for (int n = 0; n < 3; n++) minnorm_rotate(c, s, v0[n], v1[n]);
            minnorm_rotate(c, s, g0, g1);
            if (live) {
              rec[e0] = v0[0]; rec[e0 + 1] = v1[0];
              rec[e1] = v0[1]; rec[e1 + 1] = v1[1];
            }
            if (own2) { rec[e2] = v0[2]; rec[e2 + 1] = v1[2]; }
          }
          __syncthreads();
        } else {
          double k0, k1;
          minnorm_final_coeffs(a, d, g0, g1, k0, k1);
          if (cont) {
            double *xr = rec + kX + rq;
            xr[0] = CCMP_FMA(-K.step, minnorm_dx(k0, k1, v0[0], v1[0]), xr[0]);
            xr[6] = CCMP_FMA(-K.step, minnorm_dx(k0, k1, v0[1], v1[1]), xr[6]);
            if (own2) xr[12] = CCMP_FMA(-K.step, minnorm_dx(k0, k1, v0[2], v1[2]), xr[12]);
            updates++;
          }
        }
      }
    }
    __syncthreads();
