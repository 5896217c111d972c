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
    if constexpr (STOCK && CCMP_FD_ROWS) { // re-run by rows: arm 1's lanes stage ITS prefix frames
      if (CCMP_FD_X0_ROWS && x0) chain_rows<false, true>(K, rec, arm_l, row_l, live, 1, d_lane, CCMP_FD_BP);
      else chain_rows<false, false>(K, rec, arm_l, row_l, live, 1, d_lane, CCMP_FD_BP);
    } else {
      double T1[12];
      chain_at_x<1, true, STOCK>(K, rec, writer, T1); // re-run arm 1's chain to stage ITS prefix frames
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
    {
      double Jr[28], dx[14];
#pragma unroll
      for (int j = 0; j < 7; j++) {
        Jr[j] = rec[kJ0 + 2 * j];
        Jr[14 + j] = rec[kJ0 + 2 * j + 1];
        Jr[7 + j] = rec[kSC + 2 * j];
        Jr[21 + j] = rec[kSC + 2 * j + 1];
      }
      solve_minnorm(Jr, f0, f1, dx);
      if (cont) {
#pragma unroll
        for (int e = 0; e < 14; e++)
          if (e % kGroup == r) rec[kX + e] = CCMP_FMA(-K.step, dx[e], rec[kX + e]);
        updates++;
      }
    }
    __syncthreads();
