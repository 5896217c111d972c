// ccmp_fd_newton_phase1.inc — phase 1 of a Newton round on the throughput layout (ten samples / edges x six lanes per wavefront):
// function(x) — sines / cosines, both chains at x, residual — and the loop test of ConstraintFunction.h:68 with its quirks.
// ONE text for project_fd_kernel and geodesic_group_kernel (ccmp_kernels_fd.hip), included into both loop bodies: the two kernels
// cannot drift apart bit-wise, and — being the same tokens in the same place as before — the register allocation of neither
// changed (shared through FUNCTIONS, the general instantiations of both kernels came out with 2.3 KB of scratch: the allocator lost
// the scoping of the pose arrays).  The including loop provides: K, rec, live, writer, r, arm_l, row_l, d_lane, CCMP_FD_BP (the lane's
// base-frame offset: a register in the projector, an LDS slot in the extend step), CCMP_FD_X0_ROWS (1: the chains by rows take the
// short rotation too; 0 in the extend step, which spilled with both copies), active, iter, norm1, norm2; it declares
// `bool x0, cont; double f0, f1;` behind which this text continues.
    // ---- phase 1: function(x) — sines/cosines, both chains, residual ---------------------------
    bool x0_off = false; // some joint of the group sits too close to a multiple of 2 pi for rot_sc_x0 (ccmp_kin.h: rot_x0_round_ok)
    for (int e = r; e < 14; e += kGroup) {
      double s, c;
      const double xe = rec[kX + e];
      ccmp_sincos(xe, &s, &c);
      if (live) { rec[kSC + 2 * e] = s; rec[kSC + 2 * e + 1] = c; }
      x0_off = x0_off || !rot_x0_round_ok(xe, c);
    }
    // wave-uniform, for the whole round: the short form of the general joints' rotations, at x and at every stencil point
    // (groups without a sample have no say)
    bool x0 = false;
    if constexpr (STOCK) x0 = K.rot_x0 != 0 && __builtin_amdgcn_ballot_w64(active && x0_off) == 0ull;
    __syncthreads();
    bool cont = false;
    double f0, f1;
    {
      double T0[12], T1[12], f[2];
      if constexpr (STOCK) {
        // both chains and both tool poses, one matrix row per lane; arm 0's prefix frames stay in LDS for its columns
        if (CCMP_FD_X0_ROWS && x0) chain_rows<true, true>(K, rec, arm_l, row_l, live, 0, d_lane, CCMP_FD_BP);
        else chain_rows<true, false>(K, rec, arm_l, row_l, live, 0, d_lane, CCMP_FD_BP);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 12; k++) { T0[k] = rec[kEE + k]; T1[k] = rec[kEE + 12 + k]; }
      } else {
        chain_at_x<1, false>(K, rec, writer, T1);
        if (writer) {
#pragma unroll
          for (int k = 0; k < 12; k++) rec[kEE + 12 + k] = T1[k];
        }
        chain_at_x<0, true>(K, rec, writer, T0); // arm 0's prefix frames stay in LDS for its columns
        if (writer) {
#pragma unroll
          for (int k = 0; k < 12; k++) rec[kEE + k] = T0[k];
        }
      }
      chain_residual(K, &T0[0], &T0[9], &T1[0], &T1[9], f, nullptr, nullptr);
      f0 = f[0]; f1 = f[1];
      // ---- loop condition of ConstraintFunction.h:68, quirks included -------------------------
      // while (((norm1 = f[0] > tol1) || (norm2 = f[1]) > tol2) && iter++ < maxIterations)
      if (active) {
        const bool c1 = f[0] > K.tol_pos;
        norm1 = c1 ? 1.0 : 0.0;
        bool resid = c1;
        if (!c1) { norm2 = f[1]; resid = f[1] > K.tol_rot; }
        if (resid) { cont = iter < K.max_iter; iter++; }
      }
    }
