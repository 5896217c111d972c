// ccmp_fd_project_finish.inc — the projector's finish block on the throughput layout: a sample whose loop test (phase 1) has ended it
// is tested for jointValid and written back — row, flag, iteration count — and its group is free again.  ONE text for both loops of
// project_fd_kernel (ccmp_kernels_fd.hip: the whole / head loop and the resume loop), included behind ccmp_fd_newton_phase1.inc; the
// including loop provides K, rec, live, g, r, leader, active, cont, idx, updates, norm1, norm2, kStateRow / kStateTag (where the head
// marks a row finished) and the kernel's arguments.
    // ---- finished groups: jointValid, write-back --------------------------------------------
    {
      const bool fin = active && !cont;
      bool bad = false;
      if constexpr (PART == kFdHead) idx = head_sample(g);
      if (fin) {
#pragma unroll
        for (int e = 0; e < 14; e++) {
          if (e % kGroup == r) { // e is a compile-time constant here: limits come from SGPRs
            const double v = rec[kX + e];
            if (v < K.lbe[e % 7]) bad = true;
            if (v > K.ube[e % 7]) bad = true;
          }
        }
        // row write-back in 16-B pieces: 96 contiguous bytes per group in one instruction + the last piece
        double2 *row = reinterpret_cast<double2 *>(q_out + idx * 14);
        double2 a;
        a.x = rec[kX + 2 * r];
        a.y = rec[kX + 2 * r + 1];
        if (MODE == 1) { a.x = wrap_pi(a.x); a.y = wrap_pi(a.y); }
        row[r] = a;
        if (r == 0) {
          double2 b;
          b.x = rec[kX + 12];
          b.y = rec[kX + 13];
          if (MODE == 1) { b.x = wrap_pi(b.x); b.y = wrap_pi(b.y); }
          row[6] = b;
        }
      }
      const unsigned long long badmask = __builtin_amdgcn_ballot_w64(bad);
      if (fin && r == 0) {
        const bool gbad = ((badmask >> leader) & 0x3Full) != 0ull;
        ok_out[idx] = (uint8_t)((!gbad) && (norm1 < K.tol_pos) && (norm2 < K.tol_rot));
        if (iters_out) iters_out[idx] = (uint16_t)updates;
        if (pool != nullptr && dump_threshold > 10) atomicAdd(queue + 3, 1ull); // finished count of the occupancy-driven hand-over
        if constexpr (PART == kFdHead) state[idx * kStateRow + kStateTag] = __longlong_as_double(-1ll); // nothing left for the resume launch
      }
      if (fin) active = false;
    }
