// ccmp_row16_geo_body.inc — the body of the analytic mode's extend-step kernel (ccmp_kernels_fast.hip: geodesic_row16_kernel, whose
// comment says what it does), as ONE text that its scene variant geodesic_row16_scene_kernel includes too: the two cannot drift apart,
// and geodesic_row16_kernel compiles to what it compiled to before (the same tokens in the same place).  With CCMP_ROW16_SCENE defined
// the reference's svc->isValid runs on the device: in kBook, after a successful projection and before the step test, the row computes
// the proxy scene's clearance of the state (ccmp_clearance.h, sixteen lanes) and a state whose clearance does not exceed `margin` ends
// the edge, blocked.  The including kernel then also provides scene, margin, blocked_out and clearance_out (nullable).
// With CCMP_ROW16_NO_PROLOGUE defined (the analytic resident service kernel, resident_row16_kernel: the text runs once per request
// inside a kernel that never ends) the including scope provides what the prologue would: K (the constants, in LDS), lane (within
// the wavefront), l, rec (the row's record) — besides the kernel's arguments from, to, E, max_states, states, n_states, ok_out,
// newton_iters, carry_in, carry_out, round_budget, check_target, queue (there: a ticket word in LDS), delta and lambda.
#ifndef CCMP_ROW16_NO_PROLOGUE
  __shared__ double ktab[kConstsDoubles + 1];
  __shared__ double lds[4 * gRec];
  {
    const double *srcp = reinterpret_cast<const double *>(&K_arg);
    for (int k = threadIdx.x; k < kConstsDoubles; k += 64) ktab[k] = srcp[k];
  }
  __syncthreads();
  const ccmp_consts &K = *reinterpret_cast<const ccmp_consts *>(ktab);
  const int lane = threadIdx.x, l = lane & 15;
  double *const rec = lds + (lane >> 4) * gRec;
#endif
#ifdef CCMP_ROW16_SCENE
  // the row's proxy centres; its frames go to the front of its record (the Newton round's workspace, dead between two projections)
  __shared__ double clr_cen[4 * kClrCentres];
  double *const cen = clr_cen + (lane >> 4) * kClrCentres;
#endif
  // joint role (lanes 14, 15 shadow joint 13 and never store), chain role: as project_row16_kernel
  const bool jl = l < 14;
  const int lj = jl ? l : 13;
  const int aj = lj >= 7 ? 1 : 0, ij = lj - 7 * aj;
  double ax[3], ap[6];
#pragma unroll
  for (int k = 0; k < 3; k++) ax[k] = K.axis[aj][ij][k];
#pragma unroll
  for (int k = 0; k < 6; k++) ap[k] = K.aprod[aj][ij][k];
  const double sgn = aj ? -1.0 : 1.0;
  const int ac = (l / 3) & 1, rc = l % 3;
  double cee[3], cRt[9];
#pragma unroll
  for (int k = 0; k < 3; k++) cee[k] = K.ee[ac][k];
#pragma unroll
  for (int k = 0; k < 9; k++) cRt[k] = K.R_tool[ac][k];
  const double cd = K.base_R[ac][4 * rc], cbp = K.base_p[ac][rc];
  const double pi = 3.14159265358979323846;

  // What the row does next (the sixteen lanes of a row hold the same stage and counters; lane l < 14 also joint l of the iterate x,
  // of `previous` and of the target in registers, and the row's LDS record holds all fourteen of each for the serial sums)
  enum { kIdle, kTarget, kProject, kEnter, kBook, kNext, kDone };
  int stage = kIdle;
  bool drained = false, target_ok = true, fits = true, suspended = false;
  unsigned long long t = 0;
  double x = 0.0, prv = 0.0, tgt = 0.0, dist = 0.0, total = 0.0, maxd = 0.0, norm1 = 0.0, norm2 = 0.0;
  int n = 0, its = 0, rounds = 0, iter = 0, updates = 0;
#ifdef CCMP_ROW16_SCENE
  bool blocked = false; // the traversal ended at a state the scene refused
  double clr = 0.0;     // the clearance of the state being booked
#endif

  for (;;) {
    // ---- between two Newton rounds: bookkeeping, ended edges, new edges — until every row projects or the tickets are gone -----
    for (;;) {
      if (stage == kBook) { // a projection has ended: jy_ProjectedStateSpace.cpp:65-92
        its += updates;
        rounds += updates + 1;
        if (jl) rec[gX + lj] = x;
        asm volatile("" ::: "memory"); // written before the row reads it (one wavefront per block: the LDS queue keeps the order)
        // jointValid(x), step = |previous - x| and newDist = |x - to| side by side, the canonical order each (ccmp_geo_edge_body.inc)
        bool jv = true;
        double s_acc = 0.0, d_acc = 0.0;
#pragma unroll
        for (int i = 0; i < 14; i++) {
          const double xi = rec[gX + i];
          const int jj = i < 7 ? i : i - 7;
          if (xi < K.lbe[jj]) jv = false;
          if (xi > K.ube[jj]) jv = false;
          const double ds = rec[gPrev + i] - xi, dd = xi - rec[gTo + i];
          s_acc = CCMP_FMA(ds, ds, s_acc);
          d_acc = CCMP_FMA(dd, dd, d_acc);
        }
        const bool conv = (norm1 < K.tol_pos) && (norm2 < K.tol_rot); // project()'s return value (project_row16_kernel's ok without jointValid)
        stage = kDone;
#ifdef CCMP_ROW16_SCENE
        if (conv && jv) { // svc->isValid(scratch): refused before the step test and the list-full rule
          clr = state_clearance<16>(K, scene, rec + gX, rec, cen, nullptr, l, lane);
          if (!(clr > margin)) { blocked = true; jv = false; }
        }
#endif
        if (conv && jv) {                                   // else: not on manifold
          const double step = ccmp_sqrt(s_acc), newDist = ccmp_sqrt(d_acc);
          const double total_before = total;
          if (!(step > lambda * delta)) {                   // else: deviated
            total += step;
            if (!(total > maxd) && !(newDist >= dist)) {    // else: wandered too far / no closer than before
              if (n >= max_states) { // the accepted state finds the list full: the continuation projects it again
                fits = false;
                n = max_states + 1;
                total = total_before;
                its -= updates;
              } else {
                dist = newDist;
                prv = x;
                if (jl) {
                  rec[gPrev + lj] = x;
                  states[(t * (unsigned long long)max_states + (unsigned long long)n) * 14ull + lj] = x;
                }
#ifdef CCMP_ROW16_SCENE
                if (l == 0 && clearance_out) clearance_out[t * (unsigned long long)max_states + (unsigned long long)n] = clr;
#endif
                n++;
                // } while (dist >= tolerance); then the call's bound on the serial work spent on one edge: past round_budget
                // Newton rounds the edge stops between two states and reports ok = 2 (ccmp_geo_edge_body.inc)
                if (dist >= delta) {
                  if (round_budget > 0 && rounds >= round_budget) suspended = true;
                  else stage = kNext;
                }
              }
            }
          }
        }
      }
      // ---- rows without an edge take the next ticket --------------------------------------------------------------------------
      {
        const bool want = stage == kIdle && !drained;
        unsigned long long tk = 0;
        if (want && l == 0) tk = atomicAdd(queue, 1ull);
        tk = __shfl(tk, lane & ~15);
        if (want) {
          if (tk < E) {
            t = tk;
            prv = from[t * 14 + lj];
            tgt = to[t * 14 + lj];
            if (jl) {
              rec[gPrev + lj] = prv;
              rec[gTo + lj] = tgt;
              states[t * (unsigned long long)max_states * 14ull + lj] = prv; // geodesic->push_back(cloneState(from))
            }
            n = 1; its = 0; rounds = 0;
            target_ok = true; fits = true; suspended = false;
#ifdef CCMP_ROW16_SCENE
            blocked = false;
#endif
            total = 0.0;
            // ConstrainedMotionValidator::checkMotion (src/planner/stefanBiPRM.cpp:397-398): isSatisfied(to) first, one evaluation
            if (check_target) { x = tgt; stage = kTarget; }
            else stage = kEnter;
          } else drained = true;
        }
      }
      if (stage == kEnter) {
        asm volatile("" ::: "memory");
        double d = 0.0;
#pragma unroll
        for (int i = 0; i < 14; i++) {
          const double diff = rec[gPrev + i] - rec[gTo + i];
          d = CCMP_FMA(diff, diff, d);
        }
        dist = ccmp_sqrt(d);
        maxd = dist * lambda;
        // a continuation is in the middle of the reference's do-while: it re-enters on the loop's own condition (dist >= delta)
        // with the running length and the bound of the first call
        bool enter = dist > delta;
        if (carry_in) {
          total = carry_in[2 * t];
          maxd = carry_in[2 * t + 1];
          enter = dist >= delta;
        }
        stage = (target_ok && enter) ? kNext : kDone;
      }
      if (stage == kNext) { // WrapperStateSpace::interpolate(previous, to, delta_ / dist, scratch) (KinematicChain.h:145-171; orc_interpolate)
        const double tt = delta / dist;
        x = ccmp_joint_interpolate(prv, tgt, tt);
        iter = 0; updates = 0; norm1 = 0.0; norm2 = 0.0;
        stage = kProject;
      }
      if (stage == kDone) {
        if (l == 0) {
          n_states[t] = n;
          ok_out[t] = suspended ? (uint8_t)2 : (uint8_t)(target_ok && fits && dist <= delta);
          if (newton_iters) newton_iters[t] = its;
          if (carry_out) { carry_out[2 * t] = total; carry_out[2 * t + 1] = maxd; }
#ifdef CCMP_ROW16_SCENE
          if (blocked_out) blocked_out[t] = blocked ? (uint8_t)1 : (uint8_t)0;
#endif
        }
        stage = kIdle;
      }
      if (__builtin_amdgcn_ballot_w64(stage == kIdle && !drained) == 0ull) break;
    }
    if (__builtin_amdgcn_ballot_w64(stage != kIdle) == 0ull) break;

    // ---- one Newton round of every row that projects (or evaluates its target) ------------------------------------------------
#include "ccmp_row16_eval.inc"
    bool cont = false;
    if (stage == kTarget) { // KinematicChainConstraint::isSatisfied (ConstraintFunction.h:114-120): finite, f0 <= tol1, f1 <= tol2
      target_ok = (f[0] - f[0] == 0.0) && (f[1] - f[1] == 0.0) && f[0] <= K.tol_pos && f[1] <= K.tol_rot;
      stage = kEnter;
    } else if (stage == kProject) { // ConstraintFunction.h:68, quirks included
      const bool c1 = f[0] > K.tol_pos;
      norm1 = c1 ? 1.0 : 0.0;
      bool resid = c1;
      if (!c1) { norm2 = f[1]; resid = f[1] > K.tol_rot; }
      if (resid) { cont = iter < K.max_iter; iter++; }
      if (!cont) stage = kBook;
    }
    if (__builtin_amdgcn_ballot_w64(cont) == 0ull) continue;
#include "ccmp_row16_step.inc"
  }
