"""Shared cases of the planner-loop tests (tests/test_plan_*.py, tests/test_gpu_plan.py).

Two things: a plain-Python restatement of the scalar parts of the rule that csrc/ccmp_plan.h states (the gate, the carry rule of
closestFromGoal, the thresholds, the caps, the ladder's prefix, the solution test) on the state dict that `Plan.state()` returns; and
`HandPlan`, a driver that runs the whole loop BY HAND over the public mirror calls that exist without ccmp_plan_* (propose, grow, commit,
closest, valid, pose_ik_batch, connect, labels) with every decision taken on the host by the restatement.  The sequence is the one
include/ccmp.h states for ccmp_plan_*; `Plan` must leave the same bits."""
import copy

import numpy as np

MAX_LIST, LADDER, TARGETS, IMPROVE = 8, 9, 11, 0.1
OPEN, SOLVED, BUDGET, FULL, INVALID_GOAL = range(5)
COUNTERS = ("proposals", "valid_proposals", "ik_successes", "vertices_kept", "mid_stones", "unsettled", "checks", "goal_pushes", "start_pushes", "ladder_vertices",
            "push_refused")
UNSETTLED = 3  # GROW_UNSETTLED


def new_state(start_pose, goal_dist, first_index=0):
    return {"starts": [], "goals": [], "nearest": -1, "sprevious": -1, "status": OPEN, "cycle": 0, "solved_start": -1, "solved_goal": -1, "size_at_check": 0,
            "next_index": int(first_index), "nearest_pose": [float(v) for v in start_pose], "prev_from_goal": float(goal_dist), "prev_from_start": float(goal_dist),
            "counters": {n: 0 for n in COUNTERS}}


def gate(size, size_at_check):
    return size > size_at_check + 3


def full(size, width, k, max_vertices):
    return size + width * (1 + k) + TARGETS > max_vertices


def carry(froms, idx, dist, from_dist, size):
    """Roadmap.closest_from_goal's fold, with the range checks of the device form: (closest or -1, closestVal)"""
    closest, val = -1, float("inf")
    for f, i, d, h in zip(froms, idx, dist, from_dist):
        if f < 0 or f >= size:
            continue
        if h < val:
            val = float(h)
        closest = int(f)
        if 0 <= i < size and d < val:
            closest, val = int(i), float(d)
    return closest, val


def check(state, size, a, b, store_poses=None):
    """the check's decisions: (new state, [ran, goal side fired, start side fired, the goal side's vertex or -1])"""
    s = copy.deepcopy(state)
    trig = [0, 0, 0, -1]
    if not gate(size, s["size_at_check"]):
        return s, trig
    trig[0] = 1
    s["counters"]["checks"] += 1
    S, G = len(s["starts"]), len(s["goals"])
    if S > 0 and G > 0:
        c, d = carry(s["starts"], *a, size)
        if c >= 0 and d < s["prev_from_goal"] - IMPROVE:
            s["nearest"], s["prev_from_goal"] = c, d
            trig[1], trig[3] = 1, c
            if store_poses is not None:
                s["nearest_pose"] = [float(v) for v in store_poses[c]]
            if G >= MAX_LIST:
                s["counters"]["push_refused"] += 1
        p, d2 = carry(s["goals"], *b, size)
        if p >= 0:
            s["sprevious"] = p
            if d2 < s["prev_from_start"] - IMPROVE:
                s["prev_from_start"] = d2
                trig[2] = 1
                if S >= MAX_LIST:
                    s["counters"]["push_refused"] += 1
    s["size_at_check"] = int(size)
    s["next_index"] += TARGETS
    return s, trig


def prefix(valid, ik_ok):
    n = 0
    while n < LADDER and valid[n] and ik_ok[n]:
        n += 1
    return np.array([1 if i < n else 0 for i in range(LADDER)], dtype=np.uint8), n


def connected(labels, state):
    s = copy.deepcopy(state)
    if s["status"] == SOLVED:
        return s
    N = len(labels)
    for a in s["starts"]:
        for b in s["goals"]:
            if 0 <= a < N and 0 <= b < N and labels[a] == labels[b]:
                s["status"], s["solved_start"], s["solved_goal"] = SOLVED, int(a), int(b)
                return s
    return s


def push(state, which, new_index):
    """in place: a committed vertex onto starts (0) or goals (1) under the cap"""
    if new_index < 0:
        return
    lst, name = (state["starts"], "start_pushes") if which == 0 else (state["goals"], "goal_pushes")
    if len(lst) >= MAX_LIST:
        state["counters"]["push_refused"] += 1
        return
    lst.append(int(new_index))
    state["counters"][name] += 1


def problem_poses(problem):
    """(start pose, goal pose) of a CcmpProblem as pose rows (8,), pad 0"""
    from closed_chain_motion_planner_amd import pose_from_t_wo

    sp = pose_from_t_wo(np.array(list(problem.obj_start_R) + list(problem.obj_start_p)))
    gp = pose_from_t_wo(np.array(list(problem.obj_goal_R) + list(problem.obj_goal_p)))
    sp[7] = gp[7] = 0.0
    return sp, gp


def far_goal_state(c, checker, max_states, lo=0.35, seed=0xFA2, n=2048):
    """A goal that one motion does not reach (the shipped goals are connected at open, so the loop never runs on them): of n sampled
    states of the constraint `c` that are within the joint limits, the one whose object pose is nearest to the start pose among those
    at least `lo` away whose mesh is free and which checkMotion from the start state does NOT reach within max_states.  In place: the
    problem's goal object pose becomes that state's; returns the state (14,), the plan's goal_joints.  Needs a device."""
    import torch
    from closed_chain_motion_planner_amd import pose_distance, pose_from_t_wo

    q, ok = c.sample_project_batch(seed, 0, n, want_iters=False)[:2]
    good = q[ok.bool() & c.joint_valid_batch(q).bool()].contiguous()
    t = c.compute_t_wo_batch(good).cpu().numpy().reshape(-1, 12)
    poses = pose_from_t_wo(t)
    poses[:, 7] = 0.0
    sp, _ = problem_poses(c.problem)
    d = np.array([pose_distance(sp, p) for p in poses])
    free = checker.valid(torch.from_numpy(poses).cuda()).cpu().numpy() != 0
    start = torch.from_numpy(np.tile(np.array(c.problem.start_joint[:]), (len(good), 1))).cuda()
    direct = c.discrete_geodesic_batch(start, good, max_states=max_states, check_target=True)[2].cpu().numpy() == 1
    pick = np.flatnonzero(free & ~direct & (d >= lo))
    assert len(pick) >= 1  # a condition on the sample, not on the code under test
    i = int(pick[np.argmin(d[pick])])
    c.problem.obj_goal_R[:] = t[i, :9].tolist()
    c.problem.obj_goal_p[:] = t[i, 9:].tolist()
    return good[i].cpu().numpy().copy()


def state_bits(s):
    """a state dict as a tuple that compares bit for bit (floats by their bytes)"""
    f = lambda v: np.float64(v).tobytes()
    return (tuple(s["starts"]), tuple(s["goals"]), s["nearest"], s["sprevious"], s["status"], s["cycle"], s["solved_start"], s["solved_goal"], s["size_at_check"],
            s["next_index"], tuple(f(v) for v in s["nearest_pose"]), f(s["prev_from_goal"]), f(s["prev_from_start"]), tuple(s["counters"][n] for n in COUNTERS))


class HandPlan:
    """the loop over the mirror's calls, one decision at a time on the host (needs a device)"""

    def __init__(self, rm, c, checker, goal_joints=None, scene=None, margin=0.0, width=32, k=5, rng_seed=0, first_index=0, attempts=2, max_states=64, t=0.3,
                 sigma=0.2, inflate=0.0, max_vertices=2**31 - 1):
        import torch
        from closed_chain_motion_planner_amd import pose_distance
        from closed_chain_motion_planner_amd.roadmap import COMMIT_KEEP_ISOLATED

        self.torch, self.keep = torch, COMMIT_KEEP_ISOLATED
        self.rm, self.c, self.checker, self.scene, self.margin = rm, c, checker, scene, float(margin) if scene is not None else 0.0
        self.W, self.k, self.seed, self.attempts, self.ms, self.t, self.sigma, self.inflate, self.max_vertices = width, k, rng_seed, attempts, max_states, t, sigma, inflate, max_vertices
        self.start_pose, self.goal_pose = problem_poses(c.problem)
        self.reads = self.calls = 0
        s = self.state = new_state(self.start_pose, pose_distance(self.start_pose, self.goal_pose), first_index)
        sj = self._dev(np.array(c.problem.start_joint[:]).reshape(1, 14))
        self._milestone(sj, self._dev(self.start_pose.reshape(1, 8)), 0)
        if goal_joints is None:
            ik = self._ik(self._dev(self.goal_pose.reshape(1, 8)), sj.reshape(1, 1, 14), first_index)
            gj = ik["q"] if int(ik["ok"][0]) else None
        else:
            gj = self._dev(np.asarray(goal_joints, dtype=np.float64).reshape(1, 14))
        if gj is not None:
            self._milestone(gj, self._dev(self.goal_pose.reshape(1, 8)), 1)
        s["next_index"] = int(first_index) + 1
        s["nearest"] = s["starts"][0] if s["starts"] else -1
        s["sprevious"] = s["goals"][0] if s["goals"] else -1
        s["size_at_check"] = len(rm)
        if gj is None:
            s["status"] = INVALID_GOAL
        else:
            self.state = connected(self._labels(), s)

    def _dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def _labels(self):
        self.reads += 1
        return self.rm.labels(host=True)

    def _ik(self, targets, seeds, first):
        self.calls += 1
        return self.c.pose_ik_batch(targets, seeds, rng_seed=self.seed, first_index=first, scene=self.scene, margin=self.margin if self.scene is not None else None)

    def _milestone(self, joints, pose, which):
        """startgoalMilestone: connect with check_target, commit with KEEP_ISOLATED, push"""
        torch, k = self.torch, self.k
        if len(self.rm) == 0:
            nbr = torch.full((1, k), -1, dtype=torch.int32, device="cuda")
            ok, ns = torch.zeros(k, dtype=torch.uint8, device="cuda"), torch.zeros(k, dtype=torch.int32, device="cuda")
        else:
            out = self.rm.connect(joints, k, query_poses=pose, check_target=True, max_states=self.ms, scene=self.scene, margin=self.margin)
            nbr, ok, ns = out["nbr_idx"], out["ok"], out["n_states"]
            self.calls += 1
        got = self.rm.commit(nbr, ok, ns, joints, pose, flags=self.keep)
        self.calls += 1
        self.reads += 2  # the commit's own and new_index
        push(self.state, which, int(got["new_index"][0]))

    def cycle(self):
        """one cycle; returns False when the loop has ended (SOLVED, FULL, INVALID_GOAL)"""
        torch, rm, s, W, k = self.torch, self.rm, self.state, self.W, self.k
        if s["status"] in (SOLVED, INVALID_GOAL):
            return False
        if full(len(rm), W, k, self.max_vertices):
            s["status"] = FULL
            return False
        cnt = s["counters"]
        # growth
        frm = self._dev(np.tile(np.array(s["nearest_pose"]), (W, 1)))
        prop = self.checker.propose(frm, self._dev(self.goal_pose.reshape(1, 8)), t=self.t, sigma=self.sigma, attempts=self.attempts, rng_seed=self.seed,
                                    first_index=s["next_index"], inflate=self.inflate)
        out = rm.grow(prop["pose"], k, rng_seed=self.seed, first_index=s["next_index"], max_states=self.ms, scene=self.scene, margin=self.margin,
                      vet=self.scene is not None)
        got = rm.commit(out["nbr_idx"], out["ok"], out["n_states"], out["q_new"], prop["pose"], states=out["states"], vertex_ok=out["ik_ok"],
                        goal_pose=self.goal_pose, roots=s["starts"])
        self.calls += 3
        self.reads += 6
        cnt["proposals"] += W
        cnt["valid_proposals"] += int((prop["which"] >= 0).sum())
        cnt["ik_successes"] += int((out["ik_ok"] != 0).sum())
        cnt["vertices_kept"] += int((got["new_index"] >= 0).sum())
        cnt["mid_stones"] += int((got["mid_index"] >= 0).sum())
        cnt["unsettled"] += int((got["grow_state"] == UNSETTLED).sum())
        s["next_index"] += W
        # check
        size = len(rm)
        if gate(size, s["size_at_check"]) and s["starts"] and s["goals"]:
            first = s["next_index"]
            joints, poses = rm.read(host=True)
            a = [x.cpu().numpy() for x in rm.closest(self._dev(np.array(s["starts"], dtype=np.int32)), self._dev(poses[s["goals"][0]]))]
            b = [x.cpu().numpy() for x in rm.closest(self._dev(np.array(s["goals"], dtype=np.int32)), self._dev(poses[s["starts"][0]]))]
            self.calls += 2
            self.reads += 8
            n_goals, n_starts = len(s["goals"]), len(s["starts"])
            s, trig = check(s, size, a, b, poses)
            self.state = s
            goal_q = start_q = None
            L = 0
            if trig[1]:
                from closed_chain_motion_planner_amd import pose_interpolate

                c = trig[3]
                seed = self._dev(joints[c].reshape(1, 1, 14))
                if n_goals < MAX_LIST:
                    ik = self._ik(self._dev(self.goal_pose.reshape(1, 8)), seed, first)
                    goal_q = ik["q"] if int(ik["ok"][0]) else None
                ladder = self._dev(np.stack([pose_interpolate(poses[c], self.goal_pose, 0.1 * i) for i in range(1, LADDER + 1)]))
                valid = self.checker.valid(ladder, inflate=self.inflate).cpu().numpy()
                ikl = self._ik(ladder, seed.expand(LADDER, 1, 14).contiguous(), first + 1)
                self.calls += 1
                self.reads += 3
                _, L = prefix(valid, ikl["ok"].cpu().numpy())
            if trig[2] and n_starts < MAX_LIST:
                ik = self._ik(self._dev(self.start_pose.reshape(1, 8)), self._dev(joints[s["sprevious"]].reshape(1, 1, 14)), first + TARGETS - 1)
                start_q = ik["q"] if int(ik["ok"][0]) else None
            if goal_q is not None:
                self._milestone(goal_q, self._dev(self.goal_pose.reshape(1, 8)), 1)
            if L > 0:  # addMilestone of the prefix as one batch
                lj, lp = ikl["q"][:L].contiguous(), ladder[:L].contiguous()
                out = rm.connect(lj, k, query_poses=lp, check_target=True, max_states=self.ms, scene=self.scene, margin=self.margin)
                got = rm.commit(out["nbr_idx"], out["ok"], out["n_states"], lj, lp)
                self.calls += 2
                self.reads += 2
                s["counters"]["ladder_vertices"] += int((got["new_index"] >= 0).sum())
            if start_q is not None:
                self._milestone(start_q, self._dev(self.start_pose.reshape(1, 8)), 0)
        s["cycle"] += 1
        self.state = connected(self._labels(), s)
        return self.state["status"] != SOLVED

    def run(self, max_cycles):
        ran = 0
        while ran < max_cycles:
            if self.state["status"] in (SOLVED, INVALID_GOAL):
                return ran
            before = self.state["cycle"]
            more = self.cycle()
            ran += self.state["cycle"] - before
            if not more:
                return ran
        if self.state["status"] not in (SOLVED, INVALID_GOAL, FULL):
            self.state["status"] = BUDGET
        return ran
