// ccmp::discreteGeodesicBatch with a proxy scene (include/ccmp_ompl_adapter.hpp, part 1: plain C++14, no OMPL) at the shapes its host
// loop treats differently: lists too short for an edge (continued from the last stored state), a batch of 1024 edges (first pass with
// lists of 16 and a budget of Newton rounds, then continuation) and no scene at all (the plain overload).  Whatever the shape, an edge
// must come out the same — reached, blocked, its list bit for bit — and the host checker must be asked the same questions in the same
// order.  Every run prints one line per edge and the checker's log; tests/test_cpp_adapter_scene_batch.py compares the runs.  The one
// thing no result shows, that a small batch is a single library call, is counted at the end.
// usage: adapter_scene_batch_check <margin> <start_joint 14 values...>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ccmp_ompl_adapter.hpp"

static const uint64_t FNV_BASIS = 0xcbf29ce484222325ull, FNV_PRIME = 0x100000001b3ull;

static uint64_t hash_state(uint64_t h, const double *x)
{
  for (int i = 0; i < 14; i++) {
    uint64_t u;
    std::memcpy(&u, &x[i], 8);
    h = (h ^ u) * FNV_PRIME;
  }
  return h;
}

// the host checker behind the proxies (MoveIt in the reference): ExactChecker's rule of adapter_scene_check and a log of its questions
struct Checker {
  int asked = 0, refused = 0;
  uint64_t hash = FNV_BASIS;
  bool operator()(const double *x)
  {
    asked++;
    hash = hash_state(hash, x);
    const bool ok = std::fmod(std::fabs(x[3]) * 1000.0, 11.0) >= 1.0; // refuses about one state in eleven
    if (!ok) refused++;
    return ok;
  }
  void print(const char *tag) const { std::printf("%s log asked %d refused %d hash %016" PRIx64 "\n", tag, asked, refused, hash); }
};

typedef std::vector<std::vector<std::vector<double>>> Lists;

static void print_edges(const char *tag, size_t first, const Lists &lists, const std::vector<char> &reached, const std::vector<char> &blocked)
{
  for (size_t e = 0; e < lists.size(); e++) {
    uint64_t h = FNV_BASIS;
    for (const auto &st : lists[e]) h = hash_state(h, st.data());
    std::printf("%s e %zu reached %d blocked %d n %zu hash %016" PRIx64 "\n", tag, first + e, (int)reached[e], blocked.empty() ? 0 : (int)blocked[e],
                lists[e].size(), h);
  }
}

static const int V = 24;           // vertices
static const uint64_t SEED = 2;
static const double SPACING = 0.5; // sampleUniformNear's distance between a vertex and the one it was drawn around
static const double DELTA = 0.05, LAMBDA = 2.0;
// The six edges of (a) and (c), as (from, to) vertices.  With this seed and spacing 18 of the 24 vertices clear the proxies by more than
// 0.02 and none by 0.12 (the hands hold the object: 0.114 at most).  At margin 0.02 and with a checker that accepts everything the
// edges are: blocked after 5 states; blocked after 17; 19 states, of which the checker refuses the 7th; 19, refused the 19th; reached
// with 28 states, none refused; a target the first step cannot approach (the list is `from` alone).  At margin 0.12 the proxies refuse
// the first step of every edge.
static const int EDGES[6][2] = {{0, 19}, {5, 6}, {0, 1}, {1, 0}, {1, 8}, {0, 4}};

int main(int argc, char **argv)
{
  if (argc < 16) return 2;
  try {
    const double margin = std::atof(argv[1]);
    double start[14];
    for (int i = 0; i < 14; i++) start[i] = std::atof(argv[2 + i]);
    // the set-up of adapter_scene_check's KinematicChainConstraint, on the Projector itself
    ccmp::Projector P;
    P.setArmModels("panda_left", 0, "panda_right", 1);
    const double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p_left[3] = {0.0, 0.3, 1.006}, p_right[3] = {0.0, -0.3, 1.006};
    P.setBaseFrame(0, R, p_left);
    P.setBaseFrame(1, R, p_right);
    P.setInitialPosition(start);
    P.setTolerance(1e-3, 5e-3);
    // adapter_scene_check's proxies: spheres along both arms' links and hands, the sub_table; neighbouring links allowed
    std::vector<ccmp_sphere> sph;
    for (int arm = 0; arm < 2; arm++)
      for (int k = 0; k < 8; k++) {
        ccmp_sphere s;
        std::memset(&s, 0, sizeof s);
        s.frame = CCMP_FRAME(arm, k);
        s.group = arm * 9 + k;
        s.r = k == 7 ? 0.06 : 0.07;
        sph.push_back(s);
      }
    uint32_t allowed[32] = {0};
    for (int arm = 0; arm < 2; arm++)
      for (int k = 0; k < 8; k++)
        for (int j = k + 1; j < 8 && j <= k + 3; j++) ccmp::ProxyScene::allow(allowed, arm * 9 + k, arm * 9 + j);
    std::vector<ccmp_box> boxes{ccmp::ProxyScene::subTable(19)};
    ccmp::ProxyScene scene(P, sph, boxes, allowed);

    // the planner's vertices: projected samples, each near an earlier one
    std::vector<double> verts((size_t)V * 14);
    ccmp::RefSampleBuffer near(P, SEED, ccmp::RefSampleBuffer::Near);
    for (int v = 0; v < V; v++) {
      const double *ref = v == 0 ? start : &verts[(size_t)((v * 7) % v) * 14];
      bool ok = false;
      for (int tries = 0; tries < 32 && !ok; tries++) ok = near.next(&verts[(size_t)v * 14], ref, SPACING);
      if (!ok) { std::fprintf(stderr, "vertex %d: no projected sample\n", v); return 3; }
    }
    auto edges = [&](size_t E, size_t first, std::vector<double> &from, std::vector<double> &to, bool cycle) {
      from.resize(E * 14);
      to.resize(E * 14);
      for (size_t k = 0; k < E; k++) {
        const size_t e = first + k;
        const size_t a = cycle ? e % V : (size_t)EDGES[e][0], b = cycle ? (a + 1 + e / V) % V : (size_t)EDGES[e][1];
        std::memcpy(&from[k * 14], &verts[a * 14], 14 * sizeof(double));
        std::memcpy(&to[k * 14], &verts[b * 14], 14 * sizeof(double));
      }
    };
    std::vector<double> from, to;
    Lists lists;
    std::vector<char> reached, blocked;
    char tag[64];

    // (a) lists of 2 (asked for as 1), 3 and 64 states: the same edges, the same questions
    int continued = 0, n_blocked = 0, n_cut = 0;
    edges(6, 0, from, to, false);
    for (int ct = 0; ct < 2; ct++)
      for (int max_states : {1, 3, 64}) {
        Checker chk;
        ccmp::discreteGeodesicBatch(P, from.data(), to.data(), 6, false, [&](const double *q) { return chk(q); }, &lists, &reached, max_states, ct != 0,
                                    DELTA, LAMBDA, &scene, margin, &blocked);
        std::snprintf(tag, sizeof tag, "a ct %d max_states %d |", ct, max_states);
        print_edges(tag, 0, lists, reached, blocked);
        chk.print(tag);
        if (max_states == 3) {
          for (size_t e = 0; e < 6; e++) {
            if (lists[e].size() > 3) continued++;
            if (blocked[e]) n_blocked++;
          }
          n_cut += chk.refused; // an edge stops at its first refusal
        }
      }

    // (b) 1024 edges in one call (the first pass lists 16 states and spends at most 128 rounds per edge) and in two calls of 512
    int over16 = 0;
    {
      const size_t E = 1024;
      Checker one, two;
      edges(E, 0, from, to, true);
      ccmp::discreteGeodesicBatch(P, from.data(), to.data(), E, false, [&](const double *q) { return one(q); }, &lists, &reached, 64, false, DELTA, LAMBDA,
                                  &scene, margin, &blocked);
      print_edges("b calls 1 |", 0, lists, reached, blocked);
      one.print("b calls 1 |");
      for (const auto &l : lists)
        if (l.size() > 16) over16++;
      for (size_t half = 0; half < 2; half++) {
        edges(E / 2, half * (E / 2), from, to, true);
        ccmp::discreteGeodesicBatch(P, from.data(), to.data(), E / 2, false, [&](const double *q) { return two(q); }, &lists, &reached, 64, false, DELTA,
                                    LAMBDA, &scene, margin, &blocked);
        print_edges("b calls 2 |", half * (E / 2), lists, reached, blocked);
      }
      two.print("b calls 2 |");
    }

    // (c) no scene: the plain overload
    edges(6, 0, from, to, false);
    for (int ct = 0; ct < 2; ct++)
      for (int max_states : {3, 64})
        for (int plain = 0; plain < 2; plain++) {
          Checker chk;
          blocked.clear();
          if (plain)
            ccmp::discreteGeodesicBatch(P, from.data(), to.data(), 6, false, [&](const double *q) { return chk(q); }, &lists, &reached, max_states, ct != 0,
                                        DELTA, LAMBDA);
          else
            ccmp::discreteGeodesicBatch(P, from.data(), to.data(), 6, false, [&](const double *q) { return chk(q); }, &lists, &reached, max_states, ct != 0,
                                        DELTA, LAMBDA, nullptr, margin, &blocked);
          std::snprintf(tag, sizeof tag, "c ct %d max_states %d %s |", ct, max_states, plain ? "plain" : "noscene");
          print_edges(tag, 0, lists, reached, blocked);
          chk.print(tag);
        }

    // (d) the shape of a SMALL batch, which no result shows (a continued edge equals an uninterrupted one): six edges with room for
    // every list are ONE library call.  Counted by the resident service of analytic mode, which serves batches of up to eight edges and
    // every continuation: a first pass cut to 16 states would add a request per longer edge.
    {
      long before = -1, after = -1;
      P.setJacobianMode(1);
      ccmp::check(ccmp_ctx_set_option(P.ctx(), "resident_idle_ms", 200), "resident_idle_ms");
      P.setResident(true);
      ccmp::check(ccmp_ctx_get_option(P.ctx(), "resident_served", &before), "resident_served");
      ccmp::discreteGeodesicBatch(P, from.data(), to.data(), 6, true, [](const double *) { return true; }, &lists, &reached, 64, false, DELTA, LAMBDA, nullptr,
                                  margin, &blocked);
      ccmp::check(ccmp_ctx_get_option(P.ctx(), "resident_served", &after), "resident_served");
      P.setResident(false);
      int d_over16 = 0, d_over64 = 0;
      for (const auto &l : lists) {
        if (l.size() > 16) d_over16++;
        if (l.size() > 64) d_over64++;
      }
      std::printf("d served %ld over16 %d over64 %d\n", after - before, d_over16, d_over64);
    }

    // what keeps the comparisons from being empty: edges of (a) that were continued, blocked by the proxies, cut by the checker; edges
    // of (b) longer than the first pass's lists
    std::printf("conditions continued %d blocked %d cut %d over16 %d\n", continued, n_blocked, n_cut, over16);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
