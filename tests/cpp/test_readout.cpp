// Solution readout of the C++ drop-in: PGOAgent::getTrajectoryInGlobalFrame / getPoseInGlobalFrame /
// getNeighborPoseInGlobalFrame (reference src/PGOAgent.cpp:500-562) on smallGrid3D.  The trajectory is rounded on
// the GPU (dpgo_hip_round_se); getTrajectoryInLocalFrame, its host counterpart, is the comparison.
#include <DPGO/DPGO_utils.h>
#include <DPGO/PGOAgent.h>

#include <cmath>
#include <cstdio>
#include <fstream>
#include <functional>
#include <memory>
#include <string>
#include <vector>

using namespace DPGO;

static int g_fail = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      ++g_fail;                                                             \
    }                                                                       \
  } while (0)

static std::vector<RelativeSEMeasurement> read_meas_txt(const std::string& path, size_t& n) {
  std::ifstream in(path);
  std::vector<RelativeSEMeasurement> out;
  int d = 0;
  size_t m = 0;
  in >> d >> n >> m;
  for (size_t e = 0; e < m; ++e) {
    size_t p1, p2;
    in >> p1 >> p2;
    Matrix R(d, d), t(d, 1);
    for (int u = 0; u < d; ++u)
      for (int v = 0; v < d; ++v) in >> R(u, v);
    for (int u = 0; u < d; ++u) in >> t(u, 0);
    double k, ta;
    in >> k >> ta;
    out.emplace_back(0, 0, p1, p2, R, t, k, ta);
  }
  return out;
}

static Matrix read_matrix_txt(const std::string& path) {
  std::ifstream in(path);
  long r = 0, c = 0;
  in >> r >> c;
  Matrix M(r, c);
  for (long i = 0; i < r; ++i)
    for (long j = 0; j < c; ++j) in >> M(i, j);
  return M;
}

static double maxAbs(const Matrix& M) {
  double s = 0.0;
  for (long j = 0; j < M.cols(); ++j)
    for (long i = 0; i < M.rows(); ++i) s = std::max(s, std::fabs(M(i, j)));
  return s;
}

static const unsigned d = 3, r = 5;

// smallGrid3D split into contiguous ranges over `num_robots` agents (examples/MultiRobotExample.cpp:73-120), every
// agent at its block of the golden lifted chordal initialisation X0
static std::vector<std::unique_ptr<PGOAgent>> makeAgents(const std::string& golden, unsigned num_robots, Matrix& X0,
                                                         bool setX) {
  size_t n = 0;
  const auto dataset = read_meas_txt(golden + "/smallGrid3D.meas.txt", n);
  X0 = read_matrix_txt(golden + "/smallGrid3D.X0.txt");
  const unsigned per = static_cast<unsigned>(n / num_robots);
  auto first = [&](unsigned robot) { return robot >= num_robots ? static_cast<unsigned>(n) : robot * per; };
  std::vector<std::pair<unsigned, unsigned>> PoseMap(n);
  for (unsigned robot = 0; robot < num_robots; ++robot)
    for (unsigned i = first(robot); i < first(robot + 1); ++i) PoseMap[i] = {robot, i - first(robot)};
  std::vector<std::vector<RelativeSEMeasurement>> odo(num_robots), priv(num_robots), shared(num_robots);
  for (const auto& mIn : dataset) {
    const auto src = PoseMap[mIn.p1], dst = PoseMap[mIn.p2];
    RelativeSEMeasurement m(src.first, dst.first, src.second, dst.second, mIn.R, mIn.t, mIn.kappa, mIn.tau);
    if (src.first == dst.first) {
      (src.second + 1 == dst.second ? odo : priv)[src.first].push_back(m);
    } else {
      shared[src.first].push_back(m);
      shared[dst.first].push_back(m);
    }
  }
  std::vector<std::unique_ptr<PGOAgent>> agents;
  for (unsigned robot = 0; robot < num_robots; ++robot) {
    PGOAgentParameters options(d, r, num_robots);
    agents.emplace_back(new PGOAgent(robot, options));
    if (robot > 0) {
      Matrix M;
      agents[0]->getLiftingMatrix(M);
      agents[robot]->setLiftingMatrix(M);
    }
    agents[robot]->setPoseGraph(odo[robot], priv[robot], shared[robot]);
    if (setX)
      agents[robot]->setX(X0.block(0, first(robot) * (d + 1), r, (first(robot + 1) - first(robot)) * (d + 1)));
  }
  return agents;
}

// every d x d rotation block orthonormal with determinant +1
static bool rotationsValid(const Matrix& T, double tol) {
  for (long i = 0; i < T.cols() / (d + 1); ++i) {
    const Matrix R = T.block(0, i * (d + 1), d, d);
    if (maxAbs(R.transpose() * R - Matrix::Identity(d, d)) > tol || !(R.determinant() > 0.0)) return false;
  }
  return true;
}

static void testTrajectoryInGlobalFrame(const std::string& golden) {
  Matrix X0;
  auto agents = makeAgents(golden, 1, X0, true);
  PGOAgent& agent = *agents[0];
  const long n = agent.num_poses();
  const long k = n / 2;  // the other anchor
  for (int phase = 0; phase < 2; ++phase) {
    // phase 0: X = YLift T (rank d: every frame change is exactly rigid); phase 1: after one RBCD update, when
    // Y_a^T Y_j is no longer a rotation and the projection does real work
    if (phase == 1) agent.iterate(true);
    Matrix Tloc, Tg, A;
    EXPECT(agent.getTrajectoryInLocalFrame(Tloc));
    EXPECT(agent.getSharedPose(0, A));
    agent.setGlobalAnchor(A);
    EXPECT(agent.getTrajectoryInGlobalFrame(Tg));
    EXPECT(Tg.rows() == Tloc.rows() && Tg.cols() == Tloc.cols());
    const double scale = std::max(1.0, maxAbs(Tloc));
    const double err = maxAbs(Tg - Tloc);
    std::printf("  phase %d: max |global(anchor = own pose 0) - local| = %.3e (scale %.3g)\n", phase, err, scale);
    EXPECT(err <= 1e-12 * scale);
    EXPECT(rotationsValid(Tg, 1e-12));
    // another pose as the anchor: that pose becomes [I | 0], every rotation stays a rotation
    EXPECT(agent.getSharedPose(static_cast<unsigned>(k), A));
    agent.setGlobalAnchor(A);
    Matrix Tk;
    EXPECT(agent.getTrajectoryInGlobalFrame(Tk));
    EXPECT(rotationsValid(Tk, 1e-12));
    Matrix Ik = Matrix::Zero(d, d + 1);
    Ik.setBlock(0, 0, Matrix::Identity(d, d));
    EXPECT(maxAbs(Tk.block(0, k * (d + 1), d, d + 1) - Ik) <= 1e-12);
    if (phase == 0) {
      // rigid re-framing of the same trajectory: T'_j = (T_k)^-1 T_j
      const Matrix RkT = Tloc.block(0, k * (d + 1), d, d).transpose();
      const Matrix tk = Tloc.block(0, k * (d + 1) + d, d, 1);
      double worst = 0.0;
      for (long j = 0; j < n; ++j) {
        const Matrix Rj = RkT * Tloc.block(0, j * (d + 1), d, d);
        const Matrix tj = RkT * (Tloc.block(0, j * (d + 1) + d, d, 1) - tk);
        worst = std::max(worst, maxAbs(Tk.block(0, j * (d + 1), d, d) - Rj));
        worst = std::max(worst, maxAbs(Tk.block(0, j * (d + 1) + d, d, 1) - tj));
      }
      std::printf("  re-framed at pose %ld: max deviation from (T_k)^-1 T_j = %.3e\n", k, worst);
      EXPECT(worst <= 1e-10 * scale);
    }
  }
}

// Y_a^T Xi, translation relative to the anchor's, by hand
static Matrix byHand(const Matrix& A, const Matrix& Xi) {
  Matrix T(d, d + 1);
  for (unsigned a = 0; a < d; ++a) {
    double t0 = 0.0;
    for (unsigned q = 0; q < r; ++q) t0 += A(q, a) * A(q, d);
    for (unsigned c = 0; c <= d; ++c) {
      double s = 0.0;
      for (unsigned q = 0; q < r; ++q) s += A(q, a) * Xi(q, c);
      T(a, c) = c == d ? s - t0 : s;
    }
  }
  return T;
}

static void testPoseInGlobalFrame(const std::string& golden) {
  Matrix X0;
  auto agents = makeAgents(golden, 2, X0, true);
  PGOAgent &a0 = *agents[0], &a1 = *agents[1];
  a0.iterate(true);
  Matrix A, X;
  EXPECT(a0.getSharedPose(3, A));
  a0.setGlobalAnchor(A);
  EXPECT(a0.getX(X));
  Matrix Ti, Ttraj;
  EXPECT(a0.getTrajectoryInGlobalFrame(Ttraj));
  for (unsigned i : {0u, 3u, a0.num_poses() - 1}) {
    EXPECT(a0.getPoseInGlobalFrame(i, Ti));
    EXPECT(Ti.rows() == d && Ti.cols() == d + 1);
    EXPECT(maxAbs(Ti - byHand(A, X.block(0, i * (d + 1), r, d + 1))) <= 1e-13 * std::max(1.0, maxAbs(Ti)));
    // the same translation as the rounded trajectory; the rotation block is not projected
    EXPECT(maxAbs(Ti.block(0, d, d, 1) - Ttraj.block(0, i * (d + 1) + d, d, 1)) <= 1e-12 * std::max(1.0, maxAbs(Ti)));
  }
  EXPECT(!a0.getPoseInGlobalFrame(a0.num_poses(), Ti));
  // neighbour poses: known once the neighbour's shared poses were delivered
  PoseDict pd;
  EXPECT(a1.getSharedPoseDict(pd));
  EXPECT(!pd.empty());
  const PoseID some = pd.begin()->first;
  EXPECT(!a0.getNeighborPoseInGlobalFrame(some.first, some.second, Ti));
  a0.setNeighborStatus(a1.getStatus());
  a0.updateNeighborPoses(a1.getID(), pd);
  unsigned known = 0;
  for (const auto& kv : pd) {
    if (!a0.getNeighborPoseInGlobalFrame(kv.first.first, kv.first.second, Ti)) continue;
    ++known;
    EXPECT(maxAbs(Ti - byHand(A, kv.second)) <= 1e-13 * std::max(1.0, maxAbs(Ti)));
  }
  EXPECT(known > 0);
  EXPECT(!a0.getNeighborPoseInGlobalFrame(1, a1.num_poses() + 7, Ti));
}

static void testGlobalFrameNeedsAnchor(const std::string& golden) {
  Matrix X0, T;
  {
    // initialised, no anchor yet
    auto agents = makeAgents(golden, 2, X0, true);
    PGOAgent& a0 = *agents[0];
    EXPECT(a0.getState() == INITIALIZED);
    EXPECT(!a0.getTrajectoryInGlobalFrame(T));
    EXPECT(!a0.getPoseInGlobalFrame(0, T));
    EXPECT(!a0.getNeighborPoseInGlobalFrame(1, 0, T));
    Matrix A;
    EXPECT(a0.getSharedPose(0, A));
    a0.setGlobalAnchor(A);
    EXPECT(a0.getTrajectoryInGlobalFrame(T));
    EXPECT(a0.getPoseInGlobalFrame(0, T));
  }
  {
    // an anchor, but agent 1 still waits for its initialisation in the global frame
    auto agents = makeAgents(golden, 2, X0, false);
    PGOAgent& a1 = *agents[1];
    EXPECT(a1.getState() == WAIT_FOR_INITIALIZATION);
    a1.setGlobalAnchor(X0.block(0, 0, r, d + 1));
    EXPECT(!a1.getTrajectoryInGlobalFrame(T));
    EXPECT(!a1.getPoseInGlobalFrame(0, T));
    EXPECT(!a1.getNeighborPoseInGlobalFrame(0, 0, T));
  }
}

int main(int argc, char** argv) {
  const std::string golden = argc > 1 ? argv[1] : "tests/golden";
  struct T {
    const char* name;
    std::function<void()> fn;
  } tests[] = {{"TrajectoryInGlobalFrame", [&] { testTrajectoryInGlobalFrame(golden); }},
               {"PoseInGlobalFrame", [&] { testPoseInGlobalFrame(golden); }},
               {"GlobalFrameNeedsAnchor", [&] { testGlobalFrameNeedsAnchor(golden); }}};
  for (auto& t : tests) {
    const int before = g_fail;
    try {
      t.fn();
    } catch (const std::exception& e) {
      std::printf("  EXCEPTION %s\n", e.what());
      ++g_fail;
    }
    std::printf("[%s] %s\n", g_fail == before ? "PASS" : "FAIL", t.name);
  }
  std::printf("%s\n", g_fail ? "SOME TESTS FAILED" : "ALL TESTS PASSED");
  return g_fail ? 1 : 0;
}
