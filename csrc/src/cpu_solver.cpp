// Whole-domain CPU solver (sequential / OpenMP). See wave3d/cpu.hpp.
//
// Reference programs: `wave` (sequential, readme.md:33-36) and `openmpwave`/`wave3dOMP` (report.pdf p.21 §5.2). Phase
// timers follow the reference's CPU breakdown columns init / compute / (check) (report.pdf p.16 §4.4).
#include <algorithm>
#include <chrono>
#include <cmath>

#include "wave3d/cpu.hpp"

namespace wave3d {

namespace {
double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace

CpuSolver::CpuSolver(const Problem& p, int check_every, int threads) : prob_(p), check_every_(check_every) {
  prob_.validate();
  cpu_set_threads(threads);
  Box b{0, p.N + 1, 0, p.N + 1, 0, p.N + 1};
  lay_ = make_layout(prob_, b);
  u_[0].assign(static_cast<size_t>(lay_.total), 0.0);
  u_[1].assign(static_cast<size_t>(lay_.total), 0.0);
  if (prob_.time_order == 4) v_.assign(static_cast<size_t>(lay_.total), 0.0);  // (only cpu_lap4 writes it: the faces stay 0)
  s_ = sin_table_ext(prob_);
  if (prob_.sponge.on()) sponge_ = sponge_tables(prob_);
}

void global_to_local(const Layout& l, const double* g, double* out) {
  const i64 n1 = l.N + 1;
  std::fill(out, out + l.total, 0.0);
#pragma omp parallel for schedule(static)
  for (i64 x = -l.xg; x < l.nx + l.xg; ++x) {
    const i64 gx = l.gx0 + x;
    if (gx < 0 || gx > l.N) continue;
    for (i64 y = -l.yg; y < l.ny + l.yg; ++y) {
      const i64 gy = l.gy0 + y;
      if (gy < 0 || gy > l.N) continue;
      const i64 z0 = imax(-l.zg, -l.gz0), z1 = imin(l.nz + l.zg, n1 - l.gz0);
      if (z1 <= z0) continue;
      std::copy(g + (gx * n1 + gy) * n1 + l.gz0 + z0, g + (gx * n1 + gy) * n1 + l.gz0 + z1, out + l.off(x, y, z0));
    }
  }
}

void initial_to_local(const Layout& l, const double* g, double* out) {
  global_to_local(l, g, out);
  // the six global faces: exact zeros whatever the arrays hold there (homogeneous Dirichlet)
#pragma omp parallel for schedule(static)
  for (i64 x = -l.xg; x < l.nx + l.xg; ++x) {
    const i64 gx = l.gx0 + x;
    if (gx < 0 || gx > l.N) continue;
    for (i64 y = -l.yg; y < l.ny + l.yg; ++y) {
      const i64 gy = l.gy0 + y;
      if (gy < 0 || gy > l.N) continue;
      const bool face = gx == 0 || gx == l.N || gy == 0 || gy == l.N;
      for (i64 z = -l.zg; z < l.nz + l.zg; ++z) {
        const i64 gz = l.gz0 + z;
        if (gz >= 0 && gz <= l.N && (face || gz == 0 || gz == l.N)) out[l.off(x, y, z)] = 0.0;
      }
    }
  }
}

SpeedRange speed_to_local(const Problem& p, const Layout& l, const double* c, double* lamf, double* c2) {
  W3D_REQUIRE(c != nullptr, "speed: no coefficient field");
  const i64 N = p.N, n1 = N + 1;
  SpeedRange r;
  bool bad = false;
  double lo = HUGE_VAL, hi = 0.0;
  // every rank checks the whole global interior, so a refusal and the range do not depend on the decomposition
#pragma omp parallel for schedule(static) reduction(min : lo) reduction(max : hi) reduction(|| : bad)
  for (i64 x = 1; x < N; ++x)
    for (i64 y = 1; y < N; ++y)
      for (i64 z = 1; z < N; ++z) {
        const double v = c[(x * n1 + y) * n1 + z];
        if (!(std::isfinite(v) && v > 0.0)) bad = true;
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
      }
  W3D_REQUIRE(!bad, "speed: every interior value of c must be finite and > 0");
  r.cmin = lo;
  r.cmax = hi;
  const double lam = Coeffs::from(p).lam;
  for (double* out : {lamf, c2})
    if (out) std::fill(out, out + l.total, 0.0);
#pragma omp parallel for schedule(static)
  for (i64 x = -l.xg; x < l.nx + l.xg; ++x) {
    const i64 gx = l.gx0 + x;
    if (gx <= 0 || gx >= N) continue;
    for (i64 y = -l.yg; y < l.ny + l.yg; ++y) {
      const i64 gy = l.gy0 + y;
      if (gy <= 0 || gy >= N) continue;
      for (i64 z = -l.zg; z < l.nz + l.zg; ++z) {
        const i64 gz = l.gz0 + z;
        if (gz <= 0 || gz >= N) continue;
        const double v = c[(gx * n1 + gy) * n1 + gz];
        const double v2 = v * v;
        const i64 o = l.off(x, y, z);
        if (c2) c2[o] = v2;
        if (lamf) lamf[o] = lam * v2;
      }
    }
  }
  return r;
}

void speed_cfl(const Problem& p, const SpeedRange& r, bool force) {
  const double cn = p.courant() * r.cmax;
  W3D_REQUIRE(force || cn <= 1.0, "speed: CFL violated: courant * max c = " + std::to_string(cn) +
                                      " > 1 (max c = " + std::to_string(r.cmax) + "); use a smaller tau, or force");
}

void CpuSolver::set_speed(const double* c, bool force) {
  W3D_REQUIRE(!c || prob_.order == 2, "order: no speed field with order = 4 (the coefficient form of the fourth-order "
                                      "operator is a follow-up)");
  if (!c) {
    lamf_.clear();
    c2_.clear();
    speed_range_ = SpeedRange{};
    runs_ = 0;
    return;
  }
  std::vector<double> lamf(static_cast<size_t>(lay_.total)), c2(static_cast<size_t>(lay_.total));
  const SpeedRange r = speed_to_local(prob_, lay_, c, lamf.data(), c2.data());
  speed_cfl(prob_, r, force);
  lamf_ = std::move(lamf);
  c2_ = std::move(c2);
  speed_range_ = r;
  runs_ = 0;
}

void CpuSolver::set_initial(const double* phi, const double* psi) {
  W3D_REQUIRE(1 < prob_.K, "resume step must be in [1, K)");
  init_lay_ = initial_layout(prob_, lay_);
  for (int k = 0; k < 2; ++k) {
    const double* g = k == 0 ? phi : psi;
    init_[k].clear();
    if (!g) continue;
    init_[k].assign(static_cast<size_t>(init_lay_.total), 0.0);
    initial_to_local(init_lay_, g, init_[k].data());
  }
  initial_ = true;
  resume_n_ = 0;
  resume_[0].clear();
  resume_[1].clear();
  runs_ = 0;
}

EnergySums CpuSolver::energy_sums(int which) const {
  W3D_REQUIRE(which == 0 || which == 1, "energy: which is 0 (E at K-1/2) or 1 (E at 1/2)");
  W3D_REQUIRE(prob_.order == 2, "order: the second-order discrete energy is not the conserved quantity of the order = 4 scheme");
  W3D_REQUIRE(runs_ > 0, "energy: no solve has run yet");
  if (which == 1) {
    W3D_REQUIRE(initial_ || speed(), "energy: E(1/2) is kept by solves that start from set_initial");
    return e_start_;
  }
  return cpu_energy(lay_, Coeffs::from(prob_), prob_.tau, field(1).data(), field(0).data(), speed() ? c2_.data() : nullptr);
}

double CpuSolver::energy(int which) const {
  const EnergySums e = energy_sums(which);
  return energy_value(prob_, e.kin, e.pot);
}

void CpuSolver::set_state(const double* prev, const double* cur, int n0) {
  W3D_REQUIRE(prob_.order == 2, "order: not together with set_state / --resume");
  W3D_REQUIRE(n0 >= 1 && n0 < prob_.K, "resume step must be in [1, K)");
  W3D_REQUIRE(src_off_.empty(), "sources: not together with set_state (a resumed solve has no step 0 to start the "
                                "wavelet from)");
  initial_ = false;
  init_[0].clear();
  init_[1].clear();
  for (int k = 0; k < 2; ++k) {
    resume_[k].assign(static_cast<size_t>(lay_.total), 0.0);
    global_to_local(lay_, k == 0 ? prev : cur, resume_[k].data());
  }
  resume_n_ = n0;
}

void CpuSolver::set_receivers(const i64* ijk, int R) {
  W3D_REQUIRE(R >= 0 && (R == 0 || ijk != nullptr), "set_receivers: bad receiver list");
  std::vector<i64> off;
  for (int r = 0; r < R; ++r) {
    const i64 i = ijk[3 * r], j = ijk[3 * r + 1], k = ijk[3 * r + 2];
    W3D_REQUIRE(i >= 0 && i <= prob_.N && j >= 0 && j <= prob_.N && k >= 0 && k <= prob_.N,
                "receiver " + std::to_string(r) + " = (" + std::to_string(i) + ", " + std::to_string(j) + ", " +
                    std::to_string(k) + ") is outside the grid 0.." + std::to_string(prob_.N));
    off.push_back(lay_.off(i, j, k));
  }
  recv_off_ = std::move(off);
  traces_.clear();
}

std::vector<double> source_addends(const Problem& p, const i64* ijk, int Q, const double* w) {
  W3D_REQUIRE(Q >= 0 && (Q == 0 || (ijk != nullptr && w != nullptr)), "sources: bad source list");
  for (int q = 0; q < Q; ++q) {
    const i64 i = ijk[3 * q], j = ijk[3 * q + 1], k = ijk[3 * q + 2];
    W3D_REQUIRE(i > 0 && i < p.N && j > 0 && j < p.N && k > 0 && k < p.N,
                "sources: source " + std::to_string(q) + " = (" + std::to_string(i) + ", " + std::to_string(j) + ", " +
                    std::to_string(k) + ") is not strictly inside the grid 1.." + std::to_string(p.N - 1) +
                    " (a node on a global face or outside the grid)");
  }
  std::vector<double> a(static_cast<size_t>(p.K) * static_cast<size_t>(Q));
  for (size_t m = 0; m < a.size(); ++m) {
    W3D_REQUIRE(std::isfinite(w[m]), "sources: w[" + std::to_string(m / static_cast<size_t>(Q)) + "][" +
                                         std::to_string(m % static_cast<size_t>(Q)) + "] is not finite");
    a[m] = source_addend(p, w[m]);
    W3D_REQUIRE(std::isfinite(a[m]), "sources: the scaled sample tau^2 w / (hx hy hz) overflows");
  }
  return a;
}

void CpuSolver::set_sources(const i64* ijk, int Q, const double* w) {
  W3D_REQUIRE(Q == 0 || prob_.time_order == 2, "time_order: no point sources with time_order = 4 (the forcing's tau^4 terms "
                                               "are a follow-up)");
  W3D_REQUIRE(Q == 0 || resume_n_ == 0, "sources: not together with set_state (a resumed solve has no step 0 to start "
                                        "the wavelet from)");
  std::vector<double> a = source_addends(prob_, ijk, Q, w);
  src_off_.clear();
  for (int q = 0; q < Q; ++q) src_off_.push_back(lay_.off(ijk[3 * q], ijk[3 * q + 1], ijk[3 * q + 2]));
  src_a_ = std::move(a);
}

std::vector<int> CpuSolver::check_steps() const {
  std::vector<int> v;
  for (int n = 1; n <= prob_.K; ++n)
    if ((check_every_ > 0 && n % check_every_ == 0) || n == prob_.K) v.push_back(n);
  return v;
}

CpuResult CpuSolver::run() {
  CpuResult r;
  const Coeffs c = Coeffs::from(prob_);
  const double* s = s_.data() + 1;
  // sponge layers: every step is the damped one (cpu_leapfrog's table argument); the start levels are what they are
  const SpongeView sponge_view = prob_.sponge.on() ? sponge_.view() : SpongeView{};
  const SpongeView* sp = prob_.sponge.on() ? &sponge_view : nullptr;
  const double* lamf = speed() ? lamf_.data() : nullptr;  // (a speed field: the coefficient per node)
  const LBox box = compute_box(lay_);
  const double n_int = static_cast<double>(prob_.N - 1);
  const double denom = n_int * n_int * n_int;
  std::vector<char> is_check(static_cast<size_t>(prob_.K + 1), 0);
  for (int n : check_steps()) is_check[static_cast<size_t>(n)] = 1;
  auto record = [&](int n, const ErrAcc& a) {
    r.steps.push_back(n);
    r.max_err.push_back(a.max);
    r.rms_err.push_back(std::sqrt(a.sum / denom));
    if (!std::isfinite(a.max) || !std::isfinite(a.sum)) r.finite = false;
  };
  const double t0 = now_s();
  const int n_start = resume_n_ > 0 ? resume_n_ : 1;
  if (resume_n_ > 0) {
    u_[0] = resume_[0];
    u_[1] = resume_[1];
  } else if (prob_.time_order == 4) {
    // time order 4: φ (set_initial's, or the eigenmode array) and ψ through cpu_first_step_t4
    std::vector<double> phi0;
    Layout il = init_lay_;
    if (!initial_) {
      il = initial_layout(prob_, lay_);
      phi0 = eigenmode_local(prob_, il);
    }
    cpu_first_step_t4(lay_, il, c, prob_.tau, initial_ ? init_[0].data() : phi0.data(),
                      initial_ && !init_[1].empty() ? init_[1].data() : nullptr, v_.data(), u_[0].data(), u_[1].data());
  } else if (initial_) {
    cpu_first_step_field(lay_, init_lay_, c, prob_.tau, init_[0].data(), init_[1].empty() ? nullptr : init_[1].data(),
                         u_[0].data(), u_[1].data(), lamf);
    if (prob_.order == 2) e_start_ = cpu_energy(lay_, c, prob_.tau, u_[0].data(), u_[1].data(), lamf ? c2_.data() : nullptr);
  } else if (prob_.order == 4) {
    // order 4 without set_initial: the eigenmode array through the first-step-field path, as a speed solve starts
    const Layout il = initial_layout(prob_, lay_);
    std::vector<double> phi0 = eigenmode_local(prob_, il);
    cpu_first_step_field(lay_, il, c, prob_.tau, phi0.data(), nullptr, u_[0].data(), u_[1].data(), nullptr);
  } else if (lamf) {
    // a speed field without set_initial: the eigenmode array through the first-step-field path (u⁰ is cpu_init_first's)
    const Layout il = initial_layout(prob_, lay_);
    std::vector<double> phi0 = eigenmode_local(prob_, il);
    cpu_first_step_field(lay_, il, c, prob_.tau, phi0.data(), nullptr, u_[0].data(), u_[1].data(), lamf);
    e_start_ = cpu_energy(lay_, c, prob_.tau, u_[0].data(), u_[1].data(), c2_.data());
  } else {
    cpu_init_first(lay_, c, s, u_[0].data(), u_[1].data());
  }
  // sources: level m + 1 gets a^m at every source node, in list order (the start level u¹: ½·a⁰)
  const size_t nsrc = src_off_.size();
  auto add_sources = [&](int m, double scale, std::vector<double>& u) {
    for (size_t q = 0; q < nsrc; ++q)
      u[static_cast<size_t>(src_off_[q])] += scale * src_a_[static_cast<size_t>(m) * nsrc + q];
  };
  if (nsrc > 0) add_sources(0, 0.5, u_[1]);
  const size_t nrec = recv_off_.size();
  auto trace_row = [&](int n, const std::vector<double>& u) {
    for (size_t k = 0; k < nrec; ++k) traces_[static_cast<size_t>(n) * nrec + k] = u[static_cast<size_t>(recv_off_[k])];
  };
  if (nrec > 0) {
    traces_.assign(static_cast<size_t>(prob_.K + 1) * nrec, std::nan(""));
    trace_row(n_start - 1, u_[0]);
    trace_row(n_start, u_[1]);
  }
  const double t1 = now_s();
  r.init_s = t1 - t0;
  if (is_check[1] && resume_n_ == 0) {
    ErrAcc a;
    cpu_error(lay_, u_[1].data(), box, s, time_factor(prob_, 1), &a);
    record(1, a);
  }
  int cur = 1, old = 0;
  for (int n = n_start; n <= prob_.K - 1; ++n) {
    const double tc = now_s();
    if (prob_.time_order == 4) {
      const bool chk = is_check[static_cast<size_t>(n + 1)] != 0;
      ErrAcc a;
      cpu_lap4(lay_, c, u_[cur].data(), v_.data(), box);
      cpu_leapfrog44(lay_, c, u_[cur].data(), v_.data(), u_[old].data(), box, s, chk ? time_factor(prob_, n + 1) : 0.0,
                     chk ? &a : nullptr);
      if (chk) record(n + 1, a);
    } else if (is_check[static_cast<size_t>(n + 1)]) {
      ErrAcc a;
      cpu_leapfrog(lay_, c, u_[cur].data(), u_[old].data(), box, s, time_factor(prob_, n + 1), &a, sp, lamf);
      record(n + 1, a);
    } else {
      cpu_leapfrog(lay_, c, u_[cur].data(), u_[old].data(), box, s, 0.0, nullptr, sp, lamf);
    }
    r.compute_s += now_s() - tc;
    std::swap(cur, old);
    if (nsrc > 0) add_sources(n, 1.0, u_[cur]);
    if (nrec > 0) trace_row(n + 1, u_[cur]);
  }
  final_ = cur;
  ++runs_;
  r.solve_s = now_s() - t0;
  r.slow_phases[0] = r.init_s;
  r.slow_phases[1] = r.compute_s;
  return r;
}

}  // namespace wave3d
