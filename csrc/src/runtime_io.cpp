// Field dumps and checkpoints of the native runtime: wave3d-dump-v1 (SURVEY.md §5.9 — the reference writes no field
// at all, report.pdf / readme.md have only stdout). See wave3d/runtime.hpp.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "wave3d/runtime.hpp"

namespace wave3d {

void write_dump(const std::string& prefix, const Problem& p, const Layout& l, const std::vector<double>& u, int rank,
                int world, const Dims& d, int step, const SpeedRange* speed) {
  if (step < 0) step = p.K;
  const std::string base = world > 1 ? prefix + ".rank" + std::to_string(rank) : prefix;
  std::ofstream f(base + ".bin", std::ios::binary | std::ios::trunc);
  std::vector<double> row(static_cast<size_t>(l.nz));
  for (i64 ix = 0; ix < l.nx; ++ix)
    for (i64 iy = 0; iy < l.ny; ++iy) {
      const double* src = u.data() + l.off(ix, iy, 0);
      std::memcpy(row.data(), src, row.size() * sizeof(double));
      f.write(reinterpret_cast<const char*>(row.data()), static_cast<std::streamsize>(row.size() * sizeof(double)));
    }
  std::ofstream j(base + ".json", std::ios::trunc);
  j.precision(17);
  j << "{\"format\": \"wave3d-dump-v1\", \"dtype\": \"float64\", \"order\": \"C\", \"N\": " << p.N
    << ", \"L\": " << p.L;
  // (a rectangular box: its three edges under a key of their own; a cube's sidecar is what it always was)
  if (p.is_box()) j << ", \"box\": [" << p.L << ", " << p.edge_y() << ", " << p.edge_z() << "]";
  // (sponge layers: width, sigma as given (0: the default), face mask; absent without a sponge)
  if (p.sponge.on())
    j << ", \"sponge\": [" << p.sponge.width << ", " << p.sponge.sigma << ", " << p.sponge.faces << "]";
  // (a speed field: the interior minimum and maximum of c; absent without one)
  if (speed) j << ", \"speed\": [" << speed->cmin << ", " << speed->cmax << "]";
  // (the spatial order, when it is not 2 — "order" is the array's memory order here; absent for order 2)
  if (p.order != 2) j << ", \"space_order\": " << p.order;
  if (p.time_order != 2) j << ", \"time_order\": " << p.time_order;
  j << ", \"tau\": " << p.tau << ", \"step\": " << step << ", \"t\": " << step * p.tau
    << ", \"shape\": [" << l.nx << ", " << l.ny << ", " << l.nz << "], \"offset\": [" << l.gx0 << ", " << l.gy0
    << ", " << l.gz0 << "], \"global_shape\": [" << p.N + 1 << ", " << p.N + 1 << ", " << p.N + 1
    << "], \"rank\": " << rank << ", \"world\": " << world << ", \"dims\": [" << d.px << ", " << d.py << ", " << d.pz
    << "]}\n";
}

// --checkpoint PREFIX: u^K → PREFIX.cur, u^{K−1} → PREFIX.prev (wave3d-dump-v1, per rank when world > 1)
void write_checkpoint(const std::string& prefix, const Problem& p, const Layout& l, const std::vector<double>& cur,
                      const std::vector<double>& prev, int rank, int world, const Dims& d) {
  write_dump(prefix + ".cur", p, l, cur, rank, world, d, p.K);
  write_dump(prefix + ".prev", p, l, prev, rank, world, d, p.K - 1);
}

// Number after "key": in a one-line JSON object (the dump sidecars this program writes).
std::vector<double> json_numbers(const std::string& text, const std::string& key) {
  std::vector<double> out;
  const size_t k = text.find("\"" + key + "\"");
  if (k == std::string::npos) return out;
  size_t i = text.find(':', k) + 1;
  const bool list = text.find_first_not_of(" ", i) != std::string::npos && text[text.find_first_not_of(" ", i)] == '[';
  if (list) i = text.find('[', i) + 1;
  for (;;) {
    char* end = nullptr;
    const double v = std::strtod(text.c_str() + i, &end);
    if (end == text.c_str() + i) break;
    out.push_back(v);
    i = static_cast<size_t>(end - text.c_str());
    if (!list) break;
    i = text.find_first_of(",]", i);
    if (i == std::string::npos || text[i] == ']') break;
    ++i;
  }
  return out;
}

// The GLOBAL (N+1)³ field of a dump PREFIX (one file, or PREFIX.rankR of any decomposition); returns its step.
int load_dump_global(const std::string& prefix, const Problem& p, std::vector<double>& g, const std::string& what) {
  auto slurp = [](const std::string& path) {
    std::ifstream f(path);
    return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  };
  std::string meta = slurp(prefix + ".json");
  std::vector<std::string> bases;
  if (!meta.empty()) {
    bases.push_back(prefix);
  } else {
    meta = slurp(prefix + ".rank0.json");
    W3D_REQUIRE(!meta.empty(), what + ": no dump " + prefix + ".json or " + prefix + ".rank0.json");
    const std::vector<double> w = json_numbers(meta, "world");
    W3D_REQUIRE(!w.empty() && w[0] >= 1, what + ": dump without a world size");
    for (int r = 0; r < static_cast<int>(w[0]); ++r) bases.push_back(prefix + ".rank" + std::to_string(r));
  }
  const i64 n1 = p.N + 1;
  g.assign(static_cast<size_t>(n1 * n1 * n1), 0.0);
  int step = -1;
  for (const std::string& b : bases) {
    const std::string m = slurp(b + ".json");
    const std::vector<double> sh = json_numbers(m, "shape"), of = json_numbers(m, "offset"), st = json_numbers(m, "step"),
                              nn = json_numbers(m, "N");
    W3D_REQUIRE(sh.size() == 3 && of.size() == 3 && st.size() == 1 && nn.size() == 1, what + ": bad sidecar " + b);
    W3D_REQUIRE(static_cast<i64>(nn[0]) == p.N, what + ": dump N differs from the run's N");
    // (tau and L too: a checkpoint of another problem would continue from an inconsistent state; the sidecar holds
    // them with 17 significant digits, so they round-trip exactly)
    for (const auto& [key, want] : {std::pair<const char*, double>{"tau", p.tau}, {"L", p.L}}) {
      const std::vector<double> v = json_numbers(m, key);
      W3D_REQUIRE(v.size() == 1 && std::fabs(v[0] - want) <= 1e-15 * std::fabs(want),
                  std::string(what + ": dump ") + key + " differs from the run's " + key);
    }
    // (the box: a sidecar without the key is a cube of edge L, as every dump written before boxes existed)
    {
      const std::vector<double> bx = json_numbers(m, "box"), ll = json_numbers(m, "L");
      W3D_REQUIRE(bx.empty() || bx.size() == 3, what + ": bad box in sidecar " + b);
      const double have[3] = {bx.empty() ? ll[0] : bx[0], bx.empty() ? ll[0] : bx[1], bx.empty() ? ll[0] : bx[2]};
      const double want[3] = {p.L, p.edge_y(), p.edge_z()};
      for (int a = 0; a < 3; ++a)
        W3D_REQUIRE(std::fabs(have[a] - want[a]) <= 1e-15 * std::fabs(want[a]),
                    what + ": dump box differs from the run's box");
    }
    W3D_REQUIRE(step < 0 || step == static_cast<int>(st[0]), what + ": rank dumps of different steps");
    step = static_cast<int>(st[0]);
    const i64 nx = static_cast<i64>(sh[0]), ny = static_cast<i64>(sh[1]), nz = static_cast<i64>(sh[2]);
    const i64 x0 = static_cast<i64>(of[0]), y0 = static_cast<i64>(of[1]), z0 = static_cast<i64>(of[2]);
    W3D_REQUIRE(x0 >= 0 && y0 >= 0 && z0 >= 0 && x0 + nx <= n1 && y0 + ny <= n1 && z0 + nz <= n1,
                what + ": dump box outside the grid");
    std::ifstream f(b + ".bin", std::ios::binary);
    W3D_REQUIRE(static_cast<bool>(f), what + ": cannot read " + b + ".bin");
    for (i64 x = 0; x < nx; ++x)
      for (i64 y = 0; y < ny; ++y)
        f.read(reinterpret_cast<char*>(g.data() + ((x0 + x) * n1 + (y0 + y)) * n1 + z0),
               static_cast<std::streamsize>(nz * static_cast<i64>(sizeof(double))));
    W3D_REQUIRE(static_cast<bool>(f), what + ": short file " + b + ".bin");
  }
  return step;
}

std::vector<i64> load_receivers(const std::string& path) {
  std::ifstream f(path);
  W3D_REQUIRE(static_cast<bool>(f), "receivers: cannot read " + path);
  std::vector<i64> ijk;
  std::string line;
  for (int no = 1; std::getline(f, line); ++no) {
    const size_t b = line.find_first_not_of(" \t\r");
    if (b == std::string::npos || line[b] == '#') continue;
    long long i = 0, j = 0, k = 0;
    char extra = 0;
    W3D_REQUIRE(std::sscanf(line.c_str(), "%lld %lld %lld %c", &i, &j, &k, &extra) == 3,
                "receivers: " + path + " line " + std::to_string(no) + ": expected three integers i j k");
    ijk.insert(ijk.end(), {static_cast<i64>(i), static_cast<i64>(j), static_cast<i64>(k)});
  }
  W3D_REQUIRE(!ijk.empty(), "receivers: " + path + " lists no node");
  return ijk;
}

void write_traces(const std::string& out, const Problem& p, const std::vector<i64>& ijk,
                  const std::vector<double>& values) {
  const size_t R = ijk.size() / 3, rows = static_cast<size_t>(p.K + 1);
  W3D_REQUIRE(values.size() == rows * R, "traces: " + std::to_string(values.size()) + " values for " +
                                             std::to_string(rows) + " x " + std::to_string(R));
  std::ofstream f(out + ".bin", std::ios::binary | std::ios::trunc);
  f.write(reinterpret_cast<const char*>(values.data()), static_cast<std::streamsize>(values.size() * sizeof(double)));
  W3D_REQUIRE(static_cast<bool>(f), "traces: cannot write " + out + ".bin");
  std::ofstream j(out + ".json", std::ios::trunc);
  j.precision(17);
  j << "{\"format\": \"wave3d-traces-v1\", \"dtype\": \"float64\", \"order\": \"C\", \"N\": " << p.N << ", \"K\": " << p.K
    << ", \"L\": " << p.L;
  if (p.is_box()) j << ", \"box\": [" << p.L << ", " << p.edge_y() << ", " << p.edge_z() << "]";
  if (p.order != 2) j << ", \"space_order\": " << p.order;
  if (p.time_order != 2) j << ", \"time_order\": " << p.time_order;
  j << ", \"tau\": " << p.tau << ", \"shape\": [" << rows << ", " << R << "], \"nodes\": [";
  for (size_t r = 0; r < R; ++r)
    j << (r ? ", [" : "[") << ijk[3 * r] << ", " << ijk[3 * r + 1] << ", " << ijk[3 * r + 2] << "]";
  j << "]}\n";
}

int load_sources(const std::string& path, const Problem& p, std::vector<i64>& ijk, std::vector<double>& w) {
  std::ifstream f(path);
  W3D_REQUIRE(static_cast<bool>(f), "sources: cannot read " + path);
  ijk.clear();
  std::vector<double> par;  // f0, t0, amp per source
  std::string line;
  for (int no = 1; std::getline(f, line); ++no) {
    const size_t b = line.find_first_not_of(" \t\r");
    if (b == std::string::npos || line[b] == '#') continue;
    long long i = 0, j = 0, k = 0;
    double f0 = 0.0, t0 = 0.0, amp = 0.0;
    char extra = 0;
    W3D_REQUIRE(std::sscanf(line.c_str(), "%lld %lld %lld %lf %lf %lf %c", &i, &j, &k, &f0, &t0, &amp, &extra) == 6,
                "sources: " + path + " line " + std::to_string(no) + ": expected i j k f0 t0 amp");
    ijk.insert(ijk.end(), {static_cast<i64>(i), static_cast<i64>(j), static_cast<i64>(k)});
    par.insert(par.end(), {f0, t0, amp});
  }
  W3D_REQUIRE(!ijk.empty(), "sources: " + path + " lists no source");
  const size_t Q = ijk.size() / 3;
  w.assign(static_cast<size_t>(p.K) * Q, 0.0);
  for (int m = 0; m < p.K; ++m)
    for (size_t q = 0; q < Q; ++q) {
      const double t = static_cast<double>(m) * p.tau - par[3 * q + 1];
      const double x = (M_PI * par[3 * q] * t) * (M_PI * par[3 * q] * t);
      w[static_cast<size_t>(m) * Q + q] = (1.0 - 2.0 * x) * std::exp(-x) * par[3 * q + 2];
    }
  return static_cast<int>(Q);
}

// --resume PREFIX: u^{n0−1} from PREFIX.prev, u^{n0} from PREFIX.cur; returns n0
int load_checkpoint(const std::string& prefix, const Problem& p, std::vector<double>& prev, std::vector<double>& cur) {
  const int sc = load_dump_global(prefix + ".cur", p, cur);
  const int sp = load_dump_global(prefix + ".prev", p, prev);
  W3D_REQUIRE(sp == sc - 1, "resume: PREFIX.prev must hold the step before PREFIX.cur");
  W3D_REQUIRE(sc >= 1 && sc < p.K, "resume: checkpoint step " + std::to_string(sc) + " is not before K");
  return sc;
}

// --initial PREFIX: φ from PREFIX.phi, ψ from PREFIX.psi when that dump exists (psi left empty otherwise)
void load_initial(const std::string& prefix, const Problem& p, std::vector<double>& phi, std::vector<double>& psi) {
  load_dump_global(prefix + ".phi", p, phi, "initial");
  psi.clear();
  const bool have = std::ifstream(prefix + ".psi.json").good() || std::ifstream(prefix + ".psi.rank0.json").good();
  if (have) load_dump_global(prefix + ".psi", p, psi, "initial");
}

void load_speed(const std::string& prefix, const Problem& p, std::vector<double>& c) {
  load_dump_global(prefix + ".c", p, c, "speed");
}

}  // namespace wave3d
