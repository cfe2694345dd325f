// Python bindings of the native runtime (pybind11). Module: mpi_cuda_amd._C
//
// The GPU path is fully native (GpuSolver: HIP kernels + RCCL, C++ step loop, hipGraph). The raw kernel launchers take
// device pointers as integers (torch.Tensor.data_ptr()) and a stream handle (torch.cuda.current_stream().cuda_stream)
// so the tests can drive each kernel against a PyTorch fp64 reference. The CPU kernels take numpy float64 arrays.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <array>
#include <cstring>
#include <tuple>

#include "wave3d/capture_guard.hpp"
#include "wave3d/cpu.hpp"
#include "wave3d/decomp.hpp"
#include "wave3d/kernels.hpp"
#include "wave3d/pass_grid.hpp"
#include "wave3d/problem.hpp"
#include "wave3d/runtime.hpp"
#include "wave3d/solver.hpp"
#include "wave3d/stencil.hpp"

namespace py = pybind11;
using namespace wave3d;

namespace {

using darr = py::array_t<double, py::array::c_style | py::array::forcecast>;

double* mut_ptr(darr& a, i64 need, const char* what) {
  W3D_REQUIRE(a.size() >= need, std::string(what) + ": array too small");
  return a.mutable_data();
}
const double* ro_ptr(const darr& a, i64 need, const char* what) {
  W3D_REQUIRE(a.size() >= need, std::string(what) + ": array too small");
  return a.data();
}

// receivers: an (R, 3) integer array of global node indices
using iarr = py::array_t<i64, py::array::c_style | py::array::forcecast>;
const i64* receiver_ptr(const iarr& a, int* R) {
  W3D_REQUIRE(a.size() == 0 || (a.ndim() == 2 && a.shape(1) == 3), "receivers: an (R, 3) integer array of node indices");
  *R = a.size() == 0 ? 0 : static_cast<int>(a.shape(0));
  return a.data();
}
std::vector<std::array<i64, 3>> receiver_nodes(const iarr& a) {
  int R = 0;
  const i64* p = receiver_ptr(a, &R);
  std::vector<std::array<i64, 3>> v(static_cast<size_t>(R));
  for (int r = 0; r < R; ++r) v[static_cast<size_t>(r)] = {p[3 * r], p[3 * r + 1], p[3 * r + 2]};
  return v;
}

// sources: an (Q, 3) integer array of global node indices and the (K, Q) wavelet samples
const double* source_w(const Problem& p, const iarr& nodes, const darr& w, int* Q) {
  W3D_REQUIRE(nodes.size() == 0 || (nodes.ndim() == 2 && nodes.shape(1) == 3),
              "sources: an (Q, 3) integer array of node indices");
  *Q = nodes.size() == 0 ? 0 : static_cast<int>(nodes.shape(0));
  W3D_REQUIRE(*Q == 0 || (w.ndim() == 2 && w.shape(0) == p.K && w.shape(1) == *Q),
              "sources: w must have shape (K, Q) = (" + std::to_string(p.K) + ", " + std::to_string(*Q) +
                  "): row m = the sources' samples at t = m tau");
  return w.data();
}

template <class T>
T* dptr(std::uintptr_t p) {
  return reinterpret_cast<T*>(p);
}
hipStream_t sptr(std::uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

// The flat argument list that the Python pass launchers (gpu_leapfrog_tb, gpu_leapfrog_p2_boxes) share, in their
// order, as the launchers' struct.
PassArgs py_pass_args(std::uintptr_t prev, std::uintptr_t cur, std::uintptr_t out1, std::uintptr_t out2,
                      std::uintptr_t s, const std::vector<double>& ct, int check_mask, std::uintptr_t partials,
                      const LeapfrogTbTiling& t, const LBox& real, bool analytic_start, int level_stride,
                      int grid_blocks, std::uintptr_t lamf = 0) {
  PassArgs a;
  a.lamf = dptr<const double>(lamf);  // (a speed field's device array in `layout`; 0: constant speed)
  a.prev = dptr<const double>(prev);
  a.cur = dptr<const double>(cur);
  a.out1 = dptr<double>(out1);
  a.out2 = dptr<double>(out2);
  a.d_s = dptr<const double>(s) + 1;
  std::copy_n(ct.begin(), std::min<size_t>(ct.size(), 5), a.ct);
  a.check_mask = check_mask;
  a.partials = dptr<Partial>(partials);
  a.level_stride = level_stride;
  a.grid_blocks = grid_blocks;
  a.tiling = t;
  a.real = real;
  a.analytic_start = analytic_start;
  return a;
}

py::dict result_dict(const RunResult& r) {
  py::dict d;
  d["steps"] = r.steps;
  d["max_err"] = r.max_err;
  d["rms_err"] = r.rms_err;
  d["solve_s"] = r.solve_s;
  d["batched"] = r.batched;
  d["finite"] = r.finite;
  py::dict ph;
  ph["init_ms"] = r.phases.init_ms;
  ph["shell_ms"] = r.phases.shell_ms;
  ph["compute_ms"] = r.phases.interior_ms;
  ph["comm_ms"] = r.phases.comm_ms;
  ph["check_ms"] = r.phases.check_ms;
  ph["gather_ms"] = r.phases.gather_ms;
  d["phases"] = ph;
  py::list tr;
  for (const UnitTrace& t : r.trace) {
    py::dict u;
    u["unit"] = t.unit;
    u["n"] = t.n;
    u["steps"] = t.steps;
    u["shell_ms"] = t.shell_ms;
    u["comm_ms"] = t.comm_ms;
    u["compute_ms"] = t.compute_ms;
    u["check_ms"] = t.check_ms;
    tr.append(u);
  }
  d["trace"] = tr;
  return d;
}

}  // namespace

PYBIND11_MODULE(_C, m) {
  m.doc() = "wave3d native runtime: CDNA4 HIP kernels, RCCL halo exchange, CPU/OpenMP path";

  py::class_<Sponge>(m, "Sponge")
      .def(py::init([](int width, double sigma, int faces) { return Sponge{width, sigma, faces}; }),
           py::arg("width") = 0, py::arg("sigma") = 0.0, py::arg("faces") = 63)
      .def_readwrite("width", &Sponge::width)
      .def_readwrite("sigma", &Sponge::sigma)
      .def_readwrite("faces", &Sponge::faces)
      .def_property_readonly("on", &Sponge::on);
  py::class_<Problem>(m, "Problem")
      .def(py::init([](i64 N, double tau, int K, double L, double Ly, double Lz, const Sponge& sponge, int order,
                       int time_order) {
             Problem p;
             p.N = N;
             p.tau = tau;
             p.K = K;
             p.L = L;
             p.Ly = Ly;
             p.Lz = Lz;
             p.sponge = sponge;
             p.order = order;
             p.time_order = time_order;
             p.validate();
             return p;
           }),
           py::arg("N") = 512, py::arg("tau") = 1e-3, py::arg("K") = 20, py::arg("L") = 1.0, py::kw_only(),
           py::arg("Ly") = 0.0, py::arg("Lz") = 0.0, py::arg("sponge") = Sponge{}, py::arg("order") = 2,
           py::arg("time_order") = 2)
      .def_readwrite("sponge", &Problem::sponge)
      .def_readwrite("order", &Problem::order)
      .def_readwrite("time_order", &Problem::time_order)
      .def_property_readonly("courant_limit", &Problem::courant_limit)
      .def_property_readonly("courant_eff", &Problem::courant_eff)
      .def_property_readonly("cfl_ok_eff", &Problem::cfl_ok_eff)
      .def("validate", &Problem::validate)
      .def_readwrite("N", &Problem::N)
      .def_readwrite("tau", &Problem::tau)
      .def_readwrite("K", &Problem::K)
      .def_readwrite("L", &Problem::L)
      .def_readwrite("Ly", &Problem::Ly)
      .def_readwrite("Lz", &Problem::Lz)
      .def_property_readonly("edges",
                             [](const Problem& p) { return py::make_tuple(p.L, p.edge_y(), p.edge_z()); })
      .def_property_readonly("is_box", &Problem::is_box)
      .def_property_readonly("hx", &Problem::hx)
      .def_property_readonly("hy", &Problem::hy)
      .def_property_readonly("hz", &Problem::hz)
      .def_property_readonly("h", &Problem::h)
      .def_property_readonly("a_t", &Problem::a_t)
      .def_property_readonly("courant", &Problem::courant)
      .def_property_readonly("cfl_ok", &Problem::cfl_ok)
      .def_property_readonly("tau_max", &Problem::tau_max)
      .def_property_readonly("cell_updates", &Problem::cell_updates)
      .def("__repr__", [](const Problem& p) {
        return "Problem(N=" + std::to_string(p.N) + ", tau=" + std::to_string(p.tau) + ", K=" + std::to_string(p.K) +
               ", L=" + std::to_string(p.L) +
               (p.is_box() ? ", Ly=" + std::to_string(p.edge_y()) + ", Lz=" + std::to_string(p.edge_z()) : "") + ")";
      });

  py::class_<Coeffs>(m, "Coeffs")
      .def_static("from_problem", &Coeffs::from, py::arg("problem"), py::arg("force_box") = false)
      .def_readonly("ihx2", &Coeffs::ihx2)
      .def_readonly("ihy2", &Coeffs::ihy2)
      .def_readonly("ihz2", &Coeffs::ihz2)
      .def_readonly("tau2", &Coeffs::tau2)
      .def_readonly("half_tau2", &Coeffs::half_tau2)
      .def_readonly("lam", &Coeffs::lam)
      .def_readonly("half_lam", &Coeffs::half_lam)
      .def_readonly("ry", &Coeffs::ry)
      .def_readonly("rz", &Coeffs::rz)
      .def_readonly("box", &Coeffs::box)
      .def_readonly("order", &Coeffs::order)
      .def_readonly("time_order", &Coeffs::time_order)
      .def_readonly("lam12", &Coeffs::lam12)
      .def_readonly("lam24", &Coeffs::lam24)
      .def_readonly("lam6", &Coeffs::lam6);

  m.def("sin_table_ext", [](const Problem& p) {
    auto v = sin_table_ext(p);
    return darr(static_cast<py::ssize_t>(v.size()), v.data());
  });
  m.def("time_factor", &time_factor);
  m.def("sponge_tables", [](const Problem& p) {
    const SpongeTables t = sponge_tables(p);
    const py::ssize_t n = static_cast<py::ssize_t>(p.N + 3);
    darr out({static_cast<py::ssize_t>(6), n});
    for (int a = 0; a < 3; ++a) {
      std::memcpy(out.mutable_data(a), t.g[a].data(), static_cast<size_t>(n) * sizeof(double));
      std::memcpy(out.mutable_data(3 + a), t.r[a].data(), static_cast<size_t>(n) * sizeof(double));
    }
    return out;
  }, "the sponge coefficient tables as rows (gx, gy, gz, rx, ry, rz) of N + 3 entries: element [i + 1] = node i");
  m.def("sponge_sigma", &sponge_sigma, py::arg("problem"), py::arg("axis"));
  // elementwise IEEE fused multiply-add (the rounding of stencil.hpp's leapfrog / first_step / err_sq_acc), for the
  // numpy emulators that must reproduce the kernels bit for bit (numpy has no fma)
  m.def("fma_array", [](const darr& a, const darr& b, const darr& c) {
    W3D_REQUIRE(a.size() == b.size() && a.size() == c.size(), "fma_array: sizes differ");
    darr out(a.size());
    double* o = out.mutable_data();
    const double *pa = a.data(), *pb = b.data(), *pc = c.data();
    for (py::ssize_t i = 0; i < a.size(); ++i) o[i] = fma_exact(pa[i], pb[i], pc[i]);
    return out;
  });

  py::class_<Dims>(m, "Dims")
      .def(py::init([](int px, int py_, int pz) { return Dims{px, py_, pz}; }))
      .def_readwrite("px", &Dims::px)
      .def_readwrite("py", &Dims::py)
      .def_readwrite("pz", &Dims::pz)
      .def("size", &Dims::size)
      .def("as_tuple", [](const Dims& d) { return py::make_tuple(d.px, d.py, d.pz); });
  m.def("parse_dims", &parse_dims);
  m.def("block_dims", &block_dims);
  m.def("split_axis", [](i64 N, int p, int c) {
    i64 b, e;
    split_axis(N, p, c, &b, &e);
    return py::make_tuple(b, e);
  });

  py::class_<Box>(m, "Box")
      .def_readonly("x0", &Box::x0)
      .def_readonly("x1", &Box::x1)
      .def_readonly("y0", &Box::y0)
      .def_readonly("y1", &Box::y1)
      .def_readonly("z0", &Box::z0)
      .def_readonly("z1", &Box::z1)
      .def("count", &Box::count);
  m.def("rank_box", &rank_box);
  m.def("neighbor_rank", &neighbor_rank);
  m.def("rank_coords", &rank_coords);

  py::class_<Layout>(m, "Layout")
      .def_readonly("N", &Layout::N)
      .def_readonly("xg", &Layout::xg)
      .def_readonly("yg", &Layout::yg)
      .def_readonly("zg", &Layout::zg)
      .def("zero_off", &Layout::zero_off)
      .def_readonly("nx", &Layout::nx)
      .def_readonly("ny", &Layout::ny)
      .def_readonly("nz", &Layout::nz)
      .def_readonly("gx0", &Layout::gx0)
      .def_readonly("gy0", &Layout::gy0)
      .def_readonly("gz0", &Layout::gz0)
      .def_readonly("zs", &Layout::zs)
      .def_readonly("pitch", &Layout::pitch)
      .def_readonly("plane", &Layout::plane)
      .def_readonly("total", &Layout::total)
      .def_readonly("cx0", &Layout::cx0)
      .def_readonly("cx1", &Layout::cx1)
      .def_readonly("cy0", &Layout::cy0)
      .def_readonly("cy1", &Layout::cy1)
      .def_readonly("cz0", &Layout::cz0)
      .def_readonly("cz1", &Layout::cz1)
      .def("off", [](const Layout& l, i64 x, i64 y, i64 z) { return l.off(x, y, z); });
  m.def("make_layout", &make_layout, py::arg("problem"), py::arg("box"), py::arg("pitch_align") = 16,
        py::arg("xg") = 1, py::arg("yg") = 1, py::arg("zg") = 1);

  py::class_<Face>(m, "Face")
      .def_readonly("axis", &Face::axis)
      .def_readonly("side", &Face::side)
      .def_readonly("peer", &Face::peer)
      .def_readonly("count", &Face::count)
      .def_readonly("contiguous", &Face::contiguous)
      .def_readonly("send_off", &Face::send_off)
      .def_readonly("recv_off", &Face::recv_off)
      .def_readonly("send_layer", &Face::send_layer)
      .def_readonly("recv_layer", &Face::recv_layer)
      .def_readonly("pack_off", &Face::pack_off);
  py::class_<HaloPlan>(m, "HaloPlan")
      .def_readonly("faces", &HaloPlan::faces)
      .def_readonly("packed_doubles", &HaloPlan::packed_doubles);
  m.def("make_halo_plan", &make_halo_plan);

  py::class_<DeepPart>(m, "DeepPart")
      .def_readonly("field", &DeepPart::field)
      .def_readonly("send", &DeepPart::send)
      .def_readonly("recv", &DeepPart::recv)
      .def_readonly("off", &DeepPart::off);
  py::class_<DeepPeer>(m, "DeepPeer")
      .def_readonly("peer", &DeepPeer::peer)
      .def_readonly("dir", &DeepPeer::dir)
      .def_readonly("count", &DeepPeer::count)
      .def_readonly("buf_off", &DeepPeer::buf_off)
      .def_readonly("parts", &DeepPeer::parts);
  py::class_<DeepPlan>(m, "DeepPlan")
      .def_readonly("s", &DeepPlan::s)
      .def_readonly("peers", &DeepPlan::peers)
      .def_readonly("total", &DeepPlan::total);
  m.def("make_deep_plan", &make_deep_plan, py::arg("layout"), py::arg("dims"), py::arg("rank"), py::arg("s"));

  py::class_<LBox>(m, "LBox")
      .def(py::init([](i64 x0, i64 x1, i64 y0, i64 y1, i64 z0, i64 z1) { return LBox{x0, x1, y0, y1, z0, z1}; }))
      .def_readwrite("x0", &LBox::x0)
      .def_readwrite("x1", &LBox::x1)
      .def_readwrite("y0", &LBox::y0)
      .def_readwrite("y1", &LBox::y1)
      .def_readwrite("z0", &LBox::z0)
      .def_readwrite("z1", &LBox::z1)
      .def("empty", &LBox::empty)
      .def("count", &LBox::count)
      .def("as_tuple", [](const LBox& b) { return py::make_tuple(b.x0, b.x1, b.y0, b.y1, b.z0, b.z1); });
  m.def("compute_box", &compute_box);
  m.def("sponge_boxes", &sponge_boxes, py::arg("problem"), py::arg("layout"), py::arg("steps"),
        "disjoint boxes whose union is the slabs d < W + steps - 1 from the damped faces, clipped to the interior");
  m.def("plan_receivers",
        [](const Problem& p, const Dims& d, int rank, const Layout& l, const iarr& nodes) {
          const std::vector<Receiver> v = plan_receivers(p, d, rank, l, receiver_nodes(nodes));
          static_assert(sizeof(Receiver) == 5 * sizeof(i64), "a Receiver is five int64s");
          iarr out({static_cast<py::ssize_t>(v.size()), static_cast<py::ssize_t>(5)});
          if (!v.empty()) std::memcpy(out.mutable_data(), v.data(), v.size() * sizeof(Receiver));
          return out;
        },
        py::arg("problem"), py::arg("dims"), py::arg("rank"), py::arg("layout"), py::arg("nodes"),
        "this rank's receivers of the (R, 3) global node list: int64 rows (slot, x, y, z, off)");
  m.def("plan_sources",
        [](const Problem& p, const Dims& d, int rank, const Layout& l, const iarr& nodes, int radius) {
          const SourcePlan v = plan_sources(p, d, rank, l, receiver_nodes(nodes), radius);
          static_assert(sizeof(Source) == 5 * sizeof(i64), "a Source is five int64s");
          iarr out({static_cast<py::ssize_t>(v.table.size()), static_cast<py::ssize_t>(5)});
          if (!v.table.empty()) std::memcpy(out.mutable_data(), v.table.data(), v.table.size() * sizeof(Source));
          return py::make_tuple(out, v.class_begin);
        },
        py::arg("problem"), py::arg("dims"), py::arg("rank"), py::arg("layout"), py::arg("nodes"), py::arg("radius"),
        "the sources of the (Q, 3) global node list whose L1 ball of `radius` meets this rank's allocation, ordered by "
        "colour class: (int64 rows (slot, x, y, z, off), class_begin)");
  m.def("source_addend", &source_addend, py::arg("problem"), py::arg("w"), "tau^2 w / (hx hy hz)");
  m.def("cpu_source_response",
        [](const Problem& p, const Coeffs& c, const std::array<i64, 3>& node, const darr& a, bool start, int s) {
          W3D_REQUIRE(a.size() >= (start ? 1 : s), "source_response: a holds fewer than s addends");
          darr last({kSourceSide, kSourceSide, kSourceSide}), prev({kSourceSide, kSourceSide, kSourceSide});
          cpu_source_response(p, c, node.data(), a.data(), start, s, last.mutable_data(), prev.mutable_data());
          return py::make_tuple(last, prev);
        },
        py::arg("problem"), py::arg("coeffs"), py::arg("node"), py::arg("a"), py::arg("first_is_start"), py::arg("s"),
        "(r^{n+s}, r^{n+s-1}) on the 11^3 cube around the node: the response of a zero field to the addends a[0..s)");
  m.def(
      "shell_split",
      [](const LBox& full, const std::vector<std::vector<bool>>& nbv) {
        W3D_REQUIRE(nbv.size() == 3 && nbv[0].size() == 2 && nbv[1].size() == 2 && nbv[2].size() == 2,
                    "shell_split: neighbours as [[x lo, x hi], [y lo, y hi], [z lo, z hi]]");
        bool nb[3][2];
        for (int a = 0; a < 3; ++a)
          for (int s = 0; s < 2; ++s) nb[a][s] = nbv[static_cast<size_t>(a)][static_cast<size_t>(s)];
        std::vector<LBox> shell;
        LBox interior;
        shell_split(full, nb, shell, interior);
        return py::make_tuple(shell, interior);
      },
      "(shell boxes, interior box) of a compute box with neighbours nb[axis][side] (the runtime's own split)");
  m.def(
      "deep_split",
      [](const LBox& full, const std::vector<std::vector<bool>>& nbv, i64 w, i64 tile) {
        W3D_REQUIRE(nbv.size() == 3 && nbv[0].size() == 2 && nbv[1].size() == 2 && nbv[2].size() == 2,
                    "deep_split: neighbours as [[x lo, x hi], [y lo, y hi], [z lo, z hi]]");
        bool nb[3][2];
        for (int a = 0; a < 3; ++a)
          for (int s = 0; s < 2; ++s) nb[a][s] = nbv[static_cast<size_t>(a)][static_cast<size_t>(s)];
        std::vector<LBox> shell;
        LBox interior;
        deep_split(full, nb, w, tile, shell, interior);
        return py::make_tuple(shell, interior);
      },
      py::arg("full"), py::arg("nb"), py::arg("w"), py::arg("tile") = 32,
      "(shell boxes, interior box) of a deep-tb unit whose exchange of depth w overlaps the pass (GpuSolver::tb_split)");

  // ---------------- CPU kernels ----------------
  m.def("cpu_set_threads", &cpu_set_threads);
  m.def("cpu_max_threads", &cpu_max_threads);
  m.def("cpu_init_first", [](const Layout& l, const Coeffs& c, const darr& s, darr u0, darr u1) {
    const double* sp = ro_ptr(s, l.N + 3, "s") + 1;
    double* a = mut_ptr(u0, l.total, "u0");
    double* b = mut_ptr(u1, l.total, "u1");
    py::gil_scoped_release nogil;
    cpu_init_first(l, c, sp, a, b);
  });
  m.def("initial_layout", &initial_layout, py::arg("problem"), py::arg("layout"),
        "the layout set_initial slices phi / psi into: the solve layout's box with one ghost layer more per axis");
  m.def("initial_to_local", [](const Layout& src, const darr& g) {
    const i64 n = src.N + 1;
    const double* gp = ro_ptr(g, n * n * n, "global");
    darr out(static_cast<py::ssize_t>(src.total));
    initial_to_local(src, gp, out.mutable_data());
    return out;
  }, py::arg("layout"), py::arg("field"), "a GLOBAL (N+1)^3 field sliced into `layout`, the six global faces zeroed");
  m.def("speed_to_local", [](const Problem& p, const Layout& l, const darr& c) {
    const i64 n = p.N + 1;
    const double* cp = ro_ptr(c, n * n * n, "c");
    darr lamf(static_cast<py::ssize_t>(l.total)), c2(static_cast<py::ssize_t>(l.total));
    const SpeedRange r = speed_to_local(p, l, cp, lamf.mutable_data(), c2.mutable_data());
    return py::make_tuple(lamf, c2, r.cmin, r.cmax);
  }, py::arg("problem"), py::arg("layout"), py::arg("c"),
        "a GLOBAL (N+1)^3 speed field as (lamf = lam c^2, c2 = c^2) in `layout` (zeros outside the global interior) and "
        "the interior minimum and maximum of c; refuses non-finite or non-positive interior values");
  m.def("eigenmode_local", [](const Problem& p, const Layout& src) {
    const std::vector<double> v = eigenmode_local(p, src);
    return darr(static_cast<py::ssize_t>(v.size()), v.data());
  }, py::arg("problem"), py::arg("layout"));
  m.def("cpu_first_step_field",
        [](const Layout& l, const Layout& src, const Coeffs& c, double tau, const darr& phi, py::object psi, darr u0,
           darr u1, py::object lamf) {
          darr lamf_a;
          const double* lp = nullptr;
          if (!lamf.is_none()) {
            lamf_a = lamf.cast<darr>();
            lp = ro_ptr(lamf_a, l.total, "lamf");
          }
          const double* fp = ro_ptr(phi, src.total, "phi");
          const double* sp = nullptr;
          darr psi_a;
          if (!psi.is_none()) {
            psi_a = psi.cast<darr>();
            sp = ro_ptr(psi_a, src.total, "psi");
          }
          double* a = mut_ptr(u0, l.total, "u0");
          double* b = mut_ptr(u1, l.total, "u1");
          py::gil_scoped_release nogil;
          cpu_first_step_field(l, src, c, tau, fp, sp, a, b, lp);
        },
        py::arg("layout"), py::arg("src"), py::arg("coeffs"), py::arg("tau"), py::arg("phi"), py::arg("psi"),
        py::arg("u0"), py::arg("u1"), py::arg("lamf") = py::none());
  m.def("cpu_energy",
        [](const Problem& p, const Layout& l, const darr& a, const darr& b, py::object c2) {
          darr c2_a;  // c2: speed_to_local's c^2 array in `layout` (the mass weight 1/c^2 of the kinetic term)
          const double* c2p = nullptr;
          if (!c2.is_none()) {
            c2_a = c2.cast<darr>();
            c2p = ro_ptr(c2_a, l.total, "c2");
          }
          const EnergySums e =
              cpu_energy(l, Coeffs::from(p), p.tau, ro_ptr(a, l.total, "a"), ro_ptr(b, l.total, "b"), c2p);
          const double half_v = 0.5 * ((p.hx() * p.hy()) * p.hz());
          py::dict d;
          d["E"] = energy_value(p, e.kin, e.pot);
          d["kin"] = e.kin;
          d["pot"] = e.pot;
          d["abs_terms"] = half_v * e.abs;
          d["depth"] = e.depth;
          return d;
        },
        py::arg("problem"), py::arg("layout"), py::arg("a"), py::arg("b"), py::arg("c2") = py::none(),
        "discrete energy of a = u^n, b = u^{n+1} (local arrays in `layout`): E, its kinetic / potential sums, "
        "abs_terms = V/2 * sum |terms| (the scale of the summation error) and the summation depth");
  m.def("energy_value", &energy_value);
  m.def(
      "cpu_leapfrog",
      [](const Layout& l, const Coeffs& c, const darr& cur, darr old, const LBox& box, const darr& s, double ct,
         bool check, py::object sponge, py::object lamf) -> py::object {
        const double* cp = ro_ptr(cur, l.total, "cur");
        darr lamf_a;  // lamf: a speed field's lam c^2 array in `layout`
        const double* lp = nullptr;
        if (!lamf.is_none()) {
          lamf_a = lamf.cast<darr>();
          lp = ro_ptr(lamf_a, l.total, "lamf");
        }
        double* op = mut_ptr(old, l.total, "old");
        const double* sp = ro_ptr(s, l.N + 3, "s") + 1;
        SpongeTables tab;  // sponge: a Problem whose sponge_tables give the damped step
        SpongeView view;
        if (!sponge.is_none()) {
          tab = sponge_tables(sponge.cast<Problem>());
          view = tab.view();
        }
        ErrAcc acc;
        {
          py::gil_scoped_release nogil;
          cpu_leapfrog(l, c, cp, op, box, sp, ct, check ? &acc : nullptr, sponge.is_none() ? nullptr : &view, lp);
        }
        if (!check) return py::none();
        return py::make_tuple(acc.max, acc.sum);
      },
      py::arg("layout"), py::arg("coeffs"), py::arg("cur"), py::arg("old"), py::arg("box"), py::arg("s"),
      py::arg("ct") = 0.0, py::arg("check") = false, py::arg("sponge") = py::none(), py::arg("lamf") = py::none());
  m.def("cpu_lap4",
        [](const Layout& l, const Coeffs& c, const darr& u, darr v, const LBox& box) {
          const double* up = ro_ptr(u, l.total, "u");
          double* vp = mut_ptr(v, l.total, "v");
          py::gil_scoped_release nogil;
          cpu_lap4(l, c, up, vp, box);
        },
        py::arg("layout"), py::arg("coeffs"), py::arg("u"), py::arg("v"), py::arg("box"),
        "time order 4: v = lam s(u) on the nodes of `box`, nothing else of v is written");
  m.def("cpu_leapfrog44",
        [](const Layout& l, const Coeffs& c, const darr& cur, const darr& v, darr old, const LBox& box, const darr& s,
           double ct, bool check) -> py::object {
          const double* cp = ro_ptr(cur, l.total, "cur");
          const double* vp = ro_ptr(v, l.total, "v");
          double* op = mut_ptr(old, l.total, "old");
          const double* sp = ro_ptr(s, l.N + 3, "s") + 1;
          ErrAcc acc;
          {
            py::gil_scoped_release nogil;
            cpu_leapfrog44(l, c, cp, vp, op, box, sp, ct, check ? &acc : nullptr);
          }
          if (!check) return py::none();
          return py::make_tuple(acc.max, acc.sum);
        },
        py::arg("layout"), py::arg("coeffs"), py::arg("cur"), py::arg("v"), py::arg("old"), py::arg("box"), py::arg("s"),
        py::arg("ct") = 0.0, py::arg("check") = false,
        "time order 4: u^{n+1} = leapfrog_t4(u^n, u^{n-1}, v, s(v), lam12) in place over `old`");
  m.def("cpu_first_step_t4",
        [](const Layout& l, const Layout& src, const Coeffs& c, double tau, const darr& phi, py::object psi, darr v,
           darr u0, darr u1) {
          const double* fp = ro_ptr(phi, src.total, "phi");
          const double* sp = nullptr;
          darr psi_a;
          if (!psi.is_none()) {
            psi_a = psi.cast<darr>();
            sp = ro_ptr(psi_a, src.total, "psi");
          }
          double* vp = mut_ptr(v, l.total, "v");
          double* a = mut_ptr(u0, l.total, "u0");
          double* b = mut_ptr(u1, l.total, "u1");
          py::gil_scoped_release nogil;
          cpu_first_step_t4(l, src, c, tau, fp, sp, vp, a, b);
        },
        py::arg("layout"), py::arg("src"), py::arg("coeffs"), py::arg("tau"), py::arg("phi"), py::arg("psi"), py::arg("v"),
        py::arg("u0"), py::arg("u1"));
  m.def("cpu_error", [](const Layout& l, const darr& u, const LBox& box, const darr& s, double ct) {
    ErrAcc acc;
    cpu_error(l, ro_ptr(u, l.total, "u"), box, ro_ptr(s, l.N + 3, "s") + 1, ct, &acc);
    return py::make_tuple(acc.max, acc.sum);
  });
  m.def("cpu_pack_face", [](const Layout& l, const Face& f, const darr& u, darr buf) {
    cpu_pack_face(l, f, ro_ptr(u, l.total, "u"), mut_ptr(buf, f.count, "buf"));
  });
  m.def("cpu_unpack_face", [](const Layout& l, const Face& f, const darr& buf, darr u) {
    cpu_unpack_face(l, f, ro_ptr(buf, f.count, "buf"), mut_ptr(u, l.total, "u"));
  });

  py::class_<CpuSolver>(m, "CpuSolver")
      .def(py::init<const Problem&, int, int>(), py::arg("problem"), py::arg("check_every") = 2,
           py::arg("threads") = 0)
      .def("run",
           [](CpuSolver& s) {
             CpuResult r;
             {
               py::gil_scoped_release nogil;
               r = s.run();
             }
             py::dict d;
             d["steps"] = r.steps;
             d["max_err"] = r.max_err;
             d["rms_err"] = r.rms_err;
             d["solve_s"] = r.solve_s;
             d["init_s"] = r.init_s;
             d["compute_s"] = r.compute_s;
             d["finite"] = r.finite;
             return d;
           })
      .def("field",
           [](const CpuSolver& s, int which) {
             const auto& v = s.field(which);
             return darr(static_cast<py::ssize_t>(v.size()), v.data());
           })
      .def_property_readonly("layout", &CpuSolver::layout)
      .def("check_steps", &CpuSolver::check_steps)
      .def("set_state", [](CpuSolver& s, const darr& prev, const darr& cur, int n0) {
        const i64 n = s.layout().N + 1;
        s.set_state(ro_ptr(prev, n * n * n, "prev"), ro_ptr(cur, n * n * n, "cur"), n0);
      }, py::arg("prev"), py::arg("cur"), py::arg("step"))
      .def("set_initial", [](CpuSolver& s, const darr& phi, py::object psi) {
        const i64 n = s.layout().N + 1;
        darr psi_a;
        if (!psi.is_none()) psi_a = psi.cast<darr>();
        s.set_initial(ro_ptr(phi, n * n * n, "phi"), psi.is_none() ? nullptr : ro_ptr(psi_a, n * n * n, "psi"));
      }, py::arg("phi"), py::arg("psi") = py::none())
      .def("set_speed", [](CpuSolver& s, py::object c, bool force) {
        if (c.is_none()) return s.set_speed(nullptr);
        const i64 n = s.layout().N + 1;
        const darr c_a = c.cast<darr>();
        s.set_speed(ro_ptr(c_a, n * n * n, "c"), force);
      }, py::arg("c"), py::arg("force") = false, "solve u_tt = c(x)^2 Lap u with this global (N+1)^3 field (None clears it)")
      .def_property_readonly("speed", &CpuSolver::speed)
      .def_property_readonly("speed_range", [](const CpuSolver& s) {
        return py::make_tuple(s.speed_range().cmin, s.speed_range().cmax);
      })
      .def("set_receivers", [](CpuSolver& s, const iarr& nodes) {
        int R = 0;
        const i64* p = receiver_ptr(nodes, &R);
        s.set_receivers(p, R);
      }, py::arg("nodes"), "record u^n at these (R, 3) global nodes in every following run()")
      .def("traces", [](const CpuSolver& s) {
        const i64 R = s.receivers();
        W3D_REQUIRE(R > 0 && !s.traces().empty(), "traces: no receivers are set, or no solve has run since");
        return darr({static_cast<py::ssize_t>(s.traces().size() / static_cast<size_t>(R)), static_cast<py::ssize_t>(R)},
                    s.traces().data());
      }, "the last run()'s (K+1, R) values, row n = u^n")
      .def("set_sources", [](CpuSolver& s, const iarr& nodes, const darr& w) {
        int Q = 0;
        const double* wp = source_w(s.problem(), nodes, w, &Q);
        s.set_sources(nodes.data(), Q, wp);
      }, py::arg("nodes"), py::arg("w"), "point sources at these (Q, 3) global nodes with the (K, Q) samples w")
      .def_property_readonly("sources", &CpuSolver::sources)
      .def("energy", &CpuSolver::energy, py::arg("which") = 0)
      .def("energy_sums", [](const CpuSolver& s, int which) {
             const EnergySums e = s.energy_sums(which);
             py::dict d;
             d["kin"] = e.kin;
             d["pot"] = e.pot;
             d["abs"] = e.abs;
             d["depth"] = e.depth;
             return d;
           }, py::arg("which") = 0, "the sums behind energy(which): kin, pot, abs (the summation-error scale), depth");

  // ---------------- GPU ----------------
  m.def("gpu_device_count", []() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
      (void)hipGetLastError();
      return 0;
    }
    return n;
  });
  m.def("gpu_set_device", [](int d) { W3D_HIP(hipSetDevice(d)); });
  // versions of the HIP runtime and RCCL this process actually resolved (torch may have loaded its bundled copies)
  m.def("runtime_versions", []() {
    int hv = 0, dv = 0, nv = 0;
    (void)hipRuntimeGetVersion(&hv);
    (void)hipDriverGetVersion(&dv);
    nv = rccl_version();
    py::dict d;
    d["hip_runtime"] = hv;
    d["hip_driver"] = dv;
    d["rccl"] = nv;
    d["multistream_capture_safe"] = multistream_capture_safe();
    return d;
  });
  m.def("gpu_synchronize", []() { W3D_HIP(hipDeviceSynchronize()); });
  m.def("gpu_arch", []() {
    int d = 0;
    W3D_HIP(hipGetDevice(&d));
    hipDeviceProp_t p;
    W3D_HIP(hipGetDeviceProperties(&p, d));
    return std::string(p.gcnArchName);
  });

  py::class_<LeapfrogTiling>(m, "LeapfrogTiling")
      .def(py::init<>())
      .def_readwrite("variant", &LeapfrogTiling::variant)
      .def_readwrite("rows", &LeapfrogTiling::rows)
      .def_readwrite("ty", &LeapfrogTiling::ty)
      .def_readwrite("target_blocks", &LeapfrogTiling::target_blocks)
      .def_readwrite("xcd_remap", &LeapfrogTiling::xcd_remap)
      .def_readwrite("nt_store", &LeapfrogTiling::nt_store);

  m.def("gpu_init_first", [](const Layout& l, const Coeffs& c, std::uintptr_t s, std::uintptr_t u0, std::uintptr_t u1,
                             std::uintptr_t stream) {
    launch_init_first(l, c, dptr<const double>(s) + 1, dptr<double>(u0), dptr<double>(u1), sptr(stream));
  });
  m.def("gpu_first_step_field",
        [](const Layout& l, const Layout& src, const Coeffs& c, double tau, std::uintptr_t phi, std::uintptr_t psi,
           std::uintptr_t u0, std::uintptr_t u1, std::uintptr_t stream, std::uintptr_t lamf) {
          launch_first_step_field(l, src, c, tau, dptr<const double>(phi), dptr<const double>(psi), dptr<double>(u0),
                                  dptr<double>(u1), sptr(stream), dptr<const double>(lamf));
        },
        py::arg("layout"), py::arg("src"), py::arg("coeffs"), py::arg("tau"), py::arg("phi"), py::arg("psi"),
        py::arg("u0"), py::arg("u1"), py::arg("stream"), py::arg("lamf") = 0,
        "k_first_step_field (psi = 0: no psi term; lamf: a speed field's device array in `layout`)");
  // receivers: the table is `count` rows of plan_receivers' array in device memory (a Receiver is its five int64s)
  m.def("gpu_record_cone",
        [](const Layout& l, const Coeffs& c, std::uintptr_t prev, std::uintptr_t cur, int n, int steps,
           std::uintptr_t table, int count, std::uintptr_t trace, i64 rtotal, std::uintptr_t stream) {
          launch_record_cone(l, c, dptr<const double>(prev), dptr<const double>(cur), n, steps,
                             dptr<const Receiver>(table), count, dptr<double>(trace), rtotal, sptr(stream));
        },
        py::arg("layout"), py::arg("coeffs"), py::arg("prev"), py::arg("cur"), py::arg("n"), py::arg("steps"),
        py::arg("table"), py::arg("count"), py::arg("trace"), py::arg("rtotal"), py::arg("stream"),
        "k_record_cone: rows n+1 .. n+steps of trace from the pass inputs prev = u^{n-1}, cur = u^n");
  m.def("gpu_record_gather",
        [](std::uintptr_t field, int n, std::uintptr_t table, int count, std::uintptr_t trace, i64 rtotal,
           std::uintptr_t stream) {
          launch_record_gather(dptr<const double>(field), n, dptr<const Receiver>(table), count, dptr<double>(trace),
                               rtotal, sptr(stream));
        },
        py::arg("field"), py::arg("n"), py::arg("table"), py::arg("count"), py::arg("trace"), py::arg("rtotal"),
        py::arg("stream"), "k_record_gather: row n of trace from a stored level");
  // sources: the table is plan_sources' array in device memory (a Source is its five int64s)
  m.def("gpu_source_cone",
        [](const Layout& l, const Coeffs& c, std::uintptr_t out_prev, std::uintptr_t out_last, int n, int steps, bool start,
           std::uintptr_t table, const std::vector<int>& class_begin, std::uintptr_t a, i64 Q, std::uintptr_t rtable,
           int rcount, std::uintptr_t trace, i64 rtotal, std::uintptr_t stream) {
          W3D_REQUIRE(!class_begin.empty(), "source_cone: class_begin holds classes + 1 entries");
          launch_source_cone(l, c, dptr<double>(out_prev), dptr<double>(out_last), n, steps, start,
                             dptr<const Source>(table), class_begin.data(), static_cast<int>(class_begin.size()) - 1,
                             dptr<const double>(a), Q, dptr<const Receiver>(rtable), rcount, dptr<double>(trace), rtotal,
                             sptr(stream));
        },
        py::arg("layout"), py::arg("coeffs"), py::arg("out_prev"), py::arg("out_last"), py::arg("n"), py::arg("steps"),
        py::arg("start"), py::arg("table"), py::arg("class_begin"), py::arg("a"), py::arg("Q"), py::arg("rtable"),
        py::arg("rcount"), py::arg("trace"), py::arg("rtotal"), py::arg("stream"),
        "k_source_cone: adds the response to the forcing of a pass n -> n + steps to its outputs (and trace rows)");
  m.def("gpu_energy_depth", &energy_depth, "depth D of k_energy's reduction tree for this layout");
  m.def("gpu_energy_partials", &energy_partials);
  m.def("gpu_energy",
        [](const Layout& l, const Coeffs& c, double tau, std::uintptr_t a, std::uintptr_t b, std::uintptr_t partials,
           std::uintptr_t out, std::uintptr_t stream) {
          launch_energy(l, c, tau, dptr<const double>(a), dptr<const double>(b), dptr<Partial>(partials), sptr(stream));
          launch_energy_reduce(dptr<const Partial>(partials), energy_partials(l), dptr<Partial>(out), sptr(stream));
        },
        py::arg("layout"), py::arg("coeffs"), py::arg("tau"), py::arg("a"), py::arg("b"), py::arg("partials"),
        py::arg("out"), py::arg("stream"),
        "k_energy of a = u^n, b = u^{n+1} into gpu_energy_partials(layout) partials, then k_energy_reduce of them "
        "into out[0] = (kinetic sum, potential sum)");
  m.def("gpu_energy_reduce",
        [](std::uintptr_t partials, int n, std::uintptr_t out, std::uintptr_t stream) {
          launch_energy_reduce(dptr<const Partial>(partials), n, dptr<Partial>(out), sptr(stream));
        },
        py::arg("partials"), py::arg("n"), py::arg("out"), py::arg("stream"), "k_energy_reduce alone");
  m.def("gpu_init_two_partials", &init_two_partials);
  m.def("gpu_init_two", [](const Layout& l, const Coeffs& c, std::uintptr_t s, std::uintptr_t u1, std::uintptr_t u2,
                           double ct2, std::uintptr_t partials, std::uintptr_t stream) {
    launch_init_two(l, c, dptr<const double>(s) + 1, dptr<double>(u1), dptr<double>(u2), ct2,
                    dptr<Partial>(partials), sptr(stream));
  });
  m.def("gpu_leapfrog_blocks", [](const Layout& l, const std::vector<LBox>& boxes, const LeapfrogTiling& t) {
    return leapfrog_blocks(l, boxes.data(), static_cast<int>(boxes.size()), t);
  });
  m.def("gpu_leapfrog",
        [](const Layout& l, const Coeffs& c, std::uintptr_t cur, std::uintptr_t old, const std::vector<LBox>& boxes,
           std::uintptr_t s, double ct, std::uintptr_t partials, const LeapfrogTiling& t, std::uintptr_t stream,
           std::uintptr_t sponge, std::uintptr_t lamf) {
          // sponge: sponge_tables' (6, N + 3) array in device memory (0: the undamped step); lamf: a speed field's
          // device array in `layout` (0: constant speed)
          SpongeView view;
          if (sponge) {
            const i64 n = l.N + 3;
            const double* g = dptr<const double>(sponge);
            view = SpongeView{g + 1, g + n + 1, g + 2 * n + 1, g + 3 * n + 1, g + 4 * n + 1, g + 5 * n + 1};
          }
          launch_leapfrog(l, c, dptr<const double>(cur), dptr<double>(old), boxes.data(),
                          static_cast<int>(boxes.size()), dptr<const double>(s) + 1, ct, dptr<Partial>(partials), t,
                          sptr(stream), sponge ? &view : nullptr, dptr<const double>(lamf));
        },
        py::arg("layout"), py::arg("coeffs"), py::arg("cur"), py::arg("old"), py::arg("boxes"), py::arg("s"),
        py::arg("ct"), py::arg("partials"), py::arg("tiling"), py::arg("stream"), py::arg("sponge") = 0,
        py::arg("lamf") = 0);
  m.def("gpu_leapfrog4_ty", &leapfrog4_ty, py::arg("tiling"), "tile rows of k_leapfrog4 for this tiling (8 or 16)");
  m.def("gpu_leapfrog4_blocks",
        [](const Layout& l, const std::vector<LBox>& boxes, const LeapfrogTiling& t, int min_chunk) {
          return leapfrog4_blocks(l, boxes.data(), static_cast<int>(boxes.size()), t, min_chunk);
        },
        py::arg("layout"), py::arg("boxes"), py::arg("tiling"), py::arg("min_chunk") = 16);
  m.def("gpu_leapfrog4",
        [](const Layout& l, const Coeffs& c, std::uintptr_t cur, std::uintptr_t old, const std::vector<LBox>& boxes,
           std::uintptr_t s, double ct, std::uintptr_t partials, const LeapfrogTiling& t, std::uintptr_t stream,
           int min_chunk) {
          launch_leapfrog4(l, c, dptr<const double>(cur), dptr<double>(old), boxes.data(), static_cast<int>(boxes.size()),
                           dptr<const double>(s) + 1, ct, dptr<Partial>(partials), t, sptr(stream), min_chunk);
        },
        py::arg("layout"), py::arg("coeffs"), py::arg("cur"), py::arg("old"), py::arg("boxes"), py::arg("s"),
        py::arg("ct"), py::arg("partials"), py::arg("tiling"), py::arg("stream"), py::arg("min_chunk") = 16,
        "k_leapfrog4: the fourth-order single step (coeffs of an order = 4 problem)");
  m.def("gpu_leapfrog44_blocks",
        [](const Layout& l, const std::vector<LBox>& boxes, const LeapfrogTiling& t, int min_chunk) {
          return leapfrog44_blocks(l, boxes.data(), static_cast<int>(boxes.size()), t, min_chunk);
        },
        py::arg("layout"), py::arg("boxes"), py::arg("tiling"), py::arg("min_chunk") = 16);
  m.def("gpu_lap4",
        [](const Layout& l, const Coeffs& c, std::uintptr_t u, std::uintptr_t v, const std::vector<LBox>& boxes,
           const LeapfrogTiling& t, std::uintptr_t stream, int min_chunk) {
          launch_lap4(l, c, dptr<const double>(u), dptr<double>(v), boxes.data(), static_cast<int>(boxes.size()), t,
                      sptr(stream), min_chunk);
        },
        py::arg("layout"), py::arg("coeffs"), py::arg("u"), py::arg("v"), py::arg("boxes"), py::arg("tiling"),
        py::arg("stream"), py::arg("min_chunk") = 16, "k_lap4: v = lam s(u) (coeffs of a time_order = 4 problem)");
  m.def("gpu_leapfrog44",
        [](const Layout& l, const Coeffs& c, std::uintptr_t cur, std::uintptr_t v, std::uintptr_t old,
           const std::vector<LBox>& boxes, std::uintptr_t s, double ct, std::uintptr_t partials, const LeapfrogTiling& t,
           std::uintptr_t stream, int min_chunk) {
          launch_leapfrog44(l, c, dptr<const double>(cur), dptr<const double>(v), dptr<double>(old), boxes.data(),
                            static_cast<int>(boxes.size()), dptr<const double>(s) + 1, ct, dptr<Partial>(partials), t,
                            sptr(stream), min_chunk);
        },
        py::arg("layout"), py::arg("coeffs"), py::arg("cur"), py::arg("v"), py::arg("old"), py::arg("boxes"), py::arg("s"),
        py::arg("ct"), py::arg("partials"), py::arg("tiling"), py::arg("stream"), py::arg("min_chunk") = 16,
        "k_leapfrog44: the update of a time_order = 4 step from v = gpu_lap4's of `cur`");
  m.def("gpu_first_step_t4",
        [](const Layout& l, const Layout& src, const Coeffs& c, double tau, std::uintptr_t phi, std::uintptr_t psi,
           std::uintptr_t v, std::uintptr_t u0, std::uintptr_t u1, const LeapfrogTiling& t, std::uintptr_t stream) {
          launch_first_step_t4(l, src, c, tau, dptr<const double>(phi), dptr<const double>(psi), dptr<double>(v),
                               dptr<double>(u0), dptr<double>(u1), t, sptr(stream));
        },
        py::arg("layout"), py::arg("src"), py::arg("coeffs"), py::arg("tau"), py::arg("phi"), py::arg("psi"), py::arg("v"),
        py::arg("u0"), py::arg("u1"), py::arg("tiling"), py::arg("stream"),
        "the first step of a time_order = 4 solve (psi = 0: no psi term)");
  m.def("gpu_leapfrog_speed_supported", &leapfrog_speed_supported, py::arg("tiling"), py::arg("sponge"));
  m.def("gpu_sponge_box",
        [](const Layout& l, const Coeffs& c, std::uintptr_t tables, std::uintptr_t prev, std::uintptr_t cur,
           std::uintptr_t out1, std::uintptr_t out2, const LBox& box, int steps, std::uintptr_t stream) {
          const i64 n = l.N + 3;
          const double* g = dptr<const double>(tables);
          W3D_REQUIRE(g != nullptr, "sponge_box: no tables");
          const SpongeView view{g + 1, g + n + 1, g + 2 * n + 1, g + 3 * n + 1, g + 4 * n + 1, g + 5 * n + 1};
          launch_sponge_box(l, c, view, dptr<const double>(prev), dptr<const double>(cur), dptr<double>(out1),
                            dptr<double>(out2), box, steps, sptr(stream));
        },
        py::arg("layout"), py::arg("coeffs"), py::arg("tables"), py::arg("prev"), py::arg("cur"), py::arg("out1"),
        py::arg("out2"), py::arg("box"), py::arg("steps"), py::arg("stream"),
        "k_sponge_box: out2 = u^{n+steps}, out1 = u^{n+steps-1} on `box` by `steps` damped steps from prev, cur; "
        "tables: sponge_tables' (6, N + 3) array in device memory");
  py::class_<Leapfrog2Tiling>(m, "Leapfrog2Tiling")
      .def(py::init<>())
      .def_readwrite("rows", &Leapfrog2Tiling::rows)
      .def_readwrite("target_waves", &Leapfrog2Tiling::target_waves)
      .def_readwrite("occupancy", &Leapfrog2Tiling::occupancy)
      .def_readwrite("xcd_remap", &Leapfrog2Tiling::xcd_remap)
      .def_readwrite("nt_store", &Leapfrog2Tiling::nt_store);
  m.def("gpu_leapfrog2_partials", &leapfrog2_partials);
  m.def("gpu_leapfrog2",
        [](const Layout& l, const Coeffs& c, std::uintptr_t prev, std::uintptr_t cur, std::uintptr_t out1,
           std::uintptr_t out2, const LBox& box, std::uintptr_t s, double ct2, std::uintptr_t partials,
           const Leapfrog2Tiling& t, std::uintptr_t stream, i64 sx0, i64 sx1, std::uintptr_t lamf) {
          launch_leapfrog2(l, c, dptr<const double>(prev), dptr<const double>(cur), dptr<double>(out1),
                           dptr<double>(out2), box, dptr<const double>(s) + 1, ct2, dptr<Partial>(partials), t,
                           sptr(stream), sx0, sx1, dptr<const double>(lamf));
        },
        py::arg("layout"), py::arg("coeffs"), py::arg("prev"), py::arg("cur"), py::arg("out1"), py::arg("out2"),
        py::arg("box"), py::arg("s"), py::arg("ct2"), py::arg("partials"), py::arg("tiling"), py::arg("stream"),
        py::arg("sx0") = 1, py::arg("sx1") = 0, py::arg("lamf") = 0);
  py::class_<LeapfrogTbTiling>(m, "LeapfrogTbTiling")
      .def(py::init<>())
      .def_readwrite("stages", &LeapfrogTbTiling::stages)
      .def_readwrite("threads", &LeapfrogTbTiling::threads)
      .def_readwrite("init_threads", &LeapfrogTbTiling::init_threads)
      .def_readwrite("xcd_remap", &LeapfrogTbTiling::xcd_remap)
      .def_readwrite("xcd_blocks", &LeapfrogTbTiling::xcd_blocks)
      .def_readwrite("target_blocks", &LeapfrogTbTiling::target_blocks)
      .def_readwrite("min_chunk", &LeapfrogTbTiling::min_chunk)
      .def_readwrite("p2", &LeapfrogTbTiling::p2)
      .def_readwrite("ghost_x1", &LeapfrogTbTiling::ghost_x1);
  m.def("capture_guard_selftest", &wave3d::capture::selftest, py::arg("mode"),
        "the probe topologies through the stream-capture guard (0: production, 2: the round-4 sibling wait)");
  m.def("leapfrog_p2_table", [](int stages) {
        std::vector<long> geo;
        std::vector<int> t = wave3d::leapfrog_p2_table(stages, &geo);
        return py::make_tuple(t, geo);
      }, py::arg("stages"), "the pair-tiled pass's compile-time thread table and geometry (host copy, no GPU)");
  m.def("gpu_leapfrog_p2_supported", &leapfrog_p2_supported);
  m.def("gpu_leapfrog_tb_lds_bytes", &leapfrog_tb_lds_bytes);
  m.def("gpu_leapfrog_tb_partials", &leapfrog_tb_partials);
  // pack_zf: the fused z-face pack (TbPack, k_leapfrog_tb only): device pointers of the four staging parts
  // [low z u^{n+S}, low z u^{n+S−1}, high z u^{n+S}, high z u^{n+S−1}] (0: no such part), pack_w: the band width
  m.def("gpu_leapfrog_tb",
        [](const Layout& l, const Coeffs& c, std::uintptr_t prev, std::uintptr_t cur, std::uintptr_t out1,
           std::uintptr_t out2, const LBox& box, std::uintptr_t s, const std::vector<double>& ct, int check_mask,
           std::uintptr_t partials, const LeapfrogTbTiling& t, std::uintptr_t stream, const LBox& real,
           bool analytic_start, int level_stride, int grid_blocks, const std::vector<std::uintptr_t>& pack_zf,
           int pack_w, std::uintptr_t lamf) {
          PassArgs a = py_pass_args(prev, cur, out1, out2, s, ct, check_mask, partials, t, real, analytic_start,
                                    level_stride, grid_blocks, lamf);
          TbPack pk;
          TbPack* dev = nullptr;
          if (!pack_zf.empty()) {
            W3D_REQUIRE(pack_zf.size() == 4, "gpu_leapfrog_tb: pack_zf takes four pointers");
            for (int side = 0; side < 2; ++side)
              for (int f = 0; f < 2; ++f) pk.zf[side][f] = dptr<double>(pack_zf[static_cast<size_t>(2 * side + f)]);
            pk.w = pack_w;
            pk.ny = static_cast<int>(l.ny);
            pk.nz = static_cast<int>(l.nz);
            W3D_HIP(hipMalloc(&dev, sizeof(TbPack)));
            a.pack = &pk;
            a.pack_dev = dev;
          }
          try {
            if (dev) W3D_HIP(hipMemcpy(dev, &pk, sizeof(TbPack), hipMemcpyHostToDevice));
            launch_leapfrog_tb(l, c, box, a, sptr(stream));
            if (dev) W3D_HIP(hipStreamSynchronize(sptr(stream)));  // (the kernel reads the parameters from `dev`)
          } catch (...) {
            (void)hipFree(dev);
            throw;
          }
          if (dev) W3D_HIP(hipFree(dev));
        },
        py::arg("layout"), py::arg("coeffs"), py::arg("prev"), py::arg("cur"), py::arg("out1"), py::arg("out2"),
        py::arg("box"), py::arg("s"), py::arg("ct"), py::arg("check_mask"), py::arg("partials"), py::arg("tiling"),
        py::arg("stream"), py::arg("real") = tb_default_real(), py::arg("analytic_start") = false,
        py::arg("level_stride") = 0, py::arg("grid_blocks") = 0, py::arg("pack_zf") = std::vector<std::uintptr_t>{},
        py::arg("pack_w") = 0, py::arg("lamf") = 0);
  m.def("gpu_leapfrog_p2_partials", &leapfrog_p2_partials);
  m.def("gpu_leapfrog_p2_boxes",
        [](const Layout& l, const Coeffs& c, std::uintptr_t prev, std::uintptr_t cur, std::uintptr_t out1,
           std::uintptr_t out2, const std::vector<LBox>& boxes, std::uintptr_t s, const std::vector<double>& ct,
           int check_mask, std::uintptr_t partials, const LeapfrogTbTiling& t, std::uintptr_t stream, const LBox& real,
           bool analytic_start, int level_stride, int grid_blocks, std::uintptr_t lamf) {
          PassArgs a = py_pass_args(prev, cur, out1, out2, s, ct, check_mask, partials, t, real, analytic_start,
                                    level_stride, grid_blocks, lamf);
          launch_leapfrog_p2_boxes(l, c, boxes.data(), static_cast<int>(boxes.size()), a, sptr(stream));
        },
        py::arg("layout"), py::arg("coeffs"), py::arg("prev"), py::arg("cur"), py::arg("out1"), py::arg("out2"),
        py::arg("boxes"), py::arg("s"), py::arg("ct"), py::arg("check_mask"), py::arg("partials"), py::arg("tiling"),
        py::arg("stream"), py::arg("real") = tb_default_real(), py::arg("analytic_start") = false,
        py::arg("level_stride") = 0, py::arg("grid_blocks") = 0, py::arg("lamf") = 0,
        "one pair-tiled launch over up to 6 boxes (the overlapped schedules' shells); their partials share one slot. "
        "lamf: a speed field's device array in `layout` (the VARC passes, 2..p2_varc_max_stages steps; 0: constant speed)");
  m.attr("p2_varc_max_stages") = kP2VarcMaxStages;
  // the host-side workgroup arithmetic of the passes (pass_grid.hpp)
  m.def("p2_launch_blocks", [](const std::vector<LBox>& boxes, const LeapfrogTbTiling& t) {
    const P2LaunchGrid g = p2_launch_grid(boxes.data(), static_cast<int>(boxes.size()), t);
    std::vector<std::tuple<int, int, int, int, int>> per;  // (nty, ntz, xlen, nxc, blk0) per box
    for (int k = 0; k < g.nbox; ++k)
      per.emplace_back(g.box[k].nty, g.box[k].ntz, g.box[k].xlen, g.box[k].nxc, g.box[k].blk0);
    return py::make_tuple(g.nblocks, per);
  });
  // the unit plan of a one-rank solve (schedule.cpp, host only): speed = 0 none, 1 pairs, 2 singles, 3 fused (SpeedPlan)
  m.def("plan_units", [](const Problem& p, const SolverOptions& o, int start_n, bool analytic, bool sources, int speed) {
    W3D_REQUIRE(speed >= 0 && speed <= 3, "plan_units: speed plan 0..3");
    const RankSchedule s = make_rank_schedule(p, o, 0, 1, 1e13);
    // lds_pass: the unit is one LDS S-step pass, which checks any of its levels (PassArgs::check_mask); every other
    // unit (a single step, a k_leapfrog2 pair) checks its last level only. checked: the unit's levels n + k that are
    // check steps of the schedule (RankSchedule::is_check, what GpuSolver builds the pass's check mask from)
    const SpeedPlan sp = static_cast<SpeedPlan>(speed);
    const bool passes = sp == SpeedPlan::kNone ? (s.mode == Mode::kFusedSingle && s.opt.tb) || s.mode == Mode::kDeepTb
                                               : sp == SpeedPlan::kFused && speed_fused_ok(s);
    py::list out;
    for (const UnitPlan& u : plan_units(s, start_n, analytic, sources, sp)) {
      py::dict d;
      d["lds_pass"] = passes && u.fused();
      py::list chk;
      for (int k = 1; k <= u.steps; ++k)
        if (s.is_check(u.n + k)) chk.append(u.n + k);
      d["checked"] = chk;
      d["n"] = u.n;
      d["steps"] = u.steps;
      d["analytic"] = u.analytic;
      d["drop_prev"] = u.drop_prev;
      d["exchange"] = u.exchange;
      out.append(d);
    }
    return out;
  }, py::arg("problem"), py::arg("options"), py::arg("start_n") = 1, py::arg("analytic") = false,
     py::arg("sources") = false, py::arg("speed") = 0);
  m.def("tb_slot_blocks", &tb_slot_blocks);
  m.def("tb_shells_launch_blocks", [](const Layout& l, const std::vector<LBox>& boxes, const LeapfrogTbTiling& t,
                                      int slot) {
    return tb_shells_launch_blocks(l, boxes.data(), static_cast<int>(boxes.size()), t, slot);
  });
  // S-deep exchange regions <-> staging (k_box_copy); the table handle is freed with free_box_copy_table
  py::class_<BoxCopyTable>(m, "BoxCopyTable")
      .def_readonly("njobs", &BoxCopyTable::njobs)
      .def_readonly("nblocks", &BoxCopyTable::nblocks);
  m.def("make_box_copy_table", &make_box_copy_table, py::arg("plan"), py::arg("recv_side"),
        py::arg("skip_zfaces") = false);
  m.def("free_box_copy_table", &free_box_copy_table);
  m.def("launch_box_copy", [](const Layout& l, const BoxCopyTable& t, int mode, std::uintptr_t u_s,
                              std::uintptr_t u_s1, std::uintptr_t buf, std::uintptr_t stream) {
    W3D_REQUIRE(mode >= 0 && mode <= 2, "launch_box_copy: mode 0 (pack), 1 (unpack) or 2 (NaN fill)");
    launch_box_copy(l, t, mode, dptr<double>(u_s), dptr<double>(u_s1), dptr<double>(buf), sptr(stream));
  });
  m.def("launch_field_hash", [](const Layout& l, std::uintptr_t f, std::uintptr_t out, std::uintptr_t stream) {
    launch_field_hash(l, dptr<const double>(f), dptr<unsigned long long>(out), sptr(stream));
  }, "adds the hash of the owned nodes of field f into the 64-bit word at `out` (zeroed by the caller)");
  m.def("gpu_error_blocks", &error_blocks);
  m.def("gpu_error", [](const Layout& l, std::uintptr_t u, const LBox& b, std::uintptr_t s, double ct,
                        std::uintptr_t partials, std::uintptr_t stream) {
    launch_error(l, dptr<const double>(u), b, dptr<const double>(s) + 1, ct, dptr<Partial>(partials), sptr(stream));
  });
  m.def("gpu_reduce_batch", [](const std::vector<std::tuple<std::uintptr_t, int, std::uintptr_t>>& jobs,
                               std::uintptr_t stream) {
    std::vector<ReduceJob> js;
    for (const auto& [in, n, out] : jobs) js.push_back(ReduceJob{dptr<const Partial>(in), n, dptr<Partial>(out)});
    launch_reduce_batch(js.data(), static_cast<int>(js.size()), sptr(stream));
  });
  m.def("gpu_reduce", [](std::uintptr_t partials, int n, std::uintptr_t out, std::uintptr_t stream) {
    launch_reduce(dptr<const Partial>(partials), n, dptr<Partial>(out), sptr(stream));
  });
  m.def("gpu_pack", [](const Layout& l, const HaloPlan& p, std::uintptr_t u, std::uintptr_t buf, std::uintptr_t st) {
    launch_pack(l, p, dptr<const double>(u), dptr<double>(buf), sptr(st));
  });
  m.def("gpu_unpack", [](const Layout& l, const HaloPlan& p, std::uintptr_t buf, std::uintptr_t u, std::uintptr_t st) {
    launch_unpack(l, p, dptr<const double>(buf), dptr<double>(u), sptr(st));
  });

  py::class_<SolverOptions>(m, "SolverOptions")
      .def(py::init<>())
      .def_readwrite("decomp", &SolverOptions::decomp)
      .def_readwrite("check_every", &SolverOptions::check_every)
      .def_readwrite("overlap", &SolverOptions::overlap)
      .def_readwrite("graph", &SolverOptions::graph)
      .def_readwrite("timers", &SolverOptions::timers)
      .def_readwrite("debug_sync", &SolverOptions::debug_sync)
      .def_readwrite("poison_ghosts", &SolverOptions::poison_ghosts)
      .def_readwrite("fake_comm", &SolverOptions::fake_comm)
      .def_readwrite("push", &SolverOptions::push)
      .def_readwrite("push_cp_wait", &SolverOptions::push_cp_wait)
      .def_readwrite("sdma", &SolverOptions::sdma)
      .def_readwrite("shells_concurrent", &SolverOptions::shells_concurrent)
      .def_readwrite("reserve_cus", &SolverOptions::reserve_cus)
      .def_readwrite("fake_traffic", &SolverOptions::fake_traffic)
      .def_readwrite("fused_pack", &SolverOptions::fused_pack)
      .def_readwrite("ghost_store", &SolverOptions::ghost_store)
      .def_readwrite("keep_prev", &SolverOptions::keep_prev)
      .def_readwrite("sdma_streams", &SolverOptions::sdma_streams)
      .def_readwrite("flag_timeout_s", &SolverOptions::flag_timeout_s)
      .def_readwrite("push_no_collective", &SolverOptions::push_no_collective)
      .def_readwrite("temporal", &SolverOptions::temporal)
      .def_readwrite("init2", &SolverOptions::init2)
      .def_readwrite("deep_min_planes", &SolverOptions::deep_min_planes)
      .def_readwrite("tb_min_planes", &SolverOptions::tb_min_planes)
      .def_readwrite("tiling2", &SolverOptions::tiling2)
      .def_readwrite("tb", &SolverOptions::tb)
      .def_readwrite("tiling_tb", &SolverOptions::tiling_tb)
      .def_readwrite("tiling", &SolverOptions::tiling);

  py::class_<Comm, std::shared_ptr<Comm>>(m, "Comm")
      .def(py::init([](int rank, int world, py::bytes uid) {
             std::string s = uid;
             py::gil_scoped_release nogil;
             return std::make_shared<Comm>(rank, world, s);
           }),
           py::arg("rank"), py::arg("world"), py::arg("unique_id"))
      .def_static("make_unique_id", []() { return py::bytes(Comm::make_unique_id()); })
      .def_property_readonly("rank", &Comm::rank)
      .def_property_readonly("world", &Comm::world)
      .def("count", &Comm::count)
      .def("device", &Comm::device)
      .def("check_async", &Comm::check_async);

  py::class_<GpuSolver>(m, "GpuSolver")
      .def(py::init([](const Problem& p, const SolverOptions& o, int rank, int world, std::shared_ptr<Comm> c) {
             return std::make_unique<GpuSolver>(p, o, rank, world, std::move(c));
           }),
           py::arg("problem"), py::arg("options"), py::arg("rank") = 0, py::arg("world") = 1,
           py::arg("comm") = nullptr)
      .def_property_readonly("push", &GpuSolver::push)
      .def("push_handles", [](const GpuSolver& s) { return py::bytes(s.push_handles()); },
           "this rank's IPC handles (staging, flags) + device, to be all-gathered")
      .def("connect_push", [](GpuSolver& s, const std::vector<py::bytes>& all) {
             std::vector<std::string> v;
             for (const py::bytes& b : all) v.emplace_back(b);
             s.connect_push(v);
           },
           "open the slab neighbours' staging and flags from every rank's push_handles() (index = rank)")
      .def_property_readonly("sdma", &GpuSolver::sdma)
      .def("sdma_handles", [](const GpuSolver& s) { return py::bytes(s.sdma_handles()); },
           "this rank's IPC handles (field buffers, staging, flags) + layout facts, to be all-gathered")
      .def("connect_sdma", [](GpuSolver& s, const std::vector<py::bytes>& all) {
             std::vector<std::string> v;
             for (const py::bytes& b : all) v.emplace_back(b);
             s.connect_sdma(v);
           },
           "map every neighbour's buffers and flag words from all ranks' sdma_handles() (index = rank)")
      .def_property_readonly("overlapped", &GpuSolver::overlapped)
      .def_property_readonly("transport", &GpuSolver::transport)
      .def("traffic",
           [](GpuSolver& s) {
             const GpuSolver::Traffic t = s.traffic();
             py::dict d;
             d["field_bytes"] = t.field_bytes;
             d["halo_bytes"] = t.halo_bytes;
             return d;
           },
           "bytes one solve of the last run()'s schedule moves: compulsory field reads + writes, halo bytes sent")
      .def("run",
           [](GpuSolver& s) {
             RunResult r;
             {
               py::gil_scoped_release nogil;
               r = s.run();
             }
             return result_dict(r);
           })
      .def("run_batch",
           [](GpuSolver& s, int n) {
             std::vector<RunResult> rs;
             {
               py::gil_scoped_release nogil;
               rs = s.run_batch(n);
             }
             py::list out;
             for (const RunResult& r : rs) out.append(result_dict(r));
             return out;
           },
           py::arg("n"),
           "n solves back to back; a one-rank graph-captured solver enqueues them all and synchronises once (each "
           "solve's own log copied out)")
      .def("download",
           [](const GpuSolver& s, int which) {
             auto v = s.download(which);
             return darr(static_cast<py::ssize_t>(v.size()), v.data());
           },
           py::arg("which") = 0)
      .def("field_hash", &GpuSolver::field_hash, py::arg("which") = 0,
           "order-independent 64-bit hash of the owned nodes of u^K (0) / u^{K-1} (1); summed over the ranks it is "
           "the same for every decomposition that computes bit-identical fields")
      .def_property_readonly("layout", &GpuSolver::layout)
      .def_property_readonly("dims", &GpuSolver::dims)
      .def_property_readonly("halo", &GpuSolver::halo)
      .def_property_readonly("rank", &GpuSolver::rank)
      .def_property_readonly("world", &GpuSolver::world)
      .def("set_state", [](GpuSolver& s, const darr& prev, const darr& cur, int n0) {
        const i64 n = s.problem().N + 1;
        s.set_state(ro_ptr(prev, n * n * n, "prev"), ro_ptr(cur, n * n * n, "cur"), n0);
      }, py::arg("prev"), py::arg("cur"), py::arg("step"))
      .def("set_initial", [](GpuSolver& s, const darr& phi, py::object psi) {
        const i64 n = s.problem().N + 1;
        darr psi_a;
        if (!psi.is_none()) psi_a = psi.cast<darr>();
        s.set_initial(ro_ptr(phi, n * n * n, "phi"), psi.is_none() ? nullptr : ro_ptr(psi_a, n * n * n, "psi"));
      }, py::arg("phi"), py::arg("psi") = py::none())
      .def("set_speed", [](GpuSolver& s, py::object c, bool force) {
        if (c.is_none()) return s.set_speed(nullptr);
        const i64 n = s.problem().N + 1;
        const darr c_a = c.cast<darr>();
        s.set_speed(ro_ptr(c_a, n * n * n, "c"), force);
      }, py::arg("c"), py::arg("force") = false, "solve u_tt = c(x)^2 Lap u with this global (N+1)^3 field (None clears it)")
      .def_property_readonly("speed", &GpuSolver::speed)
      .def_property_readonly("speed_range", [](const GpuSolver& s) {
        return py::make_tuple(s.speed_range().cmin, s.speed_range().cmax);
      })
      .def("set_receivers", [](GpuSolver& s, const iarr& nodes) {
        int R = 0;
        const i64* p = receiver_ptr(nodes, &R);
        s.set_receivers(p, R);
      }, py::arg("nodes"), "record u^n at these (R, 3) global nodes in every following solve (this rank: the ones it owns)")
      .def("traces", [](const GpuSolver& s) {
        const GpuSolver::Traces t = s.traces();
        const py::ssize_t own = static_cast<py::ssize_t>(t.slots.size());
        darr v({static_cast<py::ssize_t>(s.problem().K + 1), own});
        if (own > 0) std::memcpy(v.mutable_data(), t.values.data(), t.values.size() * sizeof(double));
        return py::make_tuple(v, t.slots);
      }, "the last solve's ((K+1, owned) values, the owned receivers' slots in the list)")
      .def_property_readonly("analytic_start", &GpuSolver::analytic_start)
      .def("set_sources", [](GpuSolver& s, const iarr& nodes, const darr& w) {
        int Q = 0;
        const double* wp = source_w(s.problem(), nodes, w, &Q);
        s.set_sources(nodes.data(), Q, wp);
      }, py::arg("nodes"), py::arg("w"), "point sources at these (Q, 3) global nodes with the (K, Q) samples w")
      .def_property_readonly("sources", &GpuSolver::sources)
      .def_property_readonly("sponge", &GpuSolver::sponge)
      .def("energy", &GpuSolver::energy, py::arg("which") = 0,
           "discrete energy E^{K-1/2} (which = 0) / E^{1/2} (which = 1, after set_initial); one rank only")
      .def("energy_sums", [](const GpuSolver& s, int which) {
             const Partial e = s.energy_sums(which);
             return py::make_tuple(e.x, e.y);
           }, py::arg("which") = 0, "the kinetic and potential sums energy() is formed from")
      .def("shell_boxes", &GpuSolver::shell_boxes)
      .def("interior_box", &GpuSolver::interior_box)
      .def("check_steps", &GpuSolver::check_steps)
      .def("device_bytes", &GpuSolver::device_bytes)
      .def_property_readonly("mode", &GpuSolver::mode)
      .def_property_readonly("stored_prev", &GpuSolver::stored_prev)
      .def_property_readonly("unit_steps", &GpuSolver::unit_steps)
      .def_property_readonly("graph_enabled", [](const GpuSolver& s) { return s.options().graph; });

  // the CLI's multi-rank schedule autotune (runtime_autotune.cpp): same candidates, same rules; collectives over the
  // RCCL communicator (world > 1) or none (one rank / a fake rank)
  m.def(
      "autotune",
      [](const Problem& p, const SolverOptions& o, int rank, int world, std::shared_ptr<Comm> c, bool fake,
         bool with_push, int rounds, double tie, bool with_sdma, int reps, double budget_s) {
        W3D_REQUIRE(world == 1 || fake || c, "autotune: world > 1 needs an RCCL communicator");
        const HostColl hc = c ? HostColl::rccl(c) : HostColl::single(rank);
        AutotuneOptions ao;
        ao.with_push = with_push;
        ao.with_sdma = with_sdma;
        ao.rounds = rounds;
        ao.reps = reps;
        ao.tie = tie;
        ao.budget_s = budget_s;
        AutotuneResult r;
        {
          py::gil_scoped_release nogil;
          r = autotune(p, o, rank, world, c, hc, fake, ao);
        }
        py::dict times, rejected;
        for (const auto& [k, v] : r.times) times[py::str(k)] = v;
        for (const auto& [k, v] : r.rejected) rejected[py::str(k)] = v;
        return py::make_tuple(py::cast(std::move(r.solver)), r.name, times, rejected);
      },
      py::arg("problem"), py::arg("options"), py::arg("rank") = 0, py::arg("world") = 1, py::arg("comm") = nullptr,
      py::arg("fake") = false, py::arg("with_push") = false, py::arg("rounds") = 5, py::arg("tie") = 0.02,
      py::arg("with_sdma") = false, py::arg("reps") = 5, py::arg("budget_s") = 120.0,
      "time the schedule candidates (slab/block, pass depth, overlap, RCCL/copy engines) and return "
      "(GpuSolver, name, {name: seconds}, {name: reason rejected})");

  py::class_<GpuGroup>(m, "GpuGroup")
      .def(py::init([](const Problem& p, const SolverOptions& o, int world, const std::string& transport) {
             py::gil_scoped_release nogil;
             return std::make_unique<GpuGroup>(p, o, world, transport);
           }),
           py::arg("problem"), py::arg("options"), py::arg("world"), py::arg("transport") = "loopback")
      .def("run",
           [](GpuGroup& g) {
             RunResult r;
             {
               py::gil_scoped_release nogil;
               r = g.run();
             }
             return result_dict(r);
           })
      .def("download",
           [](GpuGroup& g, int rank, int which) {
             auto v = g.rank(rank).download(which);
             return darr(static_cast<py::ssize_t>(v.size()), v.data());
           },
           py::arg("rank"), py::arg("which") = 0)
      .def("field_hash", [](GpuGroup& g, int rank, int which) { return g.rank(rank).field_hash(which); },
           py::arg("rank"), py::arg("which") = 0)
      .def("layout", [](GpuGroup& g, int rank) { return g.rank(rank).layout(); })
      .def("dims", [](GpuGroup& g) { return g.rank(0).dims(); })
      .def("mode", [](GpuGroup& g) { return g.rank(0).mode(); })
      .def("stored_prev", [](GpuGroup& g, int rank) { return g.rank(rank).stored_prev(); }, py::arg("rank") = 0)
      .def("temporal", [](GpuGroup& g) { return g.rank(0).options().temporal; },
           "pass depth every rank runs (the constructor lowers the requested depth where a schedule needs it)")
      .def("overlapped", [](GpuGroup& g) { return g.rank(0).overlapped(); })
      .def("comm_counts", &GpuGroup::comm_counts)
      .def("traffic",
           [](GpuGroup& g, int rank) {
             const GpuSolver::Traffic t = g.rank(rank).traffic();
             py::dict d;
             d["field_bytes"] = t.field_bytes;
             d["halo_bytes"] = t.halo_bytes;
             return d;
           },
           py::arg("rank"), "GpuSolver.traffic() of one rank (bytes per solve of the last run()'s schedule)")
      .def("set_state", [](GpuGroup& g, const darr& prev, const darr& cur, int n0) {
        const i64 n = g.rank(0).problem().N + 1;
        g.set_state(ro_ptr(prev, n * n * n, "prev"), ro_ptr(cur, n * n * n, "cur"), n0);
      }, py::arg("prev"), py::arg("cur"), py::arg("step"))
      .def("set_initial", [](GpuGroup& g, const darr& phi, py::object psi) {
        const i64 n = g.rank(0).problem().N + 1;
        darr psi_a;
        if (!psi.is_none()) psi_a = psi.cast<darr>();
        g.set_initial(ro_ptr(phi, n * n * n, "phi"), psi.is_none() ? nullptr : ro_ptr(psi_a, n * n * n, "psi"));
      }, py::arg("phi"), py::arg("psi") = py::none())
      .def("set_receivers", [](GpuGroup& g, const iarr& nodes) {
        int R = 0;
        const i64* p = receiver_ptr(nodes, &R);
        g.set_receivers(p, R);
      }, py::arg("nodes"))
      .def("traces", [](const GpuGroup& g) {
        const std::vector<double> t = g.traces();
        const py::ssize_t rows = static_cast<py::ssize_t>(g.problem().K + 1);
        return darr({rows, static_cast<py::ssize_t>(t.size()) / rows}, t.data());
      }, "the last run()'s global (K+1, R) values, assembled from the ranks")
      .def("set_sources", [](GpuGroup& g, const iarr& nodes, const darr& w) {
        int Q = 0;
        const double* wp = source_w(g.problem(), nodes, w, &Q);
        g.set_sources(nodes.data(), Q, wp);
      }, py::arg("nodes"), py::arg("w"))
      .def_property_readonly("sources", &GpuGroup::sources)
      .def_property_readonly("transport", &GpuGroup::transport)
      .def_property_readonly("graph_enabled", &GpuGroup::graph_enabled)
      .def_property_readonly("world", &GpuGroup::world);
}
