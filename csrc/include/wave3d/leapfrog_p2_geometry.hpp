// LDS geometry of the pair-tiled S-step pass (k_leapfrog_p2): the tile edge, the plane layout per stage count and the
// bytes a pass takes. Plain constexpr arithmetic, no HIP header: the kernel (leapfrog_p2_kernel.hpp) and the host-side
// block-count arithmetic (pass_grid.hpp) both read it from here.
#pragma once

#include <cstddef>

namespace wave3d {
namespace p2k {

constexpr int kT = 32;      // output tile edge (y and z)

// Geometry of an S-step tile (region coordinates: row a = y − (ty0 − (S−1)), z_r = z − (tz0 − E)).
//   stage-1 region: rows [0, HY), z_r ∈ [0, HZ); its z extent is rounded out to whole 16-byte pairs (E ≥ S − 1, even)
//   level-0 (u^n) planes add a one-pair ring: rows −1..HY, pair columns −1..PZ (row stride R0 pairs)
//   levels 1..S−1 live in compact planes of HY rows × R1 pairs
// R0, R1 ≡ 4 (mod 8) pairs: a ds_write_b128 serves 8 lanes per LDS cycle (8 × 16 B = 128 B, banks (addr/4) mod 32),
// and the inner waves' lanes 0–7 hold pair columns 0–3 of two rows: R ≡ 4 (mod 8) puts the second row's four pairs on
// the other half of the 128 B (MI355X_MICROARCH.md §LDS).
template <int S>
struct Geo {
  static_assert(S >= 2 && S <= 5, "p2: S must be 2..5");
  static constexpr int E = (S / 2) * 2;
  static constexpr int HY = kT + 2 * (S - 1);
  static constexpr int HZ = kT + 2 * E;
  static constexpr int PZ = HZ / 2;
  static constexpr int NP = HY * PZ;
  static constexpr int pad4(int v) { return v + ((4 - v % 8) + 8) % 8; }
  static constexpr int R0 = pad4(PZ + 2);
  static constexpr int P0 = (HY + 2) * R0;
  static constexpr int R1 = pad4(PZ);
  static constexpr int P1 = HY * R1;
  static constexpr int G1 = R1 + 1;   // guard pairs before / after the compact block (edge reads stay inside LDS)
  static constexpr int NY = HY + 4;   // y sin table: a ∈ [−2, HY + 2)
  static constexpr int NZ = HZ + 8;   // z sin table: z_r ∈ [−4, HZ + 4)
  // (in pairs) level-0 slots [0, 2·P0), then the compact levels (the analytic start needs no more: φ and its
  // neighbours are table products)
  static constexpr int lk0() { return 2 * P0 + G1; }
  static constexpr int pairs() { return lk0() + 2 * (S - 1) * P1 + G1; }
  static constexpr int tab_doubles(int nxt) { return NY + NZ + nxt; }
};

template <int S>
constexpr size_t p2_lds_bytes(int nxt) {
  return static_cast<size_t>(Geo<S>::pairs()) * 16 + static_cast<size_t>(Geo<S>::tab_doubles(nxt)) * 8;
}
// x sin table length for a chunk of xlen planes: x ∈ [x0 − S − 1, x1 + S + 2]
template <int S>
constexpr int p2_nxt(int xlen) {
  return xlen + 2 * S + 4;
}

}  // namespace p2k
}  // namespace wave3d
