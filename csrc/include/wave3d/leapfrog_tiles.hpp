// The (y rows × 64 pairs × x chunk) tiling of the single-step kernels (k_leapfrog_lds, k_leapfrog_rq, the fourth-order
// march): one TileBox per launched box, the host planner that fills them, and the device decode blockIdx → tile → box →
// (tz, ty, tx). Host and device; no HIP header is needed for the planner.
#pragma once

#include <string>

#include "wave3d/cpu.hpp"
#include "wave3d/decomp.hpp"
#if defined(__HIPCC__)
#include "wave3d/device_util.hpp"
#endif

namespace wave3d {

constexpr int kMaxBoxes = 6;    // boxes per launch (shell_split: up to 6 shells)
constexpr int kTilePairs = 64;  // pairs per tile row: one wave

struct TileBox {
  i64 x0, x1;    // local x range
  i64 y0, y1;    // local y range
  i64 zo0, zo1;  // row-offset range of the updated nodes
  i64 pz0, pz_end;
  int ntz, nty, xchunk, tile_begin;
};

// The tiles of one launch, the tail of a kernel's argument struct. nblocks and xcd_remap are the launcher's.
struct TileGrid {
  int nbox, ntiles, nblocks, xcd_remap;
  TileBox box[kMaxBoxes];
};

// Tiles of `rows` rows: the non-empty boxes in order, tz fastest, then ty, then the x chunk. The x chunks are spread over
// the boxes by work so that the launch has about `target` tiles, and no chunk is shorter than `min_chunk` planes (a chunk
// re-reads the planes of its x halo) unless its box is. Fills g.box, g.nbox and g.ntiles. `prefix` starts the message
// about min_chunk, which a caller's own argument can break.
inline void plan_tiles(const Layout& l, const LBox* boxes, int nbox, int rows, int min_chunk, int target,
                       const char* prefix, TileGrid& g) {
  W3D_REQUIRE(nbox >= 0 && nbox <= kMaxBoxes, "too many boxes in one leapfrog launch");
  W3D_REQUIRE(min_chunk >= 1, std::string(prefix) + "the x chunk floor must be >= 1");
  // tiles before x-chunking, to spread the x-chunk count over boxes
  i64 base_total = 0;
  for (int b = 0; b < nbox; ++b) {
    const LBox& x = boxes[b];
    if (x.empty()) continue;
    const i64 zo0 = x.z0 + 1 + l.zs, zo1 = x.z1 + 1 + l.zs;
    base_total += ceil_div((zo1 + 1) / 2 - zo0 / 2, kTilePairs) * ceil_div(x.y1 - x.y0, rows);
  }
  const i64 want = base_total > 0 ? imax(1, ceil_div(target, base_total)) : 1;
  int nb = 0, tiles = 0;
  for (int b = 0; b < nbox; ++b) {
    const LBox& x = boxes[b];
    if (x.empty()) continue;
    TileBox& tb = g.box[nb];
    tb.x0 = x.x0;
    tb.x1 = x.x1;
    tb.y0 = x.y0;
    tb.y1 = x.y1;
    tb.zo0 = x.z0 + 1 + l.zs;
    tb.zo1 = x.z1 + 1 + l.zs;
    tb.pz0 = tb.zo0 / 2;
    tb.pz_end = (tb.zo1 + 1) / 2;
    // (the pair right of the last pair lies inside the row)
    W3D_REQUIRE(2 * tb.pz_end + 2 <= l.pitch, "row pitch too small for the pair tiling");
    tb.ntz = static_cast<int>(ceil_div(tb.pz_end - tb.pz0, kTilePairs));
    tb.nty = static_cast<int>(ceil_div(x.y1 - x.y0, rows));
    const i64 nxb = x.x1 - x.x0;
    i64 chunk = imax(static_cast<i64>(min_chunk), ceil_div(nxb, want));
    chunk = imin(chunk, nxb);
    tb.xchunk = static_cast<int>(chunk);
    const i64 nxc = ceil_div(nxb, chunk);
    tb.tile_begin = tiles;
    const i64 bt = static_cast<i64>(tb.ntz) * tb.nty * nxc;
    W3D_REQUIRE(tiles + bt < (1ll << 30), "too many tiles");
    tiles += static_cast<int>(bt);
    ++nb;
  }
  g.nbox = nb;
  g.ntiles = tiles;
}

#if defined(__HIPCC__)
static_assert(kTilePairs == kLanes, "the planner's tile row is the kernels' wave");

// blockIdx → tile: with xcd_remap each XCD (blockIdx % 8) gets a contiguous run of tiles, so y-adjacent tiles that share
// halo rows share one L2 (nblocks is a multiple of 8 then)
__device__ __forceinline__ int tile_of_block(const TileGrid& g) {
  int tile = static_cast<int>(blockIdx.x);
  if (g.xcd_remap) {
    const int per = g.nblocks >> 3;
    tile = (static_cast<int>(blockIdx.x) & 7) * per + (static_cast<int>(blockIdx.x) >> 3);
  }
  return tile;
}

// tile → its box and its place (tz, ty, tx) in it; false: no such tile (a grid rounded up for xcd_remap).
// (g by value, not by reference: with a reference into the kernel-argument struct the compiler copies the six boxes to
// scratch, 488 bytes per lane; by value they stay scalar loads of the arguments — profiles/march4)
__device__ __forceinline__ bool decode_tile(const TileGrid g, int tile, TileBox& B, int& tz, int& ty, int& tx) {
  if (tile >= g.ntiles) return false;
  // select the box (scalar selects, no dynamic indexing of the kernarg struct)
  B = g.box[0];
#pragma unroll
  for (int k = 1; k < kMaxBoxes; ++k)
    if (k < g.nbox && tile >= g.box[k].tile_begin) B = g.box[k];
  int t = tile - B.tile_begin;
  tz = t % B.ntz;
  t /= B.ntz;
  ty = t % B.nty;
  tx = t / B.nty;
  return true;
}
#endif

}  // namespace wave3d
