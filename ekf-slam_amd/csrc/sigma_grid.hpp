// The Σ pass's tile grid, once for host and device: the grid a pass of n rows over n_filters
// filters launches (launch_sigma_pass: sigma_grid()) and the tile of which filter each wave of it
// takes (k_sigma_pass: sigma_grid_tile()). If the two disagreed a tile would silently never be
// written, or be written twice by racing waves: tests/sigma_grid_host_main.cpp walks every wave of
// every grid through the mapping on the host. Plain C++, nothing of HIP is needed.
//
// One tile per wave, row-major over the filter's trows × tcols tiles, in one of three modes:
//   plain      grid (workgroups per filter, filters): workgroup b's wave w takes tile b·wpb + w.
//   XCD-dealt  (many filters) a 1-D grid whose block L runs on XCD L % 8 (dispatch deals blocks
//              round-robin over the XCDs); it is given filter 8·⌊(L/8)/B⌋ + L % 8, tile block
//              (L/8) % B, so all of a filter's B blocks share one XCD and its Kcat/Mcat are fetched
//              into one L2 instead of eight.
//   regions    (few filters, one per blockIdx.y) the tile grid is cut 2 × 4, block L takes region
//              L % 8 (so XCD L % 8 does): each XCD's L2 then fetches half of Kcat and a quarter of
//              Mcat instead of both whole (beyond Σ: 8 × (Kcat + Mcat) → 4 × Kcat + 2 × Mcat).
// Symmetric (the fp64 pass): only the tiles holding an element on or above the diagonal, tile row
// tr's columns ⌊32·tr / cols⌋ … tcols − 1; in regions mode XCD x takes the x-th eighth of that list.
// Placement changes speed only, but it is a measured property: keep the enumeration order.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EKF_GRID_HD __host__ __device__
#else
#define EKF_GRID_HD
#endif
// the wave's tile index, provably wave-uniform on the device: the buffer descriptors built from it
// stay in SGPRs instead of a waterfall loop around every access
#if defined(__HIP_DEVICE_COMPILE__)
#define EKF_GRID_UNIFORM(v) __builtin_amdgcn_readfirstlane(v)
#else
#define EKF_GRID_UNIFORM(v) (v)
#endif

namespace ekfslam {

enum SigmaGridMode : int { kGridPlain = 0, kGridXcd = 1, kGridRegions = 2 };
constexpr int kGridXcdFilters = 16;        // this many filters or more: the XCD-dealt grid
constexpr int kRegRows = 2, kRegCols = 4;  // the regions of a full pass (one per XCD)

struct SigmaGrid {
  int trows, tcols;  // the tile grid of one filter
  int mode;          // SigmaGridMode
  int tiles;         // tiles per filter: all trows·tcols, or the symmetric pass's upper ones
  int per;           // workgroups per filter (plain, XCD-dealt) or per XCD (regions)
  int nf, wpb;       // filters; waves per workgroup
  int grid_x, grid_y;
};
struct SigmaTileAt {
  int filter, tr, tc;  // filter < 0: the wave has no tile
};

// tile rows are 32 high whatever the tile's width (cols)
EKF_GRID_HD inline int sym_first(int cols, int tr) { return 32 * tr / cols; }
EKF_GRID_HD inline int sym_tiles(int cols, int trows, int tcols) {
  int t = 0;
  for (int tr = 0; tr < trows; ++tr) t += tcols - sym_first(cols, tr);
  return t;
}
// the t-th of them, row-major (wave-uniform t: a scalar walk over the tile rows)
EKF_GRID_HD inline bool sym_tile(int cols, int t, int trows, int tcols, int& tr, int& tc) {
  int base = 0;
  for (tr = 0; tr < trows; ++tr) {
    const int c = tcols - sym_first(cols, tr);
    if (t < base + c) break;
    base += c;
  }
  tc = tr < trows ? sym_first(cols, tr) + (t - base) : 0;
  return tr < trows;
}
EKF_GRID_HD inline int region_tiles(int trows, int tcols) {  // the largest region's tiles
  return ((trows + kRegRows - 1) / kRegRows) * ((tcols + kRegCols - 1) / kRegCols);
}

// The grid of one pass: n rows and columns per filter in tiles of rows × cols, wpb waves (= tiles)
// per workgroup.
EKF_GRID_HD inline SigmaGrid sigma_grid(int n, int n_filters, int rows, int cols, bool symmetric,
                                        int wpb) {
  SigmaGrid g;
  g.trows = (n + rows - 1) / rows;
  g.tcols = (n + cols - 1) / cols;
  g.tiles = symmetric ? sym_tiles(cols, g.trows, g.tcols) : g.trows * g.tcols;
  g.nf = n_filters;
  g.wpb = wpb;
  g.grid_y = n_filters;
  if (n_filters >= kGridXcdFilters) {
    g.mode = kGridXcd;
    g.per = (g.tiles + wpb - 1) / wpb;
    g.grid_x = 8 * ((n_filters + 7) / 8) * g.per;
    g.grid_y = 1;
  } else if (g.trows >= 2 * kRegRows && g.tcols >= 2 * kRegCols) {
    // XCD regions, each at least 2 × 2 tiles
    g.mode = kGridRegions;
    const int per_x = symmetric ? (g.tiles + 7) / 8 : region_tiles(g.trows, g.tcols);
    g.per = (per_x + wpb - 1) / wpb;
    g.grid_x = 8 * g.per;
  } else {
    g.mode = kGridPlain;
    g.per = (g.tiles + wpb - 1) / wpb;
    g.grid_x = g.per;
  }
  return g;
}

// The filter of workgroup (bx, by), < 0 for none, and b, the workgroup's index among its filter's
// (XCD-dealt, plain) or bx itself (regions).
EKF_GRID_HD inline int sigma_grid_filter(const SigmaGrid& g, int bx, int by, int& b) {
  b = bx;
  if (g.mode != kGridXcd) return by;
  const int j = bx >> 3;
  const int f = (bx & 7) + 8 * (j / g.per);
  b = j % g.per;
  return f < g.nf ? f : -1;
}

// The tile of wave `wave` (0 … wpb − 1) of workgroup (bx, by) in g's grid. kCols, kSym: the cols
// and symmetric g was built with, as constants (the kernel's tile type: ⌊32·tr / cols⌋ folds).
template <int kCols, bool kSym>
EKF_GRID_HD inline SigmaTileAt sigma_grid_tile(const SigmaGrid& g, int bx, int by, int wave) {
  int b;
  SigmaTileAt at{sigma_grid_filter(g, bx, by, b), 0, 0};
  if (at.filter < 0) return at;
  bool ok;
  if (g.mode == kGridRegions) {
    const int x = bx & 7;  // the XCD
    const int w = EKF_GRID_UNIFORM((bx >> 3) * g.wpb + wave);
    if (kSym) {  // the x-th eighth of the upper tiles
      const int lo = x * g.tiles / 8, hi = (x + 1) * g.tiles / 8;
      ok = lo + w < hi && sym_tile(kCols, lo + w, g.trows, g.tcols, at.tr, at.tc);
    } else {
      const int hx = x / kRegCols, qx = x % kRegCols;
      const int r0 = hx * g.trows / kRegRows, r1 = (hx + 1) * g.trows / kRegRows;
      const int c0 = qx * g.tcols / kRegCols, c1 = (qx + 1) * g.tcols / kRegCols;
      const int cw = c1 - c0;
      ok = w < (r1 - r0) * cw;
      at.tr = r0 + w / cw;
      at.tc = c0 + w % cw;
    }
  } else {
    const int t = EKF_GRID_UNIFORM(b * g.wpb + wave);
    if (kSym) {
      ok = sym_tile(kCols, t, g.trows, g.tcols, at.tr, at.tc);
    } else {
      ok = t < g.tiles;
      at.tr = t / g.tcols;
      at.tc = t - at.tr * g.tcols;
    }
  }
  if (!ok) at.filter = -1;
  return at;
}

}  // namespace ekfslam
