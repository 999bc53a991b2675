// Stand-alone driver for tests/test_sigma_grid_host.py: the Σ pass's tile grid (sigma_grid.hpp, what
// launch_sigma_pass sizes its grid from and k_sigma_pass takes its tile from) on the host. No HIP,
// no GPU.
//
//   sigma_grid_host_main        prints one line per mode and "ok", or the failures; exit 1 on any
//
// Per case (tile shape, n, n_filters) every (blockIdx.x, blockIdx.y, wave) of the geometry's grid
// goes through sigma_grid_tile. The (filter, tile row, tile column) it yields must be exactly the
// required set, each member once, no filter ≥ n_filters: every tile of the trows × tcols grid for a
// full pass; for a symmetric pass the tiles holding an element on or above the diagonal, those with
// 32·tr ≤ cols·tc + cols − 1 (worked out here, not with the header's helpers). The grid's
// dimensions must be what the launcher computed before the header existed (expected_grid).
// Shapes and filter counts as the launcher pairs them: 32 × 32 full (fp32) with any count, 32 × 32
// symmetric (fp64) below 16 filters, 32 × 64 symmetric from 16 on. n = 1 … 300, 513, 1025, 2051.
#include <cstdio>
#include <vector>

#include "sigma_grid.hpp"

using namespace ekfslam;

namespace {

constexpr int kWpb = 4;  // waves per workgroup (kPassWaves)
const int kFilters[6] = {1, 2, 15, 16, 17, 24};

int g_bad = 0;
long g_cases[3][2];  // [mode][symmetric]

bool required(int cols, bool sym, int tr, int tc) { return !sym || 32 * tr <= cols * tc + cols - 1; }

// launch_sigma_pass's grid before sigma_grid.hpp
void expected_grid(int n, int nf, int rows, int cols, bool sym, int& gx, int& gy, int& mode) {
  const int trows = (n + rows - 1) / rows, tcols = (n + cols - 1) / cols;
  int tiles = trows * tcols;
  if (sym) {
    tiles = 0;
    for (int tr = 0; tr < trows; ++tr) tiles += tcols - 32 * tr / cols;
  }
  if (nf >= 16) {
    const int per_filter = (tiles + kWpb - 1) / kWpb;
    gx = 8 * ((nf + 7) / 8) * per_filter;
    gy = 1;
    mode = kGridXcd;
  } else if (trows >= 4 && tcols >= 8) {
    const int per_x = sym ? (tiles + 7) / 8 : ((trows + 1) / 2) * ((tcols + 3) / 4);
    gx = 8 * ((per_x + kWpb - 1) / kWpb);
    gy = nf;
    mode = kGridRegions;
  } else {
    gx = (tiles + kWpb - 1) / kWpb;
    gy = nf;
    mode = kGridPlain;
  }
}

template <int kRows, int kCols, bool kSym>
void run_case(int n, int nf) {
  const SigmaGrid g = sigma_grid(n, nf, kRows, kCols, kSym, kWpb);
  int gx, gy, mode;
  expected_grid(n, nf, kRows, kCols, kSym, gx, gy, mode);
  const int trows = (n + kRows - 1) / kRows, tcols = (n + kCols - 1) / kCols;
  int bad = 0;
  if (g.grid_x != gx || g.grid_y != gy || g.mode != mode || g.trows != trows || g.tcols != tcols ||
      g.nf != nf || g.wpb != kWpb)
    ++bad;
  std::vector<int> seen(static_cast<size_t>(nf) * trows * tcols, 0);
  for (int by = 0; by < g.grid_y && !bad; ++by)
    for (int bx = 0; bx < g.grid_x; ++bx)
      for (int w = 0; w < kWpb; ++w) {
        const SigmaTileAt at = sigma_grid_tile<kCols, kSym>(g, bx, by, w);
        // (the kernel resolves the workgroup's filter on its own first)
        int b;
        const int fb = sigma_grid_filter(g, bx, by, b);
        if (at.filter >= 0 && at.filter != fb) ++bad;
        if (at.filter < 0) continue;
        if (at.filter >= nf || at.tr < 0 || at.tr >= trows || at.tc < 0 || at.tc >= tcols) {
          ++bad;
          continue;
        }
        ++seen[(static_cast<size_t>(at.filter) * trows + at.tr) * tcols + at.tc];
      }
  long want = 0;
  for (int f = 0; f < nf; ++f)
    for (int tr = 0; tr < trows; ++tr)
      for (int tc = 0; tc < tcols; ++tc) {
        const int need = required(kCols, kSym, tr, tc) ? 1 : 0;
        want += need;
        if (seen[(static_cast<size_t>(f) * trows + tr) * tcols + tc] != need) ++bad;
      }
  if (g.tiles * static_cast<long>(nf) != want) ++bad;
  ++g_cases[mode][kSym];
  if (bad && ++g_bad <= 20)
    std::printf("FAIL tile %dx%d sym %d n %d filters %d: grid %d x %d mode %d (want %d x %d mode %d), "
                "%d wrong\n", kRows, kCols, kSym, n, nf, g.grid_x, g.grid_y, g.mode, gx, gy, mode, bad);
}

void run_size(int n) {
  for (int nf : kFilters) {
    run_case<32, 32, false>(n, nf);
    if (nf < 16)
      run_case<32, 32, true>(n, nf);
    else
      run_case<32, 64, true>(n, nf);
  }
}

}  // namespace

int main() {
  for (int n = 1; n <= 300; ++n) run_size(n);
  for (int n : {513, 1025, 2051}) run_size(n);
  const char* names[3] = {"plain", "xcd", "regions"};
  for (int m = 0; m < 3; ++m)
    std::printf("mode %s: full %ld symmetric %ld\n", names[m], g_cases[m][0], g_cases[m][1]);
  if (g_bad) {
    std::printf("%d cases failed\n", g_bad);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
