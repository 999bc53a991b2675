// match_math.hpp (ekf-slam_amd/csrc) on the CPU: the matching arithmetic of k_eval_match
// (ekf_eval.hip), driven phase by phase the way the kernel drives it, on cases
// tests/test_match_math_host.py writes and holds against numpy. Compiled by the host compiler alone,
// under AddressSanitizer + UndefinedBehaviorSanitizer.
//
//   match_math_host_main <cases.bin> <results.bin>
//
// Both files are flat arrays of doubles. cases.bin: the number of cases, then per case
//   N, n_map, max_dist, x[N][2] (the slots' estimates), truth[n_map][2] (in the map frame)
// results.bin: per case
//   match[N], best_d2[N] (the nearest truth's squared distance, +inf if none), n_truth, n_matched,
//   n_primary, n_dup, n_spurious, n_missed, max_match_dist, n_seen
#include <cstdio>
#include <vector>

#include "match_math.hpp"

using namespace ekfslam;

namespace {

std::vector<double> read_all(const char* path) {
  std::vector<double> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) return v;
  double buf[512];
  size_t k;
  while ((k = std::fread(buf, sizeof(double), 512, f)) > 0) v.insert(v.end(), buf, buf + k);
  std::fclose(f);
  return v;
}

struct Reader {
  const std::vector<double>& v;
  size_t at = 0;
  bool bad = false;
  const double* take(size_t k) {
    if (at + k > v.size()) {
      bad = true;
      return nullptr;
    }
    const double* p = v.data() + at;
    at += k;
    return p;
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s cases.bin results.bin\n", argv[0]);
    return 2;
  }
  const std::vector<double> in = read_all(argv[1]);
  Reader r{in};
  const double* head = r.take(1);
  if (!head) return 2;
  const int cases = static_cast<int>(head[0]);
  std::vector<double> out;
  int done = 0;
  for (; done < cases; ++done) {
    const double* h = r.take(3);
    if (!h) break;
    const int N = static_cast<int>(h[0]), n_map = static_cast<int>(h[1]);
    if (N < 0 || n_map < 1 || n_map > kMatchMaxMap) break;
    const double gate2 = h[2] * h[2];
    const double* x = r.take(2 * static_cast<size_t>(N));
    const double* T = r.take(2 * static_cast<size_t>(n_map));
    if (r.bad) break;
    // stage
    MatchAcc acc{};
    std::vector<int> claim(n_map, kClaimFree);
    for (int k = 0; k < n_map; ++k) acc.n_truth += truth_present(T[2 * k], T[2 * k + 1]) ? 1 : 0;
    // scan and claim, slots in descending order: the claim must not depend on it
    std::vector<int> match(N, -1);
    std::vector<Nearest> best(N, nearest_none());
    for (int j = N - 1; j >= 0; --j) {
      best[j] = nearest_truth(x[2 * j], x[2 * j + 1], T, n_map);
      if (!lm_seen(x[2 * j], x[2 * j + 1]) || !match_gate(best[j], gate2)) continue;
      match[j] = best[j].k;
      claim_take(&claim[best[j].k], j);
    }
    // count
    int n_seen = 0;
    for (int j = 0; j < N; ++j) {
      n_seen += lm_seen(x[2 * j], x[2 * j + 1]) ? 1 : 0;
      if (match[j] >= 0) match_count(&acc, j, best[j].d2, claim[match[j]]);
    }
    const MatchRec rec = match_store(acc, n_seen);
    for (int j = 0; j < N; ++j) out.push_back(match[j]);
    for (int j = 0; j < N; ++j) out.push_back(best[j].d2);
    const double res[8] = {static_cast<double>(rec.n_truth),    static_cast<double>(rec.n_matched),
                           static_cast<double>(rec.n_primary),  static_cast<double>(rec.n_dup),
                           static_cast<double>(rec.n_spurious), static_cast<double>(rec.n_missed),
                           rec.max_match_dist,                  static_cast<double>(n_seen)};
    out.insert(out.end(), res, res + 8);
  }
  if (done != cases || r.at != in.size()) {
    std::fprintf(stderr, "malformed case file: %d of %d cases, %zu of %zu doubles\n", done, cases,
                 r.at, in.size());
    return 2;
  }
  FILE* f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) return 2;
  std::fclose(f);
  std::printf("cases %d results %zu\nok\n", cases, out.size());
  return 0;
}
