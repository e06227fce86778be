// A program of its own that walks outerbase_amd/csrc/acquire_front.h (plain C++): front_insert against a brute-force
// undominated set on seeded point clouds with ties, duplicates and points outside the box, and the capacity of
// 2048 points filled to the last slot.  tests/test_acquire_multi_host.py builds it with the address and
// undefined-behaviour sanitizers and runs it; it prints "ok <cases>" and returns 0, or says what failed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <utility>
#include <vector>

#include "../outerbase_amd/csrc/acquire_front.h"

using obhip::front_insert;
typedef std::pair<double, double> Pt;

static uint64_t rng_state = 12345;
static double uniform() {  // a small LCG: the same points everywhere
  rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
  return (double)(rng_state >> 11) / 9007199254740992.0;
}

static std::vector<Pt> brute(const std::vector<Pt> &pts, double r1, double r2) {
  std::vector<Pt> in, out;
  for (const Pt &p : pts)
    if (p.first < r1 && p.second < r2) in.push_back(p);
  for (size_t i = 0; i < in.size(); ++i) {
    bool dominated = false;
    for (size_t l = 0; l < in.size() && !dominated; ++l)
      if (l != i && in[l].first <= in[i].first && in[l].second <= in[i].second && (in[l] != in[i] || l < i)) dominated = true;
    if (!dominated) out.push_back(in[i]);
  }
  std::sort(out.begin(), out.end());
  return out;
}

int main() {
  int cases = 0;
  for (int trial = 0; trial < 200; ++trial) {
    const int n = 1 + trial % 40;
    const double r1 = 0.8, r2 = 0.9;
    std::vector<Pt> pts;
    for (int i = 0; i < n; ++i) {
      // a coarse grid makes ties and duplicates; some points lie outside the box, one is not a number
      double a = std::floor(uniform() * 12) / 10.0, b = std::floor(uniform() * 12) / 10.0;
      if (trial % 7 == 3 && i == n / 2) a = NAN;
      pts.push_back(Pt(a, b));
    }
    std::vector<double> u(n + 1), c(n + 1);  // exactly F + 1 slots at every step: the sanitizer sees one more
    uint64_t F = 0;
    for (int i = 0; i < n; ++i) {
      F = front_insert(u.data(), c.data(), F, pts[i].first, pts[i].second, r1, r2);
      if (F > (uint64_t)i + 1) return std::printf("trial %d: F = %llu after %d points\n", trial, (unsigned long long)F, i + 1), 1;
    }
    std::vector<Pt> clean;
    for (const Pt &p : pts)
      if (p.first == p.first) clean.push_back(p);
    const std::vector<Pt> want = brute(clean, r1, r2);
    if (want.size() != F) return std::printf("trial %d: %llu points, brute force %zu\n", trial, (unsigned long long)F, want.size()), 1;
    for (uint64_t s = 0; s < F; ++s) {
      if (u[s] != want[s].first || c[s] != want[s].second) return std::printf("trial %d: point %llu differs\n", trial, (unsigned long long)s), 1;
      if (s && !(u[s - 1] < u[s] && c[s - 1] > c[s])) return std::printf("trial %d: order broken at %llu\n", trial, (unsigned long long)s), 1;
    }
    ++cases;
  }
  {  // the capacity: 2048 undominated points, then one that knocks all of them out
    const uint64_t cap = obhip::kMacqFrontCap;
    std::vector<double> u(cap + 1), c(cap + 1);
    uint64_t F = 0;
    for (uint64_t i = 0; i < cap; ++i) {
      const uint64_t l = (i * 7919) % cap;  // in no particular order
      F = front_insert(u.data(), c.data(), F, (double)l, (double)(cap - l), 1e9, 1e9);
    }
    if (F != cap) return std::printf("capacity: F = %llu\n", (unsigned long long)F), 1;
    for (uint64_t s = 1; s < F; ++s)
      if (!(u[s - 1] < u[s] && c[s - 1] > c[s])) return std::printf("capacity: order broken\n"), 1;
    F = front_insert(u.data(), c.data(), F, -1.0, -1.0, 1e9, 1e9);
    if (F != 1 || u[0] != -1.0 || c[0] != -1.0) return std::printf("capacity: the dominating point left F = %llu\n", (unsigned long long)F), 1;
    ++cases;
  }
  std::printf("ok %d\n", cases);
  return 0;
}
