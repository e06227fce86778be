// Host program for tests/test_glm_host.py: one row of the GLM row pass per input line, by the functions
// the kernels call (outerbase_amd/csrc/glm_row.h).
//   in:  family eta y a e2        (hexadecimal floating point)
//   out: mu sw u al mag finite
#include <cstdio>

#include "../outerbase_amd/csrc/glm_row.h"

int main() {
  int family;
  double eta, y, a, e2;
  while (std::scanf("%d %la %la %la %la", &family, &eta, &y, &a, &e2) == 5) {
    obhip::GlmRow r;
    if (family == OBHIP_GLM_GAUSSIAN) r = obhip::glm_row<OBHIP_GLM_GAUSSIAN>(eta, y, a, e2);
    else if (family == OBHIP_GLM_BINOMIAL) r = obhip::glm_row<OBHIP_GLM_BINOMIAL>(eta, y, a, e2);
    else if (family == OBHIP_GLM_POISSON) r = obhip::glm_row<OBHIP_GLM_POISSON>(eta, y, a, e2);
    else return 2;
    std::printf("%a %a %a %a %a %d\n", r.mu, r.sw, r.u, r.al, r.mag, r.finite ? 1 : 0);
  }
  return 0;
}
