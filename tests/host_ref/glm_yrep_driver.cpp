// Driver of tests/test_glm_yrep.py: the outcome sampler of include/ahmc_glm_yrep.h (csrc/ahmc_glm_yrep_draw.hpp, the text the kernel
// k_glm_yrep compiles) as a stand-alone CPU program, built by the test itself with the host compiler (-ffp-contract=off: nothing is fused
// but the fma the sampler names) — and what a host sanitizer build (-fsanitize=address,undefined) is pointed at.  The block generator is
// the host form of ahmc_device.hpp's philox4x32_10 and u53, which are device functions.
//
//   glm_yrep_driver FAMILY N_CATEGORIES N SEED ONES IN OUT
// IN:  q (planes, N) double, the plane index fastest; aux (N) double; row (N) uint32; col (N) uint32.
// OUT: y (N) double; blocks (N) int32, the 4-word blocks every element took.  ONES = 1: every uniform is 1 (the loops' worst case).
//   glm_yrep_driver check FAMILY N_CATEGORIES N HAS_Q HAS_AUX HAS_Y
// prints what ahmc_glm_yrep_at refuses (yrep_at_refusal).
#include "ahmc_glm_yrep_draw.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace {

struct Philox4 {
  uint32_t v[4];
};

Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0;
    c1 = (uint32_t)p1;
    c2 = n2;
    c3 = (uint32_t)p0;
    k0 += W0;
    k1 += W1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

double u53(uint32_t hi, uint32_t lo) {
  const uint64_t bits = ((uint64_t)(hi >> 5) << 26) | (uint64_t)(lo >> 6);
  return ((double)bits + 0.5) * (1.0 / 9007199254740992.0);
}

struct Gen {
  uint32_t k0, k1, row, col, slot;
  bool ones;
  void next(double& u, double& u2) {
    const Philox4 p = philox4x32_10(row, col, ahmc::YREP_PURPOSE, slot, k0, k1);
    ++slot;
    u = ones ? 1.0 : u53(p.v[0], p.v[1]);
    u2 = ones ? 1.0 : u53(p.v[2], p.v[3]);
  }
};

struct Planes {
  const double* q;
  double operator()(int c) const { return q[c]; }
};

template <int FAM>
void run(int C, int64_t n, int planes, const double* q, const double* aux, const uint32_t* row, const uint32_t* col, uint64_t seed, bool ones, double* y,
         int32_t* blocks) {
  for (int64_t e = 0; e < n; ++e) {
    Gen gen{(uint32_t)seed, (uint32_t)(seed >> 32), row[e], col[e], 0u, ones};
    y[e] = ahmc::yrep_draw<FAM>(Planes{q + (int64_t)planes * e}, aux[e], C, gen);
    blocks[e] = (int32_t)gen.slot;
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 8 && std::string(argv[1]) == "check") {
    printf("%d\n", ahmc::yrep_at_refusal(atoi(argv[2]), atoi(argv[3]), atoll(argv[4]), atoi(argv[5]) != 0, atoi(argv[6]) != 0, atoi(argv[7]) != 0));
    return 0;
  }
  if (argc != 8) {
    fprintf(stderr, "usage: glm_yrep_driver FAMILY N_CATEGORIES N SEED ONES IN OUT\n");
    return 2;
  }
  const int family = atoi(argv[1]), C = atoi(argv[2]);
  const int64_t n = atoll(argv[3]);
  const uint64_t seed = strtoull(argv[4], nullptr, 10);
  const bool ones = atoi(argv[5]) != 0;
  const int sampler = ahmc::yrep_sampler_of(family);
  if (sampler < 0 || n < 0 || (family >= 5 && (C < 2 || C > 16))) return 2;
  const int planes = ahmc::yrep_planes_of(family, C);
  std::vector<double> q((size_t)planes * n), aux((size_t)n), y((size_t)n);
  std::vector<uint32_t> row((size_t)n), col((size_t)n);
  std::vector<int32_t> blocks((size_t)n);
  FILE* f = fopen(argv[6], "rb");
  if (!f) return 3;
  const bool read_ok = fread(q.data(), 8, q.size(), f) == q.size() && fread(aux.data(), 8, aux.size(), f) == aux.size() &&
                       fread(row.data(), 4, row.size(), f) == row.size() && fread(col.data(), 4, col.size(), f) == col.size();
  fclose(f);
  if (!read_ok) return 3;
  switch (sampler) {
    case 0: run<0>(C, n, planes, q.data(), aux.data(), row.data(), col.data(), seed, ones, y.data(), blocks.data()); break;
    case 1: run<1>(C, n, planes, q.data(), aux.data(), row.data(), col.data(), seed, ones, y.data(), blocks.data()); break;
    case 2: run<2>(C, n, planes, q.data(), aux.data(), row.data(), col.data(), seed, ones, y.data(), blocks.data()); break;
    case 4: run<4>(C, n, planes, q.data(), aux.data(), row.data(), col.data(), seed, ones, y.data(), blocks.data()); break;
    default: run<5>(C, n, planes, q.data(), aux.data(), row.data(), col.data(), seed, ones, y.data(), blocks.data()); break;
  }
  f = fopen(argv[7], "wb");
  if (!f) return 4;
  const bool write_ok = fwrite(y.data(), 8, y.size(), f) == y.size() && fwrite(blocks.data(), 4, blocks.size(), f) == blocks.size();
  fclose(f);
  return write_ok ? 0 : 4;
}
