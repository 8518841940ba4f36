// Stand-alone host check of the partner draw for a sanitizer build: calls pcgmix_partner_permutation_i64
// over the layouts of tests/test_partner_draw_lockstep_cpu.py and checks that every group was permuted
// onto itself (the bit-exact comparison with CPython is that test's).  Host code only, no GPU.
//   cd <package>/csrc && mkdir -p /tmp/san &&
//   hipcc -O1 -g -fPIC -std=c++17 --offload-arch=gfx950 -ffp-contract=off -I../../include \
//         -Xarch_host -fsanitize=address,undefined -c pcgmix_host.hip -o /tmp/san/pcgmix_host.o &&
//   hipcc -shared --offload-arch=gfx950 -fsanitize=address,undefined -o /tmp/san/libpcgmix_hip.so \
//         /tmp/san/pcgmix_host.o $(ls *.o | grep -v pcgmix_host.o) &&
//   hipcc -x c++ -O1 -g -std=c++17 -fsanitize=address,undefined ../../profiles/probes/partner_draw_san.cpp \
//         -L/tmp/san -lpcgmix_hip -Wl,-rpath,/tmp/san -o /tmp/san/partner_draw_san && /tmp/san/partner_draw_san
#include <cstdint>
#include <cstdio>
#include <vector>

extern "C" int pcgmix_partner_permutation_i64(const int32_t* group_id, int B, int n_groups, uint64_t seed,
                                              int64_t* mix);

static const uint64_t kSeeds[] = {1, 2, 0xffffffffull, 0x100000000ull, (1ull << 40) + 7};
static int failures = 0, cases = 0;

static void check(const char* what, const std::vector<int32_t>& gid, int n_groups) {
  const int B = (int)gid.size();
  for (uint64_t seed : kSeeds) {
    std::vector<int64_t> mix((size_t)B, -1);
    const int err = pcgmix_partner_permutation_i64(gid.data(), B, n_groups, seed, mix.data());
    std::vector<char> hit((size_t)B, 0);
    bool ok = err == 0;
    for (int b = 0; ok && b < B; ++b) {
      const int64_t m = mix[(size_t)b];
      ok = m >= 0 && m < B && gid[(size_t)m] == gid[(size_t)b] && !hit[(size_t)m];
      if (ok) hit[(size_t)m] = 1;
    }
    ++cases;
    if (!ok) {
      ++failures;
      std::printf("FAILED %s B=%d groups=%d seed=%llu err=%d\n", what, B, n_groups, (unsigned long long)seed, err);
    }
  }
}

int main() {
  uint32_t lcg = 12345u;
  const auto next = [&lcg](uint32_t n) { lcg = lcg * 1664525u + 1013904223u; return (lcg >> 8) % n; };
  for (int B : {1, 2, 3, 63, 64, 65, 255, 256, 257}) {
    std::vector<int32_t> gid((size_t)B, 0);
    check("one class", gid, 1);
    for (int b = 0; b < B; ++b) gid[(size_t)b] = b & 1;
    check("alternating", gid, 2);
    for (int b = 0; b < B; ++b) gid[(size_t)b] = b == B / 2;
    check("one singleton", gid, 2);
    for (int K = 3; K <= 6; ++K) {
      for (int b = 0; b < B; ++b) gid[(size_t)b] = (int32_t)((next(7) ? next((uint32_t)K) : 0u) * 5u % (uint32_t)K);
      check("scrambled", gid, K);                          // (groups may be empty: allowed)
    }
  }
  {
    std::vector<int32_t> gid(1024, 0);
    for (int b = 0; b < 124; ++b) gid[(size_t)(b * 8 + 3)] = 1 + b % 3;
    check("900 of 1024", gid, 4);
  }
  {
    std::vector<int32_t> gid(40000);
    for (auto& g : gid) g = next(10) < 3;
    check("wide pool", gid, 2);
  }
  {
    const int32_t bad[4] = {0, 1, 2, 0};
    int64_t mix[4] = {-1, -1, -1, -1};
    ++cases;
    if (pcgmix_partner_permutation_i64(bad, 4, 2, 1, mix) != 1 || mix[0] != -1) {
      ++failures;
      std::printf("FAILED out-of-range group id accepted\n");
    }
  }
  std::printf("%d cases, %d failed\n", cases, failures);
  return failures ? 1 : 0;
}
