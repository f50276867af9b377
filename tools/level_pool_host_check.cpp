// tools/level_pool_host_check.cpp — the host side of a level pool (what multi_car_racing_amd/levels.py: make_levels and mcr_pool_level run)
// as a stand-alone program for the sanitizers: host code only, no GPU, nothing loaded into an interpreter.  Build and run from the repository root:
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/level_pool_host_check.cpp multi_car_racing_amd/csrc/mcr_host.cpp -o tools/tmp/level_pool_host_check && tools/tmp/level_pool_host_check
// (any C++17 compiler; tools/tmp/ is not tracked).  Exit status 0 and "ok" when every check holds.
#include "../include/mcr.h"
#include <cstdio>
#include <cstring>
#include <vector>

static bool make_levels(int K, int N, uint32_t seed, int direction_mode, int threads, std::vector<uint8_t>& blobs, std::vector<int32_t>& info) {
  std::vector<uint32_t> mt_track((size_t)K * MCR_MT_WORDS), mt_draw((size_t)K * MCR_MT_WORDS);
  for (int j = 0; j < K; ++j) {
    const uint32_t g = seed + (uint32_t)j;                       // (mod 2^32, as levels.py seeds them)
    mcr_mt_seed(&mt_track[(size_t)j * MCR_MT_WORDS], g);
    mcr_mt_seed(&mt_draw[(size_t)j * MCR_MT_WORDS], g + 0x80000000u);
  }
  blobs.assign((size_t)K * mcr_episode_bytes(), 0); info.assign((size_t)K * 12, 0);
  return mcr_episodes_generate(mt_track.data(), mt_draw.data(), K, N, direction_mode, blobs.data(), info.data(), threads) == MCR_OK;
}

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
  const size_t eb = mcr_episode_bytes();
  CHECK(eb % 16 == 0 && eb > 80000);
  std::vector<uint8_t> b5, b5t, b3; std::vector<int32_t> i5, i5t, i3;
  CHECK(make_levels(5, 2, 40, 2, 4, b5, i5));
  CHECK(make_levels(5, 2, 40, 2, 1, b5t, i5t));                  // the thread count changes nothing
  CHECK(make_levels(3, 2, 40, 2, 2, b3, i3));
  CHECK(b5 == b5t && i5 == i5t);
  CHECK(std::memcmp(b5.data(), b3.data(), 3 * eb) == 0 && std::memcmp(i5.data(), i3.data(), 3 * 12 * sizeof(int32_t)) == 0);
  for (int j = 0; j < 5; ++j) {
    int32_t T = 0, P = 0, cw = -1;
    CHECK(mcr_episode_unpack(b5.data() + (size_t)j * eb, &T, &P, &cw, nullptr, nullptr, nullptr, nullptr, nullptr) == MCR_OK);
    CHECK(T == i5[(size_t)j * 12] && P == i5[(size_t)j * 12 + 1] && cw == i5[(size_t)j * 12 + 3] && T > 100 && T <= MCR_TILE_CAP && P <= MCR_QUAD_CAP);
    std::vector<double> xyb((size_t)T * 3); std::vector<float> quads((size_t)P * 8); std::vector<uint32_t> meta(P); double spawn[8 * 3];
    CHECK(mcr_episode_unpack(b5.data() + (size_t)j * eb, nullptr, nullptr, nullptr, xyb.data(), quads.data(), meta.data(), spawn, nullptr) == MCR_OK);
  }
  std::vector<uint8_t> w; std::vector<int32_t> wi;
  CHECK(make_levels(2, 8, 0xffffffffu, 1, 2, w, wi));           // the seeds wrap; eight cars; a fixed direction
  CHECK(wi[3] == 1 && wi[12 + 3] == 1);
  // the level function: range, purity, the cycle, K = 1, errors, extreme arguments
  for (uint64_t seed : {0ull, 7ull, 0x8000000000000005ull, ~0ull})
    for (uint32_t g : {0u, 1u, 4095u, 0xffffffffu})
      for (uint32_t k : {0u, 1u, 77u, 0xffffffffu})
        for (int32_t K : {1, 2, 3, 256, 0x7fffffff}) {
          const int32_t a = mcr_pool_level(seed, g, k, K, 0), c = mcr_pool_level(seed, g, k, K, 1);
          CHECK(a >= 0 && a < K && a == mcr_pool_level(seed, g, k, K, 0));
          CHECK(c == (int32_t)(((uint64_t)g + k) % (uint64_t)K));
          if (K == 1) CHECK(a == 0 && c == 0);
        }
  CHECK(mcr_pool_level(0, 0, 0, 0, 0) == MCR_ERR_ARG && mcr_pool_level(0, 0, 0, -5, 1) == MCR_ERR_ARG && mcr_pool_level(0, 0, 0, 3, 2) == MCR_ERR_ARG);
  std::printf("ok\n");
  return 0;
}
