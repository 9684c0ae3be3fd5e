// Hashes of what the HOST builders (pbrlab_amd/csrc/bvh_build.cpp: build_bvh + build_qlayout) make of a few seeded soups: the Q tree's
// nodes, triangle leaves, curve records, hit codes and stack need.  tests/test_qcollapse_model_cpu.py compares them with the hashes
// recorded before the quantiser moved into the header the device collapse shares (tests/golden/qlayout_hashes.txt): host-built
// trees stay byte-identical.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "host_scene.h"

static uint64_t rng_state;
static float rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (float)((rng_state >> 40) & 0xFFFFFF) / 16777216.0f;
}
static uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

// shape 0: unit cube, 1: around 1e6 (step-growth retries), 2: flat in z, 3: sixty decades
static void soup(const char* name, uint32_t n, float curve_share, int shape, uint64_t seed) {
  rng_state = seed;
  std::vector<float> lo(3 * (size_t)n), hi(3 * (size_t)n);
  std::vector<uint8_t> kinds(n);
  for (uint32_t g = 0; g < n; g++) {
    kinds[g] = rnd() < curve_share ? 1 : 0;
    for (int a = 0; a < 3; a++) {
      float c = rnd(), h = rnd() * 0.02f;
      if (shape == 1) c = c * 0.5f + 1e6f, h = h * 0.5f + 0.001f;
      if (shape == 2 && a == 2) c = 0.5f, h = 0.f;
      if (shape == 3) c = powf(10.f, c * 60.f - 30.f), h = c * 0.125f;
      lo[3 * g + a] = c - h, hi[3 * g + a] = c + h;
    }
  }
  pb::FlatBvh bvh;
  pb::build_bvh(lo, hi, kinds, &bvh);
  std::vector<float4> slots(4 * (size_t)n);
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t g = bvh.slot_gid[k];
    float4* sl = &slots[4 * (size_t)k];
    const uint32_t route = (g * 2654435761u) & 0x78000000u;
    if (!kinds[g]) {
      sl[0] = make_float4(lo[3 * g], lo[3 * g + 1], lo[3 * g + 2], 0.f);
      sl[1] = make_float4(hi[3 * g], lo[3 * g + 1], hi[3 * g + 2], 0.f);
      sl[2] = make_float4(hi[3 * g], hi[3 * g + 1], hi[3 * g + 2], 0.f);
      sl[3] = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      const uint32_t sub = g & 3u;
      float fs;
      memcpy(&fs, &sub, 4);
      sl[0] = make_float4(lo[3 * g], lo[3 * g + 1], lo[3 * g + 2], 0.001f);
      sl[1] = make_float4(hi[3 * g], hi[3 * g + 1], hi[3 * g + 2], 0.001f);
      sl[2] = make_float4(fs, 0.f, 0.f, 0.f);
      sl[3] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    memcpy(&sl[2].w, &route, 4);
  }
  pb::QLayout q;
  pb::build_qlayout(bvh, slots, kinds, &q);
  uint64_t h = 14695981039346656037ull;
  h = fnv(h, q.nodes.data(), q.nodes.size() * sizeof(pb::QNode));
  h = fnv(h, q.tri.data(), q.tri.size() * 16);
  h = fnv(h, q.pts.data(), q.pts.size() * 16);
  h = fnv(h, q.hit.data(), q.hit.size() * 4);
  h = fnv(h, &q.stack_need, 4);
  printf("%s %zu %zu %zu %u %016llx\n", name, q.nodes.size(), q.tri.size(), q.pts.size(), q.stack_need, (unsigned long long)h);
}

int main() {
  soup("triangles_2000", 2000, 0.f, 0, 1);
  soup("mixed_1500", 1500, 0.4f, 0, 2);
  soup("curves_700", 700, 1.f, 0, 3);
  soup("shifted_1e6_800", 800, 0.f, 1, 4);
  soup("flat_z_600", 600, 0.2f, 2, 5);
  soup("decades_500", 500, 0.f, 3, 6);
  soup("one", 1, 0.f, 0, 7);
  soup("three", 3, 0.5f, 0, 8);
  return 0;
}
