// launch_plan_san.cpp -- the launch planner (csrc/brotli_launch_plan.h) under AddressSanitizer and UBSan, as a program of its own:
//   g++ -std=c++17 -fsanitize=address,undefined -I rust-brotli-decompressor_amd/csrc tests/tools/launch_plan_san.cpp
// Sweeps batch sizes, stream sizes, probe answers, knobs and device descriptions (a device without an engine, with little LDS, with an
// explicit arena and grid) through plan_launch and plan_later_pass, the size arrays in heap blocks of exactly their size, and holds every
// plan to what a launch needs: blocks to launch, a wave count the kernel has, an arena a block can hold.  Exits 0 when every plan did.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "brotli_launch_plan.h"

using namespace brotli_amd_plan;

int main() {
  BrotliAmdPlanDevice base = {};
  // (an MI355X as BrotliAmdBatchCreate describes it)
  base.cus = 256; base.lds_per_cu = 163840; base.block_max = 65536; base.lds_fixed = 6160; base.lds_helper4 = 5376; base.lds_helper8 = 10752;
  base.lds_helper16 = 121104; base.lds_arena = 25328; base.max_arena = 54000; base.grid_max = 1024; base.retry_grid_max = 512; base.auto_arena = 1;
  base.engine_ok = 1;
  std::vector<BrotliAmdPlanDevice> devices(5, base);
  devices[1].engine_ok = 0;
  devices[2].lds_per_cu = 65536; devices[2].engine_ok = 0; devices[2].grid_max = 256; devices[2].retry_grid_max = 256;
  devices[3].auto_arena = 0; devices[3].lds_arena = 16384; devices[3].grid_max = 2304;
  devices[4].grid_max = 300; devices[4].cus = 120;
  BrotliAmdPlanKnobs knobs0 = {};
  knobs0.max_blocks_per_cu = 14; knobs0.min_small_arena = 3584; knobs0.engine_queue_max = 4; knobs0.gang = -1; knobs0.pool = -1;
  unsigned long long plans = 0;
  uint64_t seed = 88172645463325252ull;
  const auto rnd = [&seed]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
  for (const BrotliAmdPlanDevice& d : devices) {
    for (int variant = 0; variant < 6; variant++) {
      BrotliAmdPlanKnobs k = knobs0;
      if (variant == 1) k.gang = 0;
      if (variant == 2) { k.gang = 16; k.no_order = 1; }
      if (variant == 3) k.pool = 2;
      if (variant == 4) { k.no_engine_queue = 1; k.no_record_blocks = 1; }
      if (variant == 5) { k.engine_queue_max = 8; k.max_blocks_per_cu = 16; }
      for (uint32_t n : {1u, 2u, 7u, 8u, 9u, 33u, 65u, 128u, 129u, 255u, 256u, 257u, 384u, 600u, 1024u, 1025u, 2048u, 4096u, 5000u}) {
        for (int mix = 0; mix < 4; mix++) {
          size_t* sizes = static_cast<size_t*>(std::malloc(sizeof(size_t) * n));   // (exactly n entries)
          uint8_t* kinds = static_cast<uint8_t*>(std::malloc(n));
          for (uint32_t i = 0; i < n; i++) {
            sizes[i] = mix == 0 ? 400000 : mix == 1 ? 2000 + rnd() % 3000 : mix == 2 ? (i == 0 ? (size_t)64 << 20 : 100000) : rnd() % ((size_t)8 << 20);
            kinds[i] = mix == 0 ? 7 : (uint8_t)(rnd() % 16);
          }
          const auto size_at = [sizes](uint32_t i) { return (uint64_t)sizes[i]; };
          for (uint32_t cap : {4u, 8u, k.max_blocks_per_cu}) {
            BrotliAmdLaunchPlan p = plan_launch(d, k, cap, n, size_at, nullptr);
            if (p.want_probe) {
              const BrotliAmdLaunchPlan probe = p;
              p = plan_launch(d, k, cap, n, size_at, kinds);
              if (p.want_probe || probe.grid <= d.cus) { std::fprintf(stderr, "probe: n %u\n", n); return 1; }
            }
            plans++;
            const bool ok = p.grid >= 1u && (p.waves == 1u || p.waves == 4u || p.waves == 8u || p.waves == 16u) &&
                            (p.gang != 0u || p.grid <= n) && p.arena != 0u && d.lds_fixed + p.arena <= d.lds_per_cu &&
                            (p.waves != 1u || (uint64_t)(d.lds_fixed + p.arena) * p.cur_per_cu <= d.lds_per_cu) &&
                            (p.gang == 0u || (p.waves == 16u && n <= d.cus)) && (!p.engine_queue || p.waves == 16u) && (p.ordered != 0u) == (n > p.grid && !k.no_order);
            if (!ok) {
              std::fprintf(stderr, "n %u mix %d variant %d: grid %u waves %u arena %u per_cu %u gang %u\n", n, mix, variant, p.grid, p.waves, p.arena, p.cur_per_cu, p.gang);
              return 1;
            }
            // the passes behind it: every chain of levels ends in the last pass
            uint32_t level = p.cur_per_cu, arena = p.arena;
            bool last = false;
            for (int pass = 0; pass < 4 && !last; pass++) {
              const BrotliAmdLaterPass l = plan_later_pass(d, k, cap, level, arena, 1u + (uint32_t)(rnd() % n), pass == 0 && p.engine_queue);
              if (l.grid_max == 0u || (l.waves != 1u && l.waves != 4u)) { std::fprintf(stderr, "later pass: n %u level %u\n", n, level); return 1; }
              level = l.level; last = l.last != 0u;
              plans++;
            }
            if (!last) { std::fprintf(stderr, "no last pass: n %u\n", n); return 1; }
          }
          std::free(sizes); std::free(kinds);
        }
      }
    }
  }
  std::printf("%llu plans\n", plans);
  return 0;
}
