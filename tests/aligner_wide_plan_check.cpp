// Stand-alone check of the wide pass's launch planning (hip/aligner_plan:
// aln_plan_wave_launches, aln_wave_single_slide), meant to be built with
// -fsanitize=address,undefined (test_aligner_wide_plan.py does). Every planned
// alignment's first and last step are written into arenas of exactly the
// planned capacity, as the wave kernel's stores would.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "hip/aligner_plan.hpp"

using namespace rga::hip;

namespace {

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

uint32_t lcg(uint32_t* state) {
  *state = *state * 1664525u + 1013904223u;
  return *state >> 8;
}

AlnDesc desc_of(uint32_t q_len, uint32_t t_len) {
  AlnDesc d{};
  d.q_len = q_len;
  d.t_len = t_len;
  return d;
}

AlnArenaCaps caps_for_steps(uint64_t steps) {
  return {0, steps * kAlnWaveTbPerStep, steps * kAlnWaveSPerStep};
}

// The band rule itself, one division per column: what aln_wave_single_slide
// must agree with.
bool single_slide_by_walk(uint32_t n, uint32_t m) {
  const uint64_t step = (static_cast<uint64_t>(n) << 32) / m;
  const int64_t nbt = (n + 63) / 64;
  const int64_t hi = nbt > 64 ? nbt - 64 : 0;
  int64_t prev = 0;
  for (uint64_t j = 1; j <= m; ++j) {
    int64_t top = static_cast<int64_t>(((j * step) >> 32) >> 6) - 32;
    top = top < 0 ? 0 : (top > hi ? hi : top);
    if (top - prev > 1) return false;
    prev = top;
  }
  return true;
}

struct PassCounts {
  size_t launches, never_run, refused;
};

// Plans a pass over descs in the given order and checks every property of
// the plan against arenas of exactly `caps`.
PassCounts check_pass(const std::vector<AlnDesc>& descs, const std::vector<uint32_t>& order,
                      const AlnArenaCaps& caps) {
  const uint32_t count = static_cast<uint32_t>(order.size());
  const AlnWavePlan plan = aln_plan_wave_launches(descs.data(), order.data(), count, caps);
  std::vector<uint64_t> tb(caps.tb_u64);
  std::vector<int32_t> sbuf(caps.s_i32);
  std::vector<int> seen(descs.size(), 0);
  uint32_t next_pos = 0, next_desc = 0;
  for (const AlnSubLaunch& l : plan.launches) {
    CHECK(l.num_waves > 0 && l.num_align == l.num_waves);
    CHECK(l.first_wave >= next_pos);
    CHECK(l.desc_off == next_desc);
    CHECK(l.first_wave + l.num_waves <= count);
    uint64_t tb_end = 0, s_end = 0;
    for (uint32_t w = 0; w < l.num_waves; ++w) {
      const AlnWaveDesc& wd = plan.waves[l.desc_off + w];
      const AlnDesc& d = descs[order[l.first_wave + w]];
      CHECK(aln_wave_single_slide(d.q_len, d.t_len));
      const uint64_t steps = aln_wave_steps(d.q_len, d.t_len);
      // offsets never overlap: each region starts where the one before ended
      CHECK(wd.tb_off == tb_end && wd.s_off == s_end);
      tb_end = wd.tb_off + steps * kAlnWaveTbPerStep;
      s_end = wd.s_off + steps * kAlnWaveSPerStep;
      CHECK(tb_end <= caps.tb_u64 && s_end <= caps.s_i32);
      // the kernel's last store: step t_len + btop(t_len) + 63, lane 63
      const uint64_t nbt = (d.q_len + 63) / 64;
      const uint64_t last = d.t_len + (nbt > 64 ? nbt - 64 : 0) + 63;
      CHECK(last < steps);
      tb[wd.tb_off] = 1;
      tb[wd.tb_off + last * kAlnWaveTbPerStep + 2 * 63 + 1] = 1;
      sbuf[wd.s_off] = 1;
      sbuf[wd.s_off + last * kAlnWaveSPerStep + 63] = 1;
      ++seen[order[l.first_wave + w]];
    }
    // greedy: the launch ends at the end of the pass, at an alignment without
    // a descriptor, or where the next one no longer fits
    const uint32_t after = l.first_wave + l.num_waves;
    if (after < count) {
      const AlnDesc& d = descs[order[after]];
      const uint64_t steps = aln_wave_steps(d.q_len, d.t_len);
      const bool alone = steps * kAlnWaveTbPerStep <= caps.tb_u64 &&
                         steps * kAlnWaveSPerStep <= caps.s_i32;
      CHECK(!alone || !aln_wave_single_slide(d.q_len, d.t_len) ||
            tb_end + steps * kAlnWaveTbPerStep > caps.tb_u64 ||
            s_end + steps * kAlnWaveSPerStep > caps.s_i32);
    }
    next_pos = after;
    next_desc = l.desc_off + l.num_waves;
  }
  CHECK(next_desc == plan.waves.size());
  for (uint32_t i : plan.never_run) {
    const uint64_t steps = aln_wave_steps(descs[i].q_len, descs[i].t_len);
    CHECK(steps * kAlnWaveTbPerStep > caps.tb_u64 || steps * kAlnWaveSPerStep > caps.s_i32);
    ++seen[i];
  }
  for (uint32_t i : plan.refused) {
    CHECK(!aln_wave_single_slide(descs[i].q_len, descs[i].t_len));
    ++seen[i];
  }
  // every alignment of the pass exactly once: launched, never_run or refused
  std::vector<int> want(descs.size(), 0);
  for (uint32_t i : order) ++want[i];
  CHECK(seen == want);
  return {plan.launches.size(), plan.never_run.size(), plan.refused.size()};
}

}  // namespace

int main() {
  // ---- the single-slide rule against a walk of the band rule ----
  CHECK(aln_wave_single_slide(1, 1));
  CHECK(aln_wave_single_slide(4096, 1));      // fits the band: nothing slides
  CHECK(aln_wave_single_slide(64 * 100, 100));  // one block per column exactly
  CHECK(!aln_wave_single_slide(4200, 1));     // 0 -> 2 in one column
  // one slide, but at column 1: admitted, and the kernel recycles lane 0
  // before its first step
  CHECK(aln_wave_single_slide(4097, 1));
  CHECK(aln_wave_single_slide(4160, 1));
  CHECK(!aln_wave_single_slide(4161, 1));
  CHECK(aln_wave_single_slide(4224, 2));
  CHECK(!aln_wave_single_slide(9000, 100));
  CHECK(!aln_wave_single_slide(262144, 8));
  CHECK(!aln_wave_single_slide(5, 0));
  {
    uint32_t seed = 7;
    for (int k = 0; k < 2000; ++k) {
      const uint32_t m = 1 + lcg(&seed) % 300;
      const uint32_t n = 1 + lcg(&seed) % (m * 100);
      CHECK(aln_wave_single_slide(n, m) == single_slide_by_walk(n, m));
    }
  }

  // ---- an empty pass ----
  {
    std::vector<AlnDesc> descs;
    const PassCounts c = check_pass(descs, {}, caps_for_steps(1000));
    CHECK(c.launches == 0 && c.never_run == 0 && c.refused == 0);
  }

  // ---- fits exactly / exceeds by one step ----
  {
    const std::vector<AlnDesc> descs = {desc_of(5000, 4000)};
    const uint64_t steps = aln_wave_steps(5000, 4000);
    CHECK(steps == 4000 + 64 + 79 + 1);
    PassCounts c = check_pass(descs, {0}, caps_for_steps(steps));
    CHECK(c.launches == 1 && c.never_run == 0);
    c = check_pass(descs, {0}, caps_for_steps(steps - 1));
    CHECK(c.launches == 0 && c.never_run == 1);
    // each arena on its own decides
    AlnArenaCaps caps = caps_for_steps(steps);
    caps.s_i32 -= 1;
    c = check_pass(descs, {0}, caps);
    CHECK(c.launches == 0 && c.never_run == 1);
    caps = caps_for_steps(steps);
    caps.tb_u64 -= 1;
    c = check_pass(descs, {0}, caps);
    CHECK(c.launches == 0 && c.never_run == 1);
  }

  // ---- sub-launch cuts at the arena boundary ----
  {
    // four equal alignments, arenas of exactly two of them: two launches of
    // two; one step fewer: the second of each pair no longer fits
    const std::vector<AlnDesc> descs(4, desc_of(3000, 3000));
    const uint64_t steps = aln_wave_steps(3000, 3000);
    PassCounts c = check_pass(descs, {0, 1, 2, 3}, caps_for_steps(2 * steps));
    CHECK(c.launches == 2 && c.never_run == 0);
    c = check_pass(descs, {0, 1, 2, 3}, caps_for_steps(2 * steps - 1));
    CHECK(c.launches == 4 && c.never_run == 0);
    c = check_pass(descs, {0, 1, 2, 3}, caps_for_steps(4 * steps));
    CHECK(c.launches == 1);
  }

  // ---- the tiny-target pairs are planned like any other ----
  {
    const std::vector<AlnDesc> descs = {desc_of(4097, 1), desc_of(4160, 1), desc_of(4224, 2)};
    const PassCounts c = check_pass(descs, {0, 1, 2}, caps_for_steps(1000));
    CHECK(c.launches == 1 && c.never_run == 0 && c.refused == 0);
  }

  // ---- never_run and refused in the middle of a pass end the launch ----
  {
    const std::vector<AlnDesc> descs = {desc_of(100, 100), desc_of(100000, 90000),
                                        desc_of(200, 100), desc_of(9000, 100),
                                        desc_of(300, 100)};
    const PassCounts c = check_pass(descs, {0, 1, 2, 3, 4}, caps_for_steps(5000));
    CHECK(c.never_run == 1 && c.refused == 1 && c.launches == 3);
  }

  // ---- random passes over subsets, in launch order ----
  {
    uint32_t seed = 99;
    for (int round = 0; round < 50; ++round) {
      const uint32_t count = 1 + lcg(&seed) % 200;
      std::vector<AlnDesc> descs(count);
      for (auto& d : descs) {
        d = desc_of(1 + lcg(&seed) % 20000, 1 + lcg(&seed) % 20000);
        if (lcg(&seed) % 16 == 0) d.t_len = 1 + d.t_len % 64;  // steep: may be refused
      }
      std::vector<uint32_t> subset;
      for (uint32_t i = 0; i < count; ++i) {
        if (lcg(&seed) % 3 != 0) subset.push_back(i);
      }
      aln_sort_for_launch(descs.data(), &subset);
      check_pass(descs, subset, caps_for_steps(1000 + lcg(&seed) % 60000));
    }
  }
  printf("aligner wide plan OK\n");
  return 0;
}
