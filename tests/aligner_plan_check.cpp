// Stand-alone check of the HIP aligner's launch planning (hip/aligner_plan),
// meant to be built with -fsanitize=address,undefined (test_aligner_plan.py
// does): synthetic descriptors through the sort and the sub-launch splitter,
// for both sbuf strides, then every wave's first and last per-column word is
// written into arenas of exactly the planned capacity, as the kernel's
// stores would.
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

std::vector<AlnDesc> make_descs(uint32_t count, uint32_t max_len, uint32_t seed) {
  std::vector<AlnDesc> descs(count);
  for (auto& d : descs) {
    d = AlnDesc{};
    d.q_len = 1 + lcg(&seed) % max_len;
    d.t_len = 1 + lcg(&seed) % max_len;
  }
  return descs;
}

// Plans one pass over `subset` and checks it; returns the number of
// sub-launches.
size_t check_pass(const std::vector<AlnDesc>& descs, std::vector<uint32_t> subset,
                  uint32_t lanes, uint32_t K, bool adaptive, const AlnArenaCaps& caps,
                  size_t* never_run_count) {
  const uint32_t stride = aln_s_stride(K, adaptive);
  const uint32_t count = static_cast<uint32_t>(subset.size());
  aln_sort_for_launch(descs.data(), &subset);
  for (size_t i = 1; i < subset.size(); ++i) {
    CHECK(descs[subset[i - 1]].t_len >= descs[subset[i]].t_len);
  }
  const AlnLaunchPlan plan =
      aln_plan_launches(descs.data(), subset.data(), count, lanes, K, stride, caps);

  std::vector<uint64_t> peq(caps.peq_u64), tb(caps.tb_u64);
  std::vector<int32_t> sbuf(caps.s_i32);
  std::vector<int> seen(descs.size(), 0);
  const uint32_t waves_total = (count + lanes - 1) / lanes;
  CHECK(plan.waves.size() <= waves_total);
  uint32_t next_wave = 0, next_desc = 0;
  for (const AlnSubLaunch& l : plan.launches) {
    CHECK(l.num_waves > 0);
    CHECK(l.first_wave >= next_wave);
    CHECK(l.desc_off == next_desc);
    CHECK(static_cast<uint64_t>(l.first_wave) * lanes + l.num_align <= count);
    CHECK(l.num_align > (l.num_waves - 1) * lanes && l.num_align <= l.num_waves * lanes);
    uint64_t peq_end = 0, tb_end = 0, s_end = 0;
    for (uint32_t w = 0; w < l.num_waves; ++w) {
      const AlnWaveDesc& wd = plan.waves[l.desc_off + w];
      CHECK(wd.peq_off == peq_end && wd.tb_off == tb_end && wd.s_off == s_end);
      CHECK(wd.nb >= K);
      for (uint32_t lane = 0; lane < lanes; ++lane) {
        const uint64_t slot = static_cast<uint64_t>(l.first_wave + w) * lanes + lane;
        if (slot >= static_cast<uint64_t>(l.first_wave) * lanes + l.num_align) break;
        const AlnDesc& d = descs[subset[slot]];
        CHECK(d.t_len <= wd.mmax);
        CHECK((d.q_len + 63) / 64 <= wd.nb);
        ++seen[subset[slot]];
      }
      // the kernel's extreme stores: lane 63, last column, last word
      peq[wd.peq_off] = 1;
      peq[wd.peq_off + (static_cast<uint64_t>(wd.nb - 1) * 4 + 3) * 64 + 63] = 1;
      tb[wd.tb_off] = 1;
      tb[wd.tb_off + ((static_cast<uint64_t>(wd.mmax) * K + (K - 1)) * 2 + 1) * 64 + 63] = 1;
      sbuf[wd.s_off] = 1;
      sbuf[wd.s_off + (static_cast<uint64_t>(wd.mmax) * stride + (stride - 1)) * 64 + 63] = 1;
      peq_end += static_cast<uint64_t>(wd.nb) * 4 * 64;
      tb_end += (static_cast<uint64_t>(wd.mmax) + 1) * K * 2 * 64;
      s_end += (static_cast<uint64_t>(wd.mmax) + 1) * stride * 64;
    }
    CHECK(peq_end <= caps.peq_u64 && tb_end <= caps.tb_u64 && s_end <= caps.s_i32);
    next_wave = l.first_wave + l.num_waves;
    next_desc += l.num_waves;
  }
  CHECK(next_desc == plan.waves.size());
  for (uint32_t idx : plan.never_run) {
    ++seen[idx];
  }
  std::vector<int> in_subset(descs.size(), 0);
  for (uint32_t idx : subset) {
    ++in_subset[idx];
  }
  for (size_t i = 0; i < descs.size(); ++i) {
    CHECK(seen[i] == in_subset[i]);  // launched or refused, exactly once
  }
  *never_run_count = plan.never_run.size();
  return plan.launches.size();
}

}  // namespace

int main() {
  CHECK(aln_lanes_per_wave(100, 0) == 16);
  CHECK(aln_lanes_per_wave(16384, 0) == 64);
  CHECK(aln_lanes_per_wave(100, 64) == 64);
  CHECK(aln_lanes_per_wave(20000, 32) == 32);
  CHECK(aln_lanes_per_wave(100, 7) == 16);

  size_t multi = 0, refused = 0, passes = 0;
  for (uint32_t K : {4u, 8u, 16u}) {
    for (uint32_t lanes : {16u, 32u, 64u}) {
      for (bool adaptive : {false, true}) {
        const uint32_t count = 150 + 13 * K + lanes;  // partial last wave
        std::vector<AlnDesc> descs = make_descs(count, 400, 77 * K + lanes);
        descs[count / 2].t_len = 5000;  // one wave no arena below can hold
        std::vector<uint32_t> all(count);
        std::iota(all.begin(), all.end(), 0u);
        // room for about three waves of 401 columns: several sub-launches
        AlnArenaCaps caps;
        caps.peq_u64 = 3ull * 8 * 4 * 64 + 64 * 4 * K;
        caps.tb_u64 = 3ull * 401 * K * 2 * 64;
        caps.s_i32 = 3ull * 401 * aln_s_stride(K, true) * 64;
        size_t never = 0;
        multi += check_pass(descs, all, lanes, K, adaptive, caps, &never) > 1;
        CHECK(never >= 1 && never <= lanes);
        refused += never;
        // the retry pass: a sparse subset of the same arena
        std::vector<uint32_t> subset;
        for (uint32_t i = 0; i < count; i += 7) {
          if (i != count / 2) subset.push_back(i);
        }
        check_pass(descs, subset, lanes, K, true, caps, &never);
        CHECK(never == 0);
        // ample arenas (short pairs keep them small): one sub-launch,
        // nothing refused
        const std::vector<AlnDesc> shorts = make_descs(count, 100, 5 * K + lanes);
        const uint64_t waves = (count + lanes - 1) / lanes;
        AlnArenaCaps big{waves * 16 * 4 * 64, waves * 101 * K * 2 * 64,
                         waves * 101 * aln_s_stride(K, true) * 64};
        CHECK(check_pass(shorts, all, lanes, K, adaptive, big, &never) == 1);
        CHECK(never == 0);
        passes += 3;
      }
    }
  }
  // an empty pass plans nothing
  size_t never = 0;
  std::vector<AlnDesc> none;
  CHECK(check_pass(none, {}, 16, 4, true, AlnArenaCaps{1, 1, 1}, &never) == 0);
  CHECK(multi > 0);
  printf("aligner plan OK: %zu passes, %zu with several sub-launches, %zu alignments refused\n",
         passes, multi, refused);
  return 0;
}
