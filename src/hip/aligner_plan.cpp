#include "hip/aligner_plan.hpp"

#include <algorithm>

namespace rga::hip {

namespace {
constexpr uint32_t kLanes = 64;

struct WaveNeeds {
  uint64_t peq, tb, s;
  uint32_t nb, mmax;
};

// Per-column state of wave w: every lane of the wave gets the wave's longest
// target and widest query, whatever its own.
WaveNeeds wave_needs(const AlnDesc* descs, const uint32_t* order, uint32_t count, uint32_t lanes,
                     uint32_t band_k, uint32_t s_stride, uint32_t w) {
  uint32_t nb = band_k, mmax = 0;
  for (uint32_t l = 0; l < lanes; ++l) {
    const uint64_t slot = static_cast<uint64_t>(w) * lanes + l;
    if (slot >= count) break;
    const AlnDesc& d = descs[order[slot]];
    nb = std::max(nb, (d.q_len + 63) / 64);
    mmax = std::max(mmax, d.t_len);
  }
  WaveNeeds n;
  n.peq = static_cast<uint64_t>(nb) * 4 * kLanes;
  n.tb = (static_cast<uint64_t>(mmax) + 1) * band_k * 2 * kLanes;
  n.s = (static_cast<uint64_t>(mmax) + 1) * s_stride * kLanes;
  n.nb = nb;
  n.mmax = mmax;
  return n;
}
}  // namespace

uint32_t aln_lanes_per_wave(uint32_t count, long lanes_override) {
  // Full 64-lane packing for big jobs; small jobs still under-fill waves so
  // every CU gets interleavable work. (The 32-lane middle tier predated the
  // back-to-back sub-launch pipeline; measured post-pipeline, 64 wins at
  // the flagship size: 6.00 vs 5.89 Mbp/s.)
  uint32_t lanes = kLanes;
  if (count < 16384) {
    lanes = 16;
  }
  if (lanes_override == 16 || lanes_override == 32 || lanes_override == 64) {
    lanes = static_cast<uint32_t>(lanes_override);
  }
  return lanes;
}

void aln_sort_for_launch(const AlnDesc* descs, std::vector<uint32_t>* order) {
  std::sort(order->begin(), order->end(), [&](uint32_t x, uint32_t y) {
    if (descs[x].t_len != descs[y].t_len) return descs[x].t_len > descs[y].t_len;
    return x < y;
  });
}

AlnLaunchPlan aln_plan_launches(const AlnDesc* descs, const uint32_t* order, uint32_t count,
                                uint32_t lanes, uint32_t band_k, uint32_t s_stride,
                                const AlnArenaCaps& caps) {
  AlnLaunchPlan plan;
  const uint32_t num_waves_total = (count + lanes - 1) / lanes;
  plan.waves.reserve(num_waves_total);
  uint32_t wave_begin = 0;
  while (wave_begin < num_waves_total) {
    // a wave whose state alone exceeds an arena (giant target at a wide
    // explicit band: e.g. 262 kbp at K=16 needs ~4.3 GB of tb) can never
    // launch — fail its alignments to the CPU pairwise fallback instead of
    // writing out of bounds. No construction-time carve guarantees a full
    // max_len wave fits; this check is the guarantee.
    {
      const WaveNeeds n = wave_needs(descs, order, count, lanes, band_k, s_stride, wave_begin);
      if (n.peq > caps.peq_u64 || n.tb > caps.tb_u64 || n.s > caps.s_i32) {
        for (uint32_t l = 0; l < lanes; ++l) {
          const uint64_t slot = static_cast<uint64_t>(wave_begin) * lanes + l;
          if (slot >= count) break;
          plan.never_run.push_back(order[slot]);
        }
        ++wave_begin;
        continue;
      }
    }
    // greedy: as many further waves as the three arenas hold together
    uint64_t peq_off = 0, tb_off = 0, s_off = 0;
    AlnSubLaunch launch;
    launch.first_wave = wave_begin;
    launch.num_waves = 0;
    launch.desc_off = static_cast<uint32_t>(plan.waves.size());
    for (uint32_t w = wave_begin; w < num_waves_total; ++w) {
      const WaveNeeds n = wave_needs(descs, order, count, lanes, band_k, s_stride, w);
      if (launch.num_waves > 0 && (peq_off + n.peq > caps.peq_u64 ||
                                   tb_off + n.tb > caps.tb_u64 || s_off + n.s > caps.s_i32)) {
        break;
      }
      AlnWaveDesc wd;
      wd.peq_off = peq_off;
      wd.tb_off = tb_off;
      wd.s_off = s_off;
      wd.nb = n.nb;
      wd.mmax = n.mmax;
      plan.waves.push_back(wd);
      peq_off += n.peq;
      tb_off += n.tb;
      s_off += n.s;
      ++launch.num_waves;
    }
    launch.num_align = std::min(count - wave_begin * lanes, launch.num_waves * lanes);
    plan.launches.push_back(launch);
    wave_begin += launch.num_waves;
  }
  return plan;
}

bool aln_wave_single_slide(uint32_t q_len, uint32_t t_len) {
  if (t_len == 0) {
    return false;
  }
  if (q_len <= 64ull * t_len) {
    return true;  // the band centre moves at most 64 rows per column
  }
  // t_len < q_len / 64 here, a few thousand columns at most: walk the rule
  // (btop_of of the kernels at K = 64)
  const uint64_t step = (static_cast<uint64_t>(q_len) << 32) / t_len;
  const int64_t nbt = (q_len + 63) / 64;
  const int64_t hi = nbt > kAlnWaveBandK ? nbt - kAlnWaveBandK : 0;
  int64_t prev = 0;
  for (uint64_t j = 1; j <= t_len; ++j) {
    const int64_t center_blk = static_cast<int64_t>(static_cast<uint32_t>((j * step) >> 32) >> 6);
    const int64_t top = std::max<int64_t>(0, std::min(center_blk - kAlnWaveBandK / 2, hi));
    if (top - prev > 1) {
      return false;
    }
    prev = top;
  }
  return true;
}

AlnWavePlan aln_plan_wave_launches(const AlnDesc* descs, const uint32_t* order, uint32_t count,
                                   const AlnArenaCaps& caps) {
  AlnWavePlan plan;
  AlnSubLaunch launch{0, 0, 0, 0};
  uint64_t tb_off = 0, s_off = 0;
  auto close_launch = [&] {
    if (launch.num_waves > 0) {
      launch.num_align = launch.num_waves;
      plan.launches.push_back(launch);
    }
    launch.num_waves = 0;
    tb_off = s_off = 0;
  };
  for (uint32_t w = 0; w < count; ++w) {
    const AlnDesc& d = descs[order[w]];
    const uint64_t steps = aln_wave_steps(d.q_len, d.t_len);
    const uint64_t tb = steps * kAlnWaveTbPerStep, s = steps * kAlnWaveSPerStep;
    const bool fits = tb <= caps.tb_u64 && s <= caps.s_i32;
    if (!fits || !aln_wave_single_slide(d.q_len, d.t_len)) {
      // no descriptor: the launch before it ends here
      close_launch();
      (fits ? plan.refused : plan.never_run).push_back(order[w]);
      continue;
    }
    if (tb_off + tb > caps.tb_u64 || s_off + s > caps.s_i32) {
      close_launch();
    }
    if (launch.num_waves == 0) {
      launch.first_wave = w;
      launch.desc_off = static_cast<uint32_t>(plan.waves.size());
    }
    AlnWaveDesc wd{};  // the wave kernel reads the two offsets and nothing else
    wd.tb_off = tb_off;
    wd.s_off = s_off;
    plan.waves.push_back(wd);
    tb_off += tb;
    s_off += s;
    ++launch.num_waves;
  }
  close_launch();
  return plan;
}

}  // namespace rga::hip
