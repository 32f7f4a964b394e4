// Launch planning for the HIP aligner: host-only, no device calls, so it can
// be exercised by a plain C++ program (tests/aligner_plan_check.cpp, built
// with the address and undefined-behaviour sanitizers).
//
// A pass over a set of alignments sorts them into waves by descending target
// length and cuts the waves into sub-launches, each of which fits the
// per-column state arenas (peq / tb / sbuf) at once. AlignerBatch plans its
// diagonal pass and, under the retry policy, the adaptive pass over the
// escaped alignments with the same code.
#pragma once

#include <cstdint>
#include <vector>

#include "hip/aligner_types.hpp"

namespace rga::hip {

struct AlnArenaCaps {
  uint64_t peq_u64;  // arena capacities in their element units
  uint64_t tb_u64;
  uint64_t s_i32;
};

// Waves [first_wave, first_wave + num_waves) of the pass, whose descriptors
// are waves[desc_off ..]; the launch's first lane slot is first_wave * lanes.
struct AlnSubLaunch {
  uint32_t first_wave;
  uint32_t num_waves;
  uint32_t num_align;
  uint32_t desc_off;
};

struct AlnLaunchPlan {
  std::vector<AlnWaveDesc> waves;       // of all sub-launches, in launch order
  std::vector<AlnSubLaunch> launches;
  std::vector<uint32_t> never_run;      // alignments of waves no arena can hold
};

// Alignments per 64-lane wave for a pass of `count` alignments. Small passes
// under-fill their waves so that every CU gets interleavable work;
// lanes_override (16, 32 or 64; anything else = none) is the tuning knob.
uint32_t aln_lanes_per_wave(uint32_t count, long lanes_override);

// Sorts `order` (alignment indices) by descending target length, ties by
// index: uniform loop bounds per wave.
void aln_sort_for_launch(const AlnDesc* descs, std::vector<uint32_t>* order);

// Cuts the sorted pass into sub-launches. band_k blocks per band; s_stride
// sbuf words per column (aln_s_stride). A wave whose state alone exceeds an
// arena goes to never_run and takes no descriptor.
AlnLaunchPlan aln_plan_launches(const AlnDesc* descs, const uint32_t* order, uint32_t count,
                                uint32_t lanes, uint32_t band_k, uint32_t s_stride,
                                const AlnArenaCaps& caps);

}  // namespace rga::hip
