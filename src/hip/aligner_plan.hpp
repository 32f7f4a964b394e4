// Launch planning for the HIP aligner: host-only, no device calls, so it can
// be exercised by a plain C++ program (tests/aligner_plan_check.cpp, built
// with the address and undefined-behaviour sanitizers).
//
// A pass over a set of alignments sorts them into waves by descending target
// length and cuts the waves into sub-launches, each of which fits the
// per-column state arenas (peq / tb / sbuf) at once. AlignerBatch plans its
// diagonal pass and, under the retry policy, the adaptive pass over the
// escaped alignments with the same code. The wide pass (one wavefront per
// alignment, state indexed by step) has a planner of its own at the end of
// this file, checked the same way (tests/aligner_wide_plan_check.cpp).
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

// ---- wide pass: one wavefront per alignment (aligner_wave_kernel.hip) ----

// True when the diagonal band at K = 64 slides at most one block per column
// for a q_len x t_len rectangle. The wave kernel's schedule needs that; the
// other pairs (q_len > 64 * t_len and more than 64 query blocks) are refused.
bool aln_wave_single_slide(uint32_t q_len, uint32_t t_len);

// `launches` cut `order` as AlnSubLaunch describes with one alignment per
// wave: first_wave is the position in `order` and every launched alignment
// has one descriptor. Alignments in never_run or refused have none and lie
// between launches.
struct AlnWavePlan {
  std::vector<AlnWaveDesc> waves;
  std::vector<AlnSubLaunch> launches;
  std::vector<uint32_t> never_run;  // state alone exceeds the tb or sbuf arena
  std::vector<uint32_t> refused;    // not aln_wave_single_slide
};

// Cuts the pass over order[0 .. count) into sub-launches whose step-indexed
// states (aln_wave_steps x kAlnWaveTbPerStep / kAlnWaveSPerStep) fit the tb
// and sbuf arenas together. caps.peq_u64 is not used: the kernel builds its
// masks in registers.
AlnWavePlan aln_plan_wave_launches(const AlnDesc* descs, const uint32_t* order, uint32_t count,
                                   const AlnArenaCaps& caps);

}  // namespace rga::hip
