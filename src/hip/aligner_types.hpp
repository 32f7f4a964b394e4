// Device-side batch layout for the HIP pairwise (overlap) aligner.
//
// Capability parity target: GenomeWorks cudaaligner as driven by reference
// src/cuda/cudaaligner.cpp (add_alignment / align_all / get CIGARs, skip
// statuses feeding the CPU pairwise fallback) — re-designed for CDNA4:
// ONE LANE PER ALIGNMENT banded Myers bit-vector DP. Each lane advances a
// sliding band of K 64-row blocks (band = 64*K cells) column by column with
// the blocked Myers recurrence — 64 DP cells per VALU instruction, no
// cross-lane traffic in the hot loop. Per-column Pv/Mv words and block-bottom
// scores are stored wave-coalesced for the on-device O(1)-per-step traceback
// (popcount score reconstruction). Alignments whose optimal path leaves the
// band fail with kAlnBandEdge and fall back to the CPU aligner (reference
// contract: cudaaligner skip statuses -> edlib, src/cuda/cudaaligner.cpp:63-72).
#pragma once

#include <cstdint>

namespace rga::hip {

struct AlnLimits {
  uint32_t band = 512;        // band cells (64 * K); K in {4, 8, 16}
  uint32_t max_len = 262144;  // per-side length cap
};

enum AlnStatus : int32_t {
  kAlnOk = 0,
  kAlnBandEdge = 1,  // traceback hit an invalid cell: band too narrow
  kAlnNotRun = 2,
};

struct AlnDesc {
  uint32_t q_offset;  // into packed seq arena
  uint32_t q_len;     // n (DP rows)
  uint32_t t_offset;
  uint32_t t_len;      // m (DP columns)
  uint32_t path_offset;  // bytes into the path arena (capacity q_len+t_len)
  // breaking-point mode only (see AlnBpRecord)
  uint32_t t_origin;   // global target position of t[0]
  uint32_t q_origin;   // global query position of q[0]
  uint32_t bp_offset;  // records into the record arena
  uint32_t bp_count;   // window slices the target span touches
};

// Breaking-point mode: one record per window_length slice of the target
// (slices aligned to target coordinate 0) that the span [t_origin,
// t_origin + t_len) touches, in ascending target order. A slice without a
// match holds kAlnBpNone in every field.
struct alignas(16) AlnBpRecord {
  uint32_t first_t, first_q;  // first matched (target, query) position
  uint32_t last_t, last_q;    // last matched position + 1 on both axes
};
constexpr uint32_t kAlnBpNone = 0xffffffffu;

// Per-wave offsets into the shared arenas (element units). Lanes of a wave
// share one region so per-column stores coalesce across the 64 alignments.
struct AlnWaveDesc {
  uint64_t peq_off;  // u64 units: [(block*4 + code)*64 + lane]
  uint64_t tb_off;   // u64 units: [((col*K + block)*2 + {Pv,Mv})*64 + lane]
  uint64_t s_off;    // i32 units: [(col*K + block)*64 + lane]; the adaptive
                     // kernel's columns are K+1 words, word K = band top
  uint32_t nb;       // query blocks allocated in peq for this wave (>= K)
  uint32_t mmax;     // max t_len in this wave (uniform column loop bound)
};

struct AlnDeviceArena {
  const uint8_t* seqs;       // packed query/target bytes
  const AlnDesc* descs;      // original order
  const uint32_t* order;     // launch: alignment index per sorted lane slot
  const AlnWaveDesc* waves;  // launch: per-wave arena offsets
  uint64_t* peq;             // match bit-vectors per query block/code
  uint64_t* tb;              // per-column Pv/Mv band state (traceback)
  int32_t* sbuf;             // per-column block-bottom scores
  uint8_t* path;             // per alignment: ops from (n,m); 0=M,1=I,2=D
  uint32_t* path_len;        // per alignment (original index)
  int32_t* status;           // per alignment
  int32_t* edit_distance;    // per alignment (diagnostic)
  AlnBpRecord* bp;           // breaking-point mode: window records
  uint32_t window_length;    // breaking-point mode: slice width (> 0)
  uint32_t lanes_per_wave;   // alignments packed per 64-lane wave; fewer
                             // than 64 when the job is too small to give
                             // every CU multiple waves (latency hiding)
  AlnLimits limits;
};

// Where the band of K blocks lies. kDiagonal: on the rectangle diagonal.
// kAdaptive: it starts at block 0 and follows the scores downwards. kRetry:
// diagonal first, then adaptive at the same K over the alignments that came
// back kAlnBandEdge (the two policies cover different ground).
// kWide: every alignment goes through the wave kernel below (one wavefront per
// alignment, band 4096), whatever the batch's own band.
enum class AlnBandPolicy : int32_t { kDiagonal = 0, kAdaptive = 1, kRetry = 2, kWide = 3 };

// sbuf words per column: the adaptive kernel records the column's band top
// after the K block-bottom scores.
constexpr uint32_t aln_s_stride(uint32_t band_k, bool adaptive) {
  return adaptive ? band_k + 1 : band_k;
}

// Launches the K-block Myers kernel over `num_align` sorted alignments
// packed arena.lanes_per_wave to a wave. band_k must be 4, 8 or 16. With
// emit_path the traceback writes path / path_len; without it the traceback
// writes the window records (arena.bp, arena.window_length) and leaves the
// path arena alone. `adaptive` selects the adaptive-band kernel, whose waves'
// sbuf regions hold aln_s_stride(band_k, true) words per column.
void launch_aligner_kernel(const AlnDeviceArena& arena, uint32_t num_waves, uint32_t num_align,
                           uint32_t band_k, bool emit_path, bool adaptive, void* stream);

// ---- wide band: one wavefront per alignment (aligner_wave_kernel.hip) ----
//
// The band is kAlnWaveBandK blocks, one per lane. Column states are stored by
// step, [step][lane], in the same tb / sbuf arenas: per step 64 x 16 B of
// Pv/Mv and 64 x 4 B of scores. Block B of column j is stored at step j + B,
// so an alignment needs t_len + 64 + query blocks + 1 steps.
constexpr uint32_t kAlnWaveBandK = 64;
constexpr uint32_t kAlnWaveTbPerStep = 2 * 64;  // u64 words of tb per step
constexpr uint32_t kAlnWaveSPerStep = 64;       // i32 words of sbuf per step
constexpr uint64_t aln_wave_steps(uint32_t q_len, uint32_t t_len) {
  return static_cast<uint64_t>(t_len) + 64 + (q_len + 63) / 64 + 1;
}

// Launches the wave kernel: one 64-lane workgroup per alignment, alignment
// order[w] with the tb / sbuf offsets of waves[w] (peq_off, nb and mmax are
// not used). The band lies as the lane kernel's diagonal band would at
// K = 64 and the products are the same: path / path_len with emit_path, the
// window records without. Every alignment must satisfy aln_wave_single_slide
// (aligner_plan.hpp).
void launch_aligner_wave_kernel(const AlnDeviceArena& arena, uint32_t num_align, bool emit_path,
                                void* stream);

}  // namespace rga::hip
