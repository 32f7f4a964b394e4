// Host adapter: Overlap -> HIP Myers aligner batches.
// Capability parity: reference src/cuda/cudaaligner.{hpp,cpp}
// (addOverlap / alignAll / generate_cigar_strings / reset; skip statuses
// leave the CIGAR empty so the CPU pairwise aligner picks the overlap up).
// Alignments are sorted by target length into 64-lane waves (uniform loop
// bounds per wave) and dispatched in as many sub-launches as the traceback
// arena requires.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "core/overlap.hpp"
#include "core/sequence.hpp"
#include "hip/aligner_types.hpp"

namespace rga::hip {

class AlignerBatch {
 public:
  // band_width: requested band in cells (rounded to K in {4,8,16} blocks);
  // 0 selects the default 512.
  AlignerBatch(int device, size_t mem_budget, uint32_t band_width);
  ~AlignerBatch();

  AlignerBatch(const AlignerBatch&) = delete;
  AlignerBatch& operator=(const AlignerBatch&) = delete;

  // Reserves arena space for the overlap's query/target spans (bookkeeping
  // only — callable under the shared queue lock). Returns false when the
  // batch is full; never_fits is set when this overlap cannot run on the GPU
  // at all. The actual copies happen in pack().
  // window_length > 0 reserves the overlap in breaking-point mode (below),
  // with the overlap's own target / query origins.
  bool add_overlap(Overlap* overlap, const std::vector<std::unique_ptr<Sequence>>& sequences,
                   bool* never_fits, uint32_t window_length = 0);

  // Raw-span variant (testing / direct use): returns the slot index, -1 when
  // the batch is full, -2 when the pair can never run here: empty or over-long
  // sequences, or non-ACGT bytes in both of them (checked unless
  // scan_non_acgt is false, for callers that already know one side is pure
  // A/C/G/T).
  //
  // window_length selects what the batch produces. 0: a path per alignment
  // (cigar_of). > 0: breaking points per alignment (breaking_points_of) for
  // window_length slices of the target, with t[0] at global target position
  // t_origin and q[0] at query position q_origin; the kernel then writes one
  // 16-byte record per slice instead of the path. A batch holds one
  // window_length at a time: a reservation with another one gets -1 (flush
  // first), and one whose records alone exceed the record arena gets -2.
  int32_t reserve_span(const char* q, uint32_t q_len, const char* t, uint32_t t_len,
                       bool scan_non_acgt = true, uint32_t window_length = 0,
                       uint32_t t_origin = 0, uint32_t q_origin = 0);

  // Where the band lies for the runs that follow (AlnBandPolicy; diagonal
  // unless set). A property of the use, not of the batch: pooled batches are
  // keyed by device and band only, so whoever takes one sets the policy.
  void set_band_policy(AlnBandPolicy policy) { policy_ = policy; }
  AlnBandPolicy band_policy() const { return policy_; }

  // Last pass before the CPU aligner (off unless set): the alignments that
  // the policy's own passes leave kAlnBandEdge go through the wave kernel,
  // one wavefront per alignment with a band of 4096. Like the policy, a
  // property of the use: whoever takes a pooled batch sets it.
  void set_wide_pass(bool on) { wide_pass_ = on; }
  bool wide_pass() const { return wide_pass_; }

  // Runs the kernel over everything reserved (pack + sub-launches + D2H). In
  // breaking-point mode the records come back instead of path / path_len.
  // Under kRetry a second, adaptive pass runs over the alignments the
  // diagonal pass returned as kAlnBandEdge; every other alignment keeps its
  // first-pass result, and kAlnNotRun alignments are not retried. The wide
  // pass, when set, follows under the same rules. Under kWide the wave kernel
  // is the only pass; a pair it refuses (aln_wave_single_slide) comes back
  // kAlnBandEdge.
  void run();
  // Alignments the last run()'s second pass completed (kRetry only).
  uint32_t retry_completed() const { return retry_completed_; }
  // Alignments the last run()'s wide pass completed (set_wide_pass only).
  uint32_t wide_completed() const { return wide_completed_; }
  // Post-run accessors per slot.
  int32_t status_of(uint32_t slot) const { return h_status_[slot]; }
  int32_t edit_distance_of(uint32_t slot) const { return h_edit_[slot]; }
  std::string cigar_of(uint32_t slot) const;  // path mode only
  // Breaking-point mode only: (t, q) of the first match and one past the
  // last match of every slice that has a match, in target order. Empty for a
  // non-zero status.
  std::vector<std::pair<uint32_t, uint32_t>> breaking_points_of(uint32_t slot) const;

  // Copies every reserved span into the pinned staging buffers. Called
  // outside the queue lock so fills from different batches proceed in
  // parallel.
  void pack();

  uint32_t size() const { return static_cast<uint32_t>(overlaps_.size()); }

  // Runs the kernel (possibly several sub-launches) and hands the result to
  // the accepted overlaps. Overlaps reserved in breaking-point mode get their
  // breaking points straight from the kernel's records. Overlaps reserved in
  // path mode get a CIGAR string, which window_length > 0 then walks into
  // breaking points right on the emit threads — the walk overlaps the other
  // batches' kernels instead of serializing in the post-GPU CPU pass.
  // Returns how many overlaps fell back (band-edge -> CPU aligner); under
  // kRetry that is the count after the second pass, and *adaptive_completed
  // (when given) gets the number of overlaps the second pass completed, and
  // *wide_completed the number the wide pass completed.
  uint32_t align_and_emit(uint32_t window_length = 0, uint32_t* adaptive_completed = nullptr,
                          uint32_t* wide_completed = nullptr);

  void reset();

 private:
  void allocate_arenas(size_t mem_budget);
  void release_all();
  // One kernel pass over the alignments in `order` (any order; sorted here):
  // plans the sub-launches and enqueues them. Alignments of waves that can
  // never launch are appended to *never_run.
  void launch_pass(std::vector<uint32_t> order, bool adaptive, std::vector<uint32_t>* never_run);
  // One pass of the wave kernel over the alignments in `order`. Alignments
  // whose state no arena can hold are appended to *never_run, those the
  // kernel's schedule does not cover to *refused; neither is touched on the
  // device.
  void launch_wide_pass(std::vector<uint32_t> order, std::vector<uint32_t>* never_run,
                        std::vector<uint32_t>* refused);
  // D2H of the products and statuses, then a stream sync.
  void read_back();

 private:
  int device_;
  void* stream_ = nullptr;
  AlnLimits limits_;
  uint32_t band_k_;  // blocks per band (4, 8 or 16)

  size_t seq_cap_, path_cap_;
  size_t bp_cap_;  // window records
  uint64_t tb_cap_u64_, s_cap_i32_, peq_cap_u64_;
  uint64_t fill_cap_u64_;  // tb words one fill may reserve
  uint32_t max_alignments_;
  uint32_t max_waves_ = 0;  // descriptors h_waves_ / d_waves_ hold

  uint8_t* h_seqs_ = nullptr;
  AlnDesc* h_descs_ = nullptr;
  uint8_t* h_path_ = nullptr;
  uint32_t* h_path_len_ = nullptr;
  int32_t* h_status_ = nullptr;
  int32_t* h_edit_ = nullptr;
  uint32_t* h_order_ = nullptr;
  AlnWaveDesc* h_waves_ = nullptr;
  AlnBpRecord* h_bp_ = nullptr;

  void* d_pool_ = nullptr;
  AlnDeviceArena arena_{};
  uint32_t* d_order_ = nullptr;
  AlnWaveDesc* d_waves_ = nullptr;

  size_t seq_bytes_ = 0;
  size_t path_bytes_ = 0;
  uint64_t tb_reserved_ = 0;  // u64 units of per-column state reserved
  size_t bp_records_ = 0;     // window records reserved
  uint32_t window_length_ = 0;  // of the current fill; 0 = path mode
  AlnBandPolicy policy_ = AlnBandPolicy::kDiagonal;
  bool wide_pass_ = false;
  uint32_t retry_completed_ = 0;
  uint32_t wide_completed_ = 0;
  std::vector<Overlap*> overlaps_;
  struct PendingSpan {
    const char* q;
    const char* t;
  };
  std::vector<PendingSpan> pending_;  // parallel to overlaps_; consumed by pack()
  size_t packed_upto_ = 0;
};

}  // namespace rga::hip
