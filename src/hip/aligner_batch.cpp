#include "hip/aligner_batch.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "hip/aligner_plan.hpp"
#include "hip/hip_common.hpp"

namespace rga::hip {

namespace {
constexpr uint32_t kLanes = 64;

// Band blocks for a requested width. The polisher's auto heuristic clamps
// to 256 (K=4; see hip_polisher.cpp) — explicit --cudaaligner-band-width
// values still select up to K=16.
uint32_t pick_band_k(uint32_t band_width) {
  if (band_width == 0) return 8;  // default band 512
  uint32_t blocks = (band_width + 63) / 64;
  if (blocks <= 4) return 4;
  if (blocks <= 8) return 8;
  return 16;
}

// True when every byte is one of A/C/G/T (branch-free compares, so the loop
// auto-vectorizes).
bool only_acgt(const char* s, uint32_t len) {
  uint8_t bad = 0;
  for (uint32_t i = 0; i < len; ++i) {
    const uint8_t c = static_cast<uint8_t>(s[i]);
    bad |= static_cast<uint8_t>((c != 'A') & (c != 'C') & (c != 'G') & (c != 'T'));
  }
  return bad == 0;
}

}  // namespace

AlignerBatch::AlignerBatch(int device, size_t mem_budget, uint32_t band_width)
    : device_(device), band_k_(pick_band_k(band_width)) {
  limits_.band = band_k_ * 64;
  try {
    allocate_arenas(mem_budget);
  } catch (...) {
    release_all();
    throw;
  }
}

void AlignerBatch::allocate_arenas(size_t mem_budget) {
  RGA_HIP_TRY(hipSetDevice(device_));
  hipStream_t s;
  RGA_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  stream_ = s;

  // arena split: the per-column band state dominates — per alignment
  // ~ (m+1) * K * (16 B Pv/Mv + 4 B S); seqs/path/peq are q+t-scale.
  // Cap the device pool so construction stays cheap and the POA arenas
  // (pooled at the same time) keep headroom on 288 GB parts: at K=4 a
  // 20 kbp alignment's state is ~1.3 MB, so 12 GB holds ~9k alignments.
  // On OOM (shared-device setups) the pool halves and retries.
  size_t pool = std::min<size_t>(mem_budget, 12ull << 30);
  size_t total = 0;
  // Every arena starts on a 256-byte boundary and owns a multiple of 256
  // bytes. The lane kernel relies on that for the sequence arena: it reads
  // sequences in aligned 8-byte words, and the word that holds the last
  // sequence byte of a fill may extend up to 7 bytes past seq_bytes_, which
  // the rounding keeps inside the carve whatever seq_cap_ is (no slack is
  // taken from reserve_span's capacity check).
  auto carve = [&total](size_t bytes) {
    size_t off = total;
    total += (bytes + 255) & ~size_t(255);
    return off;
  };
  size_t o_seqs = 0, o_descs = 0, o_peq = 0, o_tb = 0, o_s = 0, o_path = 0, o_plen = 0,
         o_status = 0, o_ed = 0, o_order = 0, o_waves = 0, o_bp = 0;
  uint32_t max_waves = 0;
  for (;; pool /= 2) {
    seq_cap_ = std::max<size_t>(16u << 20, pool / 96);
    path_cap_ = seq_cap_;
    peq_cap_u64_ = seq_cap_ / 8;  // 4 codes per 64 bases = q_bytes/2 of u64s
                                  // is generous; /8 covers wave-max padding
    max_alignments_ = 65536;
    // window records: an alignment needs t_len / window_length + 2 at most,
    // ~31 for a 15 kbp overlap at 500. One per 64 sequence bytes plus two per
    // alignment never binds before the sequence arena at window_length >= 64
    // (t_len is part of the alignment's sequence bytes); narrower windows
    // can fill the record arena first and the batch then flushes early.
    bp_cap_ = seq_cap_ / 64 + 2 * static_cast<size_t>(max_alignments_);

    const size_t fixed = 2 * seq_cap_ + peq_cap_u64_ * 8 + bp_cap_ * sizeof(AlnBpRecord) +
                         max_alignments_ * (sizeof(AlnDesc) + 16) + (2u << 20);
    const size_t state = pool > fixed ? pool - fixed : (16u << 20);
    // Per column and block: 16 B of Pv/Mv and 4 B of score, plus 4 B per
    // column for the adaptive kernel's band top (aln_s_stride). The policy is
    // chosen per run, so the split is always the adaptive one: both arenas
    // then hold the same number of columns under either policy, and
    // reserve_span can count tb words alone.
    const size_t per_col = 16 * band_k_ + 4 * aln_s_stride(band_k_, true);
    const size_t cols = state / per_col;  // wave-lane columns of state
    tb_cap_u64_ = cols * band_k_ * 2;
    s_cap_i32_ = cols * aln_s_stride(band_k_, true);
    // The per-fill cap (reserve_span) is a load-balancing knob, not a
    // capacity: it stays at the value the flagship was tuned with, half of a
    // 16 : 4 split's tb arena, whatever the carve above gives the arenas.
    fill_cap_u64_ = state / 20 * 16 / 8 / 2;

    // sized for the SMALLEST lanes-per-wave the launcher may pick (16 for
    // small jobs), not kLanes — and the per-sub-launch descriptor slices
    // accumulate across the whole run
    max_waves = max_alignments_ / 16 + 2;
    total = 0;
    o_seqs = carve(seq_cap_);
    o_descs = carve(max_alignments_ * sizeof(AlnDesc));
    o_peq = carve(peq_cap_u64_ * 8);
    o_tb = carve(tb_cap_u64_ * 8);
    o_s = carve(s_cap_i32_ * 4);
    o_path = carve(path_cap_);
    o_plen = carve(max_alignments_ * 4);
    o_status = carve(max_alignments_ * 4);
    o_ed = carve(max_alignments_ * 4);
    o_order = carve(max_alignments_ * 4);
    o_waves = carve(max_waves * sizeof(AlnWaveDesc));
    o_bp = carve(bp_cap_ * sizeof(AlnBpRecord));

    hipError_t err = hipMalloc(&d_pool_, total);
    if (err == hipSuccess) {
      break;
    }
    d_pool_ = nullptr;
    (void)hipGetLastError();
    if (pool <= (256u << 20)) {
      throw std::runtime_error(
          "[rga::hip::AlignerBatch] device arena allocation failed (out of memory)");
    }
  }

  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_seqs_), seq_cap_));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_descs_),
                            max_alignments_ * sizeof(AlnDesc)));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_path_), path_cap_));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_path_len_), max_alignments_ * 4));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_status_), max_alignments_ * 4));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_edit_), max_alignments_ * 4));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_order_), max_alignments_ * 4));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_waves_),
                            max_waves * sizeof(AlnWaveDesc)));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_bp_), bp_cap_ * sizeof(AlnBpRecord)));
  auto base = static_cast<uint8_t*>(d_pool_);
  arena_.seqs = base + o_seqs;
  arena_.descs = reinterpret_cast<AlnDesc*>(base + o_descs);
  arena_.peq = reinterpret_cast<uint64_t*>(base + o_peq);
  arena_.tb = reinterpret_cast<uint64_t*>(base + o_tb);
  arena_.sbuf = reinterpret_cast<int32_t*>(base + o_s);
  arena_.path = base + o_path;
  arena_.path_len = reinterpret_cast<uint32_t*>(base + o_plen);
  arena_.status = reinterpret_cast<int32_t*>(base + o_status);
  arena_.edit_distance = reinterpret_cast<int32_t*>(base + o_ed);
  arena_.bp = reinterpret_cast<AlnBpRecord*>(base + o_bp);
  arena_.window_length = 0;
  d_order_ = reinterpret_cast<uint32_t*>(base + o_order);
  d_waves_ = reinterpret_cast<AlnWaveDesc*>(base + o_waves);
  arena_.order = d_order_;
  arena_.waves = d_waves_;
  max_waves_ = max_waves;
  arena_.lanes_per_wave = kLanes;
  arena_.limits = limits_;
}

AlignerBatch::~AlignerBatch() { release_all(); }

void AlignerBatch::release_all() {
  (void)hipSetDevice(device_);
  if (d_pool_ != nullptr) {
    (void)hipFree(d_pool_);
  }
  for (void* p : {static_cast<void*>(h_seqs_), static_cast<void*>(h_descs_),
                  static_cast<void*>(h_path_), static_cast<void*>(h_path_len_),
                  static_cast<void*>(h_status_), static_cast<void*>(h_edit_),
                  static_cast<void*>(h_order_), static_cast<void*>(h_waves_),
                  static_cast<void*>(h_bp_)}) {
    if (p != nullptr) {
      (void)hipHostFree(p);
    }
  }
  if (stream_ != nullptr) {
    (void)hipStreamDestroy(static_cast<hipStream_t>(stream_));
  }
}

int32_t AlignerBatch::reserve_span(const char* q, uint32_t q_len, const char* t,
                                   uint32_t t_len, bool scan_non_acgt, uint32_t window_length,
                                   uint32_t t_origin, uint32_t q_origin) {
  if (q_len == 0 || t_len == 0 || q_len > limits_.max_len || t_len > limits_.max_len) {
    return -2;  // reference: exceeded_max_length -> CPU fallback
  }
  // window slices [k * window_length, (k + 1) * window_length) of the target
  // that the span touches: one record each
  size_t bp_need = 0;
  if (window_length > 0) {
    const uint64_t t_last = static_cast<uint64_t>(t_origin) + t_len - 1;
    if (t_last >= kAlnBpNone || static_cast<uint64_t>(q_origin) + q_len >= kAlnBpNone) {
      return -2;  // positions must stay below the 32-bit no-match marker
    }
    bp_need = static_cast<size_t>(t_last / window_length - t_origin / window_length + 1);
    if (bp_need > bp_cap_) {
      return -2;
    }
  }
  if (!overlaps_.empty() && window_length != window_length_) {
    return -1;  // one product per fill: the caller flushes first
  }
  const size_t bytes = static_cast<size_t>(q_len) + t_len;
  // per-lane share of the wave's tb region (the wave total is 64 of these,
  // and the arena-capacity check is against the sum of all shares). The
  // per-fill cap is about HALF a tb arena: a greedy first fill at the full
  // cap would swallow most of the overlap queue and starve the other batch
  // threads (the pull model balances only when rounds are smaller than
  // queue/threads). Counting tb words covers the score arena under either
  // band policy: the two are carved in proportion (allocate_arenas).
  const uint64_t tb_need = static_cast<uint64_t>(t_len + 1) * band_k_ * 2;
  if (overlaps_.size() >= max_alignments_ || seq_bytes_ + bytes > seq_cap_ ||
      path_bytes_ + bytes > path_cap_ || tb_reserved_ + tb_need > fill_cap_u64_ ||
      bp_records_ + bp_need > bp_cap_) {
    return -1;
  }
  // The kernel's base_code() matches A/C/G/T only, while the CPU aligner
  // (Peq::code_of) matches any equal bytes — N against N costs 1 on the
  // device and 0 on the host. The two agree unless BOTH sequences hold such
  // a byte (against pure A/C/G/T it mismatches either way); those pairs go
  // to the CPU path.
  if (scan_non_acgt && !only_acgt(t, t_len) && !only_acgt(q, q_len)) {
    return -2;
  }

  AlnDesc d;
  d.q_offset = static_cast<uint32_t>(seq_bytes_);
  d.q_len = q_len;
  seq_bytes_ += q_len;
  d.t_offset = static_cast<uint32_t>(seq_bytes_);
  d.t_len = t_len;
  seq_bytes_ += t_len;
  d.path_offset = static_cast<uint32_t>(path_bytes_);
  path_bytes_ += bytes;
  tb_reserved_ += tb_need;
  d.t_origin = t_origin;
  d.q_origin = q_origin;
  d.bp_offset = static_cast<uint32_t>(bp_records_);
  d.bp_count = static_cast<uint32_t>(bp_need);
  bp_records_ += bp_need;
  window_length_ = window_length;

  const int32_t slot = static_cast<int32_t>(overlaps_.size());
  h_descs_[slot] = d;
  overlaps_.emplace_back(nullptr);
  pending_.push_back({q, t});
  return slot;
}

bool AlignerBatch::add_overlap(Overlap* overlap,
                               const std::vector<std::unique_ptr<Sequence>>& sequences,
                               bool* never_fits, uint32_t window_length) {
  *never_fits = false;
  auto q = overlap->query_span(sequences);
  auto t = overlap->target_span(sequences);
  // this runs under the polisher's queue lock, where scanning every span
  // cost ~5% of flagship throughput (measured): the spans are scanned only
  // when the contig AND the read hold a non-ACGT byte somewhere (cached per
  // sequence; a pure-ACGT draft never looks at its reads)
  const bool scan = !sequences[overlap->t_id()]->acgt_only() &&
                    !sequences[overlap->q_id()]->acgt_only();
  // RGA_ALN_HOST_BP=1 keeps the path -> CIGAR -> host walk route (A/B timing
  // and the route differ test): the overlap is reserved in path mode and
  // align_and_emit walks its CIGAR
  static const bool host_bp = [] {
    const char* e = getenv("RGA_ALN_HOST_BP");
    return e != nullptr && atol(e) == 1;
  }();
  int32_t slot = reserve_span(q.first, q.second, t.first, t.second, scan,
                              host_bp ? 0 : window_length, overlap->t_begin(),
                              overlap->q_span_begin());
  if (slot == -2) {
    *never_fits = true;
    return false;
  }
  if (slot < 0) {
    return false;
  }
  overlaps_[slot] = overlap;
  return true;
}

void AlignerBatch::pack() {
  for (; packed_upto_ < overlaps_.size(); ++packed_upto_) {
    const AlnDesc& d = h_descs_[packed_upto_];
    const PendingSpan& p = pending_[packed_upto_];
    std::memcpy(h_seqs_ + d.q_offset, p.q, d.q_len);
    std::memcpy(h_seqs_ + d.t_offset, p.t, d.t_len);
  }
}

void AlignerBatch::launch_pass(std::vector<uint32_t> order, bool adaptive,
                               std::vector<uint32_t>* never_run) {
  auto s = static_cast<hipStream_t>(stream_);
  const uint32_t count = static_cast<uint32_t>(order.size());
  // sort into waves by descending target length (uniform per-wave loops)
  aln_sort_for_launch(h_descs_, &order);
  std::copy(order.begin(), order.end(), h_order_);
  RGA_HIP_CHECK(hipMemcpyAsync(d_order_, h_order_, count * 4, hipMemcpyHostToDevice, s));

  // greedy sub-launches bounded by the tb/s/peq arenas. Waves are
  // deliberately under-filled for small jobs: at 64 alignments/wave a
  // typical polish run yields ~1.5 waves per CU and every gather latency
  // lands on the wall clock; 16-32/wave gives each CU interleavable waves
  // at the cost of idle lanes (which issue no extra instructions).
  // tuning override (RGA_ALN_LANES in {16,32,64}): alignments packed per
  // 64-lane wave — fewer per wave = more interleavable waves per CU at the
  // cost of idle lanes
  static const long lanes_env = [] {
    const char* e = getenv("RGA_ALN_LANES");
    return e != nullptr ? atol(e) : 0;
  }();
  const uint32_t lanes = aln_lanes_per_wave(count, lanes_env);
  const AlnLaunchPlan plan =
      aln_plan_launches(h_descs_, h_order_, count, lanes, band_k_,
                        aln_s_stride(band_k_, adaptive), {peq_cap_u64_, tb_cap_u64_, s_cap_i32_});
  never_run->insert(never_run->end(), plan.never_run.begin(), plan.never_run.end());
  if (plan.launches.empty()) {
    return;
  }
  // every sub-launch has its own slice of the descriptor array, so they
  // enqueue back-to-back with no intervening stream sync
  std::copy(plan.waves.begin(), plan.waves.end(), h_waves_);
  RGA_HIP_CHECK(hipMemcpyAsync(d_waves_, h_waves_, plan.waves.size() * sizeof(AlnWaveDesc),
                               hipMemcpyHostToDevice, s));
  for (const AlnSubLaunch& l : plan.launches) {
    AlnDeviceArena launch_arena = arena_;
    launch_arena.order = d_order_ + static_cast<size_t>(l.first_wave) * lanes;
    launch_arena.waves = d_waves_ + l.desc_off;
    launch_arena.lanes_per_wave = lanes;
    launch_arena.window_length = window_length_;
    launch_aligner_kernel(launch_arena, l.num_waves, l.num_align, band_k_, window_length_ == 0,
                          adaptive, stream_);
  }
}

void AlignerBatch::launch_wide_pass(std::vector<uint32_t> order, std::vector<uint32_t>* never_run,
                                    std::vector<uint32_t>* refused) {
  auto s = static_cast<hipStream_t>(stream_);
  // longest first: a wave lasts as long as its alignment
  aln_sort_for_launch(h_descs_, &order);
  const uint32_t count = static_cast<uint32_t>(order.size());
  std::copy(order.begin(), order.end(), h_order_);
  RGA_HIP_CHECK(hipMemcpyAsync(d_order_, h_order_, count * 4, hipMemcpyHostToDevice, s));
  // one descriptor per alignment: the descriptor arrays, sized for the lane
  // kernel's waves, take the pass in pieces
  for (uint32_t begin = 0; begin < count; begin += max_waves_) {
    const uint32_t piece = std::min(max_waves_, count - begin);
    const AlnWavePlan plan = aln_plan_wave_launches(h_descs_, h_order_ + begin, piece,
                                                    {peq_cap_u64_, tb_cap_u64_, s_cap_i32_});
    never_run->insert(never_run->end(), plan.never_run.begin(), plan.never_run.end());
    refused->insert(refused->end(), plan.refused.begin(), plan.refused.end());
    if (plan.launches.empty()) {
      continue;
    }
    if (begin > 0) {
      RGA_HIP_CHECK(hipStreamSynchronize(s));  // the copy of the piece before read h_waves_
    }
    std::copy(plan.waves.begin(), plan.waves.end(), h_waves_);
    RGA_HIP_CHECK(hipMemcpyAsync(d_waves_, h_waves_, plan.waves.size() * sizeof(AlnWaveDesc),
                                 hipMemcpyHostToDevice, s));
    for (const AlnSubLaunch& l : plan.launches) {
      AlnDeviceArena launch_arena = arena_;
      launch_arena.order = d_order_ + begin + l.first_wave;
      launch_arena.waves = d_waves_ + l.desc_off;
      launch_arena.lanes_per_wave = 1;
      launch_arena.window_length = window_length_;
      launch_aligner_wave_kernel(launch_arena, l.num_align, window_length_ == 0, stream_);
    }
  }
}

void AlignerBatch::read_back() {
  auto s = static_cast<hipStream_t>(stream_);
  const uint32_t na = static_cast<uint32_t>(overlaps_.size());
  if (window_length_ == 0) {
    RGA_HIP_CHECK(hipMemcpyAsync(h_path_, arena_.path, path_bytes_, hipMemcpyDeviceToHost, s));
    RGA_HIP_CHECK(
        hipMemcpyAsync(h_path_len_, arena_.path_len, na * 4, hipMemcpyDeviceToHost, s));
  } else {
    RGA_HIP_CHECK(hipMemcpyAsync(h_bp_, arena_.bp, bp_records_ * sizeof(AlnBpRecord),
                                 hipMemcpyDeviceToHost, s));
  }
  RGA_HIP_CHECK(hipMemcpyAsync(h_status_, arena_.status, na * 4, hipMemcpyDeviceToHost, s));
  RGA_HIP_CHECK(hipMemcpyAsync(h_edit_, arena_.edit_distance, na * 4, hipMemcpyDeviceToHost, s));
  RGA_HIP_CHECK(hipStreamSynchronize(s));
}

void AlignerBatch::run() {
  retry_completed_ = 0;
  wide_completed_ = 0;
  if (overlaps_.empty()) {
    return;
  }
  pack();
  RGA_HIP_CHECK(hipSetDevice(device_));
  auto s = static_cast<hipStream_t>(stream_);
  const uint32_t na = static_cast<uint32_t>(overlaps_.size());
  RGA_HIP_CHECK(hipMemcpyAsync(const_cast<uint8_t*>(arena_.seqs), h_seqs_, seq_bytes_,
                               hipMemcpyHostToDevice, s));
  RGA_HIP_CHECK(hipMemcpyAsync(const_cast<AlnDesc*>(arena_.descs), h_descs_,
                               na * sizeof(AlnDesc), hipMemcpyHostToDevice, s));

  std::vector<uint32_t> all(na);
  std::iota(all.begin(), all.end(), 0u);
  std::vector<uint32_t> never_run;  // original indices of un-runnable waves
  if (policy_ == AlnBandPolicy::kWide) {
    // the wave kernel alone; what it refuses comes back as an escape
    std::vector<uint32_t> refused;
    launch_wide_pass(std::move(all), &never_run, &refused);
    read_back();
    for (uint32_t orig : never_run) {
      h_status_[orig] = kAlnNotRun;
      h_path_len_[orig] = 0;
      h_edit_[orig] = -1;
    }
    for (uint32_t orig : refused) {
      h_status_[orig] = kAlnBandEdge;
      h_path_len_[orig] = 0;
      h_edit_[orig] = -1;
    }
    return;
  }
  launch_pass(std::move(all), policy_ == AlnBandPolicy::kAdaptive, &never_run);
  read_back();
  // the device never wrote these alignments' results
  auto mark_never_run = [&] {
    for (uint32_t orig : never_run) {
      h_status_[orig] = kAlnNotRun;
      h_path_len_[orig] = 0;
      h_edit_[orig] = -1;
    }
  };
  mark_never_run();
  // alignments still escaped, for the pass that follows
  auto escaped_now = [&] {
    std::vector<uint32_t> escaped;
    for (uint32_t i = 0; i < na; ++i) {
      if (h_status_[i] == kAlnBandEdge) {
        escaped.push_back(i);
      }
    }
    return escaped;
  };
  if (policy_ == AlnBandPolicy::kRetry) {
    // second chance: the adaptive band at the same K over the escaped
    // alignments only, on the arena as packed. The kernel writes results of
    // the alignments it runs and of no other, so the device still holds the
    // first pass's for the rest and the second read-back returns them as
    // they were.
    const std::vector<uint32_t> escaped = escaped_now();
    if (!escaped.empty()) {
      // a wave the adaptive pass cannot launch leaves its alignments as the
      // first pass reported them (kAlnBandEdge)
      std::vector<uint32_t> not_retried;
      launch_pass(escaped, true, &not_retried);
      read_back();
      mark_never_run();
      for (uint32_t i : escaped) {
        retry_completed_ += h_status_[i] == kAlnOk ? 1 : 0;
      }
    }
  }
  if (!wide_pass_) {
    return;
  }
  // last chance before the CPU: the wave kernel over what is still escaped.
  // Again the device holds the earlier results of every alignment this pass
  // does not run, the ones it refuses or cannot hold included.
  const std::vector<uint32_t> escaped = escaped_now();
  if (escaped.empty()) {
    return;
  }
  std::vector<uint32_t> not_run, refused;
  launch_wide_pass(escaped, &not_run, &refused);
  read_back();
  mark_never_run();
  for (uint32_t i : escaped) {
    wide_completed_ += h_status_[i] == kAlnOk ? 1 : 0;
  }
}

std::string AlignerBatch::cigar_of(uint32_t slot) const {
  std::string cigar;
  if (h_status_[slot] != kAlnOk || h_path_len_[slot] == 0) {
    return cigar;
  }
  const uint8_t* path = h_path_ + h_descs_[slot].path_offset;
  const uint32_t plen = h_path_len_[slot];
  static const char kOps[3] = {'M', 'I', 'D'};
  // path is reversed (walked from (n, m)); emit forward with run-lengths
  uint32_t run = 0;
  uint8_t run_op = 255;
  char buf[16];
  for (int64_t k = static_cast<int64_t>(plen) - 1; k >= 0; --k) {
    uint8_t op = path[k];
    if (op == run_op) {
      ++run;
    } else {
      if (run > 0) {
        cigar.append(buf, snprintf(buf, sizeof(buf), "%u%c", run, kOps[run_op]));
      }
      run_op = op;
      run = 1;
    }
  }
  if (run > 0) {
    cigar.append(buf, snprintf(buf, sizeof(buf), "%u%c", run, kOps[run_op]));
  }
  return cigar;
}

std::vector<std::pair<uint32_t, uint32_t>> AlignerBatch::breaking_points_of(
    uint32_t slot) const {
  std::vector<std::pair<uint32_t, uint32_t>> points;
  if (h_status_[slot] != kAlnOk) {
    return points;
  }
  const AlnDesc& d = h_descs_[slot];
  const AlnBpRecord* recs = h_bp_ + d.bp_offset;
  points.reserve(2 * static_cast<size_t>(d.bp_count));
  for (uint32_t w = 0; w < d.bp_count; ++w) {
    if (recs[w].last_t == kAlnBpNone) {
      continue;  // window without a match
    }
    points.emplace_back(recs[w].first_t, recs[w].first_q);
    points.emplace_back(recs[w].last_t, recs[w].last_q);
  }
  return points;
}

uint32_t AlignerBatch::align_and_emit(uint32_t window_length, uint32_t* adaptive_completed,
                                      uint32_t* wide_completed) {
  if (adaptive_completed != nullptr) {
    *adaptive_completed = 0;
  }
  if (wide_completed != nullptr) {
    *wide_completed = 0;
  }
  if (overlaps_.empty()) {
    return 0;
  }
  run();
  if (adaptive_completed != nullptr) {
    *adaptive_completed = retry_completed_;
  }
  if (wide_completed != nullptr) {
    *wide_completed = wide_completed_;
  }
  if (window_length_ > 0) {
    // breaking-point mode: a few records per overlap, nothing worth threads.
    // An overlap without a single matched window stays untouched, as it
    // does on the CIGAR route (the CPU pass realigns it to the same end).
    uint32_t failed_bp = 0;
    for (size_t i = 0; i < overlaps_.size(); ++i) {
      if (overlaps_[i] == nullptr) {
        continue;
      }
      if (h_status_[i] != kAlnOk) {
        ++failed_bp;
        continue;
      }
      auto points = breaking_points_of(static_cast<uint32_t>(i));
      if (!points.empty()) {
        overlaps_[i]->set_breaking_points(std::move(points));
      }
    }
    return failed_bp;
  }
  // CIGAR strings are independent per slot: build them on a few threads
  // (the run-length walk over ~30 kbp paths x thousands of alignments is
  // otherwise a serial tail after every batch round)
  const size_t n = overlaps_.size();
  const uint32_t nthreads = std::min<uint32_t>(8, std::max<uint32_t>(1, n / 512));
  std::atomic<uint32_t> failed{0};
  auto emit_range = [&](size_t begin, size_t end) {
    uint32_t local_failed = 0;
    for (size_t i = begin; i < end; ++i) {
      if (overlaps_[i] == nullptr) {
        continue;
      }
      std::string cigar = cigar_of(static_cast<uint32_t>(i));
      if (cigar.empty()) {
        ++local_failed;  // empty CIGAR -> CPU pairwise fallback
        continue;
      }
      overlaps_[i]->set_cigar(std::move(cigar));
      if (window_length > 0) {
        // walk into breaking points here (overlapped with other batches'
        // GPU work); the polisher's final CPU pass then no-ops for this
        // overlap and only realigns the skipped ones
        overlaps_[i]->find_breaking_points_from_cigar(window_length);
        overlaps_[i]->set_cigar(std::string());  // consumed; free the bytes
      }
    }
    failed += local_failed;
  };
  if (nthreads <= 1) {
    emit_range(0, n);
  } else {
    std::vector<std::thread> threads;
    const size_t step = (n + nthreads - 1) / nthreads;
    for (uint32_t t = 0; t < nthreads; ++t) {
      const size_t b = t * step, e = std::min(n, b + step);
      if (b < e) {
        threads.emplace_back(emit_range, b, e);
      }
    }
    for (auto& t : threads) {
      t.join();
    }
  }
  return failed.load();
}

void AlignerBatch::reset() {
  overlaps_.clear();
  pending_.clear();
  packed_upto_ = 0;
  seq_bytes_ = 0;
  path_bytes_ = 0;
  tb_reserved_ = 0;
  bp_records_ = 0;
  window_length_ = 0;
}

}  // namespace rga::hip
