#include "hip/poa_batch.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <stdexcept>
#include <type_traits>

#include "hip/hip_common.hpp"

namespace rga::hip {

namespace {

constexpr size_t kSeqArenaPerWindow = 96 * 1024;  // bases+weights staging per window (avg)

constexpr PoaLimits L = kPoaLimits;
constexpr PoaLimits LL = kPoaLargeLimits;  // the large-graph pass's class

// Large pool rule (docs/DESIGN.md, "Large-graph pass"): a quarter of the
// batch's memory budget, at most the 2048 windows that can be resident at
// once (256 CUs x 8 workgroups of 20 KiB LDS), at least one.
constexpr size_t kLargeBudgetDivisor = 4;
constexpr size_t kLargeSlabCap = 2048;
constexpr size_t kLargePerWindow =
    poa_slab_bytes<true>() + LL.max_consensus * 3 + sizeof(PoaWindowDesc) + 1024;

}  // namespace

bool PoaBatch::large_scores_fit(int8_t match, int8_t mismatch, int8_t gap, bool banded) {
  return poa_scores_fit_worst_case(LL, match, mismatch, gap, banded);
}

bool PoaBatch::score_check_applies(int8_t match, int8_t mismatch, int8_t gap, bool banded,
                                   bool score_check) {
  static_assert(L.matrix_width == LL.matrix_width);
  // banded rows reuse the values below the floor as out-of-band marks, and
  // rows whose band excludes column 0 have no column-0 score to check
  return score_check && !banded && poa_score_check_static(match, mismatch, gap, L.matrix_width);
}

PoaBatch::PoaBatch(int device, size_t mem_budget, int8_t match, int8_t mismatch, int8_t gap,
                   bool banded, uint32_t max_depth, bool large_graphs, bool score_check)
    : device_(device), match_(match), mismatch_(mismatch), gap_(gap), max_depth_(max_depth),
      score_check_(score_check_applies(match, mismatch, gap, banded, score_check)) {
  // int16 score guard: worst |score| <= (max_nodes + matrix_width) * max|param|
  // (banded mode additionally reserves values below -28000 as out-of-band)
  int32_t worst = static_cast<int32_t>(L.max_nodes + L.matrix_width) *
                  std::max({std::abs(static_cast<int32_t>(match)),
                            std::abs(static_cast<int32_t>(mismatch)),
                            std::abs(static_cast<int32_t>(gap))});
  // the kernel clamps stored scores at -28000 in every mode, so the usable
  // magnitude is 28000 (not the int16 32767 limit); banded mode additionally
  // reserves values below -28000 as out-of-band sentinels.
  // With the score check the checked kernels guard each window themselves,
  // in both capacity classes, and neither product applies.
  if (!score_check_ && worst > (banded ? 27000 : 28000)) {
    char msg[160];
    snprintf(msg, sizeof(msg),
             "[rga::hip::PoaBatch] score parameters too large for int16 GPU "
             "scores (|m|,|x|,|g| must keep (%u+%u)*max <= %d)",
             L.max_nodes, L.matrix_width, banded ? 27000 : 28000);
    throw std::runtime_error(msg);
  }

  if (large_graphs && !score_check_ && !large_scores_fit(match, mismatch, gap, banded)) {
    fprintf(stderr,
            "[rga::hip::PoaBatch] warning: score parameters too large for the int16 scores "
            "of the large-graph pass ((%u+%u)*max > %d); the pass is off for this batch\n",
            LL.max_nodes, LL.matrix_width, banded ? 27000 : 28000);
    large_graphs = false;
  }

  RGA_HIP_TRY(hipSetDevice(device_));
  hipStream_t s;
  RGA_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  stream_ = s;

  // the large pool comes out of the budget before the regular slabs are
  // counted. RGA_POA_LARGE_SLABS is a test knob that sets its size directly
  // (a small pool forces sub-launches), held to the same cap and to half of
  // the budget so that the regular batch keeps the other half.
  if (large_graphs) {
    size_t n = std::min(kLargeSlabCap, mem_budget / kLargeBudgetDivisor / kLargePerWindow);
    const char* e = getenv("RGA_POA_LARGE_SLABS");
    const long v = e != nullptr ? atol(e) : 0;
    if (v > 0) {
      n = std::min({static_cast<size_t>(v), kLargeSlabCap, mem_budget / 2 / kLargePerWindow});
    }
    large_slabs_ = static_cast<uint32_t>(std::max<size_t>(1, n));
    const size_t taken = static_cast<size_t>(large_slabs_) * kLargePerWindow;
    mem_budget = mem_budget > taken ? mem_budget - taken : 0;
  }

  const size_t per_window = poa_slab_bytes() + kSeqArenaPerWindow +
                            L.max_consensus * 3 + sizeof(PoaWindowDesc) + 1024;
  // slab cap: 8192 default; RGA_POA_SLABS raises it for single-mega-batch
  // experiments (all windows in one launch vs several contending launches)
  static const size_t slab_cap = [] {
    const char* e = getenv("RGA_POA_SLABS");
    long v = e != nullptr ? atol(e) : 0;
    return v > 0 ? static_cast<size_t>(v) : static_cast<size_t>(8192);
  }();
  num_slabs_ = static_cast<uint32_t>(
      std::min<size_t>(slab_cap, std::max<size_t>(32, mem_budget / per_window)));

  // Exception safety: the destructor does not run when the constructor
  // throws, so free whatever was acquired before rethrowing (the polisher
  // catches and falls back to the CPU engine).
  try {
    allocate_arenas(banded);
  } catch (...) {
    release_all();
    throw;
  }
}

// ---- device pool + pinned staging. The device pool is the big allocation:
// on OOM the slab count is halved and the layout retried — shared-device
// setups (rehearsals, several ranks per GPU) must degrade to smaller
// batches, not die (the round-1 sizing assumed one exclusive device).
void PoaBatch::allocate_arenas(bool banded) {
  // Lays every array out from `base` in allocation order, each rounded up
  // to 256 bytes, pointing arena_ at them; returns the pool size. Run with a
  // null base to size the pool, then again with the allocation.
  size_t max_layers = 0;
  auto lay_out = [&](void* base) {
    size_t total = 0;
    auto carve = [&](auto*& p, size_t count) {
      p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(
          reinterpret_cast<uintptr_t>(base) + total);
      total += (count * sizeof(*p) + 255) & ~size_t(255);
    };
    const size_t slabs = num_slabs_;
    carve(arena_.seq_data, seq_arena_cap_);
    carve(arena_.weight_data, seq_arena_cap_);
    carve(arena_.layer_ends, max_layers);
    carve(arena_.layer_spans, max_layers);
    carve(arena_.layer_ends_index, slabs + 1);
    carve(arena_.windows, slabs);
    for_each_poa_slab(arena_.slabs,
                      [&](auto*& p, size_t count) { carve(p, slabs * count); });
    carve(arena_.timing, slabs * kPoaTimingSlots);
    carve(arena_.consensus, slabs * L.max_consensus);
    carve(arena_.coverage, slabs * L.max_consensus);
    carve(arena_.consensus_len, slabs);
    carve(arena_.status, slabs);
    carve(arena_.num_nodes, slabs);
    return total;
  };
  for (;; num_slabs_ /= 2) {
    seq_arena_cap_ = static_cast<size_t>(num_slabs_) * kSeqArenaPerWindow;
    max_layers = static_cast<size_t>(num_slabs_) * (max_depth_ + 1);
    hipError_t err = hipMalloc(&d_pool_, lay_out(nullptr));
    if (err == hipSuccess) {
      break;
    }
    d_pool_ = nullptr;
    (void)hipGetLastError();  // clear the sticky OOM
    if (num_slabs_ <= 64) {
      throw std::runtime_error(
          "[rga::hip::PoaBatch] device arena allocation failed (out of memory)");
    }
    if (large_slabs_ > 1) {
      large_slabs_ /= 2;  // memory is short: the pool to come shrinks with the batch
    }
  }

  // ---- pinned host staging, sized to the slab count that fit ----
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_seq_), seq_arena_cap_));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_weight_), seq_arena_cap_));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_layer_ends_), max_layers * 4));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_layer_span_), max_layers * 4));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_layer_index_), (num_slabs_ + 1) * 4));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_desc_),
                            num_slabs_ * sizeof(PoaWindowDesc)));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_consensus_),
                            static_cast<size_t>(num_slabs_) * L.max_consensus));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_coverage_),
                            static_cast<size_t>(num_slabs_) * L.max_consensus * 2));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_consensus_len_), num_slabs_ * 4));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_status_), num_slabs_ * 4));

  lay_out(d_pool_);
  arena_.match = match_;
  arena_.mismatch = mismatch_;
  arena_.gap = gap_;
  arena_.lean_rows = 0;  // set per run (generate); the large class has no lean row
  arena_.band_width = banded ? 256 : 0;  // reference static band 256

  if (large_slabs_ != 0) {
    allocate_large_pool();
  }
}

// ---- the large-graph pass's pool: large-class slabs with descriptors,
// timing and outputs of their own, in one allocation next to the regular
// one. The packed inputs are shared with arena_. Degrades on OOM as the
// regular pool does.
void PoaBatch::allocate_large_pool() {
  large_arena_ = arena_;  // inputs, scores and band; the rest is carved below
  auto lay_out = [&](void* base) {
    size_t total = 0;
    auto carve = [&](auto*& p, size_t count) {
      p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(
          reinterpret_cast<uintptr_t>(base) + total);
      total += (count * sizeof(*p) + 255) & ~size_t(255);
    };
    const size_t slabs = large_slabs_;
    carve(large_arena_.layer_ends_index, slabs + 1);
    carve(large_arena_.windows, slabs);
    for_each_poa_slab<true>(large_arena_.slabs,
                            [&](auto*& p, size_t count) { carve(p, slabs * count); });
    carve(large_arena_.timing, slabs * kPoaTimingSlots);
    carve(large_arena_.consensus, slabs * LL.max_consensus);
    carve(large_arena_.coverage, slabs * LL.max_consensus);
    carve(large_arena_.consensus_len, slabs);
    carve(large_arena_.status, slabs);
    carve(large_arena_.num_nodes, slabs);
    return total;
  };
  for (;; large_slabs_ /= 2) {
    if (large_slabs_ == 0) {
      // not worth failing the batch for: the regular path is complete without
      fprintf(stderr,
              "[rga::hip::PoaBatch] warning: no memory for a large-graph slab; the "
              "large-graph pass is off for this batch\n");
      return;
    }
    hipError_t err = hipMalloc(&d_large_pool_, lay_out(nullptr));
    if (err == hipSuccess) {
      break;
    }
    d_large_pool_ = nullptr;
    (void)hipGetLastError();  // clear the sticky OOM
  }
  lay_out(d_large_pool_);

  const size_t n = large_slabs_;
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_large_desc_),
                            n * sizeof(PoaWindowDesc)));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_large_layer_index_), n * 4));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_large_consensus_),
                            n * LL.max_consensus));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_large_coverage_),
                            n * LL.max_consensus * 2));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_large_consensus_len_), n * 4));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_large_status_), n * 4));
  RGA_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h_large_num_nodes_), n * 4));
}

PoaBatch::~PoaBatch() { release_all(); }

void PoaBatch::release_all() {
  (void)hipSetDevice(device_);
  if (d_pool_ != nullptr) {
    (void)hipFree(d_pool_);
  }
  if (d_large_pool_ != nullptr) {
    (void)hipFree(d_large_pool_);
  }
  for (void* p : {static_cast<void*>(h_large_desc_), static_cast<void*>(h_large_layer_index_),
                  static_cast<void*>(h_large_consensus_), static_cast<void*>(h_large_coverage_),
                  static_cast<void*>(h_large_consensus_len_),
                  static_cast<void*>(h_large_status_), static_cast<void*>(h_large_num_nodes_)}) {
    if (p != nullptr) {
      (void)hipHostFree(p);
    }
  }
  for (void* p : {static_cast<void*>(h_seq_), static_cast<void*>(h_weight_),
                  static_cast<void*>(h_layer_ends_), static_cast<void*>(h_layer_span_),
                  static_cast<void*>(h_layer_index_),
                  static_cast<void*>(h_desc_), static_cast<void*>(h_consensus_),
                  static_cast<void*>(h_coverage_), static_cast<void*>(h_consensus_len_),
                  static_cast<void*>(h_status_)}) {
    if (p != nullptr) {
      (void)hipHostFree(p);
    }
  }
  if (stream_ != nullptr) {
    (void)hipStreamDestroy(static_cast<hipStream_t>(stream_));
  }
}

bool PoaBatch::add_window(const std::shared_ptr<Window>& window, bool* never_fits) {
  *never_fits = false;
  const uint32_t total_layers = window->num_layers();

  // backbone must fit the DP row; otherwise this window can never run here
  if (window->sequence(0).second + 1 > L.matrix_width) {
    *never_fits = true;
    return false;
  }
  if (windows_.size() >= num_slabs_) {
    return false;
  }

  // CPU-identical layer order: backbone, then layers by window start position
  std::vector<uint32_t> order = window->layer_order();

  // count + measure what ships (skip too-long layers, cap depth)
  uint32_t shipped = 1;
  uint32_t max_len = window->sequence(0).second;
  size_t bytes = window->sequence(0).second;
  for (uint32_t k = 1; k < total_layers && shipped < max_depth_ + 1; ++k) {
    uint32_t i = order[k];
    uint32_t len = window->sequence(i).second;
    if (len + 1 > L.matrix_width) {
      continue;  // reference: exceeded_maximum_sequence_size -> skipped
    }
    bytes += len;
    max_len = std::max(max_len, len);
    ++shipped;
  }

  if (seq_bytes_ + bytes > seq_arena_cap_) {
    return false;  // arena full; try the next batch round
  }

  // reserve (bookkeeping only; copies happen in pack() outside the queue lock)
  const uint32_t win_idx = static_cast<uint32_t>(windows_.size());
  PoaWindowDesc desc;
  desc.seq_offset = static_cast<uint32_t>(seq_bytes_);
  desc.scratch_idx = win_idx;
  desc.num_seqs = shipped;
  desc.max_len = max_len;
  h_layer_index_[win_idx] = static_cast<uint32_t>(num_layer_ends_);
  seq_bytes_ += bytes;
  num_layer_ends_ += shipped;
  h_desc_[win_idx] = desc;

  windows_.emplace_back(window);
  pending_orders_.emplace_back(std::move(order));
  seqs_added_.emplace_back(shipped - 1);  // layers only (effective coverage)
  return true;
}

void PoaBatch::pack() {
  for (; packed_upto_ < windows_.size(); ++packed_upto_) {
    const auto& window = windows_[packed_upto_];
    const auto& order = pending_orders_[packed_upto_];
    const PoaWindowDesc& desc = h_desc_[packed_upto_];
    size_t off = desc.seq_offset;
    uint32_t ends_at = h_layer_index_[packed_upto_];
    uint32_t rel_end = 0;
    uint32_t packed = 0;
    const uint32_t total_layers = window->num_layers();
    const uint32_t bb_len = window->sequence(0).second;
    // CPU spanning rule (Window::generate_consensus): a layer within 1% of
    // both window edges aligns against the full graph
    const uint32_t edge_margin = static_cast<uint32_t>(0.01 * bb_len);
    for (uint32_t k = 0; k < total_layers && packed < desc.num_seqs; ++k) {
      uint32_t i = order[k];
      auto seq = window->sequence(i);
      auto qual = window->quality(i);
      if (k > 0 && seq.second + 1 > L.matrix_width) {
        continue;
      }
      uint32_t span_word = 0xFFFFFFFFu;  // backbone / spanning layers: full DP
      if (k > 0) {
        auto sp = window->span(i);
        const bool spans_window =
            sp.first < edge_margin && sp.second > bb_len - edge_margin;
        if (!spans_window) {
          span_word = (sp.first << 16) | (sp.second & 0xffffu);
        }
      }
      h_layer_span_[ends_at] = span_word;
      std::memcpy(h_seq_ + off, seq.first, seq.second);
      if (qual.first != nullptr) {
        for (uint32_t b = 0; b < seq.second; ++b) {
          h_weight_[off + b] = static_cast<uint8_t>(qual.first[b]) - 33;
        }
      } else {
        std::memset(h_weight_ + off, 1, seq.second);
      }
      off += seq.second;
      rel_end += seq.second;
      h_layer_ends_[ends_at++] = rel_end;
      ++packed;
    }
  }
}

std::vector<bool> PoaBatch::generate(bool trim) {
  std::vector<bool> polished(windows_.size(), false);
  if (windows_.empty()) {
    return polished;
  }
  using clk = std::chrono::steady_clock;
  const bool host_timing = getenv("RGA_POA_HOSTTIME") != nullptr;
  auto t0 = clk::now();

  pack();
  const size_t nw0 = windows_.size();
  // order: kernel variant first (each is its own instantiation launched
  // over a contiguous desc range), heaviest windows first within a variant
  // (blocks launch roughly in order, so the long poles start early instead
  // of defining the tail)
  std::vector<uint32_t> perm(nw0);
  for (uint32_t i = 0; i < nw0; ++i) perm[i] = i;
  auto cost = [&](uint32_t w) {
    const uint32_t first = h_layer_index_[w];
    return h_layer_ends_[first + h_desc_[w].num_seqs - 1];  // total layer bytes
  };
  // routing reads h_desc_, which is overwritten with the sorted descriptors
  // below — snapshot per original window up front so both the comparator and
  // the launch-range split see the pre-sort values
  std::vector<PoaVariant> variant_of(nw0);
  for (uint32_t i = 0; i < nw0; ++i) {
    variant_of[i] = poa_route(h_desc_[i].max_len, h_desc_[i].num_seqs, arena_.band_width);
  }
  std::sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
    const PoaVariant va = variant_of[a], vb = variant_of[b];
    if (va != vb) return va < vb;
    const uint32_t ca = cost(a), cb = cost(b);
    if (ca != cb) return ca > cb;
    return a < b;
  });
  std::vector<PoaWindowDesc> desc_sorted(nw0);
  std::vector<uint32_t> lidx_sorted(nw0);
  launch_slot_.assign(nw0, 0);
  for (uint32_t w = 0; w < nw0; ++w) {
    desc_sorted[w] = h_desc_[perm[w]];
    lidx_sorted[w] = h_layer_index_[perm[w]];
    launch_slot_[perm[w]] = w;
  }
  std::copy(desc_sorted.begin(), desc_sorted.end(), h_desc_);
  std::copy(lidx_sorted.begin(), lidx_sorted.end(), h_layer_index_);

  RGA_HIP_CHECK(hipSetDevice(device_));
  auto s = static_cast<hipStream_t>(stream_);
  auto d = [&](const void* dst, const void* src, size_t bytes) {
    RGA_HIP_CHECK(hipMemcpyAsync(const_cast<void*>(dst), src, bytes, hipMemcpyHostToDevice, s));
  };
  d(arena_.seq_data, h_seq_, seq_bytes_);
  d(arena_.weight_data, h_weight_, seq_bytes_);
  d(arena_.layer_ends, h_layer_ends_, num_layer_ends_ * 4);
  d(arena_.layer_spans, h_layer_span_, num_layer_ends_ * 4);
  d(arena_.layer_ends_index, h_layer_index_, windows_.size() * 4);
  d(arena_.windows, h_desc_, windows_.size() * sizeof(PoaWindowDesc));

  // Lean rows: the batch's switch, the range condition of the packed row
  // (decided here, once per launch, next to the constructor's guards) and the
  // process-wide A/B switch.
  static const bool lean_env = [] {
    const char* e = getenv("RGA_POA_LEAN_ROWS");
    return e == nullptr || atoi(e) != 0;
  }();
  arena_.lean_rows =
      lean_rows_ && lean_env && poa_lean_rows_fit(match_, mismatch_, gap_) ? 1 : 0;

  // one launch per variant over its contiguous range
  for (uint32_t begin = 0, end; begin < nw0; begin = end) {
    const PoaVariant v = variant_of[perm[begin]];
    for (end = begin + 1; end < nw0 && variant_of[perm[end]] == v; ++end) {
    }
    if (score_check_) {
      launch_poa_kernel_checked(arena_, begin, end - begin, v, stream_);
    } else {
      launch_poa_kernel(arena_, begin, end - begin, v, stream_);
    }
  }

  const size_t nw = windows_.size();
  RGA_HIP_CHECK(hipMemcpyAsync(h_consensus_, arena_.consensus,
                               nw * L.max_consensus, hipMemcpyDeviceToHost, s));
  RGA_HIP_CHECK(hipMemcpyAsync(h_coverage_, arena_.coverage,
                               nw * L.max_consensus * 2, hipMemcpyDeviceToHost, s));
  RGA_HIP_CHECK(hipMemcpyAsync(h_consensus_len_, arena_.consensus_len, nw * 4,
                               hipMemcpyDeviceToHost, s));
  RGA_HIP_CHECK(hipMemcpyAsync(h_status_, arena_.status, nw * 4, hipMemcpyDeviceToHost, s));
  auto t1 = clk::now();
  RGA_HIP_CHECK(hipStreamSynchronize(s));
  auto t2 = clk::now();

  // second chance for the windows that outgrew their variant's node cap
  large_completed_ = 0;
  large_slab_of_.assign(nw, -1);
  large_nodes_of_.assign(nw, 0);
  auto t_post = t2;  // where the post-processing share of the host timing starts
  if (large_slabs_ != 0) {
    const uint32_t ran = run_large_pass();
    t_post = clk::now();
    if (host_timing && ran != 0) {
      fprintf(stderr,
              "[rga::hip::PoaBatch] host timing: large-graph pass over %u window(s) %.1f ms\n",
              ran,
              std::chrono::duration_cast<std::chrono::microseconds>(t_post - t2).count() /
                  1000.0);
    }
  }

  if (getenv("RGA_POA_TIMING") != nullptr) {
    constexpr size_t kSlots = kPoaTimingSlots;
    std::vector<unsigned long long> t(nw * kSlots);
    RGA_HIP_CHECK(hipMemcpy(t.data(), arena_.timing, t.size() * sizeof(t[0]),
                            hipMemcpyDeviceToHost));
    unsigned long long sum[kSlots] = {0};
    std::vector<unsigned long long> totals(nw);
    unsigned long long rows = 0, lean = 0;
    for (size_t i = 0; i < nw; ++i) {
      for (size_t k = 0; k < kSlots - 1; ++k) sum[k] += t[i * kSlots + k];
      // slot 7 holds three counts (poa_pack_counts)
      sum[7] += poa_count_layers(t[i * kSlots + 7]);
      lean += poa_count_lean_rows(t[i * kSlots + 7]);
      rows += poa_count_rows(t[i * kSlots + 7]);
      totals[i] = t[i * kSlots + 6];
    }
    std::sort(totals.begin(), totals.end());
    fprintf(stderr,
            "[rga::hip::PoaBatch] timing (wall ticks, %zu windows): dp=%llu tb=%llu "
            "add=%llu topo=%llu rdesc=%llu cons=%llu total=%llu layers=%llu rows=%llu "
            "lean_rows=%llu (%.1f%%)\n"
            "[rga::hip::PoaBatch] window total ticks: p50=%llu p90=%llu p99=%llu max=%llu\n",
            nw, sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6], sum[7], rows, lean,
            rows != 0 ? 100.0 * static_cast<double>(lean) / static_cast<double>(rows) : 0.0,
            totals[nw / 2], totals[nw * 9 / 10], totals[nw * 99 / 100], totals[nw - 1]);
  }

  // CPU-parity post-processing (reference cudabatch.cpp:199-261).
  // Kernel slot i handled original window perm[i].
  score_refused_ = 0;
  for (size_t i = 0; i < nw; ++i) {
    const uint32_t orig = perm[i];
    auto& window = windows_[orig];
    if (h_status_[i] == kPoaScoreRange) {
      ++score_refused_;  // either pass; counted for the polisher's report
    }
    if (h_status_[i] != kPoaOk || h_consensus_len_[i] == 0) {
      polished[orig] = false;  // device-side failure -> CPU fallback
      continue;
    }
    std::string consensus(reinterpret_cast<char*>(h_consensus_ + i * L.max_consensus),
                          h_consensus_len_[i]);
    bool status = true;
    if (window->type() == WindowType::kTGS && trim) {
      const uint16_t* cov = h_coverage_ + i * L.max_consensus;
      uint32_t average = seqs_added_[orig] / 2;
      int32_t begin = 0, end = static_cast<int32_t>(consensus.size()) - 1;
      for (; begin < static_cast<int32_t>(consensus.size()); ++begin) {
        if (cov[begin] >= average) {
          break;
        }
      }
      for (; end >= 0; --end) {
        if (cov[end] >= average) {
          break;
        }
      }
      if (begin >= end) {
        fprintf(stderr, "[rga::hip::PoaBatch] warning: contig %lu might be chimeric in window %u!\n",
                static_cast<unsigned long>(window->id()), window->rank());
        status = false;
      } else {
        consensus = consensus.substr(begin, end - begin + 1);
      }
    }
    if (status) {
      window->set_consensus(std::move(consensus));
      if (large_slab_of_[i] >= 0) {
        ++large_completed_;
      }
    }
    polished[orig] = status;
  }
  if (host_timing) {
    auto t3 = clk::now();
    auto ms = [](auto a, auto b) {
      return std::chrono::duration_cast<std::chrono::microseconds>(b - a).count() / 1000.0;
    };
    fprintf(stderr,
            "[rga::hip::PoaBatch] host timing (%zu windows): pack+sort+h2d+launch %.1f ms, "
            "gpu sync %.1f ms, post %.1f ms\n",
            nw, ms(t0, t1), ms(t1, t2), ms(t_post, t3));
  }
  return polished;
}

// The windows the regular launches left with kPoaNodeOverflow, again, in the
// large slabs. Runs after the status copy of generate(): h_desc_ and
// h_layer_index_ hold the sorted (kernel slot) order and the packed inputs
// are on the device, so a window only needs a descriptor that names a large
// slab. The kernel builds its graph from the backbone up, whatever the slab
// held. Status, consensus, coverage and node count of every window of the
// pass replace those of its kernel slot, so the post-processing of generate()
// treats it like any other. Only kPoaNodeOverflow is retried: the other caps
// are the same in both classes.
uint32_t PoaBatch::run_large_pass() {
  const size_t nw = windows_.size();
  std::vector<uint32_t> todo;
  for (uint32_t i = 0; i < nw; ++i) {
    if (h_status_[i] == kPoaNodeOverflow) {
      todo.push_back(i);
    }
  }
  if (todo.empty()) {
    return 0;
  }
  // heaviest first, as in the regular launches
  auto cost = [&](uint32_t slot) {
    return h_layer_ends_[h_layer_index_[slot] + h_desc_[slot].num_seqs - 1];
  };
  std::sort(todo.begin(), todo.end(), [&](uint32_t a, uint32_t b) {
    const uint32_t ca = cost(a), cb = cost(b);
    return ca != cb ? ca > cb : a < b;
  });

  auto s = static_cast<hipStream_t>(stream_);
  const bool timing = getenv("RGA_POA_TIMING") != nullptr;
  large_slab_owner_.assign(large_slabs_, -1);
  for (size_t begin = 0; begin < todo.size(); begin += large_slabs_) {
    const uint32_t n = static_cast<uint32_t>(std::min<size_t>(large_slabs_, todo.size() - begin));
    for (uint32_t k = 0; k < n; ++k) {
      const uint32_t slot = todo[begin + k];
      h_large_desc_[k] = h_desc_[slot];
      h_large_desc_[k].scratch_idx = k;
      h_large_layer_index_[k] = h_layer_index_[slot];
    }
    RGA_HIP_CHECK(hipMemcpyAsync(const_cast<PoaWindowDesc*>(large_arena_.windows), h_large_desc_,
                                 n * sizeof(PoaWindowDesc), hipMemcpyHostToDevice, s));
    RGA_HIP_CHECK(hipMemcpyAsync(const_cast<uint32_t*>(large_arena_.layer_ends_index),
                                 h_large_layer_index_, n * 4, hipMemcpyHostToDevice, s));
    if (score_check_) {
      launch_poa_kernel_large_checked(large_arena_, 0, n, stream_);
    } else {
      launch_poa_kernel_large(large_arena_, 0, n, stream_);
    }
    RGA_HIP_CHECK(hipMemcpyAsync(h_large_consensus_, large_arena_.consensus,
                                 static_cast<size_t>(n) * LL.max_consensus,
                                 hipMemcpyDeviceToHost, s));
    RGA_HIP_CHECK(hipMemcpyAsync(h_large_coverage_, large_arena_.coverage,
                                 static_cast<size_t>(n) * LL.max_consensus * 2,
                                 hipMemcpyDeviceToHost, s));
    RGA_HIP_CHECK(hipMemcpyAsync(h_large_consensus_len_, large_arena_.consensus_len, n * 4,
                                 hipMemcpyDeviceToHost, s));
    RGA_HIP_CHECK(hipMemcpyAsync(h_large_status_, large_arena_.status, n * 4,
                                 hipMemcpyDeviceToHost, s));
    RGA_HIP_CHECK(hipMemcpyAsync(h_large_num_nodes_, large_arena_.num_nodes, n * 4,
                                 hipMemcpyDeviceToHost, s));
    RGA_HIP_CHECK(hipStreamSynchronize(s));

    static_assert(L.max_consensus == LL.max_consensus);
    for (uint32_t k = 0; k < n; ++k) {
      const uint32_t slot = todo[begin + k];
      h_status_[slot] = h_large_status_[k];
      h_consensus_len_[slot] = h_large_consensus_len_[k];
      std::memcpy(h_consensus_ + static_cast<size_t>(slot) * L.max_consensus,
                  h_large_consensus_ + static_cast<size_t>(k) * LL.max_consensus,
                  LL.max_consensus);
      std::memcpy(h_coverage_ + static_cast<size_t>(slot) * L.max_consensus,
                  h_large_coverage_ + static_cast<size_t>(k) * LL.max_consensus,
                  LL.max_consensus * 2);
      large_slab_of_[slot] = static_cast<int32_t>(k);
      large_nodes_of_[slot] = h_large_num_nodes_[k];
      large_slab_owner_[k] = slot;
    }

    if (timing) {
      constexpr size_t kSlots = kPoaTimingSlots;
      std::vector<unsigned long long> t(n * kSlots);
      RGA_HIP_CHECK(hipMemcpy(t.data(), large_arena_.timing, t.size() * sizeof(t[0]),
                              hipMemcpyDeviceToHost));
      unsigned long long sum[kSlots] = {0};
      unsigned long long longest = 0;
      for (size_t i = 0; i < n; ++i) {
        for (size_t k = 0; k < kSlots - 1; ++k) sum[k] += t[i * kSlots + k];
        sum[7] += poa_count_layers(t[i * kSlots + 7]);  // poa_pack_counts
        longest = std::max(longest, t[i * kSlots + 6]);
      }
      fprintf(stderr,
              "[rga::hip::PoaBatch] large-graph pass timing (wall ticks, %u windows): dp=%llu "
              "tb=%llu add=%llu topo=%llu rdesc=%llu cons=%llu total=%llu layers=%llu max=%llu\n",
              n, sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], sum[6], sum[7], longest);
    }
  }
  return static_cast<uint32_t>(todo.size());
}

PoaBatch::WindowGraph PoaBatch::read_graph(uint32_t index) const {
  if (index >= launch_slot_.size() || launch_slot_.size() != windows_.size()) {
    throw std::runtime_error("[rga::hip::PoaBatch] read_graph: no such window in the last run");
  }
  RGA_HIP_CHECK(hipSetDevice(device_));
  WindowGraph g;
  g.status = h_status_[launch_slot_[index]];
  if (g.status != kPoaOk) {
    return g;
  }
  uint32_t n = 0;
  const PoaSlabs* slabs = &arena_.slabs;
  size_t slab = 0;  // first node of the window's slab
  const uint32_t slot = launch_slot_[index];
  if (slot < large_slab_of_.size() && large_slab_of_[slot] >= 0) {
    // finished in the large-graph pass: the graph is in its large slab
    const uint32_t k = static_cast<uint32_t>(large_slab_of_[slot]);
    if (large_slab_owner_[k] != static_cast<int64_t>(slot)) {
      throw std::runtime_error(
          "[rga::hip::PoaBatch] read_graph: a later sub-launch of the large-graph pass "
          "reused the window's slab");
    }
    n = large_nodes_of_[slot];
    if (n > LL.max_nodes) {
      throw std::runtime_error("[rga::hip::PoaBatch] read_graph: node count beyond the slab");
    }
    slabs = &large_arena_.slabs;
    slab = static_cast<size_t>(k) * LL.max_nodes;
  } else {
    RGA_HIP_CHECK(hipMemcpy(&n, arena_.num_nodes + slot, sizeof(n), hipMemcpyDeviceToHost));
    if (n > L.max_nodes) {
      throw std::runtime_error("[rga::hip::PoaBatch] read_graph: node count beyond the slab");
    }
    // add_window gave window `index` the slab of the same number
    slab = static_cast<size_t>(index) * L.max_nodes;
  }
  static_assert(L.max_edges == LL.max_edges);
  g.rank.resize(n);
  g.out_cnt.resize(n);
  g.out_edges.resize(static_cast<size_t>(n) * L.max_edges);
  if (n != 0) {
    RGA_HIP_CHECK(hipMemcpy(g.rank.data(), slabs->rank + slab, n * sizeof(uint16_t),
                            hipMemcpyDeviceToHost));
    RGA_HIP_CHECK(hipMemcpy(g.out_cnt.data(), slabs->out_cnt + slab, n,
                            hipMemcpyDeviceToHost));
    RGA_HIP_CHECK(hipMemcpy(g.out_edges.data(), slabs->out_edges + slab * L.max_edges,
                            g.out_edges.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
  }
  return g;
}

void PoaBatch::reset() {
  launch_slot_.clear();
  large_slab_of_.clear();
  large_nodes_of_.clear();
  large_completed_ = 0;
  score_refused_ = 0;
  lean_rows_ = true;
  windows_.clear();
  seqs_added_.clear();
  pending_orders_.clear();
  packed_upto_ = 0;
  seq_bytes_ = 0;
  num_layer_ends_ = 0;
}

}  // namespace rga::hip
