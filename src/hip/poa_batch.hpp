// Host adapter: Window -> HIP POA kernel batches.
// Capability parity: reference src/cuda/cudabatch.{hpp,cpp} (addWindow /
// generateConsensus / reset contract, CPU-parity post-processing, per-seq
// skip accounting for effective coverage) on the MI355X kernel of
// poa_kernel.hip. One batch owns one device stream and a slab arena sized
// from the memory budget (reference: 90% free / batches).
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "core/window.hpp"
#include "hip/poa_types.hpp"

namespace rga::hip {

class PoaBatch {
 public:
  // large_graphs: carve a pool of large-class slabs (kPoaLargeLimits) out of
  // the budget and give the windows that end with kPoaNodeOverflow a second
  // pass in them (docs/DESIGN.md, "Large-graph pass"). Off, the batch is what
  // it was without the option: no pool, the same slab count.
  // score_check: guard the int16 scores with the static condition
  // poa_score_check_static plus the per-row check of the checked kernels, a
  // refused window ending with kPoaScoreRange, in place of the worst-case
  // products below (docs/DESIGN.md, "Score check"). With banded rows, or
  // where the static condition fails, the batch is what it is without it.
  PoaBatch(int device, size_t mem_budget, int8_t match, int8_t mismatch, int8_t gap,
           bool banded, uint32_t max_depth, bool large_graphs = false,
           bool score_check = false);
  ~PoaBatch();

  PoaBatch(const PoaBatch&) = delete;
  PoaBatch& operator=(const PoaBatch&) = delete;

  // Reserves arena space for the window's layers (sorted, CPU-identical
  // order). Bookkeeping only, callable under the shared queue lock; the
  // copies happen in pack() / generate(). Returns false when the batch is
  // full (caller retries with a fresh batch) or the window cannot fit this
  // configuration at all (never_fits set).
  bool add_window(const std::shared_ptr<Window>& window, bool* never_fits);

  // Copies every reserved window into the pinned staging buffers; called
  // outside the queue lock (generate() calls it implicitly).
  void pack();

  uint32_t size() const { return static_cast<uint32_t>(windows_.size()); }
  uint32_t capacity() const { return num_slabs_; }

  // int16 score guard of the large class: (4095 + 1024) * max(|m|,|x|,|g|)
  // within the bound the regular class is held to. A batch asked for large
  // graphs with scores that fail it warns once and runs without the pass.
  static bool large_scores_fit(int8_t match, int8_t mismatch, int8_t gap, bool banded);
  // large slabs of this batch; 0 when the pass is off
  uint32_t large_capacity() const { return large_slabs_; }
  // windows of the last generate() that the large-graph pass completed
  uint32_t large_completed() const { return large_completed_; }

  // whether a batch built with these arguments runs the checked kernels
  static bool score_check_applies(int8_t match, int8_t mismatch, int8_t gap, bool banded,
                                  bool score_check);
  bool score_checked() const { return score_check_; }
  // windows of the last generate() that ended with kPoaScoreRange
  uint32_t score_refused() const { return score_refused_; }

  // Lean single-predecessor rows (poa_kernel.hip, dp_row_lean), on by default.
  // Off, every row takes the general row; results are the same either way.
  // The rows run lean only where poa_lean_rows_fit holds for the batch's
  // scores, and RGA_POA_LEAN_ROWS=0 in the environment switches them off for
  // every batch of the process. The setting is the caller's, not the batch's
  // history: reset() puts it back on, so a pooled batch carries none over.
  void set_lean_rows(bool on) { lean_rows_ = on; }
  bool lean_rows() const { return lean_rows_; }

  // Runs the kernel and writes consensus into the windows; returns per-window
  // polish status (false = needs CPU fallback or <3-layer backbone copy).
  std::vector<bool> generate(bool trim);

  // Test and debugging entry, not used by the polishing path: the graph that
  // the last generate() left in the slab of window `index` (add_window
  // order). Every window of a batch has a slab of its own until reset().
  // For a window that did not end with kPoaOk only the status is set. A
  // window completed by the large-graph pass is read from its large slab,
  // which it keeps unless a later sub-launch of the pass needed the slab.
  struct WindowGraph {
    int32_t status = kPoaNotRun;
    std::vector<uint16_t> rank;       // node -> topological rank
    std::vector<uint8_t> out_cnt;     // node -> out-degree
    std::vector<uint16_t> out_edges;  // node * max_edges + e -> target
  };
  WindowGraph read_graph(uint32_t index) const;

  void reset();

 private:
  // Constructor phases (see .cpp): OOM-degrading arena allocation and the
  // matching cleanup used by both the destructor and a throwing constructor.
  void allocate_arenas(bool banded);
  void allocate_large_pool();
  void release_all();
  // second pass of generate(): the kPoaNodeOverflow windows through the large
  // slabs, results merged into the windows' kernel slots; returns how many
  // windows it ran
  uint32_t run_large_pass();

  int device_;
  void* stream_ = nullptr;

  uint32_t num_slabs_;
  size_t seq_arena_cap_;
  int8_t match_, mismatch_, gap_;
  uint32_t max_depth_;
  bool score_check_ = false;  // the checked kernels run, both passes
  uint32_t score_refused_ = 0;
  bool lean_rows_ = true;

  // pinned host staging
  uint8_t* h_seq_ = nullptr;
  uint8_t* h_weight_ = nullptr;
  uint32_t* h_layer_ends_ = nullptr;
  uint32_t* h_layer_span_ = nullptr;
  uint32_t* h_layer_index_ = nullptr;
  PoaWindowDesc* h_desc_ = nullptr;
  uint8_t* h_consensus_ = nullptr;
  uint16_t* h_coverage_ = nullptr;
  uint32_t* h_consensus_len_ = nullptr;
  int32_t* h_status_ = nullptr;

  // device memory (single allocation, carved)
  void* d_pool_ = nullptr;
  PoaDeviceArena arena_{};

  size_t seq_bytes_ = 0;
  size_t num_layer_ends_ = 0;
  std::vector<std::shared_ptr<Window>> windows_;
  std::vector<uint32_t> seqs_added_;  // layers shipped per window (coverage)
  std::vector<std::vector<uint32_t>> pending_orders_;  // layer order per reserved window
  size_t packed_upto_ = 0;
  std::vector<uint32_t> launch_slot_;  // last generate(): kernel slot per window

  // ---- large-graph pass (all empty / null when the option is off) ----
  uint32_t large_slabs_ = 0;
  void* d_large_pool_ = nullptr;
  // shares the packed inputs of arena_; descriptors, slabs, timing and
  // outputs are the pool's own, indexed by large slab
  PoaDeviceArena large_arena_{};
  PoaWindowDesc* h_large_desc_ = nullptr;
  uint32_t* h_large_layer_index_ = nullptr;
  uint8_t* h_large_consensus_ = nullptr;
  uint16_t* h_large_coverage_ = nullptr;
  uint32_t* h_large_consensus_len_ = nullptr;
  int32_t* h_large_status_ = nullptr;
  uint32_t* h_large_num_nodes_ = nullptr;
  uint32_t large_completed_ = 0;
  // last generate(), per kernel slot: the large slab the window ran in (-1:
  // not in the pass) and the node count it ended with
  std::vector<int32_t> large_slab_of_;
  std::vector<uint32_t> large_nodes_of_;
  std::vector<int64_t> large_slab_owner_;  // per large slab: kernel slot of its last user
};

}  // namespace rga::hip
