// Device-side batch layout for the HIP POA engine.
//
// Capability parity target: GenomeWorks cudapoa as driven by reference
// src/cuda/cudabatch.cpp (BatchConfig(1023, 200, 256, ...), add_poa_group /
// generate_poa / get_consensus contract) — re-designed for CDNA4: one 64-lane
// wavefront per window, full-width DP rows streamed through HBM as int16,
// graph phases in global memory (Kahn FIFO core on lane 0 over an LDS copy of
// the adjacency, traceback and path threading on all lanes) hidden by 16-32
// co-resident windows per CU.
#pragma once

#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace rga::hip {

// Capacity model (per window). Windows exceeding any cap are rejected or
// failed on device and fall back to the CPU path (reference contract:
// cudapolisher.cpp:354-383). Compile-time on both sides: the kernel keeps
// slab addressing in immediates instead of ~100 live SGPRs that were
// spilling into v_readlane/writelane traffic in the DP row loop.
struct PoaLimits {
  uint32_t max_nodes = 2047;      // POA graph nodes per window
  uint32_t max_edges = 48;        // in- or out-edges per node
  uint32_t max_ring = 4;          // aligned-ring partners per node
  uint32_t matrix_width = 1024;   // DP row width (longest layer + 1)
  uint32_t max_consensus = 2048;  // consensus output cap
};
inline constexpr PoaLimits kPoaLimits{};

// Second capacity class, for the opt-in large-graph pass over the windows
// that end with kPoaNodeOverflow (PoaBatch, docs/DESIGN.md "Large-graph
// pass"): twice the nodes, everything else as above. Node ids, ranks and
// descriptor rows are 16-bit fields and hold it; the slabs and the kernel are
// compiled once per class (poa_kernel.hip, poa_kernel_large.hip).
inline constexpr PoaLimits kPoaLargeLimits{4095, 48, 4, 1024, 2048};
constexpr PoaLimits poa_limits(bool large) { return large ? kPoaLargeLimits : kPoaLimits; }
static_assert(kPoaLargeLimits.max_edges == kPoaLimits.max_edges &&
                  kPoaLargeLimits.max_ring == kPoaLimits.max_ring &&
                  kPoaLargeLimits.matrix_width == kPoaLimits.matrix_width &&
                  kPoaLargeLimits.max_consensus == kPoaLimits.max_consensus,
              "the classes differ in max_nodes alone: they share inputs and outputs");

// Window status codes produced by the kernel.
enum PoaStatus : int32_t {
  kPoaOk = 0,
  kPoaNodeOverflow = 1,
  kPoaEdgeOverflow = 2,
  kPoaRingOverflow = 3,
  kPoaConsensusOverflow = 4,
  kPoaNotRun = 5,
  kPoaWidthOverflow = 6,  // layer wider than the launched ring variant
  kPoaScoreRange = 7,     // refused by the per-window score check (below)
};

// ---- int16 score range ----
// DP scores are stored as int16 and clamped at kPoaScoreFloor from below.
// Without the score check (PoaBatch, score_check off) a batch is guarded by
// one worst-case product per capacity class, poa_scores_fit_worst_case. With
// it the guard is a small static condition on the parameters
// (poa_score_check_static) plus one compare per DP row on the device
// (poa_score_row_refused); docs/DESIGN.md, "Score check". The host, the
// kernel and the CPU model (NWEngine's ScoreStats) all take the rule from
// here.
inline constexpr int32_t kPoaScoreFloor = -28000;
inline constexpr int32_t kPoaScoreFloorBanded = -27000;  // banded rows mark out-of-band
                                                         // cells with values below the floor

constexpr int32_t poa_abs(int32_t v) { return v < 0 ? -v : v; }
constexpr int32_t poa_max(int32_t a, int32_t b) { return a > b ? a : b; }

// the class-wide guard: (max_nodes + matrix_width) * max(|m|,|x|,|g|) within
// the floor
constexpr bool poa_scores_fit_worst_case(const PoaLimits& l, int32_t m, int32_t x, int32_t g,
                                         bool banded) {
  const int32_t worst = static_cast<int32_t>(l.max_nodes + l.matrix_width) *
                        poa_max(poa_abs(m), poa_max(poa_abs(x), poa_abs(g)));
  return worst <= -(banded ? kPoaScoreFloorBanded : kPoaScoreFloor);
}

// Static part of the score check. Gaps cost something, so that a run of
// horizontal gaps from column 0 bounds every cell of a row from below; and no
// score exceeds the layer length (at most matrix_width - 1 columns) times the
// best per-column gain.
constexpr bool poa_score_check_static(int32_t m, int32_t x, int32_t g, uint32_t matrix_width) {
  return g < 0 && poa_max(poa_max(m, x), 0) * static_cast<int32_t>(matrix_width - 1) <=
                      -kPoaScoreFloor;
}

// Per-row part: h0 is the row's column-0 score, len the layer's length. No
// cell of the row is below h0 + len * g, so a row that passes stores no
// clamped score. Conservative: a refused row need not hold a cell that low.
constexpr bool poa_score_row_refused(int32_t h0, uint32_t len, int32_t g) {
  return h0 + static_cast<int32_t>(len) * g < kPoaScoreFloor;
}
static_assert(poa_score_check_static(27, -20, -13, 1024) &&
              !poa_score_check_static(28, -20, -13, 1024) &&
              !poa_score_check_static(3, -5, 0, 1024));
static_assert(!poa_score_row_refused(-14000, 500, -28) && poa_score_row_refused(-14500, 500, -29));

// ---- lean single-predecessor rows ----
// The 8-wide unchecked kernels of the regular class compute a row with exactly
// one in-edge, whose source row is in the LDS ring, on packed int16 pairs
// (poa_kernel.hip, dp_row_lean; docs/DESIGN.md, "Lean rows"). A lean row is a
// single pass, so its columns stop at kPoaLeanMaxLen. What it holds in 16 bits:
//   stored scores          [kPoaScoreFloor, -kPoaScoreFloor]   (floor clamp,
//                          constructor guard)
//   candidates, v, h       one score parameter more on either side
//   u-space values         v - j * g, j <= kPoaLeanMaxLen
// The row has no "no cell" value of its own: its one predecessor row is
// complete, and the wave scan, which has one, runs on 32 bits. So the
// condition is that the largest u-space value fits, with a negative gap, which
// is what the direction of the u-space argument (u >= v, junk columns only
// feed higher columns) is written for. Every parameter set that passes the
// worst-case guard with a negative gap passes it (28000 + 9 + 512 * 9 =
// 32617); a batch that fails it runs every row through dp_row.
inline constexpr uint32_t kPoaLeanMaxLen = 512;
constexpr bool poa_lean_rows_fit(int32_t m, int32_t x, int32_t g) {
  return g < 0 && -kPoaScoreFloor + poa_max(poa_abs(m), poa_max(poa_abs(x), poa_abs(g))) +
                          static_cast<int32_t>(kPoaLeanMaxLen) * poa_abs(g) <=
                      32767;
}
static_assert(poa_lean_rows_fit(3, -5, -4) && poa_lean_rows_fit(5, -4, -8) &&
              poa_lean_rows_fit(3, -8, -4) && poa_lean_rows_fit(9, -9, -9) &&
              !poa_lean_rows_fit(3, -5, 0) && !poa_lean_rows_fit(3, -5, -10));

// ---- kernel variants ----
// The kernel is instantiated once per row of kPoaVariants (times timed /
// untimed). The enum's numeric order is the order a batch's windows are
// sorted and launched in.
enum PoaVariant : uint32_t {
  kPoaNarrow = 0,      // rows <= 320 columns, single 5-wide pass
  kPoaMid = 1,         // the hot one: default w=500 windows of moderate depth
  kPoaFull = 2,        // anything else at full width
  kPoaBandedMid = 3,   // banded rows in a mid-width ring
  kPoaBandedFull = 4,  // banded rows in a full-width ring
  kPoaNumVariants
};

struct PoaVariantParams {
  uint32_t cols_per_lane;  // columns a lane owns per pass
  uint32_t ring_width;     // LDS DP-row ring width; rows need max_len + 1
  uint32_t node_cap;       // LDS Kahn capacity; the graph holds node_cap - 1
  uint32_t min_waves;      // waves/SIMD the compiler budgets registers for
};

// The large class has one kernel variant, full width, taking banded rows at
// run time as kPoaFull does. LDS: the Kahn side is 5 B per node, 20 KiB,
// which is 8 workgroups per CU, two waves per SIMD.
inline constexpr PoaVariantParams kPoaLargeVariant = {8, kPoaLargeLimits.matrix_width,
                                                      kPoaLargeLimits.max_nodes + 1, 2};
static_assert(5 * kPoaLargeVariant.node_cap * (4 * kPoaLargeVariant.min_waves) <= 160 * 1024,
              "the large variant's Kahn side must leave min_waves waves per SIMD resident");

inline constexpr PoaVariantParams kPoaVariants[kPoaNumVariants] = {
    {5, 384, kPoaLimits.max_nodes + 1, 4},                      // kPoaNarrow
    {8, 576, 1536, 5},                                          // kPoaMid
    {8, kPoaLimits.matrix_width, kPoaLimits.max_nodes + 1, 4},  // kPoaFull
    {5, 576, kPoaLimits.max_nodes + 1, 4},                      // kPoaBandedMid
    {5, kPoaLimits.matrix_width, kPoaLimits.max_nodes + 1, 4},  // kPoaBandedFull
};

// Variant for a window whose longest layer has max_len bases. The LDS ring
// is indexed by ABSOLUTE column, so its width follows the true longest row
// (max_len); only the columns-per-pass choice follows the banded clamp.
// 9-wide single-pass was tried and spills 44-64 B/lane of scratch, which is
// catastrophically slow; 8-wide multi-pass covers any width, and the ring
// width picks the smallest LDS footprint the rows fit in.
constexpr PoaVariant poa_route(uint32_t max_len, uint32_t num_seqs, uint32_t band_width) {
  uint32_t pass_w = max_len;
  if (band_width != 0 && band_width + 64 < pass_w) {
    pass_w = band_width + 64;
  }
  const bool narrow_pass = pass_w <= 320;
  if (max_len <= 320) return kPoaNarrow;
  if (max_len <= 575) {
    if (narrow_pass) return kPoaBandedMid;
    // deep windows can outgrow the smaller node cap; route them to the
    // full variant instead of bouncing via the CPU
    return num_seqs <= 96 ? kPoaMid : kPoaFull;
  }
  return narrow_pass ? kPoaBandedFull : kPoaFull;
}

static_assert(poa_route(320, 12, 0) == kPoaNarrow && poa_route(321, 12, 0) == kPoaMid);
static_assert(poa_route(575, 12, 0) == kPoaMid && poa_route(576, 12, 0) == kPoaFull);
static_assert(poa_route(500, 96, 0) == kPoaMid && poa_route(500, 97, 0) == kPoaFull);
static_assert(poa_route(320, 12, 256) == kPoaNarrow && poa_route(321, 12, 256) == kPoaBandedMid);
static_assert(poa_route(575, 97, 256) == kPoaBandedMid &&
              poa_route(576, 12, 256) == kPoaBandedFull);

// every window is routed to a ring its rows fit in (the condition the
// kernel's kPoaWidthOverflow guards)
constexpr bool poa_routes_fit() {
  for (uint32_t len = 0; len < kPoaLimits.matrix_width; ++len) {
    for (uint32_t num_seqs : {1u, 96u, 97u}) {
      for (uint32_t bw : {0u, 256u}) {
        if (len + 1 > kPoaVariants[poa_route(len, num_seqs, bw)].ring_width) return false;
      }
    }
  }
  return true;
}
static_assert(poa_routes_fit());

// Per-window input descriptor (layers already sorted: backbone first, then
// by window start position — the same order as the CPU path).
struct PoaWindowDesc {
  uint32_t seq_offset;   // byte offset into the packed seq/weight arena
  uint32_t num_seqs;     // layers shipped to the device (<= max depth + 1)
  uint32_t scratch_idx;  // which device slab this window uses
  uint32_t max_len;      // longest layer (columns) — with num_seqs, picks the
                         // kernel variant (poa_route)
};

// ---- per-window scratch slabs ----
// X(element type, name, elements per window), in allocation order; N is
// max_nodes and L the capacity model. This is the one statement of the slab
// layout: the pointer struct, the size estimate, the host carve and the
// kernel's per-window pointers are all expansions of it.
//   nseq      sequences touching the node (coverage)
//   rank      node -> rank (Kahn scratch/queue and the topological order
//             itself live in LDS)
//   hb_*      heaviest-bundle running scores / predecessors
//   aln_nodes per sequence position: aligned node or -1 (traceback output)
//   aln_seq   per sequence position: the node id it was threaded to
//             (add_alignment_d); both use the first max layer length entries
//   matrix    DP scores
//   moves     DP move bytes: bits 0-1 {0=diag,1=up,2=left,3=invalid},
//             bits 2-7 in-edge index of the chosen predecessor
//   row_desc  per-rank packed row descriptor, built lane-parallel after each
//             topo sort: letter(8) | nin(8) | node(16) | pred_row(16) | flags(8)
//   row_desc2 per-rank second descriptor word, built in the same pass: the DP
//             rows (rank + 1) of the sources of in-edges 1, 2, 3 and 4, 16
//             bits each, 0 where the node has no such edge (a predecessor's
//             row is never 0)
#define RGA_POA_SLAB_ARRAYS(X)                   \
  X(uint8_t, letters, N)                         \
  X(uint8_t, in_cnt, N)                          \
  X(uint8_t, out_cnt, N)                         \
  X(uint8_t, ring_cnt, N)                        \
  X(uint16_t, in_edges, N * L.max_edges)         \
  X(int32_t, in_weights, N * L.max_edges)        \
  X(uint16_t, out_edges, N * L.max_edges)        \
  X(uint16_t, ring, N * L.max_ring)              \
  X(uint16_t, nseq, N)                           \
  X(uint16_t, rank, N)                           \
  X(int64_t, hb_score, N)                        \
  X(int32_t, hb_pred, N)                         \
  X(int32_t, aln_nodes, 2 * L.matrix_width + N)  \
  X(int32_t, aln_seq, 2 * L.matrix_width + N)    \
  X(int16_t, matrix, (N + 1) * L.matrix_width)   \
  X(uint8_t, moves, (N + 1) * L.matrix_width)    \
  X(uint64_t, row_desc, N)                       \
  X(uint64_t, row_desc2, N)

struct PoaSlabs {
#define RGA_X(T, name, count) T* name;
  RGA_POA_SLAB_ARRAYS(RGA_X)
#undef RGA_X
};

// calls f(pointer member, elements per window) for every slab array of the
// capacity class, in allocation order
template <bool LARGE = false, class F>
constexpr void for_each_poa_slab(PoaSlabs& s, F&& f) {
  constexpr PoaLimits L = poa_limits(LARGE);
  constexpr size_t N = L.max_nodes;
#define RGA_X(T, name, count) f(s.name, static_cast<size_t>(count));
  RGA_POA_SLAB_ARRAYS(RGA_X)
#undef RGA_X
}

constexpr size_t kPoaTimingSlots = 8;
// Timing slot 7 carries three counts, so that the slab layout stays what it
// was: layers processed in bits 0..15, DP rows taken by the lean row in bits
// 16..39 and DP rows in all in bits 40..63 (a window has at most 200 layers of
// at most 4095 rows).
constexpr unsigned long long poa_pack_counts(unsigned long long layers, unsigned long long lean,
                                             unsigned long long rows) {
  return layers | (lean << 16) | (rows << 40);
}
constexpr unsigned long long poa_count_layers(unsigned long long w) { return w & 0xffffu; }
constexpr unsigned long long poa_count_lean_rows(unsigned long long w) {
  return (w >> 16) & 0xffffffu;
}
constexpr unsigned long long poa_count_rows(unsigned long long w) { return w >> 40; }

// device scratch bytes one window needs (unrounded; sizes the batch)
template <bool LARGE = false>
constexpr size_t poa_slab_bytes() {
  PoaSlabs s{};
  size_t b = kPoaTimingSlots * sizeof(unsigned long long);
  for_each_poa_slab<LARGE>(s, [&b](auto* p, size_t count) { b += count * sizeof(*p); });
  return b;
}
static_assert(poa_slab_bytes() == 7200396, "slab layout changed: batch sizes move with it");
static_assert(poa_slab_bytes<true>() == 14384780,
              "large slab layout changed: the large pool's size moves with it");

// Device arena pointers (one allocation, carved into slabs).
struct PoaDeviceArena {
  // inputs (packed tight, H2D once per batch)
  const uint8_t* seq_data;     // concatenated layer bases
  const uint8_t* weight_data;  // matching per-base weights
  const uint32_t* layer_ends;  // per layer: end offset within window's span
  // per layer: backbone span driving the SUBGRAPH-restricted alignment
  // (begin << 16 | inclusive end; 0xFFFFFFFF = spans the window, full DP).
  // CPU parity: layers not reaching within 1% of both window edges align
  // against a subgraph of their backbone range (Window::generate_consensus);
  // the device restricts DP rows to the [rank(begin), rank(end)] window —
  // a capability the reference's cudapoa lacks (it aligns every layer to
  // the full graph, which is what degrades its w=1000 GPU goldens).
  const uint32_t* layer_spans;
  const uint32_t* layer_ends_index;  // per window: first index into layer_ends
  const PoaWindowDesc* windows;

  // per-window graph slabs (device scratch, indexed by scratch_idx)
  PoaSlabs slabs;

  // per-window phase timing (wall_clock64 deltas; slots: 0 DP rows,
  // 1 traceback, 2 add_alignment, 3 topo sort, 4 row_desc, 5 consensus,
  // 6 total, 7 layers processed) — aggregated by the host under
  // RGA_POA_TIMING for kernel-phase attribution
  unsigned long long* timing;  // [kPoaTimingSlots] per window

  // outputs (D2H once per batch)
  uint8_t* consensus;       // [max_consensus] per window, forward order
  uint16_t* coverage;       // [max_consensus] per window
  uint32_t* consensus_len;  // [1] per window
  int32_t* status;          // [1] per window
  uint32_t* num_nodes;      // [1] per window: graph size at the end; stays on
                            // the device unless PoaBatch::read_graph asks

  int8_t match, mismatch, gap;
  // 1: eligible rows take the lean row (poa_lean_rows_fit holds and the batch
  // has not switched it off). In the padding behind gap: the struct's size and
  // the other members' offsets are what they were.
  uint8_t lean_rows;
  uint32_t band_width;  // 0 = full-width DP; else static band (reference -b:
                        // BatchConfig band 256, src/cuda/cudabatch.cpp:56-59)
};

// Launches the kernel variant for windows [window_base, window_base +
// num_windows) of the (variant-sorted) desc array.
void launch_poa_kernel(const PoaDeviceArena& arena, uint32_t window_base,
                       uint32_t num_windows, PoaVariant variant, void* stream);

// The same for an arena of large-class slabs (kPoaLargeLimits), which has
// the one variant kPoaLargeVariant.
void launch_poa_kernel_large(const PoaDeviceArena& arena, uint32_t window_base,
                             uint32_t num_windows, void* stream);

// The same two with the per-row score check compiled in (poa_kernel_checked.hip,
// poa_kernel_large_checked.hip): a window that trips it ends with
// kPoaScoreRange. Unbanded rows only: arena.band_width must be 0, so the
// variant is never one of the banded ones.
void launch_poa_kernel_checked(const PoaDeviceArena& arena, uint32_t window_base,
                               uint32_t num_windows, PoaVariant variant, void* stream);
void launch_poa_kernel_large_checked(const PoaDeviceArena& arena, uint32_t window_base,
                                     uint32_t num_windows, void* stream);

}  // namespace rga::hip
