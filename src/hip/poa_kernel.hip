// HIP/CDNA4 POA mega-kernel v3: one 64-lane wavefront per window.
//
// Per window it loops over the layers: Needleman-Wunsch of the layer against
// the current POA graph (rows = graph nodes in topological order, columns =
// layer bases; the horizontal gap pass is a wave-wide max-scan with slope),
// move-byte traceback, threading the alignment into the graph, Kahn
// topological re-sort, and finally heaviest-bundle consensus with per-base
// coverage.
//
// Perf lineage. v1 streamed every DP value through HBM: 85% of wave-cycles
// parked on memory (measured, profiles/). v2 mirrored the graph arrays into
// 31 KB of LDS, which fixed the DP stalls but capped co-residency at 5
// blocks/CU — the still-global serial phases could no longer be hidden and
// wall time got worse. v3 keeps only the DP essentials in LDS (4-row ring +
// layer bases, 9 KB -> ~16 blocks/CU): predecessor rows are LDS hits unless
// the rank distance exceeds the ring (rare bubbles -> global matrix), the
// per-row scalar pointer-chase (sorted -> letter/in-count/first-edge ->
// pred rank) is replaced by two packed u64 words per rank (`row_desc`,
// `row_desc2`: the row's letter, in-count, node, flags and the rows of its
// first five predecessors) built LANE-PARALLEL after each topological sort,
// and the DP records a move byte per cell — on rows with several
// predecessors the chosen edge falls out of a keyed maximum — so the serial
// traceback is one byte load per step. The graph
// phases stay in global memory and are hidden by the deep window
// co-residency, as in v1. Threading the path into the graph
// (add_alignment_d) handles 64 sequence positions per step. The traceback
// and the Kahn FIFO, whose order is the result, keep that order but no
// longer wait for global memory step by step: the traceback reads 64 moves
// of the predicted path per round trip on all lanes (traceback_d), and the
// FIFO core, still on lane 0, runs from an LDS copy of the adjacency
// (topo_sort_d).
//
// Semantics mirror the CPU engine (src/align/poa.cpp) so GPU results are
// deterministic and window-content-only (reference racon-gpu pins separate
// GPU goldens; so do we — topological order here is Kahn FIFO, not spoa DFS).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "hip/poa_types.hpp"

namespace rga::hip {

namespace {

constexpr int kLanes = 64;
constexpr int32_t kNegInf = -(1 << 28);
// Capacity class of this translation unit. The source is compiled once per
// class: as it stands for the regular one (kPoaLimits), and through
// poa_kernel_large.hip, which defines RGA_POA_LARGE_CLASS and includes this
// file, for the large one (kPoaLargeLimits). Everything below is inside the
// unnamed namespace, so the two copies do not meet; only the launch function
// at the end has a name per class.
#ifdef RGA_POA_LARGE_CLASS
constexpr bool kLarge = true;
#else
constexpr bool kLarge = false;
#endif
// The per-row score check (poa_types.hpp, poa_score_row_refused) is a template
// flag of the kernel, CHECKED next to TIMED. The checked instantiations live
// in translation units of their own (poa_kernel_checked.hip and
// poa_kernel_large_checked.hip define RGA_POA_SCORE_CHECK and include this
// file), so that the unchecked ones compile as they did before the check
// existed and the four units build side by side.
#ifdef RGA_POA_SCORE_CHECK
constexpr bool kChecked = true;
#else
constexpr bool kChecked = false;
#endif
constexpr PoaLimits kL = poa_limits(kLarge);
constexpr uint32_t kMaxW = kL.matrix_width;   // DP row width (slab and widest ring)
constexpr uint32_t kMaxN = kL.max_nodes + 1;  // widest LDS Kahn arrays
constexpr uint32_t kMaxE = kL.max_edges;
constexpr uint32_t kMaxR = kL.max_ring;
constexpr uint32_t kRing = 4;     // DP rows kept in LDS
constexpr uint32_t kMaxPre = 5;   // predecessor rows carried by the row descriptors
// Minus infinity of a multi-predecessor row, whose candidates are compared as
// (score << 6 | edge priority) keys: far below every real score (|score| <
// 2^18 before the clamp) and still clear of overflow after the shift.
// The scaled scores stay above it under either guard. A predecessor value is
// a stored one, so at least kPoaScoreFloor and, by either guard, at most
// 28000 in magnitude; a candidate adds one score parameter, an int8, to it:
// (28000 + 127) * 64 = 1800128 < 2^21 = 2097152. With the score check
// (CHECKED) a parameter may reach 127 where the worst-case guard stopped at 9,
// and the bound is the same one.
constexpr int32_t kNegInfKeyed = -(1 << 21);
static_assert((-kPoaScoreFloor + 127) * 64 < -kNegInfKeyed);

// move byte encoding
constexpr uint8_t kMvDiag = 0;
constexpr uint8_t kMvUp = 1;
constexpr uint8_t kMvLeft = 2;  // (value 3 is reserved/invalid)

// Single-wavefront LDS visibility: waits only the LDS (lgkm) counter and
// stops compiler reordering. Unlike __syncthreads(), it does NOT drain the
// outstanding global (vm) stores of the row just written — those are
// fire-and-forget into HBM and must not sit on the per-row critical path.
__device__ inline void wave_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// Inclusive max-scan over the 64-lane wavefront via DPP row ops (VALU-speed;
// the naive __shfl_up chain is 6 dependent ds_bpermute round-trips through
// the LDS unit and dominated the DP phase — measured with RGA_POA_TIMING).
// Sequence: shr1/2/4/8 within 16-lane rows, then bcast15 into rows 1&3 and
// bcast31 into rows 2&3 (the classic GCN prefix idiom with max).
__device__ inline int32_t wave_scan_max(int32_t v) {
  int32_t t;
  t = __builtin_amdgcn_update_dpp(kNegInf, v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v = max(v, t);
  t = __builtin_amdgcn_update_dpp(kNegInf, v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v = max(v, t);
  t = __builtin_amdgcn_update_dpp(kNegInf, v, 0x114, 0xf, 0xf, false);  // row_shr:4
  v = max(v, t);
  t = __builtin_amdgcn_update_dpp(kNegInf, v, 0x118, 0xf, 0xf, false);  // row_shr:8
  v = max(v, t);
  t = __builtin_amdgcn_update_dpp(kNegInf, v, 0x142, 0xa, 0xf, false);  // row_bcast:15
  v = max(v, t);
  t = __builtin_amdgcn_update_dpp(kNegInf, v, 0x143, 0xc, 0xf, false);  // row_bcast:31
  v = max(v, t);
  return v;
}

// chunk range [klo, khi] of the static band for DP row R (1-based):
// center column follows the rank diagonal via a 16.16 slope; the band is
// rounded out to whole 64-column chunks (>= bw coverage). Full-width mode
// (bw == 0) is the caller's fast path and never calls this.
__device__ inline void band_chunks(uint32_t R, uint32_t slope16, uint32_t bw, uint32_t chunks,
                                   uint32_t* klo, uint32_t* khi) {
  const uint32_t center = (static_cast<uint64_t>(R) * slope16) >> 16;
  const uint32_t jlo = center > bw / 2 ? center - bw / 2 : 0;
  uint32_t lo = (jlo == 0) ? 0 : (jlo - 1) / 64;
  if (lo > chunks - 1) lo = chunks - 1;
  uint32_t hi = lo + bw / 64;
  if (hi > chunks - 1) hi = chunks - 1;
  *klo = lo;
  *khi = hi;
}

// packed row descriptor (one per topological rank); flags: bit0 = end node
// (no out-edges), bit1 = some successor is beyond the LDS ring, so this
// row's scores must go to global memory (matrix rows are otherwise
// write-only traffic nobody reads — the dominant HBM cost of the DP).
constexpr uint64_t kRdEnd = 1;
constexpr uint64_t kRdStore = 2;

__device__ inline uint64_t pack_rd(uint8_t letter, uint8_t nin, uint16_t node,
                                   uint16_t pred_row, uint8_t flags) {
  return static_cast<uint64_t>(letter) | (static_cast<uint64_t>(nin) << 8) |
         (static_cast<uint64_t>(node) << 16) | (static_cast<uint64_t>(pred_row) << 32) |
         (static_cast<uint64_t>(flags) << 48);
}

// Second descriptor word (slab row_desc2): the DP rows of the sources of
// in-edges 1..kMaxPre-1, 16 bits each, 0 where there is no such edge. With
// in-edge 0's row in the first word, a row with up to kMaxPre predecessors
// finds all their rows in two wave-uniform registers; only in-edges from
// kMaxPre on are looked up in the graph arrays (pred_row_of).
static_assert(kMaxPre == 5, "row_desc2 holds four 16-bit rows");

// Kahn out-adjacency word (Shared::kahn.adj): first out-edge target in the
// low 11 bits (node ids stop at max_nodes - 1 < 2048), out-degree above it,
// saturating at kAdjSat (a saturated word sends the FIFO to out_cnt).
// The large class needs a twelfth bit of node id and takes it from the
// degree, 12 + 4 saturating at 15, so the word stays 16 bits: a 32-bit word
// would grow the kahn side from 20 to 28 KiB and cost three of the eight
// resident workgroups per CU, while a node with 15 or more out-edges only
// costs the FIFO one more global load.
constexpr uint32_t kAdjBits = kLarge ? 12 : 11;
constexpr uint32_t kAdjMask = (1u << kAdjBits) - 1;
constexpr uint32_t kAdjSat = (1u << (16 - kAdjBits)) - 1;
static_assert(kAdjSat == (kLarge ? 15u : 31u));
static_assert(kL.max_nodes <= kAdjMask + 1, "node id does not fit the adjacency word");

// LDS block state — cross-batch window co-residency is the dominant
// throughput lever (a 19 KB variant with full graph-array mirrors made each
// window ~10% faster but halved residency and lost 20% end to end), so the
// block is ONE union whose sides are the phases of a layer, which never
// overlap in time:
//   dp    the DP row ring, the layer's match bitvectors and the staged row
//         descriptors;
//   tb    the traceback's first-predecessor table;
//   kahn  the topological sort's in-degree scratch, FIFO queue and packed
//         out-adjacency, so that the serial FIFO touches global memory only
//         for nodes with two or more out-edges.
// The budget is what the register-limited occupancy leaves per block, not
// what the DP needs: 160 KiB / (4 SIMDs * min_waves) is 8 KiB for the mid
// variant (5 waves) and 10 KiB for the others (4 waves), and the kahn side
// (5 bytes per node of capacity) fills exactly that. Growing any side past
// it costs residency, which is the 31 KB experiment again.
//
// Aliasing rules. A block is one wavefront, and its LDS accesses complete in
// program order, so a side is dead as soon as the code that reads it is
// behind: the barriers below only stop the compiler from moving accesses
// across a phase boundary and make a phase's writes visible to all lanes.
//   dp   -> tb:   pred0 is staged after the last row's trailing
//                 wave_lds_sync; nothing of the ring is read afterwards.
//   tb   -> kahn: traceback_d has returned, and add_alignment_d between
//                 them uses no LDS.
//   kahn -> dp:   match is rebuilt at the top of every layer
//                 (build_match_bits_d, closed by __syncthreads) and rd_block
//                 before every 64 rows (closed by wave_lds_sync); the ring
//                 rows are written before they are read, as ever. The rank
//                 write-back that reads the queue is closed by
//                 __syncthreads inside topo_sort_d.
// The queue doubles as the topological order read by consensus_d: the last
// thing a window's layer loop runs is a topological sort, and a layer that
// is skipped touches no LDS. Everything else stays in the global slabs,
// hidden by co-residency.
//
// The ring width W and the node capacity MN are template parameters: the
// kernel is instantiated per row of kPoaVariants.
template <uint32_t W, uint32_t MN>
struct alignas(16) Shared {
  union {
    struct {
      int16_t ring[kRing][W];  // DP rows (slot = row % kRing)
      // per-layer match bitvectors: bit l of match[c][k] says layer base
      // (1 + k*64 + l) equals code c — turns the per-cell seq comparison into
      // one register bit test instead of a byte load. One spare word so
      // cross-word extraction at the last chunk never reads out of bounds.
      uint64_t match[4][W / 64 + 1];
      uint64_t rd_block[64];   // row descriptors staged 64 at a time
      uint64_t rd2_block[64];  // ... and their second words (row_desc2)
    } dp;
    struct {
      // per DP row: the row of in-edge 0's source, 0 for virtual row 0
      uint16_t pred0[MN];
    } tb;
    struct {
      uint8_t work[MN];    // Kahn in-degree scratch (in-degree < 256)
      uint16_t queue[MN];  // Kahn FIFO == topological order
      uint16_t adj[MN];    // first out-edge | out-degree << kAdjBits
    } kahn;
  } u;
};

__device__ inline int32_t poa_code(uint8_t b) {
  switch (b) {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    case 'T': return 3;
    default: return -1;
  }
}

// this window's slab pointers plus its inputs and running graph state
struct WindowCtx : PoaSlabs {
  const uint8_t* seq_base;
  const uint8_t* weight_base;
  const uint32_t* ends;   // layer end offsets (relative to window start)
  const uint32_t* spans;  // per layer: begin<<16|end backbone span, or
                          // 0xFFFFFFFF for window-spanning layers (full DP)
  uint32_t num_seqs;

  uint32_t MN;  // node cap of the launched variant
  int32_t m, x, g;

  uint32_t num_nodes;
  uint32_t seqs_in_graph;
  int32_t status;
};

// ---------- graph helpers ----------

__device__ inline uint16_t out_edge_of(const WindowCtx& c, uint32_t node, uint32_t e) {
  return c.out_edges[node * kMaxE + e];
}

// Adds weight w to edge a -> b, appending the edge when it is new. One lane
// per edge; returns kPoaOk or kPoaEdgeOverflow.
__device__ inline int32_t add_edge_d(const WindowCtx& c, uint32_t a, uint32_t b, int32_t w) {
  const uint32_t n_out = c.out_cnt[a];
  for (uint32_t e = 0; e < n_out; ++e) {
    if (out_edge_of(c, a, e) == b) {
      const uint32_t n_in = c.in_cnt[b];
      for (uint32_t f = 0; f < n_in; ++f) {
        if (c.in_edges[b * kMaxE + f] == a) {
          c.in_weights[b * kMaxE + f] += w;
          break;
        }
      }
      return kPoaOk;  // a miss is unreachable for a consistent graph
    }
  }
  const uint32_t n_in = c.in_cnt[b];
  if (n_out >= kMaxE || n_in >= kMaxE) {
    return kPoaEdgeOverflow;
  }
  c.out_edges[a * kMaxE + n_out] = static_cast<uint16_t>(b);
  c.out_cnt[a] = static_cast<uint8_t>(n_out + 1);
  c.in_edges[b * kMaxE + n_in] = static_cast<uint16_t>(a);
  c.in_weights[b * kMaxE + n_in] = w;
  c.in_cnt[b] = static_cast<uint8_t>(n_in + 1);
  return kPoaOk;
}

// First non-zero status of any lane (wave-uniform), kPoaOk when all are.
__device__ inline int32_t wave_first_status(int32_t status) {
  const uint64_t bad = __ballot(status != kPoaOk);
  return bad == 0 ? kPoaOk : __shfl(status, __ffsll(static_cast<long long>(bad)) - 1, kLanes);
}

// Threads the traceback path into the graph, 64 sequence positions at a
// time. Call from ALL lanes. Mirrors Graph::add_alignment (src/align/poa.cpp)
// and builds element for element the graph its serial walk builds.
//
// Input: aln_nodes[p] = graph node sequence position p is aligned to, or -1
// for an insertion (traceback_d). The traceback always runs from column len
// to (0,0), so every position 0..len-1 has its entry: a layer with no
// aligned position at all (the head/tail chains of the CPU code) cannot
// reach this function, its positions are all insertions against row 0.
//
// Sweep A resolves position p to a node id — the aligned node when the
// letter matches, a ring partner with that letter, else a new node — and
// leaves it in aln_seq[p]. New ids are num_nodes + the number of earlier new
// positions (ballot/popcount inside a block, running base across blocks),
// which is the order the serial walk hands them out in. Sweep B gives lane p
// the edge id[p-1] -> id[p] and the coverage count of id[p].
//
// No atomics, because no two lanes write the same element. The alignment
// path is a path in the DAG, so its nodes are mutually reachable, while the
// members of one aligned ring are mutually unreachable: a new member is hung
// between the path predecessor and successor of the node it aligns to, and
// later edges only connect pairs that were already reachable. Hence the
// positions of one layer touch pairwise different rings (ring, ring_cnt:
// one writer per ring), the resolved ids are pairwise different, and every
// id is the source of exactly one edge and the target of exactly one
// (out_edges/out_cnt of id[p-1] and in_edges/in_cnt/in_weights/nseq of id[p]
// belong to lane p alone).
//
// Any overflow is terminal for the window (the layer loop stops and the
// window goes to the CPU), so the graph left behind by a failing call is
// unspecified; only "fails whenever the serial walk would" is kept.
__device__ void add_alignment_d(WindowCtx& c, const uint8_t* seq, const uint8_t* wts,
                                uint32_t len, int lane) {
  int32_t status = kPoaOk;
  uint32_t next_id = c.num_nodes;

  // ---- sweep A: position -> node id ----
  for (uint32_t blk = 0; blk < len; blk += kLanes) {
    const uint32_t p = blk + lane;
    const bool active = p < len;
    uint8_t letter = 0;
    int32_t node = -1;
    int32_t id = -1;
    uint32_t nr = 0;
    if (active) {
      letter = seq[p];
      node = c.aln_nodes[p];
      if (node != -1) {
        if (c.letters[node] == letter) {
          id = node;
        } else {
          nr = c.ring_cnt[node];
          for (uint32_t r = 0; r < nr; ++r) {
            const uint16_t aid = c.ring[node * kMaxR + r];
            if (c.letters[aid] == letter) {
              id = aid;
              break;
            }
          }
        }
      }
    }
    const bool is_new = active && id == -1;
    const uint64_t new_mask = __ballot(is_new);
    if (is_new) {
      const uint32_t nid = next_id + __popcll(new_mask & ((1ull << lane) - 1));
      id = static_cast<int32_t>(nid);
      if (nid >= c.MN) {
        status = kPoaNodeOverflow;
      } else {
        c.letters[nid] = letter;
        c.in_cnt[nid] = 0;
        c.out_cnt[nid] = 0;
        c.ring_cnt[nid] = 0;
        c.nseq[nid] = 0;
        if (node != -1) {
          // join the ring: new node linked with node and all its partners
          if (nr >= kMaxR) {
            status = kPoaRingOverflow;
          } else {
            for (uint32_t r = 0; r < nr; ++r) {
              const uint16_t aid = c.ring[node * kMaxR + r];
              c.ring[nid * kMaxR + r] = aid;
              const uint32_t arc = c.ring_cnt[aid];
              if (arc >= kMaxR) {
                status = kPoaRingOverflow;
                break;
              }
              c.ring[aid * kMaxR + arc] = static_cast<uint16_t>(nid);
              c.ring_cnt[aid] = static_cast<uint8_t>(arc + 1);
            }
            c.ring[nid * kMaxR + nr] = static_cast<uint16_t>(node);
            c.ring_cnt[nid] = static_cast<uint8_t>(nr + 1);
            c.ring[node * kMaxR + nr] = static_cast<uint16_t>(nid);
            c.ring_cnt[node] = static_cast<uint8_t>(nr + 1);
          }
        }
      }
    }
    next_id += __popcll(new_mask);
    if (active) {
      c.aln_seq[p] = id;
    }
  }
  status = wave_first_status(status);
  if (status != kPoaOk) {
    c.status = status;
    return;
  }
  c.num_nodes = next_id;
  __syncthreads();  // ids and new nodes -> visible to the lanes of sweep B

  // ---- sweep B: edges id[p-1] -> id[p], coverage ----
  // (a one-base layer has no edge and, as in the serial walk, counts nowhere)
  if (len >= 2) {
    for (uint32_t blk = 0; blk < len; blk += kLanes) {
      const uint32_t p = blk + lane;
      if (p < len) {
        const uint32_t b = static_cast<uint32_t>(c.aln_seq[p]);
        ++c.nseq[b];
        if (p != 0 && status == kPoaOk) {
          const uint32_t a = static_cast<uint32_t>(c.aln_seq[p - 1]);
          status = add_edge_d(c, a, b, static_cast<int32_t>(wts[p - 1]) + wts[p]);
        }
      }
    }
    status = wave_first_status(status);
    if (status != kPoaOk) {
      c.status = status;
      return;
    }
  }
  ++c.seqs_in_graph;
}

// Kahn topological sort (FIFO, deterministic) over the LDS mirrors. The
// FIFO queue IS the final topological order (s.u.kahn.queue); rank goes to
// the global slab (read lane-parallel by build_row_desc).
// Cooperative: the staging, the queue seeding and the rank writeback are
// lane-parallel; only the FIFO core (whose order is the deterministic
// topological order) stays on lane 0. Call from ALL lanes.
//
// The FIFO's chain of dependent reads stays in LDS on the common path: the
// staging leaves, next to the in-degrees, one word per node with its first
// out-edge and its out-degree (Shared::kahn.adj), loaded 64 nodes at a time
// with independent loads. A node with at most one out-edge then costs the
// FIFO no global access at all; a node with more reads the rest of its edge
// row eight edges per 16-byte load, and those loads do not wait for out_cnt.
// The pop order is the serial one: sources by ascending id, then every
// node's out-edges in list order.
template <class SH>
__device__ void topo_sort_d(WindowCtx& c, SH& s, int lane) {
  const uint32_t n = c.num_nodes;
  // staging + seeding: the sources of a 64-node block go to the queue behind
  // those of the blocks before it, in lane (= id) order
  uint32_t qtail = 0;
  for (uint32_t blk = 0; blk < n; blk += kLanes) {
    const uint32_t i = blk + lane;
    bool source = false;
    if (i < n) {
      const uint32_t nin = c.in_cnt[i];
      const uint32_t nout = c.out_cnt[i];
      const uint32_t first = c.out_edges[i * kMaxE];  // unused when nout == 0
      s.u.kahn.work[i] = static_cast<uint8_t>(nin);
      s.u.kahn.adj[i] = static_cast<uint16_t>(
          nout == 0 ? 0u : ((first & kAdjMask) | (min(nout, kAdjSat) << kAdjBits)));
      source = nin == 0;
    }
    const uint64_t src_mask = __ballot(source);
    if (source) {
      s.u.kahn.queue[qtail + __popcll(src_mask & ((1ull << lane) - 1))] =
          static_cast<uint16_t>(i);
    }
    qtail += __popcll(src_mask);
  }
  __syncthreads();
  if (lane == 0) {
    constexpr uint32_t kNone = 0xffffffffu;
    uint32_t qhead = 0;
    // the entry at queue[qhead] when it is also the one pushed last: the
    // next pop takes it from here (chain regions: one node in flight)
    uint32_t fwd = kNone;
    auto visit = [&](uint32_t v) {
      const uint8_t left = static_cast<uint8_t>(s.u.kahn.work[v] - 1);
      s.u.kahn.work[v] = left;
      if (left == 0) {
        if (qtail == qhead) {
          fwd = v;
        }
        s.u.kahn.queue[qtail++] = static_cast<uint16_t>(v);
      }
    };
    while (qhead < qtail) {
      const uint32_t u = fwd != kNone ? fwd : s.u.kahn.queue[qhead];
      ++qhead;
      fwd = kNone;
      const uint32_t word = s.u.kahn.adj[u];
      uint32_t nout = word >> kAdjBits;
      if (nout == 0) {
        continue;
      }
      visit(word & kAdjMask);
      if (nout == 1) {
        continue;
      }
      if (nout == kAdjSat) {
        nout = c.out_cnt[u];
      }
      // edge rows are 96 bytes from a 256-byte aligned base: 16-byte loads
      static_assert(kMaxE % 8 == 0 && (kL.max_nodes * kMaxE * 2) % 16 == 0);
      const uint16_t* row = c.out_edges + u * kMaxE;
      for (uint32_t base = 0; base < nout; base += 8) {
        const uint4 v4 = *reinterpret_cast<const uint4*>(row + base);
        const uint32_t ws[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
          const uint32_t e = base + k;
          if (e != 0 && e < nout) {
            visit((ws[k >> 1] >> ((k & 1) * 16)) & 0xffffu);
          }
        }
      }
    }
  }
  __syncthreads();
  for (uint32_t r = lane; r < n; r += kLanes) {
    c.rank[s.u.kahn.queue[r]] = static_cast<uint16_t>(r);
  }
  __syncthreads();  // rank stores -> visible to the cross-lane readers
                    // (build_row_desc, the DP's pred-rank loads)
}

// Heaviest-bundle consensus (mirrors Graph::traverse_heaviest_bundle).
// Returns consensus length written into out/cov (forward order), or -1.
template <class SH>
__device__ int32_t consensus_d(WindowCtx& c, SH& s, uint8_t* out, uint16_t* cov,
                               uint32_t max_out) {
  uint32_t n = c.num_nodes;
  for (uint32_t i = 0; i < n; ++i) {
    c.hb_score[i] = -1;
    c.hb_pred[i] = -1;
  }

  uint32_t max_id = s.u.kahn.queue[0];
  for (uint32_t r = 0; r < n; ++r) {
    uint16_t nid = s.u.kahn.queue[r];
    uint32_t nin = c.in_cnt[nid];
    for (uint32_t e = 0; e < nin; ++e) {
      uint16_t p = c.in_edges[nid * kMaxE + e];
      int64_t w = c.in_weights[nid * kMaxE + e];
      if (c.hb_score[nid] < w ||
          (c.hb_score[nid] == w && c.hb_pred[nid] != -1 &&
           c.hb_score[c.hb_pred[nid]] <= c.hb_score[p])) {
        c.hb_score[nid] = w;
        c.hb_pred[nid] = p;
      }
    }
    if (c.hb_pred[nid] != -1) {
      c.hb_score[nid] += c.hb_score[c.hb_pred[nid]];
    }
    if (c.hb_score[max_id] < c.hb_score[nid]) {
      max_id = nid;
    }
  }

  // branch completion until we end on a sink (bounded: the restart rank is
  // strictly increasing, so at most n rounds; all-zero-weight graphs would
  // otherwise spin forever — those windows fail over to the CPU instead)
  uint32_t guard = 0;
  uint32_t prev_rank = 0;
  while (c.out_cnt[max_id] != 0) {
    if (++guard > n || (guard > 1 && c.rank[max_id] <= prev_rank)) {
      c.status = kPoaConsensusOverflow;
      return -1;
    }
    prev_rank = c.rank[max_id];
    uint32_t rank0 = c.rank[max_id];
    // invalidate alternative branches
    uint32_t nout = c.out_cnt[max_id];
    for (uint32_t e = 0; e < nout; ++e) {
      uint16_t endn = out_edge_of(c, max_id, e);
      uint32_t nin = c.in_cnt[endn];
      for (uint32_t f = 0; f < nin; ++f) {
        uint16_t o = c.in_edges[endn * kMaxE + f];
        if (o != max_id) {
          c.hb_score[o] = -1;
        }
      }
    }
    int64_t best = 0;
    uint32_t best_id = 0;
    for (uint32_t r = rank0 + 1; r < n; ++r) {
      uint16_t nid = s.u.kahn.queue[r];
      c.hb_score[nid] = -1;
      c.hb_pred[nid] = -1;
      uint32_t nin = c.in_cnt[nid];
      for (uint32_t e = 0; e < nin; ++e) {
        uint16_t p = c.in_edges[nid * kMaxE + e];
        if (c.hb_score[p] == -1) {
          continue;
        }
        int64_t w = c.in_weights[nid * kMaxE + e];
        if (c.hb_score[nid] < w ||
            (c.hb_score[nid] == w && c.hb_pred[nid] != -1 &&
             c.hb_score[c.hb_pred[nid]] <= c.hb_score[p])) {
          c.hb_score[nid] = w;
          c.hb_pred[nid] = p;
        }
      }
      if (c.hb_pred[nid] != -1) {
        c.hb_score[nid] += c.hb_score[c.hb_pred[nid]];
      }
      if (best < c.hb_score[nid]) {
        best = c.hb_score[nid];
        best_id = nid;
      }
    }
    max_id = best_id;
  }

  // backtrack: path length first
  int32_t path_len = 0;
  int32_t idw = static_cast<int32_t>(max_id);
  while (idw != -1) {
    ++path_len;
    idw = c.hb_pred[idw];
  }
  if (path_len > static_cast<int32_t>(max_out)) {
    c.status = kPoaConsensusOverflow;
    return -1;
  }
  idw = static_cast<int32_t>(max_id);
  for (int32_t k = path_len - 1; k >= 0; --k) {
    uint32_t node = static_cast<uint32_t>(idw);
    out[k] = c.letters[node];
    uint32_t covv = c.nseq[node];
    uint32_t nr = c.ring_cnt[node];
    for (uint32_t r = 0; r < nr; ++r) {
      covv += c.nseq[c.ring[node * kMaxR + r]];
    }
    cov[k] = static_cast<uint16_t>(min(covv, 65535u));
    idw = c.hb_pred[idw];
  }
  return path_len;
}

// Lane-parallel: rebuild the packed per-rank row descriptors from the graph
// arrays (called after backbone init and after every topo sort).
__device__ void build_row_desc(WindowCtx& c, int lane) {
  const uint32_t n = c.num_nodes;
  for (uint32_t node = lane; node < n; node += kLanes) {
    const uint32_t r = c.rank[node];
    const uint8_t nin = c.in_cnt[node];
    uint16_t pred_row = 0;
    if (nin > 0) {
      pred_row = static_cast<uint16_t>(c.rank[c.in_edges[node * kMaxE]] + 1);
    }
    uint64_t rd2 = 0;
    for (uint32_t e = 1; e < min(static_cast<uint32_t>(nin), kMaxPre); ++e) {
      const uint64_t row = c.rank[c.in_edges[node * kMaxE + e]] + 1u;
      rd2 |= row << (16 * (e - 1));
    }
    c.row_desc2[r] = rd2;
    const uint32_t nout = c.out_cnt[node];
    uint8_t flags = (nout == 0) ? kRdEnd : 0;
    for (uint32_t e = 0; e < nout; ++e) {
      const uint32_t sr = c.rank[out_edge_of(c, node, e)];
      if (sr - r >= kRing) {
        flags |= kRdStore;
        break;
      }
    }
    c.row_desc[r] = pack_rd(c.letters[node], nin, static_cast<uint16_t>(node), pred_row, flags);
  }
}

// ---------- lane-parallel phases ----------

// Graph of the backbone alone (layer 0): a chain, already in topological
// order, with its row descriptors.
template <class SH>
__device__ void init_backbone_d(WindowCtx& c, SH& s, int lane) {
  const uint32_t bb_len = c.ends[0];
  const uint8_t* bb_seq = c.seq_base;
  const uint8_t* bb_wts = c.weight_base;
  for (uint32_t i = lane; i < bb_len; i += kLanes) {
    c.letters[i] = bb_seq[i];
    c.ring_cnt[i] = 0;
    c.nseq[i] = bb_len >= 2 ? 1 : 0;
    // queue holds the trivial order for the no-aligned-layer case (it is
    // clobbered by the DP ring and rebuilt by every topo sort afterwards)
    s.u.kahn.queue[i] = static_cast<uint16_t>(i);
    c.rank[i] = static_cast<uint16_t>(i);
    uint8_t nin = 0;
    if (i == 0) {
      c.in_cnt[i] = 0;
    } else {
      nin = 1;
      c.in_cnt[i] = 1;
      c.in_edges[i * kMaxE] = static_cast<uint16_t>(i - 1);
      c.in_weights[i * kMaxE] = static_cast<int32_t>(bb_wts[i - 1]) + bb_wts[i];
    }
    uint8_t flags = 0;
    if (i + 1 < bb_len) {
      c.out_cnt[i] = 1;
      c.out_edges[i * kMaxE] = static_cast<uint16_t>(i + 1);
    } else {
      c.out_cnt[i] = 0;
      flags = kRdEnd;
    }
    c.row_desc[i] = pack_rd(bb_seq[i], nin, static_cast<uint16_t>(i),
                            static_cast<uint16_t>(i), flags);
    c.row_desc2[i] = 0;  // a chain: no node has a second in-edge
  }
  c.num_nodes = bb_len;
  c.seqs_in_graph = 1;
  __syncthreads();  // graph writes -> visible to all lanes
}

// Per-layer match bitvectors (see Shared::match) straight from the
// (L2-resident) global layer bytes, lane-parallel over chunk words; one
// spare zero word so cross-word extraction never reads out of bounds.
template <class SH>
__device__ void build_match_bits_d(SH& s, const uint8_t* seq, uint32_t len, int lane) {
  const uint32_t words = (len + kLanes - 1) / kLanes + 1;
  for (uint32_t w = lane; w < words * 4; w += kLanes) {
    const uint32_t k = w >> 2, cc = w & 3;
    uint64_t bits = 0;
    const uint32_t base = k * kLanes;
    if (base < len) {
      const uint32_t lim = min(kLanes, len - base);
      for (uint32_t l = 0; l < lim; ++l) {
        if (poa_code(seq[base + l]) == static_cast<int32_t>(cc)) {
          bits |= 1ull << l;
        }
      }
    }
    s.u.dp.match[cc][k] = bits;
  }
  __syncthreads();
}

// What one layer's DP rows share.
struct LayerDp {
  const uint8_t* seq;
  uint32_t len;
  uint32_t chunks;  // 64-column chunks covering len
  // SUBGRAPH restriction (CPU parity, Window::generate_consensus): a
  // layer that does not span the window aligns only against the rank
  // window [rank(backbone[begin]), rank(backbone[end])]. Rows outside are
  // skipped, predecessor edges from below rank(begin) are ignored (rows
  // losing every predecessor become NW start rows), and the alignment
  // target is the span's end rank (plus true sinks inside the window).
  // The reference's cudapoa aligns every layer to the full graph instead,
  // which is what degrades its long-window GPU goldens (racon_test.cpp
  // pins 4168 vs CPU 1289 at w=1000); this engine keeps the CPU
  // windowing semantics on device.
  bool sub;
  uint32_t rlo, rhi;
  // banded mode (-b): static band of bw columns around the rank diagonal of
  // the (possibly rank-restricted) row window
  bool banded;
  uint32_t bw;
  uint32_t slope16;
};

// DP row (rank + 1) of in-edge e's source node. The first kMaxPre come from
// the row's two descriptor words (pred0 and rd2, both wave-uniform), so a row
// with up to five predecessors — one row in three has more than one on noisy
// long reads, one in ten three or more — never waits for the graph arrays.
// From in-edge kMaxPre on the row is re-derived on use: two dependent global
// loads, for rows with six or more in-edges (0.00 % of the DP rows in a probe
// of the flagship's error model; BASELINE.md, "Multi-predecessor DP rows").
__device__ __forceinline__ uint32_t pred_row_of(const WindowCtx& c, uint32_t node, uint32_t e,
                                                uint32_t pred0, uint64_t rd2) {
  if (e == 0) {
    return pred0;
  }
  if (e < kMaxPre) {
    return static_cast<uint32_t>(rd2 >> (16 * (e - 1))) & 0xffffu;
  }
  return c.rank[c.in_edges[node * kMaxE + e]] + 1;
}

// Columns of banded DP row p that hold a value: [lo + 1, hi], plus column 0
// when has0.
struct PredBand {
  uint32_t lo, hi;
  bool has0;
};

__device__ __forceinline__ PredBand pred_band(const LayerDp& d, uint32_t p) {
  uint32_t pklo, pkhi;
  band_chunks(p - d.rlo, d.slope16, d.bw, d.chunks, &pklo, &pkhi);
  return {pklo * kLanes, min(d.len, (pkhi + 1) * kLanes), pklo == 0};
}

// Gathers pv[w] = row(cbase + w), w in 0..WB, with columns outside okmask
// set to `neg` (the row's minus infinity); `last` is the row's last
// addressable column. Loads are UNCONDITIONAL with a clamped index + VALU
// select: per-element predication compiled to one exec-branched flat_load
// each (generic pointer), serializing the row. Called once for an LDS ring row and once for a
// global matrix row; each call must keep its address space (ds_read vs
// global_load), and that is brittle: `row` is a functor indexing the
// caller's own array expression, and each load is selected where it is
// made, because with a plain `const int16_t*` parameter, or with the loads
// first and one select loop after them, the compiler merged the tails of the
// two calls into flat_loads (1-6 per kernel). Re-check the ISA for flat_load
// after touching this.
template <uint32_t WB, class Row>
__device__ __forceinline__ void gather_row(const Row& row, uint32_t cbase, uint32_t last,
                                           uint32_t okmask, int32_t neg, int32_t (&pv)[WB + 1]) {
  if constexpr (WB == 8) {
    if (cbase + WB <= last) {
      // unpack a 16-byte vector load into pv[0..7] (cbase*2 is a
      // multiple of 16 when WB == 8, and both the ring rows and the
      // global matrix rows are 16-byte aligned); replaces 8 scalar
      // b16 loads — the LDS pipe is the congested unit at 20+
      // co-resident windows per CU (profiles/PARKED.md)
      const int4 v = *reinterpret_cast<const int4*>(&row(cbase));
      const int32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q) {
        pv[2 * q] = static_cast<int32_t>(static_cast<int16_t>(ws[q] & 0xffff));
        pv[2 * q + 1] = ws[q] >> 16;  // arithmetic: sign-extended
      }
      pv[WB] = row(cbase + WB);
#pragma unroll
      for (uint32_t w = 0; w <= WB; ++w) {
        pv[w] = ((okmask >> w) & 1u) ? pv[w] : neg;
      }
      return;
    }
  }
  if (cbase + WB <= last) {
#pragma unroll
    for (uint32_t w = 0; w <= WB; ++w) {
      const int32_t val = row(cbase + w);
      pv[w] = ((okmask >> w) & 1u) ? val : neg;
    }
  } else {
#pragma unroll
    for (uint32_t w = 0; w <= WB; ++w) {
      const int32_t val = row(min(cbase + w, last));
      pv[w] = ((okmask >> w) & 1u) ? val : neg;
    }
  }
}

// One DP row: rank r of the topological order (matrix row r + 1) against
// the whole layer, all lanes. Row 0 (all-gap) is arithmetic: H0[j] = j * g —
// never materialized. Updates the running alignment end (best_score,
// best_row), which stays wave-uniform. The context comes BY VALUE: the row
// only reads it, and taken by reference the whole struct stayed in scratch
// memory (208 B/lane on every variant).
//
// CHECKED: the row also applies the score check to its column-0 score
// (poa_score_row_refused) and sets score_low, which is sticky and
// wave-uniform, when it is refused. The row is computed all the same, with
// clamped and possibly wrapped scores that only ever become move bytes: the
// kernel drops the layer, and the window, after its last row. Checked kernels
// run unbanded rows only, so every row computes h0.
template <bool CHECKED, uint32_t WB, uint32_t MAXW, class SH>
__device__ __forceinline__ void dp_row(const WindowCtx c, SH& s, const LayerDp& d, uint32_t r,
                                       uint64_t rd, uint64_t rd2_lanes, int lane,
                                       int32_t& best_score, uint32_t& best_row,
                                       uint32_t& score_low) {
  // Every lane read the same two LDS words, so they are wave-uniform, but
  // they arrive in vector registers. The second word (rows of in-edges 1..4,
  // see pred_row_of) is only ever shifted by the wave-uniform edge index:
  // keep it in scalar registers. The first stays where it is: with all of it
  // scalar every variant needed 10 more VGPRs.
  const uint64_t rd2 =
      static_cast<uint64_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(rd2_lanes))) |
      (static_cast<uint64_t>(
           __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(rd2_lanes >> 32)))
       << 32);
  const uint32_t len = d.len;
  const uint8_t letter = static_cast<uint8_t>(rd);
  const int32_t letter_code = poa_code(letter);
  const uint32_t nin = static_cast<uint32_t>((rd >> 8) & 0xff);
  const uint32_t node = static_cast<uint32_t>((rd >> 16) & 0xffff);
  const uint32_t pred0 = static_cast<uint32_t>((rd >> 32) & 0xffff);
  const uint64_t flags = (rd >> 48) & 0xff;
  const bool is_end = (flags & kRdEnd) != 0;
  const bool store_row = (flags & kRdStore) != 0;
  int16_t* Hrow = c.matrix + static_cast<size_t>(r + 1) * kMaxW;
  uint8_t* Mrow = c.moves + static_cast<size_t>(r + 1) * kMaxW;
  int16_t* ring_row = s.u.dp.ring[(r + 1) % kRing];

  // usable predecessor edges: in subgraph mode edges from ranks below
  // the window are cut; a row losing every predecessor becomes an NW
  // start row (virtual row 0), matching the CPU subgraph's sources.
  // Edge index 63 in a move byte encodes that virtual start for the
  // traceback (real indices stop at max_edges-1 = 47).
  uint64_t usable = (1ull << nin) - 1;  // nin <= 48 < 64
  if (d.sub && nin != 0) {
    usable = 0;
    for (uint32_t e = 0; e < nin; ++e) {
      if (pred_row_of(c, node, e, pred0, rd2) > d.rlo) {
        usable |= 1ull << e;
      }
    }
  }
  const bool vstart = usable == 0;  // nin == 0, or every pred cut

  uint32_t row_klo = 0, row_khi = d.chunks - 1;
  if (d.banded) {
    band_chunks(r + 1 - d.rlo, d.slope16, d.bw, d.chunks, &row_klo, &row_khi);
  }

  // fetch a predecessor row value: LDS ring if close, global otherwise;
  // in banded mode, columns outside the predecessor's band are -inf
  auto pred_val = [&](uint32_t p, uint32_t col) -> int32_t {
    if (p == 0) {
      // arithmetic row 0; no in-edge leads there (see the edge loop below,
      // which has no such branch), kept because it costs nothing here
      return static_cast<int32_t>(col) * c.g;
    }
    if (d.banded) {
      const PredBand pb = pred_band(d, p);
      if (col == 0 ? !pb.has0 : (col <= pb.lo || col > pb.hi)) {
        return kNegInf;
      }
    }
    if (r + 1 - p < kRing) {
      return s.u.dp.ring[p % kRing][col];
    }
    return c.matrix[static_cast<size_t>(p) * kMaxW + col];
  };

  // first column (j = 0): max over preds of Hp[0] + gap
  // (banded: only when this row's band includes column 0)
  int32_t h0 = kNegInf;
  uint32_t e0 = 0;
  if (row_klo == 0) {
    int32_t best0 = kNegInf;
    if (vstart) {
      best0 = 0;
      e0 = 63;  // virtual-start sentinel (see `usable`)
    } else {
      for (uint32_t e = 0; e < nin; ++e) {
        if (!((usable >> e) & 1)) {
          continue;
        }
        const int32_t hp0 = pred_val(pred_row_of(c, node, e, pred0, rd2), 0);
        if (hp0 > best0) {
          best0 = hp0;
          e0 = e;
        }
      }
    }
    h0 = best0 + c.g;
    if constexpr (CHECKED) {
      // every lane holds the same h0: take it to a scalar register, so that
      // the compare and the flag cost the row no vector register
      score_low |= poa_score_row_refused(__builtin_amdgcn_readfirstlane(h0), len, c.g) ? 1u : 0u;
    }
    if (lane == 0) {
      if (store_row) {
        Hrow[0] = static_cast<int16_t>(h0);
      }
      ring_row[0] = static_cast<int16_t>(h0);
      // column 0 is always a vertical chain through the argmax edge
      // (moves layout is shifted: col j lives at j-1, col 0 at kMaxW-1,
      // so each lane's 8 move bytes form one aligned u64 store)
      Mrow[kMaxW - 1] = static_cast<uint8_t>(kMvUp | (e0 << 2));
    }
  }

  // ---- lane-blocked columns ----
  // Lane l owns WB contiguous columns per pass; one register-local
  // inclusive scan + one DPP wave scan per pass replaces the previous
  // chunk-serial carry chain (8 dependent LDS+scan segments per row).
  const uint32_t j0 = d.banded ? row_klo * kLanes : 0;
  const uint32_t jend = d.banded ? min(len, (row_khi + 1) * kLanes) : len;
  // Multi-predecessor rows take every maximum over keys (see the edge loop)
  // and have a minus infinity of their own, kNegInfKeyed, which every value
  // of the row that stands for "no cell" uses, so that such values compare
  // with each other as they do on the other rows.
  // (scalar on purpose: the flag derives from an LDS read, and everything
  // selected by it would otherwise be computed per lane in VGPRs)
  const bool keyed = __builtin_amdgcn_readfirstlane((nin > 1 && !vstart) ? 1 : 0) != 0;
  const int32_t neg = keyed ? kNegInfKeyed : kNegInf;
  // the scores as the edge loop adds them: times 64 next to keys
  const int32_t sm = keyed ? c.m * 64 : c.m;
  const int32_t sx = keyed ? c.x * 64 : c.x;
  const int32_t sg = keyed ? c.g * 64 : c.g;
  // u-space max through column j0: minus infinity when the band excludes
  // column 0 (h0 was not computed)
  int32_t carry_u = row_klo == 0 ? h0 : neg;
  int32_t last_col_val = kNegInf;
  int32_t pass_tail = 0;  // lane 63's last clamped value of the previous
                          // pass (the shifted store's column `base`)

  for (uint32_t base = j0; base < jend; base += kLanes * WB) {
    const uint32_t cbase = base + lane * WB;  // own cols: cbase+1..cbase+WB
    const uint32_t nown = (cbase < jend) ? min(WB, jend - cbase) : 0;

    // substitution matches for own columns: bits w of mbits
    uint64_t mbits = 0;
    if (letter_code >= 0 && nown > 0) {
      const uint32_t bit0 = cbase & 63;
      const uint32_t w0 = cbase >> 6;
      mbits = s.u.dp.match[letter_code][w0] >> bit0;
      if (bit0 != 0) {
        mbits |= s.u.dp.match[letter_code][w0 + 1] << (64 - bit0);
      }
    } else if (nown > 0) {
      for (uint32_t w = 0; w < nown; ++w) {
        if (d.seq[cbase + w] == letter) {  // rare: non-ACGT row letter
          mbits |= 1ull << w;
        }
      }
    }

    // Best diagonal / vertical candidates. On a row with one predecessor
    // (two rows in three) they are scores. On a multi-predecessor row they
    // are keys, (score << 6) | (63 - e) for in-edge e: one max picks the
    // highest score and, among equal scores, the lowest edge index, which is
    // the tie rule of the CPU engine's ascending edge loop, so the edge of a
    // move byte falls out of the maximum and is never looked for afterwards.
    // Edge indices stop at 47, so the low six bits of a real key are 16..63;
    // 0 marks the initial value, which stands for "no candidate at or above
    // minus infinity" and decodes to edge 0.
    int32_t bd[WB], bu[WB];
    const int32_t cand_init = keyed ? kNegInfKeyed * 64 : kNegInf;
#pragma unroll
    for (uint32_t w = 0; w < WB; ++w) {
      bd[w] = cand_init;
      bu[w] = cand_init;
    }

    if (vstart) {
#pragma unroll
      for (uint32_t w = 0; w < WB; ++w) {
        if (w < nown) {
          const int32_t j = static_cast<int32_t>(cbase + 1 + w);
          const int32_t subst = ((mbits >> w) & 1) ? c.m : c.x;
          bd[w] = (j - 1) * c.g + subst;
          bu[w] = j * c.g + c.g;
        }
      }
    } else {
      for (uint32_t e = 0; e < nin; ++e) {
        if (!((usable >> e) & 1)) {
          continue;
        }
        const uint32_t p = pred_row_of(c, node, e, pred0, rd2);
        // pred row values pv[w] = H(p, cbase + w). p is a real row: an
        // in-edge's source has a rank, so p >= 1, and the arithmetic row 0
        // belongs to the virtual start above alone. This loop has no branch
        // for p == 0 on purpose (it cost 8 VGPRs in every variant), while
        // pred_val keeps its cheap one; the difference is deliberate. What
        // keeps a zero field of rd2 out of here is the bound e < nin: fields
        // are 0 only for in-edges the node does not have. Loosen that bound
        // and a zero field reads ring or matrix row 0 (in bounds, but not
        // the arithmetic row).
        int32_t pv[WB + 1];
        {
          PredBand pb{0, len, true};
          if (d.banded) {
            pb = pred_band(d, p);
          }
          // validity of the contiguous range [lo+1, hi] (plus col 0
          // when the pred row computed it) hoisted into ONE bitmask per
          // edge — per-element compare+select chains were ~10% of the
          // kernel's VALU issue
          const uint32_t lo_col = pb.lo + 1;
          const uint32_t lo_w = lo_col > cbase ? min(lo_col - cbase, WB + 1) : 0;
          const uint32_t hi_w = (pb.hi + 1 > cbase) ? min(pb.hi + 1 - cbase, WB + 1) : 0;
          uint32_t okmask = (hi_w > lo_w) ? ((1u << hi_w) - (1u << lo_w)) : 0u;
          if (cbase == 0 && pb.has0) {
            okmask |= 1u;  // col 0 sits outside [lo+1, hi] by construction
          }
          if (r + 1 - p < kRing) {
            const uint32_t slot = p % kRing;
            gather_row<WB>([&](uint32_t col) -> const int16_t& { return s.u.dp.ring[slot][col]; },
                           cbase, MAXW - 1, okmask, neg, pv);
          } else {
            const int16_t* gsrc = c.matrix + static_cast<size_t>(p) * kMaxW;
            gather_row<WB>([&](uint32_t col) -> const int16_t& { return gsrc[col]; }, cbase,
                           kMaxW - 1, okmask, neg, pv);
          }
        }
        // no nown guard: out-of-range pv entries are -inf and propagate
        if (keyed) {
          // key the row's values once; the scores below are scaled to match
          // and leave the low six bits alone
          const uint32_t pri = 63 - e;
#pragma unroll
          for (uint32_t w = 0; w <= WB; ++w) {
            pv[w] = static_cast<int32_t>((static_cast<uint32_t>(pv[w]) << 6) | pri);
          }
        }
#pragma unroll
        for (uint32_t w = 0; w < WB; ++w) {
          const int32_t subst = ((mbits >> w) & 1) ? sm : sx;
          bd[w] = max(bd[w], pv[w] + subst);
          bu[w] = max(bu[w], pv[w + 1] + sg);
        }
      }
    }

    // v[w]: the better of the two candidates; byte w of mvbase: the move
    // byte it stands for, type | edge << 2 (diagonal on a tie). A left move
    // replaces it below where the horizontal scan wins.
    int32_t v[WB];
    uint64_t mvbase = 0;
    if (keyed) {
#pragma unroll
      for (uint32_t w = 0; w < WB; ++w) {
        const int32_t sd = bd[w] >> 6, su = bu[w] >> 6;  // arithmetic shifts
        const bool diag = sd >= su;
        v[w] = diag ? sd : su;
        const uint32_t low = static_cast<uint32_t>(diag ? bd[w] : bu[w]) & 63u;
        const uint32_t edge = low != 0 ? 63u - low : 0u;
        mvbase |= static_cast<uint64_t>((diag ? kMvDiag : kMvUp) | (edge << 2)) << (8 * w);
      }
    } else {
      // one predecessor: edge 0; none: the virtual-start sentinel
      const uint32_t edge_bits = vstart ? (63u << 2) : 0u;
#pragma unroll
      for (uint32_t w = 0; w < WB; ++w) {
        const bool diag = bd[w] >= bu[w];
        v[w] = diag ? bd[w] : bu[w];
        mvbase |= static_cast<uint64_t>((diag ? kMvDiag : kMvUp) | edge_bits) << (8 * w);
      }
    }

    // local inclusive u-space scan over own columns (out-of-range
    // candidates are already -inf; no per-element guard needed)
    int32_t us[WB];
    int32_t run = kNegInf;
#pragma unroll
    for (uint32_t w = 0; w < WB; ++w) {
      const int32_t j = static_cast<int32_t>(cbase + 1 + w);
      const int32_t u = v[w] - j * c.g;
      run = max(run, u);
      us[w] = run;
    }
    // wave scan over lane totals -> exclusive prefix for this lane
    const int32_t incl = wave_scan_max(run);
    int32_t excl =
        __builtin_amdgcn_update_dpp(kNegInf, incl, 0x138, 0xf, 0xf, false);  // wave_shr:1
    excl = max(excl, carry_u);
    // next pass's carry: wave-uniform max over everything <= this pass
    carry_u = max(carry_u, __builtin_amdgcn_readlane(incl, kLanes - 1));

    // finalize own columns: h, moves, stores. h is computed for every
    // slot (junk past the row end feeds only junk columns); no memory is
    // read here.
    int32_t h_sel = kNegInf;
    uint64_t mvpack = 0;  // 8 move bytes -> one aligned store at Mrow[cbase]
    int32_t harr[WB];
#pragma unroll
    for (uint32_t w = 0; w < WB; ++w) {
      const uint32_t j = cbase + 1 + w;
      const int32_t h = max(us[w], excl) + static_cast<int32_t>(j) * c.g;
      harr[w] = h < kPoaScoreFloor ? kPoaScoreFloor : h;
      const uint32_t mv =
          (h != v[w]) ? kMvLeft : static_cast<uint32_t>(mvbase >> (8 * w)) & 0xffu;
      if (WB == 8) {
        mvpack |= static_cast<uint64_t>(mv) << (8 * w);  // bytes past nown: cleared below
      } else if (w < nown) {
        if (store_row) {
          Hrow[j] = static_cast<int16_t>(harr[w]);
        }
        ring_row[j] = static_cast<int16_t>(harr[w]);
        Mrow[j - 1] = static_cast<uint8_t>(mv);  // shifted layout, per-byte for odd widths
      }
      if (w < nown && j == len) {
        h_sel = h;
      }
    }
    if (WB == 8 && nown < WB) {
      mvpack &= (1ull << (8 * nown)) - 1;  // columns past the row end carry byte 0
    }
    if (WB == 8) {
      // Shifted 16-byte row stores: lane l writes columns
      // [cbase .. cbase+7] = [neighbor's last value | own h[0..6]] so
      // the store is one aligned b128 instead of 8 b16 ops (LDS-pipe
      // congestion is the bottleneck — profiles/PARKED.md). Column
      // `base` comes from lane 63 of the previous pass (or h0), the
      // pass-boundary column base+512 from the NEXT pass's lane 0, and
      // a row ending exactly on the boundary stores it explicitly.
      const int32_t tail_in = (base == j0) ? h0 : pass_tail;
      const int32_t shifted =
          __builtin_amdgcn_update_dpp(tail_in, harr[WB - 1], 0x138, 0xf, 0xf, false);
      pass_tail = __builtin_amdgcn_readlane(harr[WB - 1], kLanes - 1);
      if (cbase < jend) {
        int4 vec;
        vec.x = (shifted & 0xffff) | (harr[0] << 16);
        vec.y = (harr[1] & 0xffff) | (harr[2] << 16);
        vec.z = (harr[3] & 0xffff) | (harr[4] << 16);
        vec.w = (harr[5] & 0xffff) | (harr[6] << 16);
        *reinterpret_cast<int4*>(&ring_row[cbase]) = vec;
        if (store_row) {
          *reinterpret_cast<int4*>(Hrow + cbase) = vec;
        }
      }
      // When this pass's last covered column is `len` itself AND len
      // lands on a lane boundary ((len - base) % WB == 0), the lane
      // that would store it via its shifted slot has cbase == len and
      // is excluded by the cbase < jend guard — store it explicitly
      // from the owning lane's last value. (Missing this for ANY
      // multiple-of-8 row length left ring[len] uninitialized and made
      // results depend on stale LDS — caught by tools/probe_order.py.)
      // The large class is the one 8-wide variant that runs banded rows
      // (the route gives the regular classes' banded windows to the 5-wide
      // variants): there the last covered column is the band's, jend, which
      // is always a multiple of 8 and a valid column of the row (pred_band).
      const uint32_t tail_col = kLarge ? jend : len;
      const uint32_t rem = tail_col > base ? tail_col - base : 0;
      if (rem > 0 && rem <= kLanes * WB && (rem & (WB - 1)) == 0) {
        const int owner = static_cast<int>(rem / WB) - 1;
        const int32_t t16 = __builtin_amdgcn_readlane(harr[WB - 1], owner);
        if (lane == 0) {
          ring_row[tail_col] = static_cast<int16_t>(t16);
          if (store_row) {
            Hrow[tail_col] = static_cast<int16_t>(t16);
          }
        }
      }
    }
    if (WB == 8 && cbase < len) {
      if (cbase + WB < kMaxW) {
        // one aligned u64 store covers the lane's 8 move bytes
        // (cbase is a multiple of 8 exactly when WB == 8); bytes beyond
        // nown encode columns past the row end and are never read back
        *reinterpret_cast<uint64_t*>(Mrow + cbase) = mvpack;
      } else {
        // near-full row: byte kMaxW-1 is the shifted column-0 slot (stored
        // above as kMvUp); a packed store here would clobber it with the
        // padding byte 0 (kMvDiag) and derail the traceback at j==0.
        // Store only the live bytes individually.
        for (uint32_t w = 0; w < nown; ++w) {
          Mrow[cbase + w] = static_cast<uint8_t>(mvpack >> (8 * w));
        }
      }
    }
    if (len > base && len <= base + kLanes * WB) {
      const int owner = static_cast<int>((len - 1 - base) / WB);
      last_col_val = __builtin_amdgcn_readlane(h_sel, owner);
    }
  }

  // ring writes must be visible to every lane before the next row;
  // deliberately NOT __syncthreads (would drain the global row stores)
  wave_lds_sync();

  // end-node max (strict >, first in topological order wins);
  // last_col_val is already wave-uniform (readlane). In subgraph mode
  // the span's end rank is the alignment sink (plus true sinks inside
  // the window).
  if ((is_end || (d.sub && r == d.rhi)) && last_col_val > best_score) {
    best_score = last_col_val;
    best_row = r + 1;
  }
}

// ---------- the lean row ----------

// Two int16 values in one register, the lower column in the low half: the
// layout of a ring row, so a 16-byte ring load is four of them as it stands.
using pk16 = short __attribute__((ext_vector_type(2)));
using pku16 = unsigned short __attribute__((ext_vector_type(2)));

__device__ __forceinline__ pk16 pk_from(uint32_t w) { return __builtin_bit_cast(pk16, w); }
__device__ __forceinline__ uint32_t pk_bits(pk16 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ pk16 pk_splat(int32_t v) {
  return pk16{static_cast<short>(v), static_cast<short>(v)};
}
__device__ __forceinline__ pk16 pk_max(pk16 a, pk16 b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ pk16 pk_lo(pk16 a) { return __builtin_shufflevector(a, a, 0, 0); }
__device__ __forceinline__ pk16 pk_hi(pk16 a) { return __builtin_shufflevector(a, a, 1, 1); }
// the pair one column further on: (a's high half, b's low half)
__device__ __forceinline__ pk16 pk_next(pk16 a, pk16 b) {
  return pk_from(__builtin_amdgcn_alignbit(pk_bits(b), pk_bits(a), 16));
}
// per half: 1 where the halves of a and b differ, else 0. The instruction is
// written out: as an elementwise min of the xor with 1 the compiler turns it
// back into two 16-bit compares, two selects and a byte permute per pair.
__device__ __forceinline__ uint32_t pk_differ(pk16 a, pk16 b) {
  const uint32_t x = pk_bits(a) ^ pk_bits(b);
  uint32_t r;
  asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(x), "s"(0x00010001u));
  return r;
}

// poa_code for a letter in a scalar register, without the switch's branches:
// bits 1..2 of 'A', 'C', 'T', 'G' are 0, 1, 2, 3.
__device__ __forceinline__ int32_t poa_code_uniform(uint32_t letter) {
  const uint32_t idx = letter - 'A';
  // 'A', 'C', 'G', 'T' are 0, 2, 6 and 19 letters behind 'A'
  if (idx > 19u || ((0x80045u >> idx) & 1u) == 0) {
    return -1;
  }
  const uint32_t t = (letter >> 1) & 3u;  // A 0, C 1, G 3, T 2
  return static_cast<int32_t>(t ^ (t >> 1));
}
static_assert((('A' >> 1) & 3) == 0 && (('C' >> 1) & 3) == 1 && (('G' >> 1) & 3) == 3 &&
              (('T' >> 1) & 3) == 2 && 'C' - 'A' == 2 && 'G' - 'A' == 6 && 'T' - 'A' == 19);

// dp_row for the common row, on packed int16 pairs. The kernel's row loop
// sends a row here when (all wave-uniform, tested on scalar registers)
//   - the kernel is an 8-wide, unchecked one of the regular class,
//   - the launch's score parameters pass poa_lean_rows_fit and the batch has
//     the lean row on (PoaDeviceArena::lean_rows),
//   - the layer is unbanded and at most kPoaLeanMaxLen = 64 * 8 columns long,
//     so the row is one pass,
//   - the node has exactly one in-edge, usable under the layer's rank window
//     (pred0 > rlo when d.sub), whose source row is in the LDS ring,
//   - the node's letter is A, C, G or T (`code`).
// Every other row goes through dp_row. The row leaves behind exactly what
// dp_row leaves: ring_row and Hrow in columns 0..len, the move bytes, the
// running alignment end. Rows of both kinds alternate freely.
//
// What dp_row does and this row does not, and why the result does not need it:
//   - no okmask. The predecessor row is complete in columns 0..len (an
//     unbanded row writes them all, the explicit tail column included), so
//     the mask would only turn columns past len into minus infinity. Those
//     hold whatever the LDS held. Column j reads the predecessor's columns
//     j - 1 and j and, through the scan, this row's columns below j: junk
//     flows only from a column past len to columns past it. It never reaches
//     the value at column len (last_col_val), and the move bytes of columns
//     past len are cleared before the store, as in dp_row. Score columns past
//     len are stored as junk where dp_row stores floor values; every reader,
//     dp_row's okmask or this argument, ignores them.
//   - no edge loop, no candidate initial value, no edge index: the one edge
//     is in-edge 0, and a move byte's edge field is 0.
//   - column 0 is the low half of lane 0's ring load plus the gap score:
//     no read of its own, and no global read that the ring read would have
//     to share a register (and a vmcnt wait) with.
//   - the match bits are one byte per lane: cbase is a multiple of 8, so a
//     lane's eight bits never straddle a word of Shared::match.
//
// Range (poa_types.hpp, poa_lean_rows_fit). No value of a valid column leaves
// int16: stored scores are within 28000 of zero, candidates add one
// parameter, the u-space values at most 512 * |g|. So plain packed adds
// serve, and a wrap can happen only in a junk column, which feeds junk
// columns alone; there is no saturating add in the row because none could
// change a valid column. The move-byte tests are comparisons for equality
// (max == candidate, h == v), which cannot overflow. The wave scan runs on the
// lane totals sign-extended to 32 bits, with dp_row's scan and its identity.
template <uint32_t MAXW, class SH>
__device__ __forceinline__ void dp_row_lean(const WindowCtx c, SH& s, const LayerDp& d,
                                            uint32_t r, uint32_t rd_hi, int32_t code, int lane_id,
                                            int32_t& best_score, uint32_t& best_row) {
  constexpr uint32_t WB = 8;
  // What the row derives from the lane id (addresses, the j * g pairs) does
  // not change from row to row, so the compiler would keep it in VGPRs across
  // the whole row loop, dp_row's rows included, which have none to spare (it
  // spilled them). Recomputing costs a handful of instructions per row: hide
  // the lane id from loop-invariant code motion, as the kernel does for its
  // graph phases.
  int lane = lane_id;
  asm volatile("" : "+v"(lane));
  static_assert(kLanes * WB + 1 <= MAXW, "column cbase + 8 of lane 63 is inside the ring row");
  static_assert(kLanes * WB == kPoaLeanMaxLen);
  static_assert(kLanes * WB < kMaxW, "a lane's eight move bytes never reach the column-0 slot");
  const uint32_t len = d.len;
  const uint32_t pred0 = rd_hi & 0xffffu;
  const bool is_end = ((rd_hi >> 16) & kRdEnd) != 0;
  const bool store_row = ((rd_hi >> 16) & kRdStore) != 0;
  int16_t* Hrow = c.matrix + static_cast<size_t>(r + 1) * kMaxW;
  uint8_t* Mrow = c.moves + static_cast<size_t>(r + 1) * kMaxW;
  int16_t* ring_row = s.u.dp.ring[(r + 1) % kRing];
  const int16_t* pred_row = s.u.dp.ring[pred0 % kRing];

  const uint32_t cbase = static_cast<uint32_t>(lane) * WB;  // own cols: cbase+1..cbase+8
  const int4 pvec = *reinterpret_cast<const int4*>(&pred_row[cbase]);
  const uint32_t pv8 = static_cast<uint16_t>(pred_row[cbase + WB]);
  const uint32_t mb = reinterpret_cast<const uint8_t*>(s.u.dp.match[code])[lane];

  // column 0: a vertical move through the one edge
  const int32_t h0 =
      static_cast<int16_t>(__builtin_amdgcn_readfirstlane(pvec.x) & 0xffff) + c.g;

  // P[q]: predecessor columns cbase + 2q, + 2q + 1, the diagonal neighbours
  // of own columns 2q and 2q + 1; N[q]: one column on, the vertical ones
  const pk16 P[4] = {pk_from(pvec.x), pk_from(pvec.y), pk_from(pvec.z), pk_from(pvec.w)};
  const pk16 N[4] = {pk_next(P[0], P[1]), pk_next(P[1], P[2]), pk_next(P[2], P[3]),
                     pk_next(P[3], pk_from(pv8))};
  const pk16 gg = pk_splat(c.g);
  const pku16 xx = __builtin_bit_cast(pku16, pk_splat(c.x));
  const pku16 mx = __builtin_bit_cast(pku16, pk_splat(c.m - c.x));
  // match bit i of the lane at bits i and i + 15: shifted right by 2q, bits 0
  // and 16 are those of own columns 2q and 2q + 1
  const uint32_t spread = mb * 0x8001u;
  // j * g of own columns 2q, 2q + 1 (j = cbase + 1 + w, at most 512 * |g|)
  const int32_t jg0 = static_cast<int32_t>(cbase + 1) * c.g;
  const pk16 jg01 = pk16{static_cast<short>(jg0), static_cast<short>(jg0 + c.g)};
  pk16 V[4], JG[4];
  uint32_t up[4];  // per half: 1 where the vertical candidate wins (diagonal on a tie)
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const pku16 bit = __builtin_bit_cast(pku16, (spread >> (2 * q)) & 0x00010001u);
    const pk16 subst = __builtin_bit_cast(pk16, static_cast<pku16>(bit * mx + xx));
    const pk16 bd = P[q] + subst;
    const pk16 bu = N[q] + gg;
    V[q] = pk_max(bd, bu);
    up[q] = pk_differ(V[q], bd);
    JG[q] = jg01 + pk_splat(static_cast<int32_t>(2 * q) * c.g);
  }

  // inclusive u-space scan over own columns: within a pair, then along the
  // pairs through the high half of the one before
  pk16 R[4];
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const pk16 u = V[q] - JG[q];
    R[q] = pk_max(u, pk_lo(u));
    if (q != 0) {
      R[q] = pk_max(R[q], pk_hi(R[q - 1]));
    }
  }
  const int32_t run = static_cast<int32_t>(pk_bits(R[3])) >> 16;
  const int32_t incl = wave_scan_max(run);
  int32_t excl = __builtin_amdgcn_update_dpp(kNegInf, incl, 0x138, 0xf, 0xf, false);  // wave_shr:1
  excl = max(excl, h0);  // column 0 in u-space is h0 itself; real from here on
  const pk16 ex = pk_from(__builtin_amdgcn_perm(0u, static_cast<uint32_t>(excl), 0x01000100u));

  // scores, clamped for the store; a left move where the scan strictly wins
  const pk16 floor2 = pk_splat(kPoaScoreFloor);
  pk16 H[4], HC[4];
  uint32_t mv[4];  // per half: the move byte
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    H[q] = pk_max(R[q], ex) + JG[q];
    HC[q] = pk_max(H[q], floor2);
    const uint32_t left = pk_differ(H[q], V[q]);
    static_assert(kMvDiag == 0 && kMvUp == 1 && kMvLeft == 2);
    mv[q] = __builtin_bit_cast(
        uint32_t, __builtin_elementwise_max(__builtin_bit_cast(pku16, up[q]),
                                            __builtin_bit_cast(pku16, left + left)));
  }
  uint64_t mvpack =
      static_cast<uint64_t>(__builtin_amdgcn_perm(mv[1], mv[0], 0x06040200u)) |
      (static_cast<uint64_t>(__builtin_amdgcn_perm(mv[3], mv[2], 0x06040200u)) << 32);

  // the shifted 16-byte row store of dp_row: column cbase is the lane
  // below's last value, h0 for lane 0
  const uint32_t shifted = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(
      static_cast<int32_t>(static_cast<uint32_t>(h0) << 16), static_cast<int32_t>(pk_bits(HC[3])),
      0x138, 0xf, 0xf, false));
  if (cbase < len) {
    int4 vec;
    vec.x = static_cast<int32_t>(__builtin_amdgcn_alignbit(pk_bits(HC[0]), shifted, 16));
    vec.y = static_cast<int32_t>(pk_bits(pk_next(HC[0], HC[1])));
    vec.z = static_cast<int32_t>(pk_bits(pk_next(HC[1], HC[2])));
    vec.w = static_cast<int32_t>(pk_bits(pk_next(HC[2], HC[3])));
    *reinterpret_cast<int4*>(&ring_row[cbase]) = vec;
    if (store_row) {
      *reinterpret_cast<int4*>(Hrow + cbase) = vec;
    }
    const uint32_t nown = min(WB, len - cbase);
    if (nown < WB) {
      mvpack &= (1ull << (8 * nown)) - 1;  // columns past the row end carry byte 0
    }
    *reinterpret_cast<uint64_t*>(Mrow + cbase) = mvpack;
  }
  if (lane == 0) {
    Mrow[kMaxW - 1] = kMvUp;  // column 0, edge 0
  }
  // a row length on a lane boundary: the lane that would store column len in
  // its shifted slot has cbase == len (dp_row has the story)
  if ((len & (WB - 1)) == 0) {
    const uint32_t t16 =
        static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int32_t>(pk_bits(HC[3])),
                                                        static_cast<int>(len / WB) - 1)) >> 16;
    if (lane == 0) {
      ring_row[len] = static_cast<int16_t>(t16);
      if (store_row) {
        Hrow[len] = static_cast<int16_t>(t16);
      }
    }
  }

  wave_lds_sync();

  // end-node max, as in dp_row; the unclamped score at column len is taken
  // from the registers only on the rows that can end an alignment
  if (is_end || (d.sub && r == d.rhi)) {
    const int owner = static_cast<int>((len - 1) / WB);
    const uint32_t w = (len - 1) & (WB - 1);
    const uint32_t s0 = __builtin_amdgcn_readlane(static_cast<int32_t>(pk_bits(H[0])), owner);
    const uint32_t s1 = __builtin_amdgcn_readlane(static_cast<int32_t>(pk_bits(H[1])), owner);
    const uint32_t s2 = __builtin_amdgcn_readlane(static_cast<int32_t>(pk_bits(H[2])), owner);
    const uint32_t s3 = __builtin_amdgcn_readlane(static_cast<int32_t>(pk_bits(H[3])), owner);
    const uint32_t pair = w < 2 ? s0 : w < 4 ? s1 : w < 6 ? s2 : s3;
    const int32_t last_col_val =
        (w & 1) != 0 ? static_cast<int32_t>(pair) >> 16
                     : static_cast<int32_t>(static_cast<int16_t>(pair & 0xffffu));
    if (last_col_val > best_score) {
      best_score = last_col_val;
      best_row = r + 1;
    }
  }
}

// ---------- traceback ----------

// rounds of the traceback read this many moves of the predicted path at once
constexpr uint32_t kTbDepth = 64;
static_assert(kTbDepth <= kLanes, "one lane per predicted move");

// Walks the move bytes back from (best_row, len) to the origin. The walk
// ends at column 0, so it passes every sequence position exactly once:
// aln_nodes[p] gets the node position p is aligned to, or -1 for an
// insertion — indexed by position, which is what add_alignment_d loads 64
// at a time. Path entries that consume a graph node only (up moves) thread
// nothing into the graph and are not recorded. Call from ALL lanes.
//
// The move bytes fix the path; what is speculative is only when they are
// read. The serial walk pays one global round trip per step, because the
// address of a move depends on the move before it. Nearly all moves are
// "diagonal through in-edge 0" (byte 0), so a round predicts that the next
// kTbDepth moves are, and reads them all in ONE round trip:
//   chase   from (i, j), follow pred0 (LDS, staged below from row_desc) so
//           that lane k holds the row i_k reached after k such moves, its
//           column being j - k; stop at virtual row 0, at column 0 and at
//           kTbDepth;
//   load    every lane with a position loads its move byte and its row
//           descriptor;
//   accept  the lanes before the first byte that is not 0 were on the path
//           and record their node; that first lane is on the path too (its
//           position depends only on accepted moves), and its move is taken
//           as the serial walk takes it, all lanes in step. The next round
//           starts where that move leads.
// Row 0 with columns left is a run of insertions, filled lane-parallel.
// Column 0 with rows left (the move slot at kMaxW - 1) records nothing and
// stays a serial walk.
//
// pred0 holds 0 for an in-edge that the subgraph restriction cuts (source
// row <= rlo): a row whose in-edge 0 is cut cannot carry byte 0, so no lane
// behind it is ever accepted, and the chase ends there instead of following
// rows that were not staged. Lanes beyond the first deviation load bytes of
// rows rlo+1..best_row at columns below j, which are inside the slab whether
// or not this layer wrote them, and are ignored.
//
// NOT inlined, on purpose. Inlined into the kernel, this function's values
// compete for registers with the DP rows of the mid variant, which has none
// to spare at 5 waves/SIMD: the rows gained per-row spills and 16-48
// reloads. As a call it has a register file of its own, and the rows compile
// as they did without it. That is why it takes what it reads by value and
// the staging table as an LDS pointer (a reference to the window context
// would pin the whole context in scratch memory, and a generic pointer would
// turn the chase into flat loads, as generic slab pointers would the loads),
// and returns the status instead of setting it. A call costs the kernels 8 bytes of stack per lane, outside
// the rows.
#define RGA_GLOBAL __attribute__((address_space(1)))
struct TracebackArrays {
  RGA_GLOBAL const uint8_t* moves;
  RGA_GLOBAL const uint64_t* row_desc;
  RGA_GLOBAL const uint16_t* rank;
  RGA_GLOBAL const uint16_t* in_edges;
  RGA_GLOBAL int32_t* aln_nodes;
};
using LdsU16 = __attribute__((address_space(3))) uint16_t;

__device__ __attribute__((noinline)) int32_t traceback_d(const TracebackArrays c, LdsU16* pred0,
                                                         uint32_t rlo, uint32_t best_row,
                                                         uint32_t len, int lane) {
  int32_t status = kPoaOk;
  for (uint32_t r = rlo + 1 + lane; r <= best_row; r += kLanes) {
    const uint32_t p = static_cast<uint32_t>((c.row_desc[r - 1] >> 32) & 0xffff);
    pred0[r] = static_cast<uint16_t>(p > rlo ? p : 0);
  }
  __syncthreads();

  uint32_t i = best_row, j = len;  // wave-uniform
  while (!(i == 0 && j == 0)) {
    if (i == 0) {
      // row 0: all-gap prefix — the remaining columns are insertions
      for (uint32_t p = lane; p < j; p += kLanes) {
        c.aln_nodes[p] = -1;
      }
      break;
    }
    uint32_t mv;
    uint64_t rd;
    if (j != 0) {
      uint32_t ik = 0;    // lane k: row after k predicted moves
      uint32_t cur = i;   // uniform chase cursor
      uint32_t live = 0;  // lanes 0..live-1 hold a position
      const uint32_t depth = min(kTbDepth, j);
      while (live < depth && cur != 0) {
        if (static_cast<uint32_t>(lane) == live) {
          ik = cur;
        }
        cur = pred0[cur];
        ++live;
      }
      const bool has_pos = static_cast<uint32_t>(lane) < live;
      uint32_t mvk = 0;
      uint64_t rdk = 0;
      if (has_pos) {
        mvk = c.moves[static_cast<size_t>(ik) * kMaxW + (j - lane - 1)];
        rdk = c.row_desc[ik - 1];
      }
      const uint64_t dev = __ballot(has_pos && mvk != 0);
      const uint32_t first =
          dev != 0 ? static_cast<uint32_t>(__ffsll(static_cast<long long>(dev))) - 1 : live;
      if (static_cast<uint32_t>(lane) < first) {
        c.aln_nodes[j - lane - 1] = static_cast<int32_t>((rdk >> 16) & 0xffff);
      }
      j -= first;
      if (first == live) {
        i = cur;  // every predicted move held
        continue;
      }
      i = __shfl(ik, static_cast<int>(first), kLanes);
      mv = __shfl(mvk, static_cast<int>(first), kLanes);
      const uint32_t rd_lo = __shfl(static_cast<uint32_t>(rdk), static_cast<int>(first), kLanes);
      const uint32_t rd_hi =
          __shfl(static_cast<uint32_t>(rdk >> 32), static_cast<int>(first), kLanes);
      rd = (static_cast<uint64_t>(rd_hi) << 32) | rd_lo;
    } else {
      mv = c.moves[static_cast<size_t>(i) * kMaxW + kMaxW - 1];
      rd = c.row_desc[i - 1];
    }

    // one move of the serial walk at (i, j), all lanes in step
    const uint32_t type = mv & 3;
    const uint32_t e = mv >> 2;
    const uint32_t node = static_cast<uint32_t>((rd >> 16) & 0xffff);
    const uint32_t nin = static_cast<uint32_t>((rd >> 8) & 0xff);
    // a column-0 slot only ever holds an up move; anything else there, like
    // move type 3 anywhere, is not a path: fail the window
    if (type == 3 || (j == 0 && type != kMvUp)) {
      status = kPoaConsensusOverflow;
      break;
    }
    if (type == kMvLeft) {
      if (lane == 0) {
        c.aln_nodes[j - 1] = -1;
      }
      --j;
      continue;
    }
    uint32_t p = 0;  // virtual row 0: genuine start rows (nin==0)
                     // and subgraph sources (edge sentinel 63)
    if (nin != 0 && e != 63) {
      p = (e == 0) ? static_cast<uint32_t>((rd >> 32) & 0xffff)
                   : c.rank[c.in_edges[node * kMaxE + e]] + 1;
    }
    if (type == kMvDiag) {
      if (lane == 0) {
        c.aln_nodes[j - 1] = static_cast<int32_t>(node);
      }
      --j;
    }
    i = p;
  }
  return status;
}

// ---------- the mega-kernel ----------

// MINWAVES is the occupancy the compiler must budget registers for
// (waves/SIMD floor): the 8-wide variants otherwise help themselves to the
// full 128-VGPR budget of 4 waves/SIMD and registers — not LDS — become
// the residency limiter.
// CHECKED compiles the per-row score check in (dp_row): a window one of whose
// rows is refused ends with kPoaScoreRange.
template <bool TIMED, bool CHECKED, uint32_t WB, uint32_t MAXW, uint32_t MAXN, uint32_t MINWAVES>
__launch_bounds__(kLanes, MINWAVES)
__global__ void poa_window_kernel(PoaDeviceArena a, uint32_t window_base,
                                  uint32_t num_windows) {
  static_assert(MAXW <= kMaxW, "ring width exceeds the slab matrix width");
  static_assert(MAXN <= kMaxN, "node cap exceeds the slab graph capacity");
  if (blockIdx.x >= num_windows) {
    return;
  }
  const uint32_t win = window_base + blockIdx.x;
  const int lane = threadIdx.x;
  const PoaWindowDesc desc = a.windows[win];

  __shared__ Shared<MAXW, MAXN> s;

  WindowCtx c;
  static_cast<PoaSlabs&>(c) = a.slabs;
  for_each_poa_slab<kLarge>(c, [slab = static_cast<size_t>(desc.scratch_idx)](auto*& p,
                                                                              size_t count) {
    p += slab * count;
  });

  unsigned long long* timing = a.timing + static_cast<size_t>(win) * kPoaTimingSlots;
  unsigned long long tick = TIMED ? wall_clock64() : 0;
  const unsigned long long t_start = tick;
  unsigned long long t_dp = 0, t_tb = 0, t_add = 0, t_topo = 0, t_rd = 0, t_cons = 0;
  unsigned long long layers_done = 0;
  uint32_t rows_done = 0, rows_lean = 0;  // TIMED: DP rows, and those of the lean row
  // the instantiations that have the lean row at all
  constexpr bool kLeanKernel = WB == 8 && !kLarge && !CHECKED;
  auto lap = [&]() -> unsigned long long {
    if (!TIMED) {
      return 0;
    }
    unsigned long long now = wall_clock64();
    unsigned long long d = now - tick;
    tick = now;
    return d;
  };

  c.seq_base = a.seq_data + desc.seq_offset;
  c.weight_base = a.weight_data + desc.seq_offset;
  c.ends = a.layer_ends + a.layer_ends_index[win];
  c.spans = a.layer_spans + a.layer_ends_index[win];
  c.num_seqs = desc.num_seqs;
  c.MN = MAXN - 1;  // variant Kahn capacity (see Shared)
  c.m = a.match;
  c.x = a.mismatch;
  c.g = a.gap;
  c.status = kPoaOk;

  init_backbone_d(c, s, lane);

  // ---- per-layer loop ----
  for (uint32_t layer = 1; layer < c.num_seqs && c.status == kPoaOk; ++layer) {
    const uint32_t beg = c.ends[layer - 1];
    const uint32_t len = c.ends[layer] - beg;
    const uint8_t* seq = c.seq_base + beg;
    const uint8_t* wts = c.weight_base + beg;
    if (len == 0 || len + 1 > kMaxW) {
      continue;  // host should have filtered; skip defensively
    }
    if (len + 1 > MAXW) {
      c.status = kPoaWidthOverflow;  // mis-routed: fail to the CPU path
      break;
    }

    build_match_bits_d(s, seq, len, lane);

    const uint32_t n = c.num_nodes;
    LayerDp d;
    d.seq = seq;
    d.len = len;
    d.chunks = (len + kLanes - 1) / kLanes;
    const uint32_t span_word = c.spans[layer];
    d.sub = span_word != 0xFFFFFFFFu;
    d.rlo = d.sub ? c.rank[span_word >> 16] : 0;
    d.rhi = d.sub ? c.rank[span_word & 0xffffu] : n - 1;
    d.bw = a.band_width;
    // (the checked kernels are launched with band_width 0 only, and say so at
    // compile time: their rows carry no band code)
    d.banded = !CHECKED && (d.bw != 0) && (d.bw < len);
    d.slope16 = d.banded ? static_cast<uint32_t>((static_cast<uint64_t>(len) << 16) /
                                                 (d.rhi - d.rlo + 1))
                         : 0;

    // lean rows (dp_row_lean): what the layer has to be; the rest is per row
    const bool lean_layer = kLeanKernel && a.lean_rows != 0 && !d.banded && len <= kPoaLeanMaxLen;

    int32_t best_score = kNegInf;
    uint32_t best_row = 0;
    uint32_t score_low = 0;  // CHECKED: a row of this layer was refused
    (void)lap();

    // Row descriptors are staged 64 at a time through LDS with one
    // coalesced load: a per-row dependent global read (~600 ns) was the
    // dominant per-row latency and neither scan nor store restructuring
    // moved it (measured via RGA_POA_TIMING).
    for (uint32_t rblk = d.rlo & ~(kLanes - 1); rblk <= d.rhi; rblk += kLanes) {
      if (rblk + lane < n) {
        s.u.dp.rd_block[lane] = c.row_desc[rblk + lane];
        s.u.dp.rd2_block[lane] = c.row_desc2[rblk + lane];
      }
      wave_lds_sync();
      const uint32_t rlim = min(d.rhi + 1, rblk + kLanes);
      for (uint32_t r = max(rblk, d.rlo); r < rlim; ++r) {
        if constexpr (kLeanKernel) {
          // the row's eligibility for the lean row, on scalar registers (the
          // descriptor is wave-uniform but arrives in vector registers)
          if (lean_layer) {
            const uint64_t rdv = s.u.dp.rd_block[r - rblk];
            const uint32_t rd_lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(rdv));
            const uint32_t rd_hi =
                __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(rdv >> 32));
            const uint32_t pred0 = rd_hi & 0xffffu;
            const int32_t code = poa_code_uniform(rd_lo & 0xffu);
            if (((rd_lo >> 8) & 0xffu) == 1 && code >= 0 && r + 1 - pred0 < kRing &&
                (!d.sub || pred0 > d.rlo)) {
              dp_row_lean<MAXW>(c, s, d, r, rd_hi, code, lane, best_score, best_row);
              if (TIMED) {
                ++rows_lean;
                ++rows_done;
              }
              continue;
            }
          }
        }
        if (TIMED) {
          ++rows_done;
        }
        dp_row<CHECKED, WB, MAXW>(c, s, d, r, s.u.dp.rd_block[r - rblk],
                                  s.u.dp.rd2_block[r - rblk], lane, best_score, best_row,
                                  score_low);
      }
      wave_lds_sync();  // rows done before the next cooperative rd_block load
    }

    t_dp += lap();
    ++layers_done;

    // The graph phases below address the slabs relative to the lane id.
    // Those addresses do not change from layer to layer, so the compiler
    // would compute them once per window and keep them in VGPRs across the
    // DP rows, which have none to spare (the rows spilled): give the phases
    // a lane id that loop-invariant code motion cannot see through.
    int lane_g = lane;
    asm volatile("" : "+v"(lane_g));

    // A layer that tripped the score check stops here: its moves come from
    // clamped scores, so nothing of it may reach the graph. The status is
    // wave-uniform and final; every phase below and the layer loop are gated
    // by it.
    if (CHECKED && score_low != 0) {
      c.status = kPoaScoreRange;
    }

    // ---- traceback, all lanes (the ring is dead: its LDS is reused) ----
    if (!CHECKED || c.status == kPoaOk) {
      c.status = traceback_d({(RGA_GLOBAL const uint8_t*)c.moves,
                              (RGA_GLOBAL const uint64_t*)c.row_desc,
                              (RGA_GLOBAL const uint16_t*)c.rank,
                              (RGA_GLOBAL const uint16_t*)c.in_edges,
                              (RGA_GLOBAL int32_t*)c.aln_nodes},
                             (LdsU16*)s.u.tb.pred0, d.rlo, best_row, len, lane_g);
    }
    __syncthreads();  // the path -> visible to the whole wave
    t_tb += lap();

    // ---- thread the path into the graph, all lanes ----
    if (c.status == kPoaOk) {
      add_alignment_d(c, seq, wts, len, lane_g);
    }
    // the graph updates must be visible to the whole wave
    __syncthreads();
    t_add += lap();
    // add_alignment_d keeps these wave-uniform; lane 0 is the reference
    c.num_nodes = __shfl(c.num_nodes, 0, kLanes);
    c.seqs_in_graph = __shfl(c.seqs_in_graph, 0, kLanes);
    c.status = __shfl(c.status, 0, kLanes);

    (void)lap();
    if (c.status == kPoaOk) {
      topo_sort_d(c, s, lane_g);  // cooperative (internal barriers)
    }
    if (lane == 0) {
      t_topo += lap();
    }

    // rebuild the packed row descriptors for the grown graph, lane-parallel
    (void)lap();
    if (c.status == kPoaOk) {
      build_row_desc(c, lane_g);
    }
    __syncthreads();
    t_rd += lap();
  }

  // ---- consensus ----
  if (lane == 0) {
    uint8_t* out = a.consensus + static_cast<size_t>(win) * kL.max_consensus;
    uint16_t* cov = a.coverage + static_cast<size_t>(win) * kL.max_consensus;
    int32_t clen = -1;
    (void)lap();
    if (c.status == kPoaOk) {
      clen = consensus_d(c, s, out, cov, kL.max_consensus);
    }
    t_cons = lap();
    a.consensus_len[win] = clen < 0 ? 0 : static_cast<uint32_t>(clen);
    a.status[win] = c.status;
    a.num_nodes[win] = c.num_nodes;
    if (TIMED) {
      timing[0] = t_dp;
      timing[1] = t_tb;
      timing[2] = t_add;
      timing[3] = t_topo;
      timing[4] = t_rd;
      timing[5] = t_cons;
      timing[6] = wall_clock64() - t_start;
      timing[7] = poa_pack_counts(layers_done, rows_lean, rows_done);
    }
  }
}

// One launch per table row: separate __global__ instantiations per
// (columns-per-lane, ring-width) variant, because one kernel containing all
// variants pays the widest variant's registers and LDS on every path
// (measured 3x occupancy collapse).
// Measured: the power-of-two 8-wide variant (two passes for a 530-column
// window) beats a 9-wide single-pass variant by ~8% — non-power-of-two
// unrolls lose more in generated address code than the extra, mostly
// empty pass costs. The ring width (LDS) sets occupancy; see Shared<W>.
// A unit's launch function is named for its class and for the score check.
#ifdef RGA_POA_SCORE_CHECK
#define RGA_POA_LAUNCH(name) name##_checked
#else
#define RGA_POA_LAUNCH(name) name
#endif

#ifdef RGA_POA_LARGE_CLASS
// the large class has the one variant
template <bool TIMED>
void launch_large(const PoaDeviceArena& arena, uint32_t window_base, uint32_t num_windows,
                  hipStream_t stream) {
  constexpr PoaVariantParams p = kPoaLargeVariant;
  hipLaunchKernelGGL((poa_window_kernel<TIMED, kChecked, p.cols_per_lane, p.ring_width,
                                        p.node_cap, p.min_waves>),
                     dim3(num_windows), dim3(kLanes), 0, stream, arena, window_base,
                     num_windows);
}

}  // namespace

void RGA_POA_LAUNCH(launch_poa_kernel_large)(const PoaDeviceArena& arena, uint32_t window_base,
                                             uint32_t num_windows, void* stream) {
  static const bool timed = getenv("RGA_POA_TIMING") != nullptr;
  auto st = static_cast<hipStream_t>(stream);
  if (timed) {
    launch_large<true>(arena, window_base, num_windows, st);
  } else {
    launch_large<false>(arena, window_base, num_windows, st);
  }
}
#else
template <bool TIMED, PoaVariant V>
void launch_variant(const PoaDeviceArena& arena, uint32_t window_base, uint32_t num_windows,
                    hipStream_t stream) {
  constexpr PoaVariantParams p = kPoaVariants[V];
  hipLaunchKernelGGL((poa_window_kernel<TIMED, kChecked, p.cols_per_lane, p.ring_width,
                                        p.node_cap, p.min_waves>),
                     dim3(num_windows), dim3(kLanes), 0, stream, arena, window_base,
                     num_windows);
}

template <bool TIMED>
void dispatch_variant(const PoaDeviceArena& arena, uint32_t window_base, uint32_t num_windows,
                      PoaVariant variant, hipStream_t stream) {
  switch (variant) {
    case kPoaNarrow:
      return launch_variant<TIMED, kPoaNarrow>(arena, window_base, num_windows, stream);
    case kPoaMid:
      return launch_variant<TIMED, kPoaMid>(arena, window_base, num_windows, stream);
    case kPoaFull:
      return launch_variant<TIMED, kPoaFull>(arena, window_base, num_windows, stream);
    case kPoaBandedMid:
    case kPoaBandedFull:
      // the checked unit has no banded instantiations: banded rows reuse the
      // values below the floor, and the host keeps the check off with -b
      if constexpr (!kChecked) {
        if (variant == kPoaBandedMid) {
          return launch_variant<TIMED, kPoaBandedMid>(arena, window_base, num_windows, stream);
        }
        return launch_variant<TIMED, kPoaBandedFull>(arena, window_base, num_windows, stream);
      }
      break;
    case kPoaNumVariants:
      break;
  }
  fprintf(stderr, "[rga::hip::launch_poa_kernel] error: no kernel for variant %u\n",
          static_cast<unsigned>(variant));
  abort();
}

}  // namespace

void RGA_POA_LAUNCH(launch_poa_kernel)(const PoaDeviceArena& arena, uint32_t window_base,
                                       uint32_t num_windows, PoaVariant variant, void* stream) {
  static const bool timed = getenv("RGA_POA_TIMING") != nullptr;
  auto st = static_cast<hipStream_t>(stream);
  if (timed) {
    dispatch_variant<true>(arena, window_base, num_windows, variant, st);
  } else {
    dispatch_variant<false>(arena, window_base, num_windows, variant, st);
  }
}
#endif  // RGA_POA_LARGE_CLASS

}  // namespace rga::hip
