// HIP/CDNA4 banded Myers bit-vector aligner: one LANE per alignment.
//
// Each lane runs the blocked Myers edit-distance recurrence (Myers 1999,
// Hyyro 2003 block form) over a band of K 64-row blocks that slides along
// the rectangle diagonal (or, in the adaptive instantiations, follows the
// scores downwards) — 64 DP cells per 64-bit VALU op, no cross-lane
// communication in the hot loop (the previous anti-diagonal design spent
// ~85 cycles per cell on ds_bpermute shuffles; this one spends ~0.5).
// Column state (Pv/Mv per block + block-bottom scores) is stored
// wave-coalesced; the traceback walks (n,m)->(0,0) reconstructing the three
// predecessor scores per step in O(1) via popcount over the stored vertical
// deltas. Band-edge escapes are detected during traceback and reported as
// kAlnBandEdge -> CPU pairwise fallback (reference contract:
// src/cuda/cudaaligner.cpp:63-72).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hip/aligner_types.hpp"

namespace rga::hip {

namespace {

constexpr int kLanes = 64;
// Traceback: columns of stored state fetched per round trip (docs/DESIGN.md,
// "Aligner: memory waits off the per-column chain").
constexpr int kTbBatch = 6;

__device__ inline uint32_t base_code(uint32_t b) {
  // A=0 C=1 G=2 T=3, anything else 4 (matches nothing). Branch-free: bits 1-2
  // of the four letters are distinct (A 0, C 1, T 2, G 3), so they pick the
  // one letter b can be; the lanes of a wave hold different bases and a
  // switch would run every case in turn.
  const uint32_t k = (b >> 1) & 3;
  const uint32_t letter = (0x47544341u >> (k * 8)) & 0xffu;  // "ACTG"[k]
  return b == letter ? (k ^ (k >> 1)) : 4u;
}

// Bit x of the result is set where byte x of w equals c (x in 0..3).
__device__ inline uint32_t eq_bytes4(uint32_t w, uint32_t c) {
  const uint32_t x = w ^ (c * 0x01010101u);
  // bit 7 of a byte of y is clear exactly where that byte of x is zero; the
  // 7-bit add cannot carry into the next byte
  const uint32_t y = ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x;
  const uint32_t z = (~y & 0x80808080u) >> 7;
  // gathers bits 0, 8, 16, 24 into bits 24..27: the sixteen partial products
  // land on distinct bits, so nothing carries
  return (z * 0x01020408u) >> 24;
}
__device__ inline uint64_t eq_bytes8(uint64_t w, uint32_t c) {
  return eq_bytes4(static_cast<uint32_t>(w), c) |
         (eq_bytes4(static_cast<uint32_t>(w >> 32), c) << 4);
}

// Makes a loaded word count as used here, so that the wait for it is placed
// at this point (a rare path) and not at its first real use: the compiler
// would otherwise carry the load as possibly pending around the column loop
// and wait, on every column, for stores issued after it.
__device__ inline void arrive(uint64_t& x) { asm volatile("" : "+v"(x)); }

// band top block for column j: clamp(center/64 - K/2, [0, nbt-K]).
// center = (j * n) / m computed as a fixed-point multiply with a
// precomputed 32.32 step — the integer division was microcoded and ran
// once per column in the forward pass and twice per traceback step.
template <int K>
__device__ inline int32_t btop_of(uint64_t j, uint64_t step, int32_t nbt) {
  int32_t center_blk = static_cast<int32_t>((j * step) >> 32) >> 6;
  int32_t top = center_blk - K / 2;
  int32_t hi = nbt > K ? nbt - K : 0;
  return top < 0 ? 0 : (top > hi ? hi : top);
}

// D(row, col) from stored column state: S = bottom score of block rb,
// k = (row-1) & 63 its delta bit. Subtracts the deltas of rows below it.
__device__ inline int32_t score_at(int32_t S, uint64_t Pv, uint64_t Mv, uint32_t k) {
  const uint64_t mask = (k == 63) ? 0ull : (~0ull << (k + 1));
  return S - (__popcll(Pv & mask) - __popcll(Mv & mask));
}

// kEmitPath selects what the traceback produces. Both modes take the same
// moves in the same order; path mode stores one op byte per move, while
// breaking-point mode keeps the current window's record in registers and
// stores it (one 16-byte write) when the walk leaves the window.
//
// kAdaptive selects the band policy. Off: the band top of column j is
// btop_of(j), a function of j alone. On: the top starts at block 0, never
// moves up, and before each column slides down one block when the band's
// lowest row scores below its upper boundary row, or when it must to reach
// the last block by column m (docs/DESIGN.md, "Adaptive band";
// tools/sim_myers.py is the specification). The top is then a per-column
// fact the traceback has to read back, so the score buffer's column stride
// grows from K to K + 1 words and word K holds the column's band top.
template <int K, bool kEmitPath, bool kAdaptive>
__launch_bounds__(kLanes)
__global__ void myers_kernel(AlnDeviceArena a, uint32_t num_align) {
  constexpr int kSStride = kAdaptive ? K + 1 : K;  // sbuf words per column
  const uint32_t wave = blockIdx.x;
  const int lane = threadIdx.x;
  // lanes_per_wave < 64 under-fills waves on purpose: small jobs otherwise
  // give each CU ~1 wave and every load latency lands on the wall clock
  const uint32_t slot = wave * a.lanes_per_wave + lane;
  const bool active = lane < static_cast<int>(a.lanes_per_wave) && slot < num_align;

  const AlnWaveDesc wd = a.waves[wave];
  const uint32_t idx = active ? a.order[slot] : 0u;
  const AlnDesc desc = a.descs[idx];
  const int32_t n = active ? static_cast<int32_t>(desc.q_len) : 0;
  const int32_t m = active ? static_cast<int32_t>(desc.t_len) : 0;
  const int32_t nbt = (n + 63) >> 6;  // query blocks

  uint64_t* peq = a.peq + wd.peq_off;
  uint64_t* tb = a.tb + wd.tb_off;
  int32_t* sb = a.sbuf + wd.s_off;
  // 32.32 fixed-point slope for the band center (one division per lane)
  const uint64_t step = (m > 0) ? ((static_cast<uint64_t>(n) << 32) / static_cast<uint32_t>(m))
                                : 0;

  // The sequence arena is read in aligned 8-byte words. A word that holds a
  // byte of this lane's sequence may begin before the sequence (bytes of the
  // previous one) and end up to 7 bytes past the last sequence of the fill.
  // Both stay inside the arena's allocation: its base is 256-byte aligned
  // and AlignerBatch carves it in multiples of 256 bytes (allocate_arenas),
  // so the word that holds byte seq_cap - 1 ends inside the carve. No word
  // without a byte of the sequence is ever loaded, and the foreign bytes are
  // shifted or masked out.
  const uint64_t* seq64 = reinterpret_cast<const uint64_t*>(a.seqs);

  // ---- fill Peq (wave-coalesced layout [(b*4+c)*64+lane]) ----
  // A block's 64 query bytes lie in at most nine words: all are loaded
  // before the first is used, one round trip per block.
  for (uint32_t b = 0; b < wd.nb; ++b) {
    uint64_t mask[4] = {0, 0, 0, 0};
    const int32_t base = static_cast<int32_t>(b) << 6;
    if (base < n) {
      const int32_t lim = min(64, n - base);
      const uint32_t first = desc.q_offset + static_cast<uint32_t>(base);  // row 0's byte
      const uint32_t end = first + static_cast<uint32_t>(lim);
      const uint32_t r = first & 7;  // unaligned head: bytes of word 0 before row 0
      const uint32_t w0 = first >> 3;
      uint64_t word[9];
#pragma unroll
      for (uint32_t w = 0; w < 9; ++w) {
        word[w] = ((w0 + w) << 3) < end ? seq64[w0 + w] : 0ull;
      }
#pragma unroll
      for (uint32_t w = 0; w < 9; ++w) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          // byte x of word w is row 8 * w + x - r of the block
          const uint64_t e = eq_bytes8(word[w], static_cast<uint8_t>("ACGT"[c]));
          if (w == 0) {
            mask[c] |= e >> r;
          } else {
            mask[c] |= (e << (8 * w - 1 - r)) << 1;  // in two steps: 8 * 8 - 0 is 64
          }
        }
      }
      // tail shorter than a word: rows past the query match nothing
      const uint64_t keep = lim < 64 ? (1ull << lim) - 1 : ~0ull;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        mask[c] &= keep;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      peq[(static_cast<uint64_t>(b) * 4 + c) * kLanes + lane] = mask[c];
    }
  }

  // ---- column 0 state: D(i,0) = i ----
  uint64_t Pv[K], Mv[K];
  int32_t S[K];
  int32_t btop = 0;
#pragma unroll
  for (int b = 0; b < K; ++b) {
    Pv[b] = ~0ull;
    Mv[b] = 0ull;
    S[b] = (b + 1) * 64;
  }
  {
#pragma unroll
    for (int b = 0; b < K; ++b) {
      const uint64_t o = (static_cast<uint64_t>(0) * K + b) * 2;
      tb[(o + 0) * kLanes + lane] = Pv[b];
      tb[(o + 1) * kLanes + lane] = Mv[b];
      sb[(static_cast<uint64_t>(0) * kSStride + b) * kLanes + lane] = S[b];
    }
    if constexpr (kAdaptive) {
      sb[(static_cast<uint64_t>(0) * kSStride + K) * kLanes + lane] = 0;
    }
  }

  // ---- column loop (uniform bound; finished lanes coast) ----
  // K = 8, 16 and the adaptive band: Eq words for the next column are
  // prefetched during the current column's recurrence: the gather (64 lanes
  // x scattered 8 B) would otherwise sit on the critical path.
  //
  // The adaptive band's top for the next column is only known once this
  // column is done, so its prefetch takes K + 1 words, blocks btop .. btop + K
  // of the top it knows, and the column picks its K after the slide decision.
  // Block btop + K is read only while the band can still slide (btop < hi),
  // which keeps it below nbt and so inside the wave's peq region.
  //
  // Target codes come from registers: the target is read in aligned words,
  // one per eight columns, a word ahead of the one in use, so no column
  // waits for a byte of its own. code_of(k) is the code of t[k] and is called
  // once per k, in ascending order. The instantiations that keep the gather
  // (below) are at their register limits and take 4-byte words, two
  // registers for the pair instead of four.
  using TWord = std::conditional_t<K == 4 && !kAdaptive, uint64_t, uint32_t>;
  constexpr uint32_t kTShift = sizeof(TWord) == 8 ? 3 : 2;
  constexpr uint32_t kTMask = sizeof(TWord) - 1;
  const TWord* seqw = reinterpret_cast<const TWord*>(a.seqs);
  auto t_word = [&](uint32_t wi) -> TWord {  // word wi if it holds a target byte
    return (wi << kTShift) < desc.t_offset + static_cast<uint32_t>(m) ? seqw[wi] : TWord(0);
  };
  TWord tw = t_word(desc.t_offset >> kTShift);
  TWord twn = t_word((desc.t_offset >> kTShift) + 1);
  auto code_of = [&](int32_t k) -> uint32_t {
    const uint32_t tpos = desc.t_offset + static_cast<uint32_t>(k);
    if ((tpos & kTMask) == 0 && k != 0) {  // entered the next word
      tw = twn;
      twn = t_word((tpos >> kTShift) + 1);
    }
    return base_code(static_cast<uint32_t>(tw >> ((tpos & kTMask) * 8)) & 0xffu);
  };
  auto peq_at = [&](int32_t blk, uint32_t c) -> uint64_t {
    return peq[(static_cast<uint64_t>(blk) * 4 + c) * kLanes + lane];
  };
  // K = 4 on the diagonal keeps the Peq words of the band's blocks in
  // registers (RA / RC / RG / RT, 16 words) and selects a column's Eq by
  // code: nothing is gathered per column. Rn holds block btop + K, loaded right after a slide
  // for the next one, some 64 columns later when n is about m. A slide of
  // several blocks in one column (n many times m) reloads R outright.
  // Blocks read: btop .. btop + K - 1 <= max(nbt, K) - 1 < wd.nb, and
  // btop + K only while it is below nbt.
  constexpr bool kRegPeq = K == 4 && !kAdaptive;
  // one array per code: a select between two of them stays a select (a select
  // within one array would become a dynamic index, and the array scratch)
  constexpr int kRBlocks = kRegPeq ? K : 1;
  uint64_t RA[kRBlocks], RC[kRBlocks], RG[kRBlocks], RT[kRBlocks];
  auto Rw = [&](int c, int b) -> uint64_t& {  // c and b are unrolled constants
    return c == 0 ? RA[b] : c == 1 ? RC[b] : c == 2 ? RG[b] : RT[b];
  };
  uint64_t Rn[4];
  uint64_t EqN[kSStride];
  uint32_t cN = 4;
  const int32_t hi = nbt > K ? nbt - K : 0;  // adaptive: lowest band top
  if constexpr (kRegPeq) {
    if (m > 0) {
      cN = code_of(0);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int b = 0; b < K; ++b) {
        Rw(c, b) = peq_at(b, c);
      }
      Rn[c] = K < nbt ? peq_at(K, c) : 0ull;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int b = 0; b < K; ++b) {
        arrive(Rw(c, b));
      }
    }
  } else if (m > 0) {
    const uint32_t c1 = code_of(0);
    int32_t btopN = 0;
    if constexpr (!kAdaptive) {
      btopN = btop_of<K>(1, step, nbt);
    }
#pragma unroll
    for (int b = 0; b < K; ++b) {
      EqN[b] =
          (c1 < 4) ? peq[(static_cast<uint64_t>(btopN + b) * 4 + c1) * kLanes + lane] : 0ull;
    }
    if constexpr (kAdaptive) {
      EqN[K] = (c1 < 4 && 0 < hi) ? peq[(static_cast<uint64_t>(K) * 4 + c1) * kLanes + lane]
                                  : 0ull;
    }
  }
  uint64_t jstep = 0;  // j * step of the column at hand (K = 4 diagonal)
  for (int32_t j = 1; j <= static_cast<int32_t>(wd.mmax); ++j) {
    if (j <= m) {
      uint64_t EqC[K];
      if constexpr (kRegPeq) {
        const uint32_t cC = cN;
        if (j < m) {
          cN = code_of(j);
        }
        // btop_of(j) with j * step carried as a running sum: the 64-bit
        // multiply is a slow instruction and this wave has the SIMD to itself
        jstep += step;
        const int32_t top_c = (static_cast<int32_t>(jstep >> 32) >> 6) - K / 2;
        const int32_t btop_new = top_c < 0 ? 0 : (top_c > hi ? hi : top_c);
        if (btop < btop_new) {
          const bool one = btop_new == btop + 1;
          while (btop < btop_new) {
            // band slides down one block: drop top, append pessimistic bottom
#pragma unroll
            for (int b = 0; b < K - 1; ++b) {
              Pv[b] = Pv[b + 1];
              Mv[b] = Mv[b + 1];
              S[b] = S[b + 1];
            }
            Pv[K - 1] = ~0ull;
            Mv[K - 1] = 0ull;
            S[K - 1] = S[K - 2] + 64;
            ++btop;
          }
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            if (one) {
#pragma unroll
              for (int b = 0; b < K - 1; ++b) {
                Rw(c, b) = Rw(c, b + 1);
              }
              Rw(c, K - 1) = Rn[c];
            } else {
#pragma unroll
              for (int b = 0; b < K; ++b) {
                Rw(c, b) = peq_at(btop + b, c);
              }
            }
          }
          if (!one) {  // synchronous reload: the wait belongs to this path
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
              for (int b = 0; b < K; ++b) {
                arrive(Rw(c, b));
              }
            }
          }
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            Rn[c] = btop + K < nbt ? peq_at(btop + K, c) : 0ull;
          }
        }
        // branch-free select: a code of 4 (not A/C/G/T) matches nothing
        const bool odd = (cC & 1) != 0, high = (cC & 2) != 0, none = cC >= 4;
#pragma unroll
        for (int b = 0; b < K; ++b) {
          const uint64_t e01 = odd ? RC[b] : RA[b];
          const uint64_t e23 = odd ? RT[b] : RG[b];
          EqC[b] = none ? 0ull : (high ? e23 : e01);
        }
      } else if constexpr (!kAdaptive) {
#pragma unroll
        for (int b = 0; b < K; ++b) {
          EqC[b] = EqN[b];
        }
        // the column's own top is recomputed rather than carried: these
        // instantiations have no register to spare
        const int32_t btop_new = btop_of<K>(j, step, nbt);
        if (j < m) {  // issue next column's gather before the compute chain
          const uint32_t cn = code_of(j);
          const int32_t btopN = btop_of<K>(j + 1, step, nbt);
#pragma unroll
          for (int b = 0; b < K; ++b) {
            EqN[b] = (cn < 4)
                         ? peq[(static_cast<uint64_t>(btopN + b) * 4 + cn) * kLanes + lane]
                         : 0ull;
          }
        }
        while (btop < btop_new) {
          // band slides down one block: drop top, append pessimistic bottom
#pragma unroll
          for (int b = 0; b < K - 1; ++b) {
            Pv[b] = Pv[b + 1];
            Mv[b] = Mv[b + 1];
            S[b] = S[b + 1];
          }
          Pv[K - 1] = ~0ull;
          Mv[K - 1] = 0ull;
          S[K - 1] = S[K - 2] + 64;
          ++btop;
        }
      } else {
        // scores of column j - 1 on the band's upper boundary row and on its
        // lowest row; the second condition forces the slides that are left
        // when only as many columns remain
        const int32_t top = S[0] - (__popcll(Pv[0]) - __popcll(Mv[0]));
        const bool slide = btop < hi && (S[K - 1] < top || btop < hi - (m - j));
#pragma unroll
        for (int b = 0; b < K; ++b) {
          EqC[b] = slide ? EqN[b + 1] : EqN[b];
        }
        btop += slide ? 1 : 0;
        if (j < m) {  // issue next column's gather before the compute chain
          const uint32_t cn = code_of(j);
#pragma unroll
          for (int b = 0; b < K; ++b) {
            EqN[b] = (cn < 4)
                         ? peq[(static_cast<uint64_t>(btop + b) * 4 + cn) * kLanes + lane]
                         : 0ull;
          }
          EqN[K] = (cn < 4 && btop < hi)
                       ? peq[(static_cast<uint64_t>(btop + K) * 4 + cn) * kLanes + lane]
                       : 0ull;
        }
        if (slide) {
          // drop top, append pessimistic bottom (as above, at most once)
#pragma unroll
          for (int b = 0; b < K - 1; ++b) {
            Pv[b] = Pv[b + 1];
            Mv[b] = Mv[b + 1];
            S[b] = S[b + 1];
          }
          Pv[K - 1] = ~0ull;
          Mv[K - 1] = 0ull;
          S[K - 1] = S[K - 2] + 64;
        }
      }

      int32_t hin = 1;  // top boundary: D(top-1, j) - D(top-1, j-1) = +1
#pragma unroll
      for (int b = 0; b < K; ++b) {
        uint64_t Eq = EqC[b];
        const uint64_t hin_neg = (hin < 0) ? 1ull : 0ull;
        const uint64_t hin_pos = (hin > 0) ? 1ull : 0ull;
        const uint64_t Xv = Eq | Mv[b];
        Eq |= hin_neg;
        const uint64_t Xh = (((Eq & Pv[b]) + Pv[b]) ^ Pv[b]) | Eq;
        uint64_t Ph = Mv[b] | ~(Xh | Pv[b]);
        uint64_t Mh = Pv[b] & Xh;
        const int32_t hout =
            static_cast<int32_t>((Ph >> 63) & 1) - static_cast<int32_t>((Mh >> 63) & 1);
        Ph = (Ph << 1) | hin_pos;
        Mh = (Mh << 1) | hin_neg;
        Pv[b] = Mh | ~(Xv | Ph);
        Mv[b] = Ph & Xv;
        S[b] += hout;
        hin = hout;
      }

#pragma unroll
      for (int b = 0; b < K; ++b) {
        const uint64_t o = (static_cast<uint64_t>(j) * K + b) * 2;
        tb[(o + 0) * kLanes + lane] = Pv[b];
        tb[(o + 1) * kLanes + lane] = Mv[b];
        sb[(static_cast<uint64_t>(j) * kSStride + b) * kLanes + lane] = S[b];
      }
      if constexpr (kAdaptive) {
        sb[(static_cast<uint64_t>(j) * kSStride + K) * kLanes + lane] = btop;
      }
    }
  }

  if (!active) {
    return;
  }

  // ---- final score at (n, m) ----
  int32_t st = kAlnOk;
  int32_t D = 0;
  {
    const int32_t rb = ((n - 1) >> 6) - btop;
    if (rb < 0 || rb >= K) {
      st = kAlnBandEdge;
    } else {
      D = score_at(S[rb], Pv[rb], Mv[rb], (n - 1) & 63);
    }
  }
  a.edit_distance[idx] = (st == kAlnOk) ? D : -1;

  // ---- traceback: O(1) per step via stored column states ----
  uint8_t* path = a.path + desc.path_offset;
  uint32_t plen = 0;
  // Breaking-point mode walks the target's windows from the last one down.
  // `w` is the current window's record index and `lo` its lowest target
  // position; consuming a target position below `lo` closes the window. The
  // one modulo per lane here stands in for a division on every step.
  AlnBpRecord* recs = nullptr;
  AlnBpRecord rec = {kAlnBpNone, kAlnBpNone, kAlnBpNone, kAlnBpNone};
  int32_t w = 0;
  uint32_t lo = 0;
  if constexpr (!kEmitPath) {
    recs = a.bp + desc.bp_offset;
    w = static_cast<int32_t>(desc.bp_count) - 1;
    const uint32_t t_last = desc.t_origin + static_cast<uint32_t>(m) - 1;
    lo = t_last - t_last % a.window_length;
  }
  auto close_window = [&]() {
    if (w >= 0) {  // bp_count covers every window of the span; never stores below it
      recs[w] = rec;
    }
    --w;
    rec = {kAlnBpNone, kAlnBpNone, kAlnBpNone, kAlnBpNone};
  };
  int32_t i = n, j = m;
  // adaptive: recorded band tops of columns j and j - 1, carried in registers
  // and shifted when the walk changes column. After a failed final check
  // (e.g. m < hi: a slide on every column and still short of the last block)
  // nothing is read: the loop below does not run.
  auto top_of = [&](int32_t col) {
    return sb[(static_cast<uint64_t>(col) * kSStride + K) * kLanes + lane];
  };
  int32_t rtj = 0, rtj1 = 0;
  if constexpr (kAdaptive) {
    if (st == kAlnOk && j > 0) {
      rtj = top_of(j);
      rtj1 = top_of(j - 1);
    }
  }
  // The words of q and t that hold the walk's position stay in registers,
  // with the next lower word fetched when a word is entered: the walk goes
  // down a byte at a time, so it only ever leaves a word for that one. The
  // lower word's index is clamped to the arena's first word.
  uint32_t qwi = 0, twj = 0;
  uint64_t qw = 0, qwl = 0, tjw = 0, tjwl = 0;
  if (st == kAlnOk && i > 0 && j > 0) {
    qwi = (desc.q_offset + static_cast<uint32_t>(i) - 1) >> 3;
    twj = (desc.t_offset + static_cast<uint32_t>(j) - 1) >> 3;
    qw = seq64[qwi];
    qwl = seq64[qwi > 0 ? qwi - 1 : 0];
    tjw = seq64[twj];
    tjwl = seq64[twj > 0 ? twj - 1 : 0];
  }
  auto byte_at = [&](uint32_t pos, uint32_t& wi, uint64_t& word, uint64_t& lower) -> uint32_t {
    if ((pos >> 3) != wi) {
      word = lower;
      wi = pos >> 3;
      lower = seq64[wi > 0 ? wi - 1 : 0];
    }
    return static_cast<uint32_t>(word >> ((pos & 7) * 8)) & 0xffu;
  };
  // One move from the stored states of columns j (Pvj, Mvj) and j - 1 at the
  // row block of row i. Returns 0 after a move to column j - 1 (diagonal or
  // left), 1 after a move up, 2 when the walk ends here (st is set).
  auto tb_move = [&](uint64_t Pvj, uint64_t Mvj, uint64_t Pvj1, uint64_t Mvj1,
                     int32_t S1) -> int {
    const uint32_t k = (i - 1) & 63;
    const int32_t vd = ((Pvj >> k) & 1) ? 1 : (((Mvj >> k) & 1) ? -1 : 0);
    const int32_t D_left = score_at(S1, Pvj1, Mvj1, k);
    const int32_t vd1 = ((Pvj1 >> k) & 1) ? 1 : (((Mvj1 >> k) & 1) ? -1 : 0);
    const int32_t D_diag = D_left - vd1;
    const uint32_t cq =
        base_code(byte_at(desc.q_offset + static_cast<uint32_t>(i) - 1, qwi, qw, qwl));
    const uint32_t ct =
        base_code(byte_at(desc.t_offset + static_cast<uint32_t>(j) - 1, twj, tjw, tjwl));
    const int32_t sub = (cq != ct || cq >= 4) ? 1 : 0;
    // global position of the target base a diagonal or left move consumes
    const uint32_t tg = desc.t_origin + static_cast<uint32_t>(j) - 1;
    if (D_diag + sub == D) {
      if constexpr (kEmitPath) {
        path[plen++] = 0;  // M
      } else {
        if (tg < lo) {
          close_window();
          lo -= a.window_length;
        }
        // walking backwards: the first match met is the window's last one,
        // every later match is its first so far
        const uint32_t qg = desc.q_origin + static_cast<uint32_t>(i) - 1;
        if (rec.last_t == kAlnBpNone) {
          rec.last_t = tg + 1;
          rec.last_q = qg + 1;
        }
        rec.first_t = tg;
        rec.first_q = qg;
      }
      --i;
      --j;
      D = D_diag;
      return 0;
    }
    if (D_left + 1 == D) {
      if constexpr (kEmitPath) {
        path[plen++] = 2;  // D (consume target)
      } else {
        if (tg < lo) {
          close_window();
          lo -= a.window_length;
        }
      }
      --j;
      D = D_left;
      return 0;
    }
    if ((D - vd) + 1 == D) {
      if constexpr (kEmitPath) {
        path[plen++] = 1;  // I (consume query)
      }
      --i;
      D = D - vd;
      return 1;
    }
    st = kAlnBandEdge;
    return 2;
  };
  if constexpr (kAdaptive) {
    // The band top of a column is itself read back, so a column's address
    // depends on a load: the adaptive walk fetches its five state words per
    // move, as before, and only shares the q / t words above.
    while (st == kAlnOk && i > 0 && j > 0) {
      const int32_t babs = (i - 1) >> 6;
      const int32_t rbj = babs - rtj;
      const int32_t rbj1 = babs - rtj1;
      if (rbj < 0 || rbj >= K || rbj1 < 0 || rbj1 >= K) {
        st = kAlnBandEdge;
        break;
      }
      const uint64_t oj = (static_cast<uint64_t>(j) * K + rbj) * 2;
      const uint64_t oj1 = (static_cast<uint64_t>(j - 1) * K + rbj1) * 2;
      const uint64_t Pvj = tb[(oj + 0) * kLanes + lane];
      const uint64_t Mvj = tb[(oj + 1) * kLanes + lane];
      const uint64_t Pvj1 = tb[(oj1 + 0) * kLanes + lane];
      const uint64_t Mvj1 = tb[(oj1 + 1) * kLanes + lane];
      const int32_t S1 = sb[(static_cast<uint64_t>(j - 1) * kSStride + rbj1) * kLanes + lane];
      // the top of column j - 2, wanted if this step leaves column j
      const int32_t rtj2 = j >= 2 ? top_of(j - 2) : 0;
      if (tb_move(Pvj, Mvj, Pvj1, Mvj1, S1) == 0) {
        rtj = rtj1;
        rtj1 = rtj2;
      }
    }
  } else {
    // The diagonal band's top is a function of the column, so the states of
    // columns j .. j - kTbBatch at the walk's row block are fetched together,
    // one round trip, and up to kTbBatch column moves (with any up moves
    // between them) run from registers. The fetch predicts that the walk
    // stays in its row block; when it leaves the block (a crossing every 64
    // rows, or a long vertical run) the batch ends and the next one fetches
    // at the new block. Up moves change neither column nor batch slot.
    //
    // Every address fetched lies in this wave's tb / sbuf region: the column
    // is clamped to [0, j] with j <= m <= wd.mmax, the band block to [0, K).
    // A slot whose block was clamped is marked in `bad`; the walk reports
    // kAlnBandEdge when it needs such a slot, exactly where the per-move
    // check of rbj / rbj1 did, and never looks at what the slot holds.
    while (st == kAlnOk && i > 0 && j > 0) {
      const int32_t babs = (i - 1) >> 6;
      uint64_t CP[kTbBatch + 1], CM[kTbBatch + 1];
      int32_t CS[kTbBatch + 1];
      uint32_t bad = 0;
#pragma unroll
      for (int p = 0; p <= kTbBatch; ++p) {
        const int32_t col = max(j - p, 0);
        const int32_t rb = babs - btop_of<K>(col, step, nbt);
        bad |= (rb < 0 || rb >= K) ? (1u << p) : 0u;
        const int32_t rbc = min(max(rb, 0), K - 1);
        const uint64_t o = (static_cast<uint64_t>(col) * K + rbc) * 2;
        CP[p] = tb[(o + 0) * kLanes + lane];
        CM[p] = tb[(o + 1) * kLanes + lane];
        CS[p] = sb[(static_cast<uint64_t>(col) * kSStride + rbc) * kLanes + lane];
      }
      bool more = true;
#pragma unroll
      for (int p = 0; p < kTbBatch; ++p) {
        // slot p is column j, slot p + 1 column j - 1
        while (more) {
          if (i <= 0 || j <= 0 || ((i - 1) >> 6) != babs) {
            more = false;
            break;
          }
          if ((bad >> p) & 3u) {
            st = kAlnBandEdge;
            more = false;
            break;
          }
          const int mv = tb_move(CP[p], CM[p], CP[p + 1], CM[p + 1], CS[p + 1]);
          if (mv == 0) {
            break;
          }
          more = mv == 1;
        }
      }
    }
  }
  if constexpr (kEmitPath) {
    if (st == kAlnOk) {
      while (i > 0) {
        path[plen++] = 1;
        --i;
      }
      while (j > 0) {
        path[plen++] = 2;
        --j;
      }
    }
    a.path_len[idx] = (st == kAlnOk) ? plen : 0;
  } else {
    // The tail is a run of insertions (i > 0: no target consumed, nothing to
    // do) or of deletions (j > 0: every target position left is unmatched).
    // Either way the current window closes as it stands and every window
    // below it has no match, however many the deletion run crosses.
    if (st == kAlnOk) {
      while (w >= 0) {
        close_window();
      }
    }
  }
  a.status[idx] = st;
}

}  // namespace

namespace {
template <int K, bool kAdaptive>
void launch_k(const AlnDeviceArena& arena, uint32_t num_waves, uint32_t num_align,
              bool emit_path, hipStream_t s) {
  if (emit_path) {
    hipLaunchKernelGGL((myers_kernel<K, true, kAdaptive>), dim3(num_waves), dim3(kLanes), 0, s,
                       arena, num_align);
  } else {
    hipLaunchKernelGGL((myers_kernel<K, false, kAdaptive>), dim3(num_waves), dim3(kLanes), 0, s,
                       arena, num_align);
  }
}

template <bool kAdaptive>
void launch_policy(const AlnDeviceArena& arena, uint32_t num_waves, uint32_t num_align,
                   uint32_t band_k, bool emit_path, hipStream_t s) {
  switch (band_k) {
    case 4:
      launch_k<4, kAdaptive>(arena, num_waves, num_align, emit_path, s);
      break;
    case 8:
      launch_k<8, kAdaptive>(arena, num_waves, num_align, emit_path, s);
      break;
    default:
      launch_k<16, kAdaptive>(arena, num_waves, num_align, emit_path, s);
      break;
  }
}
}  // namespace

void launch_aligner_kernel(const AlnDeviceArena& arena, uint32_t num_waves, uint32_t num_align,
                           uint32_t band_k, bool emit_path, bool adaptive, void* stream) {
  auto s = static_cast<hipStream_t>(stream);
  if (adaptive) {
    launch_policy<true>(arena, num_waves, num_align, band_k, emit_path, s);
  } else {
    launch_policy<false>(arena, num_waves, num_align, band_k, emit_path, s);
  }
}

}  // namespace rga::hip
