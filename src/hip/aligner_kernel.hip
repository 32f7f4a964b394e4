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

#include "hip/aligner_types.hpp"

namespace rga::hip {

namespace {

constexpr int kLanes = 64;

__device__ inline uint32_t base_code(uint8_t b) {
  // A=0 C=1 G=2 T=3, anything else 4 (matches nothing)
  switch (b) {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    case 'T': return 3;
    default: return 4;
  }
}

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
  const uint8_t* q = a.seqs + desc.q_offset;
  const uint8_t* t = a.seqs + desc.t_offset;
  const int32_t nbt = (n + 63) >> 6;  // query blocks

  uint64_t* peq = a.peq + wd.peq_off;
  uint64_t* tb = a.tb + wd.tb_off;
  int32_t* sb = a.sbuf + wd.s_off;
  // 32.32 fixed-point slope for the band center (one division per lane)
  const uint64_t step = (m > 0) ? ((static_cast<uint64_t>(n) << 32) / static_cast<uint32_t>(m))
                                : 0;

  // ---- fill Peq (wave-coalesced layout [(b*4+c)*64+lane]) ----
  for (uint32_t b = 0; b < wd.nb; ++b) {
    uint64_t mask[4] = {0, 0, 0, 0};
    const int32_t base = static_cast<int32_t>(b) << 6;
    if (base < n) {
      const int32_t lim = min(64, n - base);
      for (int32_t k = 0; k < lim; ++k) {
        const uint32_t c = base_code(q[base + k]);
        if (c < 4) {
          mask[c] |= 1ull << k;
        }
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
  // Eq words for the next column are prefetched during the current column's
  // recurrence: the gather (64 lanes x scattered 8 B) is the only global
  // read in the loop and would otherwise sit on the critical path.
  //
  // The adaptive band's top for the next column is only known once this
  // column is done, so its prefetch takes K + 1 words, blocks btop .. btop + K
  // of the top it knows, and the column picks its K after the slide decision.
  // Block btop + K is read only while the band can still slide (btop < hi),
  // which keeps it below nbt and so inside the wave's peq region.
  uint64_t EqN[kSStride];
  int32_t btopN = 0;
  const int32_t hi = nbt > K ? nbt - K : 0;  // adaptive: lowest band top
  if (m > 0) {
    const uint32_t c1 = base_code(t[0]);
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
  for (int32_t j = 1; j <= static_cast<int32_t>(wd.mmax); ++j) {
    if (j <= m) {
      uint64_t EqC[K];
      if constexpr (!kAdaptive) {
#pragma unroll
        for (int b = 0; b < K; ++b) {
          EqC[b] = EqN[b];
        }
        const int32_t btop_new = btopN;
        if (j < m) {  // issue next column's gather before the compute chain
          const uint32_t cn = base_code(t[j]);
          btopN = btop_of<K>(j + 1, step, nbt);
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
          const uint32_t cn = base_code(t[j]);
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
  while (st == kAlnOk && i > 0 && j > 0) {
    const int32_t babs = (i - 1) >> 6;
    const uint32_t k = (i - 1) & 63;
    const int32_t btj = kAdaptive ? rtj : btop_of<K>(j, step, nbt);
    const int32_t btj1 = kAdaptive ? rtj1 : btop_of<K>(j - 1, step, nbt);
    const int32_t rbj = babs - btj;
    const int32_t rbj1 = babs - btj1;
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
    // adaptive: the top of column j - 2, wanted if this step leaves column j
    int32_t rtj2 = 0;
    if constexpr (kAdaptive) {
      rtj2 = j >= 2 ? top_of(j - 2) : 0;
    }

    const int32_t vd = ((Pvj >> k) & 1) ? 1 : (((Mvj >> k) & 1) ? -1 : 0);
    const int32_t D_left = score_at(S1, Pvj1, Mvj1, k);
    const int32_t vd1 = ((Pvj1 >> k) & 1) ? 1 : (((Mvj1 >> k) & 1) ? -1 : 0);
    const int32_t D_diag = D_left - vd1;
    const int32_t sub = (base_code(q[i - 1]) != base_code(t[j - 1]) ||
                         base_code(q[i - 1]) >= 4)
                            ? 1
                            : 0;
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
      if constexpr (kAdaptive) {
        rtj = rtj1;
        rtj1 = rtj2;
      }
    } else if (D_left + 1 == D) {
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
      if constexpr (kAdaptive) {
        rtj = rtj1;
        rtj1 = rtj2;
      }
    } else if ((D - vd) + 1 == D) {
      if constexpr (kEmitPath) {
        path[plen++] = 1;  // I (consume query)
      }
      --i;
      D = D - vd;
    } else {
      st = kAlnBandEdge;
      break;
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
