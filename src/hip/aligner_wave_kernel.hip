// HIP/CDNA4 banded Myers bit-vector aligner: one WAVEFRONT per alignment.
//
// The band is 64 blocks of 64 rows (4096 cells) and lies on the rectangle
// diagonal exactly as the lane kernel's does at K = 64 (aligner_kernel.hip;
// tools/sim_myers.py align(q, t, 64) is the specification, align_wave() the
// model of this schedule). No lane can hold 64 blocks, so a lane holds one:
// absolute block B lives on lane B & 63, and block B of column j is computed
// at step s = j + B. Both inputs of the blocked recurrence are then exactly
// one step old: (B - 1, j) was computed on the lane above, whose hout comes
// down through one DPP shift, and (B, j - 1) on the lane itself. The
// cross-lane cost is paid once per 64 cells.
//
// A slide moves no state between lanes. When the band's top passes block B,
// lane B & 63 idles for 64 steps and comes back as block B + 64: it builds
// that block's Eq masks from the query and starts pessimistic (Pv = ~0,
// Mv = 0) from the bottom score of the block above, which that lane hands
// down with hout. Pairs whose band would slide more than one block per
// column (aln_wave_single_slide) are refused by the host.
//
// Column states are stored by step, [s][lane]: one coalesced 1 KiB write to
// tb and 256 B to sbuf per step. The traceback is wave-uniform; it stages the
// states of 64 columns x 2 blocks in LDS per global round trip and walks
// there until it leaves the tile.
//
// Termination: the forward loop runs m + btop(m) + 63 steps, known before it
// starts; every traceback step lowers i + j; nothing waits on memory flags
// and no workgroup talks to another.
#include <hip/hip_runtime.h>

#include "hip/aligner_types.hpp"

namespace rga::hip {

namespace {

constexpr int kLanes = 64;
constexpr int kWaveK = 64;  // blocks per band: one per lane

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

// The lane kernel's btop_of at K = 64 (same 32.32 fixed-point slope).
__device__ inline int32_t btop_of(int32_t j, uint64_t step, int32_t nbt) {
  const int32_t center_blk =
      static_cast<int32_t>((static_cast<uint64_t>(j) * step) >> 32) >> 6;
  const int32_t top = center_blk - kWaveK / 2;
  const int32_t hi = nbt > kWaveK ? nbt - kWaveK : 0;
  return top < 0 ? 0 : (top > hi ? hi : top);
}

__device__ inline int32_t score_at(int32_t S, uint64_t Pv, uint64_t Mv, uint32_t k) {
  const uint64_t mask = (k == 63) ? 0ull : (~0ull << (k + 1));
  return S - (__popcll(Pv & mask) - __popcll(Mv & mask));
}

// v of the lane above; lane 0 gets lane 63's (blocks wrap around the wave).
__device__ inline int32_t from_lane_above(int32_t v) {
  const int32_t wrap = __builtin_amdgcn_readlane(v, kLanes - 1);
  return __builtin_amdgcn_update_dpp(wrap, v, 0x138, 0xf, 0xf, false);  // wave_shr:1
}

struct EqMasks {
  uint64_t a, c, g, t;
};

// Eq masks of query block B; blocks at or beyond nbt are empty.
__device__ inline EqMasks masks_of(const uint8_t* q, int32_t n, int32_t nbt, int32_t B) {
  EqMasks e = {0, 0, 0, 0};
  if (B < nbt) {
    const int32_t base = B << 6;
    const int32_t lim = min(64, n - base);
    for (int32_t k = 0; k < lim; ++k) {
      const uint32_t code = base_code(q[base + k]);
      e.a |= static_cast<uint64_t>(code == 0) << k;
      e.c |= static_cast<uint64_t>(code == 1) << k;
      e.g |= static_cast<uint64_t>(code == 2) << k;
      e.t |= static_cast<uint64_t>(code == 3) << k;
    }
  }
  return e;
}

// Traceback tile: columns jt - c (c = 0..63) of blocks Bc (row 0) and Bc - 1
// (row 1), with the query bases of both blocks and the target bases of the
// columns. ok = the cell's block lies in that column's band.
struct TbTile {
  uint64_t pv[2][kLanes];
  uint64_t mv[2][kLanes];
  int32_t s[2][kLanes];
  int32_t ok[2][kLanes];
  uint8_t qc[2][kLanes];  // base codes of blocks Bc / Bc - 1
  uint8_t tc[kLanes];     // base code of t[jt - c - 1]
};

template <bool kEmitPath>
__launch_bounds__(kLanes)
__global__ void myers_wave_kernel(AlnDeviceArena a, uint32_t num_align) {
  __shared__ TbTile tile;
  const uint32_t slot = blockIdx.x;
  if (slot >= num_align) {
    return;
  }
  const int lane = threadIdx.x;
  const AlnWaveDesc wd = a.waves[slot];
  const uint32_t idx = a.order[slot];
  const AlnDesc desc = a.descs[idx];
  const int32_t n = static_cast<int32_t>(desc.q_len);
  const int32_t m = static_cast<int32_t>(desc.t_len);
  const uint8_t* q = a.seqs + desc.q_offset;
  const uint8_t* t = a.seqs + desc.t_offset;
  const int32_t nbt = (n + 63) >> 6;
  const uint64_t step = (static_cast<uint64_t>(n) << 32) / static_cast<uint32_t>(m);

  // [s][lane]: 16 B of Pv/Mv in tb, 4 B of score in sbuf
  ulonglong2* tb = reinterpret_cast<ulonglong2*>(a.tb + wd.tb_off);
  int32_t* sb = a.sbuf + wd.s_off;

  // ---- column 0: D(i, 0) = i; block B at step B ----
  int32_t B = lane;
  EqMasks eq = masks_of(q, n, nbt, B);
  uint64_t Pv = ~0ull, Mv = 0ull;
  int32_t S = (lane + 1) * 64;
  tb[static_cast<size_t>(lane) * kLanes + lane] = make_ulonglong2(Pv, Mv);
  sb[static_cast<size_t>(lane) * kLanes + lane] = S;

  // ---- step loop ----
  const int32_t btop_m = btop_of(m, step, nbt);
  const int32_t last = m + btop_m + kWaveK - 1;  // step of the band's last block at column m
  int32_t hout = 0;
  // Step 0 computes nothing but has its recycle, like every step below: with
  // btop(1) = 1 (t_len = 1 under 4097..4160 rows, 4224 x 2, ...) block 0
  // leaves the band before its first column and lane 0 starts as block 64.
  if (1 - B >= 1 && B < btop_of(1, step, nbt)) {
    B += kWaveK;
    eq = masks_of(q, n, nbt, B);
  }
  // step 1: only block 0 has a column
  uint32_t c_cur = (1 - B >= 1) ? base_code(t[0]) : 4u;
  for (int32_t s = 1; s <= last; ++s) {
    // what the lane above produced at step s - 1
    const int32_t hin_above = from_lane_above(hout);
    const int32_t s_above = from_lane_above(S);

    const int32_t j = s - B;
    const bool in_cols = j >= 1 && j <= m;
    const int32_t bt = btop_of(in_cols ? j : 0, step, nbt);
    const int32_t bt_prev = btop_of(in_cols ? j - 1 : 0, step, nbt);
    const bool act = in_cols && B <= bt + kWaveK - 1;  // B >= bt: recycled in time

    // the block and the target base of the next step, fetched under this one
    int32_t jn = s + 1 - B;
    const bool recycle = jn >= 1 && jn <= m && B < btop_of(jn, step, nbt);
    const int32_t Bn = recycle ? B + kWaveK : B;
    jn = s + 1 - Bn;
    const uint32_t c_next = (jn >= 1 && jn <= m) ? base_code(t[jn - 1]) : 4u;

    if (act) {
      if (B > bt_prev + kWaveK - 1) {
        // the block enters the band at this column: pessimistic, below the
        // bottom score the block above had at column j - 1
        Pv = ~0ull;
        Mv = 0ull;
        S = (s_above - hin_above) + 64;
      }
      const int32_t hin = (B == bt) ? 1 : hin_above;  // band top: +1
      uint64_t Eq = c_cur == 0 ? eq.a : c_cur == 1 ? eq.c : c_cur == 2 ? eq.g
                    : c_cur == 3 ? eq.t : 0ull;
      const uint64_t hin_neg = (hin < 0) ? 1ull : 0ull;
      const uint64_t hin_pos = (hin > 0) ? 1ull : 0ull;
      const uint64_t Xv = Eq | Mv;
      Eq |= hin_neg;
      const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
      uint64_t Ph = Mv | ~(Xh | Pv);
      uint64_t Mh = Pv & Xh;
      hout = static_cast<int32_t>((Ph >> 63) & 1) - static_cast<int32_t>((Mh >> 63) & 1);
      Ph = (Ph << 1) | hin_pos;
      Mh = (Mh << 1) | hin_neg;
      Pv = Mh | ~(Xv | Ph);
      Mv = Ph & Xv;
      S += hout;
      tb[static_cast<size_t>(s) * kLanes + lane] = make_ulonglong2(Pv, Mv);
      sb[static_cast<size_t>(s) * kLanes + lane] = S;
    }
    if (recycle) {
      B = Bn;
      eq = masks_of(q, n, nbt, B);
    }
    c_cur = c_next;
  }

  // ---- final score at (n, m): on the lane of the query's last block ----
  int32_t st = kAlnOk;
  int32_t D = 0;
  {
    const int32_t Bf = (n - 1) >> 6;
    const int32_t rb = Bf - btop_m;
    if (rb < 0 || rb >= kWaveK) {
      st = kAlnBandEdge;
    } else {
      D = __shfl(score_at(S, Pv, Mv, (n - 1) & 63), Bf & (kLanes - 1));
    }
  }
  if (lane == 0) {
    a.edit_distance[idx] = (st == kAlnOk) ? D : -1;
  }
  // the traceback reads what other lanes stored
  __syncthreads();

  // ---- traceback: wave-uniform walk over LDS tiles ----
  uint8_t* path = a.path + desc.path_offset;
  uint32_t plen = 0;
  uint8_t my_op = 0;  // op plen' with plen' & 63 == lane, stored 64 at a time
  auto emit = [&](uint8_t op) {
    if ((plen & (kLanes - 1)) == static_cast<uint32_t>(lane)) {
      my_op = op;
    }
    ++plen;
    if ((plen & (kLanes - 1)) == 0) {
      path[plen - kLanes + lane] = my_op;
    }
  };
  // breaking-point mode: as in the lane kernel, the record of the current
  // window lives in registers (the same in every lane); lane 0 stores it
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
    if (w >= 0 && lane == 0) {  // bp_count covers every window of the span
      recs[w] = rec;
    }
    --w;
    rec = {kAlnBpNone, kAlnBpNone, kAlnBpNone, kAlnBpNone};
  };

  int32_t i = n, j = m;
  int32_t Bc = -2, jt = -1;  // no tile yet
  // i + j drops on every step; the counter states the bound
  for (int32_t left = n + m; left > 0 && st == kAlnOk && i > 0 && j > 0; --left) {
    const int32_t babs = (i - 1) >> 6;
    const uint32_t k = (i - 1) & 63;
    if (babs > Bc || babs < Bc - 1 || j > jt || j - 1 < jt - (kLanes - 1)) {
      // next tile: this lane fetches column j - lane of blocks babs, babs - 1
      __syncthreads();  // the walk is done with the old tile
      Bc = babs;
      jt = j;
      const int32_t jc = jt - lane;
      const int32_t btc = jc >= 0 ? btop_of(jc, step, nbt) : 0;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int32_t Bl = Bc - r;
        const bool ok = jc >= 0 && Bl >= btc && Bl <= btc + kWaveK - 1;
        ulonglong2 pm = make_ulonglong2(0, 0);
        int32_t sv = 0;
        if (ok) {
          const size_t at = static_cast<size_t>(jc + Bl) * kLanes + (Bl & (kLanes - 1));
          pm = tb[at];
          sv = sb[at];
        }
        tile.pv[r][lane] = pm.x;
        tile.mv[r][lane] = pm.y;
        tile.s[r][lane] = sv;
        tile.ok[r][lane] = ok ? 1 : 0;
        const int32_t qi = (Bl << 6) + lane;
        tile.qc[r][lane] = (qi >= 0 && qi < n) ? static_cast<uint8_t>(base_code(q[qi])) : 4;
      }
      tile.tc[lane] = jc >= 1 ? static_cast<uint8_t>(base_code(t[jc - 1])) : 4;
      __syncthreads();
    }
    const int r = Bc - babs;
    const int cj = jt - j;
    if (tile.ok[r][cj] == 0 || tile.ok[r][cj + 1] == 0) {
      st = kAlnBandEdge;
      break;
    }
    const uint64_t Pvj = tile.pv[r][cj];
    const uint64_t Mvj = tile.mv[r][cj];
    const uint64_t Pvj1 = tile.pv[r][cj + 1];
    const uint64_t Mvj1 = tile.mv[r][cj + 1];
    const int32_t S1 = tile.s[r][cj + 1];
    const uint32_t qcode = tile.qc[r][k];
    const uint32_t tcode = tile.tc[cj];

    const int32_t vd = ((Pvj >> k) & 1) ? 1 : (((Mvj >> k) & 1) ? -1 : 0);
    const int32_t D_left = score_at(S1, Pvj1, Mvj1, k);
    const int32_t vd1 = ((Pvj1 >> k) & 1) ? 1 : (((Mvj1 >> k) & 1) ? -1 : 0);
    const int32_t D_diag = D_left - vd1;
    const int32_t sub = (qcode != tcode || qcode >= 4) ? 1 : 0;
    // global position of the target base a diagonal or left move consumes
    const uint32_t tg = desc.t_origin + static_cast<uint32_t>(j) - 1;
    if (D_diag + sub == D) {
      if constexpr (kEmitPath) {
        emit(0);  // M
      } else {
        if (tg < lo) {
          close_window();
          lo -= a.window_length;
        }
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
    } else if (D_left + 1 == D) {
      if constexpr (kEmitPath) {
        emit(2);  // D (consume target)
      } else {
        if (tg < lo) {
          close_window();
          lo -= a.window_length;
        }
      }
      --j;
      D = D_left;
    } else if (vd == 1) {
      if constexpr (kEmitPath) {
        emit(1);  // I (consume query)
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
      for (; i > 0; --i) {
        emit(1);
      }
      for (; j > 0; --j) {
        emit(2);
      }
      // the ops of the last, partial group of 64
      if (static_cast<uint32_t>(lane) < (plen & (kLanes - 1))) {
        path[(plen & ~static_cast<uint32_t>(kLanes - 1)) + lane] = my_op;
      }
    }
    if (lane == 0) {
      a.path_len[idx] = (st == kAlnOk) ? plen : 0;
    }
  } else {
    // as in the lane kernel: the current window closes as it stands and
    // every window below it has no match
    if (st == kAlnOk) {
      while (w >= 0) {
        close_window();
      }
    }
  }
  if (lane == 0) {
    a.status[idx] = st;
  }
}

}  // namespace

void launch_aligner_wave_kernel(const AlnDeviceArena& arena, uint32_t num_align, bool emit_path,
                                void* stream) {
  auto s = static_cast<hipStream_t>(stream);
  if (emit_path) {
    hipLaunchKernelGGL((myers_wave_kernel<true>), dim3(num_align), dim3(kLanes), 0, s, arena,
                       num_align);
  } else {
    hipLaunchKernelGGL((myers_wave_kernel<false>), dim3(num_align), dim3(kLanes), 0, s, arena,
                       num_align);
  }
}

}  // namespace rga::hip
