// Frame-level binary-feature accuracy (infer.py --calc_frame_binf_accuracy of the reference): the device side of
// phones-las_amd/frame_binf.py.
//
// dtw_kernel: per utterance of a ragged batch, fastdtw 0.3.x `dtw(range(U), range(T'), dist=lambda i, j: -A[i, j])` exactly,
// then the reference's soft2hard_attention cleanup and attention_to_segments.  The table is float64 (NumPy 1.16 promotes
// `0 + np.float32` to float64); every cell is D[i, j] = min(up + dt, left + dt, diag + dt) with dt = (double)(-A[i-1, j-1]), one
// separately rounded add per candidate (FP contraction is OFF in this file), and a candidate replaces the current minimum only
// when it is strictly smaller, in the order up, left, diagonal (Python's min).  The SUMS are compared, not the predecessors.
//
// One wave per utterance sweeps anti-diagonals over a band of 64 rows, a row per lane: lane l holds row r0 + l + 1 and at step s
// works on column s - l + 1.  The up and diagonal predecessors are lane l - 1's values of the previous two steps, handed over by
// a DPP wave_shr:1 of the f64 value (two v_mov_b32_dpp, no LDS, no barrier).  Lane 0 reads the row above the band from an LDS
// column, which the band's last row overwrites behind it for the next band.  Backpointers (2 bits per cell) are packed per row,
// 16 columns per 32-bit word that only the row's lane writes; they live in LDS when the batch's largest table fits
// DTW_BP_LDS_BYTES, otherwise in a device workspace (las_attention_dtw_workspace_bytes).  Lane 0 then walks the path back from
// (U, T') into per-column runs [lo, hi] (the path is monotone), cleans them and cuts the segments in one pass.
//
// frame_binf_count_kernel: per utterance, per feature, the number of frames whose predicted and target feature values agree
// (integers: exact in any order).  No atomics anywhere: deterministic by construction.
#include "las_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int DTW_THREADS = 64;                       // one wave per utterance
constexpr int DTW_CHUNK = 16;                         // steps per prefetched chunk of A (also columns per backpointer word)
constexpr size_t DTW_BP_LDS_BYTES = 64 * 1024;        // backpointers in LDS up to this size
constexpr int DTW_T_MAX = 8191;                       // the LDS column of D: 8 * (T' + 1) bytes <= 64 KiB
constexpr int CNT_THREADS = 256;
constexpr int MARKUP_SEARCH_WINDOW = 5;               // segments_to_attention's SEARCH_WINDOW (last_phone never advances)

__device__ __forceinline__ double shift_up_f64(double v) {   // lane l gets lane l - 1's value (lane 0: its own)
  const long long b = __builtin_bit_cast(long long, v);
  int lo = (int)b, hi = (int)(b >> 32);
  lo = __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);   // wave_shr:1
  hi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}

template <bool LDS_BP>
__device__ void dtw_utterance(const float* __restrict__ A, int U, int T, int ldu, double* dcol, uint32_t* bp_lds,
                              uint32_t* __restrict__ bp_ws, int32_t* __restrict__ run_lo, int32_t* __restrict__ run_hi,
                              int32_t* __restrict__ ph_st, int32_t* __restrict__ ph_en, int32_t* __restrict__ n_seg) {
  const int lane = threadIdx.x;
  const int W = (T + DTW_CHUNK - 1) / DTW_CHUNK;       // backpointer words per row
  const double INF = __builtin_huge_val();
  for (int j = lane; j <= T; j += DTW_THREADS) dcol[j] = j == 0 ? 0.0 : INF;     // row 0: D[0, 0] = 0, D[0, j] = inf
  __syncthreads();

  for (int r0 = 0; r0 < U; r0 += DTW_THREADS) {
    const int nrows = U - r0 < DTW_THREADS ? U - r0 : DTW_THREADS;
    const bool row_ok = lane < nrows;
    const int i = r0 + lane + 1;                        // this lane's row of D (1-based)
    const float* Ai = A + (int64_t)(row_ok ? i - 1 : 0) * ldu;
    const int nsteps = T + nrows - 1;
    double cur = INF;                                   // D[i, j - 1]: D[i, 0] = inf
    double diag_in = lane == 0 ? dcol[0] : INF;         // D[i - 1, j - 1] at j = 1
    uint32_t bits = 0;
    float nxt[DTW_CHUNK];
#pragma unroll
    for (int k = 0; k < DTW_CHUNK; ++k) {
      const int j = k - lane + 1;
      nxt[k] = (row_ok && j >= 1 && j <= T) ? Ai[j - 1] : 0.f;
    }
    for (int s0 = 0; s0 < nsteps; s0 += DTW_CHUNK) {
      float a[DTW_CHUNK];
      double above[DTW_CHUNK];                          // lane 0: the row above the band, read before the chunk overwrites it
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < DTW_CHUNK; ++k) {
          const int j = s0 + k + 1;
          above[k] = j <= T ? dcol[j] : INF;
        }
      }
#pragma unroll
      for (int k = 0; k < DTW_CHUNK; ++k) {
        a[k] = nxt[k];
        const int j = s0 + DTW_CHUNK + k - lane + 1;
        nxt[k] = (row_ok && j >= 1 && j <= T) ? Ai[j - 1] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < DTW_CHUNK; ++k) {
        const int j = s0 + k - lane + 1;                // this lane's column (1-based) at this step
        double up_in = shift_up_f64(cur);               // D[i - 1, j]: lane l - 1's value of the previous step
        if (lane == 0) up_in = above[k];
        if (row_ok && j >= 1 && j <= T) {
          const double dt = (double)(-a[k]);
          const double c_up = up_in + dt, c_left = cur + dt, c_diag = diag_in + dt;
          double best = c_up;
          uint32_t code = 0;
          if (c_left < best) { best = c_left; code = 1; }
          if (c_diag < best) { best = c_diag; code = 2; }
          cur = best;
          const int c = j - 1;
          bits |= code << (2 * (c & (DTW_CHUNK - 1)));
          if ((c & (DTW_CHUNK - 1)) == DTW_CHUNK - 1 || j == T) {
            const int64_t w = (int64_t)(i - 1) * W + (c / DTW_CHUNK);
            if (LDS_BP) bp_lds[w] = bits; else bp_ws[w] = bits;
            bits = 0;
          }
          if (lane == nrows - 1) dcol[j] = cur;         // the band's last row: the next band's row above
        }
        diag_in = up_in;
      }
    }
    __syncthreads();
    if (lane == 0) dcol[0] = INF;                        // D[r, 0] = inf below row 0
    __syncthreads();
  }

  // The path, walked back from (U, T') by one lane, into per-column runs [lo, hi] (the D column is free now).
  int32_t* lo_l = reinterpret_cast<int32_t*>(dcol);
  int32_t* hi_l = lo_l + T;
  if (lane == 0) {
    int i = U, j = T, last = -1;
    while (i > 0 && j > 0) {
      const int r = i - 1, c = j - 1;
      if (c != last) { hi_l[c] = r; last = c; }
      lo_l[c] = r;
      const int64_t w = (int64_t)r * W + (c / DTW_CHUNK);
      const uint32_t code = ((LDS_BP ? bp_lds[w] : bp_ws[w]) >> (2 * (c & (DTW_CHUNK - 1)))) & 3u;
      if (code == 0) --i;
      else if (code == 1) --j;
      else { --i; --j; }
    }
    if (i != 0 || j != 0) n_seg[0] = -2;                 // a NaN table: the path left the grid (the reference raises)
  }
  __syncthreads();
  if (n_seg[0] == -2) return;
  // The cleanup's comparison of each column, A[lo, c] > A[hi, c] on the runs before cleanup, by every lane (bit 30 of hi).
  for (int c = lane; c < T; c += DTW_THREADS) {
    const int lo = lo_l[c], hi = hi_l[c];
    if (hi > lo && A[(int64_t)lo * ldu + c] > A[(int64_t)hi * ldu + c]) hi_l[c] = hi | (1 << 30);
  }
  __syncthreads();
  if (lane != 0) return;
  // soft2hard_attention's cleanup (column c + 1 as it is before its cleanup, column c - 1 after its own) and
  // attention_to_segments (phone = the last row of the cleaned run) in one pass.
  int plo = 0, phi = -1;
  int st_frame = 0, st_phone = 0, en_phone = 0, nseg = 0;
  int lo = lo_l[0], hi = hi_l[0];
  for (int c = 0; c < T; ++c) {
    const bool gt = (hi >> 30) & 1;
    hi &= ~(1 << 30);
    int nlo = 0, nhi = -1;
    if (c + 1 < T) { nlo = lo_l[c + 1]; nhi = hi_l[c + 1]; }
    if (hi > lo) {
      if (gt) {
        if (c < T - 1 && hi >= nlo && hi <= (nhi & ~(1 << 30))) --hi;
      } else {
        if (c > 0 && lo >= plo && lo <= phi) ++lo;
      }
    }
    run_lo[c] = lo;
    run_hi[c] = hi;
    const int phone = hi;
    if (phone > en_phone && c > 0) {
      for (int f = st_frame; f < c; ++f) { ph_st[f] = st_phone; ph_en[f] = phone; }
      ++nseg;
      en_phone = phone;
      st_phone = phone;
      st_frame = c;
    }
    plo = lo;
    phi = hi;
    lo = nlo;
    hi = nhi;
  }
  for (int f = st_frame; f < T; ++f) { ph_st[f] = st_phone; ph_en[f] = U; }
  n_seg[0] = nseg + 1;
}

__global__ __launch_bounds__(DTW_THREADS) void dtw_kernel(const float* __restrict__ att, const int64_t* __restrict__ att_off,
                                                          const int32_t* __restrict__ rows, const int32_t* __restrict__ cols,
                                                          const int32_t* __restrict__ ld, int u_max, int t_max, int lds_bp_words,
                                                          int64_t ws_stride_words, const int64_t* __restrict__ out_off,
                                                          int32_t* __restrict__ run_lo, int32_t* __restrict__ run_hi,
                                                          int32_t* __restrict__ ph_st, int32_t* __restrict__ ph_en,
                                                          int32_t* __restrict__ n_seg, uint32_t* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int u = blockIdx.x;
  const int lane = threadIdx.x;
  const int U = rows[u], T = cols[u], ldu = ld[u];
  const int64_t oo = out_off[u];
  if (U < 0 || T < 0 || U > u_max || T > t_max || (U > 0 && T > 0 && ldu < T)) {   // the host checks these first
    if (lane == 0) n_seg[u] = -1;
    return;
  }
  if (U == 0 || T == 0) {                               // no phones (or no frames): no segments, empty runs
    for (int c = lane; c < T; c += DTW_THREADS) {
      run_lo[oo + c] = 0;
      run_hi[oo + c] = -1;
      ph_st[oo + c] = 0;
      ph_en[oo + c] = 0;
    }
    if (lane == 0) n_seg[u] = 0;
    return;
  }
  if (lane == 0) n_seg[u] = 0;
  __syncthreads();
  double* dcol = reinterpret_cast<double*>(smem);
  uint32_t* bp_lds = reinterpret_cast<uint32_t*>(smem + sizeof(double) * (size_t)(t_max + 1));
  const int64_t words = (int64_t)U * ((T + DTW_CHUNK - 1) / DTW_CHUNK);
  const float* A = att + att_off[u];
  if (words <= lds_bp_words)
    dtw_utterance<true>(A, U, T, ldu, dcol, bp_lds, nullptr, run_lo + oo, run_hi + oo, ph_st + oo, ph_en + oo, n_seg + u);
  else
    dtw_utterance<false>(A, U, T, ldu, dcol, nullptr, ws + (int64_t)u * ws_stride_words, run_lo + oo, run_hi + oo, ph_st + oo,
                         ph_en + oo, n_seg + u);
}

size_t dtw_bp_words(int u_max, int t_max) { return (size_t)u_max * (size_t)((t_max + DTW_CHUNK - 1) / DTW_CHUNK); }

// Per utterance: the predicted and the target feature vector of every counted frame, and the frames on which they agree.
// Target (get_binf_markup_frames): the OR of the rows of every markup segment [st, en) covering the frame.  Prediction: the OR of
// the P rows [ph_st, ph_en) of the frame's DTW segment, or (att != nullptr: --use_markup_segments) the OR of the P rows the
// covering markup segments chose (segments_to_attention: the phone whose attention peaks highest over the segment's frames among
// the first five, first maximum on ties as np.argmax, NaN as np.max / np.argmax treat it; no phone when the window is empty).
__global__ __launch_bounds__(CNT_THREADS) void frame_binf_count_kernel(
    const uint8_t* __restrict__ P, const int64_t* __restrict__ p_off, const int32_t* __restrict__ p_rows, int F,
    const int32_t* __restrict__ ph_st, const int32_t* __restrict__ ph_en, const int64_t* __restrict__ frame_off,
    const int32_t* __restrict__ seg, const uint8_t* __restrict__ seg_binf, const int64_t* __restrict__ seg_off,
    const float* __restrict__ att, const int64_t* __restrict__ att_off, const int32_t* __restrict__ att_cols,
    const int32_t* __restrict__ att_ld, const int32_t* __restrict__ n_frames, int32_t* __restrict__ seg_phone,
    int32_t* __restrict__ counts) {
  __shared__ int part[CNT_THREADS];
  const int u = blockIdx.x, tid = threadIdx.x;
  const uint8_t* Pu = P + p_off[u];
  const int U = p_rows[u];
  const int64_t s0 = seg_off[u], s1 = seg_off[u + 1];
  const int n = n_frames[u];
  const bool markup = att != nullptr;
  if (markup) {
    const float* A = att + att_off[u];
    const int Tc = att_cols[u], lda = att_ld[u];
    const int R = U < MARKUP_SEARCH_WINDOW ? U : MARKUP_SEARCH_WINDOW;
    for (int64_t k = s0 + tid; k < s1; k += CNT_THREADS) {
      const int st = seg[2 * k];
      int e = seg[2 * k + 1] > st + 1 ? seg[2 * k + 1] : st + 1;
      e = e < Tc ? e : Tc;
      int best = -1;
      float bv = 0.f;
      if (st < e) {
        for (int r = 0; r < R; ++r) {
          const float* Ar = A + (int64_t)r * lda;
          float m = Ar[st];
          for (int f = st + 1; f < e; ++f) {
            const float x = Ar[f];
            if (!(m != m) && (x != x || x > m)) m = x;            // np.max: NaN propagates
          }
          if (best < 0 || (!(bv != bv) && (m != m || m > bv))) {   // np.argmax: the first NaN, else the first maximum
            best = r;
            bv = m;
          }
        }
      }
      seg_phone[k] = best;
    }
    __syncthreads();
  }
  const int G = CNT_THREADS / F;
  const int g = tid / F, f = tid - g * F;
  int cnt = 0;
  if (g < G) {
    const int64_t fo = markup ? 0 : frame_off[u];
    for (int j = g; j < n; j += G) {
      int pred = 0, tgt = 0;
      if (!markup)
        for (int r = ph_st[fo + j]; r < ph_en[fo + j]; ++r) pred |= Pu[(int64_t)r * F + f];
      for (int64_t k = s0; k < s1; ++k) {
        if (seg[2 * k] <= j && j < seg[2 * k + 1]) {
          tgt |= seg_binf[k * F + f];
          if (markup) {
            const int r = seg_phone[k];
            if (r >= 0) pred |= Pu[(int64_t)r * F + f];
          }
        }
      }
      cnt += (pred != 0) == (tgt != 0);
    }
  }
  part[tid] = cnt;
  __syncthreads();
  if (tid < F) {
    int sum = 0;
    for (int k = 0; k < G; ++k) sum += part[k * F + tid];
    counts[(int64_t)u * F + tid] = sum;
  }
}

}  // namespace

extern "C" size_t las_attention_dtw_workspace_bytes(int u_max, int t_max, int n_utt) {
  if (u_max <= 0 || t_max <= 0 || n_utt <= 0) return 0;
  const size_t words = dtw_bp_words(u_max, t_max);
  if (words * 4 <= DTW_BP_LDS_BYTES) return 0;         // every table's backpointers fit in LDS
  return words * 4 * (size_t)n_utt;
}

extern "C" int las_attention_dtw_batch(const float* att, const int64_t* att_off, const int32_t* rows, const int32_t* cols,
                                       const int32_t* ld, int n_utt, int u_max, int t_max, const int64_t* out_off,
                                       int32_t* run_lo, int32_t* run_hi, int32_t* ph_st, int32_t* ph_en, int32_t* n_seg,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  LAS_REQUIRE(att_off && rows && cols && ld && out_off && n_seg && n_utt > 0 && u_max >= 0 && t_max >= 0,
              "las_attention_dtw_batch: bad arguments");
  LAS_REQUIRE(t_max <= DTW_T_MAX, "las_attention_dtw_batch: %d frames (at most %d)", t_max, DTW_T_MAX);
  LAS_REQUIRE(t_max == 0 || (run_lo && run_hi && ph_st && ph_en), "las_attention_dtw_batch: missing outputs");
  LAS_REQUIRE(u_max == 0 || t_max == 0 || att, "las_attention_dtw_batch: missing attention");
  const size_t need = las_attention_dtw_workspace_bytes(u_max, t_max, n_utt);
  LAS_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "las_attention_dtw_batch: workspace of %zu bytes needed",
              need);
  const size_t words = dtw_bp_words(u_max, t_max);
  const int lds_bp_words = need == 0 ? (int)words : (int)(DTW_BP_LDS_BYTES / 4);
  const size_t lds = sizeof(double) * (size_t)(t_max + 1) + (size_t)lds_bp_words * 4;
  // on every call: the attribute belongs to the current device, and a per-process flag would race between host threads
  const int rc = las_check_hip(hipFuncSetAttribute(reinterpret_cast<const void*>(&dtw_kernel),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                               "las_attention_dtw_batch: LDS attribute");
  if (rc) return rc;
  hipLaunchKernelGGL(dtw_kernel, dim3(n_utt), dim3(DTW_THREADS), lds, (hipStream_t)stream, att, att_off, rows, cols, ld, u_max,
                     t_max, lds_bp_words, need == 0 ? (int64_t)0 : (int64_t)words, out_off, run_lo, run_hi, ph_st, ph_en, n_seg,
                     reinterpret_cast<uint32_t*>(workspace));
  LAS_LAUNCH_CHECK("attention dtw launch");
  return LAS_OK;
}

extern "C" int las_frame_binf_count(const uint8_t* P, const int64_t* p_off, const int32_t* p_rows, int F, const int32_t* ph_st,
                                    const int32_t* ph_en, const int64_t* frame_off, const int32_t* seg, const uint8_t* seg_binf,
                                    const int64_t* seg_off, const float* att, const int64_t* att_off, const int32_t* att_cols,
                                    const int32_t* att_ld, const int32_t* n_frames, int n_utt, int32_t* seg_phone,
                                    int32_t* counts, void* stream) {
  LAS_REQUIRE(P && p_off && p_rows && seg && seg_binf && seg_off && n_frames && counts && n_utt > 0 && F > 0,
              "las_frame_binf_count: bad arguments");
  LAS_REQUIRE(F <= CNT_THREADS, "las_frame_binf_count: %d features (at most %d)", F, CNT_THREADS);
  LAS_REQUIRE(att ? (att_off && att_cols && att_ld && seg_phone) : (ph_st && ph_en && frame_off),
              "las_frame_binf_count: missing operands of the chosen mode");
  hipLaunchKernelGGL(frame_binf_count_kernel, dim3(n_utt), dim3(CNT_THREADS), 0, (hipStream_t)stream, P, p_off, p_rows, F, ph_st,
                     ph_en, frame_off, seg, seg_binf, seg_off, att, att_off, att_cols, att_ld, n_frames, seg_phone, counts);
  LAS_LAUNCH_CHECK("frame binf count launch");
  return LAS_OK;
}
