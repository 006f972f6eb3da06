// Evaluation metrics on the device: the integer side of phones-las_amd/utils/metrics_utils.py and of the CTC head's
// `ctc_edit_distance` (model_helper.py:347-367 of the reference).  Every result is an integer and exact.
//
// edit_distance_kernel: per (hypothesis, reference) pair of two ragged int32 batches, read in place: the optional id mapping,
// the reference's dense_to_sparse(merge_repeated=True) (flag bit 0: append EOS, keep element i iff mapped[i] != mapped[i + 1],
// i is before the first EOS and mapped[i] != -1), then the unit-cost Levenshtein distance of the kept tokens.  One wave per
// pair.  The kept tokens are compacted with a ballot prefix count, 64 raw elements per pass.  The table is swept by
// anti-diagonals over bands of 64 hypothesis rows, a row per lane, as align.hip's DTW: lane l holds row r0 + l + 1 and at step s
// works on column s - l + 1; its up and diagonal predecessors are lane l - 1's values of the previous two steps (DPP wave_shr:1,
// no LDS, no barrier); lane 0 reads the row above the band from a column array that the band's last row overwrites behind it.
// Live storage is the two token lists and that one row: O(n + m).  They sit in LDS (12 KiB static: 13 workgroups fit a CU's
// 160 KiB, so the registers -- 119 VGPRs, four waves per SIMD, 16 pairs per CU -- bound occupancy, not LDS) when both raw
// lengths are at most ED_LDS_LEN, otherwise in the workgroup's slice of the workspace.  A workgroup walks the pairs blockIdx.x, blockIdx.x + gridDim.x, ..., so the workspace is
// bounded by the grid (ED_MAX_GRID), not by the number of pairs.
//
// ctc_greedy_kernel: tf.nn.ctc_greedy_decoder(merge_repeated=True) + sparse.to_dense of one utterance per wave, a frame per
// lane: first-index argmax over the classes, emitted iff it differs from the previous frame's and is not the blank (the last
// class), compacted to the front of the row by the same ballot prefix count.
#include "las_common.h"

namespace {

constexpr int ED_THREADS = 64;                        // one wave per pair
constexpr int ED_CHUNK = 16;                          // steps per prefetched chunk of reference tokens / of the row above
constexpr int ED_LDS_LEN = 1023;                      // raw lengths up to this: tokens and the row in LDS
constexpr int ED_LDS_WORDS = 3 * (ED_LDS_LEN + 1);    // hypothesis tokens | reference tokens | row of m + 1 entries
constexpr int ED_LEN_MAX = 8191;
constexpr int ED_MAX_GRID = 2048;                     // 8 workgroups on each of the 256 CUs
constexpr int CTC_THREADS = 64;

__device__ __forceinline__ int shift_up_i32(int v) {  // lane l gets lane l - 1's value (lane 0: its own)
  return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false);   // wave_shr:1
}

__device__ __forceinline__ int lanes_below(unsigned long long mask, int lane) {
  return __popcll(mask & ((1ull << lane) - 1ull));
}

// One element through the mapping; an id outside [0, n_map) is never used as an index (ok = false, value 0).
__device__ __forceinline__ int ed_mapped(const int32_t* __restrict__ x, int i, const int32_t* __restrict__ mapping, int n_map,
                                         bool& ok) {
  int v = x[i];
  if (mapping) {
    if ((unsigned)v >= (unsigned)n_map) {
      ok = false;
      return 0;
    }
    v = mapping[v];
  }
  return v;
}

// The kept tokens of x[0, L) into dst (at most L of them); returns their number, or -2 when an id is outside the mapping (the
// whole sequence is looked at, as the host maps every element before it cuts at the EOS).
__device__ __forceinline__ int ed_compact(const int32_t* __restrict__ x, int L, const int32_t* __restrict__ mapping, int n_map,
                                          int eos_id, bool merge, int32_t* dst) {
  const int lane = threadIdx.x;
  int count = 0;
  bool open = true, bad = false;                       // wave-uniform: before the first EOS; an id outside the mapping
  for (int base = 0; base < L; base += ED_THREADS) {
    const int i = base + lane;
    bool ok = true;
    const int v = i < L ? ed_mapped(x, i, mapping, n_map, ok) : eos_id;     // (behind the end: the appended EOS)
    int nx = __shfl_down(v, 1, ED_THREADS);
    if (lane == ED_THREADS - 1) nx = i + 1 < L ? ed_mapped(x, i + 1, mapping, n_map, ok) : eos_id;
    bad = bad || __ballot(!ok) != 0ull;
    bool keep = i < L;
    if (merge) {
      const unsigned long long eos = __ballot(i < L && v == eos_id);
      const int first = eos ? __ffsll((long long)eos) - 1 : ED_THREADS;    // the chunk's first EOS lane
      keep = keep && open && lane < first && v != nx && v != -1;
      open = open && eos == 0ull;
    }
    const unsigned long long km = __ballot(keep);
    if (keep) dst[count + lanes_below(km, lane)] = v;
    count += __popcll(km);
  }
  return bad ? -2 : count;
}

// Levenshtein distance of a[0, n) and b[0, m), n, m >= 1, unit costs; row: m + 1 entries of scratch.
__device__ __forceinline__ int ed_table(const int32_t* a, int n, const int32_t* b, int m, int32_t* row) {
  const int lane = threadIdx.x;
  for (int j = lane; j <= m; j += ED_THREADS) row[j] = j;                   // D[0, j] = j
  __syncthreads();
  for (int r0 = 0; r0 < n; r0 += ED_THREADS) {
    const int nrows = n - r0 < ED_THREADS ? n - r0 : ED_THREADS;
    const bool row_ok = lane < nrows;
    const int i = r0 + lane + 1;                        // this lane's row of D (1-based)
    const int ai = row_ok ? a[i - 1] : 0;
    const int nsteps = m + nrows - 1;
    int cur = i;                                        // D[i, j - 1]: D[i, 0] = i
    int diag_in = r0;                                   // lane 0: D[r0, 0]; the others take lane l - 1's D[i - 1, 0] below
    int nxt[ED_CHUNK];
#pragma unroll
    for (int k = 0; k < ED_CHUNK; ++k) {
      const int j = k - lane + 1;
      nxt[k] = (j >= 1 && j <= m) ? b[j - 1] : 0;
    }
    for (int s0 = 0; s0 < nsteps; s0 += ED_CHUNK) {
      int bt[ED_CHUNK], above[ED_CHUNK];                // lane 0: the row above the band, read before the chunk overwrites it
#pragma unroll
      for (int k = 0; k < ED_CHUNK; ++k) {
        const int j = s0 + k + 1;
        above[k] = (lane == 0 && j <= m) ? row[j] : 0;
      }
#pragma unroll
      for (int k = 0; k < ED_CHUNK; ++k) {
        bt[k] = nxt[k];
        const int j = s0 + ED_CHUNK + k - lane + 1;
        nxt[k] = (j >= 1 && j <= m) ? b[j - 1] : 0;
      }
#pragma unroll
      for (int k = 0; k < ED_CHUNK; ++k) {
        const int j = s0 + k - lane + 1;                // this lane's column (1-based) at this step
        int up_in = shift_up_i32(cur);                  // D[i - 1, j]: lane l - 1's value of the previous step
        if (lane == 0) up_in = above[k];
        if (row_ok && j >= 1 && j <= m) {
          const int sub = diag_in + (ai != bt[k] ? 1 : 0);
          const int step = (cur < up_in ? cur : up_in) + 1;
          cur = sub < step ? sub : step;
          if (lane == nrows - 1) row[j] = cur;          // the band's last row: the next band's row above
        }
        diag_in = up_in;
      }
    }
    __syncthreads();
    if (lane == 0) row[0] = r0 + nrows;                 // D[r, 0] = r
    __syncthreads();
  }
  return row[m];
}

__device__ __forceinline__ void ed_pair(const int32_t* __restrict__ h, int hl, const int32_t* __restrict__ r, int rl,
                                        const int32_t* __restrict__ mapping, int n_map, int eos_id, bool merge, int32_t* a,
                                        int32_t* b, int32_t* row, int32_t* dist, int32_t* hyp_n, int32_t* ref_n) {
  const int n = ed_compact(h, hl, mapping, n_map, eos_id, merge, a);
  const int m = ed_compact(r, rl, mapping, n_map, eos_id, merge, b);
  __syncthreads();
  int d;
  if (n < 0 || m < 0) d = -2;
  else if (n == 0 || m == 0) d = n + m;
  else d = ed_table(a, n, b, m, row);
  if (threadIdx.x == 0) {
    *dist = d;
    *hyp_n = n < 0 ? 0 : n;
    *ref_n = m < 0 ? 0 : m;
  }
  __syncthreads();                                      // the next pair of this workgroup reuses a, b and row
}

__global__ __launch_bounds__(ED_THREADS) void edit_distance_kernel(
    const int32_t* __restrict__ hyp, int64_t hyp_size, const int64_t* __restrict__ hyp_off, const int32_t* __restrict__ hyp_len,
    const int32_t* __restrict__ ref, int64_t ref_size, const int64_t* __restrict__ ref_off, const int32_t* __restrict__ ref_len,
    const int32_t* __restrict__ ref_of_hyp, int n_pairs, int n_refs, const int32_t* __restrict__ mapping, int n_map, int eos_id,
    int flags, int len_max, int32_t* __restrict__ dist, int32_t* __restrict__ hyp_n, int32_t* __restrict__ ref_n,
    int32_t* __restrict__ ws) {
  __shared__ int32_t lds[ED_LDS_WORDS];
  const bool merge = (flags & 1) != 0;
  for (int p = blockIdx.x; p < n_pairs; p += gridDim.x) {
    const int q = ref_of_hyp ? ref_of_hyp[p] : p;
    bool ok = q >= 0 && q < n_refs;
    int hl = 0, rl = 0;
    int64_t ho = 0, ro = 0;
    if (ok) {
      hl = hyp_len[p];
      rl = ref_len[q];
      ho = hyp_off[p];
      ro = ref_off[q];
      // nothing is read of a pair whose lengths leave len_max or whose sequences leave the buffers
      ok = hl >= 0 && rl >= 0 && hl <= len_max && rl <= len_max && ho >= 0 && ro >= 0 && ho + hl <= hyp_size &&
           ro + rl <= ref_size;
    }
    if (!ok) {
      if (threadIdx.x == 0) {
        dist[p] = -1;
        hyp_n[p] = 0;
        ref_n[p] = 0;
      }
      continue;
    }
    if (hl <= ED_LDS_LEN && rl <= ED_LDS_LEN) {
      ed_pair(hyp + ho, hl, ref + ro, rl, mapping, n_map, eos_id, merge, lds, lds + (ED_LDS_LEN + 1), lds + 2 * (ED_LDS_LEN + 1),
              dist + p, hyp_n + p, ref_n + p);
    } else {                                            // (the host gave a workspace: len_max > ED_LDS_LEN)
      int32_t* base = ws + (int64_t)blockIdx.x * 3 * (len_max + 1);
      ed_pair(hyp + ho, hl, ref + ro, rl, mapping, n_map, eos_id, merge, base, base + (len_max + 1), base + 2 * (len_max + 1),
              dist + p, hyp_n + p, ref_n + p);
    }
  }
}

int ed_grid(int n_pairs) { return n_pairs < ED_MAX_GRID ? n_pairs : ED_MAX_GRID; }

__global__ __launch_bounds__(CTC_THREADS) void ctc_greedy_kernel(const float* __restrict__ logits, int64_t ld,
                                                                 const int32_t* __restrict__ logit_len, int T, int C,
                                                                 int32_t* __restrict__ decoded, int32_t* __restrict__ dec_len) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int L = logit_len[b];
  L = L < 0 ? 0 : (L > T ? T : L);
  const float* X = logits + (int64_t)b * T * ld;
  int32_t* out = decoded + (int64_t)b * T;
  const int blank = C - 1;
  int count = 0, carry = -1;                            // the class of the frame before this chunk
  for (int base = 0; base < L; base += CTC_THREADS) {
    const int t = base + lane;
    int cls = blank;
    if (t < L) {
      const float* x = X + (int64_t)t * ld;
      float best = x[0];
      cls = 0;
      for (int c = 1; c < C; ++c) {
        const float v = x[c];
        if (v > best) {                                 // strictly greater: the first index wins a tie (tf.argmax)
          best = v;
          cls = c;
        }
      }
    }
    int prev = shift_up_i32(cls);
    if (lane == 0) prev = carry;
    const bool emit = t < L && cls != prev && cls != blank;
    const unsigned long long em = __ballot(emit);
    if (emit) out[count + lanes_below(em, lane)] = cls;  // count + rank <= t < T
    count += __popcll(em);
    carry = __builtin_amdgcn_readlane(cls, CTC_THREADS - 1);
  }
  for (int t = count + lane; t < T; t += CTC_THREADS) out[t] = 0;
  if (lane == 0) dec_len[b] = count;
}

}  // namespace

extern "C" size_t las_edit_distance_workspace_bytes(int len_max, int n_pairs) {
  if (len_max <= ED_LDS_LEN || n_pairs <= 0) return 0;  // every pair fits in LDS
  return (size_t)ed_grid(n_pairs) * 3 * (size_t)(len_max + 1) * sizeof(int32_t);
}

extern "C" int las_edit_distance_batch(const int32_t* hyp, int64_t hyp_size, const int64_t* hyp_off, const int32_t* hyp_len,
                                       const int32_t* ref, int64_t ref_size, const int64_t* ref_off, const int32_t* ref_len,
                                       const int32_t* ref_of_hyp, int n_pairs, int n_refs, const int32_t* mapping, int n_map,
                                       int eos_id, int flags, int len_max, int32_t* dist, int32_t* hyp_n, int32_t* ref_n,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  LAS_REQUIRE(hyp_off && hyp_len && ref_off && ref_len && dist && hyp_n && ref_n && n_pairs > 0 && n_refs > 0 && hyp_size >= 0 &&
                  ref_size >= 0 && len_max >= 0,
              "las_edit_distance_batch: bad arguments");
  LAS_REQUIRE(ref_of_hyp || n_refs == n_pairs, "las_edit_distance_batch: %d references for %d pairs without ref_of_hyp", n_refs,
              n_pairs);
  LAS_REQUIRE((hyp || hyp_size == 0) && (ref || ref_size == 0), "las_edit_distance_batch: missing sequences");
  LAS_REQUIRE(len_max <= ED_LEN_MAX, "las_edit_distance_batch: %d tokens (at most %d)", len_max, ED_LEN_MAX);
  LAS_REQUIRE(mapping ? n_map > 0 : n_map == 0, "las_edit_distance_batch: mapping and n_map disagree");
  LAS_REQUIRE((flags & ~1) == 0, "las_edit_distance_batch: unknown flags %d", flags);
  const size_t need = las_edit_distance_workspace_bytes(len_max, n_pairs);
  LAS_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "las_edit_distance_batch: workspace of %zu bytes needed", need);
  hipLaunchKernelGGL(edit_distance_kernel, dim3(ed_grid(n_pairs)), dim3(ED_THREADS), 0, (hipStream_t)stream, hyp, hyp_size, hyp_off,
                     hyp_len, ref, ref_size, ref_off, ref_len, ref_of_hyp, n_pairs, n_refs, mapping, n_map, eos_id, flags, len_max,
                     dist, hyp_n, ref_n, reinterpret_cast<int32_t*>(workspace));
  LAS_LAUNCH_CHECK("edit distance launch");
  return LAS_OK;
}

extern "C" int las_ctc_greedy_batch(const float* logits, int64_t ld, const int32_t* logit_len, int B, int T, int C,
                                    int32_t* decoded, int32_t* dec_len, void* stream) {
  LAS_REQUIRE(logits && logit_len && decoded && dec_len && B > 0 && T > 0 && C > 0 && ld >= C,
              "las_ctc_greedy_batch: bad arguments");
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3(B), dim3(CTC_THREADS), 0, (hipStream_t)stream, logits, ld, logit_len, T, C, decoded,
                     dec_len);
  LAS_LAUNCH_CHECK("ctc greedy launch");
  return LAS_OK;
}
