// Beam search between the logits of step t and the operands of step t + 1, and the backtracking at its end.
//
// beam_advance_kernel: one workgroup per utterance, one ordinary launch per decoder step; no workgroup waits on another.
//   a. log-softmax per beam with the arithmetic of decoder.hip's beam_step_kernel (one wave per beam, lanes striding the row by
//      64, las_wave_max / __expf / las_wave_sum / __logf), so that the log-probs are bit-identical to las_beam_step's;
//   b. top K without the K V candidate buffer: the wave that owns a beam selects the beam's own best min(K, V) candidates in
//      order (a pass over the row per candidate: "the best one behind the last one taken", ties to the lower v), then one wave
//      merges the K sorted lists (a head per lane, ties to the lower beam).  The K best of all K V candidates are among the
//      per-beam K best, and the order (value, then flat index k V + v) restricted to a beam is the beam's own, so the winners and
//      their order are those of beam_step_kernel.  LDS holds K x K candidates whatever V is;
//   c. the beam state [B, K] re-ordered in place, the chosen words and parents into column t of the [B K, U] records, the word
//      into column t + 1 of the fed tokens;
//   d. the decoder state rows of the utterance permuted in place by the parents: a table of row-gather jobs, each staged through
//      LDS in column tiles with a barrier between the reads and the writes (duplicated parents are the normal case);
//   e. the embedded word into the next operand row (after the gathers: the row is one of their targets);
//   f. utt_done / remaining / steps_done: the workgroup whose utterance first has every beam finished takes one off `remaining`
//      (an integer atomic), the one that takes it to 0 writes steps_done = t + 1.
// Freeze: a launch for step t with 0 < *steps_done <= t writes nothing -- the search ended in an earlier launch (whose last
// workgroup left remaining == 0 and steps_done together), so steps enqueued past the end leave everything as it was.  The
// test is on steps_done and not on `remaining` because a workgroup of the CLOSING launch may start after the count reached 0
// and still has its own step to do; steps_done = t + 1 does not freeze step t.
//
// beam_gather_tree_kernel: tf.contrib.seq2seq.gather_tree, one thread per final beam.
#include "las_common.h"

namespace {

constexpr int BEAM_THREADS = 256;
constexpr int BEAM_WAVES = BEAM_THREADS / LAS_WAVE;
constexpr int BEAM_KMAX = LAS_BEAM_MAX_WIDTH;
constexpr int BEAM_STAGE_BYTES = 32 * 1024;             // K rows of one column tile
constexpr int BEAM_NONE = 0x7fffffff;

// (value, index) pairs in selection order: the larger value first, the lower index among equals; BEAM_NONE = no candidate
__device__ __forceinline__ void beam_wave_best(float& best, int& bi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oi != BEAM_NONE && (bi == BEAM_NONE || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
  }
}

template <typename T>
__device__ __forceinline__ void beam_gather_rows(char* base, int64_t stride, int64_t row_bytes, int K, const int* par, T* stage) {
  const int tid = threadIdx.x;
  const int64_t cols = row_bytes / (int64_t)sizeof(T);
  const int tile = BEAM_STAGE_BYTES / (int)sizeof(T) / K;            // elements of a row per tile (K <= 32: at least 256)
  for (int64_t c0 = 0; c0 < cols; c0 += tile) {
    const int w = (int)(cols - c0 < tile ? cols - c0 : tile);
    for (int k = 0; k < K; ++k) {
      const T* src = reinterpret_cast<const T*>(base + k * stride) + c0;
      for (int c = tid; c < w; c += BEAM_THREADS) stage[k * tile + c] = src[c];
    }
    __syncthreads();
    for (int j = 0; j < K; ++j) {
      const int k = par[j];
      if (k == j) continue;                                          // (the row is where it was)
      T* dst = reinterpret_cast<T*>(base + j * stride) + c0;
      for (int c = tid; c < w; c += BEAM_THREADS) dst[c] = stage[k * tile + c];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(BEAM_THREADS) void beam_advance_kernel(las_beam_adv a) {
  __shared__ float cval[BEAM_KMAX * BEAM_KMAX];          // [K][K]: beam k's best candidates in order
  __shared__ int cidx[BEAM_KMAX * BEAM_KMAX];            // their classes (-1: none)
  __shared__ float oldlp[BEAM_KMAX];
  __shared__ int oldfin[BEAM_KMAX], oldlen[BEAM_KMAX], par[BEAM_KMAX], word[BEAM_KMAX];
  __shared__ __attribute__((aligned(16))) unsigned stage[BEAM_STAGE_BYTES / 4];
  const int sd = *a.steps_done;
  if (sd > 0 && sd <= a.t) return;                       // frozen: the search ended in an earlier launch
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, V = a.V, eos = a.eos;
  const int n = K < V ? K : V;
  const float NEG = -3.402823466e38f;
  for (int k = wave; k < K; k += BEAM_WAVES) {
    const float* lg = a.logits + (int64_t)(b * K + k) * a.ldl;
    float mx = -INFINITY;
    for (int v = lane; v < V; v += 64) mx = fmaxf(mx, lg[v]);
    mx = las_wave_max(mx);
    float sum = 0.f;
    for (int v = lane; v < V; v += 64) sum += __expf(lg[v] - mx);
    sum = las_wave_sum(sum);
    const float lse = mx + __logf(sum);
    const float olp = a.log_probs[b * K + k];
    const int fin = a.finished[b * K + k];
    if (lane == 0) {
      oldlp[k] = olp;
      oldfin[k] = fin;
      oldlen[k] = a.lengths[b * K + k];
    }
    float pv = 0.f;                                      // the candidate taken last
    int pi = -1;
    for (int j = 0; j < n; ++j) {
      float best = -INFINITY;
      int bi = BEAM_NONE;
      if (pi != BEAM_NONE) {
        for (int v = lane; v < V; v += 64) {
          const float step = fin ? (v == eos ? 0.f : NEG) : lg[v] - lse;
          const float c = olp + step;
          const bool behind = pi < 0 || c < pv || (c == pv && v > pi);
          if (!(c != c) && behind && (bi == BEAM_NONE || c > best)) { best = c; bi = v; }      // NaN: never a candidate
        }
        beam_wave_best(best, bi);
      }
      if (lane == 0) {
        cval[k * K + j] = best;
        cidx[k * K + j] = bi == BEAM_NONE ? -1 : bi;
      }
      pv = best;
      pi = bi;
    }
  }
  __syncthreads();
  if (wave == 0) {
    // merge: lane k holds the head of beam k's list
    int pos = 0;
    float rl = -INFINITY;
    int rw = eos, rp = 0;
    for (int j = 0; j < K; ++j) {
      const bool has = lane < K && pos < n && cidx[lane * K + pos] >= 0;
      float best = has ? cval[lane * K + pos] : -INFINITY;
      int bk = has ? lane : BEAM_NONE;
      beam_wave_best(best, bk);
      if (bk == BEAM_NONE) break;                        // (fewer than K candidates that are numbers: the rest stay eos at -inf)
      const int wpos = __shfl(pos, bk, 64);
      if (lane == j) {
        rl = best;
        rp = bk;
        rw = cidx[bk * K + wpos];
      }
      if (lane == bk) ++pos;
    }
    bool nf = true;
    if (lane < K) {
      const int pf = oldfin[rp];
      nf = pf || rw == eos;
      const int64_t row = (int64_t)b * K + lane;
      a.log_probs[row] = rl;
      a.finished[row] = nf ? 1 : 0;
      a.lengths[row] = oldlen[rp] + (pf ? 0 : 1);
      a.word_ids[row * a.ld_rec + a.t] = rw;
      a.parent_ids[row * a.ld_rec + a.t] = rp;
      if (a.next_token) a.next_token[row * a.ld_tok + a.t + 1] = rw;
      par[lane] = rp;
      word[lane] = rw;
    }
    const bool all = __ballot(!nf) == 0ull;
    if (lane == 0 && all && a.utt_done[b] == 0) {
      a.utt_done[b] = 1;
      if (atomicSub(a.remaining, 1) == 1) *a.steps_done = a.t + 1;
    }
  }
  __syncthreads();
  for (int i = 0; i < a.njobs; ++i) {
    const las_beam_gather_job job = a.jobs[i];
    char* base = reinterpret_cast<char*>(job.base) + (int64_t)b * K * job.row_stride;
    const uint64_t align = (uint64_t)(uintptr_t)job.base | (uint64_t)job.row_stride | (uint64_t)job.row_bytes;
    if ((align & 3) == 0) beam_gather_rows<unsigned>(base, job.row_stride, job.row_bytes, K, par, stage);
    else if ((align & 1) == 0) beam_gather_rows<unsigned short>(base, job.row_stride, job.row_bytes, K, par, reinterpret_cast<unsigned short*>(stage));
    else beam_gather_rows<unsigned char>(base, job.row_stride, job.row_bytes, K, par, reinterpret_cast<unsigned char*>(stage));
  }
  if (a.x_next) {                                        // (behind the gathers' last barrier, or the one above)
    for (int j = 0; j < K; ++j) {
      const int w = word[j];
      if (w < 0 || w >= V) continue;
      const las_bf16* src = a.emb + (int64_t)w * a.ld_emb;
      las_bf16* dst = a.x_next + ((int64_t)b * K + j) * a.ldx;
      for (int c = tid; c < a.emb_cols; c += BEAM_THREADS) dst[c] = src[c];
    }
  }
}

__global__ __launch_bounds__(64) void beam_gather_tree_kernel(const int32_t* __restrict__ word_ids,
                                                              const int32_t* __restrict__ parent_ids, int64_t ld_rec, int col0,
                                                              int n, const int32_t* __restrict__ lengths, int B, int K, int eos,
                                                              int32_t* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= B * K) return;
  const int b = i / K, k = i % K;
  int len = 0;
  for (int q = 0; q < K; ++q) {
    const int l = lengths[b * K + q];
    len = l > len ? l : len;
  }
  len = len < n ? len : n;
  int32_t* o = out + (int64_t)b * n * K + k;             // out[b, t, k]
  for (int t = len; t < n; ++t) o[(int64_t)t * K] = eos;
  int parent = k;
  for (int t = len - 1; t >= 0; --t) {
    const int64_t at = ((int64_t)b * K + parent) * ld_rec + col0 + t;
    o[(int64_t)t * K] = word_ids[at];
    const int p = parent_ids[at];
    parent = p < 0 ? 0 : (p >= K ? K - 1 : p);           // (a record is never used as an index unchecked)
  }
  bool seen = false;
  for (int t = 0; t < len; ++t) {
    if (seen) o[(int64_t)t * K] = eos;
    else if (o[(int64_t)t * K] == eos) seen = true;
  }
}

}  // namespace

extern "C" int las_beam_advance(const las_beam_adv* args, void* stream) {
  LAS_REQUIRE(args, "las_beam_advance: null argument");
  const las_beam_adv& a = *args;
  LAS_REQUIRE(a.logits && a.log_probs && a.finished && a.lengths && a.word_ids && a.parent_ids && a.utt_done && a.remaining &&
                  a.steps_done,
              "las_beam_advance: null argument");
  LAS_REQUIRE(a.B > 0 && a.K > 0 && a.V > 0 && a.eos >= 0 && a.eos < a.V && a.t >= 0 && a.ldl >= a.V && a.ld_rec > a.t,
              "las_beam_advance: bad shape B=%d K=%d V=%d eos=%d t=%d", a.B, a.K, a.V, a.eos, a.t);
  LAS_REQUIRE(a.K <= LAS_BEAM_MAX_WIDTH, "las_beam_advance: beam_width %d exceeds the cap of %d beams", a.K, LAS_BEAM_MAX_WIDTH);
  LAS_REQUIRE((int64_t)a.B * a.K <= 0x7fffffff, "las_beam_advance: B * K = %lld rows", (long long)a.B * a.K);
  LAS_REQUIRE(a.njobs >= 0 && a.njobs <= LAS_BEAM_MAX_JOBS, "las_beam_advance: %d gather jobs (at most %d)", a.njobs,
              LAS_BEAM_MAX_JOBS);
  for (int i = 0; i < a.njobs; ++i)
    LAS_REQUIRE(a.jobs[i].base && a.jobs[i].row_bytes >= 0 && a.jobs[i].row_stride >= a.jobs[i].row_bytes,
                "las_beam_advance: gather job %d: rows of %lld bytes at stride %lld", i, (long long)a.jobs[i].row_bytes,
                (long long)a.jobs[i].row_stride);
  LAS_REQUIRE(!a.next_token || a.ld_tok > a.t + 1, "las_beam_advance: no column %d in the fed tokens", a.t + 1);
  LAS_REQUIRE(!a.x_next || (a.emb && a.emb_cols > 0 && a.ld_emb >= a.emb_cols && a.ldx >= a.emb_cols),
              "las_beam_advance: the embedded feed needs emb, emb_cols, ld_emb and ldx");
  hipLaunchKernelGGL(beam_advance_kernel, dim3(a.B), dim3(BEAM_THREADS), 0, (hipStream_t)stream, a);
  LAS_LAUNCH_CHECK("beam advance launch");
  return LAS_OK;
}

extern "C" int las_beam_gather_tree(const int32_t* word_ids, const int32_t* parent_ids, int64_t ld_rec, int col0, int n,
                                    const int32_t* lengths, int B, int K, int eos, int32_t* out, void* stream) {
  LAS_REQUIRE(word_ids && parent_ids && lengths && out, "las_beam_gather_tree: null argument");
  LAS_REQUIRE(B > 0 && K > 0 && n > 0 && col0 >= 0 && ld_rec >= (int64_t)col0 + n && (int64_t)B * K <= 0x7fffffff,
              "las_beam_gather_tree: bad shape B=%d K=%d n=%d col0=%d ld=%lld", B, K, n, col0, (long long)ld_rec);
  hipLaunchKernelGGL(beam_gather_tree_kernel, dim3((B * K + 63) / 64), dim3(64), 0, (hipStream_t)stream, word_ids, parent_ids,
                     ld_rec, col0, n, lengths, B, K, eos, out);
  LAS_LAUNCH_CHECK("beam gather tree launch");
  return LAS_OK;
}
