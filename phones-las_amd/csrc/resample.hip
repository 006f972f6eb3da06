// Band-limited resampling (resampy 0.2.2 'kaiser_best', as librosa 0.7.1's load / resample call it) over a ragged batch of
// utterances in one launch: the device side of audio.resample_batch (phones-las_amd/audio.py).
//
// Every output sample is resampy's resample_f for that sample, operation for operation: the interpolated window weight
// w = win[o] + eta * delta[o], the product w * x and the accumulation into float32 storage are separately rounded float64
// operations in tap order (left wing, then right wing).  So this translation unit turns FP contraction OFF (an FMA would round
// once where resampy rounds twice; tests/test_resample_host.py checks the ISA), and f32 denormals are kept (the default).
//
// The kernel reads the UNSCALED half window (float64, nwin entries plus one copy of the last, so that the last difference is
// exactly 0 as resampy's is) and forms win = half * ratio (ratio < 1 only) and delta = win[o + 1] - win[o] on the fly, with the
// same operations resampy uses to build its scaled copy: one table serves every rate of a batch.
//
// resampy's time register is a RUNNING float64 sum of 1 / ratio; the host hands it over as segments (t_b, start_b, step_b)
// inside which tr_t = start_b + (t - t_b) * step_b exactly (audio.time_segments), so no lane walks the sum serially.
//
// One output sample per lane; a workgroup covers consecutive outputs.  The window reads are L2 / L1 reads of a 256 KiB table:
// at 48 kHz every lane of a wave has frac = 0 (one address per tap), at 44.1 kHz the offsets differ per lane (gathers).
// No atomics, no inter-workgroup communication: deterministic by construction.
#include "las_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int RS_NUM_TABLE = 512;       // 2 ** precision, precision = 9 (kaiser_best)
constexpr int RS_THREADS = 256;

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ in_off, const int64_t* __restrict__ out_off,
    const int64_t* __restrict__ n_valid, const double* __restrict__ ratios, const int32_t* __restrict__ seg_off,
    const int64_t* __restrict__ seg_t, const double* __restrict__ seg_tr, const double* __restrict__ seg_step,
    const double* __restrict__ half, int nwin, int n_utt, int64_t total_out, float* __restrict__ y) {
  const int64_t g = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
  if (g >= total_out) return;
  // the utterance: the last u with out_off[u] <= g (empty outputs are skipped past)
  int lo = 0, hi = n_utt - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (out_off[mid] <= g) lo = mid; else hi = mid - 1;
  }
  const int u = lo;
  const int64_t t = g - out_off[u];
  const float* xu = x + in_off[u];
  const int64_t nx = in_off[u + 1] - in_off[u];
  const double ratio = ratios[u];
  if (ratio == 1.0) {                   // orig_sr == target_sr: librosa returns the signal itself
    y[g] = xu[t];
    return;
  }
  if (t >= n_valid[u]) {                // fix_length: zeros up to ceil(len * ratio)
    y[g] = 0.f;
    return;
  }
  // the time register: the last segment with seg_t <= t
  int b = seg_off[u], e = seg_off[u + 1] - 1;
  while (b < e) {
    const int mid = (b + e + 1) >> 1;
    if (seg_t[mid] <= t) b = mid; else e = mid - 1;
  }
  const double tr = seg_tr[b] + (double)(t - seg_t[b]) * seg_step[b];   // exact (audio.time_segments)

  const bool scaled = ratio < 1.0;
  const double scale = scaled ? ratio : 1.0;                            // min(1.0, ratio)
  const int step = (int)(scale * (double)RS_NUM_TABLE);                 // truncated: the stride quirk
  // (through uint32: the int64 conversion is lowered with an f64 FMA -- exact, but the ISA check then cannot tell it from a
  //  contracted product; audio.resample_batch refuses signals of 2^31 samples or more)
  const int64_t n = (int64_t)(uint32_t)tr;
  if (n >= nx) {                        // bounds guard (resampy would read past the signal; no rate / length in use gets here)
    y[g] = 0.f;
    return;
  }
  double frac = scale * (tr - (double)n);
  float acc = 0.f;
#pragma unroll 1
  for (int side = 0; side < 2; ++side) {
    if (side) frac = scale - frac;
    const double idx = frac * (double)RS_NUM_TABLE;
    const int off = (int)idx;
    const double eta = idx - (double)off;
    const int64_t by_table = (int64_t)((nwin - off) / step);
    int64_t cnt = side ? nx - n - 1 : n + 1;                           // range(): a negative count is no taps
    cnt = cnt < by_table ? cnt : by_table;
    const float* xs = side ? xu + n + 1 : xu + n;
    const int64_t dir = side ? 1 : -1;
#pragma unroll 4
    for (int64_t i = 0; i < cnt; ++i) {
      const int o = off + (int)i * step;
      double w0 = half[o], w1 = half[o + 1];
      if (scaled) {
        w0 = w0 * ratio;
        w1 = w1 * ratio;
      }
      const double w = w0 + eta * (w1 - w0);
      acc = (float)((double)acc + w * (double)xs[dir * i]);
    }
  }
  y[g] = acc;
}

}  // namespace

extern "C" int las_resample_batch(const float* x, const int64_t* in_off, const int64_t* out_off, const int64_t* n_valid,
                                  const double* ratio, const int32_t* seg_off, const int64_t* seg_t, const double* seg_tr,
                                  const double* seg_step, const double* half, int nwin, int n_utt, int64_t total_out, float* y,
                                  void* stream) {
  LAS_REQUIRE(x && in_off && out_off && n_valid && ratio && seg_off && seg_t && seg_tr && seg_step && half && y && n_utt > 0 &&
                  total_out > 0 && nwin > RS_NUM_TABLE,
              "las_resample_batch: bad arguments");
  const int64_t blocks = (total_out + RS_THREADS - 1) / RS_THREADS;
  LAS_REQUIRE(blocks <= 0x7fffffff, "las_resample_batch: too many output samples for one launch");
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)blocks), dim3(RS_THREADS), 0, (hipStream_t)stream, x, in_off, out_off,
                     n_valid, ratio, seg_off, seg_t, seg_tr, seg_step, half, nwin, n_utt, total_out, y);
  LAS_LAUNCH_CHECK("resample launch");
  return LAS_OK;
}
