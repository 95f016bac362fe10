// Guided attention loss, alignment focus and the loss' gradient wrt the alignments (include/nspeech_hip.h,
// ns_guided_attention).  One workgroup per utterance: wave w takes the decoder steps w, w + 16, ... of the row, its lanes
// walk the encoder positions 64 apart (coalesced).  A lane keeps one partial sum over all its steps, a wave the sum of
// its steps' maxima; both end in block_sum's fixed tree, and a second, one-thread kernel adds the rows in index order.
// No atomics, no work area: the same inputs give the same bits.  At the benchmark shape (N 32, S 200, Tia 160) the pass
// reads 4 MB and read-modify-writes 4 MB - it is bound by its two launches, not by the bytes.
#include "common.h"

__global__ __launch_bounds__(1024) void guided_attention_kernel(ns_guided_attention_params p, float inv_2s2) {
  __shared__ float red[32];
  const int n = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int Tn = min(max(p.in_lengths[n], 1), p.Tia);
  const int Sn = p.out_steps ? min(max(p.out_steps[n], 1), p.S) : p.S;
  const float den = (float)Tn * (float)Sn;
  const float coef = p.grad_scale / ((float)p.N * den);
  const long base = (long)n * (p.S + 1) * p.Tia;
  float gsum = 0.f, fsum = 0.f;
  for (int s = wave; s < Sn; s += nw) {
    const float* __restrict__ a = p.align + base + (long)(s + 1) * p.Tia;
    float* __restrict__ da = p.da0 ? p.da0 + base + (long)(s + 1) * p.Tia : nullptr;
    float mx = -INFINITY;
    for (int t = lane; t < Tn; t += 64) {
      const float av = a[t];
      // t/T_n - s/S_n over the common denominator: the numerator is an exact integer, so the difference rounds once
      const float d = (float)((long)t * Sn - (long)s * Tn) / den;
      const float w = -expm1f(-(d * d) * inv_2s2);       // 1 - exp(.), without the cancellation near the diagonal
      gsum = fmaf(av, w, gsum);
      mx = fmaxf(mx, av);
      if (da) da[t] = fmaf(coef, w, da[t]);
    }
    fsum += wave_max(mx);
  }
  const float g = block_sum(gsum, red);
  const float f = block_sum(lane == 0 ? fsum : 0.f, red);
  if (threadIdx.x == 0) {
    p.row_out[2 * n] = g / den;
    p.row_out[2 * n + 1] = f / (float)Sn;
  }
}

__global__ void guided_attention_mean_kernel(const float* row_out, int N, float* acc) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float g = 0.f, f = 0.f;
  for (int n = 0; n < N; ++n) { g += row_out[2 * n]; f += row_out[2 * n + 1]; }
  acc[0] = g / (float)N;
  acc[1] = f / (float)N;
}

extern "C" int ns_guided_attention(const ns_guided_attention_params* p, ns_stream_t s) {
  NS_CHECK_ARG(p, "ns_guided_attention: null parameter block");
  NS_CHECK_ARG(p->align, "ns_guided_attention: align is null");
  NS_CHECK_ARG(p->in_lengths, "ns_guided_attention: in_lengths is null");
  NS_CHECK_ARG(p->row_out, "ns_guided_attention: row_out is null");
  NS_CHECK_ARG(p->sigma > 0.f, "ns_guided_attention: sigma must be positive (got %g)", (double)p->sigma);
  NS_CHECK_ARG(p->N >= 1, "ns_guided_attention: N must be at least 1 (got %d)", p->N);
  NS_CHECK_ARG(p->S >= 1, "ns_guided_attention: S must be at least 1 (got %d)", p->S);
  NS_CHECK_ARG(p->Tia >= 1, "ns_guided_attention: Tia must be at least 1 (got %d)", p->Tia);
  const float inv_2s2 = (float)(1.0 / (2.0 * (double)p->sigma * (double)p->sigma));
  hipLaunchKernelGGL(guided_attention_kernel, dim3(p->N), dim3(1024), 0, (hipStream_t)s, *p, inv_2s2);
  NS_CHECK_LAUNCH("guided_attention");
  if (p->acc) {
    hipLaunchKernelGGL(guided_attention_mean_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, (const float*)p->row_out, p->N,
                       p->acc);
    NS_CHECK_LAUNCH("guided_attention_mean");
  }
  return NS_OK;
}
