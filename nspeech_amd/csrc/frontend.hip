// Utterance front end on the device: the resampler of audio.load_wav and the frame energies behind trim_wav /
// trim_silence (include/nspeech_hip.h, "utterance front end").  All arithmetic here is float64 and none of it may be
// contracted into a fused multiply-add: the resampler's contract is bit equality with audio._resample_reference, whose
// every tap is four separately rounded operations.  build.sh compiles this file with -ffp-contract=off; the pragma
// below says the same where the arithmetic is, and tests/test_frontend_cpu.py reads the assembly for v_fma_f64.
#include "common.h"

#pragma clang fp contract(off)

// ------------------------------------------------------------------ ns_resample
// One thread per output sample, RS_BLOCK consecutive outputs per workgroup.  Their source span (RS_BLOCK / ratio + two
// wings, under 1 000 samples at 48 -> 20 kHz) is staged in LDS once as float64; a span that does not fit (extreme
// down-sampling ratios) is read from global memory instead.  The two tables are 256 KB each and live in L2; a tap step
// of one wave reads inside one num_table-entry (4 KB) stretch of each.  The up to ~700 dependent adds per thread are
// hidden by occupancy, never by reordering the sum.
constexpr int RS_BLOCK = 256;
constexpr long RS_LDS_MAX = 6144;      // staged samples (48 KB of float64) above which the span stays in global memory

struct rs_args {
  const void* x; int n_in;
  float* y; int n_out;
  const double* win; const double* delta; int nwin;
  double inv_ratio, scale, num_table;
  int index_step, max_taps;
  int staged;
};

// Indices are 32-bit (ns_resample refuses longer signals): v_cvt_i32_f64 is one instruction, while the 64-bit
// conversion expands into a sequence with fused multiply-adds of its own, and this kernel is kept free of every fma so
// that the assembly can be checked for a contraction by name.
template <typename T>
__global__ __launch_bounds__(RS_BLOCK) void resample_kernel(rs_args a) {
  extern __shared__ double rs_span[];
  const T* __restrict__ x = (const T*)a.x;
  const double* __restrict__ win = a.win;
  const double* __restrict__ delta = a.delta;
  const int j0 = blockIdx.x * RS_BLOCK;
  const int j = j0 + threadIdx.x;
  int lo = 0;
  if (a.staged) {       // uniform over the workgroup: the sources of its first and last output bound every tap
    const int jl = min(j0 + RS_BLOCK - 1, a.n_out - 1);
    lo = max(0, (int)((double)j0 * a.inv_ratio) - a.max_taps);
    const int hi = min(a.n_in - 1, (int)((double)jl * a.inv_ratio) + 1 + a.max_taps);
    for (int i = threadIdx.x; i <= hi - lo; i += RS_BLOCK) rs_span[i] = (double)x[lo + i];
    __syncthreads();
  }
  if (j >= a.n_out) return;
  const double tr = (double)j * a.inv_ratio;      // time register
  const int n = min((int)tr, a.n_in - 1);         // tr < n_in for every j < n_out: the clamp never binds, it bounds the reads
  const double frac = a.scale * (tr - (double)n);
  double acc = 0.0;
#pragma unroll
  for (int wing = 0; wing < 2; ++wing) {          // left: x[n], x[n-1], ...   right: x[n+1], x[n+2], ...
    const double fr = wing ? a.scale - frac : frac;
    const double idx = fr * a.num_table;
    const int off = (int)idx;
    const double eta = idx - (double)off;
    const int count = min(wing ? a.n_in - n - 1 : n + 1, (a.nwin - off) / a.index_step);
    const int base = wing ? n + 1 : n, sign = wing ? 1 : -1;
    int k = off;
    for (int i = 0; i < count; ++i, k += a.index_step) {
      const int src = base + sign * i;
      const double xv = a.staged ? rs_span[src - lo] : (double)x[src];
      const double w = win[k] + eta * delta[k];
      acc = acc + w * xv;
    }
  }
  a.y[j] = (float)acc;
}

extern "C" int64_t ns_resample_out_len(int64_t n_in, int sr_in, int sr_out) {
  if (n_in < 0 || sr_in <= 0 || sr_out <= 0) return -1;
  const double ratio = (double)sr_out / (double)sr_in;
  return (int64_t)((double)n_in * ratio);
}

extern "C" int ns_resample(const ns_resample_params* p, ns_stream_t s) {
  NS_CHECK_ARG(p, "ns_resample: null params");
  NS_CHECK_ARG(p->sr_in > 0 && p->sr_out > 0, "ns_resample: sample rates must be positive (%d -> %d)", p->sr_in, p->sr_out);
  NS_CHECK_ARG(p->n_in >= 0 && p->n_out == ns_resample_out_len(p->n_in, p->sr_in, p->sr_out),
               "ns_resample: n_out %ld is not ns_resample_out_len(%ld, %d, %d)", (long)p->n_out, (long)p->n_in, p->sr_in, p->sr_out);
  NS_CHECK_ARG(p->x_dtype == NS_F32 || p->x_dtype == NS_F64, "ns_resample: x_dtype must be NS_F32 or NS_F64");
  NS_CHECK_ARG(p->num_table > 0 && p->nwin > p->num_table, "ns_resample: bad table (nwin %ld, num_table %d)", (long)p->nwin, p->num_table);
  if (p->n_out == 0) return NS_OK;
  NS_CHECK_ARG(p->x && p->y && p->win && p->delta, "ns_resample: null pointer");
  NS_CHECK_ARG(p->n_in <= 0x7fffff00 && p->n_out <= 0x7fffff00 && p->nwin <= 0x7fffff00, "ns_resample: more than 2^31 samples");
  rs_args a;
  const double ratio = (double)p->sr_out / (double)p->sr_in;
  a.x = p->x; a.n_in = (int)p->n_in; a.y = p->y; a.n_out = (int)p->n_out;
  a.win = p->win; a.delta = p->delta; a.nwin = (int)p->nwin;
  a.inv_ratio = 1.0 / ratio;
  a.scale = ratio < 1.0 ? ratio : 1.0;
  a.num_table = (double)p->num_table;
  a.index_step = (int)(a.scale * p->num_table);
  NS_CHECK_ARG(a.index_step > 0, "ns_resample: ratio %d / %d is below the table's resolution", p->sr_out, p->sr_in);
  a.max_taps = a.nwin / a.index_step + 1;
  const long span = (long)(RS_BLOCK * a.inv_ratio) + 2 * a.max_taps + 4;
  a.staged = span <= RS_LDS_MAX;
  const size_t lds = a.staged ? sizeof(double) * span : 0;
  const dim3 grid((unsigned)ceil_div(p->n_out, RS_BLOCK));
  if (p->x_dtype == NS_F32) hipLaunchKernelGGL(resample_kernel<float>, grid, dim3(RS_BLOCK), lds, (hipStream_t)s, a);
  else hipLaunchKernelGGL(resample_kernel<double>, grid, dim3(RS_BLOCK), lds, (hipStream_t)s, a);
  NS_CHECK_LAUNCH("resample");
  return NS_OK;
}

// ------------------------------------------------------------------ ns_frame_power
// One workgroup per frame: every thread squares and adds its stride of the frame in float64, the workgroup adds the
// 256 partial sums in a fixed order.  The reflect padding is an index map, the padded signal never exists.
constexpr int FP_BLOCK = 256;

__global__ __launch_bounds__(FP_BLOCK) void frame_power_kernel(ns_frame_power_params p) {
  __shared__ double part[FP_BLOCK];
  const float* __restrict__ x = p.x;
  const long pad = p.frame_length / 2;
  const long q0 = (long)blockIdx.x * p.hop - pad;
  double s = 0.0;
  for (int t = threadIdx.x; t < p.frame_length; t += FP_BLOCK) {
    long i = q0 + t;
    if (i < 0) i = -i;
    if (i >= p.n) i = 2 * (p.n - 1) - i;
    const double v = (double)x[i];
    s = s + v * v;
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = FP_BLOCK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) p.out[blockIdx.x] = part[0] / (double)p.frame_length;
}

extern "C" int ns_frame_power(const ns_frame_power_params* p, ns_stream_t s) {
  NS_CHECK_ARG(p && p->x && p->out, "ns_frame_power: null");
  NS_CHECK_ARG(p->frame_length >= 2 && p->frame_length % 2 == 0 && p->hop > 0,
               "ns_frame_power: frame_length must be even and >= 2, hop positive (%d / %d)", p->frame_length, p->hop);
  NS_CHECK_ARG(p->n > p->frame_length / 2, "ns_frame_power: %ld samples cannot be reflect-padded by %d", (long)p->n, p->frame_length / 2);
  NS_CHECK_ARG(p->n_frames == 1 + p->n / p->hop && p->n_frames <= 0x7fffffff,
               "ns_frame_power: n_frames %ld is not 1 + n / hop = %ld", (long)p->n_frames, (long)(1 + p->n / p->hop));
  hipLaunchKernelGGL(frame_power_kernel, dim3((unsigned)p->n_frames), dim3(FP_BLOCK), 0, (hipStream_t)s, *p);
  NS_CHECK_LAUNCH("frame_power");
  return NS_OK;
}
