// Tacotron-2 stop token (include/nspeech_hip.h, ns_stop_token): the projection z = h . w + b of every decoder step, and in
// the same pass the weighted sigmoid cross entropy against "this step is the last one", its gradient into dh / dw / db,
// and the step at which each utterance stops.
// A wave owns a row (n, s): every lane loads its D / 64 values of the row once (16 bytes per load where D is a multiple of
// 256 and the rows are aligned), keeps them in registers, and the dot product ends in wave_sum's fixed tree.  In training
// the wave then forms dz, updates its dh row and adds dz * h to its lanes' share of dw with the registers still warm: h is
// read once, dh is read and written once.  A workgroup of 8 waves takes 32 consecutive rows, 4 per wave; its waves add their
// dw shares in wave order through LDS, and the workgroup's partial dw, db and loss go to `work`.  A second small kernel adds
// the partials in index order (in double) and finds the stop steps from the logits the first one left in `work`.
// The grid depends on (N, S, D) only, there is no float atomic: the same inputs give the same bits on every device.
#include "common.h"
#include <math.h>

#define ST_ROWS 32          // rows (n, s) per workgroup
#define ST_WAVES 8
#define ST_RPW (ST_ROWS / ST_WAVES)

static inline long st_groups(long rows) { return (rows + ST_ROWS - 1) / ST_ROWS; }

// work: [G][D] dw partials | [G] loss partials | [G] db partials | [N S] logits | [N] |S^_n - S_n|
extern "C" size_t ns_stop_token_work_floats(int N, int S, int D) {
  if (N < 1 || S < 1 || D < 1) return 0;
  const long rows = (long)N * S, G = st_groups(rows);
  return (size_t)(G * D + 2 * G + rows + N);
}

// element e of a lane: column e * 64 + lane, or (VEC) the e % 4-th of the four columns (e / 4) * 256 + lane * 4 ..
template <bool VEC> __device__ __forceinline__ int st_col(int e, int lane) {
  return VEC ? (e >> 2) * 256 + lane * 4 + (e & 3) : e * 64 + lane;
}

template <typename T, int MAXJ, bool VEC>
__device__ __forceinline__ void st_load(const T* __restrict__ row, int nk, int lane, float (&v)[MAXJ]) {
  if constexpr (VEC) {
#pragma unroll
    for (int g = 0; g < MAXJ / 4; ++g) {
      if (g * 4 < nk) {
        if constexpr (sizeof(T) == 4) {
          const float4 x = *(const float4*)((const float*)row + g * 256 + lane * 4);
          v[4 * g] = x.x; v[4 * g + 1] = x.y; v[4 * g + 2] = x.z; v[4 * g + 3] = x.w;
        } else {
          const bf16x4 x = *(const bf16x4*)((const bf16_t*)row + g * 256 + lane * 4);
          v[4 * g] = (float)x[0]; v[4 * g + 1] = (float)x[1]; v[4 * g + 2] = (float)x[2]; v[4 * g + 3] = (float)x[3];
        }
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < MAXJ; ++e)
      if (e < nk) v[e] = ldf(row + e * 64 + lane);
  }
}

template <typename T, int MAXJ, bool VEC>
__global__ __launch_bounds__(ST_WAVES * 64) void stop_token_kernel(ns_stop_token_params p, int nk, int train, float coef) {
  __shared__ float dw_lds[2048];
  __shared__ float sc_lds[2 * ST_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long rows = (long)p.N * p.S;
  const long G = gridDim.x;
  float* __restrict__ zrow = p.work + G * p.D + 2 * G;
  float wv[MAXJ], hv[MAXJ], acc[MAXJ];
  st_load<float, MAXJ, VEC>(p.w, nk, lane, wv);
#pragma unroll
  for (int e = 0; e < MAXJ; ++e) acc[e] = 0.f;
  const float bias = p.b[0];
  float lsum = 0.f, dbsum = 0.f;
  const long row0 = (long)blockIdx.x * ST_ROWS + wave * ST_RPW;
  for (int i = 0; i < ST_RPW; ++i) {
    const long row = row0 + i;
    if (row >= rows) break;
    const int n = (int)(row / p.S), s = (int)(row % p.S);
    st_load<T, MAXJ, VEC>((const T*)p.h + n * p.h_sn + s * p.h_ss, nk, lane, hv);
    float dot = 0.f;
#pragma unroll
    for (int e = 0; e < MAXJ; ++e)
      if (e < nk) dot = fmaf(hv[e], wv[e], dot);
    const float z = wave_sum(dot) + bias;
    if (lane == 0) {
      zrow[row] = z;
      if (p.logits) p.logits[row] = z;
    }
    if (!train) continue;
    const int Sn = p.out_steps ? min(max(p.out_steps[n], 1), p.S) : p.S;
    const bool y = s >= Sn - 1;
    // sp(x) = max(x, 0) + log1p(exp(-|x|)); sigma(x) from the same exponential, without overflow on either side
    const float ez = expf(-fabsf(z));
    const float lp = log1pf(ez);
    const float sig_abs = 1.f / (1.f + ez);                 // sigma(|z|)
    const float sig_neg = ez / (1.f + ez);                  // sigma(-|z|)
    float dz;
    if (y) {                                                // pos_weight * sp(-z);  -pos_weight * sigma(-z)
      lsum += p.pos_weight * (fmaxf(-z, 0.f) + lp);
      dz = -coef * p.pos_weight * (z >= 0.f ? sig_neg : sig_abs);
    } else {                                                // sp(z);  sigma(z)
      lsum += fmaxf(z, 0.f) + lp;
      dz = coef * (z >= 0.f ? sig_abs : sig_neg);
    }
    dbsum += dz;
    if (p.dh && dz != 0.f) {        // a zero dz (grad_scale 0) leaves the row's bits alone, the sign of a -0 included
      float* __restrict__ d = p.dh + n * p.dh_sn + s * p.dh_ss;
      if constexpr (VEC) {
#pragma unroll
        for (int g = 0; g < MAXJ / 4; ++g) {
          if (g * 4 < nk) {
            float4* q = (float4*)(d + g * 256 + lane * 4);
            float4 x = *q;
            x.x = fmaf(dz, wv[4 * g], x.x); x.y = fmaf(dz, wv[4 * g + 1], x.y);
            x.z = fmaf(dz, wv[4 * g + 2], x.z); x.w = fmaf(dz, wv[4 * g + 3], x.w);
            *q = x;
          }
        }
      } else {
#pragma unroll
        for (int e = 0; e < MAXJ; ++e)
          if (e < nk) d[e * 64 + lane] = fmaf(dz, wv[e], d[e * 64 + lane]);
      }
#pragma unroll
      for (int e = 0; e < MAXJ; ++e)
        if (e < nk) acc[e] = fmaf(dz, hv[e], acc[e]);
    }
  }
  if (!train) return;
  // the workgroup's partials: the waves add their dw shares in wave order, thread 0 the scalars in wave order
  if (lane == 0) { sc_lds[wave] = lsum; sc_lds[ST_WAVES + wave] = dbsum; }
  if (p.dw) {
    for (int w = 0; w < ST_WAVES; ++w) {
      if (wave == w) {
#pragma unroll
        for (int e = 0; e < MAXJ; ++e)
          if (e < nk) {
            const int c = st_col<VEC>(e, lane);
            dw_lds[c] = w == 0 ? acc[e] : dw_lds[c] + acc[e];
          }
      }
      __syncthreads();
    }
    float* __restrict__ part = p.work + (long)blockIdx.x * p.D;
    for (int c = threadIdx.x; c < p.D; c += blockDim.x) part[c] = dw_lds[c];
  } else {
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float l = 0.f, b = 0.f;
    for (int w = 0; w < ST_WAVES; ++w) { l += sc_lds[w]; b += sc_lds[ST_WAVES + w]; }
    p.work[G * p.D + blockIdx.x] = l;
    p.work[G * p.D + G + blockIdx.x] = b;
  }
}

// blocks 0 .. D / 64 - 1: dw[d] += the partials of column d in index order; the last block: the stop steps of every
// utterance, then thread 0 adds the loss, db and the step errors in index order.
__global__ __launch_bounds__(64) void stop_token_finish_kernel(ns_stop_token_params p, int G, int train) {
  const int lane = threadIdx.x;
  const int nd = p.D / 64;
  if ((int)blockIdx.x < nd) {
    if (!p.dw) return;
    const int d = blockIdx.x * 64 + lane;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += (double)p.work[(long)g * p.D + d];
    p.dw[d] += (float)s;
    return;
  }
  const long rows = (long)p.N * p.S;
  const float* __restrict__ lpart = p.work + (long)G * p.D;
  const float* __restrict__ bpart = lpart + G;
  const float* __restrict__ zrow = bpart + G;
  float* __restrict__ err = p.work + (long)G * p.D + 2 * G + rows;
  for (int n = lane; n < p.N; n += 64) {
    const float* z = zrow + (long)n * p.S;
    if (p.stop_steps) {
      int s = 0;
      while (s < p.S - 1 && !(z[s] > p.threshold_logit)) ++s;
      p.stop_steps[n] = s + 1;
    }
    if (train) {
      int s = 0;
      while (s < p.S - 1 && !(z[s] > 0.f)) ++s;         // probability over 0.5
      const int Sn = p.out_steps ? min(max(p.out_steps[n], 1), p.S) : p.S;
      err[n] = fabsf((float)(s + 1 - Sn));
    }
  }
  if (!train) return;
  __syncthreads();
  if (lane != 0) return;
  double l = 0.0, b = 0.0, e = 0.0;
  for (int g = 0; g < G; ++g) { l += (double)lpart[g]; b += (double)bpart[g]; }
  for (int n = 0; n < p.N; ++n) e += (double)err[n];
  if (p.acc) {
    p.acc[0] = (float)(l / (double)rows);
    p.acc[1] = (float)(e / (double)p.N);
  }
  if (p.db) p.db[0] += (float)b;
}

template <typename T, bool VEC>
static void st_launch(const ns_stop_token_params& p, int nk, int train, float coef, int G, hipStream_t s) {
  const dim3 grid(G), block(ST_WAVES * 64);
  if (nk <= 4) hipLaunchKernelGGL((stop_token_kernel<T, 4, VEC>), grid, block, 0, s, p, nk, train, coef);
  else if (nk <= 16) hipLaunchKernelGGL((stop_token_kernel<T, 16, VEC>), grid, block, 0, s, p, nk, train, coef);
  else hipLaunchKernelGGL((stop_token_kernel<T, 32, VEC>), grid, block, 0, s, p, nk, train, coef);
}

extern "C" int ns_stop_token(const ns_stop_token_params* p, ns_stream_t s) {
  NS_CHECK_ARG(p, "ns_stop_token: null parameter block");
  NS_CHECK_ARG(p->h, "ns_stop_token: h is null");
  NS_CHECK_ARG(p->w, "ns_stop_token: w is null");
  NS_CHECK_ARG(p->b, "ns_stop_token: b is null");
  NS_CHECK_ARG(p->N >= 1, "ns_stop_token: N must be at least 1 (got %d)", p->N);
  NS_CHECK_ARG(p->S >= 1, "ns_stop_token: S must be at least 1 (got %d)", p->S);
  NS_CHECK_ARG(p->D >= 64 && p->D <= 2048 && p->D % 64 == 0,
               "ns_stop_token: D must be a multiple of 64 in [64, 2048] (got %d)", p->D);
  NS_CHECK_ARG(p->h_dtype == NS_F32 || p->h_dtype == NS_BF16, "ns_stop_token: h_dtype must be fp32 or bf16 (got %d)",
               p->h_dtype);
  NS_CHECK_ARG(p->h_ss >= p->D && p->h_sn >= (int64_t)(p->S - 1) * p->h_ss + p->D,
               "ns_stop_token: the rows of h overlap (h_sn %lld, h_ss %lld)", (long long)p->h_sn, (long long)p->h_ss);
  NS_CHECK_ARG(!p->dh || (p->dw && p->db), "ns_stop_token: dh needs dw and db");
  NS_CHECK_ARG(p->dh || (!p->dw && !p->db), "ns_stop_token: dw and db need dh");
  NS_CHECK_ARG(!p->dh || (p->dh_ss >= p->D && p->dh_sn >= (int64_t)(p->S - 1) * p->dh_ss + p->D),
               "ns_stop_token: the rows of dh overlap (dh_sn %lld, dh_ss %lld)", (long long)p->dh_sn,
               (long long)p->dh_ss);
  const int train = (p->out_steps || p->dh || p->acc) ? 1 : 0;
  if (train) {
    NS_CHECK_ARG(p->pos_weight > 0.f, "ns_stop_token: pos_weight must be positive (got %g)", (double)p->pos_weight);
    NS_CHECK_ARG(p->grad_scale >= 0.f, "ns_stop_token: grad_scale must not be negative (got %g)", (double)p->grad_scale);
  }
  NS_CHECK_ARG(!p->stop_steps || p->threshold_logit == p->threshold_logit, "ns_stop_token: threshold_logit is NaN");
  NS_CHECK_ARG(p->work, "ns_stop_token: work is null (ns_stop_token_work_floats(N, S, D) floats)");
  const long rows = (long)p->N * p->S;
  NS_CHECK_ARG(st_groups(rows) <= 0x7fffffffL / p->D, "ns_stop_token: N * S too large (%ld rows)", rows);
  const int G = (int)st_groups(rows);
  const int nk = p->D / 64;
  const float coef = (float)((double)p->grad_scale / (double)rows);
  // 16-byte loads and stores where every row starts on such a boundary
  const int hb = p->h_dtype == NS_F32 ? 4 : 2;
  bool vec = nk % 4 == 0 && ((uintptr_t)p->h % (4 * hb)) == 0 && p->h_sn % 4 == 0 && p->h_ss % 4 == 0 &&
             ((uintptr_t)p->w % 16) == 0;
  if (p->dh) vec = vec && ((uintptr_t)p->dh % 16) == 0 && p->dh_sn % 4 == 0 && p->dh_ss % 4 == 0;
  hipStream_t st = (hipStream_t)s;
  if (p->h_dtype == NS_F32) {
    if (vec) st_launch<float, true>(*p, nk, train, coef, G, st); else st_launch<float, false>(*p, nk, train, coef, G, st);
  } else {
    if (vec) st_launch<bf16_t, true>(*p, nk, train, coef, G, st); else st_launch<bf16_t, false>(*p, nk, train, coef, G, st);
  }
  NS_CHECK_LAUNCH("stop_token");
  if (train || p->stop_steps) {
    hipLaunchKernelGGL(stop_token_finish_kernel, dim3(nk + 1), dim3(64), 0, st, *p, G, train);
    NS_CHECK_LAUNCH("stop_token_finish");
  }
  return NS_OK;
}
