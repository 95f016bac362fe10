// The vector column sum (ns_colsum's colsum4_kernel) as a device function: elementwise.hip launches it alone, gemm.hip
// runs it as an item of a grouped weight-gradient launch (gemm_group_kernel).  Both give the same bits: the partition
// into row blocks and the order of every sum depend on (bx, by, gx) only, which a caller takes from blockIdx / gridDim
// or from its own item table.
#pragma once
#include "common.h"

constexpr int CS4_QUADS = 16;             // channel quads per block (64 channels)
constexpr int CS4_LANES = 16;             // row lanes per block: 16 x 16 = 256 threads
constexpr int COLSUM_MAX_BLOCKS = 64;     // row blocks of a launch = partial sums per column
constexpr int COLSUM_CNT = 1024;          // ns_colsum_params.work: [0, 1024) arrival counters (as int), then the partial sums

__device__ __forceinline__ float4 cs4_ld(const float* p) { return *(const float4*)p; }
__device__ __forceinline__ float4 cs4_ld(const bf16_t* p) {
  const bf16x4 v = *(const bf16x4*)p;
  return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}

// whether ns_colsum takes the vector form, and its grid: gx row blocks x gy blocks of 64 columns
static inline bool colsum4_ok(const ns_colsum_params& p) {
  const int esz = p.dtype == NS_BF16 ? 2 : 4;
  // a ragged last quad reads into the row's padding (C rounded up to 4 <= ld) and adds only its valid columns
  return (p.C + 3) / 4 * 4 <= p.ld && p.ld % 4 == 0 && ((uintptr_t)p.x % (4 * esz)) == 0;
}
__host__ __device__ __forceinline__ int colsum4_grid_x(int rows) { const int b = (rows + 127) / 128; return b < 1 ? 1 : (b > 64 ? 64 : b); }
__host__ __device__ __forceinline__ int colsum4_grid_y(int C) { return ((C + 3) / 4 + CS4_QUADS - 1) / CS4_QUADS; }

// block = 16 channel quads x 16 row lanes over rows / gx rows, LDS reduction, then at most 32 adders per address
// (contended float atomics collapse, see the BatchNorm backward kernels).  red: 256 x 4 floats of LDS, last: one int.
template <typename T>
__device__ __forceinline__ void colsum4_body(const ns_colsum_params& p, int bx, int by, int gx, float (*red)[4], int* last) {
  const T* x = (const T*)p.x;
  const int tid = threadIdx.x, ql = tid % CS4_QUADS, rl = tid / CS4_QUADS;
  const int q = by * CS4_QUADS + ql;
  const bool active = 4 * q < p.C;
  const int rpb = (p.rows + gx - 1) / gx;
  const int r0 = bx * rpb, r1 = min(p.rows, r0 + rpb);
  float s4[4] = {0.f, 0.f, 0.f, 0.f};
  constexpr int CU = 8;          // rows in flight per thread (a bf16 row quad is only 8 bytes)
  if (active) {
    for (int base = r0 + rl; base < r1; base += CU * CS4_LANES) {
      float4 v[CU];
#pragma unroll
      for (int u = 0; u < CU; ++u) {
        const int row = base + u * CS4_LANES;
        v[u] = row < r1 ? cs4_ld(x + (long)row * p.ld + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < CU; ++u) { s4[0] += v[u].x; s4[1] += v[u].y; s4[2] += v[u].z; s4[3] += v[u].w; }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[tid][i] = s4[i];
  __syncthreads();
  if (rl == 0 && active) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float a = 0.f;
      for (int r = 0; r < CS4_LANES; ++r) a += red[r * CS4_QUADS + ql][i];
      if (4 * q + i < p.C) {
        if (p.work) ns_st_sc1(p.work + COLSUM_CNT + (long)bx * p.C + 4 * q + i, a);      // parked: the last row block adds them in order
        else atomicAdd(p.out + 4 * q + i, a);
      }
    }
  }
  if (!p.work) return;
  // fixed-order finish: write-through partials, drained -> this column block's counter; the last one adds partials 0, 1, ...
  ns_drain_stores();
  __syncthreads();
  int* counter = (int*)p.work + by;
  if (tid == 0) *last = atomicAdd(counter, 1) == gx - 1;
  __syncthreads();
  if (!*last) return;
  // 64 columns x 4 groups of 16 row blocks: every thread has its 16 loads in flight at once and adds them in block order,
  // the four group sums are added in group order (the serial 64-load chain of one thread per column cost 20 us a call)
  const int c0 = by * CS4_QUADS * 4;
  constexpr int GB = COLSUM_MAX_BLOCKS / 4;
  const int cc = tid & 63, grp = tid >> 6;
  float pv[GB];
#pragma unroll
  for (int i = 0; i < GB; ++i) {
    const int b = grp * GB + i;
    pv[i] = (b < gx && c0 + cc < p.C) ? ns_ld_sc1(p.work + COLSUM_CNT + (long)b * p.C + c0 + cc) : 0.f;
  }
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < GB; ++i) a += pv[i];
  red[tid][0] = a;
  __syncthreads();
  if (tid < 64 && c0 + tid < p.C) p.out[c0 + tid] += ((red[tid][0] + red[64 + tid][0]) + red[128 + tid][0]) + red[192 + tid][0];
  if (tid == 0) *counter = 0;
}
