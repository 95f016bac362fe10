// Persistent BiLSTM recurrence: ONE launch for the whole sequence instead of one per time step.
//
// A "chain" = (direction, group of batch rows) is an independent recurrence: 16 rows (the MFMA tile's other
// dimension) in the single-role kernels, 16, 8 or 4 in the role-split kernels (template parameter RPC,
// picked per launch by cluster_rows(); the rows of the tile beyond RPC are never loaded, published or stored: the narrow
// forms fill them with replicas of the live rows - the operand fragment of a padding column is read from a live row - and
// deal the element-wise work of a slot over all 64 lanes, each lane owning RPC / 16 of what its column computes; see the
// ownership rules above the two kernels, profiles/cluster_lanes.txt).  Batch rows are independent and an MFMA output column
// depends on its own operand column only, so every form writes the same bits; a narrow chain moves RPC / 16 of the bytes
// per hop - the hop is what bounds a step - and the batch takes 16 / RPC times the workgroups: at batch 32, H 256 the
// expand BiLSTM runs on 64 CUs instead of 16, forward 2.16 -> 1.59 ms, backward 2.16 -> 1.90 ms
// (profiles/cluster_rows.txt).  It runs on a
// cluster of CS = H/64 workgroups (one per CU); workgroup c owns hidden units [64c, 64c+64) and
// keeps its slice of W_h^T - 64 units x 4 gates x H - in REGISTERS as MFMA B fragments for the
// whole sequence (8 waves x 8 units, 64 VGPRs per lane), and the cell state in registers too.
// Per step the only inter-workgroup traffic is the new h slice (rows of the chain x 64 units), exchanged
// through global memory as {step tag, 2 x bf16} granules (exchange.h; the protocol - granule, poll
// cadence, bound, status word - is DESIGN.md, "The tagged-granule exchange"), double-buffered by step parity.
// Measured exchange cost: ~1.3 us per step for 4 workgroups (vs ~6-8 us per dependent launch).
//
// Correctness of the 2-deep buffering: a workgroup publishes step s+2 into the slot of step s only
// after it has gathered every peer's step s+1, which each peer published only after gathering step s.
// On a time-out (status 1 forward, 2 backward) every workgroup leaves; the single-role kernels read the status word
// at the poll cadence too, so one expired wait ends the launch instead of costing every later step its own bound.
#include "exchange.h"
#include "carve.h"
#include <stdlib.h>
#include <stdint.h>

constexpr int CW = 8;            // waves per workgroup
constexpr int CTHREADS = CW * 64;

struct LstmClusterArgs {
  int N, T, H, P, padl, CS;
  // per direction d (0 = forward in time, 1 = reversed)
  const float* xg[2]; long ld_xg;
  const bf16_t* whT[2];           // [4H, H]
  const bf16_t* wh[2];            // [H, 4H] (backward)
  bf16_t* h[2]; long ld_h;        // h[d] already offset to this direction's columns
  float* c[2];
  bf16_t* gates[2];
  // fp32-state forward (lstm_cluster3_fwd_kernel): pre-split recurrent weights, fp32 h out, optional bf16 copy of h
  const bf16_t* whT_hi[2]; const bf16_t* whT_lo[2];
  float* hf[2]; bf16_t* hb[2]; long ld_hb;
  const float* dh[2]; long ld_dh; // backward: grad wrt h outputs (offset to direction's columns)
  bf16_t* dgates[2];
  const int* lengths;
  float forget_bias, cell_clip;
  u64* xbuf;                      // [chains][2][16][granules per row]
  int* status;
  int dbg;                        // NS_CLUSTER_DBG, 0 in production; bit 16: the role-split kernels stamp into `trace`
  int xcd;                        // the members of a chain share an XCD (ns_cluster_place; NS_CLUSTER_XCD, family "bilstm" / "bilstmf32")
  long long* trace;               // dbg bit 16: [step][8] timestamps of workgroup 0 (100 MHz clock)
};

__device__ __forceinline__ int swz_off(int row, int k, int H) {   // bf16 element offset in the LDS h image
  const int chunk = k >> 3;
  const int m = ((H >> 3) & 15) ? 7 : 15;   // the XOR must stay inside an aligned group of chunks of the row
  return row * H + (((chunk ^ (row & m)) << 3) | (k & 7));
}

// ------------------------------------------------------------------ forward
__global__ __launch_bounds__(CTHREADS) void lstm_cluster_fwd_kernel(LstmClusterArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* hs = (bf16_t*)smem;                       // [16][H] swizzled
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int CS = a.CS, H = a.H;
  const int nrg = (a.N + 15) / 16;
  const ns_cluster_slot slot = ns_cluster_place(blockIdx.x, 2 * nrg, CS, a.xcd != 0);
  if (!slot.active) return;                                       // padding of a placed grid (exchange.h)
  const int chain = slot.cluster, wgc = slot.member;
  const int d = chain / nrg, rg = chain % nrg;
  const int n0 = rg * 16;
  const int r16 = lane & 15, g = lane >> 4;
  const int GPR = H / 2;                            // granules per row
  u64* xb = a.xbuf + (size_t)chain * 2 * 16 * GPR;
  const int uw0 = wgc * 64 + wave * 8;              // this wave's 8 units
  const int ksteps = H / 32;

  // ---- resident weight fragments: tile 0 = [i | j], tile 1 = [f | o] for 8 units
  bf16x8 bw[2][16];
  {
    const bf16_t* W = a.whT[d];
    const int unit = uw0 + (r16 & 7);
#pragma unroll
    for (int tl = 0; tl < 2; ++tl) {
      const int gate = tl * 2 + (r16 >> 3);
      const bf16_t* row = W + ((long)gate * H + unit) * H;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks)
        bw[tl][ks] = ks < ksteps ? *(const bf16x8*)(row + ks * 32 + g * 8) : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  float cst[4] = {0.f, 0.f, 0.f, 0.f};
  const bool cell_lane = r16 < 8;
  const int unit = uw0 + (r16 & 7);
  int len[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = n0 + g * 4 + r;
    len[r] = (a.lengths && n < a.N) ? a.lengths[n] : a.T;
  }
  const float* xg = a.xg[d];
  // xg prefetch for step 0
  float xa[4], xb2[4], xa_n[4], xb_n[4];
  auto load_xg = [&](int t, float* pa, float* pb) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + g * 4 + r;
      const long rowi = (long)n * a.P + a.padl + t;
      const bool ok = n < a.N;
      const float* xr = xg + rowi * a.ld_xg + (long)(r16 >> 3) * H + unit;   // gate i or j; f or o is two gates on
      pa[r] = ok ? xr[0] : 0.f;
      pb[r] = ok ? xr[2L * H] : 0.f;
    }
  };
  load_xg(d ? a.T - 1 : 0, xa, xb2);

  for (int step = 0; step < a.T; ++step) {
    const int t = d ? a.T - 1 - step : step;
    if (step + 1 < a.T) load_xg(d ? t - 1 : t + 1, xa_n, xb_n);
    f32x4 accA = {xa[0], xa[1], xa[2], xa[3]};
    f32x4 accB = {xb2[0], xb2[1], xb2[2], xb2[3]};
    if (step > 0) {
      // ---- gather h of the previous step from the whole cluster into LDS
      const u64* cur = xb + (size_t)(step & 1) * 16 * GPR;   // written at the end of step-1 with tag = step
      const int total = 16 * GPR;
      for (int i0 = tid; i0 < total; i0 += CTHREADS * 4) {
        u64 v[4];
        ns_spin sp;
        ns_poll_granules(v, (unsigned)step, sp, a.status, 1, [&](int j) {      // gave up: the status word is raised, read below
          const int i = i0 + j * CTHREADS;
          return i < total ? ns_ld_granule(cur + i) : ns_granule((unsigned)step, 0u);
        });
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = i0 + j * CTHREADS;
          if (i < total) {
            const int row = i / GPR, pr = i % GPR;
            *(unsigned*)(hs + swz_off(row, pr * 2, H)) = (unsigned)v[j];
          }
        }
      }
      __syncthreads();
      if (*(volatile int*)a.status) return;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        if (ks < ksteps) {
          const bf16x8 af = *(const bf16x8*)(hs + swz_off(r16, ks * 32 + g * 8, H));
          accA = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bw[0][ks], accA, 0, 0, 0);
          accB = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bw[1][ks], accB, 0, 0, 0);
        }
      }
      __syncthreads();   // hs is rewritten by the next gather
    }
    // ---- cell update: lanes r16 < 8 hold (i, f); their partners r16+8 hold (j, o)
    float hv[4], sgi[4], sgj[4], sgf[4], sgo[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float zj = __shfl_down(accA[r], 8, 64);
      const float zo = __shfl_down(accB[r], 8, 64);
      const bool masked = t >= len[r];
      const float gi = sigmoidf_(accA[r]), gj = tanhf_(zj), gf = sigmoidf_(accB[r] + a.forget_bias), go = sigmoidf_(zo);
      float cn = ns_cell_clip(gf * cst[r] + gi * gj, a.cell_clip);
      float hn = go * tanhf_(cn);
      if (masked) { cn = 0.f; hn = 0.f; }
      cst[r] = cn;
      hv[r] = hn;
      sgi[r] = masked ? 0.f : gi; sgj[r] = masked ? 0.f : gj; sgf[r] = masked ? 0.f : gf; sgo[r] = masked ? 0.f : go;
    }
    // ---- publish h first (tag = step + 1): the peers are waiting on it; even unit lanes pack (h[u], h[u+1])
    if (step + 1 < a.T) {
      u64* nxt = xb + (size_t)((step + 1) & 1) * 16 * GPR;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float hp = __shfl_down(hv[r], 1, 64);
        if (cell_lane && !(r16 & 1)) {
          const bf16_t b0 = (bf16_t)hv[r], b1 = (bf16_t)hp;
          const unsigned pay = (unsigned)(*(const unsigned short*)&b0) | ((unsigned)(*(const unsigned short*)&b1) << 16);
          const int row = g * 4 + r;
          ns_put_granule(nxt + (size_t)row * GPR + (unit >> 1), ns_granule((unsigned)(step + 1), pay));
        }
      }
    }
    // ---- then the saves for the backward pass / the consumers of h
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + g * 4 + r;
      if (cell_lane && n < a.N) {
        const long rowi = (long)n * a.P + a.padl + t;
        a.h[d][rowi * a.ld_h + unit] = (bf16_t)hv[r];
        a.c[d][rowi * H + unit] = cst[r];
        bf16_t* gp = a.gates[d] + rowi * 4 * H;
        gp[unit] = (bf16_t)sgi[r];
        gp[H + unit] = (bf16_t)sgj[r];
        gp[2 * H + unit] = (bf16_t)sgf[r];
        gp[3 * H + unit] = (bf16_t)sgo[r];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) { xa[r] = xa_n[r]; xb2[r] = xb_n[r]; }
  }
}

// ------------------------------------------------------------------ backward
// dh[t] = dh_out[t] + dgates[next].Wh^T ; this workgroup owns 64 units (rows of Wh [H,4H]); the
// contraction runs over all 4H gate gradients of the next step, gathered from the cluster.
// Wave w holds the K-slice [w*4H/8, (w+1)*4H/8) of the 4 unit tiles in registers.
struct ClusterBwdLds {                                         // dynamic LDS of lstm_cluster_bwd_kernel
  int H;
  LdsCarve c = {};
  int dgs = c.take<bf16_t>(16 * 4 * H);                        // [16][4H] swizzled gathered gate grads
  int red = c.take<float>(CW * 16 * 65);                       // [CW][16][65]
  int bytes = c.off;
};
__global__ __launch_bounds__(CTHREADS) void lstm_cluster_bwd_kernel(LstmClusterArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int CS = a.CS, H = a.H, K = 4 * a.H;
  const ClusterBwdLds lay{H};
  bf16_t* dgs = carve_at<bf16_t>(smem, lay.dgs); float* red = carve_at<float>(smem, lay.red);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nrg = (a.N + 15) / 16;
  const ns_cluster_slot slot = ns_cluster_place(blockIdx.x, 2 * nrg, CS, a.xcd != 0);
  if (!slot.active) return;                                       // padding of a placed grid (exchange.h)
  const int chain = slot.cluster, wgc = slot.member;
  const int d = chain / nrg, rg = chain % nrg;
  const int n0 = rg * 16;
  const int r16 = lane & 15, g = lane >> 4;
  const int GPR = K / 2;
  u64* xb = a.xbuf + (size_t)chain * 2 * 16 * GPR;
  const int u0 = wgc * 64;
  const int kpw = K / CW;                  // K-slice per wave (multiple of 32)
  const int ksteps = kpw / 32;             // <= 8 for H <= 512
  bf16x8 bw[4][8];
  {
    const bf16_t* W = a.wh[d];
#pragma unroll
    for (int tl = 0; tl < 4; ++tl) {
      const bf16_t* row = W + (long)(u0 + tl * 16 + r16) * K + wave * kpw;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks)
        bw[tl][ks] = ks < ksteps ? *(const bf16x8*)(row + ks * 32 + g * 8) : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  // cell ownership for the epilogue: thread -> (row = tid >> 5 (16 rows), 2 units)
  const int er = tid >> 5, eu = (tid & 31) * 2;
  const int en = n0 + er;
  const int elen = (a.lengths && en < a.N) ? a.lengths[en] : a.T;
  float dcc[2] = {0.f, 0.f};

  for (int step = a.T - 1; step >= 0; --step) {      // walk the forward order backwards
    const int t = d ? a.T - 1 - step : step;
    const int tp = d ? t + 1 : t - 1;                 // forward-pass predecessor
    const bool has_prev = step > 0;
    const bool has_next = step < a.T - 1;
    const int bs = a.T - 1 - step;                    // backward step index, 0-based
    // prefetch epilogue operands
    float pdh[2] = {0.f, 0.f}, pg[2][4], pc[2] = {0.f, 0.f}, pcp[2] = {0.f, 0.f};
    const long rowi = (long)en * a.P + a.padl + t;
    const bool ok = en < a.N;
    const bool masked = t >= elen;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int u = u0 + eu + q;
#pragma unroll
      for (int j = 0; j < 4; ++j) pg[q][j] = ok ? (float)a.gates[d][rowi * 4 * H + (long)j * H + u] : 0.f;
      if (ok) {
        pdh[q] = a.dh[d][rowi * a.ld_dh + u];
        pc[q] = a.c[d][rowi * H + u];
        if (has_prev) pcp[q] = a.c[d][((long)en * a.P + a.padl + tp) * H + u];
      }
    }
    float dhp[2] = {0.f, 0.f};
    if (has_next) {
      // ---- gather dgates of the step after (tag = bs) from the whole cluster
      const u64* cur = xb + (size_t)(bs & 1) * 16 * GPR;
      const int total = 16 * GPR;
      for (int i0 = tid; i0 < total; i0 += CTHREADS * 8) {
        u64 v[8];
        ns_spin sp;
        ns_poll_granules(v, (unsigned)bs, sp, a.status, 2, [&](int j) {        // gave up: the status word is raised, read below
          const int i = i0 + j * CTHREADS;
          return i < total ? ns_ld_granule(cur + i) : ns_granule((unsigned)bs, 0u);
        });
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int i = i0 + j * CTHREADS;
          if (i < total) {
            const int row = i / GPR, pr = i % GPR;
            *(unsigned*)(dgs + swz_off(row, pr * 2, K)) = (unsigned)v[j];
          }
        }
      }
      __syncthreads();
      if (*(volatile int*)a.status) return;
      f32x4 acc[4];
#pragma unroll
      for (int tl = 0; tl < 4; ++tl) acc[tl] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        if (ks < ksteps) {
          const bf16x8 af = *(const bf16x8*)(dgs + swz_off(r16, wave * kpw + ks * 32 + g * 8, K));
#pragma unroll
          for (int tl = 0; tl < 4; ++tl) acc[tl] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bw[tl][ks], acc[tl], 0, 0, 0);
        }
      }
#pragma unroll
      for (int tl = 0; tl < 4; ++tl)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(wave * 16 + g * 4 + r) * 65 + tl * 16 + r16] = acc[tl][r];
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < CW; ++w) s += red[(w * 16 + er) * 65 + eu + q];
        dhp[q] = s;
      }
    }
    // ---- cell gradient for (row er, units eu, eu+1)
    float dgv[2][4];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const float gi = pg[q][0], gj = pg[q][1], gf = pg[q][2], go = pg[q][3];
      const float dh = pdh[q] + dhp[q];
      const float tc = tanhf_(pc[q]);
      const float d_o = dh * tc * go * (1.f - go);
      const float dc = dh * go * (1.f - tc * tc) + dcc[q];
      dgv[q][0] = dc * gj * gi * (1.f - gi);
      dgv[q][1] = dc * gi * (1.f - gj * gj);
      dgv[q][2] = dc * pcp[q] * gf * (1.f - gf);
      dgv[q][3] = d_o;
      dcc[q] = dc * gf;
      if (masked || !ok) {
        dgv[q][0] = dgv[q][1] = dgv[q][2] = dgv[q][3] = 0.f;
        dcc[q] = 0.f;
      }
    }
    if (step > 0) {   // publish this step's gate gradients first (tag = bs + 1)
      u64* nxt = xb + (size_t)((bs + 1) & 1) * 16 * GPR;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16_t b0 = (bf16_t)dgv[0][j], b1 = (bf16_t)dgv[1][j];
        const unsigned pay = (unsigned)(*(const unsigned short*)&b0) | ((unsigned)(*(const unsigned short*)&b1) << 16);
        ns_put_granule(nxt + (size_t)er * GPR + ((j * H + u0 + eu) >> 1), ns_granule((unsigned)(bs + 1), pay));
      }
    }
    if (ok) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16_t b0 = (bf16_t)dgv[0][j], b1 = (bf16_t)dgv[1][j];
        const unsigned pay = (unsigned)(*(const unsigned short*)&b0) | ((unsigned)(*(const unsigned short*)&b1) << 16);
        *(unsigned*)(a.dgates[d] + rowi * 4 * H + (long)j * H + u0 + eu) = pay;
      }
    }
    __syncthreads();   // red / dgs reuse
  }
}

// ==================================================================== role-split kernels (H <= 256)
// Same clustering and exchange protocol as above; what takes the exchange latency (~2 us publish -> gathered, most of
// a step) off the critical path is the split into ROLES.  No wave mixes global loads and global stores (gfx9 has one
// vmcnt for both, so a polling load issued behind a store waits for the store's acknowledgement):
//   - XW compute waves (16 units each): MFMA from LDS, cell update, publish + saves.  Stores only.
//   - poller wave(s): spin on the exchange granules and drop them into the LDS operand image
//     (double-buffered).  Loads only.
//   - one prefetcher wave: streams the per-step operands (xg rows / saved gates, dh, c) one slot
//     ahead into an LDS stage.  Loads only.
//   - one saver wave: writes the slot's results out of LDS, one slot behind.  Stores only.
// One workgroup barrier per slot hands the LDS images over.  A set of workgroups serves ONE chain, so slot s is the
// chain's step s (forward) or backward step s.
//
// Exchange layout (per chain and parity): a publishing lane's granules are contiguous, so one base
// register + immediates address them; the poller decodes granule index -> (row, k) when it fills LDS.
//
// LDS hand-over audit (the class of the attention-backward race fixed in 844cc13 - an image filled by one role and
// first read by another with no barrier in between).  Every image below is double-buffered by slot parity and handed
// over by the ONE ns_lds_barrier() per slot that every role joins (ns_lds_barrier waits for lgkmcnt(0) first, so a role's LDS
// writes AND reads of the slot have completed when it arrives):
//   forward   hs[s&1]   pollers fill it in front of barrier s, compute waves read it behind barrier s; the pollers'
//                       next fill of the same image is for slot s+2, behind barrier s+1, which the compute waves join
//                       after their reads of slot s
//             xgs[s&1]  fp32 form: slot 0 in front of barrier 0, slot s+1 behind barrier s; read behind barrier s+1.
//                       bf16 form: one interval earlier, see lstm_cluster2_fwd_kernel
//             svs[s&1]  compute waves write it in slot s, the saver reads it behind barrier s+1 and joins barrier s+2
//                       (after its reads returned) before the compute waves write that image again in slot s+2
//             abortf    zeroed by wave 0 in front of its first ns_lds_barrier, read by every role behind that barrier
//   backward  see lstm_cluster2p_bwd_kernel
// The single-role kernels above use one image and __syncthreads() on both sides of every use.
constexpr int XW = 4;
constexpr int FW_POLL = 2;               // poller waves (XW and XW + 3): half of the granules each, so a sweep is half as long
                                         // (expand BiLSTM forward 3.2 -> 3.0 ms)
constexpr int FW_WAVES = XW + 2 + FW_POLL;   // compute, poller, prefetcher, saver, second poller
constexpr int XG_LD = 256 + 4;          // floats per row of the xg stage (pad: rows 4 apart hit different banks)

__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
  const bf16_t b0 = (bf16_t)lo, b1 = (bf16_t)hi;
  return (unsigned)(*(const unsigned short*)&b0) | ((unsigned)(*(const unsigned short*)&b1) << 16);
}

// The product is taken TRANSPOSED - the resident weights are the MFMA's A operand (M = the wave's 16
// units), the gathered h its B operand (N = the 16 batch rows) - so a lane's accumulators are 4 consecutive UNITS of
// one batch row: the new h packs into the exchange's {tag, 2 x bf16} unit-pair granules in the lane (two full-wave
// stores, no cross-lane shuffle), the xg operands are one 16-byte LDS read per gate instead of 16 scalar ones, and the
// saver's images take 6 vector writes instead of 24.  The workgroup's own h block goes into the next operand image
// directly (LDS), only the peers' blocks are polled.  The xg operands of slot s + 1 are read at the end of slot s (the
// prefetcher runs one interval ahead), so behind the slot barrier the chain starts with the MFMAs.
// Ownership at 8 / 4 rows per chain (R = 16 / RPC replicas): lane (r16, g) reads the h fragment and the xg operands of row
// r16 % RPC, so after the MFMAs each of the R lanes of a row holds the same four pre-activations per gate; replica
// j = r16 / RPC keeps 4 / R of the units - the pair wq + 2 j, wq + 2 j + 1 (one granule) at 8 rows, the unit wq + j at 4 -
// and does gate math, cell state, mask, clip, publish and saves for those alone (0.61 -> 0.43 us of the slot at 4 rows).
// At 4 rows two neighbouring replicas share a granule: the even one takes the odd one's h with one DPP move and stores
// it.  Granule indices, tags, LDS addresses and the saver images' bytes are those of the 16-row form.
// (audit) one barrier per slot, joined by every role: hs[s&1] is filled by the pollers (peers' blocks) and the compute
// waves (own block, in slot s-1 behind barrier(s-1)) in front of barrier(s), read behind it, refilled behind
// barrier(s+1); xgs[(s+1)&1] is stored between barrier(s-1) and barrier(s), read between barrier(s) and barrier(s+1);
// svs as above.
struct Cluster2FwdLds {                                         // dynamic LDS of lstm_cluster2_fwd_kernel<H / 64, RPC>
  int H, RPC;
  // a slot's results for the saver wave: h bf16 [rows][64], c f32 [rows][64], gates bf16 [rows][4][64]  (2 + 4 + 8 KB at 16 rows)
  static constexpr int sv_bytes(int rows) { return rows * 64 * 2 + rows * 64 * 4 + rows * 4 * 64 * 2; }
  LdsCarve c = {};
  int hs = c.take<bf16_t>(2 * 16 * H);                          // [2][16][H] swizzled
  int xgs = c.take<float>(2 * 16 * XG_LD);                      // [2][16][XG_LD]: row, gate * 64 + unit
  int svs = c.take<char>(2 * sv_bytes(RPC));                    // [2][SV_BYTES]
  int abortf = c.take<int>(8);                                  // [3] in a 32-byte slot
  int slack = c.take<char>(2 * (sv_bytes(16) - sv_bytes(RPC))); // unused: the narrow forms ask for the 16-row size
  int bytes = c.off;
};
template <int HB, int RPC>
__global__ __launch_bounds__(FW_WAVES * 64) void lstm_cluster2_fwd_kernel(LstmClusterArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int H = HB * 64, KS = H / 32, CS = HB;
  static_assert(RPC == 16 || RPC == 8 || RPC == 4, "rows per chain");
  constexpr int GPD = XW * (4 * RPC) * 2;                       // granules per source workgroup and slot: [wave][g][row][2]
  constexpr Cluster2FwdLds lay{H, RPC};
  constexpr int SV_H = RPC * 64 * 2, SV_C = RPC * 64 * 4, SV_G = RPC * 4 * 64 * 2, SV_BYTES = SV_H + SV_C + SV_G;
  static_assert(SV_BYTES == Cluster2FwdLds::sv_bytes(RPC), "the saver image");
  bf16_t* hs = carve_at<bf16_t>(smem, lay.hs); float* xgs = carve_at<float>(smem, lay.xgs);
  char* svs = carve_at<char>(smem, lay.svs); int* abortf = carve_at<int>(smem, lay.abortf);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nch = (a.N + RPC - 1) / RPC;                        // chains per direction
  const ns_cluster_slot slot = ns_cluster_place(blockIdx.x, 2 * nch, CS, a.xcd != 0);
  if (!slot.active) return;                                       // padding of a placed grid (exchange.h)
  const int chain = slot.cluster, wgc = slot.member;
  const int d = chain / nch, rg = chain % nch;                // this workgroup set serves row group rg: batch rows rg * RPC ..
  const int r16 = lane & 15, g = lane >> 4;
  u64* xb0 = a.xbuf + (size_t)(d * nch + rg) * 2 * CS * GPD;             // + parity * CS*GPD + source * GPD
  const int u0 = wgc * 64;
  const int T = a.T;
  if (tid < 3) abortf[tid] = 0;
  // rows >= RPC of the operand images are never read (the narrow forms' B fragments come from rows < RPC only) and stay unwritten
  if (RPC < 16 && (chain | wgc) == 0 && tid == 0) a.status[1] = RPC;   // which form ran (tests, A/B tools)

  if (wave < XW) {
    // ================================================================ compute role.  16 rows: lane (r16, g) owns batch row
    // r16, units wq .. wq + 3.  8 / 4 rows: column r16 of the tile is replica `rep` of row r16 % RPC, and the lane owns
    // UPL = RPC / 4 of the four units its column computes - wq + rep * UPL .. - for everything behind the MFMAs
    constexpr int UPL = RPC / 4;                       // units per lane in the cell update: 4, 2 (one granule), 1
    const int row = r16 % RPC, rep = r16 / RPC;
    const int wq = wave * 16 + g * 4;                  // first of the 4 units of the lane's column inside the workgroup's 64
    const int wo = wq + rep * UPL;                     // first of the lane's own units
    bf16x8 bw[4][KS];                                  // A fragments: row (unit) wave * 16 + r16, k chunk g
    {
      const bf16_t* W = a.whT[d];
#pragma unroll
      for (int gate = 0; gate < 4; ++gate) {
        const bf16_t* row = W + ((long)gate * H + u0 + wave * 16 + r16) * H;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bw[gate][ks] = *(const bf16x8*)(row + ks * 32 + g * 8);
      }
    }
    float cst[UPL];
#pragma unroll
    for (int r = 0; r < UPL; ++r) cst[r] = 0.f;
    const int n = rg * RPC + row;
    const int len = (a.lengths && n < a.N) ? a.lengths[n] : T;
    f32x4 acc[4];
    auto load_xg = [&](int step) {
      const float* xr = xgs + ((size_t)(step & 1) * 16 + row) * XG_LD + wq;
#pragma unroll
      for (int gate = 0; gate < 4; ++gate) acc[gate] = *(const f32x4*)(xr + gate * 64);
    };
    // pre-activation of the lane's own unit r out of its column's four: explicit selects (a dynamically indexed
    // accumulator would go to scratch)
    auto own = [&](const f32x4& v, int r) -> float {
      if constexpr (RPC == 16) return v[r];
      else if constexpr (RPC == 8) return rep ? v[2 + r] : v[r];
      else return (rep & 2) ? ((rep & 1) ? v[3] : v[2]) : ((rep & 1) ? v[1] : v[0]);
    };
    ns_lds_barrier();                                      // xg of slot 0 and abortf are in place
    load_xg(0);
    // The slot loop of a compute role is a do-while (T >= 2 is checked on the host): with a loop guard in front the
    // compiler lays the slot out less well (backward 1.96 against 1.93 ms, forward 1.65 against 1.63 at batch 32, H 256, T 1000)
    int step = 0;
    do {
      const int t = d ? T - 1 - step : step, buf = step & 1;
      ns_lds_barrier();
      if (abortf[buf]) return;
      const bool tr = (a.dbg & 16) && (chain | wgc) == 0 && tid == 0 && step < 512;
      if (tr) a.trace[step * 8 + 0] = wall_clock64();
      if (step > 0) {
        const bf16_t* hb = hs + (size_t)buf * 16 * H;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          // narrow forms: the replicas of a row read the same address (a broadcast, no bank conflict)
          const bf16x8 hf = *(const bf16x8*)(hb + swz_off(row, ks * 32 + g * 8, H));
#pragma unroll
          for (int gate = 0; gate < 4; ++gate)
            acc[gate] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[gate][ks], hf, acc[gate], 0, 0, 0);
        }
      }
      const bool masked = t >= len;
      float hv[UPL], sg[UPL][4];
#pragma unroll
      for (int r = 0; r < UPL; ++r) {
        const float gi = sigmoidf_(own(acc[0], r)), gj = tanhf_(own(acc[1], r));
        const float gf = sigmoidf_(own(acc[2], r) + a.forget_bias), go = sigmoidf_(own(acc[3], r));
        float cn = ns_cell_clip(gf * cst[r] + gi * gj, a.cell_clip);
        float hn = go * tanhf_(cn);
        if (masked) { cn = 0.f; hn = 0.f; }
        cst[r] = cn;
        hv[r] = hn;
        sg[r][0] = masked ? 0.f : gi; sg[r][1] = masked ? 0.f : gj; sg[r][2] = masked ? 0.f : gf; sg[r][3] = masked ? 0.f : go;
      }
      if (tr) a.trace[step * 8 + 1] = wall_clock64();
      char* sv = svs + (size_t)buf * SV_BYTES;
      if constexpr (RPC == 16) {
        // publish first (tag = step + 1): units (wq, wq + 1) and (wq + 2, wq + 3) of row r16
        uint2 hp;
        hp.x = pack_bf16(hv[0], hv[1]);
        hp.y = pack_bf16(hv[2], hv[3]);
        if (step + 1 < T) {
          if (CS > 1) {
            u64* nxt = xb0 + (size_t)((step + 1) & 1) * CS * GPD + (size_t)wgc * GPD + (wave * 4 * RPC + g * RPC + r16) * 2;
            ns_put_granule(nxt, ns_granule((unsigned)(step + 1), hp.x));
            ns_put_granule(nxt + 1, ns_granule((unsigned)(step + 1), hp.y));
          }
          *(uint2*)(hs + (size_t)((step + 1) & 1) * 16 * H + swz_off(r16, u0 + wq, H)) = hp;   // the own block
        }
        if (tr) a.trace[step * 8 + 2] = wall_clock64();
        // results for the backward pass / the consumers of h go to LDS; the saver wave writes them out
        *(uint2*)((bf16_t*)sv + r16 * 64 + wq) = hp;
        *(f32x4*)((float*)(sv + SV_H) + r16 * 64 + wq) = (f32x4){cst[0], cst[1], cst[2], cst[3]};
        bf16_t* gp = (bf16_t*)(sv + SV_H + SV_C) + r16 * 4 * 64 + wq;
#pragma unroll
        for (int gate = 0; gate < 4; ++gate) {
          uint2 pk;
          pk.x = pack_bf16(sg[0][gate], sg[1][gate]);
          pk.y = pack_bf16(sg[2][gate], sg[3][gate]);
          *(uint2*)(gp + gate * 64) = pk;
        }
      } else {
        // One granule = the unit pair (wq + 2 pair, wq + 2 pair + 1) of `row`, at the index and with the tag of the 16-row
        // form.  8 rows: the lane's own two units are granule `rep`.  4 rows: the lanes of replicas 2 pair and 2 pair + 1
        // each hold one unit of it; the even one fetches its neighbour's h (lane + 4, one DPP move inside the 16-lane
        // row) and stores for both.
        unsigned hp;
        bool holder = true;
        int pair = rep;
        if constexpr (RPC == 8) {
          hp = pack_bf16(hv[0], hv[1]);
        } else {
          hp = pack_bf16(hv[0], NS_DPP_F(hv[0], 0x104));   // row_shl:4: lane i takes lane i + 4's value
          holder = !(rep & 1);
          pair = rep >> 1;
        }
        if (step + 1 < T && holder) {
          if (CS > 1) {
            u64* nxt = xb0 + (size_t)((step + 1) & 1) * CS * GPD + (size_t)wgc * GPD + (wave * 4 * RPC + g * RPC + row) * 2 + pair;
            ns_put_granule(nxt, ns_granule((unsigned)(step + 1), hp));
          }
          *(unsigned*)(hs + (size_t)((step + 1) & 1) * 16 * H + swz_off(row, u0 + wq + 2 * pair, H)) = hp;   // the own block
        }
        if (tr) a.trace[step * 8 + 2] = wall_clock64();
        // the saver's images: the bytes and offsets of the 16-row form, each written by the lane that owns the unit
        if (holder) *(unsigned*)((bf16_t*)sv + row * 64 + wq + 2 * pair) = hp;
        float* cp = (float*)(sv + SV_H) + row * 64 + wo;
        bf16_t* gp = (bf16_t*)(sv + SV_H + SV_C) + row * 4 * 64 + wo;
        if constexpr (RPC == 8) {
          *(float2*)cp = make_float2(cst[0], cst[1]);
#pragma unroll
          for (int gate = 0; gate < 4; ++gate) *(unsigned*)(gp + gate * 64) = pack_bf16(sg[0][gate], sg[1][gate]);
        } else {
          *cp = cst[0];
#pragma unroll
          for (int gate = 0; gate < 4; ++gate) gp[gate * 64] = (bf16_t)sg[0][gate];
        }
      }
      if (step + 1 < T) load_xg(step + 1);
    } while (++step < T);
    ns_lds_barrier();
  } else if (wave == XW || wave == XW + 3) {
    // ================================================================ poller role: the peers' h blocks
    constexpr int NPG = (CS - 1) * GPD;                // granules to gather per slot
    constexpr int PPG = NPG / (FW_POLL * 64) > 0 ? NPG / (FW_POLL * 64) : 1;
    static_assert(CS == 1 || NPG == PPG * FW_POLL * 64, "poller coverage");
    const int j0 = (wave == XW ? 0 : 1) * PPG;
    ns_lds_barrier();
    for (int step = 0; step < T; ++step) {
      const int buf = step & 1;
      const bool tr = (a.dbg & 16) && (chain | wgc) == 0 && lane == 0 && wave == XW && step < 512;
      if (tr) a.trace[step * 8 + 4] = wall_clock64();
      if (step > 0 && CS > 1) {
        const u64* cur = xb0 + (size_t)(step & 1) * CS * GPD;   // published by the peers with tag = step
        // (own loop, the give-up rule of exchange.h spelled out: through ns_poll_granules the kernel measured 22 us a
        // launch slower - profiles/exchange_header.txt)
        u64 v[PPG];
        unsigned spins = 0, clk0 = 0;
        bool ok;
        do {
          ok = true;
#pragma unroll
          for (int j = 0; j < PPG; ++j) {
            const int li = lane + 64 * (j0 + j), sx = li / GPD;
            const int ws = sx < wgc ? sx : sx + 1;
            v[j] = __hip_atomic_load(cur + (size_t)ws * GPD + (li % GPD), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
#pragma unroll
          for (int j = 0; j < PPG; ++j) ok = ok && ((unsigned)(v[j] >> 32) == (unsigned)step);
          if (!ok) {
            if ((++spins & 1023u) == 0) {
              if (__hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { abortf[buf] = 1; ok = true; }
              else if (ns_spin_timed_out(clk0)) { atomicExch(a.status, 1); abortf[buf] = 1; ok = true; }
            }
          }
        } while (!ok);
        if (tr) { a.trace[step * 8 + 5] = wall_clock64(); a.trace[step * 8 + 6] = spins; }
        bf16_t* dst = hs + (size_t)buf * 16 * H;
#pragma unroll
        for (int j = 0; j < PPG; ++j) {
          // granule li of source ws: wave (li / (8 RPC)) % 4, lane' = (li / 2) % (4 RPC) -> row lane' % RPC, units 4 (lane' / RPC) + 2 (li % 2)
          const int li = lane + 64 * (j0 + j), sx = li / GPD, lw = li % GPD;
          const int ws = sx < wgc ? sx : sx + 1;
          const int lp = (lw >> 1) % (4 * RPC);
          const int k = ws * 64 + (lw / (8 * RPC)) * 16 + (lp / RPC) * 4 + (lw & 1) * 2;
          *(unsigned*)(dst + swz_off(lp % RPC, k, H)) = (unsigned)v[j];
        }
      }
      ns_lds_barrier();
      if (abortf[buf]) return;
    }
    ns_lds_barrier();
  } else if (wave == XW + 2) {
    // ================================================================ saver role (stores only)
    // Runs one slot behind the compute waves (slot s-1 is complete once barrier s has passed), so its store
    // issue overlaps their next slot.  Per slot and row: h 8 chunks of 16 B, c 16, gates 32 -> 14 per lane at 16 rows.
    constexpr int NH = RPC * 8, NC = RPC * 16, NG = RPC * 32, NJ = (NH + NC + NG + 63) / 64;
    auto save = [&](int step) {
      const int t = d ? T - 1 - step : step;
      const int n0 = rg * RPC;
      const char* sv = svs + (size_t)(step & 1) * SV_BYTES;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int idx = lane + 64 * j;
        if ((NH + NC + NG) % 64 != 0 && idx >= NH + NC + NG) break;
        const f32x4 v = *(const f32x4*)(sv + idx * 16);
        if (idx < NH) {
          const int row = idx >> 3, cc = idx & 7;
          if (n0 + row < a.N)
            *(f32x4*)(a.h[d] + ((unsigned)((n0 + row) * a.P + a.padl + t) * (unsigned)a.ld_h + (unsigned)(u0 + cc * 8))) = v;
        } else if (idx < NH + NC) {
          const int jj = idx - NH, row = jj >> 4, cc = jj & 15;
          if (n0 + row < a.N)
            *(f32x4*)(a.c[d] + ((unsigned)((n0 + row) * a.P + a.padl + t) * (unsigned)H + (unsigned)(u0 + cc * 4))) = v;
        } else {
          const int jj = idx - NH - NC, row = jj >> 5, gate = (jj >> 3) & 3, cc = jj & 7;
          if (n0 + row < a.N)
            *(f32x4*)(a.gates[d] + ((unsigned)((n0 + row) * a.P + a.padl + t) * (unsigned)(4 * H) + (unsigned)(gate * H + u0 + cc * 8))) = v;
        }
      }
    };
    ns_lds_barrier();
    for (int step = 0; step < T; ++step) {
      ns_lds_barrier();
      if (abortf[step & 1]) return;
      if (step > 0) save(step - 1);
    }
    ns_lds_barrier();
    save(T - 1);
  } else {
    // ================================================================ prefetcher role, one interval ahead:
    // xg of slot s + 1 is in LDS before barrier(s).  Stage row j, gate = lane / 16, 4 floats at (lane % 16) * 4
    f32x4 pf[RPC];
    const float* xg = a.xg[d];
    const int pgate = lane >> 4, pf4 = (lane & 15) * 4;
    auto pf_load = [&](int step) {
      const int t = d ? T - 1 - step : step;
      const int n0 = rg * RPC;
#pragma unroll
      for (int j = 0; j < RPC; ++j) {
        const int n = n0 + j;
        pf[j] = n < a.N ? *(const f32x4*)(xg + ((unsigned)(n * a.P + a.padl + t) * (unsigned)a.ld_xg + (unsigned)(pgate * H + u0 + pf4)))
                        : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    };
    auto pf_store = [&](int buf) {
#pragma unroll
      for (int j = 0; j < RPC; ++j) *(f32x4*)(xgs + ((size_t)buf * 16 + j) * XG_LD + pgate * 64 + pf4) = pf[j];
    };
    pf_load(0);
    pf_store(0);
    if (T > 1) pf_load(1);
    ns_lds_barrier();
    for (int step = 0; step < T; ++step) {
      if (step + 1 < T) {
        pf_store((step + 1) & 1);
        if (step + 2 < T) pf_load(step + 2);
      }
      ns_lds_barrier();
      if (abortf[step & 1]) return;
    }
    ns_lds_barrier();
  }
}


// ==================================================================== fp32-state forward
// The encoder BiLSTM of the `mixed` / `bf16x3` modes keeps its state in fp32 and forms the recurrent product as three
// split-bf16 MFMA passes (h = hi + lo, W = hi + lo: hi.hi + hi.lo + lo.hi); one launch per time step would be
// 160 + 160 launches of 6 us.  Same roles as lstm_cluster2_fwd_kernel, with what the fp32 state changes:
//   * a granule carries ONE unit: {step tag, fp32 h}; the pollers split it into the (hi, lo) LDS images;
//   * the resident weights are twice the registers per unit (hi and lo planes), and a workgroup of 8 waves has 256 VGPRs
//     per lane: a compute wave owns 8 units (two MFMA tiles [i | j], [f | o]: 128 VGPRs of weights), a workgroup 32
//     units, a chain H / 32 workgroups; the cell update pairs lanes r16 and r16 + 8;
//   * the saver writes h as fp32 (+ an optional bf16 copy for the weight gradients) and the gates as bf16: the backward
//     pass of this arrangement is the bf16 kernel (single-pass products).
constexpr int X3W = 4, X3_POLL = 2, X3_UPW = 32;
constexpr int X3_WAVES = X3W + X3_POLL + 2;          // compute, pollers, prefetcher, saver: 8 waves, two per SIMD
constexpr int XG3_LD = 4 * X3_UPW + 4;

struct Cluster3FwdLds {                                           // dynamic LDS of lstm_cluster3_fwd_kernel<H / 64, RPC>
  int H, RPC;
  // a slot's results for the saver: h f32 [rows][32], c f32 [rows][32], gates bf16 [rows][4][32], h bf16 [rows][32]  (9216 at 16 rows)
  static constexpr int sv_bytes(int rows) { return rows * 32 * 4 + rows * 32 * 4 + rows * 4 * 32 * 2 + rows * 32 * 2; }
  LdsCarve c = {};
  int hsh = c.take<bf16_t>(2 * 16 * H);                           // [2][16][H] swizzled, high parts
  int hsl = c.take<bf16_t>(2 * 16 * H);                           // [2][16][H] low parts
  int xgs = c.take<float>(2 * 16 * XG3_LD);                       // [2][16][XG3_LD]: row, gate * 32 + unit
  int svs = c.take<char>(2 * sv_bytes(RPC));                      // [2][SV_BYTES]
  int abortf = c.take<int>(8);                                    // [2] in a 32-byte slot
  int slack = c.take<char>(2 * (sv_bytes(16) - sv_bytes(RPC)));   // unused: the narrow forms ask for the 16-row size
  int bytes = c.off;
};
template <int HB, int RPC>               // HB = H / 64, RPC = batch rows per chain
__global__ __launch_bounds__(X3_WAVES * 64) void lstm_cluster3_fwd_kernel(LstmClusterArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  static_assert(RPC == 16 || RPC == 8 || RPC == 4, "rows per chain");
  constexpr int H = HB * 64, KS = H / 32, GPC = RPC * H;         // granules per chain and step
  constexpr int CS = H / X3_UPW;                                   // workgroups per chain
  constexpr int PPG = GPC / (X3_POLL * 64);                        // granules per poller lane (H / 8)
  static_assert(GPC % (X3_POLL * 64) == 0, "poller coverage");
  constexpr Cluster3FwdLds lay{H, RPC};
  constexpr int SV_H = RPC * 32 * 4, SV_C = RPC * 32 * 4, SV_G = RPC * 4 * 32 * 2, SV_HB = RPC * 32 * 2;
  constexpr int SV_BYTES = SV_H + SV_C + SV_G + SV_HB;
  static_assert(SV_BYTES == Cluster3FwdLds::sv_bytes(RPC), "the saver image");
  bf16_t* hsh = carve_at<bf16_t>(smem, lay.hsh); bf16_t* hsl = carve_at<bf16_t>(smem, lay.hsl);
  float* xgs = carve_at<float>(smem, lay.xgs); char* svs = carve_at<char>(smem, lay.svs);
  int* abortf = carve_at<int>(smem, lay.abortf);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nch = (a.N + RPC - 1) / RPC;                          // chains per direction
  const ns_cluster_slot slot = ns_cluster_place(blockIdx.x, 2 * nch, CS, a.xcd != 0);
  if (!slot.active) return;                                       // padding of a placed grid (exchange.h)
  const int chain = slot.cluster, wgc = slot.member;
  const int d = chain / nch, rg = chain % nch;                  // this workgroup set serves row group rg: batch rows rg * RPC ..
  const int r16 = lane & 15, g = lane >> 4;
  u64* xb0 = a.xbuf + (size_t)(d * nch + rg) * 2 * GPC;                    // + parity * GPC
  const int u0 = wgc * X3_UPW;
  const int T = a.T;
  if (tid < 2) abortf[tid] = 0;          // (audit) written by wave 0 in front of its first ns_lds_barrier, read behind it
  if (RPC < 16) {
    // rows >= RPC of the operand images are MFMA padding: zeroed in front of every role's first barrier, never written
    for (int i = tid; i < 2 * 2 * 16 * H / 8; i += X3_WAVES * 64) ((uint4*)hsh)[i] = make_uint4(0u, 0u, 0u, 0u);
    if ((chain | wgc) == 0 && tid == 0) a.status[1] = RPC;   // which form ran (tests, A/B tools)
  }

  if (wave < X3W) {
    // ================================================================ compute role
    const int ul = wave * 8 + (r16 & 7);                     // unit inside the workgroup's 32
    // lane groups g >= RPC / 4 are padding rows: they publish nothing and store nothing
    const bool cell_lane = r16 < 8 && (RPC == 16 || g < RPC / 4);
    const int pub0 = (wgc * X3W + wave) * 8 * RPC + (g * 8 + (r16 & 7)) * 4;   // this lane's 4 granules (rows g*4 .. g*4+3)
    bf16x8 bwh[2][KS], bwl[2][KS];
    {
#pragma unroll
      for (int tl = 0; tl < 2; ++tl) {
        const int gate = tl * 2 + (r16 >> 3);
        const long wrow = ((long)gate * H + u0 + ul) * H + g * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          bwh[tl][ks] = *(const bf16x8*)(a.whT_hi[d] + wrow + ks * 32);
          bwl[tl][ks] = *(const bf16x8*)(a.whT_lo[d] + wrow + ks * 32);
        }
      }
    }
    float cst[4];
    int len[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = rg * RPC + g * 4 + r;
      cst[r] = 0.f;
      len[r] = (a.lengths && (RPC == 16 || g < RPC / 4) && n < a.N) ? a.lengths[n] : T;
    }
    int step = 0;
    do {                                             // see lstm_cluster2_fwd_kernel
      const int t = d ? T - 1 - step : step, buf = step & 1;
      ns_lds_barrier();
      if (abortf[buf]) return;
      // tile 0 = [i | j], tile 1 = [f | o]: column r16 -> gate 2*tile + (r16 >> 3), unit ul
      const float* xr = xgs + (size_t)buf * 16 * XG3_LD + (r16 >> 3) * X3_UPW + ul;
      f32x4 accA, accB;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        accA[r] = xr[(g * 4 + r) * XG3_LD];
        accB[r] = xr[(g * 4 + r) * XG3_LD + 2 * X3_UPW];
      }
      if (step > 0) {
        const bf16_t* hbh = hsh + (size_t)buf * 16 * H;
        const bf16_t* hbl = hsl + (size_t)buf * 16 * H;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const int so = swz_off(r16, ks * 32 + g * 8, H);
          const bf16x8 ah = *(const bf16x8*)(hbh + so), al = *(const bf16x8*)(hbl + so);
          accA = mfma_split<3>(ah, al, bwh[0][ks], bwl[0][ks], accA);
          accB = mfma_split<3>(ah, al, bwh[1][ks], bwl[1][ks], accB);
        }
      }
      float hv[4], sg[4][4], cn4[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float zj = __shfl_down(accA[r], 8, 64), zo = __shfl_down(accB[r], 8, 64);
        const bool masked = t >= len[r];
        const float gi = sigmoidf_(accA[r]), gj = tanhf_(zj), gf = sigmoidf_(accB[r] + a.forget_bias), go = sigmoidf_(zo);
        float cn = ns_cell_clip(gf * cst[r] + gi * gj, a.cell_clip);
        float hn = go * tanhf_(cn);
        if (masked) { cn = 0.f; hn = 0.f; }
        cst[r] = cn;
        cn4[r] = cn;
        hv[r] = hn;
        sg[r][0] = masked ? 0.f : gi; sg[r][1] = masked ? 0.f : gj; sg[r][2] = masked ? 0.f : gf; sg[r][3] = masked ? 0.f : go;
      }
      // publish first (tag = step + 1): one granule per (row, unit), fp32
      if (step + 1 < T && cell_lane) {
        u64* nxt = xb0 + (size_t)((step + 1) & 1) * GPC + pub0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          ns_put_granule(nxt + r, ns_granule((unsigned)(step + 1), hv[r]));
      }
      // results for the backward pass / the consumers of h go to LDS; the saver wave writes them out
      if (cell_lane) {
        char* sv = svs + (size_t)buf * SV_BYTES;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = g * 4 + r;
          ((float*)sv)[row * X3_UPW + ul] = hv[r];
          ((float*)(sv + SV_H))[row * X3_UPW + ul] = cn4[r];
          bf16_t* gp = (bf16_t*)(sv + SV_H + SV_C) + row * 4 * X3_UPW + ul;
#pragma unroll
          for (int gate = 0; gate < 4; ++gate) gp[gate * X3_UPW] = (bf16_t)sg[r][gate];
          ((bf16_t*)(sv + SV_H + SV_C + SV_G))[row * X3_UPW + ul] = (bf16_t)hv[r];
        }
      }
    } while (++step < T);
    ns_lds_barrier();
  } else if (wave < X3W + X3_POLL) {
    // ================================================================ poller role: granule lane + 64 * jj of the chain
    // decodes as r = lane & 3, unit in wave = (lane >> 2) & 7, and with xi = 2 jj + (lane >> 5): g = xi % (RPC / 4),
    // publishing wave = (xi / (RPC / 4)) & 3, publishing workgroup = xi / RPC
    const int j0 = (wave - X3W) * PPG;
    const int pr_ = lane & 3, pu = (lane >> 2) & 7, pgl = lane >> 5;
    for (int step = 0; step < T; ++step) {
      const int buf = step & 1;
      if (step > 0) {
        const u64* cur = xb0 + (size_t)(step & 1) * GPC;
        u64 v[PPG];
        ns_spin sp;
        bool ok;
        do {
          ok = true;
#pragma unroll
          for (int j = 0; j < PPG; ++j) v[j] = ns_ld_granule(cur + lane + (j0 + j) * 64);
#pragma unroll
          for (int j = 0; j < PPG; ++j) ok = ok && ns_granule_tag(v[j]) == (unsigned)step;
          if (!ok && sp.give_up(a.status, 1)) { abortf[buf] = 1; ok = true; }
        } while (!ok);
        bf16_t* dh_ = hsh + (size_t)buf * 16 * H;
        bf16_t* dl_ = hsl + (size_t)buf * 16 * H;
#pragma unroll
        for (int j = 0; j < PPG; ++j) {
          const int xi = 2 * (j0 + j) + pgl;
          const int row = (xi % (RPC / 4)) * 4 + pr_;
          const int k = (xi / RPC) * X3_UPW + ((xi / (RPC / 4)) & 3) * 8 + pu;
          const float x = __uint_as_float((unsigned)v[j]);
          const bf16_t hi = (bf16_t)x;
          const int so = swz_off(row, k, H);
          dh_[so] = hi;
          dl_[so] = (bf16_t)(x - (float)hi);
        }
      }
      ns_lds_barrier();
      if (abortf[buf]) return;
    }
    ns_lds_barrier();
  } else if (wave == X3W + X3_POLL) {
    // ================================================================ saver role (stores only), one slot behind
    // per slot and row: h f32 8 chunks of 16 B, c 8, gates 16, h bf16 4 -> 9 per lane at 16 rows
    constexpr int NH = RPC * 8, NG = RPC * 16, NB = RPC * 4, NJ = (2 * NH + NG + NB + 63) / 64;
    auto save = [&](int step) {
      const int t = d ? T - 1 - step : step;
      const int n0 = rg * RPC;
      const char* sv = svs + (size_t)(step & 1) * SV_BYTES;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int idx = lane + 64 * j;
        if ((2 * NH + NG + NB) % 64 != 0 && idx >= 2 * NH + NG + NB) break;
        const f32x4 v = *(const f32x4*)(sv + idx * 16);
        if (idx < NH) {
          const int row = idx >> 3, cc = idx & 7;
          if (n0 + row < a.N)
            *(f32x4*)(a.hf[d] + ((unsigned)((n0 + row) * a.P + a.padl + t) * (unsigned)a.ld_h + (unsigned)(u0 + cc * 4))) = v;
        } else if (idx < 2 * NH) {
          const int jj = idx - NH, row = jj >> 3, cc = jj & 7;
          if (n0 + row < a.N)
            *(f32x4*)(a.c[d] + ((unsigned)((n0 + row) * a.P + a.padl + t) * (unsigned)H + (unsigned)(u0 + cc * 4))) = v;
        } else if (idx < 2 * NH + NG) {
          const int jj = idx - 2 * NH, row = jj >> 4, gate = (jj >> 2) & 3, cc = jj & 3;
          if (n0 + row < a.N)
            *(f32x4*)(a.gates[d] + ((unsigned)((n0 + row) * a.P + a.padl + t) * (unsigned)(4 * H) + (unsigned)(gate * H + u0 + cc * 8))) = v;
        } else {
          const int jj = idx - 2 * NH - NG, row = jj >> 2, cc = jj & 3;
          if (a.hb[d] && n0 + row < a.N)
            *(f32x4*)(a.hb[d] + ((unsigned)((n0 + row) * a.P + a.padl + t) * (unsigned)a.ld_hb + (unsigned)(u0 + cc * 8))) = v;
        }
      }
    };
    for (int step = 0; step < T; ++step) {
      ns_lds_barrier();
      if (abortf[step & 1]) return;
      if (step > 0) save(step - 1);
    }
    ns_lds_barrier();
    save(T - 1);
  } else {
    // ================================================================ prefetcher role: RPC rows x 4 gates x 32 units = 32 RPC
    // float4 per slot, RPC / 2 per lane: row 2j + (lane >> 5), gate (lane >> 3) & 3, 4 floats at (lane & 7) * 4
    f32x4 pf[RPC / 2];
    const float* xg = a.xg[d];
    const int prow = lane >> 5, pgate = (lane >> 3) & 3, pf4 = (lane & 7) * 4;
    auto pf_load = [&](int step) {
      const int t = d ? T - 1 - step : step;
      const int n0 = rg * RPC;
#pragma unroll
      for (int j = 0; j < RPC / 2; ++j) {
        const int n = n0 + 2 * j + prow;
        pf[j] = n < a.N ? *(const f32x4*)(xg + ((unsigned)(n * a.P + a.padl + t) * (unsigned)a.ld_xg + (unsigned)(pgate * H + u0 + pf4)))
                        : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    };
    auto pf_store = [&](int buf) {
#pragma unroll
      for (int j = 0; j < RPC / 2; ++j) *(f32x4*)(xgs + ((size_t)buf * 16 + 2 * j + prow) * XG3_LD + pgate * X3_UPW + pf4) = pf[j];
    };
    pf_load(0);
    pf_store(0);
    if (T > 1) pf_load(1);
    for (int step = 0; step < T; ++step) {
      ns_lds_barrier();
      if (abortf[step & 1]) return;
      if (step + 1 < T) {
        pf_store((step + 1) & 1);
        if (step + 2 < T) pf_load(step + 2);
      }
    }
    ns_lds_barrier();
  }
}

// ==================================================================== backward, partial-sum exchange
// Every workgroup needs all 4H gate gradients of the step after for dh[t-1] = dgates[t] . Wh^T: sent whole, that is
// 16 x 4H bf16 = 32 KB per chain at H = 256, 4x the forward payload.  The product is cut the other way instead: it is a
// sum over the gate columns, and a workgroup OWNS 256 of them (4 gates x its 64 units).  So it forms, from its own gate
// gradients alone and straight after the cell update, its partial sum for EVERY unit of the layer - P[16, H] =
// dg_own[16, 256] . Wh[:, own columns]^T, 128 MFMAs per step - and sends each peer only the 16 x 64 block of that
// peer's units: (CS - 1) x 512 granules of {step tag, 2 x bf16} in and out per step (12 KB at H = 256, less than the
// forward kernel's), the data is its own flag - no drain, no flag, no second round trip.  The receiver adds its own
// block (fp32, registers) and the peers' (bf16) in a fixed order.  Weights per workgroup: Wh[all H units][own 256
// columns], 128 VGPRs per lane.  Roles: 4 compute waves, prefetcher, saver (the gate gradients for the weight-gradient
// products).
constexpr int BP_WAVES = XW + 2;         // compute, saver, prefetcher
constexpr int DGI_LD = 256 + 8;          // bf16 per row of the operand image (row stride 4 banks mod 64: conflict-free 16-byte reads)

// Who computes what is chosen so that NOTHING of the step's dependent chain crosses waves except the operand image:
//   * compute wave w owns units [16 w, 16 w + 16) of the workgroup's 64 in the cell update, and in the product the HB
//     output tiles {(destination workgroup wd, units 16 w .. 16 w + 16 of ITS 64)}: the tile for wd = this workgroup is
//     the own block of exactly the units the wave updates next step, in exactly the accumulator layout the cell update
//     uses (lane (r16, g): unit r16, rows 4 g .. 4 g + 3 at 16 rows per chain; at 8 / 4 rows the product's A fragment of
//     a padding tile row is read from a live image row, so that lane group g finds the RPC / 4 rows it OWNS - 2 g, 2 g + 1
//     or g - in its own accumulators, and everything element-wise - the stage reads and tanh of indep(), the poll, the
//     sums, the cell update - is done per owned row: 1 row per lane instead of 4 at 4 rows per chain) - it stays in
//     registers;
//   * the peers' blocks are polled by the lane that consumes them (a lane needs only the sums of ITS unit and rows:
//     4 rows x (CS - 1) peers; the forward kernels cannot do this, every lane of theirs needs the whole gathered vector
//     as an MFMA operand): no poller waves, no LDS image of the gathered sums, no hand-over;
//   * everything of the cell update that does not depend on the exchanged sums (operand reads, tanh, the gate
//     derivatives) is done in front of the poll, inside the hop.
// ONE workgroup barrier per slot is left - between the cell update (the four compute waves write the gate gradients
// into the LDS operand image) and the product that reads it; the prefetcher's and the saver's hand-overs ride on it
// (audit, slot s = backward step s: stage[(s+1)&1] is stored between barrier(s-1) and barrier(s), last read in front of
// barrier(s-1), next read behind barrier(s); dgi[s&1] is written in front of barrier(s), read by the product and - one
// slot behind - the saver between barrier(s) and barrier(s+1), rewritten behind barrier(s+1); c0, stage[0] and abortf
// are written in front of the one ns_lds_barrier() every role passes ahead of slot 0, and read behind it).
// Slot timings of the forms that led here: profiles/r03_cluster_bwd_trace.txt.
struct Cluster2pBwdLds {                                              // dynamic LDS of lstm_cluster2p_bwd_kernel (every H, every RPC)
  static constexpr int OPS_G = 16 * 4 * 64 * 2, OPS_F = 16 * 64 * 4;  // 8192, 4096
  static constexpr int OPS_STAGE = OPS_G + 2 * OPS_F;                 // 16384
  LdsCarve c = {};
  int dgi = c.take<bf16_t>(2 * 16 * DGI_LD);                          // [2][16][DGI_LD] this slot's gate gradients (row, gate*64 + unit)
  // The operand stage keeps the row-major layout of the global arrays (a transposing prefetcher store was measured:
  // 96 scattered LDS writes per lane, slower than the compute lanes' scalar reads of this layout)
  int ops = c.take<char>(2 * OPS_STAGE);                              // [2] stages of {gates bf16 [16][4][64], dh f32 [16][64], cprev f32 [16][64]}
  int c0 = c.take<float>(16 * 64);                                    // [16][64] cell state at the first processed step
  int abortf = c.take<int>(8);                                        // [1] in a 32-byte slot
  int bytes = c.off;
};
template <int HB, int RPC>
__global__ __launch_bounds__(BP_WAVES * 64) void lstm_cluster2p_bwd_kernel(LstmClusterArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int H = HB * 64, K4 = 4 * H, CS = HB;
  static_assert(RPC == 16 || RPC == 8 || RPC == 4, "rows per chain");
  constexpr int GPD = RPC * 32;                                       // granules per (destination, source) block
  constexpr Cluster2pBwdLds lay;
  constexpr int OPS_G = Cluster2pBwdLds::OPS_G, OPS_F = Cluster2pBwdLds::OPS_F, OPS_STAGE = Cluster2pBwdLds::OPS_STAGE;
  bf16_t* dgi = carve_at<bf16_t>(smem, lay.dgi); char* ops = carve_at<char>(smem, lay.ops);
  float* c0 = carve_at<float>(smem, lay.c0); int* abortf = carve_at<int>(smem, lay.abortf);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nch = (a.N + RPC - 1) / RPC;                              // chains per direction
  const ns_cluster_slot slot = ns_cluster_place(blockIdx.x, 2 * nch, CS, a.xcd != 0);
  if (!slot.active) return;                                       // padding of a placed grid (exchange.h)
  const int chain = slot.cluster, wgc = slot.member;
  const int d = chain / nch, rg = chain % nch;                      // this workgroup set serves row group rg: batch rows rg * RPC ..
  const int r16 = lane & 15, g = lane >> 4;
  // exchange: [chain][parity][destination][source][RPC / 2 row pairs][64 units]
  u64* xb0 = a.xbuf + (size_t)(d * nch + rg) * 2 * CS * CS * GPD;
  const int u0 = wgc * 64;
  const int T = a.T;
  if (tid == 0) abortf[0] = 0;           // (audit) by wave 0 in front of its first ns_lds_barrier, read behind it
  if (RPC < 16 && (chain | wgc) == 0 && tid == 0) a.status[1] = RPC;   // which form ran (tests, A/B tools)
  auto t_of = [&](int step) { return d ? T - 1 - step : step; };

  if (wave < XW) {
    // ================================================================ compute role
    const int wu = wave * 16 + r16;                    // unit inside the workgroup's 64
    // Lane group g owns OR = RPC / 4 of the chain's rows - g * OR .. - for everything element-wise.  16 rows: those are the
    // accumulator rows 4 g .. 4 g + 3 of the product.  8 / 4 rows: the product's A fragment of tile row i is read from image
    // row arow(i), so that the padding rows of the tile are replicas and every lane group finds its own rows in its own
    // accumulators: 8 rows, arow = 2 (i / 4) + i % 2 - group g holds rows 2 g, 2 g + 1 (one granule) in elements 0, 1;
    // 4 rows, arow = i % 4 - every group holds all four rows, group g takes element g
    constexpr int OR = RPC / 4;
    const int arow = RPC == 16 ? r16 : RPC == 8 ? 2 * (r16 >> 2) + (r16 & 1) : (r16 & 3);
    // Wh[unit wu of workgroup j][own 256 gate columns], the columns in the operand image's order k = unit * 4 + gate
    bf16x8 bw[HB][8];
#pragma unroll
    for (int j = 0; j < HB; ++j) {
      const bf16_t* row = a.wh[d] + (long)(j * 64 + wu) * K4 + u0;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) bw[j][ks][e] = row[(e & 3) * H + ks * 8 + g * 2 + (e >> 2)];
    }
    float dcc[OR], pc[OR];
    f32x4 ownp = {0.f, 0.f, 0.f, 0.f};                 // own block of the partial sums of the step before (elements < OR)
    int len[OR];
#pragma unroll
    for (int r = 0; r < OR; ++r) {
      const int n = rg * RPC + g * OR + r;
      dcc[r] = 0.f; pc[r] = 0.f;
      len[r] = (a.lengths && n < a.N) ? a.lengths[n] : T;
    }
    // element of the own row r in a tile of the product (see arow): explicit selects, no dynamically indexed accumulator
    auto own = [&](const f32x4& v, int r) -> float {
      if constexpr (RPC == 4) return (g & 2) ? ((g & 1) ? v[3] : v[2]) : ((g & 1) ? v[1] : v[0]);
      else return v[r];
    };
    // the part of a slot's cell update that does not need the exchanged sums; computed one slot ahead, under the
    // product's MFMAs (the stage of slot s + 1 is complete behind barrier(s))
    float kdo[OR], kdc[OR], ki[OR], kj[OR], kf[OR], dhx[OR], cpv[OR], gfv[OR];
    auto indep = [&](int bs) {
      const char* st = ops + (size_t)(bs & 1) * OPS_STAGE;
      const bf16_t* sgt = (const bf16_t*)st;
      const float* sdh = (const float*)(st + OPS_G);
      const float* scp = (const float*)(st + OPS_G + OPS_F);
#pragma unroll
      for (int r = 0; r < OR; ++r) {
        const int row = g * OR + r;
        const float gi = (float)sgt[(row * 4 + 0) * 64 + wu], gj = (float)sgt[(row * 4 + 1) * 64 + wu];
        const float gf = (float)sgt[(row * 4 + 2) * 64 + wu], go = (float)sgt[(row * 4 + 3) * 64 + wu];
        const float cprev = scp[row * 64 + wu];
        float ccur = c0[row * 64 + wu];
        if (bs > 0) ccur = pc[r];
        const float tc = tanhf_(ccur);
        dhx[r] = sdh[row * 64 + wu];
        kdo[r] = tc * go * (1.f - go);             // d_o = dh * kdo
        kdc[r] = go * (1.f - tc * tc);             // dc = dh * kdc + dcc
        ki[r] = gj * gi * (1.f - gi);
        kj[r] = gi * (1.f - gj * gj);
        kf[r] = cprev * gf * (1.f - gf);
        cpv[r] = cprev; gfv[r] = gf;
      }
    };
    ns_lds_barrier();                                      // stage 0, c0 and abortf are in place
    indep(0);
    int bs = 0;                                      // backward step index; forward step = T-1-bs
    do {                                             // see lstm_cluster2_fwd_kernel
      const int t = t_of(T - 1 - bs), buf = bs & 1;
      const int n0 = rg * RPC;
      const bool tr = (a.dbg & 16) && (chain | wgc) == 0 && tid == 0 && bs < 512;
      if (tr) a.trace[bs * 8 + 0] = wall_clock64();
      // ---- dh of the step after, summed in a fixed order: own block, then the peers' in workgroup order.
      // Granule (source ws, row pair p, unit wu) of this workgroup's block: {tag bs, rows 2p | 2p + 1}.  A lane polls the
      // granules that hold its own rows: pairs 2 g, 2 g + 1 at 16 rows, pair g at 8, and at 4 pair g / 2, of which it
      // takes the half of row g
      constexpr int NV = OR >= 2 ? OR / 2 : 1;
      f32x4 rec = ownp;
      if (bs > 0 && CS > 1) {
        const u64* cur = xb0 + (size_t)(bs & 1) * CS * CS * GPD + (size_t)wgc * CS * GPD + (g * OR / 2) * 64 + wu;
        // (own loop, the give-up rule of exchange.h spelled out: through ns_poll_granules this kernel measured slower,
        // as its own loop around ns_spin::give_up slower still - profiles/exchange_header.txt)
        u64 v[CS > 1 ? CS - 1 : 1][NV];
        unsigned spins = 0, clk0 = 0;
        bool ok;
        do {
          ok = true;
#pragma unroll
          for (int sx = 0; sx < CS - 1; ++sx) {
            const int ws = sx < wgc ? sx : sx + 1;
#pragma unroll
            for (int h = 0; h < NV; ++h) v[sx][h] = __hip_atomic_load(cur + (size_t)ws * GPD + h * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
#pragma unroll
          for (int sx = 0; sx < CS - 1; ++sx)
#pragma unroll
            for (int h = 0; h < NV; ++h) ok = ok && ((unsigned)(v[sx][h] >> 32) == (unsigned)bs);
          if (!ok && (++spins & 1023u) == 0) {
            if (__hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { abortf[0] = 1; ok = true; }
            else if (ns_spin_timed_out(clk0)) { atomicExch(a.status, 2); abortf[0] = 1; ok = true; }
          }
        } while (!ok);
        if (tr) { a.trace[bs * 8 + 4] = wall_clock64(); a.trace[bs * 8 + 6] = spins; }
#pragma unroll
        for (int sx = 0; sx < CS - 1; ++sx)
#pragma unroll
          for (int h = 0; h < NV; ++h) {
            const unsigned pay = (unsigned)v[sx][h];
            if constexpr (OR >= 2) {
              rec[2 * h] += __uint_as_float(pay << 16);
              rec[2 * h + 1] += __uint_as_float(pay & 0xffff0000u);
            } else {
              rec[0] += __uint_as_float((g & 1) ? (pay & 0xffff0000u) : (pay << 16));
            }
          }
      }
      bf16_t* di = dgi + (size_t)buf * 16 * DGI_LD;
#pragma unroll
      for (int r = 0; r < OR; ++r) {
        const int row = g * OR + r;
        const int n = n0 + row;
        const float dh = dhx[r] + rec[r];
        const float d_o = dh * kdo[r];
        const float dc = dh * kdc[r] + dcc[r];
        float dgv[4] = {dc * ki[r], dc * kj[r], dc * kf[r], d_o};
        dcc[r] = dc * gfv[r];
        if (t >= len[r] || n >= a.N) {
          dgv[0] = dgv[1] = dgv[2] = dgv[3] = 0.f;
          dcc[r] = 0.f;
        }
        pc[r] = cpv[r];
        uint2 pk;
        pk.x = pack_bf16(dgv[0], dgv[1]);
        pk.y = pack_bf16(dgv[2], dgv[3]);
        *(uint2*)(di + row * DGI_LD + wu * 4) = pk;       // k = unit * 4 + gate
      }
      if (tr) a.trace[bs * 8 + 1] = wall_clock64();
      ns_lds_barrier();            // the operand image is complete (all four compute waves)
      if (abortf[0]) return;
      if (tr) a.trace[bs * 8 + 2] = wall_clock64();
      // ---- partial sums of dh from the own 256 gate columns; wave w: units 16 w .. 16 w + 16 of every workgroup
      if (bs + 1 < T) {
        f32x4 acc[HB];
#pragma unroll
        for (int j = 0; j < HB; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
          // narrow forms: the replicas of a row read the same address (a broadcast); image rows >= RPC are never read
          const bf16x8 af = *(const bf16x8*)(di + arow * DGI_LD + ks * 32 + g * 8);
#pragma unroll
          for (int j = 0; j < HB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bw[j][ks], acc[j], 0, 0, 0);
        }
        indep(bs + 1);
        if (tr) a.trace[bs * 8 + 3] = wall_clock64();
        // D: column r16 = unit wu of workgroup j, tile rows g*4 + r = image rows arow(g*4 + r).  A peer's tile -> its
        // granules; the own tile's own rows stay here.  Who stores a granule: at 16 and 8 rows the group that owns the row
        // pair; at 4 rows every group holds both pairs, groups 0 and 1 store pair g
        u64* nxt = xb0 + (size_t)((bs + 1) & 1) * CS * CS * GPD;
#pragma unroll
        for (int j = 0; j < HB; ++j) {
          if (j == wgc) {
            if constexpr (RPC == 16) ownp = acc[j];
            else
#pragma unroll
              for (int r = 0; r < OR; ++r) ownp[r] = own(acc[j], r);
          } else if constexpr (RPC == 16) {
            u64* dst = nxt + (size_t)(j * CS + wgc) * GPD + (g * 2) * 64 + wu;
#pragma unroll
            for (int h = 0; h < 2; ++h)
              ns_put_granule(dst + h * 64, ns_granule((unsigned)(bs + 1), pack_bf16(acc[j][2 * h], acc[j][2 * h + 1])));
          } else if (RPC == 8 || g < 2) {
            const unsigned pay = (RPC == 4 && g) ? pack_bf16(acc[j][2], acc[j][3]) : pack_bf16(acc[j][0], acc[j][1]);
            ns_put_granule(nxt + (size_t)(j * CS + wgc) * GPD + g * 64 + wu, ns_granule((unsigned)(bs + 1), pay));
          }
        }
        if (tr) a.trace[bs * 8 + 7] = wall_clock64();
      } else if (bs + 1 < T) {
        indep(bs + 1);
      }
    } while (++bs < T);
  } else if (wave == XW) {
    // ================================================================ saver role (stores only), one slot behind:
    // the slot's gate gradients out of the operand image [16 rows][unit * 4 + gate] into dgates[row][gate * H + unit]:
    // a lane takes two (row, 8 units) blocks, reads their 8 x {4 gates} and writes one 16-byte chunk per gate
    auto save = [&](int bs) {
      const int t = t_of(T - 1 - bs);
      const int n0 = rg * RPC;
      const bf16_t* di = dgi + (size_t)(bs & 1) * 16 * DGI_LD;
#pragma unroll
      for (int jj = 0; jj < (RPC * 8 + 63) / 64; ++jj) {
        const int idx = lane + 64 * jj, c8 = idx & 7, row = idx >> 3;
        uint2 x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = *(const uint2*)(di + row * DGI_LD + (c8 * 8 + e) * 4);
        if ((RPC == 16 || row < RPC) && n0 + row < a.N) {
          bf16_t* out = a.dgates[d] + ((unsigned)((n0 + row) * a.P + a.padl + t) * (unsigned)K4 + (unsigned)(u0 + c8 * 8));
#pragma unroll
          for (int gate = 0; gate < 4; ++gate) {
            unsigned w[4];
#pragma unroll
            for (int e2 = 0; e2 < 4; ++e2) {
              const unsigned lo = gate < 2 ? x[2 * e2].x : x[2 * e2].y, hi = gate < 2 ? x[2 * e2 + 1].x : x[2 * e2 + 1].y;
              w[e2] = (gate & 1) ? ((lo >> 16) | (hi & 0xffff0000u)) : ((lo & 0xffffu) | (hi << 16));
            }
            *(uint4*)(out + gate * H) = make_uint4(w[0], w[1], w[2], w[3]);
          }
        }
      }
    };
    ns_lds_barrier();
    for (int bs = 0; bs < T; ++bs) {
      if (bs > 0) save(bs - 1);
      ns_lds_barrier();
      if (abortf[0]) return;
    }
    save(T - 1);
  } else {
    // ================================================================ prefetcher role (loads only)
    f32x4 pg[RPC / 2], pd[RPC / 4], pcp[RPC / 4];      // RPC rows of the chain, nothing of the padding rows
    auto pf_load = [&](int bs) {
      const int step = T - 1 - bs;
      const int t = t_of(step), tp = d ? t + 1 : t - 1;
      const bool has_prev = step > 0;
      const int n0 = rg * RPC;
#pragma unroll
      for (int j = 0; j < RPC / 2; ++j) {
        const int idx = lane + 64 * j, c8 = idx & 7, gate = (idx >> 3) & 3, row = idx >> 5;
        const int n = n0 + row;
        pg[j] = n < a.N ? *(const f32x4*)(a.gates[d] + ((unsigned)(n * a.P + a.padl + t) * (unsigned)(4 * H) + (unsigned)(gate * H + u0 + c8 * 8)))
                        : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < RPC / 4; ++j) {
        const int idx = lane + 64 * j, c16 = idx & 15, row = idx >> 4;
        const int n = n0 + row;
        pd[j] = n < a.N ? *(const f32x4*)(a.dh[d] + ((unsigned)(n * a.P + a.padl + t) * (unsigned)a.ld_dh + (unsigned)(u0 + c16 * 4)))
                        : (f32x4){0.f, 0.f, 0.f, 0.f};
        pcp[j] = (n < a.N && has_prev) ? *(const f32x4*)(a.c[d] + ((unsigned)(n * a.P + a.padl + tp) * (unsigned)H + (unsigned)(u0 + c16 * 4)))
                                       : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    };
    auto pf_store = [&](int buf) {
      char* st = ops + (size_t)buf * OPS_STAGE;
#pragma unroll
      for (int j = 0; j < RPC / 2; ++j) *(f32x4*)(st + (size_t)(lane + 64 * j) * 16) = pg[j];
#pragma unroll
      for (int j = 0; j < RPC / 4; ++j) {
        *(f32x4*)(st + OPS_G + (size_t)(lane + 64 * j) * 16) = pd[j];
        *(f32x4*)(st + OPS_G + OPS_F + (size_t)(lane + 64 * j) * 16) = pcp[j];
      }
    };
    {
      const int t0 = t_of(T - 1);
#pragma unroll
      for (int j = 0; j < RPC / 4; ++j) {
        const int idx = lane + 64 * j, c16 = idx & 15, row = idx >> 4;
        const int n = rg * RPC + row;
        const f32x4 v = n < a.N ? *(const f32x4*)(a.c[d] + ((unsigned)(n * a.P + a.padl + t0) * (unsigned)H + (unsigned)(u0 + c16 * 4)))
                                : (f32x4){0.f, 0.f, 0.f, 0.f};
        *(f32x4*)(c0 + idx * 4) = v;
      }
      pf_load(0);
      pf_store(0);
      if (T > 1) pf_load(1);
    }
    ns_lds_barrier();
    for (int bs = 0; bs < T; ++bs) {
      if (bs + 1 < T) {
        pf_store((bs + 1) & 1);
        if (bs + 2 < T) pf_load(bs + 2);
      }
      ns_lds_barrier();
      if (abortf[0]) return;
    }
  }
}

// ------------------------------------------------------------------ C ABI
// `work`: status word at 0, row-count word at 4, the exchange granules, the debug trace behind them.
constexpr size_t RESERVED_BYTES = 4096;          // unused; keeps the exchange and trace offsets where callers and tools expect them
constexpr size_t SPARE_ROW_GROUPS = 1;           // per direction, used by nothing; kept because the size is ABI
struct ClusterWork {
  size_t N, H;
  size_t chains = 2 * ((N + 15) / 16 + SPARE_ROW_GROUPS);          // 16-row groups of both directions
  WorkCarve c = {};
  size_t status = c.take<char>(256);               // the status and row-count words in a block of their own
  size_t reserved = c.take<char>(RESERVED_BYTES);
  // per chain [2][16][2H] granules: the single-role backward kernel's payload, the largest of the forms (the launchers
  // compute what theirs uses; the narrow forms need no more than the 16-row sizing: chain_slots_ok, role_split_ok)
  size_t xbuf = c.take<u64>(chains * 2 * 16 * (4 * H / 2));
  size_t trace = c.take<long long>(512 * 8);       // NS_CLUSTER_DBG bit 16 timestamps
  size_t bytes = c.off;
};
constexpr int MAX_CHAIN_SLOTS = 128;             // 16-row chain slots of the role-split forms, the spare one per direction included: N <= 1008
static bool chain_slots_ok(int N) { return 2 * ((N + 15) / 16 + 1) <= MAX_CHAIN_SLOTS; }

static int cluster_supported(const ns_lstm_seq_params* p0, const ns_lstm_seq_params* p1) {
  return p0->dtype == NS_BF16 && p1->dtype == NS_BF16 && p0->H % 64 == 0 && p0->H <= 512 && p0->T >= 2;
}
// the fp32-state forward form: fp32 h, pre-split recurrent weights, three passes, H <= 256
static int cluster3_supported(const ns_lstm_seq_params* p0, const ns_lstm_seq_params* p1) {
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  const ns_lstm_seq_params* pp[2] = {p0, p1};
  if (p0->H % 64 != 0 || p0->H > 256 || p0->T < 2 || p0->N < 1) return 0;
  if (!chain_slots_ok(p0->N)) return 0;
  for (int d = 0; d < 2; ++d) {
    const ns_lstm_seq_params* p = pp[d];
    if (p->dtype != NS_F32 || p->f32_passes != 3 || !p->whT_hi || !p->whT_lo || !p->xg || !p->h || !p->c || !p->gates) return 0;
    if (!(al16(p->xg) && p->ld_xg % 4 == 0 && al16(p->h) && p->ld_h % 4 == 0 && al16(p->c) && al16(p->gates) &&
          al16(p->whT_hi) && al16(p->whT_lo))) return 0;
    if (p->h_bf16 && !(al16(p->h_bf16) && p->ld_h_bf16 % 8 == 0)) return 0;
    const long widest = p->ld_xg > 4L * p->H ? p->ld_xg : 4L * p->H;
    if ((long)p->N * p->P * widest >= (1L << 31)) return 0;
  }
  return 1;
}
extern "C" int ns_lstm_cluster_supported(const ns_lstm_seq_params* p0, const ns_lstm_seq_params* p1, int backward) {
  if (!p0 || !p1) return 0;
  if (!(p0->reverse == 0 && p1->reverse == 1 && p0->N == p1->N && p0->T == p1->T && p0->H == p1->H)) return 0;
  // a chain (direction, 16-row group) = H / 64 workgroups (H / 32 in the fp32 form) that must be resident together; the
  // chains are independent of one another
  if ((p0->H + 31) / 32 > ns_device_cus()) return 0;
  if (cluster_supported(p0, p1)) return 1;
  return !backward && cluster3_supported(p0, p1);
}

extern "C" size_t ns_lstm_cluster_work_bytes(const ns_lstm_seq_params* p) {
  if (!p) return 0;
  return ClusterWork{(size_t)p->N, (size_t)p->H}.bytes;
}

static void fill(LstmClusterArgs& a, const ns_lstm_seq_params* p0, const ns_lstm_seq_params* p1, void* work) {
  const ns_lstm_seq_params* pp[2] = {p0, p1};
  a.N = p0->N; a.T = p0->T; a.H = p0->H; a.P = p0->P; a.padl = p0->padl; a.CS = p0->H / 64;
  a.ld_xg = p0->ld_xg; a.ld_h = p0->ld_h; a.ld_dh = p0->ld_dh;
  a.lengths = p0->lengths; a.forget_bias = p0->forget_bias; a.cell_clip = p0->cell_clip;
  for (int d = 0; d < 2; ++d) {
    a.xg[d] = pp[d]->xg; a.whT[d] = (const bf16_t*)pp[d]->whT; a.wh[d] = (const bf16_t*)pp[d]->wh;
    a.h[d] = (bf16_t*)pp[d]->h; a.c[d] = pp[d]->c; a.gates[d] = (bf16_t*)pp[d]->gates;
    a.dh[d] = pp[d]->dh; a.dgates[d] = (bf16_t*)pp[d]->dgates;
    a.whT_hi[d] = (const bf16_t*)pp[d]->whT_hi; a.whT_lo[d] = (const bf16_t*)pp[d]->whT_lo;
    a.hf[d] = (float*)pp[d]->h; a.hb[d] = (bf16_t*)pp[d]->h_bf16;
  }
  a.ld_hb = p0->ld_h_bf16;
  const ClusterWork wl{(size_t)a.N, (size_t)a.H};
  a.status = carve_at<int>(work, wl.status);
  a.xbuf = carve_at<u64>(work, wl.xbuf);
  const char* dbg = getenv("NS_CLUSTER_DBG");
  a.dbg = dbg ? atoi(dbg) : 0;
  a.xcd = ns_cluster_placed("bilstm") ? 1 : 0;
  a.trace = carve_at<long long>(work, wl.trace);
}

// Every launch zeroes the status and row-count words and the exchange granules it will use (tag 0 = nothing published).
static int zero_work(void* work, size_t xbytes, hipStream_t s) {
  constexpr size_t xbuf = ClusterWork{0, 0}.xbuf;  // (the offset depends on neither N nor H)
  return ns_zero_async(work, ((xbuf + xbytes) + 15) & ~(size_t)15, s);
}

// The role-split kernels cover H <= 256 with 16-byte aligned operand rows; everything else the cluster path accepts
// runs the single-role kernels.
static bool role_split_ok(const LstmClusterArgs& a, bool bwd) {
  if (a.H > 256 || a.H % 64) return false;
  // the narrow forms' chains (ceil(N / rows) per direction) need no more exchange bytes than the 16-row layout the work
  // buffer is sized for: ceil(N / rows) * rows <= ceil(N / 16) * 16
  if (!chain_slots_ok(a.N)) return false;
  const long widest = a.ld_xg > 4L * a.H ? a.ld_xg : 4L * a.H;
  if ((long)a.N * a.P * (widest > a.ld_dh ? widest : a.ld_dh) >= (1L << 31)) return false;   // 32-bit element offsets
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  for (int d = 0; d < 2; ++d) {
    if (!bwd && !(al16(a.xg[d]) && a.ld_xg % 4 == 0 && al16(a.h[d]) && a.ld_h % 8 == 0 && al16(a.c[d]) && al16(a.gates[d]))) return false;
    if (bwd && !(al16(a.dh[d]) && a.ld_dh % 4 == 0 && al16(a.c[d]) && al16(a.gates[d]) && al16(a.dgates[d]))) return false;
  }
  return true;
}

// Rows per chain of the role-split kernels (lstm_cluster2_fwd, lstm_cluster3_fwd, lstm_cluster2p_bwd): 16, 8 or 4.  A
// narrower chain moves fewer bytes per hop and takes more workgroups (2 * ceil(N / rows) * wgs_per_chain).  The rule:
// the narrowest form whose grid stays within half of the device's CUs (every workgroup of a launch has to be resident,
// and other streams run beside these launches; at batch 32, H 256 that is 4 rows in all three kernels - 64 workgroups,
// 128 for the fp32 form, measured faster than 8 rows on 64: profiles/cluster_rows.txt).  NS_CLUSTER_ROWS=16|8|4, read
// per call, forces a form for A/B runs and tests; a forced form is widened until its grid fits the device.
// A narrow form writes its row count into the second int of `work` (zeroed with the status word: 0 = 16 rows).
static int cluster_rows(int N, int wgs_per_chain) {
  const int cus = ns_device_cus();
  auto grid = [&](int rows) { return 2 * ((N + rows - 1) / rows) * wgs_per_chain; };
  const char* e = getenv("NS_CLUSTER_ROWS");
  const int want = e ? atoi(e) : 0;
  if (want == 16 || want == 8 || want == 4) {
    int rows = want;
    while (rows < 16 && grid(rows) > cus) rows *= 2;
    return rows;
  }
  for (int rows = 4; rows < 16; rows *= 2)
    if (grid(rows) <= cus / 2) return rows;
  return 16;
}

// The instantiations of a role-split kernel, [H / 64 - 1][rows per chain 4, 8, 16]
typedef void (*cluster_kernel_t)(LstmClusterArgs);
#define NS_ROLE_SPLIT_FORMS(K) \
  {{K<1, 4>, K<1, 8>, K<1, 16>}, {K<2, 4>, K<2, 8>, K<2, 16>}, {K<3, 4>, K<3, 8>, K<3, 16>}, {K<4, 4>, K<4, 8>, K<4, 16>}}
static const cluster_kernel_t cluster2_fwd_forms[4][3] = NS_ROLE_SPLIT_FORMS(lstm_cluster2_fwd_kernel);
static const cluster_kernel_t cluster3_fwd_forms[4][3] = NS_ROLE_SPLIT_FORMS(lstm_cluster3_fwd_kernel);
static const cluster_kernel_t cluster2p_bwd_forms[4][3] = NS_ROLE_SPLIT_FORMS(lstm_cluster2p_bwd_kernel);
#undef NS_ROLE_SPLIT_FORMS
static cluster_kernel_t role_split_form(const cluster_kernel_t (&forms)[4][3], int H, int rows) {
  return forms[H / 64 - 1][rows == 4 ? 0 : rows == 8 ? 1 : 2];
}

// Both directions of a BiLSTM, whole sequence, one launch.  p0 must be the forward-in-time direction
// (reverse = 0) and p1 the reversed one.  `work` (ns_lstm_cluster_work_bytes) holds the exchange
// buffers; its first int is a status word: 0 ok, non-zero = a spin timed out (results invalid).
extern "C" int ns_lstm_cluster_fwd(const ns_lstm_seq_params* p0, const ns_lstm_seq_params* p1, void* work,
                                   ns_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  NS_CHECK_ARG(p0 && p1 && work, "ns_lstm_cluster_fwd: null");
  if (p0->dtype != NS_F32) NS_CHECK_ARG(cluster_supported(p0, p1), "ns_lstm_cluster_fwd: needs bf16, H %% 64 == 0, H <= 512, T >= 2");
  NS_CHECK_ARG(p0->reverse == 0 && p1->reverse == 1 && p0->N == p1->N && p0->T == p1->T && p0->H == p1->H,
               "ns_lstm_cluster_fwd: p0 forward / p1 reversed with equal shapes expected");
  if (p0->dtype == NS_F32) {
    NS_CHECK_ARG(cluster3_supported(p0, p1), "ns_lstm_cluster_fwd: the fp32 form needs H %% 64 == 0, H <= 256, T >= 2, "
                 "f32_passes 3 with whT_hi / whT_lo, 16-byte aligned operands");
    LstmClusterArgs a = {};
    fill(a, p0, p1, work);
    a.xcd = ns_cluster_placed("bilstmf32") ? 1 : 0;      // a family of its own: H / 32 members that all poll the whole chain
    const int RPC = cluster_rows(a.N, a.H / X3_UPW), nch = (a.N + RPC - 1) / RPC;   // chains per direction
    const size_t xbytes = 2 * (size_t)nch * 2 * RPC * (size_t)a.H * sizeof(u64);
    { const int zrc = zero_work(work, xbytes, s); if (zrc) return zrc; }
    const size_t lds3 = Cluster3FwdLds{a.H, RPC}.bytes;
    static bool attr3 = false;
    if (!attr3) {
      for (const auto& widths : cluster3_fwd_forms)
        for (cluster_kernel_t k : widths) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      attr3 = true;
    }
    hipLaunchKernelGGL(role_split_form(cluster3_fwd_forms, a.H, RPC), dim3((unsigned)ns_cluster_grid(2 * nch, a.H / X3_UPW, a.xcd != 0)),
                       dim3(X3_WAVES * 64), lds3, s, a);
    NS_CHECK_LAUNCH("lstm_cluster3_fwd");
    return NS_OK;
  }
  NS_CHECK_ARG(cluster_supported(p0, p1), "ns_lstm_cluster_fwd: needs bf16, H %% 64 == 0, H <= 512, T >= 2");
  LstmClusterArgs a = {};
  fill(a, p0, p1, work);
  const bool split = role_split_ok(a, false);
  const int RPC = split ? cluster_rows(a.N, a.CS) : 16, nch = (a.N + RPC - 1) / RPC;   // chains per direction
  const size_t xbytes = 2 * (size_t)nch * 2 * RPC * (size_t)(a.H / 2) * sizeof(u64);
  { const int zrc = zero_work(work, xbytes, s); if (zrc) return zrc; }
  if (split) {
    const size_t lds2 = Cluster2FwdLds{a.H, RPC}.bytes;
    hipLaunchKernelGGL(role_split_form(cluster2_fwd_forms, a.H, RPC), dim3((unsigned)ns_cluster_grid(2 * nch, a.CS, a.xcd != 0)), dim3(FW_WAVES * 64),
                       lds2, s, a);
    NS_CHECK_LAUNCH("lstm_cluster2_fwd");
    return NS_OK;
  }
  const size_t lds = (size_t)16 * a.H * 2;
  hipLaunchKernelGGL(lstm_cluster_fwd_kernel, dim3((unsigned)ns_cluster_grid(2 * nch, a.CS, a.xcd != 0)), dim3(CTHREADS), lds, s, a);
  NS_CHECK_LAUNCH("lstm_cluster_fwd");
  return NS_OK;
}

extern "C" int ns_lstm_cluster_bwd(const ns_lstm_seq_params* p0, const ns_lstm_seq_params* p1, void* work,
                                   ns_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  NS_CHECK_ARG(p0 && p1 && work, "ns_lstm_cluster_bwd: null");
  NS_CHECK_ARG(cluster_supported(p0, p1), "ns_lstm_cluster_bwd: needs bf16, H %% 64 == 0, H <= 512, T >= 2");
  NS_CHECK_ARG(p0->reverse == 0 && p1->reverse == 1 && p0->N == p1->N && p0->T == p1->T && p0->H == p1->H,
               "ns_lstm_cluster_bwd: p0 forward / p1 reversed with equal shapes expected");
  LstmClusterArgs a = {};
  fill(a, p0, p1, work);
  // exchange granules - partial-sum kernel: [chain][2][CS][CS][32 x rows]; single-role kernel: [chain][2][16][2H]
  const bool psum = role_split_ok(a, true);
  const int RPC = psum ? cluster_rows(a.N, a.CS) : 16, nch = (a.N + RPC - 1) / RPC;    // chains per direction
  const size_t xbytes = 2 * (size_t)nch * 2 * (psum ? (size_t)a.CS * a.CS * RPC * 32 : 16 * (size_t)(4 * a.H / 2)) * sizeof(u64);
  { const int zrc = zero_work(work, xbytes, s); if (zrc) return zrc; }
  if (psum) {
    const size_t ldsp = Cluster2pBwdLds().bytes;
    hipLaunchKernelGGL(role_split_form(cluster2p_bwd_forms, a.H, RPC), dim3((unsigned)ns_cluster_grid(2 * nch, a.CS, a.xcd != 0)), dim3(BP_WAVES * 64),
                       ldsp, s, a);
    NS_CHECK_LAUNCH("lstm_cluster2p_bwd");
    return NS_OK;
  }
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)lstm_cluster_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  const size_t lds = ClusterBwdLds{a.H}.bytes;
  hipLaunchKernelGGL(lstm_cluster_bwd_kernel, dim3((unsigned)ns_cluster_grid(2 * nch, a.CS, a.xcd != 0)), dim3(CTHREADS), lds, s, a);
  NS_CHECK_LAUNCH("lstm_cluster_bwd");
  return NS_OK;
}
