// Persistent LSTM recurrence for WIDE cells at small batch (the two decoder LSTMs of tacotron2.py:67-73: 1024 units,
// 32 rows, 200 steps): ONE launch for the whole sequence instead of one per time step.
//
// The launch-per-step kernels re-stream the whole recurrent matrix (16.8 MB as hi + lo bf16 planes, forward) through
// every CU each step and pay a dependent-launch boundary on top: ~9.9 us per step.  Here a workgroup keeps its slice of
// W_h resident for all steps, the cell state too, and only the state travels between the workgroups of a row group.
// The two directions exchange it differently.
//
// FORWARD (lstm_wide_fwd_kernel): workgroup = 16 batch rows x 8 units, 8 units x 4 gates x H of W_h^T as hi / lo MFMA
// B fragments in registers (64 VGPRs per lane).  h travels through the history array the kernel has to write anyway:
//   before the launch: a fill kernel writes an all-ones NaN pattern (the SENTINEL, a value the recurrence never
//              stores) over every (row, step) of h;
//   per step:  8 SWEEPER waves split K.  Each polls ONE 16-byte piece per producing workgroup of its K slice (sc1 =
//              L1- and L2-bypassing loads) and fetches the 16 rows of a producer's units as soon as that producer's
//              piece is no longer the sentinel - the data is its own flag: a step costs one store -> load hop with
//              no drain, no counter and no second round trip -, then MFMA and partial sums into LDS;
//              2 CELL waves add the partials, update the cell, publish h[t] with 16-byte sc1 write-through stores and
//              do every other memory access of the step.
// 16-byte sc1 stores arrive as untorn 8-byte halves on gfx950 (MI355X_MICROARCH.md, hand-off table) and every element
// of every fetched piece is checked, so a piece passes only when all of it is new; a stale piece is fetched again.
// The cell update never produces the sentinel (a NaN of that bit pattern is rewritten to the canonical quiet NaN).
// With fp32 storage and the optional planes h_bf16 / h_lo_bf16 (the SPLIT form, see the kernel) h travels pre-split as
// (hi, lo) bf16 pairs through an exchange array in `work` instead: the producer splits each value once, the sweepers
// load MFMA operands, and the planes, written on the side, serve the later products that would split or cast h again.
// Why a probe instead of polling with the sweep itself: 256 CUs re-reading 64 KB each per pass is 16 MB per pass on the
// memory side (sc1 loads do not hit in L2) - the passes then take 2.2 us each and the CU's own publish store queues
// behind them.  Measured per step at the benchmark shape (profiles/r02_wide_trace.txt): arrival counters + drained
// stores 8.7 us; sentinel polling by full sweeps 7.9; probe, then one sweep 5.2; probe and sweep interleaved 4.9.  What
// is left is the hop itself: store -> visible + one probe round trip (1.9 us) + one data round trip (1.5 us), then
// ~1.5 us of MFMA, barrier and cell update.
//
// BACKWARD (lstm_wide_bwd_ps_kernel): workgroup = 8 batch rows x 32 units.  dh[t-1] = dgates[t] . Wh^T is a sum over
// the gate columns and a workgroup owns 128 of them, so it sends every peer its PARTIAL SUM for that peer's units as
// {step tag, 2 x bf16} granules through an exchange area of `work` (zeroed per launch; the tag is the flag): one hop and
// no probe, 4.1 us per step.  Nothing is filled with the sentinel in this direction.  The comment above the kernel has
// the details.
//
// Tried and replaced: round 2 ran the backward recurrence in the forward kernel's form - 8 or 16 rows x 16 units, the
// bf16 gate gradients sentinel-filled and swept, all 4H of them per workgroup and step (64 KB at 8 rows) behind a
// probe.  Two dependent round trips: 7.0 us per step, 6.6 with 8-row groups, 6.0 / 5.9 with a prober wave
// (profiles/r02_wide_trace.txt).  Round 3's partial sums replaced it (profiles/r03_wide_trace.txt); that
// kernel and a 16-unit form of the partial-sum kernel (twice the write-through bytes, 4.97 us) stayed behind an
// environment switch that no test set and were retired (profiles/wide_forms_retired.txt).
//
// Every spin is bounded ("The tagged-granule exchange"; the forward sweep keeps its own loop with the same
// bound); a timeout raises the status word and all waves of the workgroup leave together.  The grid
// (row groups x unit blocks, one workgroup per CU) must be resident at once: ns_lstm_wide_supported() refuses shapes
// that do not fit.
#include "exchange.h"
#include "carve.h"
#include <stdint.h>
#include <stdlib.h>

namespace {
constexpr int WT = 512, WW = WT / 64;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr size_t WIDE_TRACE_BYTES = 256 * 8 * sizeof(long long);

struct WideArgs {
  ns_lstm_seq_params p;
  int* status;
  long long* trace;     // NS_WIDE_TRACE=1: [step][8] timestamps (100 MHz) of workgroup 0, else null
  int nub;              // forward kernel only: unit blocks (of 8) per row group, set by ns_lstm_wide_fwd
  void* xch;            // forward kernel, split form: the exchange array [N * P][H / 8][hi x 8 | lo x 8] bf16 (in work)
};
__device__ __forceinline__ void wstamp(const WideArgs& a, int st, int k) {
  if (a.trace && blockIdx.x == 0 && threadIdx.x == 0 && st < 256) a.trace[st * 8 + k] = wall_clock64();
}

// ---- the sentinel: all ones (a NaN in both storage types)
template <typename T> __device__ __forceinline__ bool has_sentinel(const u32x4& v);
template <> __device__ __forceinline__ bool has_sentinel<float>(const u32x4& v) {
  return (v[0] == 0xffffffffu) | (v[1] == 0xffffffffu) | (v[2] == 0xffffffffu) | (v[3] == 0xffffffffu);
}
// bf16: 0xffff is the largest 16-bit pattern, so a piece holds it iff the packed unsigned maximum of its halves is it
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_max_u16(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
template <> __device__ __forceinline__ bool has_sentinel<bf16_t>(const u32x4& v) {
  const unsigned m = pk_max_u16(pk_max_u16(v[0], v[1]), pk_max_u16(v[2], v[3]));
  return ((m & 0xffffu) == 0xffffu) | (m >= 0xffff0000u);
}
__device__ __forceinline__ float clean(float x, float*) { return __float_as_uint(x) == 0xffffffffu ? __uint_as_float(0x7fc00000u) : x; }
__device__ __forceinline__ bf16_t clean(float x, bf16_t*) {
  const bf16_t b = (bf16_t)x;
  return __builtin_bit_cast(unsigned short, b) == 0xffffu ? __builtin_bit_cast(bf16_t, (unsigned short)0x7fc0u) : b;
}

template <typename T>
__global__ __launch_bounds__(256) void wide_fill_kernel(T* base, int N, long P, int padl, int T_, long ld, int width) {
  // 16-byte pieces of rows (n, padl + t), t < T_
  const int ppr = width * (int)sizeof(T) / 16;
  const long total = (long)N * T_ * ppr;
  const u32x4 s = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long row = i / ppr;
    const int pc = (int)(i - row * ppr);
    const long n = row / T_, t = row - n * T_;
    *(u32x4*)((char*)(base + (n * P + padl + t) * ld) + pc * 16) = s;
  }
}

// Probe and sweep interleaved: the wave polls one piece per producer of its K slice and issues each of its NL sweep
// loads as soon as the PPCH producers that load covers (LPC consecutive loads share them) have published, so that
// when the last producer arrives only its own pieces are still to be fetched.  Every piece is checked once all are in
// (the probe looked at one row only) and a stale one is fetched again.
template <typename T, int NL, int LPC, int PPCH>
__device__ __forceinline__ unsigned sweep_progressive(const void* base, size_t bytes, unsigned poff0, unsigned pstride,
                                                      unsigned off0, unsigned in_grp, unsigned per_grp, u32x4 (&v)[NL], int lane,
                                                      int* status, int* abortf, int code, long long* tslot) {
  constexpr int NP = (NL / LPC) * PPCH;                       // producers of this wave's K slice
  constexpr unsigned long long ALLP = NP >= 64 ? ~0ull : ((1ull << NP) - 1ull);
  constexpr unsigned ALLL = (1u << NL) - 1u;
  const unsigned blo = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)base), bhi = __builtin_amdgcn_readfirstlane((unsigned)((uintptr_t)base >> 32));
  const int nrec = __builtin_amdgcn_readfirstlane((int)bytes);
  const unsigned poff = lane < NP ? poff0 + (unsigned)lane * pstride : 0x80000000u;
  unsigned long long ready = 0ull;
  unsigned done = 0u, spins = 0u, clk0 = 0u;
  for (;;) {
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)(((uintptr_t)bhi << 32) | blo), 0, nrec, 0x00020000);
    if (ready != ALLP) {
      const u32x4 pv = __builtin_amdgcn_raw_buffer_load_b128(rs, poff, 0, 16);
      ready |= __builtin_amdgcn_ballot_w64(lane < NP && !has_sentinel<T>(pv));
      if (tslot && ready == ALLP && blockIdx.x == 0 && threadIdx.x == 0) *tslot = wall_clock64();
    }
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      constexpr unsigned long long one = 1ull;
      const unsigned long long m = ((one << PPCH) - one) << ((l / LPC) * PPCH);
      if (!(done & (1u << l)) && (ready & m) == m) {
        const unsigned o = off0 + (unsigned)(l % LPC) * in_grp + (unsigned)(l / LPC) * per_grp;
        v[l] = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 16);      // sc1, as every load of handed-off bytes
        done |= 1u << l;
      }
    }
    ++spins;
    if (done == ALLL) {
      if constexpr (sizeof(T) == 2) {        // all pieces at once first (the usual outcome: none is stale)
        u32x4 m = v[0];
#pragma unroll
        for (int l = 1; l < NL; ++l)
#pragma unroll
          for (int i = 0; i < 4; ++i) m[i] = pk_max_u16(m[i], v[l][i]);
        if (!__any(has_sentinel<T>(m))) return spins;
      }
      unsigned stale = 0u;
#pragma unroll
      for (int l = 0; l < NL; ++l) if (__any(has_sentinel<T>(v[l]))) stale |= 1u << l;
      if (!stale) return spins;
      done &= ~stale;
    }
    if ((spins & 255u) == 0) {
      if (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { if (lane == 0) *abortf = 1; return 0; }
      if ((spins & 1023u) == 0 && ns_spin_timed_out(clk0)) { if (lane == 0) { atomicExch(status, code); *abortf = 1; } return 0; }
    }
  }
}

// ===================================================================================== forward
// Waves 0..7 (the sweepers) split K: sweep, MFMA, partial sums into LDS.  Waves 8, 9 (the cell waves; thread = (row,
// unit)) add the partials, update the cell, publish h[t] and do every other memory access of the step.  The roles are
// separate because a wave's vector-memory operations complete in issue order: a polling load queued behind the
// write-through publish store, the late stores or an operand fetch from HBM returns only after those (the one-role
// version measured 3.7 us for a sweep that succeeded at its first pass).
// NCH = 32-wide K chunks per sweeper (H / 256); PASSES = 3: fp32 state, hi / lo weight planes; 1: bf16 everywhere
// A PROBER wave - a third cell-side wave that polls for the whole workgroup with nothing else in its memory queue and
// hands the producers' bits to the sweepers in LDS - was tried in round 2 and round 3 and was slower forward, 5.25
// against 5.04 us per step: the sweepers keep their own probes.
// SPLIT (T = float, PASSES = 3, both planes given): h travels pre-split, hi = bf16(h) and lo = bf16(h - hi), instead of
// as fp32.  The cell waves have each value in a register exactly once and split it there; a sweeper's pieces are then
// the MFMA A operands as loaded - no conversion between "state arrives" and the products, where the fp32 form has every
// sweeper lane of every workgroup of the row group split its 32 values per step (the same 16 x H values, H / 8 times
// over).  The exchange goes through an array of its own (in work): [row][unit block][hi x 8 | lo x 8], so a producer
// still owns 32 contiguous bytes of a row and every store, probe and sweep address is the fp32 form's.  (Exchanging
// through the two planes themselves was measured first: 1.08 ms a launch against 1.06 for this layout with the same
// sentinel check - a producer's two 16-byte stores then land in lines it shares with its neighbours - and both lost
// to the fp32 form's 1.02 until the bf16 check became the packed maximum of has_sentinel<bf16_t>: eight compares a
// piece cost what the split had saved.  profiles/wide_split.txt.)
// That array carries the sentinel; the planes p.h_bf16 / p.h_lo_bf16 and the fp32 h are written with plain stores
// behind the publish (later kernels read them) and are not filled.
constexpr int WTF = WT + 128;
template <typename T, int PASSES, int NCH, bool SPLIT>
__global__ __launch_bounds__(WTF) void lstm_wide_fwd_kernel(WideArgs a) {
  static_assert(!SPLIT || (sizeof(T) == 4 && PASSES == 3), "the split form is the fp32 three-pass arrangement");
  // Partial sums, sweepers -> cell waves.  Row stride = 4 mod 16 floats: conflict-free for the MFMA C layout's writes
  // (+1 is not).  Two images by step parity (LDS hand-over audit, round 3): the barrier of step t orders the sweepers'
  // writes before the cell waves' reads, but a sweeper whose K slice does not hold this workgroup's own units needs
  // nothing from these cell waves to finish step t+1 - with ONE image its next write was kept behind their reads only by
  // the two memory round trips every sweep takes.  With two, image (t & 1) is written again in step t+2, which a sweeper
  // enters through the barrier of step t+1, and the cell waves reach that barrier after their reads of step t.
  __shared__ float red[2][WW][16][36];
  __shared__ __attribute__((aligned(16))) T hst[16][8];      // SPLIT: [plane][16][8] bf16, the same 512 bytes
  __shared__ int abortf;
  const ns_lstm_seq_params& p = a.p;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = p.H, NUB = a.nub;
  const int rg = blockIdx.x / NUB, ub = blockIdx.x % NUB;
  const int n0 = rg * 16, u0 = ub * 8;
  if (tid == 0) abortf = 0;                          // (audit) initialised in front of the barrier below
  // what is exchanged: the history array, or (SPLIT) the array of (hi x 8 | lo x 8) pieces in work
  const void* const xbase = SPLIT ? (const void*)a.xch : (const void*)p.h;
  const long xld = SPLIT ? (long)p.H : (long)p.ld_h;             // in units of XSZ bytes: a unit's (hi, lo) pair or its value
  constexpr unsigned XSZ = (unsigned)sizeof(T);
  const size_t hbytes = (size_t)p.N * p.P * xld * XSZ;
  constexpr int PPC = 8 * (int)sizeof(T) / 16;        // 16-byte pieces per 8-value fragment (2 for fp32, 1 for bf16)
  __syncthreads();

  if (wave < WW) {
    // ------------------------------------------------------------------ sweepers
    const int r16 = lane & 15, g = lane >> 4;
    const int k0 = wave * (H / WW);
    // resident weight fragments: tile j, column r16 -> gate 2j + (r16 >> 3), unit u0 + (r16 & 7)
    bf16x8 bh[2][NCH], bl[2][NCH];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const long wrow = ((long)(2 * j + (r16 >> 3)) * H + u0 + (r16 & 7)) * H + k0 + g * 8;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        if constexpr (PASSES == 3) {
          bh[j][c] = *(const bf16x8*)((const bf16_t*)p.whT_hi + wrow + c * 32);
          bl[j][c] = *(const bf16x8*)((const bf16_t*)p.whT_lo + wrow + c * 32);
        } else {
          bh[j][c] = *(const bf16x8*)((const bf16_t*)p.whT + wrow + c * 32);
          bl[j][c] = bh[j][c];
        }
      }
    }
    const bool ok = n0 + r16 < p.N;
    // the probed row differs from workgroup to workgroup and wave to wave: 2,000 waves polling the same few lines would
    // all queue on the same memory channels
    const int prb = (ub * WW + wave) % min(16, p.N - n0);
    for (int t = 0; t < p.T; ++t) {
      f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      wstamp(a, t, 0);
      if (t > 0) {
        const unsigned rowoff = ok ? (unsigned)(((long)(n0 + r16) * p.P + p.padl + t - 1) * xld + k0 + g * 8) * XSZ : 0x80000000u;
        u32x4 v[NCH * PPC];
        const unsigned prow = (unsigned)(((long)(n0 + prb) * p.P + p.padl + t - 1) * xld + k0) * XSZ;
        long long* const tslot = a.trace && t < 256 ? a.trace + t * 8 + 6 : nullptr;
        unsigned got;
        // SPLIT: the same addresses as the fp32 form; piece 0 of a chunk is the lane's hi fragment, piece 1 its lo
        // fragment (a lo piece that lags its hi piece fails the check of every piece and is fetched again)
        if constexpr (SPLIT)
          got = sweep_progressive<bf16_t, 2 * NCH, 2, 4>(xbase, hbytes, prow, 32u, rowoff, 16u, 128u, v, lane, a.status, &abortf, 1, tslot);
        else
          got = sweep_progressive<T, NCH * PPC, PPC, 4>(xbase, hbytes, prow, 8u * XSZ, rowoff, 16u, 32u * XSZ, v, lane, a.status, &abortf, 1, tslot);
        wstamp(a, t, 1);
        if (a.trace && blockIdx.x == 0 && tid == 0 && t < 256) a.trace[t * 8 + 5] = got;
        if (got) {
#pragma unroll
          for (int c = 0; c < NCH; ++c) {
            bf16x8 ah, al;
            if constexpr (SPLIT) {
              ah = *(bf16x8*)&v[2 * c];
              al = *(bf16x8*)&v[2 * c + 1];
            } else if constexpr (sizeof(T) == 4) {
              const u32x4 x = v[2 * c], y = v[2 * c + 1];
              const float f[8] = {__uint_as_float(x[0]), __uint_as_float(x[1]), __uint_as_float(x[2]), __uint_as_float(x[3]),
                                  __uint_as_float(y[0]), __uint_as_float(y[1]), __uint_as_float(y[2]), __uint_as_float(y[3])};
#pragma unroll
              for (int i = 0; i < 8; ++i) { const bf16_t h = (bf16_t)f[i]; ah[i] = h; al[i] = (bf16_t)(f[i] - (float)h); }
            } else {
              ah = *(bf16x8*)&v[c];
              al = ah;
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              if constexpr (PASSES == 3) acc[j] = mfma_split<3>(ah, al, bh[j][c], bl[j][c], acc[j]);
              else acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[j][c], acc[j], 0, 0, 0);
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[t & 1][wave][g * 4 + q][j * 16 + r16] = acc[j][q];
      __syncthreads();
      if (abortf) return;
      wstamp(a, t, 2);
    }
    return;
  }
  // -------------------------------------------------------------------- cell waves: thread = (row er, unit eu)
  const int e = tid - WT, er = e >> 3, eu = e & 7;
  const int en = n0 + er;
  const bool eok = en < p.N;
  const int elen = (eok && p.lengths) ? p.lengths[en] : p.T;
  const auto hrs = __builtin_amdgcn_make_buffer_rsrc((void*)xbase, 0, (int)hbytes, 0x00020000);
  const bool tr = a.trace && blockIdx.x == 0 && e == 0;
  float cst = 0.f;
  float hprev = 0.f;          // zoneout: this thread's h of the step before (fp32, before the store's rounding)
  const bool zone = p.zoneout_thr_cell != 0u || p.zoneout_thr_output != 0u;
  float pz[4] = {0.f, 0.f, 0.f, 0.f};
  auto load_xg = [&](int t) {
    if (eok) {
      const float* xr = p.xg + ((long)en * p.P + p.padl + t) * p.ld_xg + u0 + eu;
#pragma unroll
      for (int j = 0; j < 4; ++j) pz[j] = xr[(long)j * H];
    }
  };
  load_xg(0);
  for (int t = 0; t < p.T; ++t) {
    __syncthreads();
    if (abortf) return;
    if (tr && t < 256) a.trace[t * 8 + 3] = wall_clock64();
    float z[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float s = pz[j];
#pragma unroll
      for (int w = 0; w < WW; ++w) s += red[t & 1][w][er][(j >> 1) * 16 + (j & 1) * 8 + eu];
      z[j] = s;
    }
    float gi = sigmoidf_(z[0]), gj = tanhf_(z[1]), gf = sigmoidf_(z[2] + p.forget_bias), go = sigmoidf_(z[3]);
    float hv;
    if (!zone) {
      cst = ns_cell_clip(gf * cst + gi * gj, p.cell_clip);
      hv = go * tanhf_(cst);
    } else {                  // ns_lstm_seq_params: a kept unit carries c / h of step t-1 on, h' comes from the plain c'
      const float cn = ns_cell_clip(gf * cst + gi * gj, p.cell_clip);
      hv = go * tanhf_(cn);
      if (!ns_zone_keep(p.zoneout_seed_cell, (uint32_t)t, (uint32_t)en, (uint32_t)(u0 + eu), p.zoneout_thr_cell)) cst = cn;
      if (ns_zone_keep(p.zoneout_seed_output, (uint32_t)t, (uint32_t)en, (uint32_t)(u0 + eu), p.zoneout_thr_output)) hv = hprev;
      hprev = hv;
    }
    if (t >= elen) { cst = 0.f; hv = 0.f; gi = gj = gf = go = 0.f; }
    // (audit) hst: written and read by the SAME cell wave (wave w owns rows 8w .. 8w+7 on both sides), so the release
    // fence + wave barrier below is all the ordering it needs; no other role touches it
    if constexpr (SPLIT) {
      bf16_t* hsp = (bf16_t*)&hst[0][0];
      const bf16_t hi = clean(hv, (bf16_t*)nullptr);
      hsp[er * 8 + eu] = hi;
      hsp[128 + er * 8 + eu] = clean(hv - (float)hi, (bf16_t*)nullptr);
    } else {
      hst[er][eu] = clean(hv, (T*)nullptr);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");       // LDS write -> read inside this wave (its own 8 rows)
    __builtin_amdgcn_wave_barrier();
    // ---- publish h[t]: 16-byte write-through stores, each cell wave its own 8 rows (SPLIT: the hi and the lo piece)
    if (lane < 8 * PPC) {
      const int row = (wave - WW) * 8 + lane / PPC, pc = lane % PPC;
      if (n0 + row < p.N) {
        if constexpr (SPLIT) {
          const u32x4 x = *(const u32x4*)((const char*)&hst[0][0] + pc * 256 + row * 16);
          const unsigned off = (unsigned)(((long)(n0 + row) * p.P + p.padl + t) * xld + u0) * XSZ + pc * 16;
          __builtin_amdgcn_raw_buffer_store_b128(x, hrs, off, 0, 16);
        } else {
          const u32x4 x = *(const u32x4*)((const char*)&hst[row][0] + pc * 16);
          const unsigned off = (unsigned)(((long)(n0 + row) * p.P + p.padl + t) * p.ld_h + u0) * (unsigned)sizeof(T) + pc * 16;
          __builtin_amdgcn_raw_buffer_store_b128(x, hrs, off, 0, 16);            // aux 16 = sc1
        }
      }
    }
    if (tr && t < 256) a.trace[t * 8 + 4] = wall_clock64();
    // ---- what only later kernels read (SPLIT: the two planes, 16-byte pieces by the next 16 lanes), next step's input gates
    if constexpr (SPLIT) {
      if (lane >= 16 && lane < 32) {
        const int row = (wave - WW) * 8 + (lane - 16) / 2, pc = lane & 1;
        if (n0 + row < p.N)
          *(u32x4*)((bf16_t*)(pc ? p.h_lo_bf16 : p.h_bf16) + ((long)(n0 + row) * p.P + p.padl + t) * p.ld_h_bf16 + u0) =
              *(const u32x4*)((const char*)&hst[0][0] + pc * 256 + row * 16);
      }
    }
    if (eok) {
      const long rowi = (long)en * p.P + p.padl + t;
      if constexpr (SPLIT) ((float*)p.h)[rowi * p.ld_h + u0 + eu] = clean(hv, (float*)nullptr);     // read by later kernels only
      p.c[rowi * H + u0 + eu] = cst;
      if (p.gates) {
        T* gp = (T*)p.gates + rowi * 4 * H + u0 + eu;
        stf(gp, gi); stf(gp + H, gj); stf(gp + 2 * H, gf); stf(gp + 3 * H, go);
      }
    }
    if (t + 1 < p.T) load_xg(t + 1);
  }
}

// ===================================================================================== backward
// dh[t-1] = dgates[t] . Wh^T is a sum over the gate columns, and a workgroup (8 batch rows x UPB = 32 units) OWNS 128 of
// them (4 gates x its 32 units): as in lstm_cluster2p_bwd_kernel it forms, from its own gate gradients alone and
// straight after the cell update, its partial sum for EVERY unit of the layer - P[8, H] = dg_own[8, 128] . Wh[:, own
// columns]^T, H / 16 MFMA tiles of K = 128 - and sends each peer only the 8 x 32 block of that peer's units, as {step tag,
// 2 x bf16} granules (two rows of one unit): 128 granules per (destination, source), the data is its own flag - one
// store -> load hop per step, no probe and no second round trip.  The receiver adds the blocks in a fixed order (own
// block fp32 first, then sources in the polling order below).
//   8 product waves  : resident Wh[units of their H/128 destination tiles][own 128 columns] - 256 KB per workgroup at
//                      H = 1024, three k-steps in registers (96 VGPRs per lane), the last in LDS; per step: poll the
//                      granules of 1/8 of the sources (lane = two (unit, row pair) items), sum them, LDS -> barrier A ->
//                      (cell waves) -> barrier B -> MFMA over the operand image -> publish (the own tiles go to LDS as
//                      fp32)
//   2 cell waves     : thread = (row, two units); behind barrier A add the eight partial sums, own block and dh_out,
//                      update the cell, write the bf16 operand image, barrier B; then the stores only later kernels read
//                      and the next step's operand loads.
// What a step costs is the write-through traffic: every (row, destination unit) gets one partial sum from every SOURCE
// block, rows x H x (H / UPB) values per step chip-wide, and the fabric takes write-through stores at ~3.3 TB/s.  With
// 16-unit blocks (round 3's first form: 8 MB of granules per step at the benchmark shape, 2.4 us just to issue them)
// the step measured 4.97 us; 32-unit blocks halve the sources and with them every byte written and polled, on half the
// workgroups: 4.1 us.
// Exchange area (in work): [row group][step parity][destination][source][128 items] of 8 bytes, zeroed per launch.
constexpr int PSW = 8;                       // product waves
constexpr int PST = PSW * 64 + 128;          // + two cell waves

constexpr int UPB = 32;                      // units per workgroup
// LANES: the operand image has 8 rows and an MFMA tile 16, so half of every product is padding.  With LANES the A
// fragment of tile row r16 is read from image row r16 & 7 (an LDS broadcast, as in lstm_cluster2p_bwd_kernel): lane
// groups 2 and 3 then hold bit-identical replicas of rows 0 .. 3 and 4 .. 7, and EVERY lane converts, packs and stores
// one granule per tile (group g: row pair 2 (g & 1) + (g >> 1)) instead of groups 0 and 1 two each - 8 store
// instructions per wave and step instead of 16, on a phase that is bound by instruction issue.  Same granules, same
// addresses, same bits.  LANES = false is the form before that (NS_WIDE_LANES=0, read per call; the tests compare them).
struct WideBwdLds {                          // dynamic LDS of lstm_wide_bwd_ps_kernel<*, NT, *>
  int NT;
  static constexpr int ITEMS = UPB * 4;      // (unit, row pair) items per (destination, source) block
  static constexpr int LDW = 4 * UPB + 8;    // bf16 per row of the operand image
  LdsCarve c = {};
  int dgi = c.take<bf16_t>(16 * LDW);        // [16][LDW] the operand image, rows 8 .. 15 stay zero (LANES: unread)
  int red = c.take<float>(PSW * ITEMS * 2);  // [PSW][ITEMS][2] the polled sums
  int ownp = c.take<float>(ITEMS * 2);       // [ITEMS][2] the own block
  int abortf = c.take<int>(4);               // [4] the abort flag
  int wl = c.take<bf16x8>(PSW * NT * 64);    // [PSW * NT tiles][64 lanes] the last k-step's weight fragments
  int bytes = c.off;
};
template <typename T, int NT, bool LANES>    // NT = destination tiles per product wave = H / 128
__global__ __launch_bounds__(PST) void lstm_wide_bwd_ps_kernel(WideArgs a, u64* xbuf) {
  constexpr int TB = UPB / 16;               // 16-unit tiles per block
  constexpr int KO = 4 * UPB, KS = KO / 32;  // own gate columns, k-steps of the product
  constexpr int ITEMS = WideBwdLds::ITEMS;
  constexpr int IPL = ITEMS / 64;            // items per polling lane
  constexpr int LDW = WideBwdLds::LDW;
  constexpr int KSR = KS - 1;                // k-steps of the weights kept in registers (the last one: LDS)
  extern __shared__ __attribute__((aligned(16))) char ps_smem[];
  constexpr WideBwdLds lay{NT};
  static_assert(carve_aligned(lay.wl, 16), "the fragments are read as 16-byte vectors");
  bf16_t* dgi = carve_at<bf16_t>(ps_smem, lay.dgi); float* red = carve_at<float>(ps_smem, lay.red);
  float* ownp = carve_at<float>(ps_smem, lay.ownp); int* abortf = carve_at<int>(ps_smem, lay.abortf);
  bf16x8* wl = carve_at<bf16x8>(ps_smem, lay.wl);
  const ns_lstm_seq_params& p = a.p;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = p.H, K = 4 * H, NUB = H / UPB;
  const int rg = blockIdx.x / NUB, ub = blockIdx.x % NUB;
  const int n0 = rg * 8, u0 = ub * UPB;
  u64* xb0 = xbuf + (size_t)rg * 2 * NUB * NUB * ITEMS;
  if (tid == 0) abortf[0] = 0;
  for (int i = tid; i < 16 * LDW; i += PST) dgi[i] = (bf16_t)0.f;
  for (int i = tid; i < ITEMS * 2; i += PST) ownp[i] = 0.f;
  for (int i = tid; i < PSW * ITEMS * 2; i += PST) red[i] = 0.f;

  if (wave < PSW) {
    // ------------------------------------------------------------------ product / polling waves
    const int r16 = lane & 15, g = lane >> 4;
    const bf16_t* W = sizeof(T) == 2 ? (const bf16_t*)p.wh : (const bf16_t*)p.wh_bf16;
    // B fragments: tile j -> destination units (wave * NT + j) * 16 ..; lane (n = r16, k chunk g): own column k = 32 ks +
    // 8 g + e -> gate k / UPB, own unit k % UPB (8 consecutive units: one 16-byte load)
    bf16x8 bw[NT][KSR];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int k = 32 * ks + 8 * g;
        const bf16x8 w = *(const bf16x8*)(W + (long)((wave * NT + j) * 16 + r16) * K + (long)(k / UPB) * H + u0 + (k % UPB));
        if (ks < KSR) bw[j][ks] = w;
        else wl[(wave * NT + j) * 64 + lane] = w;
      }
    __syncthreads();
    for (int bs = 0; bs < p.T; ++bs) {
      // ---- the peers' blocks of the step before: lane = items lane, lane + 64 ..; sources wave + 8 j (fixed order)
      float s0[IPL], s1[IPL];
#pragma unroll
      for (int i = 0; i < IPL; ++i) { s0[i] = 0.f; s1[i] = 0.f; }
      wstamp(a, bs, 0);
      unsigned passes = 0;
      if (bs > 0) {
        const u64* cur = xb0 + ((size_t)(bs & 1) * NUB + ub) * NUB * ITEMS + lane;
        constexpr int NSRC = NT * 16 / UPB;            // sources per wave = NUB / PSW
        // (own loop, the give-up rule of exchange.h spelled out: through ns_poll_granules, and as its own loop around
        // ns_spin::give_up, the kernel measured slower in one of two sessions - profiles/exchange_header.txt)
        u64 v[NSRC][IPL];
        unsigned spins = 0, clk0 = 0;
        bool ok;
        do {
          ok = true;
#pragma unroll
          for (int j = 0; j < NSRC; ++j) {
            const int src = wave + PSW * j;
#pragma unroll
            for (int i = 0; i < IPL; ++i)
              v[j][i] = src == ub ? ((u64)(unsigned)bs << 32)
                                  : __hip_atomic_load((const NS_GLOBAL u64*)(cur + (size_t)src * ITEMS + 64 * i), __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT);
          }
#pragma unroll
          for (int j = 0; j < NSRC; ++j)
#pragma unroll
            for (int i = 0; i < IPL; ++i) ok = ok && ((unsigned)(v[j][i] >> 32) == (unsigned)bs);
          if (!ok && (++spins & 1023u) == 0) {   /* spins = polling passes beyond the first */
            if (__hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { ns_lds_poke(abortf, 1); ok = true; }
            else if (ns_spin_timed_out(clk0)) { atomicExch(a.status, 2); ns_lds_poke(abortf, 1); ok = true; }
          }
        } while (!ok);
        passes = spins;
#pragma unroll
        for (int j = 0; j < NSRC; ++j)
#pragma unroll
          for (int i = 0; i < IPL; ++i) {
            const unsigned pay = (unsigned)v[j][i];
            s0[i] += __uint_as_float(pay << 16);
            s1[i] += __uint_as_float(pay & 0xffff0000u);
          }
      }
      wstamp(a, bs, 1);
      if (a.trace && blockIdx.x == 0 && tid == 0 && bs < 256) a.trace[bs * 8 + 5] = passes;
      if (a.trace && blockIdx.x == 0 && tid == 7 * 64 && bs < 256) a.trace[bs * 8 + 7] = wall_clock64();      // wave 7's polls done
#pragma unroll
      for (int i = 0; i < IPL; ++i) {
        red[((wave * ITEMS) + lane + 64 * i) * 2] = s0[i];
        red[((wave * ITEMS) + lane + 64 * i) * 2 + 1] = s1[i];
      }
      ns_lds_barrier();                          // A: the partial sums are in LDS
      wstamp(a, bs, 2);
      if (abortf[0]) return;
      ns_lds_barrier();                          // B: the operand image of this step is complete
      wstamp(a, bs, 3);
      if (bs + 1 < p.T) {
        bf16x8 af[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) af[ks] = *(const bf16x8*)(dgi + (LANES ? (r16 & 7) : r16) * LDW + 32 * ks + 8 * g);
        u64* nxt = xb0 + (size_t)((bs + 1) & 1) * NUB * NUB * ITEMS;
        // four tiles at a time, k-step outermost: four independent accumulator chains keep the matrix pipe issuing
        // (one tile after the other is a chain of KS dependent MFMAs each), and the first group's stores go out under
        // the second group's products
        constexpr int TG = NT < 4 ? NT : 4;
#pragma unroll
        for (int j0 = 0; j0 < NT; j0 += TG) {
          f32x4 acc[TG];
#pragma unroll
          for (int jj = 0; jj < TG; ++jj) acc[jj] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int jj = 0; jj < TG; ++jj)
              acc[jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], ks < KSR ? bw[j0 + jj][ks < KSR ? ks : 0] : wl[(wave * NT + j0 + jj) * 64 + lane],
                                                                acc[jj], 0, 0, 0);
#pragma unroll
          for (int jj = 0; jj < TG; ++jj) {
            // D: column r16 = unit of the destination tile, rows 4 g + q (rows 0 .. 7 are this workgroup's):
            // item = unit in the destination block + UPB * (row pair)
            const int tile = wave * NT + j0 + jj, dest = tile / TB, ui = (tile % TB) * 16 + r16;
            auto granule = [&](float x0, float x1) {
              const bf16_t b0 = (bf16_t)x0, b1 = (bf16_t)x1;
              return ns_granule((unsigned)(bs + 1), (unsigned)__builtin_bit_cast(unsigned short, b0) | ((unsigned)__builtin_bit_cast(unsigned short, b1) << 16));
            };
            if constexpr (LANES) {
              // rows 4 g + q of D replicate rows 4 (g & 1) + q: this lane takes the pair q = 2 hf, 2 hf + 1 (selects, no
              // dynamic register index) = row pair 2 (g & 1) + hf
              const int gp = g & 1, hf = g >> 1;
              const float x0 = hf ? acc[jj][2] : acc[jj][0], x1 = hf ? acc[jj][3] : acc[jj][1];
              const int item = ui + UPB * (2 * gp + hf);
              if (dest == ub) {
                ownp[item * 2] = x0; ownp[item * 2 + 1] = x1;
              } else {
                ns_put_granule(nxt + ((size_t)dest * NUB + ub) * ITEMS + item, granule(x0, x1));
              }
            } else if (g < 2) {
              if (dest == ub) {
                ownp[(ui + UPB * (2 * g)) * 2] = acc[jj][0]; ownp[(ui + UPB * (2 * g)) * 2 + 1] = acc[jj][1];
                ownp[(ui + UPB * (2 * g + 1)) * 2] = acc[jj][2]; ownp[(ui + UPB * (2 * g + 1)) * 2 + 1] = acc[jj][3];
              } else {
                u64* dst = nxt + ((size_t)dest * NUB + ub) * ITEMS + ui + 2 * UPB * g;
                ns_put_granule(dst, granule(acc[jj][0], acc[jj][1]));
                ns_put_granule(dst + UPB, granule(acc[jj][2], acc[jj][3]));
              }
            }
          }
        }
      }
      wstamp(a, bs, 4);
    }
    return;
  }
  // -------------------------------------------------------------------- cell waves: thread = (row er, units eu + 16 c)
  __syncthreads();                           // pairs with the product waves' barrier behind their weight loads
  const int e = tid - PSW * 64, er = e >> 4, eu = e & 15;
  const int en = n0 + er;
  const bool eok = en < p.N;
  const int elen = (eok && p.lengths) ? p.lengths[en] : p.T;
  const int half = er & 1;
  float dcc[TB], dhc[TB];
  const bool zone = p.zoneout_thr_cell != 0u || p.zoneout_thr_output != 0u;
  float pg[TB][4], pdh[TB], pc[TB], pcp[TB];
#pragma unroll
  for (int c = 0; c < TB; ++c) { dcc[c] = 0.f; dhc[c] = 0.f; pdh[c] = 0.f; pc[c] = 0.f; pcp[c] = 0.f; pg[c][0] = pg[c][1] = pg[c][2] = pg[c][3] = 0.f; }
  auto load_ops = [&](int t) {
    if (eok) {
      const long rowi = (long)en * p.P + p.padl + t;
#pragma unroll
      for (int c = 0; c < TB; ++c) {
        const int u = u0 + eu + 16 * c;
        const T* gp = (const T*)p.gates + rowi * 4 * H + u;
#pragma unroll
        for (int j = 0; j < 4; ++j) pg[c][j] = ldf(gp + (long)j * H);
        pdh[c] = p.dh[rowi * p.ld_dh + u];
        pc[c] = p.c[rowi * H + u];
        pcp[c] = t > 0 ? p.c[(rowi - 1) * H + u] : 0.f;
      }
    }
  };
  load_ops(p.T - 1);
  for (int t = p.T - 1; t >= 0; --t) {
    if (a.trace && blockIdx.x == 0 && e == 0 && p.T - 1 - t < 256) a.trace[(p.T - 1 - t) * 8 + 6] = wall_clock64();      // a cell wave reaches A
    ns_lds_barrier();                            // A
    if (abortf[0]) return;
    float dgv[TB][4];
#pragma unroll
    for (int c = 0; c < TB; ++c) {
      const int item = eu + 16 * c + UPB * (er >> 1);
      float dh = pdh[c] + ownp[item * 2 + half];
#pragma unroll
      for (int w = 0; w < PSW; ++w) dh += red[(w * ITEMS + item) * 2 + half];
      const float gi = pg[c][0], gj = pg[c][1], gf = pg[c][2], go = pg[c][3];
      float cc = pc[c], dcin = dcc[c], dckeep = 0.f;
      if (zone) {             // the gradient of the forward kernel's masks (include/nspeech_hip.h, ns_lstm_seq_params)
        const uint32_t uu = (uint32_t)(u0 + eu + 16 * c);
        dh += dhc[c];
        const bool mh = ns_zone_keep(p.zoneout_seed_output, (uint32_t)t, (uint32_t)en, uu, p.zoneout_thr_output);
        const bool mc = ns_zone_keep(p.zoneout_seed_cell, (uint32_t)t, (uint32_t)en, uu, p.zoneout_thr_cell);
        dhc[c] = mh ? dh : 0.f;
        if (mh) dh = 0.f;
        if (mc) { dckeep = dcin; dcin = 0.f; }
        cc = ns_cell_clip(gf * pcp[c] + gi * gj, p.cell_clip);      // the forward kernel's c': h' was o tanh of the clipped value
      }
      const float tc = tanhf_(cc);
      const float dc = dh * go * (1.f - tc * tc) + dcin;
      dgv[c][0] = dc * gj * gi * (1.f - gi);
      dgv[c][1] = dc * gi * (1.f - gj * gj);
      dgv[c][2] = dc * pcp[c] * gf * (1.f - gf);
      dgv[c][3] = dh * tc * go * (1.f - go);
      dcc[c] = dc * gf + dckeep;
      if (t >= elen || !eok) { dgv[c][0] = dgv[c][1] = dgv[c][2] = dgv[c][3] = 0.f; dcc[c] = 0.f; dhc[c] = 0.f; }
#pragma unroll
      for (int j = 0; j < 4; ++j) dgi[er * LDW + j * UPB + eu + 16 * c] = (bf16_t)dgv[c][j];
    }
    ns_lds_barrier();                            // B
    // ---- what only later kernels read: the gate gradients (bf16 copy and, for fp32 storage, fp32), next operands
    if (eok) {
      const long rowi = (long)en * p.P + p.padl + t;
      bf16_t* xb = sizeof(T) == 2 ? (bf16_t*)p.dgates : (bf16_t*)p.dgates_bf16;
#pragma unroll
      for (int c = 0; c < TB; ++c) {
        bf16_t* db = xb + rowi * K + u0 + eu + 16 * c;
#pragma unroll
        for (int j = 0; j < 4; ++j) db[(long)j * H] = (bf16_t)dgv[c][j];
        if (sizeof(T) == 4) {
          float* dg = (float*)p.dgates + rowi * K + u0 + eu + 16 * c;
#pragma unroll
          for (int j = 0; j < 4; ++j) dg[(long)j * H] = dgv[c][j];
        }
      }
    }
    if (t > 0) load_ops(t - 1);
  }
}

// What both calls accept.  The set is part of the interface (the model picks its path by it, the tests pin it down):
// a condition stays even where the kernel that runs today would take more.
bool wide_shape_ok(const ns_lstm_seq_params* p, int backward) {
  if (!p || p->reverse || p->T < 2) return false;
  const int H = p->H;
  if (H != 256 && H != 512 && H != 1024) return false;
  // One workgroup per CU, all resident at once.  Forward: 16-row groups x H/8 unit blocks, the grid itself.  Backward:
  // 16-row groups x H/16 is the grid of round 2's kernel; the partial-sum kernel launches ceil(N/8) x H/32 <= 2 ceil(N/16)
  // x H/32, so every shape within the bound fits (on 256 CUs the two bounds admit exactly the same N)
  if ((p->N + 15) / 16 * (backward ? H / 16 : H / 8) > ns_device_cus()) return false;
  auto al16 = [](const void* q) { return (((uintptr_t)q) & 15) == 0; };
  const long esz = p->dtype == NS_BF16 ? 2 : 4;
  if (!backward) {
    if (p->dtype == NS_F32 && !(p->f32_passes == 3 && p->whT_hi && p->whT_lo)) return false;
    if (p->dtype == NS_BF16 && !p->whT) return false;
    if (!p->xg || !p->h || !p->c || !al16(p->h) || (p->ld_h * esz) % 16 != 0) return false;
    if ((double)p->N * p->P * p->ld_h * esz >= 2.0e9) return false;       // h is addressed through a buffer resource
  } else {
    if (p->dtype == NS_F32 && !(p->f32_passes == 1 && p->wh_bf16 && p->dgates_bf16)) return false;
    if (p->dtype == NS_BF16 && !p->wh) return false;
    if (!p->gates || !p->c || !p->dh || !p->dgates) return false;
    // the bf16 gate gradients: 16-byte aligned and below 2e9 bytes, as round 2's kernel (which exchanged them through a
    // buffer resource) required; the partial-sum kernel writes them with plain stores and needs neither
    if (!al16(p->dtype == NS_BF16 ? p->dgates : p->dgates_bf16)) return false;
    if ((double)p->N * p->P * 4 * H * 2 >= 2.0e9) return false;
  }
  return true;
}

// the backward kernel's exchange area: [8-row group][step parity][destination][source][UPB * 4 items] granules
size_t ps_exchange_bytes(const ns_lstm_seq_params* p) {
  const size_t nb = p->H / UPB;
  return (size_t)((p->N + 7) / 8) * 2 * nb * nb * (UPB * 4) * sizeof(u64);
}
}  // namespace

extern "C" int ns_lstm_wide_supported(const ns_lstm_seq_params* p, int backward) { return wide_shape_ok(p, backward) ? 1 : 0; }
// The work area.  The call is not told the direction, so the one layout holds what either takes.  Two arrays are placed
// by the ADDRESS, not the offset: xbuf at the next 16-byte boundary from its offset, xch at the next 256-byte one
// (wide_at), and the slack in front of each pays for that.
struct WideWork {
  size_t xbuf_bytes, xch_bytes;
  WorkCarve c = {};
  size_t status = c.take<char>(256);                 // the status word in a block of its own: what a launch clears
  size_t trace = c.take<char>(WIDE_TRACE_BYTES);     // the NS_WIDE_TRACE timestamps
  size_t xbuf = c.take<char>(xbuf_bytes);            // the backward kernel's exchange area (ps_exchange_bytes), cleared per launch
  size_t xbuf_slack = c.take<char>(64);              // room for xbuf's rounding (15 bytes would do)
  size_t xch_slack = c.take<char>(xch_bytes ? 256 : 0);   // room for xch's rounding
  size_t xch = c.take<char>(xch_bytes);              // the split forward form's exchange array: [N * P][H] (hi, lo) pairs
  size_t bytes = c.off;
};
static WideWork wide_work(const ns_lstm_seq_params* p) {
  // the exchange area for every shape ns_lstm_wide_bwd can take; the pairs with both planes given (the split forward form)
  const bool bwd_fits = (p->H == 256 || p->H == 512 || p->H == 1024) && (p->N + 15) / 16 * (p->H / 16) <= ns_device_cus();
  return WideWork{bwd_fits ? ps_exchange_bytes(p) : 0, (p->h_bf16 && p->h_lo_bf16) ? (size_t)p->N * p->P * p->H * 4 : 0};
}
static void* wide_at(void* work, size_t off, uintptr_t align) { return (void*)(((uintptr_t)work + off + align - 1) & ~(align - 1)); }
extern "C" size_t ns_lstm_wide_work_bytes(const ns_lstm_seq_params* p) {
  if (!p) return 0;
  return wide_work(p).bytes;
}

template <typename T, int PASSES, bool SPLIT>
static int launch_wide_fwd(const WideArgs& a, int grid, hipStream_t s) {
  switch (a.p.H) {
    case 256: hipLaunchKernelGGL((lstm_wide_fwd_kernel<T, PASSES, 1, SPLIT>), dim3(grid), dim3(WTF), 0, s, a); break;
    case 512: hipLaunchKernelGGL((lstm_wide_fwd_kernel<T, PASSES, 2, SPLIT>), dim3(grid), dim3(WTF), 0, s, a); break;
    default: hipLaunchKernelGGL((lstm_wide_fwd_kernel<T, PASSES, 4, SPLIT>), dim3(grid), dim3(WTF), 0, s, a); break;
  }
  NS_CHECK_LAUNCH("lstm_wide_fwd");
  return NS_OK;
}

// Whole-sequence forward recurrence of one wide LSTM cell, one launch (see the header of this file).  Same parameter
// block and outputs as ns_lstm_seq_fwd.  work: ns_lstm_wide_work_bytes(); work[0] (int) is a status word, non-zero
// after the call completes = a wait timed out and the outputs are invalid (h may then hold the sentinel; in the
// split form h and the planes are then incomplete).  With fp32 storage and both h_bf16 and h_lo_bf16 the call takes the
// split form: it also writes hi = bf16(h) and lo = bf16(h - hi) there (leading dimension ld_h_bf16) and exchanges h
// as those pairs through an array of its own in work.
extern "C" int ns_lstm_wide_fwd(const ns_lstm_seq_params* p, void* work, ns_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  NS_CHECK_ARG(p && work, "ns_lstm_wide_fwd: null");
  NS_CHECK_ARG(!p->h_lo_bf16 || p->h_bf16, "ns_lstm_wide_fwd: h_lo_bf16 without h_bf16 (the lo plane goes with the hi plane)");
  const bool split = p->dtype == NS_F32 && p->f32_passes == 3 && p->h_bf16 && p->h_lo_bf16;
  NS_CHECK_ARG(wide_shape_ok(p, 0), "ns_lstm_wide_fwd: unsupported (needs H in {256, 512, 1024}, row groups x H/8 <= 256, "
               "fp32 with pre-split whT_hi / whT_lo and f32_passes 3, or bf16)");
  if (split) {
    NS_CHECK_ARG(p->ld_h_bf16 >= p->H && p->ld_h_bf16 % 8 == 0 && ((uintptr_t)p->h_bf16 & 15) == 0 && ((uintptr_t)p->h_lo_bf16 & 15) == 0,
                 "ns_lstm_wide_fwd: h_bf16 / h_lo_bf16 need 16-byte alignment and ld_h_bf16 %% 8 == 0, >= H");
    NS_CHECK_ARG((double)p->N * p->P * p->H * 4 < 2.0e9, "ns_lstm_wide_fwd: exchange array beyond a buffer resource");
  }
  WideArgs a;
  const WideWork wl = wide_work(p);
  a.p = *p; a.status = carve_at<int>(work, wl.status); a.nub = p->H / 8;
  a.xch = split ? wide_at(work, wl.xch_slack, 256) : nullptr;
  a.trace = getenv("NS_WIDE_TRACE") ? carve_at<long long>(work, wl.trace) : nullptr;
  int rc = ns_zero_async(work, wl.trace, s);
  if (rc) return rc;
  const int grid = ((p->N + 15) / 16) * a.nub;
  if (p->dtype == NS_BF16) {
    hipLaunchKernelGGL(wide_fill_kernel<bf16_t>, dim3(512), dim3(256), 0, s, (bf16_t*)p->h, p->N, (long)p->P, p->padl, p->T, (long)p->ld_h, p->H);
    NS_CHECK_LAUNCH("lstm_wide_fill");
    return launch_wide_fwd<bf16_t, 1, false>(a, grid, s);
  }
  if (split) {               // the exchange array carries the sentinel (the same bytes as the fp32 fill); h is not filled
    hipLaunchKernelGGL(wide_fill_kernel<float>, dim3(512), dim3(256), 0, s, (float*)a.xch, p->N, (long)p->P, p->padl, p->T, (long)p->H, p->H);
    NS_CHECK_LAUNCH("lstm_wide_fill");
    return launch_wide_fwd<float, 3, true>(a, grid, s);
  }
  hipLaunchKernelGGL(wide_fill_kernel<float>, dim3(512), dim3(256), 0, s, (float*)p->h, p->N, (long)p->P, p->padl, p->T, (long)p->ld_h, p->H);
  NS_CHECK_LAUNCH("lstm_wide_fill");
  return launch_wide_fwd<float, 3, false>(a, grid, s);
}

// The instantiations of the backward kernel, [all-lane publish off, on][storage type bf16, fp32][H / 128 = 2, 4, 8]
typedef void (*wide_bwd_kernel_t)(WideArgs, u64*);
#define NS_WIDE_BWD_FORMS(T_, L_) {lstm_wide_bwd_ps_kernel<T_, 2, L_>, lstm_wide_bwd_ps_kernel<T_, 4, L_>, lstm_wide_bwd_ps_kernel<T_, 8, L_>}
static const wide_bwd_kernel_t wide_bwd_forms[2][2][3] = {{NS_WIDE_BWD_FORMS(bf16_t, false), NS_WIDE_BWD_FORMS(float, false)},
                                                          {NS_WIDE_BWD_FORMS(bf16_t, true), NS_WIDE_BWD_FORMS(float, true)}};
#undef NS_WIDE_BWD_FORMS

// Whole-sequence backward recurrence (the gate gradients of every step), one launch.  Same parameter block and outputs
// as ns_lstm_seq_bwd; with fp32 storage dgates_bf16 receives the bf16 copy as well.  work as for ns_lstm_wide_fwd.
extern "C" int ns_lstm_wide_bwd(const ns_lstm_seq_params* p, void* work, ns_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  NS_CHECK_ARG(p && work, "ns_lstm_wide_bwd: null");
  NS_CHECK_ARG(wide_shape_ok(p, 1), "ns_lstm_wide_bwd: unsupported (needs H in {256, 512, 1024}, row groups x H/16 <= 256, "
               "bf16, or fp32 with wh_bf16 + dgates_bf16 and f32_passes 1)");
  WideArgs a;
  const WideWork wl = wide_work(p);
  a.p = *p; a.status = carve_at<int>(work, wl.status); a.nub = 0; a.xch = nullptr;
  a.trace = getenv("NS_WIDE_TRACE") ? carve_at<long long>(work, wl.trace) : nullptr;
  int rc = ns_zero_async(work, wl.trace, s);
  if (rc) return rc;
  u64* xbuf = (u64*)wide_at(work, wl.xbuf, 16);
  rc = ns_zero_async(xbuf, ps_exchange_bytes(p), s);
  if (rc) return rc;
  const int grid = (p->N + 7) / 8 * (p->H / UPB);      // 8-row groups x unit blocks, one workgroup per CU
  const int nt = p->H / 128;
  const size_t ldsb = WideBwdLds{nt}.bytes;
  static bool attr = false;
  if (!attr) {
    for (const auto& lanes : wide_bwd_forms)
      for (const auto& widths : lanes)
        for (wide_bwd_kernel_t k : widths) (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  const char* le = getenv("NS_WIDE_LANES");           // "0": the publish by lane groups 0 and 1 only (the form before)
  const int lanes = (le && le[0] == '0' && !le[1]) ? 0 : 1;
  hipLaunchKernelGGL(wide_bwd_forms[lanes][p->dtype == NS_BF16 ? 0 : 1][nt == 2 ? 0 : nt == 4 ? 1 : 2], dim3(grid), dim3(PST), ldsb, s, a, xbuf);
  NS_CHECK_LAUNCH("lstm_wide_bwd_ps");
  return NS_OK;
}
