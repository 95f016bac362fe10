// Tacotron-1 attention RNN (decoder prenet layer 2 -> GRU(256) attention cell -> query -> Bahdanau energies -> softmax ->
// next step's prenet layer 1) as ONE persistent launch per direction instead of ~9 (forward) / ~16 (backward) dependent
// launches per decoder step (tacotron.py:64-76, modules.py:76-102, rnn_wrappers.py:25-31 under teacher forcing).
//
// Same arrangement as attn_cluster.hip (the Tacotron-2 counterpart): every operation of the chain is independent per
// utterance and its weights are stationary (0.39 M values), so an utterance gets a CLUSTER of 8 workgroups (one per CU,
// 512 threads) that keeps everything on chip for the whole sequence - the weights in REGISTERS as fp32 (one utterance
// per cluster makes every product matrix-VECTOR: exact fp32 FMAs), the utterance's keys and projected memory
// (pv = values . W1c) in LDS:
//   workgroup g owns  * GRU units [32 g, 32 g + 32): the r, u columns of gates/kernel and the columns of candidate/kernel
//                       of those units, all K = 128 + 256 input rows
//                     * the rows of W_query that belong to those units
//                     * all of W_prenet2 (every workgroup computes the whole p2: cheaper than another exchange)
//                     * memory positions [g ts, (g + 1) ts), ts = ceil(length / 8): keys and pv rows
// A GRU step has TWO dependent products (the candidate needs r * h of EVERY unit), so the forward step takes three
// exchanges inside the cluster where the LSTM cell of Tacotron-2 takes two ({step tag, fp32} granules: exchange.h; the
// protocol is DESIGN.md, "The tagged-granule exchange"):
//   X1: r * h(s-1) of the own units                                                -> every workgroup has r * h
//   X2: partial queries h_own . Wq[own rows, :] (256 values) + the new h of the own units   -> q, h
//   X3: partial next-prenet sums  sum_t w[t] pv[t, :] (256) + local softmax max / sum + the local weights
//       (combined flash-attention style)                                           -> p1[s+1], the alignment
// Backward mirrors it with four: the softmax-backward dot-product share (E1, hidden behind the energy pass), partial
// query gradients (E2), partial input gradients of the candidate kernel (E3a: they carry d(r * h)), then of the gate
// kernel (E3b).  One buffer per exchange suffices: a workgroup publishes exchange X of step s+1 only after it has gathered
// the last exchange of step s from every peer, and a peer publishes that only after it has gathered X of step s.
// On a time-out the status word is raised and every workgroup of the cluster leaves.  History is written in the
// layouts models/tacotron.py reads (the launch-per-step form stays as the fallback).
#include "exchange.h"
#include "carve.h"
#include <stdlib.h>

namespace {
constexpr int CG = 8;              // workgroups per utterance
constexpr int CT = 512;            // threads per workgroup
constexpr int TSMAX = 32;          // memory positions per workgroup (T_in <= 256)
constexpr int KPAD = 4;            // row pad of the keys image (16 rows x one bank otherwise)
constexpr int A = 256, D1 = 256, D2 = 128;
constexpr int UPW = A / CG;        // 32 GRU units per workgroup
constexpr int K = D2 + A;          // input rows of both GRU kernels
// forward thread maps
constexpr int P2G = CT / D2, P2K = D1 / P2G;             // prenet 2: 4 k groups x 64
constexpr int GC = 2 * UPW, GG = CT / GC;                // gates: 64 columns (r | u of the own units), 8 k groups
constexpr int GKP = D2 / GG, GKH = A / GG;               //   16 prenet rows + 32 h rows per thread
constexpr int CGG = CT / UPW;                            // candidate: 32 columns, 16 k groups
constexpr int CKP = D2 / CGG, CKH = A / CGG;             //   8 prenet rows + 16 r*h rows per thread
constexpr int QG = CT / A, QK = UPW / QG;                // query partials: 2 groups x 16 own rows
constexpr int CXG = CT / D1;                             // context t-groups
constexpr int X1N = UPW, X2N = A + UPW, X3N = D1 + 2 + TSMAX;
constexpr int XMAX = X3N;
// backward
constexpr int NQ = 4;                                    // column groups of the input-gradient products
constexpr int PPT = NQ * K / CT;                         // (row, group) pairs per thread: 3
constexpr int CPQ_C = UPW / NQ, CPQ_G = GC / NQ;         // columns per group: candidate 8, gates 16
constexpr int W2H = CT / D1, W2K = D2 / W2H;             // dp1 product: 2 halves x 64
// free-running synthesis: decoder workgroups (see "free-running synthesis" below)
constexpr int DD = 256;                                  // decoder width D
constexpr int DU = 16;                                   // decoder units per decoder workgroup
constexpr int DNW = DD / DU;                             // decoder workgroups per group: 16
constexpr int DNR = 2;                                   // utterances per group of decoder workgroups
static_assert(NQ * K == PPT * CT && P2K == 64 && GKP + GKH == 48 && CKP + CKH == 24, "shape");

struct TArgs {
  ns_taco1_attn_params p;
  u64* x1; u64* x2; u64* x3; u64* x4;       // fwd: [N][CG][X1N | X2N | X3N]; bwd: E1 [N][CG], E2 [N][CG][A], E3a / E3b [N][CG][K]
  int* status;
  int xcd;                   // the forward / backward kernels: an utterance's cluster shares an XCD (ns_cluster_place;
                             // NS_CLUSTER_XCD, family "taco1attn"); the decode kernel deals its own roles and ignores it
  // free-running synthesis (taco1_decode_kernel): the next step's frame term arrives as nwd partial sums per column
  // ([N][nwd][D1] granules, plus bpf), the alignment goes out as [N][Tia] granules
  u64* f1x; u64* alx; const float* bpf; int nwd;
};
// Prenet dropout (ns_taco1_attn_params.drop_*, ns_prenet_drop): taco1_run issues ONE launch for the whole batch (it needs
// N * 8 <= CUs and never groups the utterances), so the cluster index n of the kernels below IS the row of the batch.

// The partial sums of one frame-term column from the nw decoder workgroups (stride D1), polled by its owner thread and
// added in a fixed order.  Returns false on time-out / raised status.
template <int NW>
__device__ __forceinline__ bool poll_partials(const u64* src, unsigned tag, float& out, int* status, int code) {
  u64 v[NW];
  ns_spin sp;
  if (!ns_poll_granules(v, tag, sp, status, code, [&](int j) { return ns_ld_granule(src + (size_t)j * D1); })) return false;
#pragma unroll
  for (int j = 0; j < NW; ++j) out += ns_granule_value(v[j]);
  return true;
}

// ===================================================================================== forward
// One workgroup of an utterance's cluster (bid = utterance * CG + member).  INFER = free-running synthesis: the frame
// term of the next step is not hoisted (it depends on this step's output through the decoder GRUs) but polled from
// a.f1x, and the alignment is published to a.alx for the decoder workgroups (attn_cluster.hip: attn_fwd_body<INFER>).
struct FwdLds {                            // dynamic LDS of attn_fwd_body (the forward kernel, the decode kernel's clusters)
  LdsCarve c = {};
  int xs = c.take<float>(K);               // [K]      p2 | h(s-1)
  int p1s = c.take<float>(D1);             // [D1]     prenet layer 1 of the current step
  int red = c.take<float>(CT);             // [CT]     partial sums across the k / t groups of a product
  int rus = c.take<float>(GC);             // [GC]     r | u of the own units
  int hloc = c.take<float>(UPW);           // [UPW]    h of the own units
  int es = c.take<float>(TSMAX);           // [TSMAX]  local unnormalised softmax weights
  int ered = c.take<float>(8 * TSMAX);     // [8][TSMAX] per-wave energy sums
  int sc = c.take<float>(16);              // [16]     [0] local max, [1] local sum, [2] abort flag
  int gath = c.take<float>(CG * XMAX);     // [CG][XMAX]
  int vs = c.take<float>(A);               // [A]      attention_v
  int keys_s = c.take<float>(TSMAX * (A + KPAD));   // [TSMAX][A + KPAD]
  int pv_s = c.take<float>(TSMAX * D1);    // [TSMAX][D1]
  int wq_s = c.take<float>(UPW * A);       // [UPW][A]  W_query rows of the own units
  int bytes = c.off;
};
// DROP = prenet dropout (drop_thr != 0), an instantiation of its own: see attn_cluster.hip, attn_fwd_body
template <typename T, bool INFER, bool DROP = false>
__device__ __forceinline__ void attn_fwd_body(const TArgs& a, float* sm, const int bid) {
  const ns_taco1_attn_params& p = a.p;
  constexpr FwdLds lay;
  float* xs = carve_at<float>(sm, lay.xs); float* p1s = carve_at<float>(sm, lay.p1s); float* red = carve_at<float>(sm, lay.red);
  float* rus = carve_at<float>(sm, lay.rus); float* hloc = carve_at<float>(sm, lay.hloc);
  float* es = carve_at<float>(sm, lay.es); float* ered = carve_at<float>(sm, lay.ered); float* sc = carve_at<float>(sm, lay.sc);
  float* gath = carve_at<float>(sm, lay.gath); float* vs = carve_at<float>(sm, lay.vs);
  float* keys_s = carve_at<float>(sm, lay.keys_s); float* pv_s = carve_at<float>(sm, lay.pv_s);
  float* wq_s = carve_at<float>(sm, lay.wq_s);

  const int tid_ = threadIdx.x;
  const int n = bid / CG, g = bid % CG;
  const long S1 = p.S + 1;
  const int HC = A + p.E;
  // multi-speaker (rnn_wrappers.py:28-30): the GRU's input row is [p2 | speaker projection (Dsp) | h]; the projection is
  // the same in every step, so its products with the Dsp kernel rows join the biases and the loop never sees it
  const int Dsp = p.Dsp, XA = D2 + Dsp + A;
  const int L = min(p.lengths ? p.lengths[n] : p.Ti, p.Ti);
  const int ts = max(1, (L + CG - 1) / CG);
  const int t0 = g * ts, tn = max(0, min(L, t0 + ts) - t0);
  u64* x1 = a.x1 + (size_t)n * CG * X1N;
  u64* x2 = a.x2 + (size_t)n * CG * X2N;
  u64* x3 = a.x3 + (size_t)n * CG * X3N;
  if (tid_ == 0) sc[2] = 0.f;

  // ---------------------------------------------------------------- resident weights (registers)
  const T* W2 = (const T*)p.w2;            // [D1][D2]
  const T* Wg = (const T*)p.wg;            // [K][2A]
  const T* Wc = (const T*)p.wc;            // [K][A]
  const T* Wq = (const T*)p.wq;            // [A][A]
  const int tid = tid_;
  float w2r[P2K];
  {
    const T* b = W2 + (long)((tid / D2) * P2K) * D2 + tid % D2;
#pragma unroll
    for (int i = 0; i < P2K; ++i) w2r[i] = ldf(b + i * D2);
  }
  const int gc = tid % GC;
  const int gcol = gc < UPW ? g * UPW + gc : A + g * UPW + (gc - UPW);
  float wgp[GKP], wgh[GKH];
  {
    const T* bp = Wg + (long)((tid / GC) * GKP) * 2 * A + gcol;
    const T* bh = Wg + (long)(D2 + Dsp + (tid / GC) * GKH) * 2 * A + gcol;
#pragma unroll
    for (int i = 0; i < GKP; ++i) wgp[i] = ldf(bp + i * 2 * A);
#pragma unroll
    for (int i = 0; i < GKH; ++i) wgh[i] = ldf(bh + i * 2 * A);
  }
  float wcp[CKP], wch[CKH];
  {
    const int ccol = g * UPW + tid % UPW;
    const T* bp = Wc + (long)((tid / UPW) * CKP) * A + ccol;
    const T* bh = Wc + (long)(D2 + Dsp + (tid / UPW) * CKH) * A + ccol;
#pragma unroll
    for (int i = 0; i < CKP; ++i) wcp[i] = ldf(bp + i * A);
#pragma unroll
    for (int i = 0; i < CKH; ++i) wch[i] = ldf(bh + i * A);
  }
  for (int i = tid; i < UPW * A; i += CT) wq_s[i] = ldf(Wq + (long)g * UPW * A + i);
  for (int i = tid; i < A; i += CT) vs[i] = p.v[i];
  float gbias = tid < GC ? p.bg[gcol] : 0.f;
  float cbias = tid < UPW ? p.bc[g * UPW + tid] : 0.f;
  if (Dsp) {
    const T* spk = (const T*)p.xa + ((long)n * S1 + 1) * XA + D2;       // written into every slot by the caller
    for (int k = 0; k < Dsp; ++k) {
      const float sk = ldf(spk + k);
      if (tid < GC) gbias = fmaf(sk, ldf(Wg + (long)(D2 + k) * 2 * A + gcol), gbias);
      if (tid < UPW) cbias = fmaf(sk, ldf(Wc + (long)(D2 + k) * A + g * UPW + tid), cbias);
    }
  }
  const float b2c = tid < D2 ? p.b2[tid] : 0.f;
  float hpart = 0.f;                       // h(s-1) . Wg[h rows of this k group]: h(-1) = 0

  // ---------------------------------------------------------------- per-utterance LDS images
  {
    const float* kn = p.keys + ((long)n * p.Pi + p.padl_i + t0) * A;
    for (int i = tid; i < TSMAX * A; i += CT) keys_s[(i / A) * (A + KPAD) + i % A] = (i / A) < tn ? kn[i] : 0.f;
    const T* pvn = (const T*)p.pv + ((long)n * p.Pi + p.padl_i + t0) * D1;
    for (int i = tid; i < TSMAX * D1; i += CT) pv_s[i] = (i / D1) < tn ? ldf(pvn + i) : 0.f;
    for (int i = tid; i < K; i += CT) xs[i] = 0.f;
    if (tid < UPW) hloc[tid] = 0.f;
    if (tid < D1) {                                                                // the context before the first step is 0
      float v = fmaxf(p.f1[((long)n * S1 + 1) * D1 + tid], 0.f);
      if constexpr (DROP) v = ns_prenet_drop(v, p.drop_seed1, 0, n, tid, p.drop_thr, p.drop_scale);
      p1s[tid] = v;
      if (tid / (D1 / CG) == g) stf((T*)p.p1 + ((long)n * S1 + 1) * D1 + tid, v);
    }
  }
  __syncthreads();

  for (int st = 0; st < p.S; ++st) {
    const long slot = st + 1;
    const long rowS = (long)n * S1 + slot;
    const unsigned tag = (unsigned)(st + 1);
    int tid = tid_;
    asm volatile("" : "+v"(tid));           // opaque per iteration: addresses are recomputed in the loop, not hoisted as 64-bit pairs
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float f1n = 0.f;
    if (!INFER && tid < D1 && st + 1 < p.S) f1n = p.f1[(rowS + 1) * D1 + tid];

    // ---- (1) p2 = relu(p1 . W2 + b2): every workgroup computes all of it
    red[tid] = dot_regs<P2K>(w2r, p1s + (tid / D2) * P2K);
    ns_lds_barrier();
    if (tid < D2) {
      float s = b2c;
#pragma unroll
      for (int q = 0; q < P2G; ++q) s += red[q * D2 + tid];
      s = fmaxf(s, 0.f);
      if constexpr (DROP) s = ns_prenet_drop(s, p.drop_seed2, st, n, tid, p.drop_thr, p.drop_scale);
      xs[tid] = s;
      if (tid / (D2 / CG) == g) {
        stf((T*)p.xa + rowS * XA + tid, s);
        stf((T*)p.xc + rowS * XA + tid, s);
      }
    }
    ns_lds_barrier();
    // ---- (2) r, u of the own units; r * h(s-1) goes out (X1); the candidate's prenet rows meanwhile
    red[tid] = hpart + dot_regs<GKP>(wgp, xs + (tid / GC) * GKP);
    const float cpart = dot_regs<CKP>(wcp, xs + (tid / UPW) * CKP);
    ns_lds_barrier();
    float sv_r = 0.f, sv_u = 0.f, sv_rh = 0.f;
    if (tid < GC) {
      float z = gbias;
#pragma unroll
      for (int q = 0; q < GG; ++q) z += red[q * GC + tid];
      const float v = sigmoidf_(z);
      rus[tid] = v;
      if (tid < UPW) {
        sv_r = v;
        sv_rh = v * hloc[tid];
        ns_put_granule(x1 + (size_t)g * X1N + tid, tag, sv_rh);
      }
    }
    // ---- (3) gather X1: r * h of every unit (granule index = unit)
    if (!ns_gather_granules<1, CT>(x1, CG * X1N, tag, gath, tid, a.status, 1)) sc[2] = 1.f;
    ns_lds_barrier();
    if (sc[2] != 0.f) return;
    // ---- (4) candidate of the own units, the new h; h goes out with the partial queries (X2)
    red[tid] = cpart + dot_regs<CKH>(wch, gath + (tid / UPW) * CKH);
    ns_lds_barrier();
    float sv_c = 0.f, sv_h = 0.f;
    if (tid < UPW) {
      float z = cbias;
#pragma unroll
      for (int q = 0; q < CGG; ++q) z += red[q * UPW + tid];
      sv_c = tanhf_(z);
      sv_u = rus[UPW + tid];
      sv_h = sv_u * hloc[tid] + (1.f - sv_u) * sv_c;
      hloc[tid] = sv_h;
      ns_put_granule(x2 + (size_t)g * X2N + A + tid, tag, sv_h);
    }
    ns_lds_barrier();
    {
      const int qu = tid % A, qq = tid / A;
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < QK; ++i) s = fmaf(wq_s[(qq * QK + i) * A + qu], hloc[qq * QK + i], s);
      red[tid] = s;
    }
    ns_lds_barrier();
    if (tid < A) ns_put_granule(x2 + (size_t)g * X2N + tid, tag, red[tid] + red[A + tid]);
    // ---- (5) gather X2: q = sum of the partials (fixed order), h of every unit
    if (!ns_gather_granules<(CG * X2N + CT - 1) / CT, CT>(x2, CG * X2N, tag, gath, tid, a.status, 2)) sc[2] = 1.f;
    ns_lds_barrier();
    if (sc[2] != 0.f) return;
    if (tid < A) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < CG; ++q) s += gath[q * X2N + tid];
      if (tid / UPW == g) p.q[rowS * A + tid] = s;
      xs[D2 + tid] = gath[(tid / UPW) * X2N + A + (tid % UPW)];          // h(s) for the next step's gates
    }
    // ---- (6) energies of the own positions: e[t] = sum_u v[u] tanh(keys[t][u] + q[u]).  Wave w takes units 32 w ..;
    //      lane = (unit c of a 16-unit tile, 4 positions g4): 16 tanh per lane, a DPP row reduction over the unit lanes
    {
      const int c = lane & 15, g4 = lane >> 4;
      float part[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int ut = 0; ut < 2; ++ut) {
        const int u = wave * 32 + ut * 16 + c;
        const float vv = vs[u];
        float qv = 0.f;
#pragma unroll
        for (int q = 0; q < CG; ++q) qv += gath[q * X2N + u];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            part[rt][q] = fmaf(vv, tanhf_(keys_s[(rt * 16 + g4 * 4 + q) * (A + KPAD) + u] + qv), part[rt][q]);
      }
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float e = row16_sum(part[rt][q]);
          if (c == 0) ered[wave * TSMAX + rt * 16 + g4 * 4 + q] = e;
        }
    }
    ns_lds_barrier();
    if (tid < UPW) {
      // this step's cell for the backward pass / the hoisted products: stored only now, behind the polls of this wave
      const int u = g * UPW + tid;
      p.ru[rowS * 2 * A + u] = sv_r;
      p.ru[rowS * 2 * A + A + u] = sv_u;
      p.cc[rowS * A + u] = sv_c;
      stf((T*)p.xc + rowS * XA + D2 + Dsp + u, sv_rh);
      stf((T*)p.hc + rowS * HC + u, sv_h);
      if (st + 1 < p.S) stf((T*)p.xa + (rowS + 1) * XA + D2 + Dsp + u, sv_h);
    }
    if (wave == 1) {
      float e = -INFINITY;
      if (lane < tn) {
        e = 0.f;
#pragma unroll
        for (int w = 0; w < A / 32; ++w) e += ered[w * TSMAX + lane];
      }
      const float m = wave_max(e);
      const float w = lane < tn ? __expf(e - m) : 0.f;
      const float l = wave_sum(w);
      if (lane < TSMAX) es[lane] = w;
      if (lane == 0) { sc[0] = m; sc[1] = l; }
    }
    ns_lds_barrier();
    // ---- (7) partial next-prenet sums over the own positions, published with the softmax pieces (X3)
    {
      const int c = tid % D1, th = tid / D1;
      float s = 0.f;
      for (int tl = th; tl < tn; tl += CXG) s = fmaf(es[tl], pv_s[tl * D1 + c], s);
      red[tid] = s;
    }
    ns_lds_barrier();
    if (tid < D1) ns_put_granule(x3 + (size_t)g * X3N + tid, tag, red[tid] + red[D1 + tid]);
    else if (tid < D1 + 2) ns_put_granule(x3 + (size_t)g * X3N + tid, tag, sc[tid - D1]);
    else if (tid < D1 + 2 + TSMAX) ns_put_granule(x3 + (size_t)g * X3N + tid, tag, es[tid - D1 - 2]);
    // in the shadow of X3: the h rows of the NEXT step's gates (xs[D2 ..] = h(s) since (5))
    hpart = dot_regs<GKH>(wgh, xs + D2 + (tid / GC) * GKH);
    if (!ns_gather_granules<(CG * X3N + CT - 1) / CT, CT>(x3, CG * X3N, tag, gath, tid, a.status, 3)) sc[2] = 1.f;
    ns_lds_barrier();
    if (sc[2] != 0.f) return;
    float mall = -INFINITY;
#pragma unroll
    for (int q = 0; q < CG; ++q) mall = fmaxf(mall, gath[q * X3N + D1]);
    float scl[CG], lsum = 0.f;
#pragma unroll
    for (int q = 0; q < CG; ++q) {
      const float lq = gath[q * X3N + D1 + 1];
      scl[q] = lq > 0.f ? __expf(gath[q * X3N + D1] - mall) : 0.f;
      lsum = fmaf(lq, scl[q], lsum);
    }
    const float inv = 1.f / lsum;
    for (int t = tid; t < p.Tia; t += CT) {
      float v = 0.f;
      if (t < L) {
        const int q = t / ts;
        v = gath[q * X3N + D1 + 2 + (t - q * ts)] * scl[q] * inv;
      }
      const bool mine = t < L ? (t / ts == g) : (g == CG - 1);
      if (mine) {
        p.align[rowS * p.Tia + t] = v;
        if (p.align_t) stf((T*)p.align_t + rowS * p.Tia + t, v);
        if (INFER) ns_put_granule(a.alx + (size_t)n * p.Tia + t, tag, v);      // the decoder workgroups wait for it
      }
    }
    if (tid < D1) {
      // free-running: the next frame term comes back through both decoder GRUs as one partial sum per decoder workgroup
      // (tag = the consuming step + 1); the alignment above went out first - they cannot answer before they have it
      if (INFER && st + 1 < p.S) {
        f1n = a.bpf[tid];
        if (!poll_partials<DNW>(a.f1x + (size_t)n * DNW * D1 + tid, tag + 1, f1n, a.status, 4)) sc[2] = 1.f;
      }
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < CG; ++q) s = fmaf(scl[q], gath[q * X3N + tid], s);
      float v = fmaxf(fmaf(s, inv, f1n), 0.f);
      if constexpr (DROP) if (st + 1 < p.S) v = ns_prenet_drop(v, p.drop_seed1, st + 1, n, tid, p.drop_thr, p.drop_scale);
      p1s[tid] = v;
      if (st + 1 < p.S && tid / (D1 / CG) == g) stf((T*)p.p1 + (rowS + 1) * D1 + tid, v);
    }
    ns_lds_barrier();
    if (INFER && sc[2] != 0.f) return;
  }
}

template <typename T, bool DROP>
__global__ __launch_bounds__(CT) void taco1_attn_fwd_kernel(TArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const ns_cluster_slot slot = ns_cluster_place(blockIdx.x, a.p.N, CG, a.xcd != 0);
  if (!slot.active) return;                                 // padding of a placed grid (exchange.h)
  attn_fwd_body<T, false, DROP>(a, sm, slot.cluster * CG + slot.member);
}

// ===================================================================================== backward
// Walks s = S-1 .. 0.  State carried between steps: dvec = dp1 of the step after ([D1], every workgroup), hrec = the
// gradient that reaches h(s) of the own units through step s+1.  Per step:
//   P2  dalign[t] of the own positions = da0[t] (hoisted) + pv[t] . dvec; the softmax-backward dot-product share -> E1
//   P3  (runs one step AHEAD: it needs only history) g1[t,u] = v[u] (1 - tanh^2(keys[t,u] + q[u])) in registers
//       de[t] = align[t] (dalign[t] - dot)
//   P4  dq partial of unit u = sum_t de[t] g1[t,u] -> E2 -> dq
//   P6  dh = dhc + dq . Wq^T + hrec;  dzc = dh (1-u)(1-c^2), dzu = dh (h_prev - c) u (1-u), direct = dh u
//   P7a partial input gradients of the candidate kernel over the own columns, all K rows -> E3a:
//       rows < 128: dp2 (first part); rows 128 + own units: d(r h_prev) -> dzr = . h_prev r (1-r), direct += . r
//   P7b the same for the gate kernel over the own [dzr | dzu] columns -> E3b: dp2 (second part), hrec = direct + h rows
//   P9  dp1 = (dp2 . W2^T) masked = the next dvec
struct BwdLds {                            // dynamic LDS of taco1_attn_bwd_kernel
  // per-step history images, twice (parity of the step): the next step's are filled in the middle of this one
  static constexpr int HIMG = A + D1 + D2 + 2 * TSMAX + GC + 3 * UPW;
  LdsCarve c = {};
  int dvec = c.take<float>(D1);            // [D1]
  int dp2s = c.take<float>(D2);            // [D2]
  int dcs = c.take<float>(UPW);            // [UPW]  dzc of the own units
  int dgs = c.take<float>(GC);             // [GC]   dzr | dzu of the own units
  int red = c.take<float>(NQ * K);         // [NQ * K]
  int dav = c.take<float>(TSMAX);          // [TSMAX] dalign
  int dev = c.take<float>(TSMAX);          // [TSMAX] energy gradients
  int hrec = c.take<float>(UPW);           // [UPW]
  int dird = c.take<float>(UPW);           // [UPW]  direct part of the gradient wrt h_prev
  int dq_s = c.take<float>(A);             // [A]
  int sc = c.take<float>(16);              // [16]  [0] dot, [2] abort
  int gath = c.take<float>(CG * K);        // [CG][K]
  int vs = c.take<float>(A);               // [A]
  int keys_s = c.take<float>(TSMAX * (A + KPAD));   // [TSMAX][A + KPAD]
  int pv_s = c.take<float>(TSMAX * D1);    // [TSMAX][D1]
  int wq_s = c.take<float>(UPW * A);       // [UPW][A]
  int him = c.take<float>(2 * HIMG);       // [2][HIMG]: qs | p1m | p2m | acur | da0s | rus | cs | hps | dhcs
  int bytes = c.off;
};
template <typename T, bool DROP>
__global__ __launch_bounds__(CT) void taco1_attn_bwd_kernel(TArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const ns_taco1_attn_params& p = a.p;
  constexpr BwdLds lay;
  constexpr int HIMG = BwdLds::HIMG;
  float* dvec = carve_at<float>(sm, lay.dvec); float* dp2s = carve_at<float>(sm, lay.dp2s);
  float* dcs = carve_at<float>(sm, lay.dcs); float* dgs = carve_at<float>(sm, lay.dgs);
  float* red = carve_at<float>(sm, lay.red); float* dav = carve_at<float>(sm, lay.dav);
  float* dev = carve_at<float>(sm, lay.dev); float* hrec = carve_at<float>(sm, lay.hrec);
  float* dird = carve_at<float>(sm, lay.dird); float* dq_s = carve_at<float>(sm, lay.dq_s);
  float* sc = carve_at<float>(sm, lay.sc); float* gath = carve_at<float>(sm, lay.gath); float* vs = carve_at<float>(sm, lay.vs);
  float* keys_s = carve_at<float>(sm, lay.keys_s); float* pv_s = carve_at<float>(sm, lay.pv_s);
  float* wq_s = carve_at<float>(sm, lay.wq_s); float* him = carve_at<float>(sm, lay.him);

  const int tid_ = threadIdx.x;
  const ns_cluster_slot slot = ns_cluster_place(blockIdx.x, p.N, CG, a.xcd != 0);
  if (!slot.active) return;                                 // padding of a placed grid (exchange.h)
  const int n = slot.cluster, g = slot.member;
  const long S1 = p.S + 1;
  const int HC = A + p.E;
  const int Dsp = p.Dsp, XA = D2 + Dsp + A;                // the loop's K rows skip the speaker rows of both kernels (see the forward kernel)
  const int L = min(p.lengths ? p.lengths[n] : p.Ti, p.Ti);
  const int ts = max(1, (L + CG - 1) / CG);
  const int t0 = g * ts, tn = max(0, min(L, t0 + ts) - t0);
  // prenet dropout: d (relu(z) keep scale) / dz, the keep part read from the history (a dropped unit's saved output is 0)
  auto dsc = [&](float s) { if constexpr (DROP) return s * p.drop_scale; else return s; };
  u64* e1 = a.x1 + (size_t)n * CG;
  u64* e2 = a.x2 + (size_t)n * CG * A;
  u64* e3a = a.x3 + (size_t)n * CG * K;
  u64* e3b = a.x4 + (size_t)n * CG * K;

  // ---------------------------------------------------------------- resident weights
  const T* W2 = (const T*)p.w2;
  const T* Wg = (const T*)p.wg;
  const T* Wc = (const T*)p.wc;
  const T* Wq = (const T*)p.wq;
  const int tid = tid_;
  float wcr[PPT][CPQ_C], wgr[PPT][CPQ_G];  // W[row k][own columns of group qr] for this thread's (k, qr) pairs
#pragma unroll
  for (int jj = 0; jj < PPT; ++jj) {
    const int pi = tid + CT * jj, kl = pi % K, qr = pi / K;
    const int k = kl < D2 ? kl : kl + Dsp;               // kernel row of loop row kl
#pragma unroll
    for (int i = 0; i < CPQ_C; ++i) wcr[jj][i] = ldf(Wc + (long)k * A + g * UPW + qr * CPQ_C + i);
#pragma unroll
    for (int i = 0; i < CPQ_G; ++i) {
      const int c = qr * CPQ_G + i;                      // dgs order: dzr of the own units, then dzu
      wgr[jj][i] = ldf(Wg + (long)k * 2 * A + (c < UPW ? g * UPW + c : A + g * UPW + (c - UPW)));
    }
  }
  float w2r[W2K];                          // W2[c1][hf * W2K + i]
  {
    const T* b = W2 + (long)(tid % D1) * D2 + (tid / D1) * W2K;
#pragma unroll
    for (int i = 0; i < W2K; ++i) w2r[i] = ldf(b + i);
  }
  for (int i = tid; i < UPW * A; i += CT) wq_s[i] = ldf(Wq + (long)g * UPW * A + i);
  for (int i = tid; i < A; i += CT) vs[i] = p.v[i];
  {
    const float* kn = p.keys + ((long)n * p.Pi + p.padl_i + t0) * A;
    for (int i = tid; i < TSMAX * A; i += CT) keys_s[(i / A) * (A + KPAD) + i % A] = (i / A) < tn ? kn[i] : 0.f;
    const T* pvn = (const T*)p.pv + ((long)n * p.Pi + p.padl_i + t0) * D1;
    for (int i = tid; i < TSMAX * D1; i += CT) pv_s[i] = (i / D1) < tn ? ldf(pvn + i) : 0.f;
    for (int i = tid; i < D1; i += CT) dvec[i] = 0.f;
    for (int i = tid; i < 2 * HIMG; i += CT) him[i] = 0.f;
    if (tid < UPW) { hrec[tid] = 0.f; dird[tid] = 0.f; }
    if (tid < TSMAX) { dav[tid] = 0.f; dev[tid] = 0.f; }
    if (tid < 16) sc[tid] = 0.f;
  }
  // history of a step, one value per thread and role
  float h_q = 0.f, h_p1 = 0.f, h_p2 = 0.f, h_a = 0.f, h_da0 = 0.f, h_ru = 0.f, h_c = 0.f, h_hp = 0.f, h_dhc = 0.f;
  auto load_history = [&](int st_, int tid) {
    const long rowS = (long)n * S1 + st_ + 1;
    if (tid < A) h_q = p.q[rowS * A + tid];
    if (tid < D1) h_p1 = ldf((const T*)p.p1 + rowS * D1 + tid);
    if (tid < D2) h_p2 = ldf((const T*)p.xa + rowS * XA + tid);
    h_a = 0.f; h_da0 = 0.f;
    if (tid >= 256 && tid < 256 + TSMAX) {
      const int tl = tid - 256;
      if (tl < tn) { h_a = p.align[rowS * p.Tia + t0 + tl]; h_da0 = p.da0[rowS * p.Tia + t0 + tl]; }
    } else if (tid >= 320 && tid < 320 + GC) {
      const int c = tid - 320;
      h_ru = p.ru[rowS * 2 * A + (c < UPW ? g * UPW + c : A + g * UPW + (c - UPW))];
    } else if (tid >= 384 && tid < 384 + UPW) {
      const int u = g * UPW + tid - 384;
      h_c = p.cc[rowS * A + u];
      h_hp = ldf((const T*)p.xa + rowS * XA + D2 + Dsp + u);
      h_dhc = p.dhc[rowS * HC + u];
    }
  };
  auto store_history = [&](int par, int tid) {
    float* b = him + par * HIMG;
    if (tid < A) b[tid] = h_q;
    if (tid < D1) b[A + tid] = h_p1;
    if (tid < D2) b[A + D1 + tid] = h_p2;
    if (tid >= 256 && tid < 256 + TSMAX) { b[A + D1 + D2 + tid - 256] = h_a; b[A + D1 + D2 + TSMAX + tid - 256] = h_da0; }
    if (tid >= 320 && tid < 320 + GC) b[A + D1 + D2 + 2 * TSMAX + tid - 320] = h_ru;
    if (tid >= 384 && tid < 384 + UPW) {
      float* o = b + A + D1 + D2 + 2 * TSMAX + GC + (tid - 384);
      o[0] = h_c; o[UPW] = h_hp; o[2 * UPW] = h_dhc;
    }
  };
  __syncthreads();                           // the zero fills above are done before the owners' values go in
  load_history(p.S - 1, tid_);
  store_history((p.S - 1) & 1, tid_);
  __syncthreads();
  // energy pass of a step: needs only that step's history (query), runs one step ahead; g1 stays in registers
  float g1v[16];                             // [unit tile ut][position tile rt][q]: unit 32 wave + 16 ut + c, position 16 rt + 4 g4 + q
  auto energy_pass = [&](const float* qs, int lane, int wave) {
    const int c = lane & 15, g4 = lane >> 4;
#pragma unroll
    for (int ut = 0; ut < 2; ++ut) {
      const int u = wave * 32 + ut * 16 + c;
      const float qv = qs[u], vv = vs[u];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int pos = rt * 16 + g4 * 4 + q;
          const float th = tanhf_(keys_s[pos * (A + KPAD) + u] + qv);
          g1v[ut * 8 + rt * 4 + q] = pos < tn ? vv * (1.f - th * th) : 0.f;
        }
    }
  };
  energy_pass(him + ((p.S - 1) & 1) * HIMG, tid_ & 63, tid_ >> 6);

  for (int st = p.S - 1; st >= 0; --st) {
    const long rowS = (long)n * S1 + st + 1;
    const unsigned tag = (unsigned)(p.S - st);
    int tid = tid_;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float* hb = him + (st & 1) * HIMG;
    const float* p1m = hb + A; const float* p2m = hb + A + D1; const float* acur = hb + A + D1 + D2;
    const float* da0s = acur + TSMAX; const float* rusb = da0s + TSMAX; const float* csb = rusb + GC;
    const float* hpsb = csb + UPW; const float* dhcsb = hpsb + UPW;

    if (st > 0) load_history(st - 1, tid);   // lands by the middle of this step
    ns_lds_barrier();
    // ---- P2: dalign of the own positions: thread = (position tid / 16, 16 columns each)
    {
      const int tl = tid >> 4, cq = tid & 15;
      float s = 0.f;
      if (tl < tn) {
        const float* pr = pv_s + tl * D1 + cq * 4;
        const float* dv = dvec + cq * 4;
#pragma unroll
        for (int i = 0; i < D1 / 4; i += 16) {
          const float4 x = *(const float4*)(pr + 4 * i), y = *(const float4*)(dv + 4 * i);
          s = fmaf(x.x, y.x, s); s = fmaf(x.y, y.y, s); s = fmaf(x.z, y.z, s); s = fmaf(x.w, y.w, s);
        }
      }
      s = row16_sum(s);
      if (cq == 0 && tl < TSMAX) dav[tl] = tl < tn ? da0s[tl] + s : 0.f;
    }
    ns_lds_barrier();
    if (wave == 7) {
      const float d = wave_sum(lane < tn ? acur[lane] * dav[lane] : 0.f);
      if (lane == 0) ns_put_granule(e1 + g, tag, d);
      if (!ns_gather_granules<1, CT>(e1, CG, tag, gath, lane < CG ? lane : CG, a.status, 5)) sc[2] = 1.f;
      float dd = lane < CG ? gath[lane] : 0.f;
      dd = wave_sum(dd);
      if (lane == 0) sc[0] = dd;
    }
    ns_lds_barrier();
    if (tid < TSMAX) {
      float de = 0.f;
      if (tid < tn) {
        de = acur[tid] * (dav[tid] - sc[0]);
        p.de[rowS * p.Tia + t0 + tid] = de;
      }
      dev[tid] = de;
    }
    ns_lds_barrier();
    // ---- P4: dq partials -> E2
    {
      const int c = lane & 15, g4 = lane >> 4;
#pragma unroll
      for (int ut = 0; ut < 2; ++ut) {
        float s = 0.f;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int q = 0; q < 4; ++q) s = fmaf(dev[rt * 16 + g4 * 4 + q], g1v[ut * 8 + rt * 4 + q], s);
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (g4 == 0) ns_put_granule(e2 + (size_t)g * A + wave * 32 + ut * 16 + c, tag, s);
      }
    }
    if (!ns_gather_granules<(CG * A + CT - 1) / CT, CT>(e2, CG * A, tag, gath, tid, a.status, 3)) sc[2] = 1.f;
    ns_lds_barrier();
    if (sc[2] != 0.f) return;
    if (st > 0) store_history((st & 1) ^ 1, tid);
    if (tid < A) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < CG; ++q) s += gath[q * A + tid];
      dq_s[tid] = s;
      if (tid / UPW == g) stf((T*)p.dq + rowS * A + tid, s);
    }
    ns_lds_barrier();
    // ---- P6: dh of the own units through W_query, the cell's first half: thread = (unit tid / 16, 16 columns each)
    {
      const int j = tid >> 4, uq = tid & 15;
      float s = 0.f;
      if (j < UPW) {
        const float* wr = wq_s + j * A + uq * 4;
        const float* dq = dq_s + uq * 4;
#pragma unroll
        for (int i = 0; i < A / 16; i += 4) {
          const float4 x = *(const float4*)(wr + 16 * i), y = *(const float4*)(dq + 16 * i);
          s = fmaf(x.x, y.x, s); s = fmaf(x.y, y.y, s); s = fmaf(x.z, y.z, s); s = fmaf(x.w, y.w, s);
        }
      }
      s = row16_sum(s);
      if (uq == 0 && j < UPW) {
        const int u = g * UPW + j;
        const float dh = dhcsb[j] + s + hrec[j];
        const float uu = rusb[UPW + j], c = csb[j], hp = hpsb[j];
        const float dzc = dh * (1.f - uu) * (1.f - c * c);
        const float dzu = dh * (hp - c) * uu * (1.f - uu);
        dcs[j] = dzc;
        dgs[UPW + j] = dzu;
        dird[j] = dh * uu;
        stf((T*)p.dzc + rowS * A + u, dzc);
        stf((T*)p.dzg + rowS * 2 * A + A + u, dzu);
      }
    }
    ns_lds_barrier();
    // ---- P7a: candidate kernel, partial input gradients over the own columns -> E3a
#pragma unroll
    for (int jj = 0; jj < PPT; ++jj) {
      const int pi = tid + CT * jj, qr = pi / K;
      red[pi] = dot_regs<CPQ_C>(wcr[jj], dcs + qr * CPQ_C);
    }
    ns_lds_barrier();
    if (tid < K) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) s += red[q * K + tid];
      ns_put_granule(e3a + (size_t)g * K + tid, tag, s);
    }
    if (!ns_gather_granules<(CG * K + CT - 1) / CT, CT>(e3a, CG * K, tag, gath, tid, a.status, 4)) sc[2] = 1.f;
    ns_lds_barrier();
    if (sc[2] != 0.f) return;
    if (tid < D2) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < CG; ++q) s += gath[q * K + tid];
      dp2s[tid] = s;                         // first part; the mask comes with the second
    } else if (tid < D2 + UPW) {
      const int j = tid - D2, u = g * UPW + j;
      float drh = 0.f;
#pragma unroll
      for (int q = 0; q < CG; ++q) drh += gath[q * K + D2 + u];
      const float r = rusb[j], hp = hpsb[j];
      const float dzr = drh * hp * r * (1.f - r);
      dgs[j] = dzr;
      dird[j] += drh * r;
      stf((T*)p.dzg + rowS * 2 * A + u, dzr);
    }
    ns_lds_barrier();
    // ---- P7b: gate kernel -> E3b
#pragma unroll
    for (int jj = 0; jj < PPT; ++jj) {
      const int pi = tid + CT * jj, qr = pi / K;
      red[pi] = dot_regs<CPQ_G>(wgr[jj], dgs + qr * CPQ_G);
    }
    ns_lds_barrier();
    if (tid < K) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) s += red[q * K + tid];
      ns_put_granule(e3b + (size_t)g * K + tid, tag, s);
    }
    // in the shadow of E3b: the energy pass of step s-1 (its history image was stored behind E2)
    if (st > 0) energy_pass(him + ((st & 1) ^ 1) * HIMG, lane, wave);
    if (!ns_gather_granules<(CG * K + CT - 1) / CT, CT>(e3b, CG * K, tag, gath, tid, a.status, 6)) sc[2] = 1.f;
    ns_lds_barrier();
    if (sc[2] != 0.f) return;
    if (tid < D2) {
      float s = dp2s[tid];
#pragma unroll
      for (int q = 0; q < CG; ++q) s += gath[q * K + tid];
      s = p2m[tid] > 0.f ? dsc(s) : 0.f;
      dp2s[tid] = s;
      if (tid / (D2 / CG) == g) stf((T*)p.dp2 + rowS * D2 + tid, s);
    } else if (tid < D2 + UPW) {
      const int j = tid - D2, u = g * UPW + j;
      float s = dird[j];
#pragma unroll
      for (int q = 0; q < CG; ++q) s += gath[q * K + D2 + u];
      hrec[j] = s;
    }
    ns_lds_barrier();
    // ---- P9: dp1 = (dp2 . W2^T) masked: the next dvec (every workgroup computes all of it)
    red[tid] = dot_regs<W2K>(w2r, dp2s + (tid / D1) * W2K);
    ns_lds_barrier();
    if (tid < D1) {
      float s = red[tid] + red[D1 + tid];
      s = p1m[tid] > 0.f ? dsc(s) : 0.f;
      dvec[tid] = s;
      if (tid / (D1 / CG) == g) stf((T*)p.df1 + rowS * D1 + tid, s);
    }
    ns_lds_barrier();
  }
}

static_assert(FwdLds().bytes <= 160 * 1024 && BwdLds().bytes <= 160 * 1024, "LDS");


// work areas: the status word in a block of its own, then one granule array per exchange, [N] rows each
struct FwdWork {                           // ns_taco1_attn_cluster_fwd, and the head of ns_taco1_decode's
  size_t N;
  WorkCarve c = {};
  size_t status = c.take<char>(256);
  size_t x1 = c.take<u64>(N * CG * X1N);   // [N][CG][X1N]
  size_t x2 = c.take<u64>(N * CG * X2N);   // [N][CG][X2N]
  size_t x3 = c.take<u64>(N * CG * X3N);   // [N][CG][X3N]
  size_t bytes = c.off;
};
struct BwdWork {                           // ns_taco1_attn_cluster_bwd
  size_t N;
  WorkCarve c = {};
  size_t status = c.take<char>(256);
  size_t e1 = c.take<u64>(N * CG);         // [N][CG]      softmax-backward dot-product shares
  size_t e2 = c.take<u64>(N * CG * A);     // [N][CG][A]   dq partials
  size_t e3a = c.take<u64>(N * CG * K);    // [N][CG][K]   input gradients of the candidate kernel
  size_t e3b = c.take<u64>(N * CG * K);    // [N][CG][K]   input gradients of the gate kernel
  size_t bytes = c.off;
};

// ===================================================================================== free-running synthesis
// Synthesis (tacotron.py:80-86 with TacoTestHelper, helpers.py:7-38): the frame fed to step s+1 is the last frame
// predicted at step s, so nothing can be hoisted out of the time loop and the launch-per-step form needs ~28 dependent
// launches per decoder step.  Here the whole loop is ONE launch with two roles, selected by blockIdx:
//   workgroups [0, 8 nr)      the attention clusters of attn_fwd_body<INFER> above, one per row of the launch
//   the next 16 G             decoder workgroups: G = ceil(nr / 2) GROUPS of DNW = 16, DU = 16 units of D = 256 each,
//                             for BOTH decoder GRUs and the attention projection; group g serves the (at most DNR = 2)
//                             rows n0 + 2 g, n0 + 2 g + 1 of the call - a tail group has one row
// A launch takes the rows [n0, n0 + nr) of the call, nr <= ns_taco1_decode_max_rows() = 2 * (CUs / 32): every workgroup
// of the grid (8 nr + 16 G, 256 for 16 rows) must be resident at once, one per CU.  ns_taco1_decode splits a larger N
// into balanced consecutive launches on one stream.  The groups are independent: every exchange array is indexed by the
// row's number in the CALL (x1..x3, f1x, alx, xa..xe, the history), a group reads and writes its own rows' granules only,
// and no group waits on another.  All groups and launches of a call share the status word: a time-out raises it (codes
// below) and ends the group whose wait ran out; another group leaves early only if one of its own waits stalls long
// enough to read the word (ns_spin: every 1024 polls), otherwise it finishes - the call's outputs are invalid either way.
// Nothing clears the word between the launches of a call.
// A decoder workgroup keeps, as fp32 in registers, the columns of its own units: W_proj[h rows] (8 per thread), GRU_1 and
// GRU_2 gates (2 x 32) and candidates (2 x 16), and the rows of the folded feedback wpf that its y2 units multiply (8):
// 112 weights per thread, matrix-VECTOR products as exact fp32 FMAs.  The context never forms in the loop: the projected
// memory PM = memory . W_proj[ctx rows] of the own 16 columns sits in LDS (built once per call), so x1 of the own units
// = h_att . W_proj[h rows] + align . PM + b_proj.  Per step (granule exchanges, each 8 bytes {step tag, fp32}):
//   attention:  h_att(s) -> x2 (its own exchange), align(s) -> alx, then waits for f1(s+1)
//   D1: gather h_att(s), align(s); x1 of the own units                                          -> xa
//   D2: gather x1; GRU_1 gates of the own units (h rows: h1(s-1), gathered a step before); r * h1 -> xb
//   D3: gather r * h1; candidate, h1(s), y1 = x1 + h1 of the own units                           -> xc (y1 | h1)
//   D4: gather y1 | h1; GRU_2 gates; r * h2                                                      -> xd
//   D5: gather r * h2; candidate, h2(s), y2 = y1 + h2 (history); h2 -> xe; the own rows' share of the
//       folded feedback f1(s+1) = y2(s) . wpf + bpf, wpf = W_out[:, last frame] . W_prenet1[frame rows]   -> f1x
//       (the attention sums the 16 shares in a fixed order; the output projection leaves the loop: ONE product over
//       the y2 history after the launch)
//   D6: gather h2(s) for the next step's GRU_2 gates (off the critical path)
// Layout choice: folding W_proj into GRU_1's input weights would save the xa hop but needs a second copy of GRU_1's x
// rows (x1 itself is the residual) and changes the rounding of x1; with one unit range per workgroup for all three
// layers every product stays a plain fp32 dot product of the reference's weights.  One buffer per exchange suffices:
// a workgroup publishes exchange X of step s+1 only behind a chain that passes every reader of X of step s (xa..xe: the
// gathers of the same step by every decoder workgroup; f1x / alx / x2: the attention's poll of f1(s+1) needs every
// decoder workgroup's D1 of step s, and the decoder reads h_att(s+1) only after the attention has passed that poll).
// LDS hand-over audit (decoder role): ha / als are written by the D1 gather and read by D1's products only; x1f by the
// D2 gather, read through D3; rhf by the D2 (GRU_1) and D4 (GRU_2) gathers, each read by the next phase's products
// only; yh1 by the D3 gather (its h1 half is read in D2 / D3 of the NEXT step, so the D3 gather sits behind a barrier
// after D3's reduction); h2f by the D6 gather, read in D4 / D5 of the next step; red / rus / y2s are reduction
// scratch, each rewritten only behind the barrier that follows its readers.  Status codes: 1-3 the attention's three
// gathers, 4 its frame-term poll, 5-10 the decoder phases D1-D6.
// The audit for the grouped form: LDS is per workgroup and a decoder workgroup belongs to one group, so every LDS image
// above holds the group's rows only, indexed by the row's place in the GROUP (0 or 1), and the hand-overs are the ones
// listed; the global arrays are entered at the group's first row (dec_role's x2 / alx / f1x / xa..xe / y2 / val), so the
// one-buffer argument above holds per group - its readers and writers are the group's 16 workgroups and its rows'
// clusters, as they were the launch's.  Two launches of a call touch disjoint rows of every array but the status word.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, both dtypes): 229 VGPRs, 0 AGPRs, 106 SGPRs, no scratch,
// 115 328 bytes of dynamic LDS (the attention role's image; the decoder role needs 82 KB), one workgroup per CU - as
// before the groups.  Measured on one MI355X (profiles/taco1_decode.txt), 300 steps at T_in = 160, the decoder section of
// initialize(): 5.24 ms (N = 1, 17.5 us per step) / 5.77 ms (N = 2) / 5.81 ms (N = 4) / 6.02 ms (N = 16, one launch of
// 256 workgroups, 20.1 us per step) / 11.89 ms (N = 32, two launches).  Groups of four rows (dec_role templated on the
// rows per group, 243 VGPRs, 103 KB LDS) lost: 7.51 / 7.67 / 15.17 ms at N = 4 / 16 / 32.
struct DArgs {
  TArgs att;
  const void* values;                     // (dtype) [N*Pi, E]
  const float *wp, *bp, *wg1, *bg1, *wc1, *bc1, *wg2, *bg2, *wc2, *bc2, *wpf;
  float* y2;                              // [N][S+1][DD]
  u64 *xa, *xb, *xc, *xd, *xe;            // [N][DD]; xc [N][2 DD]
  int n0, nr;                             // the rows of the call that this launch serves: [n0, n0 + nr)
};

struct DecLds {                            // dynamic LDS of dec_role (the decode kernel's decoder workgroups)
  LdsCarve c = {};
  int ha = c.take<float>(DNR * A);         // [DNR][A]      h_att(s)
  int als = c.take<float>(DNR * 256);      // [DNR][256]    align(s)
  int x1f = c.take<float>(DNR * DD);       // [DNR][DD]     x1(s) of every unit
  int rhf = c.take<float>(DNR * DD);       // [DNR][DD]     r * h(s-1) of every unit (GRU_1, then GRU_2)
  int yh1 = c.take<float>(DNR * 2 * DD);   // [DNR][2 DD]   y1(s) | h1(s)
  int h2f = c.take<float>(DNR * DD);       // [DNR][DD]     h2(s-1)
  int red = c.take<float>(DNR * CT);       // [DNR][CT]     partial sums over the k groups
  int rus = c.take<float>(DNR * 2 * DU);   // [DNR][2 DU]   r | u of the own units
  int y2s = c.take<float>(DNR * DU);       // [DNR][DU]     y2 of the own units
  int flag = c.take<float>(4);             // [4]           [0] abort
  int PM = c.take<float>(DNR * 256 * DU);  // [DNR][256][DU] projected memory of the own columns
  int bytes = c.off;
};
template <typename T>
__device__ __forceinline__ void dec_role(const DArgs& d, float* sm, const int w, const int nb, const int N) {
  const ns_taco1_attn_params& p = d.att.p;
  const int tid = threadIdx.x, Tia = p.Tia, u0 = w * DU;
  const long S1 = p.S + 1;
  int* status = d.att.status;
  // the group's rows are nb .. nb + N (N <= DNR) of the call: every global array starts at row nb, LDS is group-local
  const u64* x2 = d.att.x2 + (size_t)nb * CG * X2N;
  const u64* alx = d.att.alx + (size_t)nb * Tia;
  u64* f1x = d.att.f1x + (size_t)nb * DNW * D1;
  u64* xa = d.xa + (size_t)nb * DD;
  u64* xb = d.xb + (size_t)nb * DD;
  u64* xc = d.xc + (size_t)nb * 2 * DD;
  u64* xd = d.xd + (size_t)nb * DD;
  u64* xe = d.xe + (size_t)nb * DD;
  float* y2 = d.y2 + (long)nb * S1 * DD;
  constexpr DecLds lay;
  float* ha = carve_at<float>(sm, lay.ha); float* als = carve_at<float>(sm, lay.als); float* x1f = carve_at<float>(sm, lay.x1f);
  float* rhf = carve_at<float>(sm, lay.rhf); float* yh1 = carve_at<float>(sm, lay.yh1);
  float* h2f = carve_at<float>(sm, lay.h2f); float* red = carve_at<float>(sm, lay.red);
  float* rus = carve_at<float>(sm, lay.rus); float* y2s = carve_at<float>(sm, lay.y2s);
  float* flag = carve_at<float>(sm, lay.flag); float* PM = carve_at<float>(sm, lay.PM);

  // ---- resident weights: 16 columns x 32 k groups (c16, k16) or 32 columns x 16 k groups (c32, k32)
  const int c16 = tid & 15, k16 = tid >> 4, c32 = tid & 31, k32 = tid >> 5;
  const int gcol = c32 < DU ? u0 + c32 : DD + u0 + (c32 - DU);
  float wpr[8], g1r[32], c1r[16], g2r[32], c2r[16], fpr[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) wpr[i] = d.wp[(long)(k16 * 8 + i) * DD + u0 + c16];
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    g1r[i] = d.wg1[(long)(k32 * 32 + i) * 2 * DD + gcol];
    g2r[i] = d.wg2[(long)(k32 * 32 + i) * 2 * DD + gcol];
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    c1r[i] = d.wc1[(long)(k16 * 16 + i) * DD + u0 + c16];
    c2r[i] = d.wc2[(long)(k16 * 16 + i) * DD + u0 + c16];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) fpr[i] = d.wpf[(long)(u0 + (tid >> 8) * 8 + i) * D1 + (tid & 255)];
  const float bpv = d.bp[u0 + c16], bc1v = d.bc1[u0 + c16], bc2v = d.bc2[u0 + c16];
  const float bg1v = d.bg1[gcol], bg2v = d.bg2[gcol];
  // ---- LDS images: PM = memory . W_proj[ctx rows] (own columns), zero states
  {
    const T* val = (const T*)d.values + (long)nb * p.Pi * p.E;
    for (int o = tid; o < N * 256 * DU; o += CT) {
      const int j = o % DU, t = (o / DU) % 256, n = o / (DU * 256);
      float s = 0.f;
      if (t < p.Ti) {
        const T* vr = val + ((long)n * p.Pi + p.padl_i + t) * p.E;
        const float* wc = d.wp + (long)A * DD + u0 + j;
        for (int e = 0; e < p.E; ++e) s = fmaf(ldf(vr + e), wc[(long)e * DD], s);
      }
      PM[o] = s;
    }
    for (int i = tid; i < DNR * 2 * DD; i += CT) yh1[i] = 0.f;
    for (int i = tid; i < DNR * DD; i += CT) h2f[i] = 0.f;
    if (tid < 4) flag[tid] = 0.f;
  }
  __syncthreads();

  for (int st = 0; st < p.S; ++st) {
    const unsigned tag = (unsigned)(st + 1);
    const long slot = st + 1;
    // ---- D1: h_att(s), align(s) -> x1 of the own units
    bool good = ns_gather_mapped<(DNR * A + CT - 1) / CT, CT>(N * A, tag, tid, status, 5, [&](int i, const u64*& src, float*& dst) {
      const int n = i / A, u = i % A;
      src = x2 + ((size_t)n * CG + u / UPW) * X2N + A + u % UPW;
      dst = ha + i;
    });
    good = ns_gather_mapped<(DNR * 256 + CT - 1) / CT, CT>(N * Tia, tag, tid, status, 5, [&](int i, const u64*& src, float*& dst) {
      src = alx + i;
      dst = als + (i / Tia) * 256 + i % Tia;
    }) && good;
    if (!good) flag[0] = 1.f;
    ns_lds_barrier();
    if (flag[0] != 0.f) return;
    for (int n = 0; n < N; ++n) {
      float s = dot_regs<8>(wpr, ha + n * A + k16 * 8);
      for (int t = k16; t < Tia; t += 32) s = fmaf(als[n * 256 + t], PM[(n * 256 + t) * DU + c16], s);
      red[n * CT + tid] = s;
    }
    ns_lds_barrier();
    if (tid < N * DU) {
      const int n = tid / DU, j = tid % DU;
      float s = bpv;
#pragma unroll
      for (int q = 0; q < 32; ++q) s += red[n * CT + q * DU + j];
      ns_put_granule(xa + (size_t)n * DD + u0 + j, tag, s);
    }
    // ---- D2: x1 of every unit -> GRU_1 gates of the own units, r * h1(s-1)
    good = ns_gather_mapped<(DNR * DD + CT - 1) / CT, CT>(N * DD, tag, tid, status, 6, [&](int i, const u64*& src, float*& dst) {
      src = xa + i; dst = x1f + i;
    });
    if (!good) flag[0] = 1.f;
    ns_lds_barrier();
    if (flag[0] != 0.f) return;
    for (int n = 0; n < N; ++n)
      red[n * CT + tid] = dot_regs<32>(g1r, k32 < 8 ? x1f + n * DD + k32 * 32 : yh1 + n * 2 * DD + DD + (k32 - 8) * 32);
    ns_lds_barrier();
    if (tid < N * 2 * DU) {
      const int n = tid / (2 * DU), c = tid % (2 * DU);
      float z = bg1v;
#pragma unroll
      for (int q = 0; q < 16; ++q) z += red[n * CT + q * 2 * DU + c];
      const float v = sigmoidf_(z);
      rus[n * 2 * DU + c] = v;
      if (c < DU) ns_put_granule(xb + (size_t)n * DD + u0 + c, tag, v * yh1[n * 2 * DD + DD + u0 + c]);
    }
    // ---- D3: r * h1 of every unit -> candidate, h1(s), y1 = x1 + h1 of the own units
    good = ns_gather_mapped<(DNR * DD + CT - 1) / CT, CT>(N * DD, tag, tid, status, 7, [&](int i, const u64*& src, float*& dst) {
      src = xb + i; dst = rhf + i;
    });
    if (!good) flag[0] = 1.f;
    ns_lds_barrier();
    if (flag[0] != 0.f) return;
    for (int n = 0; n < N; ++n)
      red[n * CT + tid] = dot_regs<16>(c1r, k16 < 16 ? x1f + n * DD + k16 * 16 : rhf + n * DD + (k16 - 16) * 16);
    ns_lds_barrier();
    if (tid < N * DU) {
      const int n = tid / DU, j = tid % DU;
      float z = bc1v;
#pragma unroll
      for (int q = 0; q < 32; ++q) z += red[n * CT + q * DU + j];
      const float c = tanhf_(z), u = rus[n * 2 * DU + DU + j];
      const float h = u * yh1[n * 2 * DD + DD + u0 + j] + (1.f - u) * c;
      ns_put_granule(xc + (size_t)n * 2 * DD + u0 + j, tag, x1f[n * DD + u0 + j] + h);
      ns_put_granule(xc + (size_t)n * 2 * DD + DD + u0 + j, tag, h);
    }
    ns_lds_barrier();                           // yh1's h1 half was read above; the gather below rewrites it
    // ---- D4: y1 | h1 of every unit -> GRU_2 gates of the own units, r * h2(s-1)
    good = ns_gather_mapped<(DNR * 2 * DD + CT - 1) / CT, CT>(N * 2 * DD, tag, tid, status, 8, [&](int i, const u64*& src, float*& dst) {
      src = xc + i; dst = yh1 + i;
    });
    if (!good) flag[0] = 1.f;
    ns_lds_barrier();
    if (flag[0] != 0.f) return;
    for (int n = 0; n < N; ++n)
      red[n * CT + tid] = dot_regs<32>(g2r, k32 < 8 ? yh1 + n * 2 * DD + k32 * 32 : h2f + n * DD + (k32 - 8) * 32);
    ns_lds_barrier();
    if (tid < N * 2 * DU) {
      const int n = tid / (2 * DU), c = tid % (2 * DU);
      float z = bg2v;
#pragma unroll
      for (int q = 0; q < 16; ++q) z += red[n * CT + q * 2 * DU + c];
      const float v = sigmoidf_(z);
      rus[n * 2 * DU + c] = v;
      if (c < DU) ns_put_granule(xd + (size_t)n * DD + u0 + c, tag, v * h2f[n * DD + u0 + c]);
    }
    // ---- D5: r * h2 of every unit -> candidate, h2(s), y2 = y1 + h2 of the own units; the feedback shares
    good = ns_gather_mapped<(DNR * DD + CT - 1) / CT, CT>(N * DD, tag, tid, status, 9, [&](int i, const u64*& src, float*& dst) {
      src = xd + i; dst = rhf + i;
    });
    if (!good) flag[0] = 1.f;
    ns_lds_barrier();
    if (flag[0] != 0.f) return;
    for (int n = 0; n < N; ++n)
      red[n * CT + tid] = dot_regs<16>(c2r, k16 < 16 ? yh1 + n * 2 * DD + k16 * 16 : rhf + n * DD + (k16 - 16) * 16);
    ns_lds_barrier();
    if (tid < N * DU) {
      const int n = tid / DU, j = tid % DU;
      float z = bc2v;
#pragma unroll
      for (int q = 0; q < 32; ++q) z += red[n * CT + q * DU + j];
      const float c = tanhf_(z), u = rus[n * 2 * DU + DU + j];
      const float h = u * h2f[n * DD + u0 + j] + (1.f - u) * c;
      const float y = yh1[n * 2 * DD + u0 + j] + h;
      y2s[n * DU + j] = y;
      y2[((long)n * S1 + slot) * DD + u0 + j] = y;
      if (st + 1 < p.S) ns_put_granule(xe + (size_t)n * DD + u0 + j, tag, h);
    }
    ns_lds_barrier();
    if (st + 1 < p.S) {
      // f1(s+1) share of the own rows: thread = (column tid & 255, rows 8 (tid >> 8) ..)
      for (int n = 0; n < N; ++n) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s = fmaf(fpr[i], y2s[n * DU + (tid >> 8) * 8 + i], s);
        red[n * CT + tid] = s;
      }
      ns_lds_barrier();
      if (tid < D1)
        for (int n = 0; n < N; ++n)
          ns_put_granule(f1x + ((size_t)n * DNW + w) * D1 + tid, tag + 1, red[n * CT + tid] + red[n * CT + D1 + tid]);
      // ---- D6: h2(s) of every unit for the next step
      good = ns_gather_mapped<(DNR * DD + CT - 1) / CT, CT>(N * DD, tag, tid, status, 10, [&](int i, const u64*& src, float*& dst) {
        src = xe + i; dst = h2f + i;
      });
      if (!good) flag[0] = 1.f;
      ns_lds_barrier();
      if (flag[0] != 0.f) return;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(CT) void taco1_decode_kernel(DArgs d) {
  extern __shared__ __attribute__((aligned(16))) float sm_dec[];
  const int na = d.nr * CG;
  if ((int)blockIdx.x < na) {
    attn_fwd_body<T, true>(d.att, sm_dec, d.n0 * CG + (int)blockIdx.x);
  } else {
    const int b = (int)blockIdx.x - na, nb = d.n0 + (b / DNW) * DNR;
    dec_role<T>(d, sm_dec, b % DNW, nb, min(DNR, d.n0 + d.nr - nb));
  }
}

constexpr size_t DECODE_LDS = max_of(DecLds().bytes, FwdLds().bytes);      // the two roles overlay one region
static_assert(DECODE_LDS <= 160 * 1024 && D1 == 256 && DD == 256, "LDS / shapes");
struct DecWork {                           // ns_taco1_decode: the forward form's arrays, then the decoder's
  size_t N;
  FwdWork att{N};
  WorkCarve c{att.bytes};
  size_t f1x = c.take<u64>(N * DNW * D1);  // [N][DNW][D1] partial sums of the next step's frame term
  size_t alx = c.take<u64>(N * 256);       // [N][256]     align(s)
  size_t xa = c.take<u64>(N * DD);         // [N][DD]      x1
  size_t xb = c.take<u64>(N * DD);         // [N][DD]      r * h1
  size_t xc = c.take<u64>(N * 2 * DD);     // [N][2 DD]    y1 | h1
  size_t xd = c.take<u64>(N * DD);         // [N][DD]      r * h2
  size_t xe = c.take<u64>(N * DD);         // [N][DD]      h2
  size_t bytes = c.off;
};
}  // namespace

// Everything ns_taco1_attn_cluster_supported asks but the residency of the launch (ns_taco1_decode splits its rows).
static int taco1_attn_shape_ok(const ns_taco1_attn_params* p) {
  if (!p) return 0;
  if (!(p->A == A && p->D1 == D1 && p->D2 == D2 && p->E > 0 && p->Ti >= 1 && p->Ti <= 256 && p->Tia >= p->Ti && p->S >= 1 && p->N >= 1 && p->Dsp >= 0)) return 0;
  if (!(p->dtype == NS_F32 || p->dtype == NS_BF16)) return 0;
  if (!p->keys || !p->pv || !p->f1 || !p->w2 || !p->wg || !p->wc || !p->wq || !p->b2 || !p->bg || !p->bc || !p->v) return 0;
  if (!p->p1 || !p->xa || !p->xc || !p->hc || !p->ru || !p->cc || !p->q || !p->align) return 0;
  if ((long)p->N * (p->S + 1) * (long)(p->A + p->E) >= (1L << 31)) return 0;
  return 1;
}

extern "C" int ns_taco1_attn_cluster_supported(const ns_taco1_attn_params* p) {
  if (!taco1_attn_shape_ok(p)) return 0;
  return p->N * CG <= ns_device_cus();      // every workgroup of the launch must be resident at once, one per CU
}

extern "C" size_t ns_taco1_attn_cluster_work_bytes(const ns_taco1_attn_params* p) {
  if (!p) return 0;
  return max_of(FwdWork{(size_t)p->N}.bytes, BwdWork{(size_t)p->N}.bytes);
}

static int taco1_run(const ns_taco1_attn_params* p, void* work, hipStream_t s, int backward) {
  const char* name = backward ? "ns_taco1_attn_cluster_bwd" : "ns_taco1_attn_cluster_fwd";
  NS_CHECK_ARG(p && work, "%s: null", name);
  NS_CHECK_ARG(ns_taco1_attn_cluster_supported(p), "%s: needs A = 256, D1 = 256, D2 = 128, T_in <= 256, N * 8 <= the device's CUs", name);
  if (backward) NS_CHECK_ARG(p->dhc && p->da0 && p->df1 && p->dp2 && p->dzg && p->dzc && p->dq && p->de, "%s: null backward operand", name);
  TArgs a = {};
  a.p = *p;
  size_t used;
  if (!backward) {
    const FwdWork wl{(size_t)p->N};
    a.status = carve_at<int>(work, wl.status);
    a.x1 = carve_at<u64>(work, wl.x1); a.x2 = carve_at<u64>(work, wl.x2); a.x3 = carve_at<u64>(work, wl.x3); a.x4 = nullptr;
    used = wl.bytes;
  } else {
    const BwdWork wl{(size_t)p->N};
    a.status = carve_at<int>(work, wl.status);
    a.x1 = carve_at<u64>(work, wl.e1); a.x2 = carve_at<u64>(work, wl.e2); a.x3 = carve_at<u64>(work, wl.e3a); a.x4 = carve_at<u64>(work, wl.e3b);
    used = wl.bytes;
  }
  { const int zrc = ns_zero_async(work, (used + 15) & ~(size_t)15, s); if (zrc) return zrc; }
  static bool attr = false;
  if (!attr) {
    for (const void* k : {(const void*)taco1_attn_fwd_kernel<float, false>, (const void*)taco1_attn_fwd_kernel<bf16_t, false>,
                          (const void*)taco1_attn_bwd_kernel<float, false>, (const void*)taco1_attn_bwd_kernel<bf16_t, false>,
                          (const void*)taco1_attn_fwd_kernel<float, true>, (const void*)taco1_attn_fwd_kernel<bf16_t, true>,
                          (const void*)taco1_attn_bwd_kernel<float, true>, (const void*)taco1_attn_bwd_kernel<bf16_t, true>})
      (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  a.xcd = ns_cluster_placed("taco1attn") ? 1 : 0;
  const dim3 grid((unsigned)ns_cluster_grid(p->N, CG, a.xcd != 0)), block(CT);
  if (!backward) {
    if (p->dtype == NS_BF16) {
      if (p->drop_thr) hipLaunchKernelGGL((taco1_attn_fwd_kernel<bf16_t, true>), grid, block, FwdLds().bytes, s, a);
      else hipLaunchKernelGGL((taco1_attn_fwd_kernel<bf16_t, false>), grid, block, FwdLds().bytes, s, a);
    } else {
      if (p->drop_thr) hipLaunchKernelGGL((taco1_attn_fwd_kernel<float, true>), grid, block, FwdLds().bytes, s, a);
      else hipLaunchKernelGGL((taco1_attn_fwd_kernel<float, false>), grid, block, FwdLds().bytes, s, a);
    }
  } else {
    if (p->dtype == NS_BF16) {
      if (p->drop_thr) hipLaunchKernelGGL((taco1_attn_bwd_kernel<bf16_t, true>), grid, block, BwdLds().bytes, s, a);
      else hipLaunchKernelGGL((taco1_attn_bwd_kernel<bf16_t, false>), grid, block, BwdLds().bytes, s, a);
    } else {
      if (p->drop_thr) hipLaunchKernelGGL((taco1_attn_bwd_kernel<float, true>), grid, block, BwdLds().bytes, s, a);
      else hipLaunchKernelGGL((taco1_attn_bwd_kernel<float, false>), grid, block, BwdLds().bytes, s, a);
    }
  }
  NS_CHECK_LAUNCH(name);
  return NS_OK;
}

extern "C" int ns_taco1_attn_cluster_fwd(const ns_taco1_attn_params* p, void* work, ns_stream_t s) {
  return taco1_run(p, work, (hipStream_t)s, 0);
}
extern "C" int ns_taco1_attn_cluster_bwd(const ns_taco1_attn_params* p, void* work, ns_stream_t s) {
  return taco1_run(p, work, (hipStream_t)s, 1);
}

// ------------------------------------------------------------------ free-running synthesis, C ABI
// Rows per launch: a group of DNR rows takes DNR * CG + DNW = 32 workgroups, one per CU.
extern "C" int ns_taco1_decode_max_rows(void) { return DNR * (ns_device_cus() / (DNR * CG + DNW)); }

// The call's N rows as balanced consecutive launches of at most max_rows each (20 rows at 16 per launch: 10 + 10).  A
// device below 32 CUs has max_rows = 0 and still takes the one launch of N <= 2 if that fits.
static int decode_launches(int N) {
  const int cap = ns_taco1_decode_max_rows();
  return cap > 0 ? (N + cap - 1) / cap : 1;
}
static int decode_grid(int nr) { return nr * CG + DNW * ((nr + DNR - 1) / DNR); }

extern "C" int ns_taco1_decode_supported(const ns_taco1_decode_params* q) {
  if (!q) return 0;
  const ns_taco1_attn_params* p = &q->att;
  if (!taco1_attn_shape_ok(p)) return 0;
  if (q->D != DD || p->Tia > 256 || p->E < 1) return 0;
  if (!q->values || !q->w_proj || !q->b_proj || !q->wg_1 || !q->bg_1 || !q->wc_1 || !q->bc_1 || !q->wg_2 || !q->bg_2 ||
      !q->wc_2 || !q->bc_2 || !q->wpf || !q->bpf || !q->y2)
    return 0;
  const int nl = decode_launches(p->N);
  return decode_grid((p->N + nl - 1) / nl) <= ns_device_cus();     // every workgroup of a launch resident at once, one per CU
}

extern "C" size_t ns_taco1_decode_work_bytes(const ns_taco1_decode_params* q) {
  if (!q) return 0;
  return DecWork{(size_t)q->att.N}.bytes;
}

extern "C" int ns_taco1_decode(const ns_taco1_decode_params* q, void* work, ns_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  NS_CHECK_ARG(q && work, "ns_taco1_decode: null");
  NS_CHECK_ARG(ns_taco1_decode_supported(q), "ns_taco1_decode: unsupported shape (needs A = D1 = D = 256, D2 = 128, "
               "T_in <= 256, N >= 1, 32 workgroups resident per two rows of a launch: ns_taco1_decode_max_rows) or a null operand");
  const ns_taco1_attn_params* p = &q->att;
  NS_CHECK_ARG(p->drop_thr == 0, "ns_taco1_decode: prenet dropout (att.drop_thr != 0) is a training option");
  DArgs d = {};
  d.att.p = *p;
  const DecWork wl{(size_t)p->N};
  d.att.status = carve_at<int>(work, wl.att.status);
  d.att.x1 = carve_at<u64>(work, wl.att.x1); d.att.x2 = carve_at<u64>(work, wl.att.x2); d.att.x3 = carve_at<u64>(work, wl.att.x3);
  d.att.x4 = nullptr;
  d.att.f1x = carve_at<u64>(work, wl.f1x);
  d.att.alx = carve_at<u64>(work, wl.alx);
  d.att.bpf = q->bpf;
  d.att.nwd = DNW;
  d.xa = carve_at<u64>(work, wl.xa); d.xb = carve_at<u64>(work, wl.xb); d.xc = carve_at<u64>(work, wl.xc);
  d.xd = carve_at<u64>(work, wl.xd); d.xe = carve_at<u64>(work, wl.xe);
  d.values = q->values;
  d.wp = q->w_proj; d.bp = q->b_proj;
  d.wg1 = q->wg_1; d.bg1 = q->bg_1; d.wc1 = q->wc_1; d.bc1 = q->bc_1;
  d.wg2 = q->wg_2; d.bg2 = q->bg_2; d.wc2 = q->wc_2; d.bc2 = q->bc_2;
  d.wpf = q->wpf; d.y2 = q->y2;
  // the whole work area once, status word included: the launches below share that word and none of them clears it
  { const int zrc = ns_zero_async(work, (wl.bytes + 15) & ~(size_t)15, s); if (zrc) return zrc; }
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)taco1_decode_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)taco1_decode_kernel<bf16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  const int nl = decode_launches(p->N);
  for (int l = 0; l < nl; ++l) {
    // rows [N l / nl, N (l + 1) / nl): consecutive, sizes differ by at most one
    d.n0 = (int)((long)p->N * l / nl);
    d.nr = (int)((long)p->N * (l + 1) / nl) - d.n0;
    const dim3 grid((unsigned)decode_grid(d.nr)), block(CT);
    if (p->dtype == NS_BF16) hipLaunchKernelGGL(taco1_decode_kernel<bf16_t>, grid, block, DECODE_LDS, s, d);
    else hipLaunchKernelGGL(taco1_decode_kernel<float>, grid, block, DECODE_LDS, s, d);
    NS_CHECK_LAUNCH("ns_taco1_decode");
  }
  return NS_OK;
}
