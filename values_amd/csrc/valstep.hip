// The validation step's reductions (LightningExperiment.validation_step and forward_ssn(val=True),
// lightning_experiment.py:175-219, 278-377): what turns a model's output and a label volume into val_loss and val_dice.
//   * vx_val_sums_batched            deterministic branch: softmax / log-softmax / arg-max of logits [B][C][nvox]
//   * vx_val_aleatoric_sums_batched  aleatoric head: T samples y_t = fmaf(exp(s/2), eps_t, mu), log-softmax over classes,
//                                    lavg_c = logsumexp_t - log T, p = exp(lavg)
//   * vx_val_ssn_sums_batched        SSN head: S samples of the low-rank normal, per sample sum_v log_softmax(y_s)[t] and the
//                                    arg-max counts
//   * vx_val_ssn2d_sums_batched      the same sums for the 2D SSN head (HighResolutionNet.hrnet_ssn), whose mean and factor live at
//                                    1/4 resolution: the samples are formed per full-resolution pixel inside the reduction
//                                    (val_ssn2d_kernel, further down, with its own notes)
// The reference materialises S x B x C x voxels samples and runs cross_entropy, S arg-maxes and S dice calls over them; here the
// head is read once and a few hundred bytes per item are written.  No sample is written.
//
// ARITHMETIC CONTRACT.  The sample logits are float32, formed with the very expressions of vx_aleatoric_sample /
// vx_ssn_sample (accumulate.hip; this file is compiled with -ffp-contract=off like that one).  Everything after them is
// float64: the maximum, exp, log, every sum.  Per voxel, with y the float32 logits of one sample:
//     a   = the lowest class index that holds max_c y_c          (float32 comparison: exact)
//     m   = (double) y_a,   se = sum_c exp((double) y_c - m)  in class order,   lsm_c = ((double) y_c - m) - log(se)
//   plain:      p_c = exp((double) y_c - m) / se
//   aleatoric:  the running logsumexp over t of lsm_c[t] (M, A) <- t = 0: (l, 1);  d = l - M, e = exp(-|d|),
//               d > 0: (l, A * e + 1) else (M, A + e);   lavg_c = (M + log(A)) - log((double) T),  p_c = exp(lavg_c),
//               arg-max of lavg (float64 comparison, lowest index on ties), log term lavg_t
//   SSN:        log term lsm_t of every sample
//
// SHAPE.  One thread per voxel: a span of VS_SPAN = 256 consecutive voxels belongs to a workgroup, wave w of it takes the voxels
// w * 64 + lane (coalesced plane reads; 64^3 gives 1024 workgroups per item, four waves per SIMD for a batch of one -- the kernels
// are bound by their float64 exp / log, so a batch of one needs the whole device as much as a batch of eight).  The grid is
// (spans of ONE item, B): a rule of nvox alone, so item b of a batch is cut, summed and combined exactly as the same item
// submitted alone.  Accumulators live in registers, one LANE per
// accumulator: a voxel step's contributions go through a fixed xor butterfly (every lane ends with the same bits), integer
// counts through ballot + popcount, and lane k adds the total into its register if it owns accumulator k (lane c: class c;
// SSN: lane s: sample s).  At the end of a span the four waves' registers meet in LDS and are added in wave order into the
// span's partial row; a finalize launch adds an item's rows: a wave per output, lane l the spans l, l + 64, ... in ascending order,
// then the same butterfly.  No atomics, no data-dependent order.
#include "common.h"
#include "gauss.h"
#include "bil_coord.h"
#include "ssn2d_internal.h"

constexpr int VS_SPAN = 256;
constexpr int VS_MAXC = 32;                   // plain kernel
constexpr int VS_MINCS = 2, VS_MAXCS = 8;     // sampled kernels
constexpr int VS_MAXS = 32, VS_MAXR = 32;
constexpr int VS_MAXB = 65535;
constexpr int64_t VS_MAXVOX = (int64_t)1 << 39;
constexpr int64_t VS_MAXGRID = 1 << 20;       // span workgroups of an item; more spans than that: every VS_MAXGRID-th

__device__ __forceinline__ double vs_wave_all(double x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}
__device__ __forceinline__ int vs_pop(unsigned long long m) { return __popcll(m); }

// label of a voxel as the kernels see it: 0xffff past the end of the item (no class, no log term, not invalid)
struct vs_label {
  int lab;
  bool take, inv;
};
__device__ __forceinline__ vs_label vs_load_label(const uint8_t* __restrict__ g, int64_t v, int64_t nvox, int C, int ignore) {
  vs_label l;
  const bool act = v < nvox;
  l.lab = act ? (int)g[v] : 0xffff;
  l.take = l.lab < C && l.lab != ignore;
  l.inv = act && l.lab >= C && l.lab != ignore;
  return l;
}

// the four waves' rows of LDS, added in wave order into the span's partial row
__device__ __forceinline__ void vs_flush(const double* red, int stride, int K, double* __restrict__ row) {
  __syncthreads();
  for (int k = threadIdx.x; k < K; k += 256) row[k] = ((red[k] + red[stride + k]) + red[2 * stride + k]) + red[3 * stride + k];
  __syncthreads();
}

// ---- the deterministic branch ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void val_sums_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels, int C,
                                                       int64_t nvox, int ignore, int64_t nspan, double* __restrict__ part) {
  constexpr int KMAX = 5 * VS_MAXC + 3;
  __shared__ double red[4 * KMAX];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, K = 5 * C + 3;
  const float* x = logits + (size_t)b * C * nvox;
  const uint8_t* g = labels + (size_t)b * nvox;
  for (int64_t sp = blockIdx.x; sp < nspan; sp += gridDim.x) {
    double aI = 0.0, aP = 0.0, aL = 0.0;
    int nT = 0, nTP = 0, nPR = 0, nV = 0, nInv = 0;
    for (int it = 0; it < VS_SPAN / 256; ++it) {
      const int64_t v0 = sp * VS_SPAN + it * 256 + wave * 64;
      if (v0 >= nvox) break;   // the whole wave is past the end
      const int64_t v = v0 + lane;
      const bool act = v < nvox;
      const int64_t vv = act ? v : nvox - 1;
      const vs_label l = vs_load_label(g, v, nvox, C, ignore);
      float mx = x[vv];
      int a = 0;
      for (int c = 1; c < C; ++c) {
        const float xc = x[(size_t)c * nvox + vv];
        if (xc > mx) { mx = xc; a = c; }
      }
      const double m = (double)mx;
      double se = 0.0;
      for (int c = 0; c < C; ++c) se += exp((double)x[(size_t)c * nvox + vv] - m);
      const double lse = log(se);
      double lt = 0.0;
      for (int c = 0; c < C; ++c) {
        const double d = (double)x[(size_t)c * nvox + vv] - m;
        const double p = act ? exp(d) / se : 0.0;
        const bool tc = l.lab == c;
        if (tc && l.take) lt = d - lse;
        const double sP = vs_wave_all(p), sI = vs_wave_all(tc ? p : 0.0);
        const unsigned long long bt = __ballot(tc), ba = __ballot(act && a == c);
        if (lane == c) {
          aP += sP;
          aI += sI;
          nT += vs_pop(bt);
          nPR += vs_pop(ba);
          nTP += vs_pop(bt & ba);
        }
      }
      aL += vs_wave_all(lt);
      nV += vs_pop(__ballot(l.take));
      nInv += vs_pop(__ballot(l.inv));
    }
    double* rd = red + wave * KMAX;
    if (lane < C) {
      rd[5 * lane + 0] = aI;
      rd[5 * lane + 1] = (double)nT;
      rd[5 * lane + 2] = aP;
      rd[5 * lane + 3] = (double)nTP;
      rd[5 * lane + 4] = (double)nPR;
    }
    if (lane == 0) {
      rd[5 * C + 0] = aL;
      rd[5 * C + 1] = (double)nV;
      rd[5 * C + 2] = (double)nInv;
    }
    vs_flush(red, KMAX, K, part + ((size_t)b * nspan + sp) * K);
  }
}

// float32 logits of one sample -> the arg-max (lowest index on ties) and, in float64, lsm_c for every class
template <int C>
__device__ __forceinline__ int vs_log_softmax(const float (&y)[C], double (&l)[C]) {
  if constexpr (C == 2) {
    // the arg-max class's term is exp(0) = 1 and the sum has two terms: one exp, the same bits as the general form below
    const bool a1 = y[1] > y[0];
    const double d = a1 ? (double)y[0] - (double)y[1] : (double)y[1] - (double)y[0];   // the other class - the maximum
    const double lse = log(1.0 + exp(d));
    l[0] = a1 ? d - lse : 0.0 - lse;
    l[1] = a1 ? 0.0 - lse : d - lse;
    return a1 ? 1 : 0;
  }
  float mx = y[0];
  int a = 0;
#pragma unroll
  for (int c = 1; c < C; ++c)
    if (y[c] > mx) { mx = y[c]; a = c; }
  const double m = (double)mx;
  double se = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    l[c] = (double)y[c] - m;
    se += exp(l[c]);
  }
  const double lse = log(se);
#pragma unroll
  for (int c = 0; c < C; ++c) l[c] -= lse;
  return a;
}

// ---- the aleatoric head -----------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void val_aleatoric_kernel(const float* __restrict__ mu_s, const float* __restrict__ eps, uint32_t seed,
                                                            uint32_t item0, const uint8_t* __restrict__ labels, int T, double logT,
                                                            int64_t nvox, int ignore, int64_t nspan, double* __restrict__ part) {
  constexpr int K = 5 * C + 3;
  __shared__ double red[4 * K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const int64_t per = (int64_t)C * nvox;
  const float* ms = mu_s + (size_t)b * 2 * per;
  const float* ep = eps ? eps + (size_t)b * T * per : nullptr;
  const uint8_t* g = labels + (size_t)b * nvox;
  const uint32_t slot0 = (item0 + (uint32_t)b) * (uint32_t)T;
  for (int64_t sp = blockIdx.x; sp < nspan; sp += gridDim.x) {
    double aI = 0.0, aP = 0.0, aL = 0.0;
    int nT = 0, nTP = 0, nPR = 0, nV = 0, nInv = 0;
    for (int it = 0; it < VS_SPAN / 256; ++it) {
      const int64_t v0 = sp * VS_SPAN + it * 256 + wave * 64;
      if (v0 >= nvox) break;
      const int64_t v = v0 + lane;
      const bool act = v < nvox;
      const int64_t vv = act ? v : nvox - 1;
      const vs_label l = vs_load_label(g, v, nvox, C, ignore);
      float mu[C], sg[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        mu[c] = ms[(size_t)c * nvox + vv];
        sg[c] = expf(0.5f * ms[(size_t)per + (size_t)c * nvox + vv]);
      }
      double M[C], A[C];
      for (int t = 0; t < T; ++t) {
        float y[C];
        double ls[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int64_t r = (int64_t)c * nvox + vv;
          const float e = ep ? ep[(size_t)t * per + r] : vx_gauss(seed, (uint32_t)r, slot0 + (uint32_t)t);
          y[c] = fmaf(sg[c], e, mu[c]);
        }
        vs_log_softmax<C>(y, ls);
#pragma unroll
        for (int c = 0; c < C; ++c) {
          if (t == 0) {
            M[c] = ls[c];
            A[c] = 1.0;
          } else {
            const double d = ls[c] - M[c];
            const double e = exp(-fabs(d));
            A[c] = d > 0.0 ? A[c] * e + 1.0 : A[c] + e;
            M[c] = d > 0.0 ? ls[c] : M[c];
          }
        }
      }
      double lavg[C];
#pragma unroll
      for (int c = 0; c < C; ++c) lavg[c] = (M[c] + log(A[c])) - logT;
      int a = 0;
      double best = lavg[0];
#pragma unroll
      for (int c = 1; c < C; ++c)
        if (lavg[c] > best) { best = lavg[c]; a = c; }
      double lt = 0.0;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double p = act ? exp(lavg[c]) : 0.0;
        const bool tc = l.lab == c;
        if (tc && l.take) lt = lavg[c];
        const double sP = vs_wave_all(p), sI = vs_wave_all(tc ? p : 0.0);
        const unsigned long long bt = __ballot(tc), ba = __ballot(act && a == c);
        if (lane == c) {
          aP += sP;
          aI += sI;
          nT += vs_pop(bt);
          nPR += vs_pop(ba);
          nTP += vs_pop(bt & ba);
        }
      }
      aL += vs_wave_all(lt);
      nV += vs_pop(__ballot(l.take));
      nInv += vs_pop(__ballot(l.inv));
    }
    double* rd = red + wave * K;
    if (lane < C) {
      rd[5 * lane + 0] = aI;
      rd[5 * lane + 1] = (double)nT;
      rd[5 * lane + 2] = aP;
      rd[5 * lane + 3] = (double)nTP;
      rd[5 * lane + 4] = (double)nPR;
    }
    if (lane == 0) {
      rd[5 * C + 0] = aL;
      rd[5 * C + 1] = (double)nV;
      rd[5 * C + 2] = (double)nInv;
    }
    vs_flush(red, K, K, part + ((size_t)b * nspan + sp) * K);
  }
}

// ---- the SSN head ---------------------------------------------------------------------------------------------------------------
// partial row: [S][1 + 2C] (sum_v lsm_t | tp_c | pred_c), then [C + 2] (#[t = c] | valid | invalid)
template <int C>
__global__ __launch_bounds__(256) void val_ssn_kernel(const float* __restrict__ head, const float* __restrict__ eps_w,
                                                      const float* __restrict__ eps_d, uint32_t seed, uint32_t item0,
                                                      const uint8_t* __restrict__ labels, int B, int S, int R, int64_t nvox, float epsilon,
                                                      int ignore, int64_t nspan, double* __restrict__ part) {
  constexpr int PS = 1 + 2 * C;
  constexpr int KMAX = VS_MAXS * PS + C + 2;
  __shared__ double red[4 * KMAX];
  __shared__ float sew[VS_MAXS * VS_MAXR];   // eps_w [s][k] of this item
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, K = S * PS + C + 2;
  const int64_t per = (int64_t)C * nvox;
  const float* h = head + (size_t)b * (2 + R) * per;
  const uint8_t* g = labels + (size_t)b * nvox;
  const uint32_t slot0 = (item0 + (uint32_t)b) * (uint32_t)S;
  for (int i = tid; i < S * R; i += 256) {
    const int s = i / R, k = i - s * R;
    sew[i] = eps_w ? eps_w[((size_t)s * B + b) * R + k] : vx_gauss(seed ^ 0x5bd1e995u, (uint32_t)k, slot0 + (uint32_t)s);
  }
  __syncthreads();
  for (int64_t sp = blockIdx.x; sp < nspan; sp += gridDim.x) {
    double aLL = 0.0;
    int nTP[C], nPR[C], nT = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) nTP[c] = nPR[c] = 0;
    for (int it = 0; it < VS_SPAN / 256; ++it) {
      const int64_t v0 = sp * VS_SPAN + it * 256 + wave * 64;
      if (v0 >= nvox) break;
      const int64_t v = v0 + lane;
      const bool act = v < nvox;
      const int64_t vv = act ? v : nvox - 1;
      const vs_label l = vs_load_label(g, v, nvox, C, ignore);
      float mean[C], sd[C];
      unsigned long long bt[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        mean[c] = h[(size_t)c * nvox + vv];
        sd[c] = sqrtf(expf(h[(size_t)per + (size_t)c * nvox + vv]) + epsilon);
        bt[c] = __ballot(l.lab == c);
        if (lane == c) nT += vs_pop(bt[c]);
      }
      const int nv = vs_pop(__ballot(l.take)), ni = vs_pop(__ballot(l.inv));
      if (lane == C) nT += nv;
      if (lane == C + 1) nT += ni;
      for (int s = 0; s < S; ++s) {
        float y[C];
        double ls[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int64_t r = (int64_t)c * nvox + vv;
          float low = 0.f;
          for (int k = 0; k < R; ++k) low = fmaf(h[(size_t)(2 + k) * per + r], sew[s * R + k], low);
          const float ed = eps_d ? eps_d[((size_t)s * B + b) * per + r] : vx_gauss(seed, (uint32_t)r, slot0 + (uint32_t)s);
          y[c] = (mean[c] + low) + sd[c] * ed;   // vx_ssn_sample's expression
        }
        const int a = vs_log_softmax<C>(y, ls);
        double lt = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c)
          if (l.lab == c && l.take) lt = ls[c];
        const double tot = vs_wave_all(lt);
        if (lane == s) aLL += tot;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const unsigned long long ba = __ballot(act && a == c);
          if (lane == s) {
            nPR[c] += vs_pop(ba);
            nTP[c] += vs_pop(ba & bt[c]);
          }
        }
      }
    }
    double* rd = red + wave * KMAX;
    if (lane < S) {
      rd[lane * PS] = aLL;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        rd[lane * PS + 1 + c] = (double)nTP[c];
        rd[lane * PS + 1 + C + c] = (double)nPR[c];
      }
    }
    if (lane < C + 2) rd[S * PS + lane] = (double)nT;
    vs_flush(red, KMAX, K, part + ((size_t)b * nspan + sp) * K);
  }
}

// ---- the 2D SSN head (HighResolutionNet.hrnet_ssn) ---------------------------------------------------------------------------------
// The head lives at 1/4 resolution, channels-last.  ssn2d_lowres_kernel (accumulate.hip) has left comb [S][B * h0 * w0][C] and
// expm [B * h0 * w0][C] in the workspace; a thread owns one FULL-resolution pixel and forms its S x C sample logits as
// LowRankNormal2D.sample_images does, expression for expression (bilinear_nchw_kernel's interpolation, ssn2d_add_diag_kernel's
// diagonal term), so the very float32 values that route writes are reduced here without being written:
//     sd_c = sqrtf(interp(expm)_c + epsilon),   y_s,c = interp(comb_s)_c + sd_c * eps_d
// The four low-resolution pixels of a thread are shared with its neighbours (16 full-resolution pixels per source pixel at the
// shipped 1/4) and stay in L1 / L2.  CT > 0: the class count is a template constant and a pixel's C logits and C standard
// deviations are register arrays.  CT == 0 (any C up to 32): two sweeps over the classes per sample -- maximum, arg-max and
// the label's logit, then the sum of exponentials -- each re-evaluating y_s,c from the four source pixels, so nothing is
// indexed by a runtime class and nothing lands in scratch (bn2d.hip records what a 32-wide register array cost).
// Accumulation: lane s keeps sample s's float64 log-term sum (butterfly, as above).  The counts do not go through
// per-class registers (2 C of them per lane, 38 at the shipped C = 19): a wave walks the DISTINCT arg-max classes of its 64
// pixels (ballot, popcount) and lane 0 adds each count into the workgroup's LDS table with an integer atomic -- integer adds
// commute, so the table does not depend on the order.  Partial row as val_ssn_kernel's.
template <int CT>
__global__ __launch_bounds__(256) void val_ssn2d_kernel(const float* __restrict__ comb, const float* __restrict__ expm,
                                                        const float* __restrict__ eps_d, uint32_t seed, uint32_t item0,
                                                        const uint8_t* __restrict__ labels, int B, int S, int Crt, int h0, int w0, int H,
                                                        int W, float epsilon, int ignore, int64_t nspan, double* __restrict__ part) {
  const int C = CT ? CT : Crt;
  __shared__ double sll[4 * VS_MAXS];                                // [wave][s]
  __shared__ unsigned cnt[VS_MAXS * 2 * VS_MAXC + VS_MAXC + 2];      // [s][tp_c | pred_c], then #[t = c] | valid | invalid
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, PS = 1 + 2 * C, K = S * PS + C + 2, NC = S * 2 * C + C + 2;
  const uint32_t nvox = (uint32_t)H * (uint32_t)W;                   // C * nvox < 2^32 (host check)
  const size_t per = (size_t)C * nvox;
  const size_t pix = (size_t)h0 * w0, PC = (size_t)B * pix * C;      // floats of one sample's comb
  const float ry = (float)h0 / (float)H, rx = (float)w0 / (float)W;
  const uint8_t* g = labels + (size_t)b * nvox;
  const uint32_t slot0 = (item0 + (uint32_t)b) * (uint32_t)S;
  for (int64_t sp = blockIdx.x; sp < nspan; sp += gridDim.x) {
    for (int i = tid; i < NC; i += 256) cnt[i] = 0u;
    __syncthreads();
    double aLL = 0.0;
    const int64_t v0 = sp * VS_SPAN + wave * 64;
    if (v0 < (int64_t)nvox) {   // else the whole wave is past the end
      const int64_t v = v0 + lane;
      const bool act = v < (int64_t)nvox;
      const uint32_t vv = act ? (uint32_t)v : nvox - 1u;
      const vs_label l = vs_load_label(g, v, nvox, C, ignore);
      if (act && l.lab < C) atomicAdd(&cnt[S * 2 * C + l.lab], 1u);
      const int nv = vs_pop(__ballot(l.take)), ni = vs_pop(__ballot(l.inv));
      if (lane == 0) {
        atomicAdd(&cnt[S * 2 * C + C], (unsigned)nv);
        atomicAdd(&cnt[S * 2 * C + C + 1], (unsigned)ni);
      }
      const int oy = (int)(vv / (uint32_t)W), ox = (int)(vv - (uint32_t)oy * (uint32_t)W);
      int y0, y1, x0, x1;
      float ly, lx;
      bil_coord(oy, h0, ry, y0, y1, ly);
      bil_coord(ox, w0, rx, x0, x1, lx);
      const float hy = 1.f - ly, hx = 1.f - lx;
      const size_t o00 = ((size_t)b * pix + (size_t)y0 * w0 + x0) * C, o01 = ((size_t)b * pix + (size_t)y0 * w0 + x1) * C;
      const size_t o10 = ((size_t)b * pix + (size_t)y1 * w0 + x0) * C, o11 = ((size_t)b * pix + (size_t)y1 * w0 + x1) * C;
      // bilinear_nchw_kernel's expression on the four source pixels at p + o00 .. p + o11
      auto interp = [&](const float* p, int c) {
        return hy * (hx * p[o00 + c] + lx * p[o01 + c]) + ly * (hx * p[o10 + c] + lx * p[o11 + c]);
      };
      auto sdev = [&](int c) { return sqrtf(interp(expm, c) + epsilon); };
      float sd[CT ? CT : 1];
      if constexpr (CT > 0) {
#pragma unroll
        for (int c = 0; c < CT; ++c) sd[c] = sdev(c);
      }
      for (int s = 0; s < S; ++s) {
        const float* cs = comb + (size_t)s * PC;
        const float* ed = eps_d ? eps_d + ((size_t)s * B + b) * per + vv : nullptr;
        const uint32_t slot = slot0 + (uint32_t)s;
        // ssn2d_add_diag_kernel's expression: the upsampled combination + sd * eps_d
        auto logit = [&](int c, float sdc) {
          const float e = ed ? ed[(size_t)c * nvox] : vx_gauss(seed, (uint32_t)c * nvox + vv, slot);
          return interp(cs, c) + sdc * e;
        };
        float mx, yt = 0.f;
        int a = 0;
        double se = 0.0;
        if constexpr (CT > 0) {
          float y[CT];
#pragma unroll
          for (int c = 0; c < CT; ++c) y[c] = logit(c, sd[c]);
          mx = y[0];
#pragma unroll
          for (int c = 1; c < CT; ++c)
            if (y[c] > mx) { mx = y[c]; a = c; }
          const double m = (double)mx;
#pragma unroll
          for (int c = 0; c < CT; ++c) {
            se += exp((double)y[c] - m);
            if (l.lab == c) yt = y[c];
          }
        } else {
          mx = logit(0, sdev(0));
          if (l.lab == 0) yt = mx;
          for (int c = 1; c < C; ++c) {
            const float yc = logit(c, sdev(c));
            if (yc > mx) { mx = yc; a = c; }
            if (l.lab == c) yt = yc;
          }
          const double m = (double)mx;
          for (int c = 0; c < C; ++c) se += exp((double)logit(c, sdev(c)) - m);
        }
        const double lt = l.take ? ((double)yt - (double)mx) - log(se) : 0.0;
        const double tot = vs_wave_all(lt);
        if (lane == s) aLL += tot;
        // the distinct arg-max classes of the wave's pixels
        const bool hit = a == l.lab;
        unsigned long long rem = __ballot(act);
        while (rem) {
          const int c = __builtin_amdgcn_readlane(a, __ffsll((long long)rem) - 1);
          const unsigned long long ba = __ballot(act && a == c), bh = __ballot(act && a == c && hit);
          if (lane == 0) {
            atomicAdd(&cnt[s * 2 * C + C + c], (unsigned)vs_pop(ba));
            if (bh) atomicAdd(&cnt[s * 2 * C + c], (unsigned)vs_pop(bh));
          }
          rem &= ~ba;
        }
      }
    }
    if (lane < S) sll[wave * VS_MAXS + lane] = aLL;
    __syncthreads();
    double* row = part + ((size_t)b * nspan + sp) * K;
    for (int k = tid; k < K; k += 256) {
      if (k < S * PS) {
        const int s = k / PS, j = k - s * PS;
        row[k] = j == 0 ? ((sll[s] + sll[VS_MAXS + s]) + sll[2 * VS_MAXS + s]) + sll[3 * VS_MAXS + s] : (double)cnt[s * 2 * C + j - 1];
      } else {
        row[k] = (double)cnt[S * 2 * C + (k - S * PS)];
      }
    }
    __syncthreads();
  }
}

// out[b][k] = the span partials of item b: a wave per output, lane l adds the spans l, l + 64, ... in ascending order, the lanes
// meet in the butterfly; row entries k >= K1 go to out2[b][k - K1]
__global__ __launch_bounds__(256) void val_final_kernel(const double* __restrict__ part, int64_t n, int K, int K1, int64_t nspan,
                                                        double* __restrict__ out1, double* __restrict__ out2) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;   // the whole wave
  const int64_t b = i / K;
  const int k = (int)(i - b * K);
  const double* p = part + (size_t)b * nspan * K + k;
  double s = 0.0;
  for (int64_t sp = lane; sp < nspan; sp += 64) s += p[(size_t)sp * K];
  s = vs_wave_all(s);
  if (lane == 0) {
    if (k < K1) out1[b * K1 + k] = s;
    else out2[b * (K - K1) + (k - K1)] = s;
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static int64_t vs_workspace(int B, int64_t K, int64_t nvox) {
  const int64_t nspan = (nvox + VS_SPAN - 1) / VS_SPAN;            // <= 2^31
  return (int64_t)B * nspan * K * (int64_t)sizeof(double);         // B < 2^16, K < 2^10, 8: < 2^60
}
static bool vs_common_ok(int B, int64_t nvox, int ignore) { return B >= 1 && B <= VS_MAXB && nvox >= 1 && nvox <= VS_MAXVOX && ignore >= -1 && ignore <= 255; }
static bool vs_plain_ok(int B, int C, int64_t nvox) { return vs_common_ok(B, nvox, -1) && C >= 1 && C <= VS_MAXC; }
static bool vs_al_ok(int B, int C, int64_t nvox) {
  return vs_common_ok(B, nvox, -1) && C >= VS_MINCS && C <= VS_MAXCS && (int64_t)C * nvox < ((int64_t)1 << 32);
}
static bool vs_ssn_ok(int B, int C, int S, int64_t nvox) { return vs_al_ok(B, C, nvox) && S >= 1 && S <= VS_MAXS; }

static int vs_finalize(const double* part, int B, int K, int K1, int64_t nspan, double* out1, double* out2, hipStream_t s, const char* who) {
  const int64_t n = (int64_t)B * K, fb = (n + 3) / 4;   // < 2^16 * 2^10
  hipLaunchKernelGGL(val_final_kernel, dim3((unsigned)fb), dim3(256), 0, s, part, n, K, K1, nspan, out1, out2);
  VX_CHECK_LAUNCH(who);
  return VX_OK;
}

extern "C" int64_t vx_val_sums_workspace_bytes(int B, int C, int64_t nvox) {
  return vs_plain_ok(B, C, nvox) ? vs_workspace(B, 5 * C + 3, nvox) : 0;
}

extern "C" int vx_val_sums_batched(const float* logits, const uint8_t* labels, int B, int C, int64_t nvox, int ignore_label,
                                   double* sums, void* workspace, int64_t workspace_bytes, vx_stream_t stream) {
  if (!vs_plain_ok(B, C, nvox) || !vs_common_ok(B, nvox, ignore_label))
    VX_FAIL(VX_E_SHAPE, "vx_val_sums_batched: B=%d (1..%d) C=%d (1..%d) nvox=%lld (1..2^39) ignore_label=%d (-1..255)", B, VS_MAXB, C,
            VS_MAXC, (long long)nvox, ignore_label);
  if (!logits || !labels || !sums || !workspace) VX_FAIL(VX_E_NULL, "vx_val_sums_batched: null pointer");
  if (workspace_bytes < vx_val_sums_workspace_bytes(B, C, nvox))
    VX_FAIL(VX_E_WORKSPACE, "vx_val_sums_batched: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
            (long long)vx_val_sums_workspace_bytes(B, C, nvox));
  hipStream_t s = (hipStream_t)stream;
  const int64_t nspan = (nvox + VS_SPAN - 1) / VS_SPAN;
  const dim3 grid((unsigned)(nspan < VS_MAXGRID ? nspan : VS_MAXGRID), (unsigned)B);
  hipLaunchKernelGGL(val_sums_kernel, grid, dim3(256), 0, s, logits, labels, C, nvox, ignore_label, nspan, (double*)workspace);
  const int K = 5 * C + 3;
  return vs_finalize((const double*)workspace, B, K, K, nspan, sums, sums, s, "vx_val_sums_batched");
}

extern "C" int64_t vx_val_aleatoric_sums_workspace_bytes(int B, int C, int64_t nvox) {
  return vs_al_ok(B, C, nvox) ? vs_workspace(B, 5 * C + 3, nvox) : 0;
}

extern "C" int vx_val_aleatoric_sums_batched(const float* mu_s, const float* eps, uint32_t seed, uint32_t item0, const uint8_t* labels,
                                             int B, int T, int C, int64_t nvox, int ignore_label, double* sums, void* workspace,
                                             int64_t workspace_bytes, vx_stream_t stream) {
  if (!vs_al_ok(B, C, nvox) || !vs_common_ok(B, nvox, ignore_label) || T < 1 || T > VS_MAXS)
    VX_FAIL(VX_E_SHAPE,
            "vx_val_aleatoric_sums_batched: B=%d (1..%d) T=%d (1..%d) C=%d (%d..%d) nvox=%lld (>= 1, C * nvox < 2^32) ignore_label=%d (-1..255)",
            B, VS_MAXB, T, VS_MAXS, C, VS_MINCS, VS_MAXCS, (long long)nvox, ignore_label);
  if (!mu_s || !labels || !sums || !workspace) VX_FAIL(VX_E_NULL, "vx_val_aleatoric_sums_batched: null pointer");
  if (workspace_bytes < vx_val_aleatoric_sums_workspace_bytes(B, C, nvox))
    VX_FAIL(VX_E_WORKSPACE, "vx_val_aleatoric_sums_batched: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
            (long long)vx_val_aleatoric_sums_workspace_bytes(B, C, nvox));
  hipStream_t s = (hipStream_t)stream;
  const int64_t nspan = (nvox + VS_SPAN - 1) / VS_SPAN;
  const dim3 grid((unsigned)(nspan < VS_MAXGRID ? nspan : VS_MAXGRID), (unsigned)B);
  const double logT = log((double)T);
#define VS_AL(CC)                                                                                                                       \
  case CC:                                                                                                                              \
    hipLaunchKernelGGL(val_aleatoric_kernel<CC>, grid, dim3(256), 0, s, mu_s, eps, seed, item0, labels, T, logT, nvox, ignore_label, nspan, \
                       (double*)workspace);                                                                                             \
    break;
  switch (C) { VS_AL(2) VS_AL(3) VS_AL(4) VS_AL(5) VS_AL(6) VS_AL(7) VS_AL(8) }
#undef VS_AL
  const int K = 5 * C + 3;
  return vs_finalize((const double*)workspace, B, K, K, nspan, sums, sums, s, "vx_val_aleatoric_sums_batched");
}

extern "C" int64_t vx_val_ssn_sums_workspace_bytes(int B, int S, int C, int64_t nvox) {
  return vs_ssn_ok(B, C, S, nvox) ? vs_workspace(B, (int64_t)S * (1 + 2 * C) + C + 2, nvox) : 0;
}

extern "C" int vx_val_ssn_sums_batched(const float* head, const float* eps_w, const float* eps_d, uint32_t seed, uint32_t item0,
                                       const uint8_t* labels, int B, int S, int C, int R, int64_t nvox, float epsilon, int ignore_label,
                                       double* sample_sums, double* target_sums, void* workspace, int64_t workspace_bytes,
                                       vx_stream_t stream) {
  if (!vs_ssn_ok(B, C, S, nvox) || !vs_common_ok(B, nvox, ignore_label) || R < 0 || R > VS_MAXR)
    VX_FAIL(VX_E_SHAPE,
            "vx_val_ssn_sums_batched: B=%d (1..%d) S=%d (1..%d) C=%d (%d..%d) R=%d (0..%d) nvox=%lld (>= 1, C * nvox < 2^32) ignore_label=%d (-1..255)",
            B, VS_MAXB, S, VS_MAXS, C, VS_MINCS, VS_MAXCS, R, VS_MAXR, (long long)nvox, ignore_label);
  if (!head || !labels || !sample_sums || !target_sums || !workspace) VX_FAIL(VX_E_NULL, "vx_val_ssn_sums_batched: null pointer");
  if (workspace_bytes < vx_val_ssn_sums_workspace_bytes(B, S, C, nvox))
    VX_FAIL(VX_E_WORKSPACE, "vx_val_ssn_sums_batched: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
            (long long)vx_val_ssn_sums_workspace_bytes(B, S, C, nvox));
  hipStream_t s = (hipStream_t)stream;
  const int64_t nspan = (nvox + VS_SPAN - 1) / VS_SPAN;
  const dim3 grid((unsigned)(nspan < VS_MAXGRID ? nspan : VS_MAXGRID), (unsigned)B);
#define VS_SSN(CC)                                                                                                                       \
  case CC:                                                                                                                               \
    hipLaunchKernelGGL(val_ssn_kernel<CC>, grid, dim3(256), 0, s, head, eps_w, eps_d, seed, item0, labels, B, S, R, nvox, epsilon,         \
                       ignore_label, nspan, (double*)workspace);                                                                         \
    break;
  switch (C) { VS_SSN(2) VS_SSN(3) VS_SSN(4) VS_SSN(5) VS_SSN(6) VS_SSN(7) VS_SSN(8) }
#undef VS_SSN
  const int K = S * (1 + 2 * C) + C + 2;
  return vs_finalize((const double*)workspace, B, K, S * (1 + 2 * C), nspan, sample_sums, target_sums, s, "vx_val_ssn_sums_batched");
}

// ---- vx_val_ssn2d_sums_batched ---------------------------------------------------------------------------------------------------
constexpr int VS_MAXSIDE = 65536;   // h0, w0, H, W: a float32 holds (side + 0.5) exactly, as bil_coord needs
static bool vs_ssn2d_ok(int B, int S, int C, int h0, int w0, int H, int W) {
  if (B < 1 || B > VS_MAXB || S < 1 || S > VS_MAXS || C < 2 || C > VS_MAXC) return false;
  if (h0 < 1 || w0 < 1 || H < 1 || W < 1 || h0 > VS_MAXSIDE || w0 > VS_MAXSIDE || H > VS_MAXSIDE || W > VS_MAXSIDE) return false;
  // the guards of the calls this one stands for: vx_ssn2d_add_diag (C * H * W indexes the generator in 32 bits) and
  // vx_ssn2d_lowres (B * pix pixels index in 32 bits; B * S < 2^31 holds with B < 2^16, S <= 32)
  return (int64_t)C * H * W < ((int64_t)1 << 32) && (int64_t)B * h0 * w0 < ((int64_t)1 << 32);
}
// the workspace: [comb (S) | expm] floats of the low-resolution head, rounded up to 16 bytes, then the span partial rows
static int64_t vs_ssn2d_lowres_bytes(int B, int S, int C, int h0, int w0) {
  const int64_t fl = (int64_t)(S + 1) * B * h0 * w0 * C;   // 33 * 2^32 * 32 < 2^43
  return (fl * 4 + 15) / 16 * 16;
}

extern "C" int64_t vx_val_ssn2d_sums_workspace_bytes(int B, int S, int C, int h0, int w0, int H, int W) {
  if (!vs_ssn2d_ok(B, S, C, h0, w0, H, W)) return 0;
  return vs_ssn2d_lowres_bytes(B, S, C, h0, w0) + vs_workspace(B, (int64_t)S * (1 + 2 * C) + C + 2, (int64_t)H * W);
}

extern "C" int vx_val_ssn2d_sums_batched(const float* mean_lo, int mean_pitch, const float* factor_lo, int factor_pitch,
                                         const float* eps_w, const float* eps_d, uint32_t seed, uint32_t item0, const uint8_t* labels,
                                         int B, int S, int C, int R, int h0, int w0, int H, int W, float epsilon, int ignore_label,
                                         double* sample_sums, double* target_sums, void* workspace, int64_t workspace_bytes,
                                         vx_stream_t stream) {
  if (!vs_ssn2d_ok(B, S, C, h0, w0, H, W) || ignore_label < -1 || ignore_label > 255 || R < 0 || R > VS_MAXR || mean_pitch < C ||
      (R > 0 && (int64_t)factor_pitch < (int64_t)R * C))
    VX_FAIL(VX_E_SHAPE,
            "vx_val_ssn2d_sums_batched: B=%d (1..%d) S=%d (1..%d) C=%d (2..%d) R=%d (0..%d) %dx%d -> %dx%d (sides 1..%d, C * H * W < 2^32, "
            "B * h0 * w0 < 2^32) mean_pitch=%d (>= C) factor_pitch=%d (>= R * C) ignore_label=%d (-1..255)",
            B, VS_MAXB, S, VS_MAXS, C, VS_MAXC, R, VS_MAXR, h0, w0, H, W, VS_MAXSIDE, mean_pitch, factor_pitch, ignore_label);
  if (!mean_lo || (R > 0 && !factor_lo) || !labels || !sample_sums || !target_sums || !workspace)
    VX_FAIL(VX_E_NULL, "vx_val_ssn2d_sums_batched: null pointer");
  const int64_t need = vx_val_ssn2d_sums_workspace_bytes(B, S, C, h0, w0, H, W);
  if (workspace_bytes < need)
    VX_FAIL(VX_E_WORKSPACE, "vx_val_ssn2d_sums_batched: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
  hipStream_t s = (hipStream_t)stream;
  const int64_t pix = (int64_t)h0 * w0, nvox = (int64_t)H * W;
  float* comb = (float*)workspace;
  float* expm = comb + (size_t)S * B * pix * C;
  double* part = (double*)((char*)workspace + vs_ssn2d_lowres_bytes(B, S, C, h0, w0));
  const int rc = vx_ssn2d_lowres_launch(mean_lo, mean_pitch, factor_lo, factor_pitch, R > 0 ? eps_w : nullptr, seed, item0, B, pix, S, C, R,
                                        comb, expm, s, "vx_val_ssn2d_sums_batched (low-resolution combination)");
  if (rc != VX_OK) return rc;
  const int64_t nspan = (nvox + VS_SPAN - 1) / VS_SPAN;
  const dim3 grid((unsigned)(nspan < VS_MAXGRID ? nspan : VS_MAXGRID), (unsigned)B);
#define VS_SSN2D(CC)                                                                                                                   \
  hipLaunchKernelGGL(val_ssn2d_kernel<CC>, grid, dim3(256), 0, s, comb, expm, eps_d, seed, item0, labels, B, S, C, h0, w0, H, W, epsilon, \
                     ignore_label, nspan, part)
  switch (C) {
    case 2: VS_SSN2D(2); break;
    case 3: VS_SSN2D(3); break;
    case 4: VS_SSN2D(4); break;
    case 19: VS_SSN2D(19); break;   // the shipped head (hrnet_config_ssn.yaml)
    default: VS_SSN2D(0); break;    // any other count: the two-sweep form
  }
#undef VS_SSN2D
  VX_CHECK_LAUNCH("vx_val_ssn2d_sums_batched");
  const int K = S * (1 + 2 * C) + C + 2;
  return vs_finalize(part, B, K, S * (1 + 2 * C), nspan, sample_sums, target_sums, s, "vx_val_ssn2d_sums_batched");
}
