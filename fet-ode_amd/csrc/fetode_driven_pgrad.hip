// fetode_driven_pgrad.hip — the parameter gradients of the input-driven Ferro field
//     dh/dt = tanh(Ferro_{(H+D)->H}(cat[h, x(t)])) * gain + bias
// summed over the taped rows of a one-launch solve (fetode_driven_fixed_tape: (n_ev, B, .) rows;
// fetode_driven_dopri5_tape: (B, max_ev, .) rows, ragged by nfev), from the reverse sweep's adj
// (DESIGN §4.20):
//   driven_pgrad_kernel    workgroup (input i, chunk of KC bases, slice of the rows): lane -> output o
//                          (lanes >= H idle), the four waves take the slice's rows in turn; a thread
//                          keeps its KC elements' constants and 3 KC running sums in registers
//   driven_pgrad_reduce_kernel  adds the slices in order and applies the per-element factors
// Row (b, e), e < min(nfev[b], n_ev), has the logical index q = b * n_ev + e whatever the tape's
// strides are; slice sp owns q in [sp R / S, (sp + 1) R / S), R = B n_ev, wave w its rows q0 + w + 4 j.
// So the summation order is a function of (B, n_ev, S) alone: the result is the same bit for bit from
// run to run and across the two tape layouts.  No atomics; no workgroup waits on another one.
// Algebra (branch sign 1: m = 1 + w s, w = -2(1-alpha)(1-u), u = sigma(gs(x - prev)) once per row,
// s = sigma(gs(-x - Ec)), sh = x + Ec m, th = tanh(k sh), g = adj gain (1 - tanh^2 phi)); the
// per-element constants leave the row sums:
//   Sk = sum g (1 - th^2) sh          d k    = coef Ps Sk
//   SE = sum g (1 - th^2)(m + Ec dm)  d Ec   = coef Ps k SE,   dm = -w gs s (1 - s)
//   A  = sum g th                     d Ps   = coef A,         d coef = Ps A + bias G
//   G  = sum g   (per output)         d bias = coef G
// which is ferro_point_vjp's algebra with bs = 1.  The element terms use the forward's exp2 / rcp
// forms on the raw Ec and k (their own expression, not fetode_driven_dev.h's plan element); the gate is
// the forward's drv_gate and the outer tanhf its precise one.
#include "fetode_driven_dev.h"

using namespace fetode;

namespace {

constexpr int kPgThreads = 256;      // four waves
constexpr int kPgChunk = 8;          // bases per workgroup of the generic-K kernel
constexpr int kPgMaxSplits = 64;     // row slices: the workspace is sized for min(this, rows / 4)
constexpr int kPgTarget = 2048;      // workgroups the automatic split aims at
constexpr int kPgRowsPerSlice = 64;  // ... with at least 16 rows per wave

struct DrivenPgArgs {
  fetode_ferro_t fl;
  const float* gain;       // (H)
  const int32_t* nfev;     // nullable: every row e < n_ev is live
  const float* prev0;      // (B, H+D) nullable: zeros
  const float* tape_hx;    // row (b, e) at (b stride_b + e stride_e) * (H+D)
  const float* tape_phi;   // ... * H
  const float* adj;        // ... * H
  float* part;             // [S][3][In K][H]: Sk, SE, A of element (i, k, o)
  float* side;             // [S][3][H]: G, sum adj tanh(phi), sum adj
  int64_t B, n_ev, stride_b, stride_e, nfev_stride;
  int32_t S, elems, sides;  // elems: the element sums are wanted; sides: the gain / bias sums are
};

// the live rows of sample b: min(nfev, n_ev), 0 for a count <= 0
__device__ __forceinline__ int64_t pg_live(const DrivenPgArgs& a, int64_t b) {
  if (!a.nfev) return a.n_ev;
  const int64_t n = a.nfev[b * a.nfev_stride];
  return n < 0 ? 0 : (n > a.n_ev ? a.n_ev : n);
}

template <int KC, bool FULL>
__global__ __launch_bounds__(kPgThreads) void driven_pgrad_kernel(DrivenPgArgs a) {
  static_assert(KC >= 3, "the side sums use three rows of red");
  __shared__ float red[3][KC][64];
  const int H = a.fl.out_dim, In = a.fl.in_dim, K = FULL ? KC : a.fl.num_basis;
  const int NC = FULL ? 1 : (K + KC - 1) / KC;
  const int i = blockIdx.x / NC, kc = blockIdx.x - i * NC, sp = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool act = lane < H;
  const int k0 = kc * KC, ne = FULL ? KC : (K - k0 < KC ? K - k0 : KC);
  const float gs = (float)a.fl.gate_slope, gs2 = gs * FETODE_LOG2E, wc = (float)(-2.0 * (1.0 - a.fl.alpha));
  const bool lead = i == 0 && kc == 0;   // these workgroups also carry G and the gain / bias sums
  float Ec[KC], GE[KC], k2[KC];
#pragma unroll
  for (int j = 0; j < KC; ++j) {
    const bool on = act && j < ne;
    const int e = (i * H + lane) * K + k0 + j;
    Ec[j] = on ? a.fl.Ec[e] : 0.f;
    GE[j] = gs2 * Ec[j];
    k2[j] = on ? 2.0f * FETODE_LOG2E * a.fl.k[e] : 0.f;
  }
  const float gain = act ? a.gain[lane] : 0.f;
  float sk[KC], sE[KC], sA[KC];
#pragma unroll
  for (int j = 0; j < KC; ++j) sk[j] = sE[j] = sA[j] = 0.f;
  float sG = 0.f, sgain = 0.f, sbias = 0.f;

  const int64_t R = a.B * a.n_ev;
  const int64_t q0 = (int64_t)sp * R / a.S, q1 = (int64_t)(sp + 1) * R / a.S;
  // this wave's rows: q = q0 + wv, q0 + wv + 4, ...; (b, e) follows q without a division per row
  int64_t q = q0 + wv;
  int64_t b = q / a.n_ev, e = q - b * a.n_ev;
  int64_t nl = q < q1 ? pg_live(a, b) : 0;
  for (; q < q1; q += 4) {
    if (e < nl) {
      const int64_t row = b * a.stride_b + e * a.stride_e;
      const float xv = a.tape_hx[row * In + i];
      const float pv = e > 0 ? a.tape_hx[(row - a.stride_e) * In + i] : (a.prev0 ? a.prev0[b * In + i] : 0.f);
      const float ad = act ? a.adj[row * H + lane] : 0.f;
      const float y = tanhf(act ? a.tape_phi[row * H + lane] : 0.f);
      const float go = (ad * gain) * (1.0f - y * y);
      sG += go;
      if (lead) {
        sgain += ad * y;
        sbias += ad;
      }
      if (a.elems) {
        const float w = drv_gate(gs, gs2, wc, xv, pv).v;   // the forward's gate (fetode_driven_dev.h)
        const float wg = -(w * gs), gx = gs2 * xv;
#pragma unroll
        for (int j = 0; j < KC; ++j) {
          const float sg = rcp(1.0f + ex2(gx + GE[j]));              // sigma(gs(-x - Ec))
          const float m = ffma(w, sg, 1.0f);
          const float sh = ffma(Ec[j], m, xv);
          const float th = ffma(rcp(1.0f + ex2(k2[j] * sh)), -2.0f, 1.0f);  // tanh(k sh)
          const float gz = go * ffma(-th, th, 1.0f);
          const float dm = wg * (sg * (1.0f - sg));                  // d m / d Ec
          sk[j] = ffma(gz, sh, sk[j]);
          sE[j] = ffma(gz, ffma(Ec[j], dm, m), sE[j]);
          sA[j] = ffma(go, th, sA[j]);
        }
      }
    }
    e += 4;
    if (e >= a.n_ev) {           // at most four samples further (n_ev >= 1)
      do {
        e -= a.n_ev;
        ++b;
      } while (e >= a.n_ev);
      nl = q + 4 < q1 ? pg_live(a, b) : 0;
    }
  }

  // the four waves' sums meet in LDS, added in wave order; every thread reaches every barrier
  float* __restrict__ part = a.part + (int64_t)sp * 3 * In * K * H;
  auto meet = [&](float (&v)[KC], int c) {
    if (wv > 0) {
#pragma unroll
      for (int j = 0; j < KC; ++j) red[wv - 1][j][lane] = v[j];
    }
    __syncthreads();
    if (wv == 0 && act) {
#pragma unroll
      for (int j = 0; j < KC; ++j)
        if (j < ne)
          part[((int64_t)c * In * K + (int64_t)i * K + k0 + j) * H + lane] =
              ((v[j] + red[0][j][lane]) + red[1][j][lane]) + red[2][j][lane];
    }
    __syncthreads();
  };
  if (a.elems) {
    meet(sk, 0);
    meet(sE, 1);
    meet(sA, 2);
  }
  if (lead) {   // uniform over the workgroup
    if (wv > 0) {
      red[wv - 1][0][lane] = sG;
      red[wv - 1][1][lane] = sgain;
      red[wv - 1][2][lane] = sbias;
    }
    __syncthreads();
    if (wv == 0 && act) {
      float* __restrict__ sd = a.side + (int64_t)sp * 3 * H;
      sd[lane] = ((sG + red[0][0][lane]) + red[1][0][lane]) + red[2][0][lane];
      if (a.sides) {
        sd[H + lane] = ((sgain + red[0][1][lane]) + red[1][1][lane]) + red[2][1][lane];
        sd[2 * H + lane] = ((sbias + red[0][2][lane]) + red[1][2][lane]) + red[2][2][lane];
      }
    }
  }
}

// the slices in order; thread t < In K H: element (i, k, o) = (t / (K H), (t / H) % K, t % H);
// threads In K H + o: gain / bias of output o
__global__ __launch_bounds__(256) void driven_pgrad_reduce_kernel(DrivenPgArgs a, fetode_ferro_grad_t gr,
                                                                 float* __restrict__ g_gain,
                                                                 float* __restrict__ g_bias) {
  const int H = a.fl.out_dim, In = a.fl.in_dim, K = a.fl.num_basis;
  const int64_t nE = (int64_t)In * K * H;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nE) {
    if (!a.elems) return;
    const int o = (int)(t % H), k = (int)((t / H) % K), i = (int)(t / ((int64_t)H * K));
    float v[3] = {0.f, 0.f, 0.f}, G = 0.f;
    for (int sp = 0; sp < a.S; ++sp) {
      const float* __restrict__ p = a.part + (int64_t)sp * 3 * nE + t;
      v[0] += p[0];
      v[1] += p[nE];
      v[2] += p[2 * nE];
      G += a.side[(int64_t)sp * 3 * H + o];
    }
    const int e = (i * H + o) * K + k;
    const float co = a.fl.coef[e], Ps = a.fl.Ps[e];
    if (gr.k) gr.k[e] = (co * Ps) * v[0];
    if (gr.Ec) gr.Ec[e] = ((co * Ps) * a.fl.k[e]) * v[1];
    if (gr.Ps) gr.Ps[e] = co * v[2];
    if (gr.bias) gr.bias[e] = co * G;
    if (gr.coef) gr.coef[e] = ffma(Ps, v[2], a.fl.bias[e] * G);
  } else if (t < nE + H && a.sides) {
    const int o = (int)(t - nE);
    float vg = 0.f, vb = 0.f;
    for (int sp = 0; sp < a.S; ++sp) {
      vg += a.side[(int64_t)sp * 3 * H + H + o];
      vb += a.side[(int64_t)sp * 3 * H + 2 * H + o];
    }
    if (g_gain) g_gain[o] = vg;
    if (g_bias) g_bias[o] = vb;
  }
}

// K = 10 and 12 whole in one workgroup, any other K in chunks of kPgChunk bases
const DrvKRow<DrivenPgArgs> kPgrad = {driven_pgrad_kernel<10, true>, driven_pgrad_kernel<12, true>,
                                      driven_pgrad_kernel<kPgChunk, false>};

int g_splits = 0;  // forced row split (0: from the shape)

// the largest split a launch over R rows uses, forced or not: the workspace is sized for it
int pg_max_splits(int64_t R) {
  const int64_t c = R / 4;
  return c < 1 ? 1 : (c > kPgMaxSplits ? kPgMaxSplits : (int)c);
}

int pg_chunks(int K) { return (K == 10 || K == 12) ? 1 : (K + kPgChunk - 1) / kPgChunk; }

int pg_splits(const fetode_ferro_t* fl, int64_t R) {
  const int cap = pg_max_splits(R);
  if (g_splits) return g_splits < cap ? g_splits : cap;
  int64_t S = kPgTarget / ((int64_t)fl->in_dim * pg_chunks(fl->num_basis));
  const int64_t rs = (R + kPgRowsPerSlice - 1) / kPgRowsPerSlice;
  if (S > rs) S = rs;
  return S < 1 ? 1 : (S > cap ? cap : (int)S);
}

int64_t pg_split_floats(const fetode_ferro_t* fl) {
  return 3 * ((int64_t)fl->in_dim * fl->num_basis * fl->out_dim + fl->out_dim);
}

}  // namespace

extern "C" {

int fetode_driven_param_grad_set_splits(int s) {
  const int prev = g_splits;
  if (s >= 0 && s <= kPgMaxSplits) g_splits = s;
  return prev;
}

int64_t fetode_driven_param_grad_workspace(const fetode_ferro_t* basis, int64_t B, int64_t n_ev) {
  if (!fetode_driven_supported(basis)) {
    set_err(FETODE_EUNSUPPORTED, "driven parameter gradients: shape outside the admitted family");
    return -1;
  }
  const int64_t R = (B > 0 && n_ev > 0) ? B * n_ev : 0;
  return (int64_t)sizeof(float) * pg_max_splits(R) * pg_split_floats(basis);
}

int fetode_driven_param_grad(const fetode_ferro_t* basis, const float* gain, int64_t B, int64_t n_ev, int64_t stride_b,
                             int64_t stride_e, const int32_t* nfev, int64_t nfev_stride, const float* prev0,
                             const float* tape_hx, const float* tape_phi, const float* adj,
                             const fetode_ferro_grad_t* grads, float* g_gain, float* g_bias, void* workspace,
                             void* stream) {
  if (!fetode_driven_supported(basis))
    return set_err(FETODE_EUNSUPPORTED, "driven parameter gradients: shape outside the admitted family");
  if (B <= 0 || n_ev <= 0) return FETODE_OK;
  const bool elems = grads && (grads->k || grads->Ec || grads->Ps || grads->bias || grads->coef);
  const bool sides = g_gain || g_bias;
  if (!gain || !tape_hx || !tape_phi || !adj || ((elems || sides) && !workspace))
    return set_err(FETODE_EINVAL, "driven parameter gradients: null pointer");
  if (stride_b < 1 || stride_e < 1 || (nfev && nfev_stride < 1))
    return set_err(FETODE_EINVAL, "driven parameter gradients: strides must be positive");
  if (elems && (!basis->k || !basis->Ec || !basis->Ps || !basis->bias || !basis->coef))
    return set_err(FETODE_EINVAL, "driven parameter gradients: null parameter pointer");
  if (!elems && !sides) return FETODE_OK;
  if (B > INT64_MAX / n_ev) return set_err(FETODE_EUNSUPPORTED, "driven parameter gradients: too many rows");
  hipStream_t st = (hipStream_t)stream;
  const int H = basis->out_dim, In = basis->in_dim, K = basis->num_basis;
  DrivenPgArgs a{};
  a.fl = *basis;
  a.gain = gain; a.nfev = nfev; a.prev0 = prev0; a.tape_hx = tape_hx; a.tape_phi = tape_phi; a.adj = adj;
  a.B = B; a.n_ev = n_ev; a.stride_b = stride_b; a.stride_e = stride_e; a.nfev_stride = nfev_stride;
  a.S = pg_splits(basis, B * n_ev);
  a.elems = elems ? 1 : 0;
  a.sides = sides ? 1 : 0;
  a.part = (float*)workspace;
  a.side = a.part + (int64_t)a.S * 3 * In * K * H;
  // without element sums only the workgroups of input 0 (chunk 0) have anything to do
  const dim3 grid(elems ? (unsigned)(In * pg_chunks(K)) : 1u, (unsigned)a.S);
  drv_launch(kPgrad, K, grid, kPgThreads, st, a);
  LAUNCH_CHECK();
  const fetode_ferro_grad_t none{};
  const int64_t nt = (int64_t)In * K * H + H;
  hipLaunchKernelGGL(driven_pgrad_reduce_kernel, dim3(nblk(nt, 256)), dim3(256), 0, st, a, grads ? *grads : none,
                     g_gain, g_bias);
  LAUNCH_CHECK();
  return FETODE_OK;
}

}  // extern "C"
