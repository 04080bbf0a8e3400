// fetode_dopri_bwd_body.h — the function body of the resident dopri5 reverse sweep, included (not
// called) by its two __global__ functions in fetode_bwd.hip: dopri_bwd_kernel (MP = false) and the
// multi-pass sweep dopri_bwd_mp_kernel (MP = true).  In scope at the point of inclusion: the kernel
// argument `DopriBwdArgs da` and the compile-time values D, H, K, NB, NG, FERRO, TPW, MP.  Textual
// sharing keeps dopri_bwd_kernel's code exactly what it was as a function of its own.
  const BwdArgs& a = da.b;
  using L0 = BL<D, H, K, NB, NG, FERRO>;
  using L1 = BL<H, D, K, NB, NG, FERRO>;
  constexpr int W = D + H, NS = NG - 1 - kSO, HALF = 64 / TPW;
  constexpr int CB = L0::IN * L0::NTMP > L1::IN * L1::NTMP ? L0::IN * L0::NTMP : L1::IN * L1::NTMP;
  constexpr bool PF = FERRO && 2 * W <= HALF;
  constexpr int FH = PF ? HALF / 2 : HALF, NBUF = PF ? 2 : 1;
  static_assert(W <= FH && (TPW == 1 || TPW == 2 || TPW == 4), "one lane per input of each trajectory and evaluation");
  __shared__ BInTab<W, NG, NB> TI;
  __shared__ BTab<L0> T0;
  __shared__ BTab<L1> T1;
  using FB = BFeat<W, NS, NB, PF>;
  __shared__ FB sF[kTPB][NBUF][TPW];
  __shared__ __attribute__((aligned(16))) float s_cb[kTPB][TPW][CB];
  __shared__ float s_g1[kTPB][TPW][D], s_g0[kTPB][TPW][H], s_gx[kTPB][TPW][D];
  __shared__ float s_k[kTPB][TPW][8][D], s_kb[kTPB][TPW][8][D];  // k_1..k_7 and their adjoints
  __shared__ double s_red[kTPB][2], s_res[2];
  __shared__ int s_ab;
  // the element lanes' carried adjoints, kept in LDS across the VJPs (register pressure)
  struct ElSt {
    double pd, pt;          // this attempt's d/d dt and d/d t0 terms of the outputs (+ d/d dt32 at the end)
    float yb0, yb1, dtb32;  // adjoints of the attempt's y, y1, dt32
    float ybc, fbc;         // carried: adjoints of the current y and f0
    float scb, f0bp;        // initial step: adjoint of scale, the probe's term of f0's adjoint
  };
  __shared__ ElSt s_el[kTPB][TPW][D];
  // the tableau in LDS: kernel-argument reads with constant indices would be hoisted into ~50
  // SGPRs for the whole loop (the VJP needs the SGPR file)
  __shared__ float s_beta[6][6], s_cerr[8], s_cmid[8];
  // the wave-uniform control scalars, per wave in LDS: they are touched once per attempt and would
  // otherwise hold registers across every VJP (adjoints of the next dt and of t1s, ...)
  struct WSc {
    double dtbar, tbar, dtb_base, h0b, d0b, d1b;
    float dt32, h0f;
    int jj, acc;
  };
  __shared__ WSc s_sc[MP ? 2 * kTPB : kTPB];   // MP: + the segment-start snapshots (s_sc0)
  // the arguments the per-attempt code reads, in LDS: read from the kernel arguments inside the
  // loop they would be hoisted into SGPRs (and spilled) for the whole sweep
  struct RareArgs {
    const double* att;
    const double* t;
    const float* gsol;
    float* gy0;
    const double* init_rec;
    int64_t B;
    int base, n_att;
    float rtol, atol;
    double n_el, safety, ifactor, dfactor, min_step, max_step;
  };
  __shared__ RareArgs s_ra;

  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tt = lane / HALF, sl = lane % HALF;
  const int fb = sl / FH, fsl = sl % FH;
  TI.stage(a.plan, a.P0, a.P1, D, threadIdx.x, 64 * kTPB);
  T0.stage(a.k0, a.f0, a.plan, a.P0, threadIdx.x, 64 * kTPB);
  T1.stage(a.k1, a.f1, a.plan, a.P1, threadIdx.x, 64 * kTPB);
  BReg<L0> R0;
  BReg<L1> R1;
  R0.zero();
  R1.zero();
  if (threadIdx.x == 0) {
    s_ab = 0;
    s_ra = RareArgs{da.att, da.t, a.gsol, a.gy0, da.init_rec, a.B, da.base, da.n_att, da.rtol, da.atol,
                    da.n_el, da.step.safety, da.step.ifactor, da.step.dfactor, da.step.min_step, da.step.max_step};
#pragma unroll
    for (int q = 0; q < 36; ++q) s_beta[q / 6][q % 6] = da.beta[q / 6][q % 6];
#pragma unroll
    for (int q = 0; q < 7; ++q) {
      s_cerr[q] = da.cerr[q];
      s_cmid[q] = da.cmid[q];
    }
  }
  __syncthreads();

  float* cbs = &s_cb[wid][0][0];
  float* g1s = &s_g1[wid][0][0];
  float* g0s = &s_g0[wid][0][0];
  float* gxs = &s_gx[wid][0][0];
  float(&kk)[8][D] = s_k[wid][tt];
  float(&kb)[8][D] = s_kb[wid][tt];
  const float gs0 = (float)a.f0.gate_slope, gs1 = (float)a.f1.gate_slope;
  const float gl0 = a.P0.gsl2e, gl1 = a.P1.gsl2e, wc0 = a.P0.wc, wc1 = a.P1.wc;
  const float glane = fsl < D ? gl0 : gl1, wlane = fsl < D ? wc0 : wc1, slane = fsl < D ? gs0 : gs1;
  constexpr int TW = 2 * D + H;  // tape row: layer-0 input, layer-1 input, output k
  const int64_t tstride = a.B * TW;
  const int n_ev = da.n_ev;
  // (MP: rebound per virtual workgroup, mp_bind below; constants of the one-grid sweep)
  typename std::conditional<MP, int64_t, const int64_t>::type b0 = ((int64_t)blockIdx.x * kTPB + wid) * TPW;
  typename std::conditional<MP, int64_t, const int64_t>::type b = b0 + tt;
  typename std::conditional<MP, bool, const bool>::type live = b < a.B;
  typename std::conditional<MP, bool, const bool>::type el = live && sl < D;  // this lane carries element (b, sl)
  // per-lane offsets in 32 bits, row bases uniform (scalar base + vector offset addressing)
  typename std::conditional<MP, int, const int>::type bi = live ? (int)b : 0;
  // MP: the first evaluation of the segment (the evaluations between two grid sums) being walked;
  // the feature phase pairs evaluations from there
  typename std::conditional<MP, int, const int>::type seg_top = n_ev - 1;
  auto tape_at = [&](int ev) -> float {
    if (fsl >= W || !live) return 0.f;
    if (ev >= 0) return (a.tape + (int64_t)ev * tstride)[bi * TW + fsl];
    const float v = a.tape[bi * TW + fsl];
    if (fsl < D) return (a.init_mask & 1u) ? v : (FERRO ? a.state0[bi * D + fsl] : 0.f);
    return (a.init_mask & 2u) ? v : (FERRO ? (a.state0 + a.B * D)[bi * H + (fsl - D)] : 0.f);
  };
  auto tx = [&](int ev) -> float { return (a.tape + (int64_t)ev * tstride)[bi * TW + sl]; };      // layer input (el lanes)
  auto tk = [&](int ev) -> float { return (a.tape + (int64_t)ev * tstride)[bi * TW + W + sl]; };  // output (el lanes)
  float cur = tape_at(n_ev - 1 - fb), prv = tape_at(n_ev - 2 - fb);

  // the VJP of evaluation ev: g1s (d loss / d k) -> gxs (d loss / d layer-0 input); sums into R0, R1
  auto vjp = [&](int ev) {
    int z = 0;
    asm volatile("" : "+s"(z));
    const bool fstep = !PF || (((MP ? seg_top : n_ev - 1) - ev) & 1) == 0;
    float nx1 = 0.f, nx2 = 0.f;
    FB& FF = sF[wid][PF ? (ev - fb) & 1 : 0][tt];
    if (fstep) {
      if constexpr (PF) {
        nx1 = tape_at(ev - fb - 2);
        nx2 = tape_at(ev - fb - 3);
      } else {
        nx1 = prv;
        nx2 = tape_at(ev - 2);
      }
      if (fsl < W) {
        FF.x[fsl] = cur;
        FF.pv[fsl] = prv;
      }
    }
    wsync();
    if (fstep) {
      if (fsl < W) feat_input<W, NG, NB, PF>(FF, TI, fsl, glane, wlane, slane, z);
      constexpr int NSG = TPW * W * NB, RSG = (NSG + 63) / 64;
#pragma unroll
      for (int pb = 0; pb < NBUF; ++pb) {
        FB* Fp = sF[wid][pb];
        float sa[RSG], sb[RSG], sx[RSG];
#pragma unroll
        for (int k = 0; k < RSG; ++k) {
          const int q = lane + 64 * k, qc = q < NSG ? q : 0;
          const int qt = qc / (W * NB), qq = qc % (W * NB);
          const float2 ab = *reinterpret_cast<const float2*>(&TI.lg[2 * qq + z]);
          sa[k] = ab.x;
          sb[k] = ab.y;
          sx[k] = Fp[qt].x[qq / NB];
        }
#pragma unroll
        for (int k = 0; k < RSG; ++k) {
          const int q = lane + 64 * k;
          if (q < NSG) {
            const int qt = q / (W * NB), qq = q % (W * NB);
            Fp[qt].sg[qq] = sigm_l2(ffma(sa[k], sx[k], sb[k]));
          }
        }
      }
      wsync();
      cur = nx1;
      prv = nx2;
    }
    FB* Fs = sF[wid][PF ? ev & 1 : 0];
    layer_jobs<L1, D, true, TPW, D, CB>(Fs, g1s, T1, TI.rh, R1, cbs, gl1, wc1, gs1, lane, z);
    wsync();
    reduce_gin<L1, TPW, H, CB>(cbs, g0s, lane);
    wsync();
    layer_jobs<L0, 0, true, TPW, H, CB>(Fs, g0s, T0, TI.rh, R0, cbs, gl0, wc0, gs0, lane, z);
    wsync();
    reduce_gin<L0, TPW, D, CB>(cbs, gxs, lane);
    wsync();
  };

  // grid-wide fixed-order sum of two per-lane fp64 values (every workgroup gets the same result)
  unsigned round = 0;
  auto gsum = [&](double v0, double v1, double& s0, double& s1) {
    v0 = xor_sum64(v0);
    v1 = xor_sum64(v1);
    if (lane == 0) {
      s_red[wid][0] = v0;
      s_red[wid][1] = v1;
    }
    __syncthreads();
    if (wid == 0) {
      double u0 = s_red[0][0], u1 = s_red[0][1];
#pragma unroll
      for (int w = 1; w < kTPB; ++w) {
        u0 += s_red[w][0];
        u1 += s_red[w][1];
      }
      double r0 = 0.0, r1 = 0.0;
      const bool ab = grid_sum2(da.gp, round, u0, u1, r0, r1);
      if (lane == 0) {
        s_res[0] = r0;
        s_res[1] = r1;
        if (ab) s_ab = 1;
      }
    }
    __syncthreads();
    s0 = s_res[0];
    s1 = s_res[1];
  };

  ElSt& E = s_el[wid][tt][sl < D ? sl : 0];  // written by lanes sl < D only
  if (sl < D) {
    E.ybc = E.fbc = 0.f;
    E.scb = E.f0bp = 0.f;
  }
  // wave-uniform scalars (SGPRs): adjoints of the next dt and of t1s, this attempt's control terms
  WSc& C = s_sc[wid];  // every lane writes the same values
  C.dtbar = C.tbar = C.dtb_base = C.h0b = C.d0b = C.d1b = 0.0;
  C.jj = a.T - 1;  // the last output not yet taken
  C.dt32 = C.h0f = 0.f;
  C.acc = 0;

  // ---- multi-pass (MP, fetode_dopri5_set_multipass): the grid is smaller than the batch needs ----
  // Physical workgroup p stands for the virtual workgroups vwg = p, p + gridDim.x, ... (< VG), vwg
  // being the workgroup dopri_bwd_kernel would run for trajectories kTPB TPW vwg ...  The evaluations
  // between two grid sums (a segment: an attempt's six, the probe, f(y0)) are walked for each virtual
  // workgroup in turn.  A virtual wave carries ElSt and its gradient sums R0 / R1 across a sum: both
  // are parked raw (mp_el, mp_r), so every sum keeps the association of the one-grid sweep and the
  // virtual wave's row of partial sums is bitwise that sweep's.  The control scalars C start every
  // virtual workgroup's segment from the same snapshot (they are the same for the whole grid); the
  // terms a grid sum feeds are applied once, after the segment's poll.
  WSc* s_sc0 = &s_sc[MP ? kTPB : 0];
  const unsigned VG = (unsigned)da.gp.nblk_global;
  unsigned vwg = blockIdx.x;
  bool mp_early = false;   // (test knob: grid_sum2_arrive's sample at the round's last arrival; wave 0)
  constexpr int NRW = BReg<L0>::NW + BReg<L1>::NW;
  ElSt* mp_el = reinterpret_cast<ElSt*>(da.gp.park);                     // (VG kTPB, TPW, D)
  float* mp_r = reinterpret_cast<float*>(mp_el + (int64_t)VG * kTPB * TPW * D);  // (VG kTPB, NRW, 64)
  // (every body under `if constexpr (MP)`: the one-grid sweep's lambdas are empty and capture nothing)
  auto mp_arrive = [&](double v0, double v1) {
   if constexpr (MP) {
    v0 = xor_sum64(v0);
    v1 = xor_sum64(v1);
    if (lane == 0) {
      s_red[wid][0] = v0;
      s_red[wid][1] = v1;
    }
    __syncthreads();
    if (wid == 0) {
      double u0 = s_red[0][0], u1 = s_red[0][1];
#pragma unroll
      for (int w = 1; w < kTPB; ++w) {
        u0 += s_red[w][0];
        u1 += s_red[w][1];
      }
      mp_early = grid_sum2_arrive(da.gp, round, vwg, u0, u1, vwg + gridDim.x >= VG);
    }
    __syncthreads();  // s_red is free for the next virtual workgroup
   }
  };
  auto mp_poll = [&](double& s0, double& s1) {
   if constexpr (MP) {
    if (wid == 0) {
      double r0 = 0.0, r1 = 0.0;
      const bool ab = grid_sum2_poll(da.gp, round, mp_early, r0, r1);
      if (lane == 0) {
        s_res[0] = r0;
        s_res[1] = r1;
        if (ab) s_ab = 1;
      }
    }
    ++round;
    __syncthreads();
    s0 = s_res[0];
    s1 = s_res[1];
   }
  };
  // serve virtual workgroup vwg from evaluation `top` (the first of a segment) on
  // the virtual wave's number as a wave-uniform value: scalar row bases + lane offsets
  auto mp_vw = [&]() -> int64_t {
    if constexpr (MP) return (int64_t)vwg * kTPB + __builtin_amdgcn_readfirstlane(wid);
    else return 0;
  };
  auto mp_bind = [&](int top) {
   if constexpr (MP) {
    b0 = ((int64_t)vwg * kTPB + wid) * TPW;
    b = b0 + tt;
    live = b < a.B;
    el = live && sl < D;
    bi = live ? (int)b : 0;
    const int64_t vw = mp_vw();
    C = s_sc0[wid];
    if (top == n_ev - 1) {
      if (sl < D) {
        E.ybc = E.fbc = 0.f;
        E.scb = E.f0bp = 0.f;
      }
      R0.zero();
      R1.zero();
    } else {
      if (sl < D) E = mp_el[(vw * TPW + tt) * D + sl];
      R0.unpark(mp_r + vw * (NRW * 64) + lane);
      R1.unpark(mp_r + vw * (NRW * 64) + BReg<L0>::NW * 64 + lane);
    }
    wsync();
    cur = tape_at(top - fb);
    prv = tape_at(top - 1 - fb);
   }
  };
  if constexpr (MP) {
    static_assert(sizeof(ElSt) == kMpElBytes, "the host sizes the parking area");
    s_sc0[wid] = C;
    wsync();
  }

  for (int ev = n_ev - 1; ev >= 0; --ev) {
    const bool in_att = ev >= s_ra.base;
    const int n = in_att ? (ev - s_ra.base) / 6 : -1, s = in_att ? 2 + (ev - s_ra.base) % 6 : 0;
    // ---------------- before the VJP: this evaluation's output adjoint ----------------
    if (in_att && s == 7) {
      const double t0 = s_ra.att[4 * n], dt = s_ra.att[4 * n + 1];
      const float ratio = (float)s_ra.att[4 * n + 2];
      C.acc = s_ra.att[4 * n + 3] != 0.0;
      int m = n - 1;  // the attempt whose stage 7 produced this attempt's y and f0
      while (m >= 0 && s_ra.att[4 * m + 3] == 0.0) --m;
      const int fe = m >= 0 ? s_ra.base + 6 * m + 5 : 0;
      const int e2 = s_ra.base + 6 * n;
      C.dt32 = ((float)dt);
      const double rr = (double)ratio;
      double rbar = 0.0, dtbb = 0.0;
      if (n + 1 < s_ra.n_att)
        dopri_next_dt_adjoint(C.dtbar, dt, s_ra.att[4 * (n + 1) + 1], rr, s_ra.ifactor, s_ra.dfactor, s_ra.min_step,
                              s_ra.max_step, dtbb, rbar);
      C.dtb_base = dtbb;
      double pd = 0.0, pt = 0.0;
      float dtb32 = 0.f, yb0, yb1;
      const float ybc = sl < D ? E.ybc : 0.f, fbc = sl < D ? E.fbc : 0.f;
      float kv[8], kbv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) kv[j] = kbv[j] = 0.f;
      float y = 0.f, y1 = 0.f;
      if (el) {
        y = tx(fe);
        kv[1] = tk(fe);
#pragma unroll
        for (int j = 2; j <= 7; ++j) kv[j] = tk(e2 + j - 2);
        y1 = tx(e2 + 5);
      }
      // err and mid in the forward's op order (fetode_fused.hip DOPRI)
      float err = kv[1] * (s_cerr[0] * C.dt32), midv = kv[1] * (s_cmid[0] * C.dt32);
#pragma unroll
      for (int j = 2; j <= 7; ++j) {
        err = err + kv[j] * (s_cerr[j - 1] * C.dt32);
        midv = midv + kv[j] * (s_cmid[j - 1] * C.dt32);
      }
      float midb = 0.f, fab;
      if (C.acc) {
        yb1 = ybc;
        kbv[7] = fbc;
        yb0 = 0.f;
        fab = 0.f;
        const float fa = kv[1], fbk = kv[7];
        float co[5];  // the forward's interpolant
        dopri_fit(co, y, y1, midv, fa, fbk, C.dt32);
        float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f, c4 = 0.f;
        const double t1 = t0 + dt, dlt = t1 - t0;
        for (; C.jj >= 1 && s_ra.t[C.jj] > t0; --C.jj) {  // outputs in (t0, t1]: uniform over the grid
          const float x = (float)((s_ra.t[C.jj] - t0) / dlt);
          const float g = el ? (s_ra.gsol + (int64_t)C.jj * a.B * D)[bi * D + sl] : 0.f;
          const float x2 = x * x, x3 = x2 * x;
          c0 += g;
          c1 += g * x;
          c2 += g * x2;
          c3 += g * x3;
          c4 += g * (x3 * x);
          const float dsdx = co[1] + 2.0f * x * co[2] + 3.0f * x2 * co[3] + 4.0f * x3 * co[4];
          const double xb = (double)(g * dsdx);
          pt += xb * (-1.0 / dlt);
          pd += xb * (-(double)x / dlt);
        }
        yb0 += ((c0 - 11.0f * c2) + 18.0f * c3) - 8.0f * c4;
        yb1 += (-5.0f * c2 + 14.0f * c3) - 8.0f * c4;
        const float ymb = (16.0f * c2 - 32.0f * c3) + 16.0f * c4;
        fab += C.dt32 * (((c1 - 4.0f * c2) + 5.0f * c3) - 2.0f * c4);
        kbv[7] += C.dt32 * ((c2 - 3.0f * c3) + 2.0f * c4);
        dtb32 += ((c1 * fa + c2 * (fbk - 4.0f * fa)) + c3 * (5.0f * fa - 3.0f * fbk)) + c4 * (2.0f * (fbk - fa));
        yb0 += ymb;
        midb = ymb;
      } else {
        yb0 = ybc;
        fab = fbc;
        yb1 = 0.f;
      }
      kbv[1] = fab;
      // error ratio = rms(err / tol): d ratio / d qe = qe / (N ratio)
      float errb = 0.f;
      if (rbar != 0.0 && ratio > 0.f) {
        const float tol = s_ra.atol + s_ra.rtol * fmaxf(fabsf(y), fabsf(y1));
        const float qe = err / tol;
        const float qb = (float)(rbar * (double)qe / (s_ra.n_el * rr));
        errb = qb / tol;
        const float tolb = -qb * qe / tol, ay = fabsf(y), ay1 = fabsf(y1);
        const float sy = y > 0.f ? 1.f : (y < 0.f ? -1.f : 0.f), sy1 = y1 > 0.f ? 1.f : (y1 < 0.f ? -1.f : 0.f);
        const float wy = ay > ay1 ? 1.f : (ay < ay1 ? 0.f : 0.5f);
        yb0 += tolb * s_ra.rtol * wy * sy;
        yb1 += tolb * s_ra.rtol * (1.f - wy) * sy1;
      }
      float se = 0.f, sm = 0.f;
#pragma unroll
      for (int j = 1; j <= 7; ++j) {
        kbv[j] += errb * (s_cerr[j - 1] * C.dt32) + midb * (s_cmid[j - 1] * C.dt32);
        se += s_cerr[j - 1] * kv[j];
        sm += s_cmid[j - 1] * kv[j];
      }
      dtb32 += errb * se + midb * sm;
      if (sl < D) {
#pragma unroll
        for (int j = 1; j <= 7; ++j) {
          kk[j][sl] = kv[j];
          kb[j][sl] = kbv[j];
        }
        E.pd = pd;
        E.pt = pt;
        E.yb0 = yb0;
        E.yb1 = yb1;
        E.dtb32 = dtb32;
      }
    } else if (!in_att && ev == 1) {
      // the initial step's adjoint: dt0 back to h0, d1 and the probe's rms
      const float h0 = (float)s_ra.init_rec[3];
      C.h0f = (h0);
      double h0b, d1b_, r2, r2b;
      dopri_dt0_adjoint(C.dtbar, (float)s_ra.init_rec[1], (float)s_ra.init_rec[2], h0, (float)s_ra.init_rec[4], h0b, d1b_,
                        r2, r2b);
      C.h0b = (h0b);
      C.d1b = (d1b_);
      float f1b = 0.f, f0bp = 0.f, scb = 0.f;
      if (el && r2 > 0.0) {
        const float y = tx(0), f0 = tk(0), f1 = tk(1);
        const float scale = s_ra.atol + fabsf(y) * s_ra.rtol;
        const float q2 = (f1 - f0) / scale;
        const float q2b = (float)(r2b * (double)q2 / (s_ra.n_el * r2));
        f1b = q2b / scale;
        f0bp = -q2b / scale;
        scb = -q2b * q2 / scale;
      }
      if (sl < D) {
        kb[0][sl] = f1b;
        E.f0bp = f0bp;
        E.scb = scb;
      }
      C.d0b = 0.0;
    } else if (ev == 0) {
      if (s_ra.base == 2) {  // the rest of _select_initial_step: d0 = rms(y0 / scale), d1 = rms(f0 / scale)
        const float d0 = (float)s_ra.init_rec[0], d1 = (float)s_ra.init_rec[1];
        if (el) {
          const float y = tx(0), f0 = tk(0);
          const float scale = s_ra.atol + fabsf(y) * s_ra.rtol;
          const float q0 = y / scale, q1 = f0 / scale;
          const float q0b = d0 > 0.f ? (float)(C.d0b * (double)q0 / (s_ra.n_el * d0)) : 0.f;
          const float q1b = d1 > 0.f ? (float)(C.d1b * (double)q1 / (s_ra.n_el * d1)) : 0.f;
          const float scb = E.scb - q0b * q0 / scale - q1b * q1 / scale;
          const float sy = y > 0.f ? 1.f : (y < 0.f ? -1.f : 0.f);
          E.ybc += q0b / scale + scb * s_ra.rtol * sy;
          E.fbc += q1b / scale;
        }
      }
      if (sl < D) kb[0][sl] = el ? E.fbc : 0.f;
    }
    // this evaluation's output adjoint -> the layer-1 output slots
    if (sl < D) g1s[tt * D + sl] = in_att ? kb[s][sl] : kb[0][sl];
    vjp(ev);
    // ---------------- after the VJP: the input adjoint ----------------
    const float xb = sl < D ? gxs[tt * D + sl] : 0.f;
    if (in_att) {
      double v0 = 0.0, v1 = 0.0;
      if (sl < D) {
        const float X = xb + (s == 7 ? E.yb1 : 0.f);  // stage 7's input IS y1
        E.yb0 += X;
        float sb = 0.f;
        for (int j = 1; j < s; ++j) {  // tableau row s - 2
          const float c = s_beta[s - 2][j - 1];
          kb[j][sl] += (c * C.dt32) * X;
          sb += c * kk[j][sl];
        }
        E.dtb32 += X * sb;
        if (s == 2) {  // attempt n done: the carries
          E.ybc = el ? E.yb0 : 0.f;
          E.fbc = el ? kb[1][sl] : 0.f;
          v0 = el ? E.pd + (double)E.dtb32 : 0.0;
          v1 = el ? E.pt : 0.0;
        }
      }
      if (s == 2) {  // the grid sum of the attempt's d/d dt and d/d t0 terms
        if constexpr (MP) {
          mp_arrive(v0, v1);
        } else {
          double S0, S1;
          gsum(v0, v1, S0, S1);
          C.dtbar = (C.dtb_base + (C.acc ? C.tbar : 0.0) + S0);
          C.tbar = (C.tbar + S1);
        }
      }
    } else if (ev == 1) {  // the probe: input y0 + h0 f0
      const float f0 = el ? tk(0) : 0.f;
      if (el) {
        E.ybc += xb;
        E.fbc += xb * C.h0f + E.f0bp;
      }
      if constexpr (MP) {
        mp_arrive(el ? (double)(xb * f0) : 0.0, 0.0);
      } else {
        double S0, S1;
        gsum(el ? (double)(xb * f0) : 0.0, 0.0, S0, S1);
        C.h0b = (C.h0b + S0);
        dopri_h0_adjoint(C.h0b, C.h0f, (float)s_ra.init_rec[0], (float)s_ra.init_rec[1], C.d0b, C.d1b);
      }
    } else {  // evaluation 0: f(y0)
      if (el) {
        E.ybc += xb;
        if (s_ra.gy0) s_ra.gy0[bi * D + sl] = E.ybc + s_ra.gsol[bi * D + sl];  // solution[0] = y0
      }
    }
    if constexpr (MP) {
      if (in_att ? s == 2 : true) {  // the end of a segment
        const int64_t vw = mp_vw();
        if (ev > 0) {  // park what this virtual wave carries across the sum
          wsync();
          if (sl < D) mp_el[(vw * TPW + tt) * D + sl] = E;
          R0.park(mp_r + vw * (NRW * 64) + lane);
          R1.park(mp_r + vw * (NRW * 64) + BReg<L0>::NW * 64 + lane);
        } else {       // its sweep is done: its row of partial sums
          float* part = a.part + vw * a.nacc;
          R0.template store<TPW>(part, lane);
          R1.template store<TPW>(part + L0::AL.n, lane);
        }
        if (vwg + gridDim.x < VG) {  // the same segment for the next virtual workgroup
          vwg += gridDim.x;
          mp_bind(seg_top);
          ev = seg_top + 1;
        } else if (ev > 0) {         // every arrival of this workgroup is in: the segment's sum
          double S0, S1;
          mp_poll(S0, S1);
          if (in_att) {
            C.dtbar = (C.dtb_base + (C.acc ? C.tbar : 0.0) + S0);
            C.tbar = (C.tbar + S1);
          } else {
            C.h0b = (C.h0b + S0);
            dopri_h0_adjoint(C.h0b, C.h0f, (float)s_ra.init_rec[0], (float)s_ra.init_rec[1], C.d0b, C.d1b);
          }
          wsync();
          s_sc0[wid] = C;
          wsync();
          vwg = blockIdx.x;
          if constexpr (MP) seg_top = ev - 1;
          mp_bind(seg_top);
        }
      }
    }
  }
  if constexpr (!MP) {
    float* part = a.part + ((int64_t)blockIdx.x * kTPB + wid) * a.nacc;
    R0.template store<TPW>(part, lane);
    R1.template store<TPW>(part + L0::AL.n, lane);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    da.status[0] = (s_ab || __hip_atomic_load(dp_abort(da.gp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ? 4 : 0;
