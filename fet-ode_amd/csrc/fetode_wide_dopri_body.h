// fetode_wide_dopri_body.h — the resident dopri5 kernel of the two-layer wide KAN-FET field
// (fetode_wide.hip, which includes this once per kernel).  WD_KERNEL: the kernel's name; WD_WAVES:
// its waves-per-SIMD bound; WD_TAPE: the training forward (fetode_wide_dopri5_tape) — the same
// solve, plus plain stores of every evaluation's x_e / h_e / k_e planes and of the initial-step
// scalars, nothing the solve reads.  The untaped kernel is this text with those blocks discarded.
template <int K>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(WD_WAVES))) void WD_KERNEL(WideDopriArgs a) {
  __shared__ WdCtl ctl;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int G = (int)gridDim.x;
  const int64_t B = a.B, BD = B * a.D, BH = B * a.H;
  const int D = a.D, H = a.H;
  const double n_el = a.n_el;
  // element ownership: the layer-1 tile epilogue's storing threads (waves 0-3: row 16 (w % 4) +
  // 4 (lane / 16) + v, dim lane % 16), layer-1 tile t < nT1 on workgroup t % G
  const bool owner = w < 4;
  const int rt = w & 3, kq = lane >> 4, kr = lane & 15;
  auto for_owned = [&](auto&& f) {
    if (!owner) return;
    for (int t = blockIdx.x; t < a.nT1; t += G) {
      const int64_t b0 = (int64_t)(t / a.nOT1) * kRows;
      const int d = (t % a.nOT1) * kOuts + kr;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int64_t b = b0 + 16 * rt + 4 * kq + v;
        if (b < B) f(b * D + d);
      }
    }
  };
  float* const es = a.es;
  unsigned nround = 0;  // norm rounds (wide_norm)

  for_owned([&](int64_t i) {
    const float y = a.y0[i];
    es[kEY * BD + i] = y;
    a.sol[i] = y;
    if constexpr (WD_TAPE) {
      if (a.tape_cap > 0) a.tpx[i] = y;
    }
  });
  if (tid == 0) {
    ctl.dt = a.step.first_step;
    ctl.t0 = ctl.t1 = 0.0;
    ctl.t0s = ctl.t1s = a.t[0];
    ctl.h0 = ctl.d1 = ctl.dt32 = 0.f;
    ctl.nev = ctl.nfev = ctl.n_att = ctl.n_steps = ctl.stg = 0;
    ctl.iout = 1;
    ctl.kind = kCmbF0;
    ctl.status = -1;
  }
  __syncthreads();
  int status = -1;
#pragma unroll 1
  for (;;) {
    // ---- one field evaluation: L0 phase | barrier | L1 phase | barrier ----
    const int e = ctl.nev, p = e & 1;
    if (e > 0 && wide_barrier(a.bar)) {  // the stage input came from other workgroups
      status = 4;
      break;
    }
    bool ab = false;
#pragma unroll 1
    for (int l = 0; l < 2 && !ab; ++l) {
      WideArgs L = l ? a.l1 : a.l0;
      const int nT = l ? a.nT1 : a.nT0, nOT = l ? a.nOT1 : a.nOT0, S = l ? a.S1 : a.S0;
      if (l == 0) {
        L.x = e == 0 ? a.y0 : a.xin + p * BD;
        L.nxs = L.nps = 1;
        L.reinit = e == 0 ? a.reinit0 : 0;
        L.prev = e == 0 ? a.prev0 : (e == 1 ? a.y0 : a.xin + (p ^ 1) * BD);
      } else {
        L.x = a.hs + (int64_t)p * a.S0 * BH;
        L.nxs = a.S0;
        L.xss = BH;
        L.reinit = e == 0 ? a.reinit1 : 0;
        L.prev = e == 0 ? a.prev1 : a.hs + (int64_t)(p ^ 1) * a.S0 * BH;
        L.nps = e == 0 ? 1 : a.S0;
        L.pss = BH;
      }
      L.nslice = S;
      const int ow = l ? D : H;
      float* const ob = l ? a.ks : a.hs + (int64_t)p * a.S0 * BH;  // k slabs | this parity's hidden slabs
      const int64_t sl = l ? BD : BH;
      for (int t = blockIdx.x; t < nT * S; t += G) {
        const int bz = t / nT, r = t % nT;
        float* const o = ob + bz * sl;
        wide_tile<K, true, true, kChMax, true>(L, r / nOT, r % nOT, bz,
                                               [&](int64_t b, int c, float v) { st_wt(&o[b * ow + c], v); });
      }
      ab = wide_barrier(a.bar);
    }
    if (ab) {
      status = 4;
      break;
    }
    // ---- the per-element combine of k (the host loop's fetode_lincomb / scaled_rms order) ----
    {
      const int kind = ctl.kind, stg = ctl.stg, pn = (e + 1) & 1;
      const float dt32 = ctl.dt32;
      float c[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) c[q] = ctl.cc[q];
      const int S1 = a.S1;
      // norm terms: per layer-1 tile (wide_tile_partial) when this evaluation ends in a reduction
      const bool red = (kind == kCmbF0 && !(a.step.first_step > 0.0)) || kind == kCmbF1 || (kind == kCmbStage && stg == 5);
      double acc0 = 0.0, acc1 = 0.0;
      if constexpr (WD_TAPE) {
        if (e < a.tape_cap) {  // h_e: this parity's hidden slabs in the layer-1 input's order
          const float* hp = a.hs + (int64_t)p * a.S0 * BH;
          float* const ho = a.tph + (int64_t)e * BH;
          for (int64_t j = (int64_t)blockIdx.x * kThreads + tid; j < BH; j += (int64_t)G * kThreads) {
            float v = hp[j];
            for (int s = 1; s < a.S0; ++s) v = v + hp[s * BH + j];
            ho[j] = v;
          }
        }
      }
      auto elem = [&](int64_t i) {
        float k = a.ks[i];
        for (int s = 1; s < S1; ++s) k = k + a.ks[s * BD + i];  // slab 0 + slab 1 + ..: the launch path's order
        if constexpr (WD_TAPE) {
          if (e < a.tape_cap) a.tpk[(int64_t)e * BD + i] = k;
        }
        const float y = es[kEY * BD + i];
        if (kind == kCmbF0) {  // f0 = f(t0, y0); _select_initial_step's d0 / d1 terms
          es[kEF0 * BD + i] = k;
          const float scale = a.atol + a.rtol * fabsf(y);
          const float q0 = y / scale, q1 = k / scale;
          acc0 += (double)q0 * q0;
          acc1 += (double)q1 * q1;
        } else if (kind == kCmbF1) {  // d2 term: (f1 - f0) / scale
          const float scale = a.atol + a.rtol * fabsf(y);
          const float q2 = (k - es[kEF0 * BD + i]) / scale;
          acc0 += (double)q2 * q2;
        } else {  // Dormand-Prince stage stg (k = k_{stg + 1}): the running sums take k's column
          float a0 = 0.f;
#pragma unroll
          for (int q = 0; q < 5; ++q) {
            const float v = es[(kEA + q + 1) * BD + i] + k * (c[q] * dt32);
            es[(kEA + q) * BD + i] = v;
            if (q == 0) a0 = v;
          }
          const float err = es[kEErr * BD + i] + k * (c[6] * dt32);
          es[kEErr * BD + i] = err;
          es[kEMid * BD + i] = es[kEMid * BD + i] + k * (c[7] * dt32);
          if (stg < 5) {
            const float yi = y + a0;
            st_wt(a.xin + pn * BD + i, yi);
            es[kEY1 * BD + i] = yi;
            if constexpr (WD_TAPE) {
              if (e + 1 < a.tape_cap) a.tpx[(int64_t)(e + 1) * BD + i] = yi;
            }
          } else {  // FSAL: k is f(t1, y1); the error ratio's term and torchdiffeq's finiteness assert
            es[kEKl * BD + i] = k;
            const float y1 = es[kEY1 * BD + i];
            const float tol = a.atol + a.rtol * fmaxf(fabsf(y), fabsf(y1));
            const float qe = err / tol;
            acc0 += (double)qe * qe;
            acc1 += __builtin_isfinite(y) ? 0.0 : 1.0;
          }
        }
      };
      for (int t = blockIdx.x; t < a.nT1; t += G) {
        if (owner) {
          const int64_t b0 = (int64_t)(t / a.nOT1) * kRows;
          const int d = (t % a.nOT1) * kOuts + kr;
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const int64_t b = b0 + 16 * rt + 4 * kq + v;
            if (b < B) elem(b * D + d);
          }
        }
        if (red) {
          wide_tile_partial(a.slot, t, acc0, acc1);
          acc0 = acc1 = 0.0;
        }
      }
    }
    // ---- the decision (thread 0) ----
    const int kind = ctl.kind, stg = ctl.stg;
    const bool reduce = !(kind == kCmbF0 && a.step.first_step > 0.0) && !(kind == kCmbStage && stg < 5);
    double s0 = 0.0, s1 = 0.0;
    if (reduce && wide_norm(a, nround, s0, s1)) {
      status = 4;
      break;
    }
    __syncthreads();  // every wave has read this evaluation's control words before thread 0 rewrites them
    if (tid == 0) {
      ctl.nev = e + 1;
      ++ctl.nfev;
      ctl.fit = 0;
      ctl.next = kNextNone;
      ctl.io_lo = ctl.io_hi = ctl.iout;
      bool sched = false;  // outputs due, then the next attempt
      if (kind == kCmbStage && stg < 5) {
        ctl.stg = stg + 1;
        ctl.next = kNextNone;  // the combine already wrote the next stage input
      } else if (kind == kCmbF0 && !(a.step.first_step > 0.0)) {  // the initial step: h0, then the probe
        float d0, d1;
        ctl.h0 = dopri_h0(s0, s1, n_el, d0, d1);
        ctl.d1 = d1;
        if constexpr (WD_TAPE) {
          if (blockIdx.x == 0) {
            a.init_rec[0] = d0;
            a.init_rec[1] = d1;
            a.init_rec[3] = ctl.h0;
          }
        }
        ctl.kind = kCmbF1;
        ctl.next = kNextProbe;
      } else if (kind == kCmbF1) {
        float d2, h1;
        ctl.dt = dopri_dt0(s0, n_el, ctl.h0, ctl.d1, d2, h1);
        if constexpr (WD_TAPE) {
          if (blockIdx.x == 0) {
            a.init_rec[2] = d2;
            a.init_rec[4] = h1;
          }
        }
        sched = true;
      } else if (kind == kCmbF0) {  // first_step given
        sched = true;
      } else {  // the attempt's error ratio, accept / reject, rk_common._optimal_step_size
        if (s1 != 0.0) {
          ctl.status = 1;
        } else {
          const float ratio = dopri_ratio(s0, n_el);
          const bool accept = dopri_accept(ratio);
          if (blockIdx.x == 0) dopri_log_attempt(a.att, ctl.n_att, a.max_att, ctl.t0, ctl.dt, ratio, accept);
          ++ctl.n_att;
          if (accept) {
            ctl.fit = 1;
            ctl.fit_dt32 = ctl.dt32;  // the accepted attempt's step (dt32 is about to take the next one)
            ctl.t0s = ctl.t0;
            ctl.t1s = ctl.t1;
          } else {
            ctl.t0s = ctl.t0;
          }
          ctl.dt = dopri_next_dt(ctl.dt, ratio, a.step);
          ++ctl.n_steps;
          sched = true;
        }
      }
      if (sched) {
        // outputs due (interp._interp_evaluate of the last accepted step), then the next attempt
        int io = ctl.iout;
        while (io < a.T && !(a.t[io] > ctl.t1s)) {
          ++io;
          ctl.n_steps = 0;
        }
        ctl.io_hi = io;
        ctl.iout = io;
        if (io >= a.T) {
          ctl.status = 0;
        } else if (ctl.n_steps >= a.max_steps) {
          ctl.status = 3;
        } else {
          const double t0 = ctl.t1s, dt = ctl.dt;
          if (dopri_underflow(t0, dt)) {
            ctl.status = 2;
          } else {
            ctl.t0 = t0;
            ctl.t1 = t0 + dt;
            ctl.dt32 = (float)dt;
            ctl.kind = kCmbStage;
            ctl.stg = 0;
            ctl.next = kNextAttempt;
          }
        }
      }
      // the tableau column of the next stage evaluation's k (static indices: kernel-argument reads)
#pragma unroll
      for (int j = 1; j < 7; ++j)
        if (j == ctl.stg + 1) {
#pragma unroll
          for (int q = 0; q < 8; ++q) ctl.cc[q] = a.stc[j][q];
        }
    }
    __syncthreads();
    // ---- the decision's element passes (owner threads only: no hand-off) ----
    if (ctl.fit) {  // the accepted step's interpolant; y <- y1, f0 <- k7
      const float dtc = ctl.fit_dt32;
      for_owned([&](int64_t i) {
        const float y1 = es[kEY1 * BD + i], fb = es[kEKl * BD + i];
        float co[5];
        dopri_fit(co, es[kEY * BD + i], y1, es[kEMid * BD + i], es[kEF0 * BD + i], fb, dtc);
#pragma unroll
        for (int q = 0; q < 5; ++q) es[(kECo + q) * BD + i] = co[q];
        es[kEY * BD + i] = y1;
        es[kEF0 * BD + i] = fb;
      });
    }
    for (int j = ctl.io_lo; j < ctl.io_hi; ++j) {
      const float xq = (float)((a.t[j] - ctl.t0s) / (ctl.t1s - ctl.t0s));
      float* const so = a.sol + (int64_t)j * BD;
      for_owned([&](int64_t i) {
        float co[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) co[q] = es[(kECo + q) * BD + i];
        so[i] = dopri_eval(co, xq);
      });
    }
    if (ctl.status >= 0) {
      status = ctl.status;
      break;
    }
    const int pw = (e + 1) & 1;
    if (ctl.next == kNextProbe) {  // y0 + f0 h0 (fetode_lincomb with k[0] = f0)
      const float hh = ctl.h0;
      for_owned([&](int64_t i) {
        const float yi = es[kEY * BD + i] + es[kEF0 * BD + i] * hh;
        st_wt(a.xin + pw * BD + i, yi);
        if constexpr (WD_TAPE) {
          if (e + 1 < a.tape_cap) a.tpx[(int64_t)(e + 1) * BD + i] = yi;
        }
      });
    } else if (ctl.next == kNextAttempt) {  // the attempt's running sums from f0, its first stage input
      const float dtc = ctl.dt32;
      for_owned([&](int64_t i) {
        const float f0 = es[kEF0 * BD + i];
        float a0 = 0.f;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          const float v = f0 * (a.stc[0][q] * dtc);
          es[(kEA + q) * BD + i] = v;
          if (q == 0) a0 = v;
        }
        es[kEErr * BD + i] = f0 * (a.stc[0][6] * dtc);
        es[kEMid * BD + i] = f0 * (a.stc[0][7] * dtc);
        const float yi = es[kEY * BD + i] + a0;
        st_wt(a.xin + pw * BD + i, yi);
        es[kEY1 * BD + i] = yi;
        if constexpr (WD_TAPE) {
          if (e + 1 < a.tape_cap) a.tpx[(int64_t)(e + 1) * BD + i] = yi;
        }
      });
    }
  }
  const int nev = ctl.nev;
  if (status != 4 && nev > 0) {
    // the hysteresis memory after the solve: the last evaluation's layer inputs (ferro_class.py:409)
    const int el = nev - 1, pl = el & 1;
    const float* x0 = el == 0 ? a.y0 : a.xin + pl * BD;
    const float* h0 = a.hs + (int64_t)pl * a.S0 * BH;
    const int64_t nthr = (int64_t)G * kThreads;
    const int64_t nmem = BH > BD ? BH : BD;   // either layer may be the wider one (D > H: 48 -> 16 -> 48)
    for (int64_t j = (int64_t)blockIdx.x * kThreads + tid; j < nmem; j += nthr) {
      if (j < BH) {
        float v = h0[j];
        for (int s = 1; s < a.S0; ++s) v = v + h0[s * BH + j];
        a.st1[j] = v;
      }
      if (j < BD) a.st0[j] = x0[j];
    }
  }
  if (blockIdx.x == 0 && tid == 0) {
    a.stats[0] = ctl.nfev;
    a.stats[1] = ctl.n_att;
    a.stats[2] = __hip_atomic_load(a.bar + 64 * 9 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 4 : status;
  }
}
