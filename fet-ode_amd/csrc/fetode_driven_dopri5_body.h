// fetode_driven_dopri5_body.h — the body of driven_dopri5_kernel (fetode_driven_dopri5.hip), included once
// per kernel signature: the including kernel provides KT, EVLOG and the arguments `a`; the taped kernel
// defines FETODE_DRIVEN_TAPE and provides the tape `tp`.  The tape's statements are preprocessor blocks,
// so the untaped kernels compile from exactly the tokens they had before the tape existed.
  __shared__ float xs[1][kDrvInMax], gxs[1][kDrvInMax], vs[1][kDrvInMax];  // one sample per workgroup
  __shared__ float part[4][1][64];
  __shared__ float s_beta[6][6], s_cerr[7], s_cmid[7], s_alpha[6];
  __shared__ float s_tq[6], us[6][kDrvDMax];  // the phase's evaluation times and x(t) at each
  __shared__ int s_nq;
  const int H = a.H, D = a.D, In = H + D, K = KT > 0 ? KT : a.K, T = a.T;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t b = blockIdx.x;  // grid = B
  const float4* __restrict__ el = reinterpret_cast<const float4*>(a.plan);
  const float* __restrict__ tail = a.plan + 4 * drv_plan_elems(In, H, K);
  const float* __restrict__ tg = a.tg;
  const float* __restrict__ xb = a.x + b * (int64_t)T * D;
  const bool w0 = wv == 0, own = w0 && lane < H;  // own: holds element `lane` of the state
  const int dd = tid - 64;
  const bool drv = dd >= 0 && dd < D;              // publishes driving input dd
  const float gs = a.gs, gsl2e = a.gsl2e, wc = a.wc;
  float fcon = 0.f, gain = 0.f, bias = 0.f;
  if (own) {
    fcon = tail[lane];
    gain = tail[H + lane];
    bias = tail[2 * H + lane];
  }
  // input i of the next evaluation: value, its gate against the previous evaluation's input
  // (prev <- hx, call order) and the per-input factors of the element loop
  auto publish = [&](int i, float xn, float xo) {
    const DrvGate g = drv_gate(gs, gsl2e, wc, xn, xo);
    xs[0][i] = g.x;
    gxs[0][i] = g.gx;
    vs[0][i] = g.v;
  };
  // LinearInterp1D (compare_noise_ecg.py:861-872) as drv_locate states it, but the left searchsorted
  // of an increasing grid by bisection (every index stays inside [0, T - 1])
#ifdef FETODE_DRIVEN_TAPE
  float slope = 0.f;  // the slope of the interval the last interp used
#endif
  auto interp = [&](float t, int d) -> float {
    const float lo = tg[0], hi = tg[T - 1];
#ifdef FETODE_DRIVEN_TAPE
    const bool cut = t < lo || t > hi;  // the clamp passes its gradient at equality
#endif
    t = t < lo ? lo : (t > hi ? hi : t);
    int l = 0, r = T;
    while (l < r) {
      const int m = (l + r) >> 1;
      if (tg[m] < t) l = m + 1;
      else r = m;
    }
    const int i = l < 1 ? 1 : (l > T - 1 ? T - 1 : l);
    const float t0 = tg[i - 1], t1 = tg[i];
    const float x0 = xb[(int64_t)(i - 1) * D + d], x1 = xb[(int64_t)i * D + d];
    const float w = (t - t0) / ((t1 - t0) + 1e-12f);
#ifdef FETODE_DRIVEN_TAPE
    slope = cut ? 0.f : (x1 - x0) / ((t1 - t0) + 1e-12f);
#endif
    return (1.0f - w) * x0 + w * x1;
  };
  int nfev = 0;
  // x(t) at the n evaluation times of the phase that starts (wave 1, one lane per time and input);
  // the first time's values are the next evaluation's driving inputs
  auto drive = [&](int n, bool first) {
    if (dd >= 0 && dd < n * D) {
      const int s = dd / D, d = dd - s * D;
      const float tq = s_tq[s];
      const float v = interp(tq, d);
      us[s][d] = v;
      if (EVLOG) {
        const int64_t e = (int64_t)nfev + s;
        if (e < a.max_ev) {
          float* o = a.evlog + (b * a.max_ev + e) * (1 + D);
          if (d == 0) o[0] = tq;
          o[1 + d] = v;
        }
      }
#ifdef FETODE_DRIVEN_TAPE
      {
        const int64_t e = (int64_t)nfev + s;
        if (e < tp.max_ev) {
          if (d == 0) tp.tq[b * tp.max_ev + e] = tq;
          tp.slope[(b * tp.max_ev + e) * D + d] = slope;
        }
      }
#endif
      if (s == 0) publish(H + d, v, first ? (a.prev0 ? a.prev0[b * In + H + d] : 0.f) : xs[0][H + d]);
    }
  };
  // one evaluation of the published input; wave 0 receives f (lanes >= H: 0)
  auto eval = [&]() -> float {
    __syncthreads();  // this evaluation's inputs are published
#ifdef FETODE_DRIVEN_TAPE
    if (tid < In && nfev < tp.max_ev) tp.hx[(b * tp.max_ev + nfev) * In + tid] = xs[0][tid];
#endif
    float acc[1];
    drv_eval_partial<1, KT>(el, H, In, K, lane, wv, xs, gxs, vs, acc);
    part[wv][0][lane] = acc[0];
    __syncthreads();  // partial sums are in; nobody reads this evaluation's inputs any more
    ++nfev;
    float f = 0.f;
    if (w0) {
      const float phi = drv_eval_meet<1>(part, 0, lane, fcon);
#ifdef FETODE_DRIVEN_TAPE
      // nfev counts this evaluation already
      if (own && nfev <= tp.max_ev) tp.phi[(b * tp.max_ev + (nfev - 1)) * H + lane] = phi;
#endif
      f = tanhf(phi) * gain + bias;
    }
    return f;
  };

  // ---- wave 0: the sample's solver state (one lane per element; the scalars agree on every lane) ----
  const double n_el = (double)H;
  const float rtol = a.rtol, atol = a.atol;
  float y = 0.f, f0 = 0.f, yi = 0.f, err = 0.f, mid = 0.f, dt32 = 0.f;
  float A[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float co[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  float h0p = 0.f, d1p = 0.f, scale = 1.f;  // the initial-step selection
  double dt = 0.0, t0 = 0.0, t1 = 0.0, t0s = 0.0, t1s = 0.0;
  int i_out = 1, n_steps = 0, n_att = 0, status = 0;

  // after f0, the probe and every attempt: the output rows the accepted step reaches, then the next
  // attempt's checks (the host loop's assertions, in its order), evaluation times and first input — or
  // the end.  Nothing is published at the end: xs keeps the last evaluation's input for prev_out
  auto begin_attempt = [&]() {
    int n = 6;
    while (i_out < T && !((double)tg[i_out] > t1s)) {
      const float total = dopri_eval(co, (float)(((double)tg[i_out] - t0s) / (t1s - t0s)));
      if (own) a.sol[((int64_t)i_out * gridDim.x + b) * H + lane] = total;
      ++i_out;
      n_steps = 0;
    }
    if (i_out >= T) n = 0;
    else if (n_steps >= a.max_steps) status = 3;
    else if (dopri_underflow(t1s, dt)) status = 2;
    else if (__ballot(own && !__builtin_isfinite(y)) != 0) status = 1;
    if (status) n = 0;
    if (n) {
      t0 = t1s;
      dt32 = (float)dt;
      t1 = t0 + dt;
      if (lane < 6) {
        const float al = s_alpha[lane];
        s_tq[lane] = al == 1.0f ? (float)t1 : (float)t0 + al * dt32;
      }
      // rk_common._runge_kutta_step in fetode_lincomb's op order, accumulated as the stages arrive:
      // A[i] is stage s+1+i's sum k0*b0 + k1*b1 + ... (the same left-to-right sums)
#pragma unroll
      for (int i = 0; i < 6; ++i) A[i] = f0 * (s_beta[i][0] * dt32);
      err = f0 * (s_cerr[0] * dt32);
      mid = f0 * (s_cmid[0] * dt32);
      yi = y + A[0];
      if (own) publish(lane, yi, xs[0][lane]);
    }
    if (lane == 0) s_nq = n;
  };

  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = 0; j < 6; ++j) s_beta[i][j] = a.beta[i][j];
      s_alpha[i] = a.alpha[i];
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      s_cerr[i] = a.cerr[i];
      s_cmid[i] = a.cmid[i];
    }
    s_tq[0] = tg[0];
    s_nq = 1;
#ifdef FETODE_DRIVEN_TAPE
#pragma unroll
    for (int i = 0; i < 5; ++i) tp.init_rec[b * 5 + i] = 0.0;
#endif
  }
  if (w0) {
    y = own ? a.h0[b * H + lane] : 0.f;
    co[0] = y;
    t0s = t1s = (double)tg[0];
    if (own) {
      a.sol[b * H + lane] = y;
      publish(lane, y, a.prev0 ? a.prev0[b * In + lane] : 0.f);
    }
  }

  int phase = kPhaseF0;
  for (;;) {
    __syncthreads();  // wave 0's announcement: s_nq, s_tq and its part of the first input
    const int n = s_nq;
    if (n == 0) break;  // every thread reads the same word: the four waves leave together
    drive(n, phase == kPhaseF0);
    if (phase == kPhaseF0) {
      const float f = eval();
      phase = a.step.first_step > 0.0 ? kPhaseAttempt : kPhaseProbe;
      if (w0) {
        f0 = f;
        if (phase == kPhaseAttempt) {
          dt = a.step.first_step;
          begin_attempt();
        } else {  // misc._select_initial_step: the probe f(t0 + h0, y0 + h0 f0)
          scale = atol + rtol * fabsf(y);
          const float q0 = y / scale, q1 = f0 / scale;
          const double s0 = wave_sum_d(own ? (double)q0 * q0 : 0.0);
          const double s1 = wave_sum_d(own ? (double)q1 * q1 : 0.0);
          float d0;
          h0p = dopri_h0(s0, s1, n_el, d0, d1p);
#ifdef FETODE_DRIVEN_TAPE
          if (lane == 0) {
            tp.init_rec[b * 5 + 0] = d0;
            tp.init_rec[b * 5 + 1] = d1p;
            tp.init_rec[b * 5 + 3] = h0p;
          }
#endif
          if (own) publish(lane, y + f0 * h0p, xs[0][lane]);
          if (lane == 0) {
            s_tq[0] = (float)(t0s + (double)h0p);
            s_nq = 1;
          }
        }
      }
    } else if (phase == kPhaseProbe) {
      const float f1 = eval();
      phase = kPhaseAttempt;
      if (w0) {
        const float q2 = (f1 - f0) / scale;
        const double s2 = wave_sum_d(own ? (double)q2 * q2 : 0.0);
        float d2, h1;
        dt = dopri_dt0(s2, n_el, h0p, d1p, d2, h1);
#ifdef FETODE_DRIVEN_TAPE
        if (lane == 0) {
          tp.init_rec[b * 5 + 2] = d2;
          tp.init_rec[b * 5 + 4] = h1;
        }
#endif
        begin_attempt();
      }
    } else {
      float kn = 0.f;
#pragma unroll 1
      for (int s = 0; s < 6; ++s) {
        kn = eval();
        if (w0) {
          const int j = s + 1, jc = j < 5 ? j : 5;
#pragma unroll
          for (int i = 0; i < 5; ++i) {
            const int r = j + i < 5 ? j + i : 5;
            A[i] = (j + i <= 5) ? A[i + 1] + kn * (s_beta[r][jc] * dt32) : 0.f;
          }
          err = err + kn * (s_cerr[j] * dt32);
          mid = mid + kn * (s_cmid[j] * dt32);
          if (s < 5) {
            yi = y + A[0];
            if (own) publish(lane, yi, xs[0][lane]);
          }
        }
        if (drv && s < 5) publish(H + dd, us[s + 1][dd], xs[0][H + dd]);
      }
      if (w0) {
        const float y1 = yi;
        const float tol = atol + rtol * fmaxf(fabsf(y), fabsf(y1));
        const float qe = err / tol;
        const double ss = wave_sum_d(own ? (double)qe * qe : 0.0);
        const float ratio = dopri_ratio(ss, n_el);
        const bool accept = dopri_accept(ratio);
        if (lane == 0) dopri_log_attempt(a.att + b * (int64_t)a.max_att * 4, n_att, a.max_att, t0, dt, ratio, accept);
        ++n_att;
        if (!__builtin_isfinite(ratio)) {
          status = 1;
        } else {
          if (accept) {
            dopri_fit(co, y, y1, mid, f0, kn, dt32);
            y = y1;
            f0 = kn;
            t0s = t0;
            t1s = t1;
          } else {
            t0s = t0;
          }
          dt = dopri_next_dt(dt, ratio, a.step);
          ++n_steps;
        }
        begin_attempt();
      }
    }
  }
  // prev <- the last evaluation's input (the end publishes nothing)
  if (a.prev_out && tid < In) a.prev_out[b * In + tid] = xs[0][tid];
  if (tid == 0) {
    a.stats[b * 3 + 0] = nfev;
    a.stats[b * 3 + 1] = n_att;
    a.stats[b * 3 + 2] = status;
  }
#ifdef FETODE_DRIVEN_TAPE
  {  // the rows the solve did not reach read as zeros (the parameter sums run over all rows)
    const int64_t r0 = b * tp.max_ev, n0 = nfev < tp.max_ev ? nfev : tp.max_ev, n1 = tp.max_ev;
    for (int64_t i = n0 * In + tid; i < n1 * In; i += kDrvThreads) tp.hx[r0 * In + i] = 0.f;
    for (int64_t i = n0 * H + tid; i < n1 * H; i += kDrvThreads) tp.phi[r0 * H + i] = 0.f;
    for (int64_t i = n0 * D + tid; i < n1 * D; i += kDrvThreads) tp.slope[r0 * D + i] = 0.f;
    for (int64_t i = n0 + tid; i < n1; i += kDrvThreads) tp.tq[r0 + i] = 0.f;
  }
#endif
