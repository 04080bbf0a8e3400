// fetode_fused4_body.h — the function body of the v4 kernel, included (not called) by its two
// __global__ functions in fetode_fused.hip: fused4_kernel (MP = false) and the multi-pass resident
// dopri5 driver fused4_mp_kernel (MP = true: the trajectory a lane serves changes between grid sums).
// In scope at the point of inclusion: the kernel argument `FusedArgs a` and the compile-time values
// H, K_, NB, NG, FERRO, HOT, DOPRI, TAPE, TPW, MP.  Textual sharing keeps fused4_kernel's code
// exactly what it was as a function of its own (as an inlined device function its register
// allocation moved).
  static_assert(!MP || (DOPRI && !HOT && TPW == 2), "multi-pass: the resident dopri5 driver");
  constexpr int D = 2, NI = NG - 1, NFL = 1 + NB, NFP = (NFL + 1) & ~1, K = FERRO ? K_ : 0;
  // feature jobs: logistic 0..NB-1, SiLU, [gate, exp(gs x)], then x / u / m stores
  constexpr int J_SILU = NB, J_GATE = NB + 1, J_EXP = NB + 2, J_X = FERRO ? NB + 3 : NB + 1;
  constexpr int J_M = J_X + 1;
  static_assert(J_M < 16 && NG <= 16, "v4 layout: NB logistic + SiLU (+ gate, exp) + x, m jobs on a row of 16 lanes");
  static_assert(H <= 10, "v4 layout: H <= 10 groups of 3 lanes");
  static_assert(!FERRO || K % 2 == 0, "v4 pairs Ferro elements (i, k), (i, k+1)");
  constexpr int KP = K / 2 > 0 ? K / 2 : 1;
  static_assert(TPW == 2 || (TPW == 1 && HOT && !DOPRI), "one trajectory per wave: the rk4 path");
  constexpr int NLG = TPW == 2 ? 3 : 6;                      // lanes per hidden unit
  // layer 0 (2 -> H): output o on a group of 3 lanes; layer 1 (H -> 2): hidden INPUT o on the
  // same group (v7): its features, its Ferro elements of both outputs (pairs (o, 0, k), (o, 1, k):
  // one packed pair feeds both output sums) and its two spline edges stay in the group's
  // registers — no LDS exchange between layer 0 and layer 1
  using FS0 = FerroSplit<D * KP, NLG>;
  static_assert(!FERRO || D == 2, "v7 layer 1 pairs the two outputs of an input");
  constexpr int REM1 = K % NLG;
  constexpr bool SPLIT1 = TPW == 2 && REM1 == 1;             // one k left: two singles (d = 0, 1)
  constexpr int NPL0 = FERRO ? FS0::NPL : 0, NPL1 = FERRO ? (SPLIT1 ? K / NLG : (K + NLG - 1) / NLG) : 0;
  constexpr int NSL0 = FERRO ? FS0::NSL : 0, NSL1 = (FERRO && SPLIT1) ? 1 : 0;
  constexpr int FPL0 = ((D * NFP + NLG - 1) / NLG + 3) & ~3;
  constexpr int RF1 = (NFL + NLG - 1) / NLG;                 // feature rounds of a hidden input (SiLU + NB)
  constexpr int FLEN0 = (NLG * FPL0 > D * NFP ? NLG * FPL0 : D * NFP);
  // layer 0's edge operands read in one batch (v4_edges, EB): every KAN-FET instantiation (with the
  // shared rows below none gains scratch or loses an occupancy step); the feature chunks join the
  // batch (EBF, 8 more registers) in the rk4 kernels only: the generic and taped kernels would drop
  // from 3 to 2 waves per SIMD, the taped dopri5 and multi-pass kernels would spill
  constexpr bool EB0 = FERRO, EBF0 = EB0 && HOT;
  // the hidden phase's independent sigmoid-of-affine chains issued two to a packed instruction (PKS,
  // DESIGN.md §3 round 11): the two rk4 inference kernels only, the instantiations the listing and
  // the resource table were checked for; every other one keeps the scalar chains, line for line
#ifndef FETODE_EXP_NO_PK_CHAINS
  constexpr bool PKS = FERRO && HOT && !TAPE;
#else
  constexpr bool PKS = false;
#endif
  // bit r: round r reads the row round r - 1 read, on every lane (gi0 below): it is read once
  constexpr unsigned SAME0 = [] {
    unsigned m = 0;
    for (int r = 1; r < NPL0; ++r) {
      bool same = true;
      for (int l = 0; l < NLG; ++l) {
        const int p1 = l * NPL0 + r, p0 = p1 - 1;
        same = same && (p1 < D * KP ? p1 / KP : 0) == (p0 < D * KP ? p0 / KP : 0);
      }
      if (same) m |= 1u << r;
    }
    return m;
  }();
  if constexpr (DOPRI) {
    if (a.dp.xr_world > 1 && blockIdx.x == gridDim.x - 1) {   // the cross-rank exchange workgroup
      xrank_comm(a.dp);
      return;
    }
  }
  STAMP_ENTRY
  // the headline instantiation (KAN-FET rk4 inference, two trajectories per wave): the only one whose
  // waves share a SIMD for a whole solve with nothing to synchronise them, and the only one with the
  // wave skew below (and the progress build's clock reads); every other one compiles without either
  constexpr bool SKEW = !MP && FERRO && HOT && !DOPRI && !TAPE && TPW == 2;
  PROGRESS_DECL
  PROGRESS_MARK();
  constexpr int KT = (NG + 2) / 3;                   // knots per group lane
  static_assert(3 * KT >= NG, "knots per group lane");
  // The parameters arrive in the plan's image block (fetode_fused4_image.h: the one definition of
  // this kernel's lane map): the LDS tables as the bytes of `s_tab`, this lane's constants as IMG::NV4
  // float4 slots.  Every load of the prologue is issued before the first wait.
  using BLK = Fused4Block<H, K, NB, NG>;
  using TAB = typename BLK::TAB;
  using IMG = Fused4Lanes<H, K, NB, NG, NLG>;
  static_assert(IMG::NPL0 == NPL0 && IMG::NSL0 == NSL0 && IMG::NPL1 == NPL1 && IMG::NSL1 == NSL1 &&
                    IMG::FPL0 == FPL0 && IMG::RF1 == RF1 && IMG::KT == KT,
                "the lane image and the kernel share one lane map");
  constexpr int SPR = TAB::SPR;
  // (the cubic tables' row pitch SPR and the members' order: Fused4Tables)
  struct __attribute__((aligned(16))) Tables {
    float sp0[TAB::SPT0], sp1[TAB::SPT1];
    f2 kr0[TAB::KR0], kr1[TAB::KR1];
    float c0[H], c1[D];
    float pad[TAB::NF - TAB::O_END > 0 ? TAB::NF - TAB::O_END : 1];
  };
  static_assert(offsetof(Tables, sp1) == 4 * TAB::O_SP1 && offsetof(Tables, kr0) == 4 * TAB::O_KR0 &&
                    offsetof(Tables, kr1) == 4 * TAB::O_KR1 && offsetof(Tables, c0) == 4 * TAB::O_C0 &&
                    offsetof(Tables, c1) == 4 * TAB::O_C1,
                "the LDS image is this struct byte for byte");
  __shared__ Tables s_tab;
  auto& s_sp0 = s_tab.sp0;
  auto& s_sp1 = s_tab.sp1;
  auto& s_kr0 = s_tab.kr0;
  auto& s_kr1 = s_tab.kr1;
  auto& s_c0 = s_tab.c0;
  auto& s_c1 = s_tab.c1;
  __shared__ __attribute__((aligned(16))) V4Lds<D, FLEN0> s_L0[TPW];
  // the step / output schedule is staged through LDS in chunks: per-step global loads in the
  // loop would wait (vmcnt) behind the solution stores of the previous step.  One chunk holds the
  // reference's 35-point grid; its loads belong to the prologue's burst.
  constexpr int SCH = 64;
  __shared__ float s_dt[SCH], s_hh[SCH], s_h6[SCH], s_oslope[SCH];
  __shared__ int s_ostep[SCH], s_omode[SCH];
  __shared__ f2 s_zkr[NI + 1];   // (0, 0) rows: u = 0 on the lanes whose layer-1 spline value is not used

  const int tid = threadIdx.x;
  const int hh = tid >> 5;                                   // half-wave
  const int g = TPW == 2 ? hh : 0, lane = tid & 31, row = lane >> 4, c1 = lane & 15;
  int64_t b = (int64_t)blockIdx.x * TPW + g;                // (MP: rebound per virtual workgroup)
  const bool own = TPW == 2 || hh == 0;                      // TPW 1: half 0 stores
  bool valid = b < a.B;
  V4Lds<D, FLEN0>& L0 = s_L0[g];

  // ---- layer-0 edge lane: output o0 = 5 row + q/3, part cc0 ----
  const int q = c1;
  const int o0 = row * 5 + q / 3, cc0 = q % 3;
  const bool act0 = q < 15 && o0 < H;
  const int o0c = act0 ? o0 : 0;
  const int gl = TPW == 2 ? cc0 : cc0 + 3 * hh;              // lane within the hidden unit's group
  const bool x_silu = c1 == J_SILU, x_gate = FERRO && c1 == J_GATE, x_exp = FERRO && c1 == J_EXP;
  const bool x_x = c1 == J_X;

  // ---- the prologue's loads, all issued before the first wait ----
  // the first schedule chunk: step tid and output 1 + tid on lane tid (selected when stored)
  const bool sched0 = !DOPRI && !a.single_eval;
  const bool sc_st = sched0 && a.n_steps > 0, sc_out = sched0 && a.T > 1, sc_in = 1 + tid < a.T;
  float sc_dt = 0.f, sc_hh = 0.f, sc_h6 = 0.f, sc_osl = 0.f;
  int sc_os = -1, sc_om = 1;
  if (sc_st) {
    const int i = tid < a.n_steps ? tid : a.n_steps - 1;
    sc_dt = a.step_coef[4 * i + 0];
    sc_hh = a.step_coef[4 * i + 1];
    sc_h6 = a.step_coef[4 * i + 2];
  }
  if (sc_out) {
    const int j = sc_in ? 1 + tid : a.T - 1;
    sc_os = a.out_step[j];
    sc_om = a.out_mode[j];
    sc_osl = a.out_slope[j];
  }
  // hysteresis state: prev_x of input `row` on the layer-0 gate lane, of input o0 on every lane
  // of its group (each forms the gate itself) (ferro_class.py:409); per-layer contiguous blocks
  // (include/fetode.h)
  float prev0 = 0.f, prev1 = 0.f;
  if (FERRO && valid) {
    if (x_gate) prev0 = a.state[b * D + row];
    if (act0) prev1 = a.state[a.B * D + b * H + o0];
  }
  float y = valid ? a.y0[b * D + row] : 0.f;   // state dim `row`, replicated over the row
  typedef float v4f __attribute__((ext_vector_type(4)));
  const v4f* __restrict__ img4 = reinterpret_cast<const v4f*>(a.plan + a.img);
  constexpr int NT4 = TAB::NF / 4, NTR = (NT4 + 63) / 64;    // the tables' float4s, rounds of 64 lanes
  v4f tv[NTR], li[IMG::NV4];
#pragma unroll
  for (int j = 0; j < NTR; ++j) {
    const int i = tid + 64 * j;   // (the last round's spare lanes re-read the last float4)
    tv[j] = img4[BLK::OFS_LDS / 4 + ((j + 1) * 64 <= NT4 || i < NT4 ? i : NT4 - 1)];
  }
  {
    const v4f* lp = img4 + (TPW == 2 ? BLK::OFS_L3 : BLK::OFS_L6) / 4 + (TPW == 2 ? lane : tid);
#pragma unroll
    for (int j = 0; j < IMG::NV4; ++j) li[j] = lp[j * IMG::L];
  }
  // float slot s of this lane's image (s: a constant after unrolling)
  auto LI = [&](int s) __attribute__((always_inline)) -> float {
    return li[s / 4][s % 4];
  };
  for (int i = lane; i < FLEN0; i += 32) L0.F[i] = 0.f;  // pads stay zero (finite x zero weight)
  if (tid <= NI) s_zkr[tid] = f2{0.f, 0.f};

  const bool fact = FERRO && a.plan[a.img] <= a.factor_limit && a.plan[a.img + 1] <= a.factor_limit;   // the guard words
  const float l2 = FETODE_LOG2E;

  // the Ferro constants: exp(gs Ec) when the gate is factored (pads: gec = 0, k2 = kE = cp = 0)
  auto gexp = [&](float gec) __attribute__((always_inline)) -> float { return fact ? ex2(gec) : gec; };
  f2 ep0[NPL0 > 0 ? NPL0 : 1], k20[NPL0 > 0 ? NPL0 : 1], kE0[NPL0 > 0 ? NPL0 : 1], cp0[NPL0 > 0 ? NPL0 : 1];
  int gi0[NPL0 > 0 ? NPL0 : 1];
#pragma unroll
  for (int r = 0; r < NPL0; ++r) {
    const int P = gl * NPL0 + r;
    const bool ok = act0 && P < D * KP;
    int i = ok ? P / KP : 0;
    asm volatile("" : "+v"(i));  // keep in a VGPR (no per-evaluation rematerialisation)
    gi0[r] = i;                  // (SAME0 above restates this row rule at compile time)
    const int s = IMG::S_P0 + 8 * r;
    ep0[r] = f2{gexp(LI(s)), gexp(LI(s + 1))};
    k20[r] = f2{LI(s + 2), LI(s + 3)};
    kE0[r] = f2{LI(s + 4), LI(s + 5)};
    cp0[r] = f2{LI(s + 6), LI(s + 7)};
  }
  // layer-0 single: leftover element q = cc0 of pair NPL0 * 3 + q / 2
  int gs0 = 0;
  float es0 = 0.f, k2s0 = 0.f, kEs0 = 0.f, cps0 = 0.f;
  if constexpr (NSL0 > 0) {
    const int Pl = NPL0 * NLG + gl / 2;
    const bool ok = act0 && gl < 2 * FS0::REM;
    es0 = gexp(LI(IMG::S_S0));
    k2s0 = LI(IMG::S_S0 + 1);
    kEs0 = LI(IMG::S_S0 + 2);
    cps0 = LI(IMG::S_S0 + 3);
    gs0 = ok ? Pl / KP : 0;
    asm volatile("" : "+v"(gs0));
  }
  f2 fw0[FPL0 / 2];
#pragma unroll
  for (int f = 0; f < FPL0; f += 2) fw0[f / 2] = f2{LI(IMG::S_FW0 + f), LI(IMG::S_FW0 + f + 1)};
  // ---- layer-1 (v7): hidden input o0 on its group; lane gl owns k = gl + NLG r ----
  // pair r: elements (o0, d = 0, k) and (o0, d = 1, k): .x feeds output 0, .y output 1
  // (padding: ep = 1 (fact) / 0, k = 0: th = 0, cp = 0)
  f2 ep1[NPL1 > 0 ? NPL1 : 1], k21[NPL1 > 0 ? NPL1 : 1], kE1[NPL1 > 0 ? NPL1 : 1], cp1[NPL1 > 0 ? NPL1 : 1];
#pragma unroll
  for (int r = 0; r < NPL1; ++r) {
    const int s = IMG::S_P1 + 8 * r;
    ep1[r] = f2{gexp(LI(s)), gexp(LI(s + 1))};
    k21[r] = f2{LI(s + 2), LI(s + 3)};
    kE1[r] = f2{LI(s + 4), LI(s + 5)};
    cp1[r] = f2{LI(s + 6), LI(s + 7)};
  }
  // the single left over when K % 3 == 1: element (o0, d = cc0, K - 1) on lanes cc0 = 0, 1
  float es1 = 0.f, k2s1 = 0.f, kEs1 = 0.f, cps1 = 0.f;
  if constexpr (NSL1 > 0) {
    es1 = gexp(LI(IMG::S_S1));
    k2s1 = LI(IMG::S_S1 + 1);
    kEs1 = LI(IMG::S_S1 + 2);
    cps1 = LI(IMG::S_S1 + 3);
  }
  // lane cc0 = d < 2 also owns the spline edge (o0 -> d): the single / spline value goes to output d
  const f2 dsel1 = f2{(act0 && gl == 0) ? 1.f : 0.f, (act0 && gl == 1) ? 1.f : 0.f};
  // feature rounds: job j = cc0 + 3 r (logistic j < NB, SiLU j == NB), its weights for both outputs
  float fna1[RF1], fab1[RF1], fml1[RF1];
  f2 fwt1[RF1];
#pragma unroll
  for (int r = 0; r < RF1; ++r) {
    const int j = gl + NLG * r;
    const bool silu = act0 && j == NB;   // SiLU: h * sigmoid(h)
    const int s = IMG::S_F1 + 4 * r;
    fna1[r] = silu ? -l2 : LI(s);
    fab1[r] = LI(s + 1);
    fml1[r] = silu ? 1.f : 0.f;
    fwt1[r] = f2{LI(s + 2), LI(s + 3)};
  }
  // PKS: the affine coefficients of feature rounds (2 p, 2 p + 1) as pairs, the gate's and the factored
  // exponential's slopes (gs, -gs) as one, and the single's gate constant beside the gate's 1
  f2 fna2[RF1 / 2 > 0 ? RF1 / 2 : 1], fab2[RF1 / 2 > 0 ? RF1 / 2 : 1];
#pragma unroll
  for (int p = 0; p < RF1 / 2; ++p) {
    fna2[p] = f2{fna1[2 * p], fna1[2 * p + 1]};
    fab2[p] = f2{fab1[2 * p], fab1[2 * p + 1]};
  }
  const f2 gsn1 = f2{a.P1.gsl2e, -a.P1.gsl2e}, es1p = f2{es1, 1.0f};
  // ---- layer-0 feature stream: input d = row, job c1 ----
  float xna, xab, xmul, xadd;
  float* xdst;
  {
    const int j = c1;
    xna = LI(IMG::S_X); xab = LI(IMG::S_X + 1); xmul = 1.f; xadd = 0.f;
    xdst = &L0.sink;
    if (j < NB) {
      xdst = &L0.F[row * NFP + 1 + j];
    } else if (j == J_SILU) {
      xna = -l2;
      xdst = &L0.F[row * NFP];
    } else if (FERRO && j == J_GATE) {
      xna = -a.P0.gsl2e; xmul = -a.P0.wc; xadd = a.P0.wc;
      xdst = &L0.G[row].y;
    } else if (FERRO && j == J_EXP) {
      xna = a.P0.gsl2e;
      xdst = &L0.G[row].x;
    } else if (j == J_X) {
      xdst = &L0.G[row].z;
    }
  }
  // knot interval: lane c1 holds knot c1 (and 1/(knot c1+1 - knot c1)); the lane whose knot
  // opens the interval writes u (no LDS round trip on the critical path)
  const float xknot = LI(IMG::S_X + 2);

  // knots of hidden input o0: lane cc0 holds knots KT cc0 .. KT cc0 + KT-1
  float hknot[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) hknot[t] = LI(IMG::S_HK + t);
  bool re0 = FERRO && (a.init_mask & 1u), re1 = FERRO && (a.init_mask & 2u);

  if (!a.single_eval && valid && own && c1 == 0) a.solution[b * D + row] = y;
  {
    v4f* t4 = reinterpret_cast<v4f*>(&s_tab);
#pragma unroll
    for (int j = 0; j < NTR; ++j)
      if ((j + 1) * 64 <= NT4 || tid + 64 * j < NT4) t4[tid + 64 * j] = tv[j];
  }
  if (sched0) {   // load_steps(0), load_outs(1)
    s_dt[tid] = sc_dt;
    s_hh[tid] = sc_hh;
    s_h6[tid] = sc_h6;
    s_ostep[tid] = sc_out && sc_in ? sc_os : -1;
    s_omode[tid] = sc_out && sc_in ? sc_om : 1;
    s_oslope[tid] = sc_out && sc_in ? sc_osl : 0.f;
  }
  __syncthreads();  // tables staged
  PROGRESS_MARK();
  // The younger wave of a SIMD pair: the grid's second round of workgroups (a.pair_from: the device's
  // SIMD count; partners are blockIdx.x and blockIdx.x + that count, profiles/r10_phase_before.txt).
  // a.pair is 0 where the grid leaves the waves no partner (launch_fused).  Wave-uniform: scalar code.
  const bool younger = SKEW && a.pair != 0 && (int)blockIdx.x >= a.pair_from;
  if constexpr (SKEW) {
    // Wave skew (fetode_fused_set_wave_skew): the younger wave sleeps once
    // here, so the pair runs the solve that much further apart.
    if (younger && (a.pair & 127)) {   // s_sleep takes an immediate: the count in binary
      const int sk = a.pair;
      if (sk & 64) __builtin_amdgcn_s_sleep(64);
      if (sk & 32) __builtin_amdgcn_s_sleep(32);
      if (sk & 16) __builtin_amdgcn_s_sleep(16);
      if (sk & 8) __builtin_amdgcn_s_sleep(8);
      if (sk & 4) __builtin_amdgcn_s_sleep(4);
      if (sk & 2) __builtin_amdgcn_s_sleep(2);
      if (sk & 1) __builtin_amdgcn_s_sleep(1);
    }
  }

  STAMP_DECL
  STAMP_PROLOGUE();
  const float c0o = s_c0[o0c], c1o = s_c1[row];  // per-output constants, held in registers
  const float* sp0_o = &s_sp0[o0c * D * SPR * 4];
  // layer 1: the cubic table of edge (o0 -> d = cc0) and the (knot, 1/width) rows of input o0
  const float* sp1_e = &s_sp1[((gl < D ? gl : 0) * H + o0c) * SPR * 4];
  // (lanes that own no layer-1 spline edge read zero rows: see the hidden knot interval below)
  const f2* kr1_o = (act0 && gl < D) ? &s_kr1[o0c * SPR] : s_zkr;
  const int fofs0 = gl * FPL0;
  const bool spl0 = act0 && gl < D;  // lanes owning a layer-0 spline edge (input si)
  const int si0 = spl0 ? gl : 0;

  // training tape: the two layer inputs of evaluation `ev` at tape[(ev B + b)(D + H) + c]
  // TAPE = false (every inference instantiation) carries no tape code at all: the fixed-grid
  // training forward and the dopri5 driver have taped instantiations of their own
  bool taping = TAPE && a.tape != nullptr;
  // the dopri5 tape holds the first tape_cap evaluations (the host re-runs a longer solve)
  int64_t tape_left = DOPRI ? a.dp.tape_cap : 0;
  // dopri5 training rows also hold the evaluation's output k after the two layer inputs
  constexpr int TW = DOPRI ? 2 * D + H : D + H;
  float* tape_b = taping ? a.tape + (valid ? b : 0) * TW : nullptr;
  const int64_t tape_stride = a.B * TW;
  uint64_t bal0 = 0;   // the feature phase's knot ballot (both trajectories' rows of both inputs)
  // (prio_tag: 1 in the younger wave's step loop of the headline kernel, the PRIO_HI / PRIO_LO levels)
  auto eval_body = [&](float xin, auto fact_tag, auto prio_tag) __attribute__((always_inline)) -> float {
    constexpr bool F_ = decltype(fact_tag)::value;
    constexpr int PL = decltype(prio_tag)::value;
    STAMP(6);
    FETODE_MARK("X_FEAT");
    {
      // (1) layer-0 features of input `row`: one sigmoid-of-affine job per lane
      const float pv = x_gate ? (re0 ? xin : prev0) : 0.f;
      const float e = ex2(ffma(xna, xin - pv, xab));
      const float sg = rcp(1.0f + e);
      float val = ffma(sg, x_silu ? xin : xmul, xadd);
      val = x_exp ? e : val;
      val = x_x ? xin : val;
      // knot intervals: lanes c1 < NG compare against their knot (the rest hold +inf); the edge
      // lanes count their input's row of this ballot themselves (v4_edges)
      bal0 = __builtin_amdgcn_ballot_w64(xin >= xknot);
      *xdst = val;
      if (FERRO) prev0 = xin;  // ferro_class.py:409 (meaningful on the gate lane)
      re0 = false;
    }
    STAMP(0);
    // the workgroup is this one wave: its LDS operations execute in order, so the edge reads see the
    // feature writes with no wait on them (a wave barrier only keeps the compiler from reordering)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    STAMP(0);
    FETODE_MARK("EDGES0");
    PRIO_LO();
    // (2) layer-0 edges -> h_o on the group of 3
    float h = v4_edges<D, FLEN0, NI, NPL0, NSL0, FPL0, FERRO, F_, EB0, EBF0, SAME0>(
        L0, sp0_o, s_kr0, gi0, ep0, k20, kE0, cp0, fw0, fofs0, spl0, si0, a.P0.gsl2e, gs0, es0, k2s0, kEs0, cps0, bal0,
        TPW == 2 ? 32 * g : 0);
    if constexpr (TPW == 1) {   // the two halves' partial edge sums (the same sum on both halves)
      float p = h, q2 = h;
      permlane32_swap(p, q2);
      h = p + q2;
    }
    PRIO_HI();
    h = group3_sum(h, cc0) + c0o;   // lane 15 of a row (no group) is never read by a group
    STAMP(2);
    FETODE_MARK("H_FEAT");
    // (3) layer 1 on the group of hidden input o0 (v7): partial sums of BOTH outputs in acc01
    f2 acc01 = splat(0.0f);
    {
      // knot interval of h: each lane counts its KT knots, the counts meet on the group's lanes 0
      // and 1, the owners of the unit's spline edges (dsel1)
      // (a non-finite h counts 0 or all 12 knots: the zero row, no finiteness test needed)
      // Every other lane holds some other sum of counts: the clamp keeps its index inside the
      // tables, and its (knot, 1/width) rows are the zero rows of s_zkr, so its u is 0 and its spline
      // value a finite c0 whenever h is finite (a wrong interval's own u could overflow the cubic),
      // which meets dsel1 = (0, 0); for a non-finite h lanes 0 and 1 already give the reference's
      // NaN to both outputs.
      const int mm = group3_sum_i01(knot_count<KT>(h, hknot), cc0, -1);
      const int mfix = (unsigned)mm < (unsigned)NI ? mm : NI;
      // spline operands by interval (the zero row NI holds (0, 0): u = 0 for finite h, NaN
      // otherwise, as the reference's bases); their LDS latency hides under the pairs
      // PKT (two per wave, where the single exists): the cubic's last two Horner steps share two packed
      // FMAs with the single's last two links, (t u + y, r (-2) + 1) and (. u + x, th cp + 0), the
      // scalar forms' operations (the compiler paired them already, with three moves that put y, x and
      // a second u beside their constants).  y and x are read on their own, each into the low half of
      // a pair whose high half holds the constant, z and w as one pair: two more LDS reads, two
      // fewer VALU moves.
#ifndef FETODE_EXP_NO_PK_TAIL
      constexpr bool PKT = PKS && NSL1 > 0;
#else
      constexpr bool PKT = false;
#endif
      float4 cf = make_float4(0.f, 0.f, 0.f, 0.f);
      float cx = 0.f, cy = 0.f, rs1 = 0.f;   // rs1: the single's last reciprocal
      f2 czw = splat(0.f);
      if constexpr (PKT) {
        cx = lds_now(&sp1_e[mfix * 4]);
        cy = lds_now(&sp1_e[mfix * 4 + 1]);
        czw = lds_now(reinterpret_cast<const f2*>(&sp1_e[mfix * 4 + 2]));
      } else {
        cf = *reinterpret_cast<const float4*>(&sp1_e[mfix * 4]);
      }
      const f2 kw = kr1_o[mfix];
      float sgl = 0.0f;
      if constexpr (FERRO) {
        // every lane of the group forms the gate and exp(gs h) of its input itself (three
        // transcendentals: cheaper than broadcasting them across a group of 3 lanes)
        const float pv = re1 ? h : prev1;
        float w, e = 0.0f, s1 = 0.0f;   // s1: the single's gate sigmoid (PKS)
        if constexpr (PKS) {
          // The gate's chain and the single's first link share their instructions, component for
          // component the scalar form's IEEE operations: (gs h + 0, -gs (h - pv) + 0) is one packed
          // FMA, and the gate's 1 + eg is fma(eg, 1, 1), one rounding of the same sum, beside the
          // single's fma(e, ep, 1) (factored) or its exp2 + 1 (unfactored: a packed add).
          float eg;
          if constexpr (F_) {
            const f2 ge = ex2x2(pfma(gsn1, f2{h, h - pv}, splat(0.0f)));
            e = ge.x;
            eg = ge.y;
            if constexpr (NSL1 > 0) {
              const f2 r = rcpx2(pfma(ge, es1p, splat(1.0f)));
              s1 = r.x;
              w = ffma(r.y, -a.P1.wc, a.P1.wc);
            }
          } else {
            eg = ex2(ffma(-a.P1.gsl2e, h - pv, 0.0f));
            if constexpr (NSL1 > 0) {
              const float d1 = ex2(ffma(a.P1.gsl2e, h, es1));
              const f2 r = rcpx2(f2{eg, d1} + splat(1.0f));
              w = ffma(r.x, -a.P1.wc, a.P1.wc);
              s1 = r.y;
            }
          }
          if constexpr (NSL1 == 0) w = ffma(rcp(1.0f + eg), -a.P1.wc, a.P1.wc);
        } else {
          const float eg = ex2(ffma(-a.P1.gsl2e, h - pv, 0.0f));
          w = ffma(rcp(1.0f + eg), -a.P1.wc, a.P1.wc);   // wc (1 - up)
          e = F_ ? ex2(ffma(a.P1.gsl2e, h, 0.0f)) : 0.0f;
        }
        prev1 = h;   // ferro_class.py:409
        re1 = false;
        const f2 ew = f2{e, w}, xp = f2{h, 0.0f};
        // (no priority drop for these pair rounds: where one takes effect ahead of them the B = 4096
        // solve is 4 us slower, profiles/r08_trim_fwd_ab.log; the phase stays at high priority)
        // (re-tested with the round-10 priority lift, -DFETODE_EXP_L1_DROP: profiles/r10_phase_variants.log)
#ifdef FETODE_EXP_L1_DROP
        PRIO_LO();
#endif
        if constexpr (NSL1 > 0) {
          if constexpr (PKT) {
            const float m = ffma(ew.y, s1, 1.0f);
            const float z = ffma(kEs1, m, k2s1 * xp.x);
            rs1 = rcp(ex2(z) + 1.0f);
          } else if constexpr (PKS) sgl = v4_single_from(s1, ew, xp, k2s1, kEs1, cps1, 0.0f);
          else sgl = v4_single<F_>(ew, xp, es1, k2s1, kEs1, cps1, 0.0f, a.P1.gsl2e);
        }
#pragma unroll
        for (int r = 0; r < NPL1; ++r) acc01 = v4_pair<F_>(ew, xp, ep1[r], k21[r], kE1[r], cp1[r], acc01, a.P1.gsl2e);
#ifdef FETODE_EXP_L1_DROP
        PRIO_HI();
#endif
      }
      // the group's features (SiLU + NB logistic), each weighted for both outputs
      // (PKS: rounds 2 p and 2 p + 1 share the affine FMA and the + 1, each component the scalar round's
      // operation; the accumulation keeps the rounds' order)
#pragma unroll
      for (int p = 0; p < (PKS ? RF1 / 2 : 0); ++p) {
        const f2 sg = rcpx2(splat(1.0f) + ex2x2(pfma(fna2[p], splat(h), fab2[p])));
        const float v0 = fml1[2 * p] != 0.0f ? h * sg.x : sg.x;
        const float v1 = fml1[2 * p + 1] != 0.0f ? h * sg.y : sg.y;
        acc01 = pfma(fwt1[2 * p], splat(v0), acc01);
        acc01 = pfma(fwt1[2 * p + 1], splat(v1), acc01);
      }
#pragma unroll
      for (int r = PKS ? RF1 / 2 * 2 : 0; r < RF1; ++r) {
        const float e = ex2(ffma(fna1[r], h, fab1[r]));
        const float sg = rcp(1.0f + e);
        const float val = fml1[r] != 0.0f ? h * sg : sg;   // SiLU h sigma(h) / logistic sigma
        acc01 = pfma(fwt1[r], splat(val), acc01);
      }
      const float u = (h - kw.x) * kw.y;
      if constexpr (PKT) {
        const float t = ffma(czw.y, u, czw.x);
        const f2 p1 = pfma(f2{t, rs1}, f2{u, -2.0f}, f2{cy, 1.0f});
        const f2 p2 = pfma(p1, f2{u, cps1}, f2{cx, 0.0f});
        acc01 = pfma(dsel1, splat(p2.y + p2.x), acc01);
      } else {
        const float sv = ffma(ffma(ffma(cf.w, u, cf.z), u, cf.y), u, cf.x);
        acc01 = pfma(dsel1, splat(sgl + sv), acc01);   // lane d < 2: single + spline onto output d
      }
#ifndef FETODE_EXPERIMENT_NO_TAPE_STORE
      // the evaluation's tape row in ONE non-temporal store: h_o from the group's first lane, x_row
      // from the row's idle lane 15 (two plain stores cost the B = 4096 taped solve 23 us over none,
      // this one 15: profiles/r06_tape_store_ab.log; the sweep reads the rows long after)
      if (taping && valid && own && ((act0 && cc0 == 0) || q == 15))
        __builtin_nontemporal_store(q == 15 ? xin : h, tape_b + (q == 15 ? row : D + o0));
#endif
    }
    if (taping) {
      tape_b += tape_stride;
      if constexpr (DOPRI) taping = --tape_left > 0;
    }
    STAMP(3);
    // output sums over the half-wave: the permlane16 swap folds the two rows of each output into
    // row d (rows 0 / 2: output 0, rows 1 / 3: output 1), a row sum finishes: k_row on row `row`
    PRIO_HI();
    float p0 = acc01.x, p1 = acc01.y;
    if constexpr (TPW == 1) {   // the two halves' partials first (the same sums on both halves)
      float p = p0, q2 = p0;
      permlane32_swap(p, q2);
      p0 = p + q2;
      float r = p1, t = p1;
      permlane32_swap(r, t);
      p1 = r + t;
    }
    permlane16_swap(p0, p1);
    const float kr = row_sum16(p0 + p1) + c1o;
    STAMP(5);
    FETODE_MARK("END");
    return kr;
  };
  // later schedule chunks (grids past SCH steps / outputs): the first came with the prologue
  auto load_steps = [&](int s0) {
    __syncthreads();
    for (int i = tid; i < SCH && s0 + i < a.n_steps; i += 64) {
      s_dt[i] = a.step_coef[4 * (s0 + i) + 0];
      s_hh[i] = a.step_coef[4 * (s0 + i) + 1];
      s_h6[i] = a.step_coef[4 * (s0 + i) + 2];
    }
    __syncthreads();
  };
  auto load_outs = [&](int j0) {
    __syncthreads();
    for (int i = tid; i < SCH; i += 64) {
      const bool in = j0 + i < a.T;
      s_ostep[i] = in ? a.out_step[j0 + i] : -1;
      s_omode[i] = in ? a.out_mode[j0 + i] : 1;
      s_oslope[i] = in ? a.out_slope[j0 + i] : 0.f;
    }
    __syncthreads();
  };

  auto out_write = [&](int j, float v) __attribute__((always_inline)) {
#ifndef FETODE_EXPERIMENT_NO_OUT
    if (valid && own && c1 == 0) a.solution[((int64_t)j * a.B + b) * D + row] = v;
#endif
  };
  using FT = std::integral_constant<bool, true>;
  using FF = std::integral_constant<bool, false>;
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;

  if constexpr (HOT) {
    // rk4 (torchdiffeq rk_common.rk4_alt_step_func op order); the step's first two output
    // slots are read before its stages and consumed after them, with predicated stores
    int sb = 0, jb = 1, jj = 1;
    // the solution element of output row jj this lane stores, carried and advanced by the row stride
    // with jj (out_write's address, not rebuilt from jj per store)
#ifndef FETODE_EXP_NO_OUT_PTR
    constexpr bool OPTR = true;
#else
    constexpr bool OPTR = false;
#endif
    float* outp = a.solution + (a.B + (valid ? b : 0)) * D + row;
    const int64_t out_stride = a.B * D;
    auto out_next = [&](float v) __attribute__((always_inline)) {
      if constexpr (OPTR) {
#ifndef FETODE_EXPERIMENT_NO_OUT
        if (valid && own && c1 == 0) *outp = v;
#endif
        outp += out_stride;
      } else {
        out_write(jj, v);
      }
      ++jj;
    };
    auto run = [&](auto fact_tag, auto prio_tag, int s_from, int s_to) __attribute__((always_inline)) {
      const float third = 1.0f / 3.0f;
      for (int s = s_from; s < s_to; ++s) {
        if (s - sb == SCH) {
          sb = s;
          load_steps(s);
        }
        if (jj + 1 - jb >= SCH) {
          jb = jj;
          load_outs(jj);
        }
        const int sr = s - sb, jr = jj - jb;
        const float dt = s_dt[sr];
        const int os0 = s_ostep[jr], os1 = s_ostep[jr + 1], om0 = s_omode[jr];
        const float osl0 = s_oslope[jr];
        STAMP(7);
        const float k1 = eval_body(y, fact_tag, prio_tag);
        const float k2 = eval_body(y + (dt * k1) * third, fact_tag, prio_tag);
        const float k3 = eval_body(y + dt * (k2 - k1 * third), fact_tag, prio_tag);
        const float k4 = eval_body(y + dt * ((k1 - k2) + k3), fact_tag, prio_tag);
        const float y1 = y + (((k1 + 3.0f * (k2 + k3)) + k4) * dt) * 0.125f;
        if (os0 == s) {
          // mode / slope as opaque VGPRs: VALU selects instead of scalar branches on the mode
          int m0 = om0;
          float sl0 = osl0;
          asm volatile("" : "+v"(m0), "+v"(sl0));
          const float oip = y + sl0 * (y1 - y);
          const float o1 = m0 == 1 ? y1 : oip;
          out_next(m0 == 0 ? y : o1);
          if (os1 == s) {  // several outputs inside one step (step_size grids)
            while (jj < a.T) {
              if (jj - jb == SCH) {
                jb = jj;
                load_outs(jj);
              }
              if (s_ostep[jj - jb] != s) break;
              const int mode = s_omode[jj - jb];
              out_next(mode == 0 ? y : (mode == 1 ? y1 : y + s_oslope[jj - jb] * (y1 - y)));
            }
          }
        }
        STAMP(1);
        y = y1;
        PROGRESS_STEP(s);
      }
    };
    if constexpr (SKEW) {
      // Priority lift (fetode_fused_set_wave_prio): the younger wave runs its
      // first a.pair[15:8] per cent of the steps with the lifted levels and leads, at twice its partner's
      // speed; for the rest both stand at the same levels again, the older wave leads and catches up,
      // and the two end the solve together instead of one running the last third of it alone.
      const int s_lift = younger ? (int)(((unsigned)a.n_steps * ((unsigned)a.pair >> 8 & 127u) + 50u) / 100u) : 0;
      if (fact) {
        if (s_lift > 0) run(FT{}, P1{}, 0, s_lift);
        run(FT{}, P0{}, s_lift, a.n_steps);
      } else {
        if (s_lift > 0) run(FF{}, P1{}, 0, s_lift);
        run(FF{}, P0{}, s_lift, a.n_steps);
      }
    } else {
      if (fact) run(FT{}, P0{}, 0, a.n_steps);
      else run(FF{}, P0{}, 0, a.n_steps);
    }
  } else {
    auto eval = [&](float xin) __attribute__((always_inline)) -> float {
      if (fact) return eval_body(xin, FT{}, P0{});
      return eval_body(xin, FF{}, P0{});
    };
    if constexpr (MP) {
      // ---- the resident dopri5 driver in passes (fetode_dopri5_set_multipass) ----
      // The launch's grid is smaller than the batch needs: physical workgroup p stands for the virtual
      // workgroups v = p, p + gridDim.x, ... (< P.nblk_global), v being the workgroup the single-pass
      // driver below would run for trajectories 2 v, 2 v + 1.  The step control is the same on every
      // workgroup (it follows from the grid sums alone), so the driver is one control loop whose
      // per-trajectory work between two sums is done for each virtual workgroup in turn: restore what
      // the trajectory carries (y, f0 and the last attempt's y1, k7, mid from the parking area, the
      // hysteresis memory from the state buffer), finish the last attempt (the accept update and the
      // outputs its interpolant covers), run the six stages of the next, park again, arrive.  The
      // arithmetic per trajectory, the tape rows, the attempt log and the statuses are the single-pass
      // driver's; the sums are the virtual grid's (grid_sum2_arrive / grid_sum2_poll): bitwise equal.
      auto drive = [&](auto fact_tag) __attribute__((always_inline)) {
        auto eval = [&](float xin) __attribute__((always_inline)) -> float { return eval_body(xin, fact_tag, P0{}); };
        const DopriParams& P = a.dp;
        const double n_el = P.n_total;
        const unsigned G = gridDim.x, VG = (unsigned)P.nblk_global;
        int nfev = 0, n_att = 0, status = 0;
        unsigned round = 0;
        bool real = false;
        // lane `tid`'s word k of virtual workgroup v: 0 y, 1 f0, 2 y1, 3 k7, 4 mid
        // (the lane numbers go through empty asm statements here and in bind: addresses formed from
        // them stay inside the pass loops instead of being hoisted into registers held across the
        // evaluations)
        auto pk = [&](unsigned v, int k) -> float* {
          int tl = tid;
          asm volatile("" : "+v"(tl));
          return P.park + ((int64_t)v * 5 + k) * 64 + tl;
        };
        // serve virtual workgroup v from evaluation `ev` on (`first`: the trajectory's first evaluation)
        auto bind = [&](unsigned v, int ev, bool first) {
          int gg = g;
          asm volatile("" : "+v"(gg));
          b = (int64_t)v * 2 + gg;
          valid = b < a.B;
          real = valid && c1 == 0;
          if constexpr (FERRO) {
            prev0 = 0.f;
            prev1 = 0.f;
            if (valid) {
              if (x_gate) prev0 = a.state[b * D + row];
              if (act0) prev1 = a.state[a.B * D + b * H + o0];
            }
            re0 = first && (a.init_mask & 1u);
            re1 = first && (a.init_mask & 2u);
          }
          if constexpr (TAPE) {
            tape_left = P.tape_cap - ev;
            taping = a.tape != nullptr && tape_left > 0;
            tape_b = taping ? a.tape + (valid ? b : 0) * TW + (int64_t)ev * tape_stride : nullptr;
          }
        };
        auto stash = [&]() {   // the hysteresis memory back to the state buffer
          if (FERRO && valid) {
            if (x_gate) a.state[b * D + row] = prev0;
            if (act0 && cc0 == 0) a.state[a.B * D + b * H + o0] = prev1;
          }
        };
        auto ktape = [&](float k, int ev) {
          if constexpr (TAPE)
            if (ev < P.tape_cap && valid && c1 == 0) tape_b[D + H + row - tape_stride] = k;
        };
        bool early = false;   // (test knob: grid_sum2_arrive's sample at the round's last arrival)
        auto arrive = [&](unsigned v, double v0, double v1) {
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            v0 += __shfl_xor(v0, o);
            v1 += __shfl_xor(v1, o);
          }
          early = grid_sum2_arrive(P, round, v, v0, v1, v + G >= VG);
        };
        auto poll = [&](double& s0, double& s1) {
          if (grid_sum2_poll(P, round, early, s0, s1)) status = 4;
          ++round;
        };
        // pass 0: f(y0)
        const bool auto_h = !(P.step.first_step > 0.0);
        for (unsigned v = blockIdx.x; v < VG; v += G) {
          bind(v, 0, true);
          const float yv = valid ? a.y0[b * D + row] : 0.f;
          if (valid && c1 == 0) a.solution[b * D + row] = yv;
          const float f0 = eval(yv);
          ktape(f0, 0);
          stash();
          *pk(v, 0) = yv;
          *pk(v, 1) = f0;
          if (auto_h) {
            const float scale = P.atol + P.rtol * fabsf(yv);
            const float q0 = yv / scale, q1 = f0 / scale;
            arrive(v, real ? (double)q0 * q0 : 0.0, real ? (double)q1 * q1 : 0.0);
          }
        }
        ++nfev;
        double dt;
        if (!auto_h) {
          dt = P.step.first_step;
        } else {  // the initial step, the probe as a pass of its own
          double s, s1;
          poll(s, s1);
          float d0, d1, d2, h1;
          const float h0 = dopri_h0(s, s1, n_el, d0, d1);
          for (unsigned v = blockIdx.x; v < VG; v += G) {
            bind(v, 1, false);
            const float yv = *pk(v, 0), f0 = *pk(v, 1);
            const float scale = P.atol + P.rtol * fabsf(yv);
            const float f1 = eval(yv + f0 * h0);
            ktape(f1, 1);
            stash();
            const float q2 = (f1 - f0) / scale;
            arrive(v, real ? (double)q2 * q2 : 0.0, 0.0);
          }
          ++nfev;
          poll(s, s1);
          dt = dopri_dt0(s, n_el, h0, d1, d2, h1);
          if (TAPE && blockIdx.x == 0 && tid == 0) dopri_init_record(P.init_rec, d0, d1, d2, h0, h1);
        }
        // the last attempt's part still to be done per trajectory: its accept update (pend_acc, with
        // its dt32) and the outputs [o_lo, o_hi) its interpolant over [t0s, t1s] covers
        bool pend_acc = false;
        float pend_dt32 = 0.f;
        int o_lo = 1, o_hi = 1;
        double t0s = P.t[0], t1s = P.t[0];
        auto finish_last = [&](unsigned v, float& y, float& f0) __attribute__((always_inline)) {
          y = *pk(v, 0);
          f0 = *pk(v, 1);
          if (pend_acc) {
            const float y1 = *pk(v, 2), kn = *pk(v, 3), mid = *pk(v, 4);
            float co[5];
            dopri_fit(co, y, y1, mid, f0, kn, pend_dt32);
            y = y1;
            f0 = kn;
            for (int j = o_lo; j < o_hi; ++j) out_write(j, dopri_eval(co, (float)((P.t[j] - t0s) / (t1s - t0s))));
            *pk(v, 0) = y;
            *pk(v, 1) = f0;
          }
        };
        int i = 1, n_steps = 0;
        while (status == 0) {
          // the outputs the accepted step covers (the single-pass driver's `for i`, n_steps per output)
          while (i < P.T && !(P.t[i] > t1s)) {
            ++i;
            n_steps = 0;
          }
          o_hi = i;
          if (i >= P.T) break;
          if (n_steps >= P.max_steps) { status = 3; break; }
          const double t0 = t1s;
          if (dopri_underflow(t0, dt)) { status = 2; break; }
          const float dt32 = (float)dt;
          const double t1 = t0 + dt;
          for (unsigned v = blockIdx.x; v < VG; v += G) {
            bind(v, nfev, false);
            float y, f0;
            finish_last(v, y, f0);
            // rk_common._runge_kutta_step: the single-pass driver's stage loop
            float A[6];
#pragma unroll
            for (int q2 = 0; q2 < 6; ++q2) A[q2] = f0 * (P.stc[0][q2] * dt32);
            float err = f0 * (P.stc[0][6] * dt32);
            float mid = f0 * (P.stc[0][7] * dt32);
            float yi = y, kn = f0;
#pragma unroll 1
            for (int st = 0; st < 6; ++st) {
              yi = y + A[0];
              float c[8];
#pragma unroll
              for (int q2 = 0; q2 < 8; ++q2) c[q2] = P.stc[st + 1][q2];
              kn = eval(yi);
              ktape(kn, nfev + st);
#pragma unroll
              for (int q2 = 0; q2 < 5; ++q2) A[q2] = A[q2 + 1] + kn * (c[q2] * dt32);
              err = err + kn * (c[6] * dt32);
              mid = mid + kn * (c[7] * dt32);
            }
            const float y1 = yi;
            stash();
            *pk(v, 2) = y1;
            *pk(v, 3) = kn;
            *pk(v, 4) = mid;
            const float tol = P.atol + P.rtol * fmaxf(fabsf(y), fabsf(y1));
            const float qe = err / tol;
            arrive(v, real ? (double)qe * qe : 0.0, (real && !__builtin_isfinite(y)) ? 1.0 : 0.0);
          }
          nfev += 6;
          pend_acc = false;
          o_lo = o_hi;
          double s, nbad;
          poll(s, nbad);
          if (status) break;
          if (nbad != 0.0) { status = 1; break; }
          const float ratio = dopri_ratio(s, n_el);
          const bool accept = dopri_accept(ratio);
          if (blockIdx.x == 0 && tid == 0) dopri_log_attempt(P.att, n_att, P.max_att, t0, dt, ratio, accept);
          ++n_att;
          pend_acc = accept;
          pend_dt32 = dt32;
          t0s = t0;
          if (accept) t1s = t1;
          dt = dopri_next_dt(dt, ratio, P.step);
          ++n_steps;
        }
        if (pend_acc && o_lo < o_hi)   // the outputs of the last accepted step
          for (unsigned v = blockIdx.x; v < VG; v += G) {
            b = (int64_t)v * 2 + g;
            valid = b < a.B;
            float y, f0;
            finish_last(v, y, f0);
          }
        if (blockIdx.x == 0 && tid == 0) {
          P.stats[0] = nfev;
          P.stats[1] = n_att;
          P.stats[2] = __hip_atomic_load(P.bar + kDpLine * (kDpGroups + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 4 : status;
        }
      };
      if (fact) drive(FT{});
      else drive(FF{});
    } else if constexpr (DOPRI) {
      // the whole driver once per coercive-gate form (as the rk4 path): the evaluations inline
      // one specialised field body, not a runtime choice between two per evaluation
      auto drive = [&](auto fact_tag) __attribute__((always_inline)) {
#ifndef FETODE_EXP_NO_EVAL
        auto eval = [&](float xin) __attribute__((always_inline)) -> float { return eval_body(xin, fact_tag, P0{}); };
#else   // diagnostics only: a trivial field, the reductions and control as is
        auto eval = [&](float xin) -> float { return -0.5f * xin; };
#endif
        // ---- device-resident dopri5 (dopri5.py _Dopri5, lane (traj, dim = row) carries y_row) ----
        const DopriParams& P = a.dp;
        const bool real = valid && c1 == 0;  // one lane per (trajectory, state dim) in the sums
        const double n_el = P.n_total;   // B * D, or the global batch's in a sharded solve
        int nfev = 0, n_att = 0, status = 0;
        unsigned round = 0;
        auto gsum2 = [&](double v0, double v1, double& s0, double& s1) {
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            v0 += __shfl_xor(v0, o);
            v1 += __shfl_xor(v1, o);
          }
          if (grid_sum2(P, round, v0, v1, s0, s1)) status = 4;
        };
        // training: the output of evaluation nfev (the first tape_cap of them) next to its layer
        // inputs, in the row the evaluation just wrote (tape_b has moved past it)
        auto ktape = [&](float k) {
          if constexpr (TAPE)
            if (nfev < P.tape_cap && valid && c1 == 0) tape_b[D + H + row - tape_stride] = k;
        };
        float f0 = eval(y);
        ktape(f0);
        ++nfev;
        double dt;
        if (P.step.first_step > 0.0) {
          dt = P.step.first_step;
        } else {
          const float scale = P.atol + P.rtol * fabsf(y);
          const float q0 = y / scale, q1 = f0 / scale;
          double s, s1;
          gsum2(real ? (double)q0 * q0 : 0.0, real ? (double)q1 * q1 : 0.0, s, s1);
          float d0, d1, d2, h1;
          const float h0 = dopri_h0(s, s1, n_el, d0, d1);
          const float f1 = eval(y + f0 * h0);
          ktape(f1);
          ++nfev;
          const float q2 = (f1 - f0) / scale;
          gsum2(real ? (double)q2 * q2 : 0.0, 0.0, s, s1);
          dt = dopri_dt0(s, n_el, h0, d1, d2, h1);
          if (TAPE && blockIdx.x == 0 && tid == 0) dopri_init_record(P.init_rec, d0, d1, d2, h0, h1);
        }
        float co[5] = {y, 0.f, 0.f, 0.f, 0.f};
        double t0s = P.t[0], t1s = P.t[0];
        for (int i = 1; i < P.T && status == 0; ++i) {
          const double next_t = P.t[i];
          int n_steps = 0;
          while (next_t > t1s) {
            if (n_steps >= P.max_steps) { status = 3; break; }
            const double t0 = t1s;
            if (dopri_underflow(t0, dt)) { status = 2; break; }
            const float dt32 = (float)dt;
            const double t1 = t0 + dt;
            // rk_common._runge_kutta_step in fetode_lincomb's op order, accumulated as the stages
            // arrive: A[i] is stage s+1+i's sum k0 c0 + k1 c1 + ... (the same left-to-right sums)
            float A[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) A[q] = f0 * (P.stc[0][q] * dt32);
            float err = f0 * (P.stc[0][6] * dt32);
            float mid = f0 * (P.stc[0][7] * dt32);
            float yi = y, kn = f0;
#pragma unroll 1
            for (int st = 0; st < 6; ++st) {
              yi = y + A[0];
              // stage column st + 1 into SGPRs before the evaluation (the loads complete under it)
              float c[8];
#pragma unroll
              for (int q = 0; q < 8; ++q) c[q] = P.stc[st + 1][q];
              kn = eval(yi);
              ktape(kn);
              ++nfev;
              // entries past the tableau (coefficient 0) are never read again
#pragma unroll
              for (int q = 0; q < 5; ++q) A[q] = A[q + 1] + kn * (c[q] * dt32);
              err = err + kn * (c[6] * dt32);
              mid = mid + kn * (c[7] * dt32);
              STAMP(6);
            }
            const float y1 = yi;
            const float tol = P.atol + P.rtol * fmaxf(fabsf(y), fabsf(y1));
            const float qe = err / tol;
            double s, nbad;
            gsum2(real ? (double)qe * qe : 0.0, (real && !__builtin_isfinite(y)) ? 1.0 : 0.0, s, nbad);
            STAMP(1);
            if (status) break;
            if (nbad != 0.0) { status = 1; break; }
            const float ratio = dopri_ratio(s, n_el);
            const bool accept = dopri_accept(ratio);
            if (blockIdx.x == 0 && tid == 0) dopri_log_attempt(P.att, n_att, P.max_att, t0, dt, ratio, accept);
            ++n_att;
            if (accept) {
              dopri_fit(co, y, y1, mid, f0, kn, dt32);
              y = y1;
              f0 = kn;
              t0s = t0;
              t1s = t1;
            } else {
              t0s = t0;
            }
            dt = dopri_next_dt(dt, ratio, P.step);
            ++n_steps;
            STAMP(7);
          }
          if (status) break;
          out_write(i, dopri_eval(co, (float)((next_t - t0s) / (t1s - t0s))));
        }
        if (P.xr_world > 1 && blockIdx.x == 0 && tid == 0)   // the exchange workgroup may stop
          __hip_atomic_store(dp_fin(P), round + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (blockIdx.x == 0 && tid == 0) {
          P.stats[0] = nfev;
          P.stats[1] = n_att;
          P.stats[2] = __hip_atomic_load(P.bar + kDpLine * (kDpGroups + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 4 : status;
        }
      };
      if (fact) drive(FT{});
      else drive(FF{});
    } else if (a.single_eval) {
      const float f = eval(y);
      if (valid && c1 == 0) a.eval_out[b * D + row] = f;
    } else {
      const int ns = a.method == FETODE_RK4 || a.method == FETODE_RK4_CLASSIC ? 4
                     : a.method == FETODE_MIDPOINT ? 2 : 1;
      const float third = 1.0f / 3.0f;
      int sb = 0, jb = 1, jj = 1;
      for (int s = 0; s < a.n_steps; ++s) {
        if (s - sb == SCH) {
          sb = s;
          load_steps(s);
        }
        const float dt = s_dt[s - sb], hh = s_hh[s - sb], h6 = s_h6[s - sb];
        float k1 = 0.f, k2 = 0.f, k3 = 0.f, k4 = 0.f;
        for (int st = 0; st < ns; ++st) {
          float xin = y;
          if (a.method == FETODE_RK4) {
            if (st == 1) xin = y + (dt * k1) * third;
            else if (st == 2) xin = y + dt * (k2 - k1 * third);
            else if (st == 3) xin = y + dt * ((k1 - k2) + k3);
          } else if (a.method == FETODE_RK4_CLASSIC) {
            if (st == 1) xin = y + hh * k1;
            else if (st == 2) xin = y + hh * k2;
            else if (st == 3) xin = y + dt * k3;
          } else if (a.method == FETODE_MIDPOINT) {
            if (st == 1) xin = y + k1 * hh;
          }
          const float kk = eval(xin);
          if (st == 0) k1 = kk;
          else if (st == 1) k2 = kk;
          else if (st == 2) k3 = kk;
          else k4 = kk;
        }
        float y1;
        if (a.method == FETODE_RK4) y1 = y + (((k1 + 3.0f * (k2 + k3)) + k4) * dt) * 0.125f;
        else if (a.method == FETODE_RK4_CLASSIC) y1 = y + h6 * (((k1 + 2.0f * k2) + 2.0f * k3) + k4);
        else if (a.method == FETODE_MIDPOINT) y1 = y + dt * k2;
        else y1 = y + dt * k1;
        while (jj < a.T) {
          if (jj - jb == SCH) {
            jb = jj;
            load_outs(jj);
          }
          if (s_ostep[jj - jb] != s) break;
          const int mode = s_omode[jj - jb];
          out_write(jj, mode == 0 ? y : (mode == 1 ? y1 : y + s_oslope[jj - jb] * (y1 - y)));
          ++jj;
        }
        y = y1;
      }
    }
  }
  if (!MP && FERRO && valid && own) {   // (MP: stored per pass)
    if (x_gate) a.state[b * D + row] = prev0;
    if (act0 && cc0 == 0) a.state[a.B * D + b * H + o0] = prev1;
  }
  STAMP_FLUSH();
  PROGRESS_FLUSH();
