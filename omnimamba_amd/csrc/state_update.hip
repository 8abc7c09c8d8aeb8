// state_update.hip -- SSM recurrence of decode, one token (omk_selective_state_update) or T tokens of a follow-up turn
// (omk_selective_state_extend, below):  s <- s*exp(dt*A) + dt*x (x) B ; y = s.C + D*x ; y *= silu(z)
//
// Pure bandwidth on the state (2 * B*H*P*N * s_state bytes per layer-step, 4.19 MB
// at B=1 fp32 for the 1.3B block).  A row of the state (one (b, h, p), N values) is spread over LPR lanes with
// VEC contiguous elements each (16-byte loads for fp32 VEC=4), a wave holds 64/LPR rows, y is reduced with wave
// shuffles; B_t / C_t rows are shared by every row of a head and stay in L1/L2.  In place, no allocation, no
// host scalars: safe to capture in a hipGraph (models/stage2/generation.py:372-434 replays this step 255 times).
#include "omk_common.h"

namespace omk {

struct SuArgs {
  void* state; const void* x; const void* dt; const void* A; const void* Bm; const void* Cm; const void* D; const void* z;
  const void* dtb; void* out;
  const int* sbi;                                     // ABI 8: slot of row b in the state pool (null: row b), pool rows
  int64_t ssb, ssh, ssp, ssn, xsb, xsh, xsp, dsb, dsh, dsp, ash, asp, asn, bsb, bsg, bsn, csb, csg, csn;
  int64_t Dsh, Dsp, zsb, zsh, zsp, tsh, tsp, osb, osh, osp;
  int B, H, P, N, G, softplus, xdt, dtdt, adt, ddt, tbdt, pool;
};

// the state row of batch row b: its slot in the pool, or -1 for a padding row (negative or out-of-pool index).  b is
// workgroup-uniform, so this is one scalar load in front of the state address, and a padding row leaves the workgroup as a whole.
template <class Args>
__device__ __forceinline__ int su_slot(const Args& a, int b) {
  if (!a.sbi) return b;
  const int s = a.sbi[b];
  return (s >= 0 && s < a.pool) ? s : -1;
}

template <class TS, class TX, int VEC, int LPR>
__global__ __launch_bounds__(256) void state_update_kernel(SuArgs a) {
  constexpr int RPW = 64 / LPR;                       // rows per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane % LPR, rw = lane / LPR;
  const int rows_per_block = RPW * (blockDim.x >> 6);
  const int pblocks = (a.P + rows_per_block - 1) / rows_per_block;
  const int pb = blockIdx.x % pblocks, h = (blockIdx.x / pblocks) % a.H, b = blockIdx.x / (pblocks * a.H);
  const int p = pb * rows_per_block + wave * RPW + rw;
  const bool live = p < a.P;
  const int pp = live ? p : a.P - 1;                 // keep every lane in the shuffles
  const int g = h / (a.H / a.G);
  const int sb = su_slot(a, b);
  if (sb < 0) {                                      // padding row: no state traffic, zeros out
    if (live && lr == 0) store_rt(a.out, (int64_t)b * a.osb + (int64_t)h * a.osh + (int64_t)p * a.osp, a.xdt, 0.f);
    return;
  }
  // every independent load first: the scalars of the row and (vector path, N <= LPR * VEC: one step) its state / B / C
  // (requests first, conversions behind the last request: raw_rt_flat / cvt_rt_flat in omk_common.h; D and the gate of the row ride along
  // from clamped / dummy addresses instead of sitting under branches behind the reduction)
  const RawElem q_dt = raw_rt_flat(a.dt, (int64_t)b * a.dsb + (int64_t)h * a.dsh + (int64_t)pp * a.dsp, a.dtdt);
  const RawElem q_dtb = raw_rt_flat(a.dtb ? a.dtb : a.dt, a.dtb ? (int64_t)h * a.tsh + (int64_t)pp * a.tsp : 0, a.dtb ? a.tbdt : a.dtdt);
  const RawElem q_x = raw_rt_flat(a.x, (int64_t)b * a.xsb + (int64_t)h * a.xsh + (int64_t)pp * a.xsp, a.xdt);
  const bool tied = a.asn == 0;
  const RawElem q_A = raw_rt_flat(a.A, (int64_t)h * a.ash + (int64_t)pp * a.asp, a.adt);
  const RawElem q_D = raw_rt_flat(a.D ? a.D : a.A, a.D ? (int64_t)h * a.Dsh + (int64_t)pp * a.Dsp : 0, a.D ? a.ddt : a.adt);
  const RawElem q_z = raw_rt_flat(a.z ? a.z : a.x, a.z ? (int64_t)b * a.zsb + (int64_t)h * a.zsh + (int64_t)pp * a.zsp : 0, a.xdt);
  TS* s = (TS*)a.state + (int64_t)sb * a.ssb + (int64_t)h * a.ssh + (int64_t)pp * a.ssp;
  const TX* Bp = (const TX*)a.Bm + (int64_t)b * a.bsb + (int64_t)g * a.bsg;
  const TX* Cp = (const TX*)a.Cm + (int64_t)b * a.csb + (int64_t)g * a.csg;
  float sv0[VEC], bv0[VEC], cv0[VEC];
  const bool one_step = VEC > 1 && a.N <= LPR * VEC;
  if constexpr (VEC > 1) {
    const int n0c = lr * VEC < a.N ? lr * VEC : 0;   // clamped: lanes past N re-read the row start and are not stored
    load_vec<TS, VEC>(s + n0c, sv0); load_vec<TX, VEC>(Bp + n0c, bv0); load_vec<TX, VEC>(Cp + n0c, cv0);
  }
  float dt = cvt_rt_flat(q_dt, a.dtdt);
  const float dtbv = cvt_rt_flat(q_dtb, a.dtb ? a.tbdt : a.dtdt), xv = cvt_rt_flat(q_x, a.xdt), Av = cvt_rt_flat(q_A, a.adt);
  const float Dv = cvt_rt_flat(q_D, a.D ? a.ddt : a.adt), zv = cvt_rt_flat(q_z, a.xdt);
  if (a.dtb) dt += dtbv;
  if (a.softplus) dt = softplus_f(dt);
  const float xdt = xv * dt;
  const float dA_t = tied ? expf(dt * Av) : 0.f;
  float acc = 0.f;
  for (int n0 = lr * VEC; n0 < a.N; n0 += LPR * VEC) {
    float sv[VEC], bv[VEC], cv[VEC];
    if constexpr (VEC > 1) {             // unit stride on n checked on the host
      if (n0 == lr * VEC) {
#pragma unroll
        for (int i = 0; i < VEC; i++) { sv[i] = sv0[i]; bv[i] = bv0[i]; cv[i] = cv0[i]; }
      } else {
        load_vec<TS, VEC>(s + n0, sv); load_vec<TX, VEC>(Bp + n0, bv); load_vec<TX, VEC>(Cp + n0, cv);
      }
    } else {
      bv[0] = to_f32(Bp[(int64_t)n0 * a.bsn]); cv[0] = to_f32(Cp[(int64_t)n0 * a.csn]); sv[0] = to_f32(s[(int64_t)n0 * a.ssn]);
    }
#pragma unroll
    for (int i = 0; i < VEC; i++) {
      float dA = tied ? dA_t : expf(dt * load_rt(a.A, (int64_t)h * a.ash + (int64_t)pp * a.asp + (int64_t)(n0 + i) * a.asn, a.adt));
      sv[i] = sv[i] * dA + xdt * bv[i];
      acc += sv[i] * cv[i];
    }
    if (live) {
      if constexpr (VEC > 1) store_vec<TS, VEC>(s + n0, sv);
      else s[(int64_t)n0 * a.ssn] = from_f32<TS>(sv[0]);
    }
  }
  (void)one_step;
#pragma unroll
  for (int m = LPR / 2; m >= 1; m >>= 1) acc += shfl_xor(acc, m);
  if (live && lr == 0) {
    float y = acc;
    if (a.D) y += xv * Dv;
    if (a.z) y *= silu_f(zv);
    store_rt(a.out, (int64_t)b * a.osb + (int64_t)h * a.osh + (int64_t)p * a.osp, a.xdt, y);
  }
}

// Mamba-2's configuration (A, dt, dt_bias tied over (p, n); one vector step per row: N == 4 LPR; unit strides), RPT rows
// per lane group: the per-head scalars and B / C are loaded once, the RPT state vectors fly together.  With one row per
// lane group (kernel above) a batch-8 step is 16 k waves of ten dependent-ish loads each: 17.4 us for 33.5 MB.
template <class TS, class TX, int LPR, int RPT>
__global__ __launch_bounds__(256) void state_update_tied_kernel(SuArgs a) {
  constexpr int VEC = 4, RPW = 64 / LPR, RPB = RPW * 4;         // rows per workgroup and pass
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane % LPR, rw = lane / LPR;
  const int pblocks = a.P / (RPB * RPT);                       // host: P % (RPB * RPT) == 0
  const int pb = blockIdx.x % pblocks, h = (blockIdx.x / pblocks) % a.H, b = blockIdx.x / (pblocks * a.H);
  const int g = h / (a.H / a.G);
  const int p0 = pb * RPB * RPT + wave * RPW + rw, n0 = lr * VEC;
  const int sb = su_slot(a, b);
  if (sb < 0) {                                                // padding row: no state traffic, zeros out
    if (lr == 0) {
#pragma unroll
      for (int k = 0; k < RPT; k++) ((TX*)a.out)[(int64_t)b * a.osb + (int64_t)h * a.osh + (int64_t)(p0 + k * RPB) * a.osp] = from_f32<TX>(0.f);
    }
    return;
  }
  TS* s = (TS*)a.state + (int64_t)sb * a.ssb + (int64_t)h * a.ssh + n0;
  float sv[RPT][VEC], xv[RPT], bv[VEC], cv[VEC];
#pragma unroll
  for (int k = 0; k < RPT; k++) load_vec<TS, VEC>(s + (int64_t)(p0 + k * RPB) * a.ssp, sv[k]);
  load_vec<TX, VEC>((const TX*)a.Bm + (int64_t)b * a.bsb + (int64_t)g * a.bsg + n0, bv);
  load_vec<TX, VEC>((const TX*)a.Cm + (int64_t)b * a.csb + (int64_t)g * a.csg + n0, cv);
  // every other request of the thread right behind them, none under a branch and none followed by its conversion (raw_rt_flat /
  // cvt_rt_flat): x, gate and D of its four rows, the three tied scalars.  Before round 5 dt, dt_bias, A were three dependent round trips
  // in front of the arithmetic and D, gate two more per row behind the reduction: 19.9 us for 33.5 MB at eight fp32 sequences.
  TX xq[RPT], zq[RPT];
  RawElem Dq[RPT];
#pragma unroll
  for (int k = 0; k < RPT; k++) {
    const int64_t p = p0 + k * RPB;
    const int64_t xi = (int64_t)b * a.xsb + (int64_t)h * a.xsh + p * a.xsp;
    xq[k] = ((const TX*)a.x)[xi];
    zq[k] = ((const TX*)(a.z ? a.z : a.x))[a.z ? (int64_t)b * a.zsb + (int64_t)h * a.zsh + p * a.zsp : xi];   // (no gate: x once more, not used)
    Dq[k] = raw_rt_flat(a.D ? a.D : a.A, a.D ? (int64_t)h * a.Dsh + p * a.Dsp : 0, a.D ? a.ddt : a.adt);
  }
  const RawElem q_dt = raw_rt_flat(a.dt, (int64_t)b * a.dsb + (int64_t)h * a.dsh, a.dtdt);
  const RawElem q_dtb = raw_rt_flat(a.dtb ? a.dtb : a.dt, a.dtb ? (int64_t)h * a.tsh : 0, a.dtb ? a.tbdt : a.dtdt);
  const RawElem q_A = raw_rt_flat(a.A, (int64_t)h * a.ash, a.adt);
#pragma unroll
  for (int k = 0; k < RPT; k++) xv[k] = to_f32(xq[k]);
  float dt = cvt_rt_flat(q_dt, a.dtdt);
  const float dtbv = cvt_rt_flat(q_dtb, a.dtb ? a.tbdt : a.dtdt), Av = cvt_rt_flat(q_A, a.adt);
  if (a.dtb) dt += dtbv;
  if (a.softplus) dt = softplus_f(dt);
  const float dA = expf(dt * Av);
  float acc[RPT];
#pragma unroll
  for (int k = 0; k < RPT; k++) {
    acc[k] = 0.f;
    const float xdt = xv[k] * dt;
#pragma unroll
    for (int i = 0; i < VEC; i++) {
      sv[k][i] = sv[k][i] * dA + xdt * bv[i];
      acc[k] += sv[k][i] * cv[i];
    }
    store_vec<TS, VEC>(s + (int64_t)(p0 + k * RPB) * a.ssp, sv[k]);
  }
#pragma unroll
  for (int k = 0; k < RPT; k++)
#pragma unroll
    for (int m = LPR / 2; m >= 1; m >>= 1) acc[k] += shfl_xor(acc[k], m);
  if (lr == 0) {
#pragma unroll
    for (int k = 0; k < RPT; k++) {
      const int p = p0 + k * RPB;
      float y = acc[k];
      if (a.D) y += xv[k] * cvt_rt_flat(Dq[k], a.ddt);
      if (a.z) y *= silu_f(to_f32(zq[k]));
      ((TX*)a.out)[(int64_t)b * a.osb + (int64_t)h * a.osh + (int64_t)p * a.osp] = from_f32<TX>(y);
    }
  }
}

// ---- multi-token extend (ABI 9): T tokens of one sequence applied to a cached state in one pass (a follow-up turn) -------------
// Lane layout of state_update_tied_kernel (LPR = N / 4 lanes of VEC 4 per state row, one row per lane group): the row is loaded once,
// stays in fp32 registers for all T tokens and is stored once.  Per token the recurrence is the single-token kernels' expression for
// expression (same expf / softplus, same operand order), so an fp32 state ends bit-identical to T omk_selective_state_update calls.
// The token loop is a chain of dependent updates with little else to hide memory behind (one (b, h) is 4 - 16 workgroups), so the
// requests of token t + SE_PF (B_t / C_t slice of the lane, x, gate and dt of the row) are issued before token t is computed: a ring of
// SE_PF raw register sets, converted only when their token comes up (every request in flight while SE_PF - 1 tokens are computed).
struct SeArgs {
  void* state; const void* x; const void* dt; const void* A; const void* Bm; const void* Cm; const void* D; const void* z;
  const void* dtb; void* out;
  const int* sbi;
  const int* lens;                                    // ABI 13: tokens row b applies (null: T), clamped to 0 .. T on the device
  int64_t ssb, ssh, ssp, xsb, xst, xsh, xsp, dsb, dst, dsh, dsp, ash, asp, asn, bsb, bst, bsg, csb, cst, csg;
  int64_t Dsh, Dsp, zsb, zst, zsh, zsp, tsh, tsp, osb, ost, osh, osp;
  int B, T, H, P, N, G, softplus, xdt, dtdt, adt, ddt, tbdt, pool;
};

constexpr int SE_PF = 4;                              // prefetch distance in tokens

// s * dA + xdt * b rounded as the single-token kernels' `sv * dA + xdt * bv` compiles for gfx950 (-ffp-contract=fast: v_mul s * dA,
// then v_fmac xdt * b into it).  Spelled out because inside the token loop the contraction is free to pick the other product; the
// emulator build does not contract.
__device__ __forceinline__ float se_recur(float s, float dA, float xdt, float b) {
#ifdef OMK_EMU
  return s * dA + xdt * b;
#else
  return __builtin_fmaf(xdt, b, s * dA);
#endif
}

// the number of tokens batch row b applies: seq_lens[b] clamped to 0 .. T.  Workgroup-uniform like su_slot: one scalar load.
__device__ __forceinline__ int se_len(const SeArgs& a, int b) {
  const int n = a.lens[b];
  return n < 0 ? 0 : (n < a.T ? n : a.T);
}

// RAGGED (ABI 13, seq_lens present): the token loop, the prefetch ring and the tail re-reads run on the row's own length nT, outputs behind
// it are zeros.  An instantiation of its own: as a run-time branch the length cost every caller two VGPRs and the f16-activation LPR 32
// kernels a wave per SIMD; without seq_lens the kernel is the ABI 12 one to the register.
template <class TS, class TX, int LPR, bool RAGGED>
__global__ __launch_bounds__(256) void state_extend_kernel(SeArgs a) {
  constexpr int VEC = 4, RPW = 64 / LPR, RPB = RPW * 4;       // host: N == LPR * VEC
  using VT = vec_t<TX, VEC>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane % LPR, rw = lane / LPR;
  const int pblocks = (a.P + RPB - 1) / RPB;
  const int pb = blockIdx.x % pblocks, h = (blockIdx.x / pblocks) % a.H, b = blockIdx.x / (pblocks * a.H);
  const int p = pb * RPB + wave * RPW + rw;
  const bool live = p < a.P;
  const int pp = live ? p : a.P - 1;                 // keep every lane in the shuffles
  const int g = h / (a.H / a.G), n0 = lr * VEC;
  TX* out = (TX*)a.out + (int64_t)b * a.osb + (int64_t)h * a.osh + (int64_t)pp * a.osp;
  const int sb = su_slot(a, b);
  const int nT = RAGGED ? se_len(a, b) : a.T;
  if (sb < 0 || (RAGGED && nT == 0)) {               // padding row or a row of length 0: no state traffic, zeros out
    if (live && lr == 0)
      for (int t = 0; t < a.T; t++) out[(int64_t)t * a.ost] = from_f32<TX>(0.f);
    return;
  }
  const TX* xp = (const TX*)a.x + (int64_t)b * a.xsb + (int64_t)h * a.xsh + (int64_t)pp * a.xsp;
  const TX* zp = (const TX*)(a.z ? a.z : a.x) + (a.z ? (int64_t)b * a.zsb + (int64_t)h * a.zsh + (int64_t)pp * a.zsp : 0);
  const int64_t zst = a.z ? a.zst : 0;                // (no gate: x's first token over and over, not used)
  const int64_t dto = (int64_t)b * a.dsb + (int64_t)h * a.dsh + (int64_t)pp * a.dsp;
  const TX* Bp = (const TX*)a.Bm + (int64_t)b * a.bsb + (int64_t)g * a.bsg + n0;
  const TX* Cp = (const TX*)a.Cm + (int64_t)b * a.csb + (int64_t)g * a.csg + n0;
  // ring of raw requests: slot j holds token t0 + j
  VT bq[SE_PF], cq[SE_PF];
  TX xq[SE_PF], zq[SE_PF];
  RawElem dq[SE_PF];
  auto issue = [&](int j, int t) {
    bq[j] = *reinterpret_cast<const VT*>(Bp + (int64_t)t * a.bst);
    cq[j] = *reinterpret_cast<const VT*>(Cp + (int64_t)t * a.cst);
    xq[j] = xp[(int64_t)t * a.xst];
    zq[j] = zp[(int64_t)t * zst];
    dq[j] = raw_rt_flat(a.dt, dto + (int64_t)t * a.dst, a.dtdt);
  };
#pragma unroll
  for (int j = 0; j < SE_PF; j++) issue(j, j < nT ? j : nT - 1);
  // the per-row constants and the state row, right behind the first tokens' requests
  TS* s = (TS*)a.state + (int64_t)sb * a.ssb + (int64_t)h * a.ssh + (int64_t)pp * a.ssp + n0;
  float sv[VEC], Av[VEC];
  load_vec<TS, VEC>(s, sv);
  const bool tied = a.asn == 0;
  const int64_t ao = (int64_t)h * a.ash + (int64_t)pp * a.asp;
#pragma unroll
  for (int i = 0; i < VEC; i++) Av[i] = cvt_rt_flat(raw_rt_flat(a.A, tied ? ao : ao + (int64_t)(n0 + i) * a.asn, a.adt), a.adt);
  const RawElem q_dtb = raw_rt_flat(a.dtb ? a.dtb : a.dt, a.dtb ? (int64_t)h * a.tsh + (int64_t)pp * a.tsp : 0, a.dtb ? a.tbdt : a.dtdt);
  const RawElem q_D = raw_rt_flat(a.D ? a.D : a.A, a.D ? (int64_t)h * a.Dsh + (int64_t)pp * a.Dsp : 0, a.D ? a.ddt : a.adt);
  const float dtbv = cvt_rt_flat(q_dtb, a.dtb ? a.tbdt : a.dtdt), Dv = cvt_rt_flat(q_D, a.D ? a.ddt : a.adt);
  for (int t0 = 0; t0 < nT; t0 += SE_PF) {
#pragma unroll
    for (int j = 0; j < SE_PF; j++) {
      const int t = t0 + j;
      float bv[VEC], cv[VEC];
#pragma unroll
      for (int i = 0; i < VEC; i++) { bv[i] = to_f32(bq[j].e[i]); cv[i] = to_f32(cq[j].e[i]); }
      const float xv = to_f32(xq[j]), zv = to_f32(zq[j]);
      float dt = cvt_rt_flat(dq[j], a.dtdt);
      const int tn = t + SE_PF < nT ? t + SE_PF : nT - 1;     // clamped: the tail re-reads the row's last token, never past it
      issue(j, tn);
      if (t < nT) {                                             // workgroup-uniform
        if (a.dtb) dt += dtbv;
        if (a.softplus) dt = softplus_f(dt);
        const float xdt = xv * dt;
        const float dA_t = tied ? expf(dt * Av[0]) : 0.f;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < VEC; i++) {
          const float dA = tied ? dA_t : expf(dt * Av[i]);
          sv[i] = se_recur(sv[i], dA, xdt, bv[i]);
          acc += sv[i] * cv[i];
        }
#pragma unroll
        for (int m = LPR / 2; m >= 1; m >>= 1) acc += shfl_xor(acc, m);
        if (live && lr == 0) {
          float y = acc;
          if (a.D) y += xv * Dv;
          if (a.z) y *= silu_f(zv);
          out[(int64_t)t * a.ost] = from_f32<TX>(y);
        }
      }
    }
  }
  if (live) store_vec<TS, VEC>(s, sv);              // the one rounding to the storage dtype, after token nT - 1
  if constexpr (RAGGED) {                             // behind the row's length: zeros, from the lanes that store y
    if (live && lr == 0)
      for (int t = nT; t < a.T; t++) out[(int64_t)t * a.ost] = from_f32<TX>(0.f);
  }
}

}  // namespace omk

using namespace omk;

extern "C" int omk_selective_state_update(const OmkStateUpdate* p, omk_stream stream) {
  OMK_REQUIRE(p && present(p->state) && present(p->x) && present(p->dt) && present(p->A) && present(p->Bm) && present(p->Cm) && present(p->out),
              "selective_state_update: state, x, dt, A, B, C, out required");
  OMK_REQUIRE(p->state.ndim == 4 && p->x.ndim == 3 && p->dt.ndim == 3 && p->A.ndim == 3 && p->Bm.ndim == 3 && p->Cm.ndim == 3 && p->out.ndim == 3,
              "selective_state_update: state (B,H,P,N), x/dt/out (B,H,P), A (H,P,N), B/C (B,G,N)");
  SuArgs a = {};
  // with slot indices the state is a pool of any number of rows and the batch is x's; without, they are one and the same
  const bool indexed = present(p->state_batch_indices);
  a.B = (int)(indexed ? p->x.shape[0] : p->state.shape[0]); a.pool = (int)p->state.shape[0];
  a.H = (int)p->state.shape[1]; a.P = (int)p->state.shape[2]; a.N = (int)p->state.shape[3]; a.G = (int)p->Bm.shape[1];
  OMK_REQUIRE(indices_ok(p->state_batch_indices, a.B), "selective_state_update: state_batch_indices must be contiguous int32 (B)");
  a.sbi = (const int*)p->state_batch_indices.data;
  OMK_REQUIRE(a.G > 0 && a.H % a.G == 0, "selective_state_update: H must be a multiple of ngroups");
  OMK_REQUIRE(p->x.shape[0] == a.B && p->x.shape[1] == a.H && p->x.shape[2] == a.P, "selective_state_update: x shape");
  OMK_REQUIRE(p->Bm.shape[0] == a.B && p->Bm.shape[2] == a.N && p->Cm.shape[1] == a.G && p->Cm.shape[2] == a.N, "selective_state_update: B/C shape");
  OMK_REQUIRE(p->Bm.dtype == p->x.dtype && p->Cm.dtype == p->x.dtype && p->out.dtype == p->x.dtype, "selective_state_update: B, C, out must have x's dtype");
  OMK_REQUIRE(!present(p->z) || p->z.dtype == p->x.dtype, "selective_state_update: z dtype");
  a.state = p->state.data; a.x = p->x.data; a.dt = p->dt.data; a.A = p->A.data; a.Bm = p->Bm.data; a.Cm = p->Cm.data;
  a.D = p->D.data; a.z = p->z.data; a.dtb = p->dt_bias.data; a.out = p->out.data;
  a.ssb = p->state.stride[0]; a.ssh = p->state.stride[1]; a.ssp = p->state.stride[2]; a.ssn = p->state.stride[3];
  a.xsb = p->x.stride[0]; a.xsh = p->x.stride[1]; a.xsp = p->x.stride[2];
  a.dsb = p->dt.stride[0]; a.dsh = p->dt.stride[1]; a.dsp = p->dt.stride[2];
  a.ash = p->A.stride[0]; a.asp = p->A.stride[1]; a.asn = p->A.stride[2];
  a.bsb = p->Bm.stride[0]; a.bsg = p->Bm.stride[1]; a.bsn = p->Bm.stride[2];
  a.csb = p->Cm.stride[0]; a.csg = p->Cm.stride[1]; a.csn = p->Cm.stride[2];
  if (present(p->D)) { a.Dsh = p->D.stride[0]; a.Dsp = p->D.ndim > 1 ? p->D.stride[1] : 0; }
  if (present(p->z)) { a.zsb = p->z.stride[0]; a.zsh = p->z.stride[1]; a.zsp = p->z.stride[2]; }
  if (present(p->dt_bias)) { a.tsh = p->dt_bias.stride[0]; a.tsp = p->dt_bias.ndim > 1 ? p->dt_bias.stride[1] : 0; }
  a.osb = p->out.stride[0]; a.osh = p->out.stride[1]; a.osp = p->out.stride[2];
  a.softplus = p->dt_softplus; a.xdt = p->x.dtype; a.dtdt = p->dt.dtype; a.adt = p->A.dtype; a.ddt = p->D.dtype; a.tbdt = p->dt_bias.dtype;
  if ((int64_t)a.B * a.H * a.P * a.N == 0) return OMK_OK;
  // vector path: N % 4 == 0, unit stride on n everywhere, 16-byte (fp32) / 8-byte (16-bit) aligned rows
  const int sb = (int)dtype_size(p->state.dtype), xb = (int)dtype_size(p->x.dtype);
  bool vec = a.N % 4 == 0 && a.ssn == 1 && a.bsn == 1 && a.csn == 1 &&
             ((uintptr_t)p->state.data % (4 * sb)) == 0 && ((uintptr_t)p->Bm.data % (4 * xb)) == 0 && ((uintptr_t)p->Cm.data % (4 * xb)) == 0 &&
             a.ssb % 4 == 0 && a.ssh % 4 == 0 && a.ssp % 4 == 0 && a.bsb % 4 == 0 && a.bsg % 4 == 0 && a.csb % 4 == 0 && a.csg % 4 == 0;
  dim3 block(256);
  // Mamba-2 decode with several sequences: tied scalars, one vector step per row, four rows per lane group
  {
    const int lpr = a.N / 4;
    const bool tied = vec && a.asn == 0 && a.asp == 0 && a.dsp == 0 && (!present(p->dt_bias) || a.tsp == 0) && (lpr == 32 || lpr == 16) && a.N % 4 == 0 &&
                      (!present(p->z) || p->z.dtype == p->x.dtype) && p->out.dtype == p->x.dtype &&   // (an ABSENT gate has dtype 0 = fp32: the bf16 decode at batch 8 fell to the row kernel)
                      (int64_t)a.B * a.H * a.P * a.N >= ((int64_t)1 << 21);
    const int rpb = tied ? (64 / lpr) * 4 : 1;
    if (tied && a.P % (rpb * 4) == 0) {
      dim3 grid((unsigned)((int64_t)a.B * a.H * (a.P / (rpb * 4))));
#define SU_TIED(TS, TX) do { if (lpr == 32) OMK_LAUNCH((state_update_tied_kernel<TS, TX, 32, 4>), grid, block, 0, stream, a); \
                             else OMK_LAUNCH((state_update_tied_kernel<TS, TX, 16, 4>), grid, block, 0, stream, a); } while (0)
      OMK_DISPATCH_DTYPE(p->state.dtype, TS, OMK_DISPATCH_DTYPE(p->x.dtype, TX, SU_TIED(TS, TX)));
#undef SU_TIED
      return finish_launch("selective_state_update");
    }
  }
#define SU_LAUNCH(TS, TX, VEC, LPR) do { \
    int rpb = (64 / LPR) * 4; int pblocks = (a.P + rpb - 1) / rpb; \
    dim3 grid((unsigned)((int64_t)a.B * a.H * pblocks)); \
    OMK_LAUNCH((state_update_kernel<TS, TX, VEC, LPR>), grid, block, 0, stream, a); } while (0)
#define SU_SHAPE(TS, TX) do { \
    if (vec && a.N >= 128) SU_LAUNCH(TS, TX, 4, 32); \
    else if (vec && a.N >= 64) SU_LAUNCH(TS, TX, 4, 16); \
    else if (vec) SU_LAUNCH(TS, TX, 4, 4); \
    else SU_LAUNCH(TS, TX, 1, 16); } while (0)
  OMK_DISPATCH_DTYPE(p->state.dtype, TS, OMK_DISPATCH_DTYPE(p->x.dtype, TX, SU_SHAPE(TS, TX)));
#undef SU_SHAPE
#undef SU_LAUNCH
  return finish_launch("selective_state_update");
}


extern "C" int omk_selective_state_extend(const OmkStateExtend* p, omk_stream stream) {
  OMK_REQUIRE(p && present(p->state) && present(p->x) && present(p->dt) && present(p->A) && present(p->Bm) && present(p->Cm) && present(p->out),
              "selective_state_extend: state, x, dt, A, B, C, out required");
  OMK_REQUIRE(p->state.ndim == 4 && p->x.ndim == 4 && p->dt.ndim == 4 && p->A.ndim == 3 && p->Bm.ndim == 4 && p->Cm.ndim == 4 && p->out.ndim == 4 &&
              (!present(p->z) || p->z.ndim == 4) && (!present(p->D) || p->D.ndim <= 2) && (!present(p->dt_bias) || p->dt_bias.ndim <= 2),
              "selective_state_extend: state (B,H,P,N), x/dt/z/out (B,T,H,P), A (H,P,N), B/C (B,T,G,N), D/dt_bias (H,P)");
  SeArgs a = {};
  const bool indexed = present(p->state_batch_indices);
  a.B = (int)(indexed ? p->x.shape[0] : p->state.shape[0]); a.pool = (int)p->state.shape[0];
  a.T = (int)p->x.shape[1];
  a.H = (int)p->state.shape[1]; a.P = (int)p->state.shape[2]; a.N = (int)p->state.shape[3]; a.G = (int)p->Bm.shape[2];
  OMK_REQUIRE(indices_ok(p->state_batch_indices, a.B), "selective_state_extend: state_batch_indices must be contiguous int32 (B)");
  a.sbi = (const int*)p->state_batch_indices.data;
  OMK_REQUIRE(indices_ok(p->seq_lens, a.B), "selective_state_extend: seq_lens must be contiguous int32 (B)");
  a.lens = (const int*)p->seq_lens.data;
  OMK_REQUIRE(a.G > 0 && a.H % a.G == 0, "selective_state_extend: H must be a multiple of ngroups");
  auto bthp = [&](const OmkTensor& t) {
    return t.shape[0] == a.B && t.shape[1] == a.T && t.shape[2] == a.H && t.shape[3] == a.P;
  };
  OMK_REQUIRE(bthp(p->x) && bthp(p->dt) && bthp(p->out) && (!present(p->z) || bthp(p->z)), "selective_state_extend: x, dt, z, out must be (B, T, H, P)");
  OMK_REQUIRE(p->A.shape[0] == a.H && p->A.shape[1] == a.P && p->A.shape[2] == a.N, "selective_state_extend: A must be (H, P, N)");
  OMK_REQUIRE(p->Bm.shape[0] == a.B && p->Bm.shape[1] == a.T && p->Bm.shape[3] == a.N && p->Cm.shape[0] == a.B && p->Cm.shape[1] == a.T &&
              p->Cm.shape[2] == a.G && p->Cm.shape[3] == a.N, "selective_state_extend: B/C must be (B, T, G, N)");
  OMK_REQUIRE(p->Bm.dtype == p->x.dtype && p->Cm.dtype == p->x.dtype && p->out.dtype == p->x.dtype, "selective_state_extend: B, C, out must have x's dtype");
  OMK_REQUIRE(!present(p->z) || p->z.dtype == p->x.dtype, "selective_state_extend: z dtype");
  OMK_REQUIRE(p->state.dtype <= OMK_F16 && p->x.dtype <= OMK_F16 && p->dt.dtype <= OMK_F16 && p->A.dtype <= OMK_F16 &&
              (!present(p->D) || p->D.dtype <= OMK_F16) && (!present(p->dt_bias) || p->dt_bias.dtype <= OMK_F16),
              "selective_state_extend: tensors must be fp32, bf16 or fp16");
  a.state = p->state.data; a.x = p->x.data; a.dt = p->dt.data; a.A = p->A.data; a.Bm = p->Bm.data; a.Cm = p->Cm.data;
  a.D = p->D.data; a.z = p->z.data; a.dtb = p->dt_bias.data; a.out = p->out.data;
  a.ssb = p->state.stride[0]; a.ssh = p->state.stride[1]; a.ssp = p->state.stride[2];
  a.xsb = p->x.stride[0]; a.xst = p->x.stride[1]; a.xsh = p->x.stride[2]; a.xsp = p->x.stride[3];
  a.dsb = p->dt.stride[0]; a.dst = p->dt.stride[1]; a.dsh = p->dt.stride[2]; a.dsp = p->dt.stride[3];
  a.ash = p->A.stride[0]; a.asp = p->A.stride[1]; a.asn = p->A.stride[2];
  a.bsb = p->Bm.stride[0]; a.bst = p->Bm.stride[1]; a.bsg = p->Bm.stride[2];
  a.csb = p->Cm.stride[0]; a.cst = p->Cm.stride[1]; a.csg = p->Cm.stride[2];
  if (present(p->D)) { a.Dsh = p->D.stride[0]; a.Dsp = p->D.ndim > 1 ? p->D.stride[1] : 0; }
  if (present(p->z)) { a.zsb = p->z.stride[0]; a.zst = p->z.stride[1]; a.zsh = p->z.stride[2]; a.zsp = p->z.stride[3]; }
  if (present(p->dt_bias)) { a.tsh = p->dt_bias.stride[0]; a.tsp = p->dt_bias.ndim > 1 ? p->dt_bias.stride[1] : 0; }
  a.osb = p->out.stride[0]; a.ost = p->out.stride[1]; a.osh = p->out.stride[2]; a.osp = p->out.stride[3];
  a.softplus = p->dt_softplus; a.xdt = p->x.dtype; a.dtdt = p->dt.dtype; a.adt = p->A.dtype; a.ddt = p->D.dtype; a.tbdt = p->dt_bias.dtype;
  if ((int64_t)a.B * a.T * a.H * a.P * a.N == 0) return OMK_OK;
  // one vector step per row: N = 4 LPR, LPR a power of two from 4 to 32; unit stride on n, 16-byte (fp32) / 8-byte (16-bit) aligned rows
  const int lpr = a.N / 4, sbytes = (int)dtype_size(p->state.dtype), xbytes = (int)dtype_size(p->x.dtype);
  const bool shape_ok = a.N % 4 == 0 && (lpr == 4 || lpr == 8 || lpr == 16 || lpr == 32);
  const bool vec_ok = p->state.stride[3] == 1 && p->Bm.stride[3] == 1 && p->Cm.stride[3] == 1 && ((uintptr_t)p->state.data % (4 * sbytes)) == 0 &&
                      ((uintptr_t)p->Bm.data % (4 * xbytes)) == 0 && ((uintptr_t)p->Cm.data % (4 * xbytes)) == 0 &&
                      a.ssb % 4 == 0 && a.ssh % 4 == 0 && a.ssp % 4 == 0 && a.bsb % 4 == 0 && a.bst % 4 == 0 && a.bsg % 4 == 0 &&
                      a.csb % 4 == 0 && a.cst % 4 == 0 && a.csg % 4 == 0;
  if (!shape_ok || !vec_ok)
    return fail(OMK_EUNSUPPORTED, "selective_state_extend: dstate must be 16, 32, 64 or 128 with unit-stride, 4-element aligned state / B / C rows "
                "(got N=%d); step such states one token at a time with omk_selective_state_update", a.N);
  const int rpb = (64 / lpr) * 4;
  dim3 grid((unsigned)((int64_t)a.B * a.H * ((a.P + rpb - 1) / rpb))), block(256);
#define SE_LAUNCH(TS, TX, RAGGED) do { \
    if (lpr == 32) OMK_LAUNCH((state_extend_kernel<TS, TX, 32, RAGGED>), grid, block, 0, stream, a); \
    else if (lpr == 16) OMK_LAUNCH((state_extend_kernel<TS, TX, 16, RAGGED>), grid, block, 0, stream, a); \
    else if (lpr == 8) OMK_LAUNCH((state_extend_kernel<TS, TX, 8, RAGGED>), grid, block, 0, stream, a); \
    else OMK_LAUNCH((state_extend_kernel<TS, TX, 4, RAGGED>), grid, block, 0, stream, a); } while (0)
  if (a.lens) OMK_DISPATCH_DTYPE(p->state.dtype, TS, OMK_DISPATCH_DTYPE(p->x.dtype, TX, SE_LAUNCH(TS, TX, true)));
  else OMK_DISPATCH_DTYPE(p->state.dtype, TS, OMK_DISPATCH_DTYPE(p->x.dtype, TX, SE_LAUNCH(TS, TX, false)));
#undef SE_LAUNCH
  return finish_launch("selective_state_extend");
}
