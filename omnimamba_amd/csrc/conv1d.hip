// conv1d.hip -- causal depthwise conv1d (width 2..4) + bias + SiLU: forward, backward, single-step update.
//
// HBM-bound (2 * tok * C * s bytes).  The Mamba-2 block stores xBC channel-last
// ((B, L, C) view of the in_proj output, row stride 8512), so the fast path gives each lane 8 adjacent channels
// (one 16-byte load per token, a wave covers 1 KB of one token row) and walks TL consecutive tokens with the
// W-1 previous inputs held in registers: every input byte is fetched once per tile (+ a W-1 token halo that
// hits L2).  Any other layout (channel-first, odd sizes, fp32 rows not 16-byte aligned) takes the strided
// scalar kernel, whose fastest thread index follows the unit-stride dimension.
#include <algorithm>
#include <initializer_list>
#include <type_traits>
#include "omk_common.h"
#include "ssd_tiles.h"

namespace omk {

constexpr int CONV_MAXW = 4;

struct ConvArgs {
  const void* x; const void* w; const void* bias; const void* init; const void* dout;
  void* out; void* fin; void* dx; float* dw; float* db; void* dinit;
  float* part;   // backward, optional: [B * tiles][C * (W + 1)] partial dw / db rows instead of atomics (conv1d_bwd_cl4_kernel)
  int FW;   // columns of final_states (>= W - 1)
  int64_t xsb, xsc, xsl, osb, osc, osl, isb, isc, isl, fsb, fsc, fsl, dosb, dosc, dosl, dxsb, dxsc, dxsl, disb, disc, disl;
  int64_t wsc, wsk;
  int B, C, L, W, silu, wdt, bdt, idt, fdt;
  const int* lens;   // optional (B): final_states[b] ends at position lens[b] instead of L (right-padded rows of a ragged prefill); read by
                     // conv1d_final_states_kernel only -- with it the channel-last kernels run without their epilogue (omk_causal_conv1d_fwd)
};

// where row b's final_states end: its own length (clamped to 0 .. L, so a bad value cannot address outside x), or L
__device__ __forceinline__ int conv_fin_end(const ConvArgs& a, int b) {
  if (!a.lens) return a.L;
  const int n = a.lens[b];
  return n < 0 ? 0 : (n > a.L ? a.L : n);
}

__device__ __forceinline__ float silu_grad(float pre) {
  float s = sigmoid_fast(pre);
  return s * (1.f + pre * (1.f - s));
}

// ---------------------------------------------------------------------------------------------------------
// channel-last vectorised forward: thread = (b, token tile, 8-channel vector)
// ---------------------------------------------------------------------------------------------------------
template <class T, int VEC, int TL, int W, int TG>
__global__ __launch_bounds__(256) void conv1d_fwd_cl_kernel(ConvArgs a) {
  const int CV = a.C / VEC, NT = (a.L + TL - 1) / TL;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (int64_t)a.B * NT * CV) return;
  const int cv = (int)(g % CV), tile = (int)((g / CV) % NT), b = (int)(g / ((int64_t)CV * NT));
  const int c0 = cv * VEC, l0 = tile * TL;
  const T* x = (const T*)a.x + (int64_t)b * a.xsb + c0;
  T* out = (T*)a.out + (int64_t)b * a.osb + c0;
  // win[k] holds the input at position l - (W-1) + k  (k = W-1 is the current token)
  float w[W][VEC], bias[VEC], win[W][VEC];
  // The prologue of a thread -- taps, bias, the W - 1 rows in front of its tile -- as ONE batch of requests, conversions behind the last
  // of them (raw_rt_flat / cvt_rt_flat, omk_common.h).  Written as `cond ? load_rt(...) : 0` (rounds 1 - 4) every one of these ~ 20 small
  // loads was a branch with s_waitcnt vmcnt(0) behind it: ~ 20 dependent round trips in front of a main loop of 8 (tools/isa_waits.py).
  {
    RawElem qb[VEC], qw[W][VEC], qi[W][VEC];
    vec_t<T, VEC> qx[W];
#pragma unroll
    for (int i = 0; i < VEC; i++) {
      qb[i] = raw_rt_flat(a.bias ? a.bias : a.w, a.bias ? c0 + i : 0, a.bias ? a.bdt : a.wdt);
#pragma unroll
      for (int k = 0; k < W; k++) qw[k][i] = raw_rt_flat(a.w, (int64_t)(c0 + i) * a.wsc + k * a.wsk, a.wdt);
    }
    // before the first shift slot s (1..W-1) holds position l0 - W + s: the row itself (clamped), or the initial state in front of the sequence
#pragma unroll
    for (int s = 1; s < W; s++) {
      const int l = l0 - W + s;
      qx[s] = *reinterpret_cast<const vec_t<T, VEC>*>(x + (int64_t)(l >= 0 ? l : 0) * a.xsl);
      const bool ini = a.init != nullptr && l < 0 && W - 1 + l >= 0;
#pragma unroll
      for (int i = 0; i < VEC; i++)
        qi[s][i] = raw_rt_flat(ini ? a.init : a.w, ini ? (int64_t)b * a.isb + (int64_t)(c0 + i) * a.isc + (int64_t)(W - 1 + l) * a.isl : 0, ini ? a.idt : a.wdt);
    }
#pragma unroll
    for (int i = 0; i < VEC; i++) {
      bias[i] = a.bias ? cvt_rt_flat(qb[i], a.bdt) : 0.f;
#pragma unroll
      for (int k = 0; k < W; k++) w[k][i] = cvt_rt_flat(qw[k][i], a.wdt);
    }
#pragma unroll
    for (int s = 1; s < W; s++) {
      const int l = l0 - W + s;
      const bool ini = a.init != nullptr && l < 0 && W - 1 + l >= 0;
#pragma unroll
      for (int i = 0; i < VEC; i++) win[s][i] = l >= 0 ? to_f32(qx[s].e[i]) : (ini ? cvt_rt_flat(qi[s][i], a.idt) : 0.f);
    }
  }
  const int lend = (l0 + TL < a.L) ? l0 + TL : a.L;
  // groups of TG tokens: all TG row loads are issued before the first one is consumed (a strictly sequential walk
  // exposes one HBM latency per token)
#pragma unroll 1
  for (int lg = l0; lg < lend; lg += TG) {
    vec_t<T, VEC> raw[TG];
#pragma unroll
    for (int j = 0; j < TG; j++) {
      const int l = lg + j < lend ? lg + j : lend - 1;   // clamped, so the loads stay unconditional
      raw[j] = *reinterpret_cast<const vec_t<T, VEC>*>(x + (int64_t)l * a.xsl);
    }
#pragma unroll
    for (int j = 0; j < TG; j++) {
      if (lg + j < lend) {
#pragma unroll
        for (int s = 0; s + 1 < W; s++)
#pragma unroll
          for (int i = 0; i < VEC; i++) win[s][i] = win[s + 1][i];
#pragma unroll
        for (int i = 0; i < VEC; i++) win[W - 1][i] = to_f32(raw[j].e[i]);
        float o[VEC];
#pragma unroll
        for (int i = 0; i < VEC; i++) {
          float acc = bias[i];
#pragma unroll
          for (int k = 0; k < W; k++) acc = fma_f32(w[k][i], win[k][i], acc);
          o[i] = a.silu ? silu_fast(acc) : acc;
        }
        store_vec<T, VEC>(out + (int64_t)(lg + j) * a.osl, o);
      }
    }
  }
  if (a.fin && lend == a.L) {
    // final_states[j] = xpad[L + (W - 1) - FW + j], xpad = [init | x]: the last FW >= W - 1 inputs (FW = W: the conv_state of Mamba2's cache)
    for (int j = 0; j < a.FW; j++) {
      const int l = a.L + j - a.FW;
#pragma unroll
      for (int i = 0; i < VEC; i++) {
        float v = 0.f;
        if (l >= 0) v = to_f32(x[(int64_t)l * a.xsl + i]);
        else if (a.init && W - 1 + l >= 0) v = load_rt(a.init, (int64_t)b * a.isb + (int64_t)(c0 + i) * a.isc + (int64_t)(W - 1 + l) * a.isl, a.idt);
        store_rt(a.fin, (int64_t)b * a.fsb + (int64_t)(c0 + i) * a.fsc + (int64_t)j * a.fsl, a.fdt, v);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// strided scalar forward: thread = one output element; fastest thread index along the unit-stride dim
// ---------------------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ float conv_in(const ConvArgs& a, const T* x, int b, int c, int l) {
  if (l >= 0) return to_f32(x[(int64_t)b * a.xsb + (int64_t)c * a.xsc + (int64_t)l * a.xsl]);
  if (a.init && a.W - 1 + l >= 0) return load_rt(a.init, (int64_t)b * a.isb + (int64_t)c * a.isc + (int64_t)(a.W - 1 + l) * a.isl, a.idt);
  return 0.f;
}

// ---------------------------------------------------------------------------------------------------------
// The forward walk with scalar token positions (round 5; see conv1d_bwd_cl4_kernel): four 16-bit channels (8 bytes) per lane, a wave =
// one strip of TL tokens x 64 channel quads, the strip index through readfirstlane -- row offsets are scalar, rows move through buffer
// resources (idle lanes of the last channel block point behind the range), the interior groups of a tile run a test-free token step.
// ---------------------------------------------------------------------------------------------------------
#ifndef TGF
#define TGF 8   // tokens requested per group
#endif
template <class T, int TL, int W, int TG, bool WF>
__global__ __launch_bounds__(256) void conv1d_fwd_cl8_kernel(ConvArgs a) {
  constexpr int VEC = 4;
  static_assert(sizeof(T) == 2, "four 16-bit channels = 8 bytes per lane");
  const int CV = a.C / VEC, NT4 = (a.L + 4 * TL - 1) / (4 * TL), CVB = (CV + 63) / 64;
  const int cvb = blockIdx.x % CVB, t4 = (blockIdx.x / CVB) % NT4, b = blockIdx.x / (CVB * NT4);
  const int cvl = threadIdx.x & 63, strip = uniform_i(threadIdx.x >> 6);
  const int cv = cvb * 64 + cvl;
  const bool cvok = cv < CV;
  const int c0 = (cvok ? cv : 0) * VEC, l0 = (t4 * 4 + strip) * TL;
  if (l0 >= a.L) return;                                           // (scalar: the whole wave)
  const T* x = (const T*)a.x + (int64_t)b * a.xsb + c0;
  float w[W][VEC], bias[VEC], win[W][VEC];
  if constexpr (WF) {
    // SHORT strips need a short prologue (WF: fp32 (C, W) weight rows, contiguous and 16-byte aligned, fp32 bias or none -- checked by the
    // launcher): the lane's VEC x W taps are VEC x W consecutive floats = W 16-byte requests, the bias one more, the W - 1 halo rows three
    // 8-byte requests behind ONE scalar test -- against 16 + 4 + 12 run-time-dtype element requests in the general prologue below, which
    // costs a 16-token strip more than its tokens (profiles/r06_stream_kernels.txt).
    f32x4 wq[W], bq = {0.f, 0.f, 0.f, 0.f};
    const f32x4* wp = reinterpret_cast<const f32x4*>((const float*)a.w + (int64_t)c0 * W);
#pragma unroll
    for (int q = 0; q < W; q++) wq[q] = wp[q];
    if (a.bias) bq = *reinterpret_cast<const f32x4*>((const float*)a.bias + c0);
    const bool interior = l0 >= W - 1;                                // (scalar)
    vec_t<T, VEC> qx[W];
    if (interior) {
#pragma unroll
      for (int s = 1; s < W; s++) qx[s] = *reinterpret_cast<const vec_t<T, VEC>*>(x + (int64_t)(l0 - W + s) * a.xsl);
    }
#pragma unroll
    for (int i = 0; i < VEC; i++) {
      bias[i] = bq[i];
      win[0][i] = 0.f;
#pragma unroll
      for (int k = 0; k < W; k++) w[k][i] = wq[(i * W + k) / 4][(i * W + k) % 4];
    }
    if (interior) {
#pragma unroll
      for (int s = 1; s < W; s++)
#pragma unroll
        for (int i = 0; i < VEC; i++) win[s][i] = to_f32(qx[s].e[i]);
    } else {   // the first strip of a sequence: initial states or zeros, earlier tokens of the strip's own sequence
#pragma unroll
      for (int s = 1; s < W; s++) {
        const int l = l0 - W + s;
#pragma unroll
        for (int i = 0; i < VEC; i++) {
          float v = 0.f;
          if (l >= 0) v = to_f32(x[(int64_t)l * a.xsl + i]);
          else if (a.init && W - 1 + l >= 0) v = load_rt(a.init, (int64_t)b * a.isb + (int64_t)(c0 + i) * a.isc + (int64_t)(W - 1 + l) * a.isl, a.idt);
          win[s][i] = v;
        }
      }
    }
  } else {
    RawElem qb[VEC], qw[W][VEC], qi[W][VEC];
    vec_t<T, VEC> qx[W];
#pragma unroll
    for (int i = 0; i < VEC; i++) {
      qb[i] = raw_rt_flat(a.bias ? a.bias : a.w, a.bias ? c0 + i : 0, a.bias ? a.bdt : a.wdt);
#pragma unroll
      for (int k = 0; k < W; k++) qw[k][i] = raw_rt_flat(a.w, (int64_t)(c0 + i) * a.wsc + k * a.wsk, a.wdt);
    }
#pragma unroll
    for (int s = 1; s < W; s++) {
      const int l = l0 - W + s;
      qx[s] = *reinterpret_cast<const vec_t<T, VEC>*>(x + (int64_t)(l >= 0 ? l : 0) * a.xsl);
      const bool ini = a.init != nullptr && l < 0 && W - 1 + l >= 0;
#pragma unroll
      for (int i = 0; i < VEC; i++)
        qi[s][i] = raw_rt_flat(ini ? a.init : a.w, ini ? (int64_t)b * a.isb + (int64_t)(c0 + i) * a.isc + (int64_t)(W - 1 + l) * a.isl : 0, ini ? a.idt : a.wdt);
    }
#pragma unroll
    for (int i = 0; i < VEC; i++) {
      bias[i] = a.bias ? cvt_rt_flat(qb[i], a.bdt) : 0.f;
#pragma unroll
      for (int k = 0; k < W; k++) w[k][i] = cvt_rt_flat(qw[k][i], a.wdt);
    }
#pragma unroll
    for (int i = 0; i < VEC; i++) win[0][i] = 0.f;
#pragma unroll
    for (int s = 1; s < W; s++) {
      const int l = l0 - W + s;
      const bool ini = a.init != nullptr && l < 0 && W - 1 + l >= 0;
#pragma unroll
      for (int i = 0; i < VEC; i++) win[s][i] = l >= 0 ? to_f32(qx[s].e[i]) : (ini ? cvt_rt_flat(qi[s][i], a.idt) : 0.f);
    }
  }
  const int lend = (l0 + TL < a.L) ? l0 + TL : a.L;
  const uint32_t vch = cvok ? 2u * (uint32_t)c0 : 0x7ffffff0u;
  const BufRes xr = make_buf((const T*)a.x + (int64_t)b * a.xsb, (uint32_t)(((int64_t)(a.L - 1) * a.xsl + a.C) * 2));
  const BufRes orr = make_buf((T*)a.out + (int64_t)b * a.osb, (uint32_t)(((int64_t)(a.L - 1) * a.osl + a.C) * 2));
  const uint32_t xrow = 2u * (uint32_t)a.xsl, orow = 2u * (uint32_t)a.osl;
  const bool silu_on = a.silu != 0;
  auto un4 = [](u32x2 r, float (&o)[VEC]) {
    if constexpr (std::is_same<T, bf16_t>::value) {
      o[0] = __builtin_bit_cast(float, r[0] << 16); o[1] = __builtin_bit_cast(float, r[0] & 0xffff0000u);
      o[2] = __builtin_bit_cast(float, r[1] << 16); o[3] = __builtin_bit_cast(float, r[1] & 0xffff0000u);
    } else {
      o[0] = to_f32(__builtin_bit_cast(T, (uint16_t)r[0])); o[1] = to_f32(__builtin_bit_cast(T, (uint16_t)(r[0] >> 16)));
      o[2] = to_f32(__builtin_bit_cast(T, (uint16_t)r[1])); o[3] = to_f32(__builtin_bit_cast(T, (uint16_t)(r[1] >> 16)));
    }
  };
  auto token = [&](auto fast_c, u32x2 rx_, int l) {   // l: scalar
    constexpr bool FAST = decltype(fast_c)::value;
    if (FAST || l < lend) {
#pragma unroll
      for (int s = 0; s + 1 < W; s++)
#pragma unroll
        for (int i = 0; i < VEC; i++) win[s][i] = win[s + 1][i];
      un4(rx_, win[W - 1]);
      T o4[VEC];
#pragma unroll
      for (int i = 0; i < VEC; i++) {
        float acc = bias[i];
#pragma unroll
        for (int k = 0; k < W; k++) acc = fma_f32(w[k][i], win[k][i], acc);
        o4[i] = from_f32<T>(silu_on ? silu_fast(acc) : acc);
      }
      u32x2 pk;
      pk[0] = (uint32_t)__builtin_bit_cast(uint16_t, o4[0]) | ((uint32_t)__builtin_bit_cast(uint16_t, o4[1]) << 16);
      pk[1] = (uint32_t)__builtin_bit_cast(uint16_t, o4[2]) | ((uint32_t)__builtin_bit_cast(uint16_t, o4[3]) << 16);
      buf_st8(orr, pk, vch, orow * (uint32_t)l);
    }
  };
#pragma unroll 1
  for (int lg = l0; lg < lend; lg += TG) {
    u32x2 raw[TG];
#pragma unroll
    for (int j = 0; j < TG; j++) {
      const int l = lg + j < lend ? lg + j : lend - 1;   // (scalar clamp)
      raw[j] = buf_ld8(xr, vch, xrow * (uint32_t)l);
    }
    if (lg + TG <= lend) {
#pragma unroll
      for (int j = 0; j < TG; j++) token(std::true_type{}, raw[j], lg + j);
    } else {
#pragma unroll
      for (int j = 0; j < TG; j++) token(std::false_type{}, raw[j], lg + j);
    }
  }
  if (a.fin && lend == a.L && cvok) {
    // final_states[j] = xpad[L + (W - 1) - FW + j], xpad = [init | x]: the last FW >= W - 1 inputs (FW = W: the conv_state of Mamba2's cache)
    for (int j = 0; j < a.FW; j++) {
      const int l = a.L + j - a.FW;
#pragma unroll
      for (int i = 0; i < VEC; i++) {
        float v = 0.f;
        if (l >= 0) v = to_f32(x[(int64_t)l * a.xsl + i]);
        else if (a.init && W - 1 + l >= 0) v = load_rt(a.init, (int64_t)b * a.isb + (int64_t)(c0 + i) * a.isc + (int64_t)(W - 1 + l) * a.isl, a.idt);
        store_rt(a.fin, (int64_t)b * a.fsb + (int64_t)(c0 + i) * a.fsc + (int64_t)j * a.fsl, a.fdt, v);
      }
    }
  }
}

template <class T>
__global__ void conv1d_fwd_generic_kernel(ConvArgs a, int l_fastest) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (int64_t)a.B * a.C * a.L) return;
  int b, c, l;
  if (l_fastest) { l = (int)(g % a.L); c = (int)((g / a.L) % a.C); b = (int)(g / ((int64_t)a.L * a.C)); }
  else { c = (int)(g % a.C); l = (int)((g / a.C) % a.L); b = (int)(g / ((int64_t)a.L * a.C)); }
  const T* x = (const T*)a.x;
  float acc = a.bias ? load_rt(a.bias, c, a.bdt) : 0.f;
  for (int k = 0; k < a.W; k++) acc = fma_f32(load_rt(a.w, (int64_t)c * a.wsc + k * a.wsk, a.wdt), conv_in<T>(a, x, b, c, l - (a.W - 1) + k), acc);
  if (a.silu) acc = silu_f(acc);
  ((T*)a.out)[(int64_t)b * a.osb + (int64_t)c * a.osc + (int64_t)l * a.osl] = from_f32<T>(acc);
}

template <class T>
__global__ void conv1d_final_states_kernel(ConvArgs a) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int Wm = a.FW;
  if (g >= (int64_t)a.B * a.C * Wm) return;
  const int c = (int)(g % a.C), j = (int)((g / a.C) % Wm), b = (int)(g / ((int64_t)a.C * Wm));
  float v = conv_in<T>(a, (const T*)a.x, b, c, conv_fin_end(a, b) + j - Wm);
  store_rt(a.fin, (int64_t)b * a.fsb + (int64_t)c * a.fsc + (int64_t)j * a.fsl, a.fdt, v);
}

// ---------------------------------------------------------------------------------------------------------
// backward.  pre[l] = bias + sum_k w[k] xpad[l+k] ; dpre = dout * silu'(pre)
//   dx[l] = sum_k w[k] dpre[l + (W-1) - k]   (terms with index >= L vanish)
//   dw[k] = sum_{b,l} dpre[l] xpad[l+k] ; db = sum dpre ; dinit[j] = sum_k w[k] dpre[j - k] (j-k >= 0, < L)
// channel-last vectorised: thread = (b, tile of TL tokens, 8 channels); dw/db reduced with one atomic per thread.
// ---------------------------------------------------------------------------------------------------------
// block = 64 channel vectors (one wave row of 1 KB per token) x 4 token strips of TL tokens; the four strips fold
// their dw / db partials through LDS so each (channel, tap) costs one global atomic per block.
template <class T, int VEC, int TL, int W, int TG>
__global__ __launch_bounds__(256) void conv1d_bwd_cl_kernel(ConvArgs a) {
  __shared__ float sred[4][64][VEC * (W + 1)];
  const int CV = a.C / VEC, NT4 = (a.L + 4 * TL - 1) / (4 * TL), CVB = (CV + 63) / 64;
  const int cvb = blockIdx.x % CVB, t4 = (blockIdx.x / CVB) % NT4, b = blockIdx.x / (CVB * NT4);
  const int cvl = threadIdx.x & 63, strip = threadIdx.x >> 6;
  const int cv = cvb * 64 + cvl;
  const bool cvok = cv < CV;
  const int c0 = (cvok ? cv : 0) * VEC, l0 = (t4 * 4 + strip) * TL;
  const T* x = (const T*)a.x;
  const T* dout = (const T*)a.dout + (int64_t)b * a.dosb + c0;
  T* dx = (T*)a.dx + (int64_t)b * a.dxsb + c0;
  float w[W][VEC], bias[VEC], dwacc[W][VEC], dbacc[VEC];
  // (taps, bias and the rows in front of the tile: one batch of requests, conversions behind -- see conv1d_fwd_cl_kernel)
  RawElem qb[VEC], qw[W][VEC];
#pragma unroll
  for (int i = 0; i < VEC; i++) {
    qb[i] = raw_rt_flat(a.bias ? a.bias : a.w, a.bias ? c0 + i : 0, a.bias ? a.bdt : a.wdt);
    dbacc[i] = 0.f;
#pragma unroll
    for (int k = 0; k < W; k++) {
      qw[k][i] = raw_rt_flat(a.w, (int64_t)(c0 + i) * a.wsc + k * a.wsk, a.wdt);
      dwacc[k][i] = 0.f;
    }
  }
  const int lend = !cvok ? l0 : ((l0 + TL < a.L) ? l0 + TL : a.L);   // idle lanes (cv out of range) do zero tokens
  // walking p = l0 .. lend+W-2: xw[k] = xpad at position p-(W-1)+k, dp[k] = dpre[p-(W-1)+k];
  // at step p dpre[p] becomes known and dx[p-(W-1)] = sum_k w[k] dpre[p-k] = sum_k w[k] dp[W-1-k] is complete.
  float xw[W][VEC], dp[W][VEC];
#pragma unroll
  for (int s = 0; s < W; s++)
#pragma unroll
    for (int i = 0; i < VEC; i++) { xw[s][i] = 0.f; dp[s][i] = 0.f; }
  {
    T qx[W][VEC];
    RawElem qi[W][VEC];
#pragma unroll
    for (int s = 1; s < W; s++) {
      const int l = l0 - W + s;
      const bool ini = a.init != nullptr && l < 0 && a.W - 1 + l >= 0;
#pragma unroll
      for (int i = 0; i < VEC; i++) {
        qx[s][i] = x[(int64_t)b * a.xsb + (int64_t)(c0 + i) * a.xsc + (int64_t)(l >= 0 ? l : 0) * a.xsl];
        qi[s][i] = raw_rt_flat(ini ? a.init : a.w, ini ? (int64_t)b * a.isb + (int64_t)(c0 + i) * a.isc + (int64_t)(a.W - 1 + l) * a.isl : 0, ini ? a.idt : a.wdt);
      }
    }
#pragma unroll
    for (int i = 0; i < VEC; i++) {
      bias[i] = a.bias ? cvt_rt_flat(qb[i], a.bdt) : 0.f;
#pragma unroll
      for (int k = 0; k < W; k++) w[k][i] = cvt_rt_flat(qw[k][i], a.wdt);
    }
#pragma unroll
    for (int s = 1; s < W; s++) {
      const int l = l0 - W + s;
      const bool ini = a.init != nullptr && l < 0 && a.W - 1 + l >= 0;
#pragma unroll
      for (int i = 0; i < VEC; i++) xw[s][i] = l >= 0 ? to_f32(qx[s][i]) : (ini ? cvt_rt_flat(qi[s][i], a.idt) : 0.f);
    }
  }
  // dpre of the W-1 positions before l0 is NOT needed: dx[lo] only uses dpre[lo .. lo+W-1], lo >= l0.
  const int pend = lend + W - 1;
  const T* xb = x + (int64_t)b * a.xsb + c0;
#pragma unroll 1
  for (int pg = l0; pg < pend; pg += TG) {
    vec_t<T, VEC> rawx[TG], rawg[TG];
#pragma unroll
    for (int j = 0; j < TG; j++) {
      const int pc = pg + j < a.L ? pg + j : a.L - 1;   // clamped: unconditional loads, masked below
      rawx[j] = *reinterpret_cast<const vec_t<T, VEC>*>(xb + (int64_t)pc * a.xsl);
      rawg[j] = *reinterpret_cast<const vec_t<T, VEC>*>(dout + (int64_t)pc * a.dosl);
    }
#pragma unroll
    for (int j = 0; j < TG; j++) {
      const int p = pg + j;
      if (p < pend) {
#pragma unroll
        for (int s = 0; s + 1 < W; s++)
#pragma unroll
          for (int i = 0; i < VEC; i++) { xw[s][i] = xw[s + 1][i]; dp[s][i] = dp[s + 1][i]; }
        const bool inside = p < a.L;
        float go[VEC];
#pragma unroll
        for (int i = 0; i < VEC; i++) {
          xw[W - 1][i] = inside ? to_f32(rawx[j].e[i]) : 0.f;
          go[i] = inside ? to_f32(rawg[j].e[i]) : 0.f;
        }
#pragma unroll
        for (int i = 0; i < VEC; i++) {
          float d = go[i];
          if (a.silu && inside) {
            float pre = bias[i];
#pragma unroll
            for (int k = 0; k < W; k++) pre += w[k][i] * xw[k][i];
            d *= silu_grad(pre);
          }
          dp[W - 1][i] = inside ? d : 0.f;
          if (inside && p < lend) {   // dw/db: each position is counted by exactly one tile
            dbacc[i] += d;
#pragma unroll
            for (int k = 0; k < W; k++) dwacc[k][i] += d * xw[k][i];
          }
        }
        const int lo = p - (W - 1);
        if (lo >= l0 && lo < lend) {
          float o[VEC];
#pragma unroll
          for (int i = 0; i < VEC; i++) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < W; k++) acc += w[k][i] * dp[W - 1 - k][i];
            o[i] = acc;
          }
          store_vec<T, VEC>(dx + (int64_t)lo * a.dxsl, o);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < VEC; i++) {
    sred[strip][cvl][i * (W + 1) + W] = dbacc[i];
#pragma unroll
    for (int k = 0; k < W; k++) sred[strip][cvl][i * (W + 1) + k] = dwacc[k][i];
  }
  block_sync();
  if (strip == 0 && cvok) {
#pragma unroll
    for (int i = 0; i < VEC; i++) {
#pragma unroll
      for (int k = 0; k <= W; k++) {
        const int j = i * (W + 1) + k;
        const float v = sred[0][cvl][j] + sred[1][cvl][j] + sred[2][cvl][j] + sred[3][cvl][j];
        if (k < W) atomic_add_f32(a.dw + (int64_t)(c0 + i) * W + k, v);
        else if (a.db) atomic_add_f32(a.db + c0 + i, v);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// The same walk for two 16-bit channels per lane (the shipped configuration), round 5.  conv1d_bwd_cl_kernel is VALU bound: ~ 125
// instructions per token and lane, of which ~ 60 are v_cndmask / v_mov for the tile- and sequence-edge masks and ~ 14 are 64-bit address
// arithmetic per request.  Here
//   * the token position of a wave is a SCALAR (strip = readfirstlane): row offsets are s_mul / s_add, every edge test a scalar branch;
//   * rows move through buffer resources: the lane part of an address is one constant VGPR (idle lanes of the last channel block point
//     behind the range: their loads read zeros and their stores are dropped), the row part the instruction's scalar offset;
//   * the token step exists twice: the seven interior groups of a 64-token tile take a copy without any test -- the window shifts are
//     register renames there;
//   * (round 6) the lane's two channels are one packed fp32 pair (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32) and contiguous fp32 weights take a
//     prologue of 16-byte requests (WF): 207 -> 185 us at the cfg 2 slice (profiles/r06_stream_kernels.txt).
// ---------------------------------------------------------------------------------------------------------
#ifndef TGX
#define TGX 4   // tokens requested per group (round 6, packed pairs: 4 / 8 / 16 = 76 / 94 / 142 registers, 193.8 / 189.6 / 194.2 us -- no difference)
#endif
template <class T, int TL, int W, int TG, int NS, bool WF>   // NS strips of TL tokens per workgroup (one wave each): NS TL tokens per set of dw / db atomics
__global__ __launch_bounds__(64 * NS) void conv1d_bwd_cl4_kernel(ConvArgs a) {   // (74 - 76 registers with the packed pairs of round 6; 102 before)
  constexpr int VEC = 2;
  static_assert(sizeof(T) == 2, "two 16-bit channels = one dword per lane");
  __shared__ float sred[NS][64][VEC * (W + 1)];
  const int CV = a.C / VEC, NT4 = (a.L + NS * TL - 1) / (NS * TL), CVB = (CV + 63) / 64;
  const int cvb = blockIdx.x % CVB, t4 = (blockIdx.x / CVB) % NT4, b = blockIdx.x / (CVB * NT4);
  const int cvl = threadIdx.x & 63, strip = uniform_i(threadIdx.x >> 6);
  const int cv = cvb * 64 + cvl;
  const bool cvok = cv < CV;
  const int c0 = (cvok ? cv : 0) * VEC, l0 = (t4 * NS + strip) * TL;
  const T* x = (const T*)a.x;
  // the lane's two channels are ONE packed fp32 pair everywhere below: taps, window, sums -- v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 do
  // both channels per instruction (the scalar form is VALU bound: ~ 45 vector + 4 transcendental instructions per token, ~ 25 + 4 packed)
  f32x2 w[W], bias, dwacc[W], dbacc;
  const int lend = (l0 + TL < a.L) ? l0 + TL : a.L;   // (scalar; idle lanes walk along on zeros)
  f32x2 xw[W], dp[W];
#pragma unroll
  for (int s = 0; s < W; s++) { xw[s] = f32x2{0.f, 0.f}; dp[s] = f32x2{0.f, 0.f}; dwacc[s] = f32x2{0.f, 0.f}; }
  dbacc = f32x2{0.f, 0.f};
  if constexpr (WF) {
    // the short prologue of the forward kernel (fp32 (C, W) weight rows, contiguous and 16-byte aligned; fp32 bias or none): the lane's 2 W taps are
    // 2 W consecutive floats, the halo rows three dword requests behind one scalar test
    const float* wp = (const float*)a.w + (int64_t)c0 * W;
    float wf[VEC * W];
    if constexpr ((VEC * W) % 4 == 0) {
#pragma unroll
      for (int q = 0; q < VEC * W / 4; q++) {
        const f32x4 v = reinterpret_cast<const f32x4*>(wp)[q];
#pragma unroll
        for (int e = 0; e < 4; e++) wf[4 * q + e] = v[e];
      }
    } else {
#pragma unroll
      for (int q = 0; q < VEC * W / 2; q++) {
        const f32x2 v = reinterpret_cast<const f32x2*>(wp)[q];
        wf[2 * q] = v[0]; wf[2 * q + 1] = v[1];
      }
    }
    bias = a.bias ? *reinterpret_cast<const f32x2*>((const float*)a.bias + c0) : f32x2{0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < W; kk++) w[kk] = f32x2{wf[kk], wf[W + kk]};
    if (l0 >= W - 1 && l0 < a.L) {                                      // (scalar)
      uint32_t qx[W];
#pragma unroll
      for (int s = 1; s < W; s++) qx[s] = *reinterpret_cast<const uint32_t*>(x + (int64_t)b * a.xsb + c0 + (int64_t)(l0 - W + s) * a.xsl);
#pragma unroll
      for (int s = 1; s < W; s++) {
        if constexpr (std::is_same<T, bf16_t>::value) xw[s] = f32x2{__builtin_bit_cast(float, qx[s] << 16), __builtin_bit_cast(float, qx[s] & 0xffff0000u)};
        else xw[s] = f32x2{to_f32(__builtin_bit_cast(T, (uint16_t)qx[s])), to_f32(__builtin_bit_cast(T, (uint16_t)(qx[s] >> 16)))};
      }
    } else {
#pragma unroll
      for (int s = 1; s < W; s++) {
        const int l = l0 - W + s;
#pragma unroll
        for (int i = 0; i < VEC; i++) {
          float v = 0.f;
          if (l >= 0) v = to_f32(x[(int64_t)b * a.xsb + (int64_t)(c0 + i) * a.xsc + (int64_t)(l < a.L ? l : a.L - 1) * a.xsl]);
          else if (a.init && a.W - 1 + l >= 0) v = load_rt(a.init, (int64_t)b * a.isb + (int64_t)(c0 + i) * a.isc + (int64_t)(a.W - 1 + l) * a.isl, a.idt);
          xw[s][i] = v;
        }
      }
    }
  } else {
  RawElem qb[VEC], qw[W][VEC];
#pragma unroll
  for (int i = 0; i < VEC; i++) {
    qb[i] = raw_rt_flat(a.bias ? a.bias : a.w, a.bias ? c0 + i : 0, a.bias ? a.bdt : a.wdt);
#pragma unroll
    for (int k = 0; k < W; k++) qw[k][i] = raw_rt_flat(a.w, (int64_t)(c0 + i) * a.wsc + k * a.wsk, a.wdt);
  }
  {
    T qx[W][VEC];
    RawElem qi[W][VEC];
#pragma unroll
    for (int s = 1; s < W; s++) {
      const int l = l0 - W + s;
      const bool ini = a.init != nullptr && l < 0 && a.W - 1 + l >= 0;
#pragma unroll
      for (int i = 0; i < VEC; i++) {
        qx[s][i] = x[(int64_t)b * a.xsb + (int64_t)(c0 + i) * a.xsc + (int64_t)(l >= 0 ? (l < a.L ? l : a.L - 1) : 0) * a.xsl];
        qi[s][i] = raw_rt_flat(ini ? a.init : a.w, ini ? (int64_t)b * a.isb + (int64_t)(c0 + i) * a.isc + (int64_t)(a.W - 1 + l) * a.isl : 0, ini ? a.idt : a.wdt);
      }
    }
#pragma unroll
    for (int i = 0; i < VEC; i++) {
      bias[i] = a.bias ? cvt_rt_flat(qb[i], a.bdt) : 0.f;
#pragma unroll
      for (int k = 0; k < W; k++) w[k][i] = cvt_rt_flat(qw[k][i], a.wdt);
    }
#pragma unroll
    for (int s = 1; s < W; s++) {
      const int l = l0 - W + s;
      const bool ini = a.init != nullptr && l < 0 && a.W - 1 + l >= 0;
#pragma unroll
      for (int i = 0; i < VEC; i++) xw[s][i] = l >= 0 ? to_f32(qx[s][i]) : (ini ? cvt_rt_flat(qi[s][i], a.idt) : 0.f);
    }
  }
  }
  const int pend = lend + W - 1;
  // rows of this batch element as buffers; lane part of every address: the channel pair (idle lanes: behind the range)
  const uint32_t vch = cvok ? 2u * (uint32_t)c0 : 0x7ffffff0u;
  const BufRes xr = make_buf(x + (int64_t)b * a.xsb, (uint32_t)(((int64_t)(a.L - 1) * a.xsl + a.C) * 2));
  const BufRes gr = make_buf((const T*)a.dout + (int64_t)b * a.dosb, (uint32_t)(((int64_t)(a.L - 1) * a.dosl + a.C) * 2));
  const BufRes dr = make_buf((T*)a.dx + (int64_t)b * a.dxsb, (uint32_t)(((int64_t)(a.L - 1) * a.dxsl + a.C) * 2));
  const uint32_t xrow = 2u * (uint32_t)a.xsl, grow = 2u * (uint32_t)a.dosl, drow = 2u * (uint32_t)a.dxsl;
  const bool silu_on = a.silu != 0;
  auto un2 = [](uint32_t r) -> f32x2 {
    f32x2 o;
    if constexpr (std::is_same<T, bf16_t>::value) { o[0] = __builtin_bit_cast(float, r << 16); o[1] = __builtin_bit_cast(float, r & 0xffff0000u); }
    else { o[0] = to_f32(__builtin_bit_cast(T, (uint16_t)r)); o[1] = to_f32(__builtin_bit_cast(T, (uint16_t)(r >> 16))); }
    return o;
  };
  auto silu_grad2 = [](f32x2 pre) -> f32x2 {   // silu_grad of both channels: the two exp2 / rcp are the only unpacked steps
    const f32x2 t = pre * (-LOG2E);
    const f32x2 e = {exp2_fast(t[0]), exp2_fast(t[1])};
    const f32x2 q = e + 1.f;
    const f32x2 sg = {rcp_fast(q[0]), rcp_fast(q[1])};
    return sg * (1.f + pre * (1.f - sg));
  };
  auto token = [&](auto fast_c, uint32_t rx_, uint32_t rg_, int p) {   // p: scalar
    constexpr bool FAST = decltype(fast_c)::value;
    if (FAST || p < pend) {
#pragma unroll
      for (int s = 0; s + 1 < W; s++) { xw[s] = xw[s + 1]; dp[s] = dp[s + 1]; }
      const bool inside = FAST ? true : p < a.L;
      f32x2 d = un2(rg_), xn = un2(rx_);
      if (!inside) { d = f32x2{0.f, 0.f}; xn = f32x2{0.f, 0.f}; }
      xw[W - 1] = xn;
      if (silu_on) {
        f32x2 pre = bias;
#pragma unroll
        for (int k = 0; k < W; k++) pre = fma_f32x2(w[k], xw[k], pre);
        d *= silu_grad2(pre);
      }
      dp[W - 1] = d;
      if (FAST || p < lend) {   // dw/db: each position is counted by exactly one tile (behind the sequence d is zero)
        dbacc += d;
#pragma unroll
        for (int k = 0; k < W; k++) dwacc[k] = fma_f32x2(d, xw[k], dwacc[k]);
      }
      const int lo = p - (W - 1);
      if (FAST || (lo >= l0 && lo < lend)) {
        f32x2 acc = w[0] * dp[W - 1];
#pragma unroll
        for (int k = 1; k < W; k++) acc = fma_f32x2(w[k], dp[W - 1 - k], acc);
        T o2[VEC] = {from_f32<T>(acc[0]), from_f32<T>(acc[1])};
        const uint32_t pk = (uint32_t)__builtin_bit_cast(uint16_t, o2[0]) | ((uint32_t)__builtin_bit_cast(uint16_t, o2[1]) << 16);
        buf_st_f32(dr, __builtin_bit_cast(float, pk), vch, drow * (uint32_t)lo);
      }
    }
  };
#pragma unroll 1
  for (int pg = l0; pg < pend; pg += TG) {
    uint32_t rawx[TG], rawg[TG];
#pragma unroll
    for (int j = 0; j < TG; j++) {
      const int pc = pg + j < a.L ? pg + j : a.L - 1;   // (scalar clamp; masked in the edge copy of the step)
      rawx[j] = __builtin_bit_cast(uint32_t, buf_ld_f32(xr, vch, xrow * (uint32_t)pc));
      rawg[j] = __builtin_bit_cast(uint32_t, buf_ld_f32(gr, vch, grow * (uint32_t)pc));
    }
    if (pg >= l0 + W - 1 && pg + TG <= lend) {   // interior group (lend <= L)
#pragma unroll
      for (int j = 0; j < TG; j++) { token(std::true_type{}, rawx[j], rawg[j], pg + j); OMK_SCHED_FENCE(); }   // (fence: eight steps scheduled as one block keep 146 registers live)
    } else {
#pragma unroll
      for (int j = 0; j < TG; j++) token(std::false_type{}, rawx[j], rawg[j], pg + j);
    }
  }
#pragma unroll
  for (int i = 0; i < VEC; i++) {
    sred[strip][cvl][i * (W + 1) + W] = dbacc[i];
#pragma unroll
    for (int k = 0; k < W; k++) sred[strip][cvl][i * (W + 1) + k] = dwacc[k][i];
  }
  block_sync();
  if (a.part) {
    // one partial row per (batch, tile of NS strips): the lane's VEC (W + 1) sums are consecutive floats, spread over the NS waves; a second launch
    // (conv1d_bwd_fold_kernel) adds the rows in a fixed order -- no atomics, the same gradients on every run
    if (cvok) {
      float* prow = a.part + ((int64_t)b * NT4 + t4) * ((int64_t)a.C * (W + 1)) + (int64_t)c0 * (W + 1);
      for (int j = strip; j < VEC * (W + 1); j += NS) {
        float v = sred[0][cvl][j];
#pragma unroll
        for (int q = 1; q < NS; q++) v += sred[q][cvl][j];
        prow[j] = v;
      }
    }
    return;
  }
  if (strip == 0 && cvok) {
#pragma unroll
    for (int i = 0; i < VEC; i++) {
#pragma unroll
      for (int k = 0; k <= W; k++) {
        const int j = i * (W + 1) + k;
        float v = sred[0][cvl][j];
#pragma unroll
        for (int q = 1; q < NS; q++) v += sred[q][cvl][j];
        if (k < W) atomic_add_f32(a.dw + (int64_t)(c0 + i) * W + k, v);
        else if (a.db) atomic_add_f32(a.db + c0 + i, v);
      }
    }
  }
}

// dw[c][k] += sum_p part[p][c (W + 1) + k], db[c] += sum_p part[p][c (W + 1) + W]: 64 columns x 16 row groups per workgroup, four requests in flight per
// lane, rows added in a fixed order (group sums in index order)
__global__ __launch_bounds__(1024) void conv1d_bwd_fold_kernel(const float* part, int P, int C, int W, float* dw, float* db) {
  __shared__ float sh[16][64];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t ncol = (int64_t)C * (W + 1), col = (int64_t)blockIdx.x * 64 + cl;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (col < ncol) {
    for (int p0 = g; p0 < P; p0 += 64) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) { const int p = p0 + 16 * u; v[u] = p < P ? part[(int64_t)p * ncol + col] : 0.f; }
#pragma unroll
      for (int u = 0; u < 4; u++) s[u] += v[u];
    }
  }
  sh[g][cl] = (s[0] + s[1]) + (s[2] + s[3]);
  block_sync();
  if (g == 0 && col < ncol) {
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < 16; q++) v += sh[q][cl];
    const int c = (int)(col / (W + 1)), k = (int)(col % (W + 1));
    if (k < W) dw[(int64_t)c * W + k] += v;
    else if (db) db[c] += v;
  }
}

// strided scalar backward: thread = (b, c), sequential over L (fallback for channel-first / odd layouts)
template <class T>
__global__ void conv1d_bwd_generic_kernel(ConvArgs a) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (int64_t)a.B * a.C) return;
  const int c = (int)(g % a.C), b = (int)(g / a.C), W = a.W;
  const T* x = (const T*)a.x;
  const T* dout = (const T*)a.dout;
  float w[CONV_MAXW], dwacc[CONV_MAXW] = {0.f, 0.f, 0.f, 0.f}, dbacc = 0.f;
  for (int k = 0; k < CONV_MAXW; k++) w[k] = k < W ? load_rt(a.w, (int64_t)c * a.wsc + k * a.wsk, a.wdt) : 0.f;
  const float bias = a.bias ? load_rt(a.bias, c, a.bdt) : 0.f;
  auto dpre = [&](int l) -> float {
    if (l < 0 || l >= a.L) return 0.f;
    float d = to_f32(dout[(int64_t)b * a.dosb + (int64_t)c * a.dosc + (int64_t)l * a.dosl]);
    if (a.silu) {
      float pre = bias;
      for (int k = 0; k < W; k++) pre += w[k] * conv_in<T>(a, x, b, c, l - (W - 1) + k);
      d *= silu_grad(pre);
    }
    return d;
  };
  for (int l = 0; l < a.L; l++) {
    float acc = 0.f;
    for (int k = 0; k < W; k++) acc += w[k] * dpre(l + (W - 1) - k);
    ((T*)a.dx)[(int64_t)b * a.dxsb + (int64_t)c * a.dxsc + (int64_t)l * a.dxsl] = from_f32<T>(acc);
    float d = dpre(l);
    dbacc += d;
    for (int k = 0; k < W; k++) dwacc[k] += d * conv_in<T>(a, x, b, c, l - (W - 1) + k);
  }
  if (a.db) atomic_add_f32(a.db + c, dbacc);
  for (int k = 0; k < W; k++) atomic_add_f32(a.dw + (int64_t)c * W + k, dwacc[k]);
}

// dinitial_states[b, c, j] = sum_k w[k] dpre[j - k] over 0 <= j-k < L  (tiny: B*C*(W-1) threads)
template <class T>
__global__ void conv1d_dinit_kernel(ConvArgs a) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int Wm = a.W - 1, W = a.W;
  if (g >= (int64_t)a.B * a.C * Wm) return;
  const int c = (int)(g % a.C), j = (int)((g / a.C) % Wm), b = (int)(g / ((int64_t)a.C * Wm));
  const T* x = (const T*)a.x;
  const T* dout = (const T*)a.dout;
  const float bias = a.bias ? load_rt(a.bias, c, a.bdt) : 0.f;
  float acc = 0.f;
  for (int k = 0; k < W; k++) {
    int l = j - k;   // xpad index j feeds pre[l] through weight k when l + k == j
    if (l < 0 || l >= a.L) continue;
    float d = to_f32(dout[(int64_t)b * a.dosb + (int64_t)c * a.dosc + (int64_t)l * a.dosl]);
    if (a.silu) {
      float pre = bias;
      for (int kk = 0; kk < W; kk++) pre += load_rt(a.w, (int64_t)c * a.wsc + kk * a.wsk, a.wdt) * conv_in<T>(a, x, b, c, l - (W - 1) + kk);
      d *= silu_grad(pre);
    }
    acc += load_rt(a.w, (int64_t)c * a.wsc + k * a.wsk, a.wdt) * d;
  }
  store_rt(a.dinit, (int64_t)b * a.disb + (int64_t)c * a.disc + (int64_t)j * a.disl, a.idt, acc);
}

// ---------------------------------------------------------------------------------------------------------
// decode update: thread = (b, c); state (B, C, S) shifted left by T, new inputs appended
// ---------------------------------------------------------------------------------------------------------
struct ConvUpdArgs {
  const void* x; void* state; const void* w; const void* bias; void* out;
  const int* csi;                        // ABI 8: slot of row b in the state pool (null: row b)
  const int* lens;                       // ABI 13: tokens row b applies (null: T), clamped to 0 .. T on the device
  int64_t xsb, xsc, xsl, ssb, ssc, ssl, osb, osc, osl, wsc, wsk;
  int B, C, T, S, W, silu, xdt, sdt, wdt, bdt, pool;
};
// RAGGED (ABI 13, seq_lens present): the row shifts and appends by its own length nT, outputs behind it are zeros.  An instantiation of
// its own: as a run-time branch the length cost every caller five VGPRs.
template <bool RAGGED>
__global__ void conv1d_update_kernel(ConvUpdArgs a) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (int64_t)a.B * a.C) return;
  const int c = (int)(g % a.C), b = (int)(g / a.C);
  int sb = b, nT = a.T;
  if (a.csi) sb = a.csi[b];              // slot of this row; negative or outside the pool: a padding row
  if constexpr (RAGGED) {
    const int n = a.lens[b];
    nT = n < 0 ? 0 : (n < a.T ? n : a.T);
  }
  if (sb < 0 || sb >= a.pool || (RAGGED && nT == 0)) {   // padding row or a row of length 0: no state traffic, zeros out
    for (int t = 0; t < a.T; t++) store_rt(a.out, (int64_t)b * a.osb + (int64_t)c * a.osc + (int64_t)t * a.osl, a.xdt, 0.f);
    return;
  }
  float w[CONV_MAXW], win[CONV_MAXW];
  for (int k = 0; k < CONV_MAXW; k++) w[k] = k < a.W ? load_rt(a.w, (int64_t)c * a.wsc + k * a.wsk, a.wdt) : 0.f;
  const float bias = a.bias ? load_rt(a.bias, c, a.bdt) : 0.f;
  const int64_t sbase = (int64_t)sb * a.ssb + (int64_t)c * a.ssc;
  // window = last W-1 state entries
  for (int k = 0; k < CONV_MAXW; k++) win[k] = 0.f;
  for (int k = 0; k + 1 < a.W; k++) win[k] = load_rt(a.state, sbase + (int64_t)(a.S - (a.W - 1) + k) * a.ssl, a.sdt);
  // shift the stored state left by the row's nT tokens (S is tiny: W-1 or W)
  if (nT < a.S) {
    for (int s = 0; s + nT < a.S; s++) store_rt(a.state, sbase + (int64_t)s * a.ssl, a.sdt, load_rt(a.state, sbase + (int64_t)(s + nT) * a.ssl, a.sdt));
  }
  for (int t = 0; t < nT; t++) {
    float xv = load_rt(a.x, (int64_t)b * a.xsb + (int64_t)c * a.xsc + (int64_t)t * a.xsl, a.xdt);
    win[a.W - 1] = xv;
    float acc = bias;
    for (int k = 0; k < a.W; k++) acc = fma_f32(w[k], win[k], acc);
    if (a.silu) acc = silu_f(acc);
    store_rt(a.out, (int64_t)b * a.osb + (int64_t)c * a.osc + (int64_t)t * a.osl, a.xdt, acc);
    for (int k = 0; k + 1 < a.W; k++) win[k] = win[k + 1];
    int spos = a.S - nT + t;
    if (spos >= 0) store_rt(a.state, sbase + (int64_t)spos * a.ssl, a.sdt, xv);
  }
  if constexpr (RAGGED) {                // behind the row's length: zeros
    for (int t = nT; t < a.T; t++) store_rt(a.out, (int64_t)b * a.osb + (int64_t)c * a.osc + (int64_t)t * a.osl, a.xdt, 0.f);
  }
}

static bool cl_fast_ok(const OmkTensor& t, int C) {   // (B, C, L) logical, channel contiguous, 16-byte rows (8 x 2-byte)
  return t.stride[1] == 1 && (t.stride[0] % 8) == 0 && (t.stride[2] % 8) == 0 && aligned16(t) && (C % 8) == 0;
}

static int fill_common(ConvArgs& a, const OmkTensor& x, const OmkTensor& w, const OmkTensor& bias, const OmkTensor& init, const char* who) {
  OMK_REQUIRE(x.ndim == 3 && w.ndim == 2, "%s: x must be (B, C, L), weight (C, W)", who);
  a.B = (int)x.shape[0]; a.C = (int)x.shape[1]; a.L = (int)x.shape[2]; a.W = (int)w.shape[1];
  OMK_REQUIRE(w.shape[0] == a.C && a.W >= 2 && a.W <= CONV_MAXW, "%s: weight must be (C, W) with W in 2..4", who);
  a.x = x.data; a.xsb = x.stride[0]; a.xsc = x.stride[1]; a.xsl = x.stride[2];
  a.w = w.data; a.wsc = w.stride[0]; a.wsk = w.stride[1]; a.wdt = w.dtype;
  a.bias = bias.data; a.bdt = bias.dtype;
  if (present(bias)) OMK_REQUIRE(numel(bias) == a.C && is_contig_last(bias), "%s: bias must be (C) contiguous", who);
  a.init = init.data; a.idt = init.dtype;
  if (present(init)) {
    OMK_REQUIRE(init.ndim == 3 && init.shape[0] == a.B && init.shape[1] == a.C && init.shape[2] == a.W - 1, "%s: initial_states must be (B, C, W-1)", who);
    a.isb = init.stride[0]; a.isc = init.stride[1]; a.isl = init.stride[2];
  }
  return OMK_OK;
}

// ---- who decides in the backward: conv_bwd_plan(), a pure function of the descriptor.  The launches read the plan only,
// omk_causal_conv1d_bwd_workspace_bytes asks the same function (tests/test_stream_dispatch.py holds the table call by call).
enum ConvFamily { CONV_GENERIC,   // strided scalar kernel: any layout
                  CONV_CL,        // channel-last 16-bit rows, per-thread tiles (conv1d_bwd_cl_kernel, round 3)
                  CONV_CL4 };     // channel-last 16-bit rows with scalar token positions (conv1d_bwd_cl4_kernel)
constexpr int CONV_BWD_TL = 64, CONV_BWD_NS = 4;                // strips of 64 tokens, four strips (waves) per workgroup
constexpr int CONV_BWD_TILE = CONV_BWD_NS * CONV_BWD_TL;        // = 256 tokens per workgroup and per partial dw / db row

// conv1d_bwd_cl4_kernel adds a row offset of 32 bits to a buffer resource: every offset of L rows of 16-bit elements must fit 31 bits
static bool conv_rows_near(int L, std::initializer_list<int64_t> row_strides) { return (int64_t)L * 2 * std::max(row_strides) < ((int64_t)1 << 31); }
// The short prologue (WF) of conv1d_bwd_cl4_kernel: fp32 (C, W) weight rows, contiguous and 16-byte aligned, and an fp32 bias (or none) aligned
// for the ONE request that fetches a lane's channels -- two channels per lane, one f32x2: 8 bytes.  (The forward's cl8 kernel has four channels
// per lane, one f32x4, and asks 16 in omk_causal_conv1d_fwd: the two masks differ on purpose.)
constexpr uintptr_t CONV_BWD_BIAS_ALIGN = 8;
static bool conv_bwd_wf(const OmkTensor& w, const OmkTensor& bias) {
  return w.dtype == OMK_F32 && w.stride[1] == 1 && w.stride[0] == w.shape[1] && ((uintptr_t)w.data & 15) == 0 &&
         (!present(bias) || (bias.dtype == OMK_F32 && ((uintptr_t)bias.data & (CONV_BWD_BIAS_ALIGN - 1)) == 0));
}
static dim3 conv_blocks(int64_t threads) { return dim3((unsigned)((threads + 255) / 256)); }
// f(integral constant W) for the run-time width 2 .. 4
template <class F> static void conv_width(int W, F&& f) {
  if (W == 4) f(std::integral_constant<int, 4>{}); else if (W == 3) f(std::integral_constant<int, 3>{}); else f(std::integral_constant<int, 2>{});
}

struct ConvBwdPlan {
  ConvFamily family; int dt, W;
  bool wf;             // CONV_CL4: the short prologue
  int tiles;           // 256-token tiles per batch element: workgroups along L, and the partial rows each batch element takes
  size_t part_bytes;   // one partial dw / db row per (batch, tile), C (W + 1) floats each: what the workspace query answers (0: atomics only)
  bool fold, dinit;    // conv1d_bwd_fold_kernel / conv1d_dinit_kernel follow
  dim3 grid, fold_grid, dinit_grid;
};
// (asked by the workspace query on a descriptor nothing has checked yet: reads shapes, strides and pointers only)
static ConvBwdPlan conv_bwd_plan(const OmkConv1dBwd* p) {
  ConvBwdPlan pl = {};
  const int B = (int)p->x.shape[0], C = (int)p->x.shape[1], L = (int)p->x.shape[2];
  pl.dt = p->x.dtype; pl.W = (int)p->weight.shape[1];
  pl.tiles = (L + CONV_BWD_TILE - 1) / CONV_BWD_TILE;
  pl.dinit = present(p->dinitial_states);
  pl.dinit_grid = conv_blocks((int64_t)B * C * (pl.W - 1));
  // (the 16-bit channel-last kernels only; every other layout keeps its atomics and needs no workspace)
  const bool fast = pl.dt != OMK_F32 && cl_fast_ok(p->x, C) && cl_fast_ok(p->dout, C) && cl_fast_ok(p->dx, C);
  if (!fast) {
    pl.family = CONV_GENERIC; pl.grid = conv_blocks((int64_t)B * C);
    return pl;
  }
  pl.part_bytes = (size_t)B * pl.tiles * (size_t)C * (pl.W + 1) * 4;
  // the scalar-position kernel (conv1d_bwd_cl4_kernel) when every row offset fits 31 bits; the round-3 kernel otherwise
  const bool cl4 = conv_rows_near(L, {p->x.stride[2], p->dout.stride[2], p->dx.stride[2]}) && p->x.stride[1] == 1 && p->dout.stride[1] == 1 && p->dx.stride[1] == 1;
  pl.family = cl4 ? CONV_CL4 : CONV_CL;
  pl.grid = dim3((unsigned)((int64_t)B * pl.tiles * ((C / 2 + 63) / 64)));
  if (cl4) {
    pl.wf = conv_bwd_wf(p->weight, p->bias);
    pl.fold = p->workspace && p->workspace_bytes >= pl.part_bytes;   // (none: fp32 atomics into dw / db)
    pl.fold_grid = dim3((unsigned)(((int64_t)C * (pl.W + 1) + 63) / 64));
  }
  return pl;
}

}  // namespace omk

using namespace omk;

extern "C" int omk_causal_conv1d_fwd(const OmkConv1dFwd* p, omk_stream stream) {
  OMK_REQUIRE(p && present(p->x) && present(p->weight) && present(p->out), "causal_conv1d_fwd: x, weight, out required");
  ConvArgs a = {};
  int rc = fill_common(a, p->x, p->weight, p->bias, p->initial_states, "causal_conv1d_fwd");
  if (rc) return rc;
  OMK_REQUIRE(p->out.ndim == 3 && p->out.shape[0] == a.B && p->out.shape[1] == a.C && p->out.shape[2] == a.L && p->out.dtype == p->x.dtype, "causal_conv1d_fwd: out mismatch");
  a.out = p->out.data; a.osb = p->out.stride[0]; a.osc = p->out.stride[1]; a.osl = p->out.stride[2];
  a.silu = p->silu;
  a.fin = p->final_states.data; a.fdt = p->final_states.dtype;
  if (present(p->final_states)) {
    OMK_REQUIRE(p->final_states.ndim == 3 && p->final_states.shape[0] == a.B && p->final_states.shape[1] == a.C && p->final_states.shape[2] >= a.W - 1 &&
                p->final_states.shape[2] <= 2 * a.W, "causal_conv1d_fwd: final_states must be (B, C, state_len) with W - 1 <= state_len <= 2 W");
    a.FW = (int)p->final_states.shape[2];
    a.fsb = p->final_states.stride[0]; a.fsc = p->final_states.stride[1]; a.fsl = p->final_states.stride[2];
  }
  if (present(p->seq_lens)) {
    OMK_REQUIRE(p->seq_lens.dtype == OMK_I32 && p->seq_lens.ndim == 1 && p->seq_lens.shape[0] == a.B && p->seq_lens.stride[0] == 1, "causal_conv1d_fwd: seq_lens must be dense int32 (B)");
    a.lens = (const int*)p->seq_lens.data;
  }
  if ((int64_t)a.B * a.C * a.L == 0) return OMK_OK;
  const bool fast = cl_fast_ok(p->x, a.C) && cl_fast_ok(p->out, a.C);   // (fp32 too: the prefill of the reference's fp32 inference ran the scalar kernel at 0.85 TB/s)
  // Per-row lengths: the final states come from conv1d_final_states_kernel (B * C * state_len threads, one launch of a few us) behind the
  // channel-last kernels too, whose epilogues are left out.  Reading lens[b] inside those epilogues cost the per-thread tile kernel two
  // VGPRs in every instantiation and its bf16 width-2 one a wave per SIMD (80 -> 82 VGPRs, occupancy 6 -> 5) for every caller, ragged or not.
  void* const fin_all = a.fin;
  if (a.lens) a.fin = nullptr;
  if (fast) {
    // 4 channels (8 bytes) per lane and 8 tokens per load group: 100 VGPRs / 4 waves per SIMD measured fastest on the
    // 1.3B shape (141 us vs 171 us for 8 channels per lane, which needs 158 VGPRs)
#define CONV_FWD_V(T_, VEC_, TL_, TG_) do { int64_t n = (int64_t)a.B * ((a.L + TL_ - 1) / TL_) * (a.C / VEC_); \
      dim3 grid((unsigned)((n + 255) / 256)), block(256); \
      if (a.W == 4) OMK_LAUNCH((conv1d_fwd_cl_kernel<T_, VEC_, TL_, 4, TG_>), grid, block, 0, stream, a); \
      else if (a.W == 3) OMK_LAUNCH((conv1d_fwd_cl_kernel<T_, VEC_, TL_, 3, TG_>), grid, block, 0, stream, a); \
      else OMK_LAUNCH((conv1d_fwd_cl_kernel<T_, VEC_, TL_, 2, TG_>), grid, block, 0, stream, a); } while (0)
    const int tl = a.L >= 1024 ? 64 : 32;   // 64: -4 % on the 1.3B slice (halo rows), 128: worse again
    const int64_t farf = (int64_t)a.L * 2 * (a.xsl > a.osl ? a.xsl : a.osl);
    if ((p->x.dtype == OMK_BF16 || p->x.dtype == OMK_F16) && a.L >= 256 && a.C % 4 == 0 && farf < ((int64_t)1 << 31) &&
        a.xsc == 1 && a.osc == 1) {
      // scalar token positions (conv1d_fwd_cl8_kernel); the per-thread tiles of rounds 1 - 4 below take the other layouts
      // strips of 16 tokens: the shorter a wave lives the better these streams run (tools/probe/conv_probe.hip: 128 / 64 / 32 / 16 tokens
      // per strip = 4.73 / 5.06 / 5.17 / 5.45 TB/s, three halo rows per strip included) -- once the prologue is a handful of 16-byte
      // requests (WF); the general prologue keeps 64
      const bool wf = p->weight.dtype == OMK_F32 && a.wsk == 1 && a.wsc == a.W && ((uintptr_t)p->weight.data & 15) == 0 &&
                      (!present(p->bias) || (p->bias.dtype == OMK_F32 && ((uintptr_t)p->bias.data & 15) == 0));
      const int tlf = wf ? 16 : 64;
      const int CVB = (a.C / 4 + 63) / 64, NT4 = (a.L + 4 * tlf - 1) / (4 * tlf);
      dim3 grid((unsigned)((int64_t)a.B * NT4 * CVB)), block(256);
#define CONV_FWD_8W(T_, TL_, WF_) do { if (a.W == 4) OMK_LAUNCH((conv1d_fwd_cl8_kernel<T_, TL_, 4, TGF, WF_>), grid, block, 0, stream, a); \
        else if (a.W == 3) OMK_LAUNCH((conv1d_fwd_cl8_kernel<T_, TL_, 3, TGF, WF_>), grid, block, 0, stream, a); \
        else OMK_LAUNCH((conv1d_fwd_cl8_kernel<T_, TL_, 2, TGF, WF_>), grid, block, 0, stream, a); } while (0)
#define CONV_FWD_8(T_) do { if (wf) CONV_FWD_8W(T_, 16, true); else CONV_FWD_8W(T_, 64, false); } while (0)
      if (p->x.dtype == OMK_BF16) CONV_FWD_8(bf16_t); else CONV_FWD_8(f16_t);
#undef CONV_FWD_8W
#undef CONV_FWD_8
    } else
    if (p->x.dtype == OMK_BF16) { if (tl == 64) CONV_FWD_V(bf16_t, 4, 64, 8); else CONV_FWD_V(bf16_t, 4, 32, 8); }
    else if (p->x.dtype == OMK_F32) { if (tl == 64) CONV_FWD_V(float, 4, 64, 8); else CONV_FWD_V(float, 4, 32, 8); }
    else CONV_FWD_V(f16_t, 4, 32, 8);
#undef CONV_FWD_V
  } else {
    int64_t n = (int64_t)a.B * a.C * a.L;
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    int lf = (a.xsl == 1 && a.xsc != 1) ? 1 : 0;
    OMK_DISPATCH_DTYPE(p->x.dtype, T, OMK_LAUNCH((conv1d_fwd_generic_kernel<T>), grid, block, 0, stream, a, lf));
  }
  a.fin = fin_all;
  if (a.fin && (!fast || a.lens)) {
    int64_t m = (int64_t)a.B * a.C * a.FW;
    dim3 g2((unsigned)((m + 255) / 256)), block(256);
    OMK_DISPATCH_DTYPE(p->x.dtype, T, OMK_LAUNCH((conv1d_final_states_kernel<T>), g2, block, 0, stream, a));
  }
  return finish_launch("causal_conv1d_fwd");
}

extern "C" size_t omk_causal_conv1d_bwd_workspace_bytes(const OmkConv1dBwd* p) {
  if (!p || !present(p->x) || !present(p->weight) || !present(p->dout) || !present(p->dx) || p->x.ndim != 3 || p->weight.ndim != 2) return 0;
  return conv_bwd_plan(p).part_bytes;
}

extern "C" int omk_causal_conv1d_bwd(const OmkConv1dBwd* p, omk_stream stream) {
  kernels_reset();
  OMK_REQUIRE(p && present(p->x) && present(p->weight) && present(p->dout) && present(p->dx) && present(p->dweight), "causal_conv1d_bwd: x, weight, dout, dx, dweight required");
  ConvArgs a = {};
  int rc = fill_common(a, p->x, p->weight, p->bias, p->initial_states, "causal_conv1d_bwd");
  if (rc) return rc;
  OMK_REQUIRE(p->dout.dtype == p->x.dtype && p->dx.dtype == p->x.dtype, "causal_conv1d_bwd: dout/dx dtype must equal x dtype");
  OMK_REQUIRE(p->dweight.dtype == OMK_F32 && p->dweight.stride[1] == 1 && p->dweight.stride[0] == a.W, "causal_conv1d_bwd: dweight must be contiguous f32 (C, W)");
  OMK_REQUIRE(!present(p->dbias) || p->dbias.dtype == OMK_F32, "causal_conv1d_bwd: dbias must be f32");
  a.dout = p->dout.data; a.dosb = p->dout.stride[0]; a.dosc = p->dout.stride[1]; a.dosl = p->dout.stride[2];
  a.dx = p->dx.data; a.dxsb = p->dx.stride[0]; a.dxsc = p->dx.stride[1]; a.dxsl = p->dx.stride[2];
  a.dw = (float*)p->dweight.data; a.db = (float*)p->dbias.data; a.silu = p->silu;
  a.dinit = p->dinitial_states.data;
  if (present(p->dinitial_states)) {
    OMK_REQUIRE(present(p->initial_states) && p->dinitial_states.dtype == p->initial_states.dtype, "causal_conv1d_bwd: dinitial_states needs initial_states of the same dtype");
    a.disb = p->dinitial_states.stride[0]; a.disc = p->dinitial_states.stride[1]; a.disl = p->dinitial_states.stride[2];
  }
  if ((int64_t)a.B * a.C * a.L == 0) return OMK_OK;
  const ConvBwdPlan pl = conv_bwd_plan(p);
  a.part = pl.fold ? (float*)p->workspace : nullptr;
  const char* t = dtype_name(pl.dt);
  const KernelId id = pl.family == CONV_CL4  ? kernel_id("conv1d_bwd_cl4<t=%s,w=%d,wf=%d>", t, pl.W, (int)pl.wf)
                      : pl.family == CONV_CL ? kernel_id("conv1d_bwd_cl<t=%s,w=%d>", t, pl.W)
                                             : kernel_id("conv1d_bwd_generic<t=%s>", t);
  auto go = [&](auto kern) { omk_launch(id, kern, pl.grid, dim3(256), 0, stream, a); };
  if (pl.family == CONV_GENERIC) OMK_DISPATCH_DTYPE(pl.dt, T, go(conv1d_bwd_generic_kernel<T>));
  else OMK_DISPATCH_DTYPE(pl.dt, T, conv_width(pl.W, [&](auto w) {
    constexpr int W = decltype(w)::value;
    if constexpr (sizeof(T) == 2) {
      // strips of 64 tokens, 8 tokens in flight: 402 -> 373 us per call on the 1.3B slice against 32 / 4 (halo re-reads of W - 1 rows
      // per strip and twice the loads in flight); 128-token strips gain nothing more
      if (pl.family == CONV_CL) return go(conv1d_bwd_cl_kernel<T, 2, CONV_BWD_TL, W, 8>);
      // (measured and not kept, profiles/r06_stream_kernels.txt: 8 / 16 strips per workgroup, 32- and 16-token strips, 8 / 16 tokens requested
      // per group -- 189 ... 194 us all, 16 waves per workgroup 220 ... 262)
      pl.wf ? go(conv1d_bwd_cl4_kernel<T, CONV_BWD_TL, W, TGX, CONV_BWD_NS, true>) : go(conv1d_bwd_cl4_kernel<T, CONV_BWD_TL, W, TGX, CONV_BWD_NS, false>);
    }
  }));
  if (pl.fold) omk_launch(kernel_id("conv1d_bwd_fold"), conv1d_bwd_fold_kernel, pl.fold_grid, dim3(1024), 0, stream, a.part, a.B * pl.tiles, a.C, a.W, a.dw, a.db);
  if (pl.dinit) OMK_DISPATCH_DTYPE(pl.dt, T, omk_launch(kernel_id("conv1d_dinit<t=%s>", t), conv1d_dinit_kernel<T>, pl.dinit_grid, dim3(256), 0, stream, a));
  return finish_launch("causal_conv1d_bwd");
}

extern "C" int omk_causal_conv1d_update(const OmkConv1dUpdate* p, omk_stream stream) {
  OMK_REQUIRE(p && present(p->x) && present(p->conv_state) && present(p->weight) && present(p->out), "causal_conv1d_update: x, conv_state, weight, out required");
  OMK_REQUIRE(p->x.ndim == 3 && p->conv_state.ndim == 3 && p->out.ndim == 3 && p->weight.ndim == 2, "causal_conv1d_update: x/out (B, C, T), conv_state (B, C, S), weight (C, W)");
  ConvUpdArgs a = {};
  a.B = (int)p->x.shape[0]; a.C = (int)p->x.shape[1]; a.T = (int)p->x.shape[2]; a.S = (int)p->conv_state.shape[2]; a.W = (int)p->weight.shape[1];
  OMK_REQUIRE(a.W >= 2 && a.W <= CONV_MAXW && a.S >= a.W - 1, "causal_conv1d_update: W in 2..4 and state_len >= W-1");
  // with slot indices conv_state is a pool of any number of rows
  const bool indexed = present(p->conv_state_indices);
  OMK_REQUIRE((indexed || p->conv_state.shape[0] == a.B) && p->conv_state.shape[1] == a.C && p->weight.shape[0] == a.C, "causal_conv1d_update: shape mismatch");
  OMK_REQUIRE(indices_ok(p->conv_state_indices, a.B), "causal_conv1d_update: conv_state_indices must be contiguous int32 (B)");
  a.csi = (const int*)p->conv_state_indices.data; a.pool = (int)p->conv_state.shape[0];
  OMK_REQUIRE(indices_ok(p->seq_lens, a.B), "causal_conv1d_update: seq_lens must be contiguous int32 (B)");
  a.lens = (const int*)p->seq_lens.data;
  OMK_REQUIRE(p->out.dtype == p->x.dtype, "causal_conv1d_update: out dtype");
  a.x = p->x.data; a.state = p->conv_state.data; a.w = p->weight.data; a.bias = p->bias.data; a.out = p->out.data;
  a.xsb = p->x.stride[0]; a.xsc = p->x.stride[1]; a.xsl = p->x.stride[2];
  a.ssb = p->conv_state.stride[0]; a.ssc = p->conv_state.stride[1]; a.ssl = p->conv_state.stride[2];
  a.osb = p->out.stride[0]; a.osc = p->out.stride[1]; a.osl = p->out.stride[2];
  a.wsc = p->weight.stride[0]; a.wsk = p->weight.stride[1];
  a.silu = p->silu; a.xdt = p->x.dtype; a.sdt = p->conv_state.dtype; a.wdt = p->weight.dtype; a.bdt = p->bias.dtype;
  if ((int64_t)a.B * a.C * a.T == 0) return OMK_OK;
  int64_t n = (int64_t)a.B * a.C;
  dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (a.lens) OMK_LAUNCH(conv1d_update_kernel<true>, grid, block, 0, stream, a);
  else OMK_LAUNCH(conv1d_update_kernel<false>, grid, block, 0, stream, a);
  return finish_launch("causal_conv1d_update");
}
