// sample_select.h -- what the sampler (sample.hip) and the log-probability kernel (token_logprobs.hip) both select with: the
// order-preserving integer key of a float, the LDS adds of the histograms, the wave ballot and scan, and the one-wave digit walk of a radix
// pass.  Everything here is inlined into its caller, and the kernels of both files compile to the instruction sequences they had with a copy
// each.  The radix select loop, the walk over the ties at the threshold and the bitonic sort are NOT here: as shared templates each of them
// changed the instruction sequence of the kernels of both files (profiles/sampler_one_body.txt section 2), so each file keeps its own.
#pragma once
#include "omk_common.h"

namespace omk {

// the most candidates a row hands to one wave (top_k of the sampler, top_n of the log-probabilities): one per lane
constexpr int SELECT_NMAX = 64;

// order-preserving key: larger float <-> larger unsigned (NaN sorts above +inf; -0 below +0), and back
__device__ __forceinline__ uint32_t fkey(float f) {
  const uint32_t u = __builtin_bit_cast(uint32_t, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_f32(uint32_t k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

#ifdef OMK_EMU
__device__ __forceinline__ uint32_t lds_fetch_add_u32(uint32_t* p, uint32_t v) { const uint32_t o = *p; *p = o + v; return o; }
__device__ __forceinline__ void lds_add_u64(unsigned long long* p, unsigned long long v) { *p += v; }
__device__ __forceinline__ unsigned long long ballot64(bool p) { return emu::ballot(p ? 1 : 0); }
#else
__device__ __forceinline__ uint32_t lds_fetch_add_u32(uint32_t* p, uint32_t v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_add_u64(unsigned long long* p, unsigned long long v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }
#endif

// inclusive scan over the lanes of a wave (any additive type the shuffles move)
template <class T> __device__ __forceinline__ T wave_incl_scan_t(T v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const T o = shfl(v, lane >= off ? lane - off : lane); if (lane >= off) v += o; }
  return v;
}
// The digit walk of a radix pass by ONE WAVE instead of one thread (a thread reading 60 - 190 counters one after the other was 2 - 8 us per pass):
// cnt(r) for r = 0 .. 255 in WALK order, lane l holds r = 4 l .. 4 l + 3; returns in every lane the first r whose running total reaches `need`
// by the rule `total before + cnt(r) > limit` (limit = need - 1 for "covers need keys"), and the total BEFORE it; r = 255 when none does.
template <class T, class F> __device__ __forceinline__ void wave_find_digit(F cnt, T limit, int lane, uint32_t& r_out, T& before_out) {
  T c[4], s = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) { c[j] = cnt(4 * lane + j); s += c[j]; }
  const T incl = wave_incl_scan_t<T>(s, lane);
  T run = incl - s;
  int jj = -1; T bef = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) { if (jj < 0 && run + c[j] > limit) { jj = j; bef = run; } run += c[j]; }
  const unsigned long long m = ballot64(jj >= 0);
  if (m) {
    const int l0 = __builtin_ctzll(m);
    r_out = (uint32_t)(4 * l0 + shfl(jj, l0));
    before_out = shfl(bef, l0);
  } else {   // (the walk ends on the last digit: everything in front of it is "before")
    r_out = 255u;
    before_out = shfl(incl, 63) - shfl(c[3], 63);
  }
}

}  // namespace omk
